"""The cascade without its extrapolation (make_params(extrapolate=False): k_local, one kernel) against the default path and a plain
device copy of the flagged call's bytes, at 1, 8, 128 and 1024 frames of 352x1216 (synthetic frames at KITTI density): complete_dev
(8 B/px: 4 read, 4 written) and complete_u16_dev (6 B/px).  Beside them the flagged call on the staged
kernels (FORCE_STAGED: two launches through X5), the form k_local replaces.  One alternating session on one box: medians of REPS repetitions
with the range, every case once per round in turn.
    python tools/time_no_extrapolate.py [--bands N] [--batches 1,8]      (--bands: DCMT_LOCAL_BANDS for the whole session)"""
import os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if "--bands" in sys.argv:
    os.environ["DCMT_LOCAL_BANDS"] = sys.argv[sys.argv.index("--bands") + 1]
import torch
from depth_completion_mt_amd import Context, make_params, synth
R, C = 352, 1216
BATCHES = tuple(int(v) for v in sys.argv[sys.argv.index("--batches") + 1].split(",")) if "--batches" in sys.argv else (1, 8, 128, 1024)
REPS = 7
frames = synth.synth_batch(32, R, C, 0)
frames = (torch.round(torch.from_numpy(frames) * 256.0) / 256.0)          # KITTI's payload: multiples of 1/256 m


def timed(fn, reps):
    for _ in range(3): fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(); a.record()
    for _ in range(reps): fn()
    b.record(); torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def alternating(cases, reps):
    """cases: {name: fn}; REPS rounds, every case once per round in turn.  Returns {name: (median, min, max)} in ms."""
    ms = {k: [] for k in cases}
    for _ in range(REPS):
        for k, fn in cases.items():
            ms[k].append(timed(fn, reps))
    return {k: (statistics.median(v), min(v), max(v)) for k, v in ms.items()}


def line(name, t, bytes_moved=None):
    med, lo, hi = t
    tail = ""
    if bytes_moved:
        rate = bytes_moved / (med * 1e-3)
        tail = f", {bytes_moved / 1e9:.4f} GB stated -> {rate / 1e12:.3f} TB/s = {rate / 8e12:.3f} of 8 TB/s"
    print(f"{name}: {med:.4f} ms [{lo:.4f} .. {hi:.4f}]{tail}")


with Context(0, R, C, max(BATCHES)) as ctx:
    flag, default = make_params(extrapolate=False), make_params()
    two = make_params(extrapolate=False, force_staged=True)       # two launches through X5: k_pre_v1, then k_post_v1
    for B in BATCHES:
        src = frames.cuda().repeat((B + 31) // 32, 1, 1)[:B].contiguous()
        src16 = torch.round(src * 256.0).to(torch.int32).to(torch.int16)
        dst = torch.empty_like(src)
        px = B * R * C
        reps = 10 if B >= 128 else 50
        print(f"--- {B} frame(s) of {R} x {C}")
        for name, bpp, call, cin in (("complete_dev", 8, lambda p: ctx.complete_dev(src, dst, p), src),
                                     ("complete_u16_dev", 6, lambda p: ctx.complete_u16_dev(src16, 1.0 / 256.0, dst, p), src16)):
            # the copy of the flagged call's bytes: its input read once, its output written once (uint16: torch's converting copy)
            copy = lambda cin=cin: dst.copy_(cin)
            t = alternating({"flag": lambda: call(flag), "default": lambda: call(default), "copy": copy, "two": lambda: call(two)}, reps)
            call(flag); pf = ctx.last_path()
            call(default); pd = ctx.last_path()
            line(f"{name}, extrapolate=False ({pf})", t["flag"], bpp * px)
            line(f"{name}, default ({pd})", t["default"])
            line(f"device copy of {bpp} B/px", t["copy"], bpp * px)
            line(f"{name}, extrapolate=False with FORCE_STAGED (two launches through X5)", t["two"])
            print(f"{name}: extrapolate=False / default = {t['flag'][0] / t['default'][0]:.3f}, / copy = {t['flag'][0] / t['copy'][0]:.2f}; "
                  f"{B / t['default'][0] * 1e3:.0f} -> {B / t['flag'][0] * 1e3:.0f} frames/s; the default call's own range is "
                  f"{t['default'][2] - t['default'][1]:.4f} ms")
