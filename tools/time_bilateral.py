"""The bilateral finish on the device (352x1216, 1024 frames): dcmt_bilateral5_dev against dcmt_gaussian5_dev and a plain device copy
of the same bytes (8 B/px each: a read and a write), then complete_dev / complete_u16_dev with blur_type="bilateral_clone" against
the same calls with "gaussian" -- the cost of leaving the fused H7..H11 kernel for the unfused route plus one pass -- and with
"gaussian" at stop_after = MEDIAN5 (the unfused route alone).  Medians of REPS alternating repetitions in one process, with the range."""
import os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from depth_completion_mt_amd import Context, make_params, synth
from depth_completion_mt_amd import _lib as L
B, R, C = 1024, 352, 1216
REPS = 7
frames = synth.synth_batch(32, R, C, 0)
src = torch.from_numpy(frames).cuda().repeat(B // 32, 1, 1).contiguous()
src16 = torch.round(src * 256.0).to(torch.int32).to(torch.int16)           # KITTI's payload: multiples of 1/256 m (below 128 m)


def timed(fn, reps=10):
    for _ in range(3): fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(); a.record()
    for _ in range(reps): fn()
    b.record(); torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def alternating(cases):
    """cases: {name: fn}; REPS rounds, every case once per round in turn.  Returns {name: (median, min, max)} in ms."""
    ms = {k: [] for k in cases}
    for _ in range(REPS):
        for k, fn in cases.items():
            ms[k].append(timed(fn))
    return {k: (statistics.median(v), min(v), max(v)) for k, v in ms.items()}


def line(name, t, bytes_moved=None):
    med, lo, hi = t
    tail = ""
    if bytes_moved:
        rate = bytes_moved / (med * 1e-3)
        tail = f", {bytes_moved / 1e9:.3f} GB stated -> {rate / 1e12:.2f} TB/s = {rate / 8e12:.3f} of 8 TB/s"
    print(f"{name}: {med:.4f} ms [{lo:.4f} .. {hi:.4f}]{tail}")


with Context(0, R, C, B) as ctx:
    dense = ctx.complete_dev(src, params=make_params())
    out = torch.empty_like(dense)
    px = B * R * C
    t = alternating({
        "bilateral5": lambda: ctx.bilateral5_dev(dense, d_dst=out),
        "gaussian5": lambda: ctx.gaussian5_dev(dense, d_dst=out),
        "copy": lambda: out.copy_(dense),
    })
    print(f"--- {B} frames of {R} x {C}")
    line("bilateral5_dev, out of place (8 B/px)", t["bilateral5"], 8 * px)
    line("gaussian5_dev, out of place (8 B/px)", t["gaussian5"], 8 * px)
    line("device copy (8 B/px)", t["copy"], 8 * px)
    print(f"bilateral5_dev / gaussian5_dev = {t['bilateral5'][0] / t['gaussian5'][0]:.2f}, / copy = {t['bilateral5'][0] / t['copy'][0]:.2f}")

    dst = torch.empty_like(src)
    g, b, m = make_params(), make_params(blur_type="bilateral_clone"), make_params(stop_after=L.STAGE_MEDIAN5)
    for name, call in (("complete_dev", lambda p: ctx.complete_dev(src, dst, p)),
                       ("complete_u16_dev", lambda p: ctx.complete_u16_dev(src16, 1.0 / 256.0, dst, p))):
        t = alternating({"gaussian": lambda: call(g), "bilateral_clone": lambda: call(b), "median5": lambda: call(m)})
        call(g); pg = ctx.last_path()
        call(b); pb = ctx.last_path()
        line(f'{name}, "gaussian" ({pg})', t["gaussian"])
        line(f'{name}, "bilateral_clone" ({pb})', t["bilateral_clone"])
        line(f'{name}, "gaussian" up to MEDIAN5 (the unfused route alone)', t["median5"])
        print(f'{name}: "bilateral_clone" costs {t["bilateral_clone"][0] - t["gaussian"][0]:+.3f} ms per {B} frames over "gaussian" '
              f'({B / t["gaussian"][0] * 1e3:.0f} -> {B / t["bilateral_clone"][0] * 1e3:.0f} frames/s); the Gaussian call\'s own range is '
              f'{t["gaussian"][2] - t["gaussian"][1]:.3f} ms')
