"""The Gaussian that ignores holes (blur_type="gaussian_valid", gaussian5_dev(valid_thresh=...)) against what it replaces, on synthetic
frames at KITTI density, 352x1216.  One alternating session on one box: medians of REPS repetitions with the range, every case once per
round in turn.
  1. complete_dev(extrapolate=False) with "gaussian_valid" against "gaussian" and "none" (k_local, one kernel each) at 1, 8, 128 and 1024
     frames, and against the plan the fused kind replaces: k_local to MEDIAN5 plus the stand-alone kernel;
  2. complete_u16_dev at the largest batch;
  3. gaussian5_dev(valid_thresh=0.1) against gaussian5_dev and a device copy of its 8 B/px, on a completed plane with its holes;
  4. the extrapolating cascade's extra kernel against "bilateral_clone"'s: both calls share the chain to MEDIAN5.
    python tools/time_gauss_valid.py [--batches 1,8]"""
import os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from depth_completion_mt_amd import Context, make_params, synth
from depth_completion_mt_amd import _lib as L
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
    ne = dict(extrapolate=False)
    valid, gauss, none = make_params(blur_type="gaussian_valid", **ne), make_params(**ne), make_params(blur_type="none", **ne)
    median = make_params(blur_type="none", stop_after=L.STAGE_MEDIAN5, **ne)
    for B in BATCHES:
        src = frames.cuda().repeat((B + 31) // 32, 1, 1)[:B].contiguous()
        src16 = torch.round(src * 256.0).to(torch.int32).to(torch.int16)
        dst, mid = torch.empty_like(src), torch.empty_like(src)
        px = B * R * C
        reps = 10 if B >= 128 else 50
        print(f"--- {B} frame(s) of {R} x {C}")

        def two_step():                      # the plan the fused kind replaces; its second kernel without the final invert
            ctx.complete_dev(src, mid, median)
            ctx.gaussian5_dev(mid, dst, valid_thresh=0.1)

        t = alternating({"valid": lambda: ctx.complete_dev(src, dst, valid), "gauss": lambda: ctx.complete_dev(src, dst, gauss),
                         "none": lambda: ctx.complete_dev(src, dst, none), "two": two_step, "copy": lambda: dst.copy_(src)}, reps)
        ctx.complete_dev(src, dst, valid)
        line(f"complete_dev, gaussian_valid ({ctx.last_path()})", t["valid"], 8 * px)
        ctx.complete_dev(src, dst, gauss)
        line(f"complete_dev, gaussian ({ctx.last_path()})", t["gauss"], 8 * px)
        line("complete_dev, none", t["none"], 8 * px)
        line("k_local to MEDIAN5 + gaussian5_dev(valid_thresh) (two launches, 16 B/px)", t["two"])
        line("device copy of 8 B/px", t["copy"], 8 * px)
        print(f"gaussian_valid / gaussian = {t['valid'][0] / t['gauss'][0]:.3f}, / none = {t['valid'][0] / t['none'][0]:.3f}, / two launches = "
              f"{t['valid'][0] / t['two'][0]:.3f}, / copy = {t['valid'][0] / t['copy'][0]:.2f}; the Gaussian's own range is {t['gauss'][2] - t['gauss'][1]:.4f} ms")
        if B == max(BATCHES):
            call = lambda p: ctx.complete_u16_dev(src16, 1.0 / 256.0, dst, p)
            t = alternating({"valid": lambda: call(valid), "gauss": lambda: call(gauss), "none": lambda: call(none)}, reps)
            for k in ("valid", "gauss", "none"):
                line(f"complete_u16_dev, {k}", t[k], 6 * px)
            print(f"complete_u16_dev: gaussian_valid / gaussian = {t['valid'][0] / t['gauss'][0]:.3f}")
        # the stand-alone call on the completed plane (its holes are the frame's upper third and the region's ragged border)
        ctx.complete_dev(src, mid, none)
        t = alternating({"valid": lambda: ctx.gaussian5_dev(mid, dst, valid_thresh=0.1), "plain": lambda: ctx.gaussian5_dev(mid, dst),
                         "copy": lambda: dst.copy_(mid)}, reps)
        line("gaussian5_dev(valid_thresh=0.1)", t["valid"], 8 * px)
        line("gaussian5_dev", t["plain"], 8 * px)
        line("device copy of 8 B/px", t["copy"], 8 * px)
        print(f"gaussian5_dev: valid / plain = {t['valid'][0] / t['plain'][0]:.3f}, valid / copy = {t['valid'][0] / t['copy'][0]:.2f}")
        # with the extrapolation: the chain to MEDIAN5 is the same in both calls, the difference is the last kernel's
        ex_valid, ex_clone = make_params(blur_type="gaussian_valid"), make_params(blur_type="bilateral_clone")
        ex_median = make_params(blur_type="none", stop_after=L.STAGE_MEDIAN5)
        t = alternating({"valid": lambda: ctx.complete_dev(src, dst, ex_valid), "clone": lambda: ctx.complete_dev(src, dst, ex_clone),
                         "median": lambda: ctx.complete_dev(src, dst, ex_median), "default": lambda: ctx.complete_dev(src, dst)}, reps)
        ctx.complete_dev(src, dst, ex_valid)
        line(f"complete_dev with the extrapolation, gaussian_valid ({ctx.last_path()})", t["valid"])
        line("complete_dev with the extrapolation, bilateral_clone", t["clone"])
        line("complete_dev with the extrapolation, stop_after = MEDIAN5", t["median"])
        line("complete_dev, default", t["default"])
        print(f"the extra kernel: gauss5_valid {t['valid'][0] - t['median'][0]:.4f} ms, bilateral5 {t['clone'][0] - t['median'][0]:.4f} ms")
