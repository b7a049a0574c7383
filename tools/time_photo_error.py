"""get_initial_error on the device (352x1216, 1024 frames): photo_error_dev with both outputs, the map only and the statistics only, and its
_calib twin, against a plain device copy of the 7 B/px the call moves (depth 4, two images 1 + 1, the map 1) and stereo_refine_dev
with 0 iterations, the nearest existing kernel with the same access pattern (10 B/px).  Medians of REPS alternating repetitions in one
process, with the range.  --profile: only a few calls with both outputs, for a counters-only run, e.g.
    rocprofv3 --pmc SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_WAIT_INST_ANY SQ_ACTIVE_INST_VALU SQ_ACTIVE_INST_LDS SQ_WAIT_INST_LDS SQ_LDS_BANK_CONFLICT SQ_INSTS_VALU \\
        --output-format csv -d OUT -o q -- python3 tools/time_photo_error.py --profile        (then tools/pmc_summary.py)"""
import os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from depth_completion_mt_amd import Context, calib_to_device, make_params, make_stereo_calib, synth
B, R, C = 1024, 352, 1216
REPS = 7
PROFILE = "--profile" in sys.argv[1:]
frames = synth.synth_batch(32, R, C, 0)
src = torch.from_numpy(frames).cuda().repeat(B // 32, 1, 1).contiguous()
g = torch.Generator(device="cuda").manual_seed(1)
left = torch.randint(0, 256, (B, R, C), dtype=torch.uint8, device="cuda", generator=g)
right = torch.randint(0, 256, (B, R, C), dtype=torch.uint8, device="cuda", generator=g)


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


def line(name, t, bytes_moved):
    med, lo, hi = t
    rate = bytes_moved / (med * 1e-3)
    print(f"{name}: {med:.4f} ms [{lo:.4f} .. {hi:.4f}], {bytes_moved / 1e9:.3f} GB stated -> {rate / 1e12:.2f} TB/s = {rate / 8e12:.3f} of 8 TB/s")


with Context(0, R, C, B) as ctx:
    dense = ctx.complete_dev(src, params=make_params())                    # a dense plane, as the call meets it
    err = torch.empty((B, R, C), dtype=torch.uint8, device="cuda")
    stats = torch.empty((B, 4), dtype=torch.int64, device="cuda")
    if PROFILE:
        for _ in range(3):
            ctx.photo_error_dev(dense, left, right, d_err=err, d_stats=stats)
        torch.cuda.synchronize()
        sys.exit(0)
    refined = torch.empty_like(dense)
    table = calib_to_device(make_stereo_calib(np.full(B, 0.54, np.float32), 9.597910e+02))
    moved = torch.empty(7 * B * R * C, dtype=torch.uint8, device="cuda")   # the copy's two ends: 3.5 B/px read, 3.5 B/px written
    half = moved.numel() // 2
    px = B * R * C
    t = alternating({
        "both": lambda: ctx.photo_error_dev(dense, left, right, d_err=err, d_stats=stats),
        "map": lambda: ctx.photo_error_dev(dense, left, right, d_err=err, stats=False),
        "stats": lambda: ctx.photo_error_dev(dense, left, right, err=False, d_stats=stats),
        "calib": lambda: ctx.photo_error_calib_dev(dense, left, right, table, d_err=err, d_stats=stats),
        "copy": lambda: moved[half:2 * half].copy_(moved[:half]),
        "stereo0": lambda: ctx.stereo_refine_dev(dense, left, right, d_out=refined, iterations=0),
    })
    s = stats.cpu().numpy()
    print(f"--- {B} frames of {R} x {C}; per frame: {s[0, 0]} valid pixels of {R * C}, {s[0, 1]} matches, mean error {s[0, 3] / max(1, s[0, 0]):.1f}")
    line("photo_error_dev, map + stats (7 B/px)", t["both"], 7 * px)
    line("photo_error_dev, map only (7 B/px)", t["map"], 7 * px)
    line("photo_error_dev, stats only (6 B/px)", t["stats"], 6 * px)
    line("photo_error_calib_dev, map + stats (7 B/px)", t["calib"], 7 * px)
    line("device copy of 7 B/px (3.5 read, 3.5 written)", t["copy"], 7 * px)
    line("stereo_refine_dev, 0 iterations (10 B/px)", t["stereo0"], 10 * px)
    print(f"photo_error_dev / copy = {t['both'][0] / t['copy'][0]:.2f}, / stereo_refine_dev(0) = {t['both'][0] / t['stereo0'][0]:.2f}; "
          f"{B / t['both'][0] * 1e3:.0f} frames/s")
