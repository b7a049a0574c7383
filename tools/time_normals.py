"""Normals and the flying-pixel filter on the device (1024 frames of 352x1216): depth_normals_dev on a completed synth.synth_batch --
the records alone, the filter alone out of place and in place, both -- against plain device copies of each variant's stated bytes
(20, 8, 8 and 24 per pixel), against gaussian5_dev and depth_to_cloud_dev on the same planes, and the table twin against the uniform
call, in one alternating session.  Medians of REPS alternating repetitions in one process, with the range.  The in-place variant
filters the same buffer again and again: after its first call nothing is left to remove, so it times the decisions and the mask, not
the zeroing of a fresh plane (a few pixels in a thousand).
    python3 tools/time_normals.py [--frames B]"""
import os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np, torch  # noqa: E402
from depth_completion_mt_amd import Context, calib_to_device, make_cloud_params, make_normals_calib, make_params, synth  # noqa: E402
B = int(sys.argv[sys.argv.index("--frames") + 1]) if "--frames" in sys.argv else 1024
R, C = 352, 1216
REPS, INNER = 7, 3
KITTI = dict(fx=721.5, fy=721.5, cx=608.0, cy=176.0)


def timed(fn):
    for _ in range(1): fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(); a.record()
    for _ in range(INNER): fn()
    b.record(); torch.cuda.synchronize()
    return a.elapsed_time(b) / INNER


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
    print(f"{name}: {med:.4f} ms [{lo:.4f} .. {hi:.4f}] = {med / B * 1e3:.2f} us per frame{tail}")


def copier(nbytes):
    """A device copy that moves nbytes in all: half of them read, half written."""
    src = torch.empty((int(nbytes) // 2,), dtype=torch.uint8, device="cuda").fill_(3)
    dst = torch.empty_like(src)
    return lambda: dst.copy_(src)


with Context(0, R, C, B) as ctx:
    rep = B // 32 if B >= 32 else 1
    n0 = min(B, 32)
    sparse = torch.from_numpy(synth.synth_batch(n0, R, C, 0)).cuda().repeat(rep, 1, 1).contiguous()
    dense = ctx.complete_dev(sparse, None, make_params())
    del sparse
    cp = make_cloud_params(**KITTI)
    table = calib_to_device(make_normals_calib(np.full(B, KITTI["fx"]), KITTI["fy"], KITTI["cx"], KITTI["cy"]))
    px = B * R * C
    normals = torch.empty((B, R, C, 4), dtype=torch.float32, device="cuda")
    out, inplace = torch.empty_like(dense), dense.clone()
    points = torch.empty((px, 4), dtype=torch.float32, device="cuda")
    offsets = torch.empty((B + 1,), dtype=torch.int32, device="cuda")
    _, cnt = ctx.depth_normals_dev(dense, cp, normals=False, d_out=out, counts=True)
    torch.cuda.synchronize()
    print(f"--- {B} frames of {R} x {C}: the default removes {float(cnt[:n0, 0].double().mean()) / (R * C):.5f} of the pixels, "
          f"{float(cnt[:n0, 1].double().mean()) / (R * C):.5f} have no normal")
    cases = {
        "normals": lambda: ctx.depth_normals_dev(dense, cp, d_normals=normals),
        "filter": lambda: ctx.depth_normals_dev(dense, cp, normals=False, d_out=out),
        "in place": lambda: ctx.depth_normals_dev(inplace, cp, normals=False, d_out=inplace),
        "both": lambda: ctx.depth_normals_dev(dense, cp, d_normals=normals, d_out=out),
        "both + counts": lambda: ctx.depth_normals_dev(dense, cp, d_normals=normals, d_out=out, d_counts=cnt),
        "twin both": lambda: ctx.depth_normals_calib_dev(dense, table, d_normals=normals, d_out=out),
        "twin normals": lambda: ctx.depth_normals_calib_dev(dense, table, d_normals=normals),
        "gaussian5": lambda: ctx.gaussian5_dev(dense, out),
        "cloud": lambda: ctx.depth_to_cloud_dev(dense, None, cp, d_points=points, d_offsets=offsets),
        "copy8": copier(8 * px), "copy20": copier(20 * px), "copy24": copier(24 * px),
    }
    t = alternating(cases)
    stated = {"normals": 20, "filter": 8, "in place": 8, "both": 24, "both + counts": 24, "twin both": 24, "twin normals": 20}
    for key, bpp in stated.items():
        line(f"depth_normals{'_calib' if 'twin' in key else ''}_dev {key}", t[key], bpp * px)
    line("gaussian5_dev", t["gaussian5"], 8 * px)
    line("depth_to_cloud_dev (every pixel a point)", t["cloud"], 24 * px)
    for b in (8, 20, 24):
        line(f"device copy ({b} B/px)", t[f"copy{b}"], b * px)
    for key, bpp in stated.items():
        print(f"{key}: / its copy = {t[key][0] / t[f'copy{bpp}'][0]:.2f}, / gaussian5_dev = {t[key][0] / t['gaussian5'][0]:.2f}, "
              f"/ depth_to_cloud_dev = {t[key][0] / t['cloud'][0]:.2f}")
    print(f"table twin / uniform call: both {t['twin both'][0] / t['both'][0]:.3f}, normals {t['twin normals'][0] / t['normals'][0]:.3f}")
