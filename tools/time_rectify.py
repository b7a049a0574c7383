"""dcmt_rectify_dev against what bounds it, on one device-resident workload: 1024 frames of 375x1242 undistorted and rectified to
352x1216 through a map of KITTI's magnitude (D_02, R_rect_02, unit magnification), grey and BGR.

Timed, per channel count:
    the default route (a tile's source box staged in LDS, the map read once per group of frames);
    the forced gather route (DCMT_RECTIFY_FORCE_GATHER);
    n_maps = batch: a map per frame, so the 8 B/px of the map are read for every frame -- no amortisation;
    (a) a plain device-to-device copy of the bytes the call must move, 1 read + 1 written per channel and pixel;
    the dcmt_bgr_convert_dev call that follows it in the pipeline (BGR -> grey; BGR only).

One process, the candidates of a group alternating: REPS rounds, in every round each timed over `reps` back-to-back calls between
two events.  Per candidate the median and the range over the rounds, and the rate its bytes make of the median."""
import os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from depth_completion_mt_amd import Context, api

B, SR, SC, R, C = 1024, 375, 1242, 352, 1216
REPS = 9
K = np.array([[7.215377e+02, 0.0, 6.21e+02], [0.0, 7.215377e+02, 1.875e+02], [0.0, 0.0, 1.0]])
D = np.array([-3.691481e-01, 1.968681e-01, 1.353473e-03, 5.677587e-04, -6.770705e-02])
RR = np.array([[9.998817e-01, 1.511453e-02, -2.841595e-03], [-1.511724e-02, 9.998853e-01, -9.338510e-04],
               [2.827154e-03, 9.766976e-04, 9.999955e-01]])
P = np.array([[7.215377e+02, 0.0, 6.08e+02], [0.0, 7.215377e+02, 1.76e+02], [0.0, 0.0, 1.0]])


def timed(fn, reps):
    for _ in range(2): fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(); a.record()
    for _ in range(reps): fn()
    b.record(); torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def group(title, candidates):
    """candidates: [(name, fn, bytes moved, reps)]"""
    ms = {name: [] for name, *_ in candidates}
    for _ in range(REPS):
        for name, fn, _, reps in candidates:
            ms[name].append(timed(fn, reps))
    print(title)
    for name, _, moved, _ in candidates:
        v = ms[name]
        m = statistics.median(v)
        print(f"    {name}: {m:.4f} ms [{min(v):.4f} .. {max(v):.4f}], {moved / m / 1e9:.2f} TB/s of {moved / 1e6:.0f} MB")
    return {name: (statistics.median(v), min(v), max(v)) for name, v in ms.items()}


def main():
    assert torch.cuda.is_available(), "no GPU: nothing is measured without one"
    with Context(0, R, C, B) as ctx:
        d_table = api.make_rectify_calib(K, D, RR, P)
        d_map = ctx.rectify_map_dev(d_table, R, C)
        d_maps = d_map.expand(B, R, C, 2).contiguous()                  # n_maps = batch: the same map, B copies of it
        for ch, name in ((1, "grey"), (3, "BGR")):
            shape = (B, SR, SC) + ((3,) if ch == 3 else ())
            d_src = torch.randint(0, 256, shape, dtype=torch.uint8, device="cuda")
            d_dst = torch.empty((B, R, C) + shape[3:], dtype=torch.uint8, device="cuda")
            d_ref = torch.empty_like(d_dst)
            moved = 2 * B * R * C * ch
            d_flat = torch.empty((moved // 2,), dtype=torch.uint8, device="cuda")
            ctx.rectify_dev(d_src, d_map, out=d_dst); torch.cuda.synchronize()
            path = ctx.last_path()
            ctx.rectify_dev(d_src, d_map, out=d_ref, force_gather=True); torch.cuda.synchronize()
            assert torch.equal(d_dst, d_ref), f"{name}: the two routes differ"
            ctx.rectify_dev(d_src, d_maps, out=d_ref); torch.cuda.synchronize()
            assert torch.equal(d_dst, d_ref), f"{name}: a map per frame differs"
            cands = [(f"default route ({path})", lambda: ctx.rectify_dev(d_src, d_map, out=d_dst), moved, 5),
                     ("forced gather route", lambda: ctx.rectify_dev(d_src, d_map, out=d_dst, force_gather=True), moved, 5),
                     ("n_maps = batch, default route", lambda: ctx.rectify_dev(d_src, d_maps, out=d_dst), moved + 8 * B * R * C, 5),
                     (f"(a) plain copy of {ch} B/px read + {ch} written", lambda: d_flat.copy_(d_dst.view(-1)), moved, 10)]
            if ch == 3:
                d_gray = torch.empty((B, R, C), dtype=torch.uint8, device="cuda")
                cands.append(("the dcmt_bgr_convert_dev (grey) that follows", lambda: ctx.bgr_convert_dev(d_dst, lab=False, d_gray=d_gray), 4 * B * R * C, 5))
            med = group(f"rectify, {B} frames of {SR}x{SC} -> {R}x{C}, {name}", cands)
            vals = list(med.values())
            (lds, _, _), (gat, gmin, gmax) = vals[0], vals[1]
            print(f"    default / plain copy {lds / vals[3][0]:.2f}; gather - default {gat - lds:.4f} ms against the gather route's own range {gmax - gmin:.4f} ms")
            del d_src, d_dst, d_ref, d_flat


if __name__ == "__main__":
    main()
