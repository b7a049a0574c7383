"""The nearest-wins scatter calls against their last-wins twins (dcmt_*_nearest*_dev against dcmt_*_dev, `nearest=True` against the
default) on the same device-resident batch: 256 sweeps of 120 000 points into 352x1216 planes for the projection, 1024 dense frames
of 352x1216 for the reprojection -- under the near-identity warp of unrectify_sol (KITTI's R_rect_02, inverted) and under a real
change of viewpoint (the stereo baseline, 0.54 m along x).  The two rules do different work: last-wins scatters tags into the winner
plane and gathers and recomputes each winner; nearest-wins clears the output (4 B per pixel more), scatters keys into it and fixes it
up in place.  First the pair is compared on the device: the same occupancy, nearest <= last everywhere, and the share of occupied
pixels where the rules differ is printed.

One process, the calls of a pair alternating: REPS rounds, in every round each call timed over `reps` back-to-back calls between
two events.  Per call the median and the range over the rounds; per pair the difference of the medians against the last-wins call's
own range, which is the yardstick: a difference inside it is not a difference.  There is no threshold."""
import os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from depth_completion_mt_amd import Context, api, make_params, synth

B, R, C = 1024, 352, 1216
SWEEPS, PER_SWEEP = 256, 120000
REPS = 9


def timed(fn, reps=10):
    for _ in range(3): fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(); a.record()
    for _ in range(reps): fn()
    b.record(); torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def pair(name, call, out):
    """call(nearest, k) writes to out[k].  Last-wins into out[0] and nearest into out[1] are compared, then both are timed on out[0]
    in alternating rounds."""
    call(False, 0); call(True, 1); torch.cuda.synchronize()
    last, near = out
    occupied = last != 0
    assert torch.equal(occupied, near != 0), f"{name}: the occupancy differs between the two rules"
    assert bool((near <= last).all()), f"{name}: a nearest value above the last-wins value"
    occ, diff = int(occupied.sum().item()), int((near != last).sum().item())
    del occupied
    ms = {False: [], True: []}
    for _ in range(REPS):
        for nearest in (False, True):
            ms[nearest].append(timed(lambda: call(nearest, 0)))
    l, n = ms[False], ms[True]
    ml, mn = statistics.median(l), statistics.median(n)
    spread = max(l) - min(l)
    verdict = "inside" if abs(mn - ml) <= spread else "OUTSIDE"
    print(f"{name}: {occ} occupied pixels ({100.0 * occ / last.numel():.2f} %), the rules differ in {diff} ({100.0 * diff / max(occ, 1):.2f} % of them); "
          f"last-wins {ml:.4f} ms [{min(l):.4f} .. {max(l):.4f}], nearest {mn:.4f} ms [{min(n):.4f} .. {max(n):.4f}], "
          f"nearest - last {mn - ml:+.4f} ms ({(mn / ml - 1) * 100:+.2f} %), {verdict} the last-wins call's range of {spread:.4f} ms")


def main():
    assert torch.cuda.is_available(), "no GPU: nothing is measured without one"
    # ---- projection
    sweep = synth.synth_points(PER_SWEEP, 3)
    points = torch.from_numpy(sweep).cuda().repeat(SWEEPS, 1).contiguous()
    offsets = torch.arange(0, (SWEEPS + 1) * PER_SWEEP, PER_SWEEP, dtype=torch.int32, device="cuda")
    T, P = synth.KITTI_T_VELO_TO_CAM, synth.KITTI_P2
    pt = api.calib_to_device(api.make_project_calib(np.repeat(T[None], SWEEPS, 0), np.repeat(P[None], SWEEPS, 0)))
    with Context(0, R, C, SWEEPS) as ctx:
        sp = [torch.empty((SWEEPS, R, C), dtype=torch.float32, device="cuda") for _ in range(2)]
        pair(f"project_points, {SWEEPS} sweeps of {PER_SWEEP} points", lambda nearest, k: ctx.project_points_dev(points, offsets, T, P, R, C, sp[k], nearest=nearest), sp)
        pair(f"project_points_calib, {SWEEPS} sweeps of {PER_SWEEP} points",
             lambda nearest, k: ctx.project_points_calib_dev(points, offsets, pt, R, C, sp[k], nearest=nearest), sp)
        del sp
    del points
    # ---- reprojection
    frames = synth.synth_batch(32, R, C, 0)
    src = torch.from_numpy(frames).cuda().repeat(B // 32, 1, 1).contiguous()
    with Context(0, R, C, B) as ctx:
        dense = ctx.complete_dev(src, params=make_params())
        del src
        out = [torch.empty_like(dense) for _ in range(2)]
        M = api.inverse_f32(np.array([[9.998817e-01, 1.511453e-02, -2.841595e-03, 0], [-1.511724e-02, 9.998853e-01, -9.338510e-04, 0],
                                      [2.827154e-03, 9.766976e-04, 9.999955e-01, 0], [0, 0, 0, 1]]))
        shift = np.eye(4, dtype=np.float32)
        shift[0, 3] = 0.54
        for what, m in (("R_rect_02 inverted", M), ("0.54 m along x", shift)):
            rp = api.make_reproject_params(M=m)
            K = np.array(list(rp.K), np.float32).reshape(3, 3)
            rt = api.calib_to_device(api.make_reproject_calib(np.repeat(m[None], B, 0), np.repeat(K[None], B, 0), rp.fx, rp.fy, rp.cx, rp.cy))
            pair(f"reproject_depth, {B} dense frames, {what}", lambda nearest, k: ctx.reproject_depth_dev(dense, R, C, rp, d_out=out[k], nearest=nearest), out)
            pair(f"reproject_depth_calib, {B} dense frames, {what}", lambda nearest, k: ctx.reproject_depth_calib_dev(dense, R, C, rt, d_out=out[k], nearest=nearest), out)


if __name__ == "__main__":
    main()
