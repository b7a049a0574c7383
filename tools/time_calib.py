"""The four table calls against their uniform twins (dcmt_*_calib_dev against dcmt_*_dev) on the same device-resident batch: 1024
frames of 352x1216 for the cloud, the reprojection and the stereo refinement, 256 sweeps of 120 000 points for the projection.
Every record of a table equals the uniform call's parameters, so the two calls of a pair do the same arithmetic and write the same
bits (checked first); what is timed is what the table costs -- at most 136 bytes per frame through the scalar cache.

One process, the calls of a pair alternating: REPS rounds, in every round each call timed over `reps` back-to-back calls between
two events.  Per call the median and the range over the rounds; per pair the difference of the medians against the uniform call's
own range, which is the yardstick: a difference inside it is not a difference."""
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


def pair(name, uniform, table, same):
    """Alternating rounds of the two calls, uniform(k) and table(k) writing to output buffer k: first uniform(0) against table(1),
    which `same()` compares bit for bit, then both timed on buffer 0, so that the two calls differ in nothing but the table."""
    uniform(0); table(1); torch.cuda.synchronize()
    assert same(), f"{name}: the table call and the uniform call differ"
    uniform, table = (lambda f=uniform: f(0)), (lambda f=table: f(0))
    ms = {"uniform": [], "table": []}
    for _ in range(REPS):
        ms["uniform"].append(timed(uniform))
        ms["table"].append(timed(table))
    u, t = ms["uniform"], ms["table"]
    mu, mt = statistics.median(u), statistics.median(t)
    spread = max(u) - min(u)
    verdict = "inside" if abs(mt - mu) <= spread else "OUTSIDE"
    print(f"{name}: uniform {mu:.4f} ms [{min(u):.4f} .. {max(u):.4f}], table {mt:.4f} ms [{min(t):.4f} .. {max(t):.4f}], "
          f"table - uniform {mt - mu:+.4f} ms ({(mt / mu - 1) * 100:+.2f} %), {verdict} the uniform call's range of {spread:.4f} ms")


def bits(t):
    return t.view(torch.int32)


def main():
    assert torch.cuda.is_available(), "no GPU: nothing is measured without one"
    frames = synth.synth_batch(32, R, C, 0)
    src = torch.from_numpy(frames).cuda().repeat(B // 32, 1, 1).contiguous()
    bgr = torch.randint(0, 256, (B, R, C, 3), dtype=torch.uint8, device="cuda")
    with Context(0, R, C, B) as ctx:
        dense = ctx.complete_dev(src, params=make_params())
        # ---- cloud
        cp = api.make_cloud_params()
        ct = api.calib_to_device(api.make_cloud_calib([cp.fx] * B, cp.fy, cp.cx, cp.cy))
        pts = [torch.empty((B * R * C, 4), dtype=torch.float32, device="cuda") for _ in range(2)]
        off = [torch.empty((B + 1,), dtype=torch.int32, device="cuda") for _ in range(2)]

        def cloud_same():
            n = int(off[0][B].item())
            return torch.equal(off[0], off[1]) and torch.equal(bits(pts[0][:n]), bits(pts[1][:n]))

        pair(f"depth_to_cloud, {B} dense frames, colour", lambda k: ctx.depth_to_cloud_dev(dense, bgr, cp, d_points=pts[k], d_offsets=off[k]),
             lambda k: ctx.depth_to_cloud_calib_dev(dense, ct, bgr, d_points=pts[k], d_offsets=off[k]), cloud_same)
        pair(f"depth_to_cloud, {B} sparse frames, no colour", lambda k: ctx.depth_to_cloud_dev(src, None, cp, d_points=pts[k], d_offsets=off[k]),
             lambda k: ctx.depth_to_cloud_calib_dev(src, ct, None, d_points=pts[k], d_offsets=off[k]), cloud_same)
        del pts
        # ---- reprojection (KITTI's R_rect_02, inverted: the reference's unrectify_sol)
        M = api.inverse_f32(np.array([[9.998817e-01, 1.511453e-02, -2.841595e-03, 0], [-1.511724e-02, 9.998853e-01, -9.338510e-04, 0],
                                      [2.827154e-03, 9.766976e-04, 9.999955e-01, 0], [0, 0, 0, 1]]))
        rp = api.make_reproject_params(M=M)
        K = np.array(list(rp.K), np.float32).reshape(3, 3)
        rt = api.calib_to_device(api.make_reproject_calib(np.repeat(M[None], B, 0), np.repeat(K[None], B, 0), rp.fx, rp.fy, rp.cx, rp.cy))
        out = [torch.empty_like(dense) for _ in range(2)]
        pair(f"reproject_depth, {B} dense frames", lambda k: ctx.reproject_depth_dev(dense, R, C, rp, d_out=out[k]),
             lambda k: ctx.reproject_depth_calib_dev(dense, R, C, rt, d_out=out[k]), lambda: torch.equal(bits(out[0]), bits(out[1])))
        # ---- stereo refinement
        l, r, d = synth.synth_stereo(R, C, 5)
        left, right = (torch.from_numpy(x).cuda().repeat(B, 1, 1).contiguous() for x in (l, r))
        guess = torch.from_numpy(d).cuda().repeat(B, 1, 1).contiguous()
        st = api.calib_to_device(api.make_stereo_calib(0.54, [9.597910e+02] * B))
        pair(f"stereo_refine, {B} frames, 4 sweeps", lambda k: ctx.stereo_refine_dev(guess, left, right, out[k]),
             lambda k: ctx.stereo_refine_calib_dev(guess, left, right, st, out[k]), lambda: torch.equal(bits(out[0]), bits(out[1])))
        del out, left, right, guess
    # ---- projection
    sweep = synth.synth_points(PER_SWEEP, 3)
    points = torch.from_numpy(sweep).cuda().repeat(SWEEPS, 1).contiguous()
    offsets = torch.arange(0, (SWEEPS + 1) * PER_SWEEP, PER_SWEEP, dtype=torch.int32, device="cuda")
    T, P = synth.KITTI_T_VELO_TO_CAM, synth.KITTI_P2
    pt = api.calib_to_device(api.make_project_calib(np.repeat(T[None], SWEEPS, 0), np.repeat(P[None], SWEEPS, 0)))
    with Context(0, R, C, SWEEPS) as ctx:
        sp = [torch.empty((SWEEPS, R, C), dtype=torch.float32, device="cuda") for _ in range(2)]
        pair(f"project_points, {SWEEPS} sweeps of {PER_SWEEP} points", lambda k: ctx.project_points_dev(points, offsets, T, P, R, C, sp[k]),
             lambda k: ctx.project_points_calib_dev(points, offsets, pt, R, C, sp[k]), lambda: torch.equal(bits(sp[0]), bits(sp[1])))


if __name__ == "__main__":
    main()
