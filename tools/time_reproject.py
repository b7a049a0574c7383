"""Reprojection on the device (dcmt_reproject_depth_dev): 1024 dense frames of 352x1216 into 375x1242 with the f32-rounded inverse of
KITTI's R_rect_02, timed with HIP events, against the composition that was possible before the call existed -- depth_to_cloud_dev
without colour followed by project_points_dev with T = M, P = [K | 0] -- alternating in the same process (each side on a context of its own), REPS rounds, medians with
the range.  (The composition is not the same arithmetic: it drops depth <= 0 and divides by P's third row.)  Bytes by the formula of
dcmt_kernels_reproject.h: 4 per source pixel + 4 per landing pixel + 8 per destination pixel + 4 per destination pixel with a winner;
the composition's by those of dcmt_kernels_cloud.h (4 + 4 + 16 v per source pixel) and of N2 (16 + 4 per point, 8 per destination
pixel + 16 per winner).  `--frames N` changes the batch; the per-kernel split comes from a kernel trace of this tool."""
import argparse, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from depth_completion_mt_amd import Context, make_reproject_params, synth
from depth_completion_mt_amd.api import inverse_f32

ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, default=1024)
ap.add_argument("--reps", type=int, default=6)
args = ap.parse_args()
B, R, C, OR, OC = args.frames, 352, 1216, 375, 1242
R_RECT_02 = np.eye(4)
R_RECT_02[:3, :3] = np.array([9.998817e-01, 1.511453e-02, -2.841595e-03, -1.511724e-02, 9.998853e-01, -9.338510e-04,
                              2.827154e-03, 9.766976e-04, 9.999955e-01]).reshape(3, 3)
M = inverse_f32(R_RECT_02)
p = make_reproject_params(M=M)
K = np.array(p.K[:], np.float32).reshape(3, 3)
P = np.concatenate([K, np.zeros((3, 1), np.float32)], axis=1)


def timed(fn, reps=5):
    for _ in range(2): fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(); a.record()
    for _ in range(reps): fn()
    b.record(); torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def show(name, v, bytes_moved):
    med = statistics.median(v)
    rate = bytes_moved / (med * 1e-3)
    print(f"{name}: median {med:.4f} ms [{min(v):.4f} .. {max(v):.4f}], {bytes_moved / 1e9:.3f} GB stated -> {rate / 1e12:.2f} TB/s = {rate / 8e12:.3f} of 8 TB/s")


# one context per side: the composition's projection takes 438 M points, which moves its winner plane to 29 index bits (7 generations:
# a clear of the whole plane every 7th call) for good; a caller of the reprojection alone stays at 24 bits and 255 generations
with Context(0, OR, OC, B) as ctx, Context(0, OR, OC, B) as ctx2:
    nb = min(B, 32)
    src = torch.from_numpy(synth.synth_batch(nb, R, C, 0)).cuda()
    dense = ctx.complete_dev(src).repeat((B + nb - 1) // nb, 1, 1)[:B].contiguous()
    del src
    out = torch.empty((B, OR, OC), dtype=torch.float32, device="cuda")
    out2 = torch.empty((B, OR, OC), dtype=torch.float32, device="cuda")
    pts = torch.empty((B * R * C, 4), dtype=torch.float32, device="cuda")
    off = torch.empty((B + 1,), dtype=torch.int32, device="cuda")

    def new():
        ctx.reproject_depth_dev(dense, OR, OC, p, d_out=out)

    def composed():
        ctx2.depth_to_cloud_dev(dense, None, d_points=pts, d_offsets=off)
        ctx2.project_points_dev(pts, off, M, P, OR, OC, d_sparse=out2)

    new(); composed()
    torch.cuda.synchronize()
    n_pts = int(off[B].item())
    won = int((out != 0).sum().item())
    won2 = int((out2 != 0).sum().item())
    # pixels that land: counted on frame 0 with the same arithmetic on the host would cost a restatement here; the winners bound them from
    # below and the source pixels from above, and with this matrix the two differ by 1 %: the stated bytes use the source pixel count
    spx, dpx = B * R * C, B * OR * OC
    bytes_new = 4 * spx + 4 * spx + 8 * dpx + 4 * won
    bytes_cmp = (8 * spx + 16 * n_pts) + (20 * n_pts + 8 * dpx + 16 * won2)
    print(f"--- {B} frame(s) {R}x{C} -> {OR}x{OC}; {n_pts / spx:.4f} of the source pixels have depth > 0; destination pixels with a winner: "
          f"{won / dpx:.4f} (reproject), {won2 / dpx:.4f} (composition); same planes: {bool(torch.equal(out, out2))}")
    t_new, t_cmp = [], []
    for _ in range(args.reps):
        t_new.append(timed(new))
        t_cmp.append(timed(composed))
    show("reproject_depth_dev", t_new, bytes_new)
    show("depth_to_cloud_dev + project_points_dev", t_cmp, bytes_cmp)
    print(f"ranges overlap: {not (max(t_new) < min(t_cmp) or max(t_cmp) < min(t_new))}; composition / reproject = {statistics.median(t_cmp) / statistics.median(t_new):.2f}")
