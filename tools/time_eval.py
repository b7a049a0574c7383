"""Accuracy metrics on the device (dcmt_evaluate*_dev, 352x1216): ms, GB/s of algorithmic bytes (8 B/px with f32 GT, 6 B/px with
uint16 GT; the slab is not counted) and the fraction of 8 TB/s, at 1024 frames and at batch 1; what the inverse-depth terms cost
(every pixel masked, with and without them); one complete + evaluate step against complete alone on the same stream."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from depth_completion_mt_amd import Context, make_params, synth
B, R, C = 1024, 352, 1216
gt = synth.synth_batch(32, R, C, 0)
sub = gt.copy()
sub[np.random.default_rng(0).random(sub.shape) < 0.5] = 0
ctx = Context(0, R, C, B)
pred32 = ctx.complete_dev(torch.from_numpy(sub).cuda())
d_gt = torch.from_numpy(gt).cuda().repeat(B // 32, 1, 1).contiguous()
d_u16 = torch.from_numpy(np.round(gt * 256).astype(np.uint16).view(np.int16)).cuda().repeat(B // 32, 1, 1).contiguous()
d_pred = pred32.repeat(B // 32, 1, 1).contiguous()
src = torch.from_numpy(gt).cuda().repeat(B // 32, 1, 1).contiguous()
dst = torch.empty_like(src)
out = torch.empty((B, 7), dtype=torch.float64, device="cuda")
p = make_params()


def timed(fn, reps=20):
    for _ in range(3): fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(); a.record()
    for _ in range(reps): fn()
    b.record(); torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def report(name, ms, n, bpp):
    gbs = n * R * C * bpp / (ms * 1e-3) / 1e9
    print(f"{name}: {ms:.4f} ms ({gbs:.0f} GB/s of the {bpp} B/px = {gbs / 8000:.3f} of 8 TB/s)")


report("evaluate_dev f32 GT, 1024 frames, mode both", timed(lambda: ctx.evaluate_dev(d_gt, d_pred, 0.0, "both", d_out=out)), B, 8)
report("evaluate_dev f32 GT, 1024 frames, mode gt", timed(lambda: ctx.evaluate_dev(d_gt, d_pred, 0.0, "gt", d_out=out)), B, 8)
report("evaluate_dev u16 GT, 1024 frames, mode both", timed(lambda: ctx.evaluate_dev(d_u16, d_pred, 0.0, "both", d_out=out)), B, 6)
report("evaluate_dev f32 GT, batch 1", timed(lambda: ctx.evaluate_dev(d_gt[:1], d_pred[:1], 0.0, "both", d_out=out[:1]), 200), 1, 8)
report("evaluate_dev u16 GT, batch 1", timed(lambda: ctx.evaluate_dev(d_u16[:1], d_pred[:1], 0.0, "both", d_out=out[:1]), 200), 1, 6)
# every pixel in the mask: with the inverse terms (pred > 0) and without them (pred < 0, mode gt)
dense = d_pred + 1.0
pos, neg = d_pred + 0.5, -dense
report("every pixel masked, with inverse terms", timed(lambda: ctx.evaluate_dev(dense, pos, 0.0, "gt", d_out=out)), B, 8)
report("every pixel masked, no inverse terms", timed(lambda: ctx.evaluate_dev(dense, neg, 0.0, "gt", d_out=out)), B, 8)
t_c = timed(lambda: ctx.complete_dev(src, dst, p))
t_ce = timed(lambda: (ctx.complete_dev(src, dst, p), ctx.evaluate_dev(d_gt, dst, 0.0, "both", d_out=out)))
print(f"step, 1024 frames: complete {t_c:.3f} ms ({B / t_c * 1e3:.0f} frames/s); complete + evaluate {t_ce:.3f} ms "
      f"({B / t_ce * 1e3:.0f} frames/s, +{(t_ce / t_c - 1) * 100:.1f} %)")
