"""JET colourisation on the device (dcmt_colorize_dev, 352x1216): ms and the fraction of 8 TB/s at 1024 frames, for the 11 B/px the
two passes move (min/max read, re-read, 3-byte write) and for the 7 B/px lower bound (one read, one write); batch 1; one
complete + colorize step against complete alone on the same stream."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from depth_completion_mt_amd import Context, make_params, synth
B, R, C = 1024, 352, 1216
frames = synth.synth_batch(32, R, C, 0)
src = torch.from_numpy(frames).cuda().repeat(B // 32, 1, 1).contiguous()
out = torch.empty((B, R, C, 3), dtype=torch.uint8, device="cuda")
p = make_params()


def timed(fn, reps=20):
    for _ in range(3): fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(); a.record()
    for _ in range(reps): fn()
    b.record(); torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def report(name, ms, n):
    px = n * R * C
    f11, f7 = px * 11 / (ms * 1e-3) / 8e12, px * 7 / (ms * 1e-3) / 8e12
    print(f"{name}: {ms:.4f} ms ({px * 11 / (ms * 1e-3) / 1e9:.0f} GB/s of the 11 B/px = {f11:.3f} of 8 TB/s; "
          f"7 B/px lower bound: {f7:.3f})")


with Context(0, R, C, B) as ctx:
    dense = ctx.complete_dev(src, params=p)                      # dense planes, as a caller colourises them
    report("colorize_dev, 1024 frames", timed(lambda: ctx.colorize_dev(dense, d_bgr=out)), B)
    report("colorize_dev, batch 1", timed(lambda: ctx.colorize_dev(dense[:1], d_bgr=out[:1]), 200), 1)
    dst = torch.empty_like(src)
    t_c = timed(lambda: ctx.complete_dev(src, dst, p))
    t_cc = timed(lambda: (ctx.complete_dev(src, dst, p), ctx.colorize_dev(dst, d_bgr=out)))
    print(f"step, 1024 frames: complete {t_c:.3f} ms ({B / t_c * 1e3:.0f} frames/s); complete + colorize {t_cc:.3f} ms "
          f"({B / t_cc * 1e3:.0f} frames/s, +{(t_cc / t_c - 1) * 100:.1f} %)")
