"""BGR ingest on the device (dcmt_bgr_convert_dev, 352x1216): ms per 1024 frames for Lab only, grey only and both, the bytes the
kernel moves (6 / 4 / 7 B/px: 3 read, 3 and / or 1 written) over that time, and the ratio to a plain device copy of the SAME byte
count (a copy of n bytes moves 2n) that runs alternating with it in the same process.  Two images: smooth colour regions (synth_lab
read as B, G, R: neighbouring lanes look up equal table entries, which broadcast) and uniform noise (every lookup a different entry:
the worst case for LDS bank conflicts).  Medians of REPS alternating repetitions, with the range; batch 1 last."""
import os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from depth_completion_mt_amd import Context, synth
B, R, C = 1024, 352, 1216
REPS = 7
PX = B * R * C
smooth = torch.from_numpy(np.stack([synth.synth_lab(R, C, i) for i in range(8)])).cuda().repeat(B // 8, 1, 1, 1).contiguous()
noise = torch.randint(0, 256, (B, R, C, 3), dtype=torch.uint8, device="cuda")
lab = torch.empty((B, R, C, 3), dtype=torch.uint8, device="cuda")
gray = torch.empty((B, R, C), dtype=torch.uint8, device="cuda")
copy_src = torch.randint(0, 256, (PX * 7 // 2,), dtype=torch.uint8, device="cuda")
copy_dst = torch.empty_like(copy_src)


def timed(fn, reps=10):
    for _ in range(3): fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(); a.record()
    for _ in range(reps): fn()
    b.record(); torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def alternating(cases, reps=10):
    """cases: {name: fn}; REPS rounds, every case once per round in turn.  Returns {name: (median, min, max)} in ms."""
    ms = {k: [] for k in cases}
    for _ in range(REPS):
        for k, fn in cases.items():
            ms[k].append(timed(fn, reps))
    return {k: (statistics.median(v), min(v), max(v)) for k, v in ms.items()}


def copy_of(moved):
    n = moved // 2
    return lambda: copy_dst[:n].copy_(copy_src[:n])


def report(frames, img, name, reps):
    px = frames * R * C
    i, l, g = img[:frames], lab[:frames], gray[:frames]
    t = alternating({
        "lab": lambda: ctx.bgr_convert_dev(i, d_lab=l), "copy6": copy_of(6 * px),
        "gray": lambda: ctx.bgr_convert_dev(i, lab=False, d_gray=g), "copy4": copy_of(4 * px),
        "both": lambda: ctx.bgr_convert_dev(i, d_lab=l, d_gray=g), "copy7": copy_of(7 * px),
        "in place": lambda: ctx.bgr_convert_dev(l, d_lab=l),
    }, reps)
    print(f"--- {frames} frame(s) of {R} x {C}, {name}")
    for k, c, bpp in (("lab", "copy6", 6), ("gray", "copy4", 4), ("both", "copy7", 7), ("in place", "copy6", 6)):
        (med, lo, hi), (cm, cl, ch) = t[k], t[c]
        rate, crate = bpp * px / (med * 1e-3) / 1e12, bpp * px / (cm * 1e-3) / 1e12
        print(f"bgr_convert_dev {k} ({bpp} B/px): {med:.4f} ms [{lo:.4f} .. {hi:.4f}] = {rate:.2f} TB/s; copy of the same bytes {cm:.4f} ms "
              f"[{cl:.4f} .. {ch:.4f}] = {crate:.2f} TB/s; kernel / copy rate {cm / med:.2f}")


with Context(0, R, C, B) as ctx:
    report(B, smooth, "smooth colour regions", 10)
    report(B, noise, "uniform noise", 10)
    report(1, smooth, "smooth colour regions", 200)
