"""SLIC's two pixel renderings on the device (352x1216, 256 frames of real SLIC labels, step 18, nc 50, behind slic_connectivity_dev):
slic_contours_dev with both outputs and slic_cluster_means_dev against the slic_labels_dev and slic_connectivity_dev calls they
follow and plain device copies of the bytes they move (contours: 4 B/px of labels in, 1 B/px of mask and 3 B/px of image = 8 B/px;
means: the labels twice, the image in and out = 14 B/px), in one alternating session.  Medians of REPS alternating repetitions in
one process, with the range.  The per-kernel split (the three contour launches, the three of the means) comes from the same script
under the profiler, with fewer repetitions:
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o contours -- python3 tools/time_contours.py --profile"""
import os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from depth_completion_mt_amd import Context, synth
B, R, C, STEP, NC = 256, 352, 1216, 18, 50
PROFILE = "--profile" in sys.argv
REPS, INNER = (1, 2) if PROFILE else (7, 5)
imgs = torch.from_numpy(np.ascontiguousarray(np.stack([synth.synth_lab(R, C, i) for i in range(8)]))).cuda().repeat(B // 8, 1, 1, 1).contiguous()


def timed(fn):
    for _ in range(0 if PROFILE else 2): fn()
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


with Context(0, R, C, B) as ctx:
    raw, n = ctx.slic_labels_dev(imgs, STEP, NC)
    labels, max_labels, counts = ctx.slic_connectivity_dev(raw, n)
    bgr, mask = imgs.clone(), torch.empty((B, R, C), dtype=torch.uint8, device="cuda")
    sums = torch.empty((B, max_labels, 4), dtype=torch.int32, device="cuda")
    scratch, scratch2 = torch.empty_like(raw), torch.empty_like(labels)
    seven, seven2 = torch.empty((B, R, C, 7), dtype=torch.uint8, device="cuda"), torch.empty((B, R, C, 7), dtype=torch.uint8, device="cuda")
    ctx.slic_contours_dev(labels, bgr, (0, 0, 200), mask)
    torch.cuda.synchronize()
    print(f"--- {B} frames of {R} x {C}, step {STEP}, nc {NC}: {n} centres, max_labels {max_labels}, regions {counts[:8].tolist()}; "
          f"taken {[round(float((mask[f] != 0).float().mean()), 4) for f in range(4)]} of the pixels")
    px = B * R * C
    t = alternating({
        "contours": lambda: ctx.slic_contours_dev(labels, bgr, (0, 0, 200), mask),
        "contours, mask only": lambda: ctx.slic_contours_dev(labels, None, (0, 0, 200), mask),
        "means": lambda: ctx.slic_cluster_means_dev(labels, max_labels, bgr, sums),
        "means, raw labels": lambda: ctx.slic_cluster_means_dev(raw, n, bgr, None),
        "slic": lambda: ctx.slic_labels_dev(imgs, STEP, NC, scratch),
        "connectivity": lambda: ctx.slic_connectivity_dev(raw, n, scratch2, counts),
        "copy8": lambda: scratch2.copy_(labels),
        "copy14": lambda: seven2.copy_(seven),
    })
    line("slic_contours_dev, image and mask", t["contours"], 8 * px)
    line("slic_contours_dev, mask only", t["contours, mask only"], 5 * px)
    line("slic_cluster_means_dev with d_sums, connected labels", t["means"], 14 * px)
    line("slic_cluster_means_dev without d_sums, raw labels", t["means, raw labels"], 14 * px)
    line("slic_labels_dev (the call they follow)", t["slic"])
    line("slic_connectivity_dev (out of place)", t["connectivity"], 8 * px)
    line("device copy (8 B/px)", t["copy8"], 8 * px)
    line("device copy (14 B/px)", t["copy14"], 14 * px)
    print(f"slic_contours_dev / slic_labels_dev = {t['contours'][0] / t['slic'][0]:.3f}, / copy = {t['contours'][0] / t['copy8'][0]:.2f}; "
          f"slic_cluster_means_dev / slic_labels_dev = {t['means'][0] / t['slic'][0]:.3f}, / copy = {t['means'][0] / t['copy14'][0]:.2f}")
