"""The SLIC connectivity pass on the device (352x1216, 256 frames -- the batch the labelled configurations use -- of real SLIC labels,
step 18, nc 50): slic_connectivity_dev against the slic_labels_dev call it follows and a plain device copy of 8 B/px, in one
alternating session.  Medians of REPS alternating repetitions in one process, with the range.  The per-kernel split comes from
the same script under the profiler, with fewer repetitions:
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o conn -- python3 tools/time_connectivity.py --profile"""
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
    labels, n = ctx.slic_labels_dev(imgs, STEP, NC)
    out, counts = torch.empty_like(labels), torch.empty(B, dtype=torch.int32, device="cuda")
    raw = torch.empty_like(labels)
    _, max_labels, _ = ctx.slic_connectivity_dev(labels, n, out, counts)
    torch.cuda.synchronize()
    used = [int(torch.unique(labels[f]).numel()) for f in range(8)]
    print(f"--- {B} frames of {R} x {C}, step {STEP}, nc {NC}: {n} centres, max_labels {max_labels}; labels used {used} -> regions {counts[:8].tolist()}")
    px = B * R * C
    t = alternating({
        "connectivity": lambda: ctx.slic_connectivity_dev(labels, n, out, counts),
        "slic": lambda: ctx.slic_labels_dev(imgs, STEP, NC, raw),
        "copy": lambda: out.copy_(labels),
    })
    line("slic_connectivity_dev, out of place", t["connectivity"], 8 * px)
    line("slic_labels_dev (the call it follows)", t["slic"])
    line("device copy (8 B/px)", t["copy"], 8 * px)
    print(f"slic_connectivity_dev / slic_labels_dev = {t['connectivity'][0] / t['slic'][0]:.3f}, / copy = {t['connectivity'][0] / t['copy'][0]:.2f}")
    if not PROFILE:
        t = alternating({"in place": lambda: ctx.slic_connectivity_dev(out, n, out, counts)})
        line("slic_connectivity_dev, in place (on its own output: connected labels)", t["in place"], 8 * px)
