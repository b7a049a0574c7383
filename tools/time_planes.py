"""The per-superpixel plane fit on the device (352x1216, 256 frames of real SLIC labels, step 18, nc 50, behind slic_connectivity_dev; a
synthetic sparse plane at KITTI density, about 5 % of the pixels): superpixel_planes_dev without and with the trimmed refit, in place
and with d_fits, against slic_cluster_means_dev on the same labels and a plain device copy of the bytes the call must move (depth and
labels in, the plane out, the depth a second time for the paint: 16 B/px; 20 B/px with the refit), in one alternating session.
Medians of REPS alternating repetitions in one process, with the range.  The per-kernel split comes from a child run of the same
script under the profiler, started before this process touches the device:
    python3 tools/time_planes.py --split        (runs rocprofv3 --kernel-trace --stats ... -- python3 tools/time_planes.py --profile)"""
import csv, glob, os, statistics, subprocess, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PROFILE, SPLIT = "--profile" in sys.argv, "--split" in sys.argv


def kernel_split():
    """The k_planes_* rows of the child's kernel statistics: (name, calls, total ns, average ns)."""
    with tempfile.TemporaryDirectory() as d:
        r = subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "planes", "--", sys.executable,
                            os.path.abspath(__file__), "--profile"], capture_output=True, text=True)
        if r.returncode != 0:
            print(f"--- the profiler child failed ({r.returncode}): {r.stderr[-400:]}")
            return []
        rows = []
        for path in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
            with open(path, newline="") as f:
                for row in csv.DictReader(f):
                    if "k_planes" in row.get("Name", ""):
                        rows.append((row["Name"].split("(")[0], int(row["Calls"]), int(row["TotalDurationNs"]), float(row["AverageNs"])))
        return rows


split = kernel_split() if SPLIT else []

import numpy as np, torch  # noqa: E402
from depth_completion_mt_amd import Context, synth  # noqa: E402
B, R, C, STEP, NC = 256, 352, 1216, 18, 50
REPS, INNER = (1, 2) if PROFILE else (7, 5)
imgs = torch.from_numpy(np.ascontiguousarray(np.stack([synth.synth_lab(R, C, i) for i in range(8)]))).cuda().repeat(B // 8, 1, 1, 1).contiguous()


def sparse_plane(seed):
    """A slanted ground and two walls in inverse depth, returns at 5 % of the pixels, a tenth of them displaced (what the refit drops)."""
    g = np.random.Generator(np.random.PCG64(seed))
    V, U = np.mgrid[0:R, 0:C]
    q = np.where(V > 150, 0.012 + 0.0009 * (V - 150), np.where(U < 500, 0.03 + 0.00004 * U, 0.07 - 0.00003 * U))
    z = (1.0 / q) * np.where(g.random((R, C)) < 0.1, 1.3, 1.0)
    return np.where(g.random((R, C)) < 0.05, z, 0.0).astype(np.float32)


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
    depth = torch.from_numpy(np.stack([sparse_plane(i) for i in range(8)])).cuda().repeat(B // 8, 1, 1).contiguous()
    out, work = torch.empty_like(depth), depth.clone()
    fits = torch.empty((B, max_labels, 48), dtype=torch.uint8, device="cuda")
    bgr = imgs.clone()
    eight, eight2 = torch.empty((B, R, C, 2), dtype=torch.float32, device="cuda"), torch.empty((B, R, C, 2), dtype=torch.float32, device="cuda")
    ten, ten2 = torch.empty((B, R, C, 10), dtype=torch.uint8, device="cuda"), torch.empty((B, R, C, 10), dtype=torch.uint8, device="cuda")
    ctx.superpixel_planes_dev(depth, labels, max_labels, out, fits, refit_tol=0.1)
    torch.cuda.synchronize()
    f = fits[:8].cpu().numpy().view(np.dtype([("abc", "<f8", 3), ("seen", "<u4"), ("used", "<u4"), ("w", "<u4", 2), ("kind", "<u4"), ("r", "<u4")]))[..., 0]
    print(f"--- {B} frames of {R} x {C}, step {STEP}, nc {NC}: {n} centres, max_labels {max_labels}; returns {float((depth[:8] > 0).float().mean()):.4f} of the pixels, "
          f"painted {float((out[:8] > 0).float().mean()):.4f}; kinds none / constant / plane {np.bincount(f['kind'].reshape(-1), minlength=3).tolist()}, "
          f"refit kept {int(f['used'].sum())} of {int(f['seen'].sum())} returns")
    px = B * R * C
    t = alternating({
        "planes": lambda: ctx.superpixel_planes_dev(depth, labels, max_labels, out),
        "planes, fits": lambda: ctx.superpixel_planes_dev(depth, labels, max_labels, out, fits),
        "planes, in place": lambda: ctx.superpixel_planes_dev(work, labels, max_labels, work),
        "refit": lambda: ctx.superpixel_planes_dev(depth, labels, max_labels, out, refit_tol=0.1),
        "means": lambda: ctx.slic_cluster_means_dev(labels, max_labels, bgr, None),
        "copy16": lambda: eight2.copy_(eight),
        "copy20": lambda: ten2.copy_(ten),
    })
    line("superpixel_planes_dev", t["planes"], 16 * px)
    line("superpixel_planes_dev with d_fits", t["planes, fits"], 16 * px)
    line("superpixel_planes_dev in place (dense after the first call)", t["planes, in place"], 16 * px)
    line("superpixel_planes_dev, refit_tol 0.1", t["refit"], 20 * px)
    line("slic_cluster_means_dev without d_sums (same labels)", t["means"], 14 * px)
    line("device copy (16 B/px)", t["copy16"], 16 * px)
    line("device copy (20 B/px)", t["copy20"], 20 * px)
    print(f"superpixel_planes_dev / slic_cluster_means_dev = {t['planes'][0] / t['means'][0]:.3f}, / copy = {t['planes'][0] / t['copy16'][0]:.2f}; "
          f"with the refit / without = {t['refit'][0] / t['planes'][0]:.3f}, / copy = {t['refit'][0] / t['copy20'][0]:.2f}")
for name, calls, total, avg in sorted(split, key=lambda r: -r[2]):
    print(f"[profiler child] {name}: {calls} calls, {avg / 1e6:.4f} ms each, {total / 1e6:.3f} ms in all")
