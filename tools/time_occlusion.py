"""The occlusion filter of projected LiDAR returns on the device (1024 frames of 352x1216, synth.synth_batch: about 5 % returns):
sparse_occlusion_dev out of place, in place and on the uint16 payload, at the default window (rx 3, ry 6) and at the largest one
(rx 8, ry 16), against a plain device copy of the 8 B/px the out-of-place call must move (4 read, 4 written) and against the
project_points_dev(nearest=True) call it follows (1024 sweeps of 120 000 points into the same planes), in one alternating session.
Medians of REPS alternating repetitions in one process, with the range.  The in-place call runs on a plane it has already filtered
after its first repetition (nothing left to remove); its kernels do the same work whatever the data, but for the handful of stores.
The per-kernel split comes from a child run of the same script under the profiler, started before this process touches the device:
    python3 tools/time_occlusion.py --split     (runs rocprofv3 --kernel-trace --stats ... -- python3 tools/time_occlusion.py --profile)"""
import csv, glob, os, statistics, subprocess, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PROFILE, SPLIT = "--profile" in sys.argv, "--split" in sys.argv


def kernel_split():
    """The k_occl* rows of the child's kernel statistics: (name, calls, total ns, average ns)."""
    with tempfile.TemporaryDirectory() as d:
        r = subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "occlusion", "--", sys.executable,
                            os.path.abspath(__file__), "--profile"], capture_output=True, text=True)
        if r.returncode != 0:
            print(f"--- the profiler child failed ({r.returncode}): {r.stderr[-400:]}")
            return []
        rows = []
        for path in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
            with open(path, newline="") as f:
                for row in csv.DictReader(f):
                    if "k_occl" in row.get("Name", ""):
                        rows.append((row["Name"].split("(")[0], int(row["Calls"]), int(row["TotalDurationNs"]), float(row["AverageNs"])))
        return rows


split = kernel_split() if SPLIT else []

import numpy as np, torch  # noqa: E402
from depth_completion_mt_amd import Context, synth  # noqa: E402
B, R, C, PER_SWEEP = 1024, 352, 1216, 120000
REPS, INNER = (1, 2) if PROFILE else (7, 5)


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
    sparse = torch.from_numpy(synth.synth_batch(32, R, C, 0)).cuda().repeat(B // 32, 1, 1).contiguous()
    payload = (sparse * 256.0).round().clamp(0, 65535).to(torch.int32).to(torch.int16)          # the bits of the uint16 payload
    out, work, out16 = torch.empty_like(sparse), sparse.clone(), torch.empty_like(payload)
    copy_to = torch.empty_like(sparse)
    removed = torch.empty((B,), dtype=torch.int32, device="cuda")
    points = torch.from_numpy(synth.synth_points(PER_SWEEP, 3)).cuda().repeat(B, 1).contiguous()
    offsets = torch.arange(0, (B + 1) * PER_SWEEP, PER_SWEEP, dtype=torch.int32, device="cuda")
    T, P = synth.KITTI_T_VELO_TO_CAM, synth.KITTI_P2
    projected = torch.empty_like(sparse)
    ctx.sparse_occlusion_dev(sparse, out, d_removed=removed)
    ctx.project_points_dev(points, offsets, T, P, R, C, projected, nearest=True)
    rem_p = ctx.sparse_occlusion_dev(projected, copy_to, removed=True)[1]
    torch.cuda.synchronize()
    print(f"--- {B} frames of {R} x {C}: returns {float((sparse[:32] > 0).float().mean()):.4f} of the pixels, removed at the defaults "
          f"{float(removed[:32].float().mean()):.1f} a frame; of one projected sweep ({int((projected[0] > 0).sum())} returns) {int(rem_p[0])}")
    px = B * R * C
    t = alternating({
        "out": lambda: ctx.sparse_occlusion_dev(sparse, out),
        "out, removed": lambda: ctx.sparse_occlusion_dev(sparse, out, d_removed=removed),
        "in place": lambda: ctx.sparse_occlusion_dev(work, work),
        "payload": lambda: ctx.sparse_occlusion_dev(payload, out16, u16=True),
        "out, 8 x 16": lambda: ctx.sparse_occlusion_dev(sparse, out, rx=8, ry=16),
        "in place, 8 x 16": lambda: ctx.sparse_occlusion_dev(work, work, rx=8, ry=16),
        "project": lambda: ctx.project_points_dev(points, offsets, T, P, R, C, projected, nearest=True),
        "copy8": lambda: copy_to.copy_(sparse),
    })
    line("sparse_occlusion_dev out of place", t["out"], 8 * px)
    line("sparse_occlusion_dev out of place with d_removed", t["out, removed"], 8 * px)
    line("sparse_occlusion_dev in place (4 B/px read, the mask written and read)", t["in place"], 4 * px + px // 4)
    line("sparse_occlusion_dev, uint16 payload, out of place", t["payload"], 4 * px)
    line("sparse_occlusion_dev out of place, rx 8, ry 16", t["out, 8 x 16"], 8 * px)
    line("sparse_occlusion_dev in place, rx 8, ry 16", t["in place, 8 x 16"], 4 * px + px // 4)
    line(f"project_points_dev(nearest=True), {B} sweeps of {PER_SWEEP} points", t["project"])
    line("device copy (8 B/px)", t["copy8"], 8 * px)
    print(f"out of place / copy = {t['out'][0] / t['copy8'][0]:.2f}, in place / copy = {t['in place'][0] / t['copy8'][0]:.2f}, "
          f"payload / copy = {t['payload'][0] / t['copy8'][0]:.2f}, out of place / project_points_dev = {t['out'][0] / t['project'][0]:.3f}")
for name, calls, total, avg in sorted(split, key=lambda r: -r[2]):
    print(f"[profiler child] {name}: {calls} calls, {avg / 1e6:.4f} ms each, {total / 1e6:.3f} ms in all")
