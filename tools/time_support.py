"""The distance to the nearest LiDAR return and the trust mask on the device (1024 frames of 352x1216, synth.synth_batch: about 4 %
returns, none in the upper third): support_distance_dev as dist2 alone, as the trust mask alone out of place, and as the trust mask
alone in place, at R = 9 and at R = 32, against a plain device copy of each form's stated bytes (dist2: 4 read, 2 written; out of
place: 4 + 4 read, 4 written; in place: 4 read and 4 written per pixel beyond R) and against the sparse_occlusion_dev call on the same
planes, in one alternating session; and dist2 alone on ONE frame per call, where the column pass has 19 waves.  Medians of REPS alternating repetitions in one process, with the range.  The in-place call runs
on a plane it has already masked after its first repetition; its kernels do the same work whatever the dense plane holds.
The per-kernel split comes from two child runs of the same script under the profiler (the dist2-alone call at R = 9, then at R = 32, and
nothing else), started before this process touches the device:
    python3 tools/time_support.py --split     (runs rocprofv3 --kernel-trace --stats ... -- python3 tools/time_support.py --profile R)"""
import csv, glob, os, statistics, subprocess, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PROFILE, SPLIT = "--profile" in sys.argv, "--split" in sys.argv


def kernel_split(radius):
    """The k_support* rows of the kernel statistics of a child that makes the dist2-alone call at that radius and nothing else:
    (radius, name, calls, total ns, average ns)."""
    with tempfile.TemporaryDirectory() as d:
        r = subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "support", "--", sys.executable,
                            os.path.abspath(__file__), "--profile", str(radius)], capture_output=True, text=True)
        if r.returncode != 0:
            print(f"--- the profiler child failed ({r.returncode}): {r.stderr[-400:]}")
            return []
        rows = []
        for path in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
            with open(path, newline="") as f:
                for row in csv.DictReader(f):
                    if "k_support" in row.get("Name", ""):
                        rows.append((radius, row["Name"].split("(")[0], int(row["Calls"]), int(row["TotalDurationNs"]), float(row["AverageNs"])))
        return rows


split = kernel_split(9) + kernel_split(32) if SPLIT else []

import numpy as np, torch  # noqa: E402
from depth_completion_mt_amd import Context, synth  # noqa: E402
B, R, C = 1024, 352, 1216
RADII = (int(sys.argv[sys.argv.index("--profile") + 1]),) if PROFILE else (9, 32)      # (the child: one radius and one form, so that a kernel's row of the statistics is one configuration)
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


def copier(nbytes):
    """A device copy that moves nbytes in all: half of them read, half written."""
    src = torch.empty((int(nbytes) // 2,), dtype=torch.uint8, device="cuda").fill_(3)
    dst = torch.empty_like(src)
    return lambda: dst.copy_(src)


with Context(0, R, C, B) as ctx:
    sparse = torch.from_numpy(synth.synth_batch(32, R, C, 0)).cuda().repeat(B // 32, 1, 1).contiguous()
    dense = torch.rand((B, R, C), dtype=torch.float32, device="cuda") * 80.0 + 1.0
    out, work, filtered = torch.empty_like(dense), dense.clone(), torch.empty_like(sparse)
    dist2 = torch.empty((B, R, C), dtype=torch.uint16, device="cuda")
    px = B * R * C
    share = {}
    for radius in RADII:
        beyond = ctx.support_distance_dev(sparse, d_dist2=dist2, beyond=True, max_radius=radius)[1]
        share[radius] = float(beyond[:32].double().mean()) / (R * C)
    torch.cuda.synchronize()
    print(f"--- {B} frames of {R} x {C}: returns {float((sparse[:32] > 0).float().mean()):.4f} of the pixels; beyond R: "
          + ", ".join(f"{share[r]:.4f} at R = {r}" for r in RADII))
    cases = {}
    for radius in RADII:
        cases[f"dist2 {radius}"] = lambda radius=radius: ctx.support_distance_dev(sparse, d_dist2=dist2, max_radius=radius)
        if PROFILE:
            continue
        cases[f"out {radius}"] = lambda radius=radius: ctx.support_distance_dev(sparse, dense, d_out=out, max_radius=radius)
        cases[f"in place {radius}"] = lambda radius=radius: ctx.support_distance_dev(sparse, work, d_out=work, max_radius=radius)
        cases[f"copy in place {radius}"] = copier(px * (4 + 4 * share[radius]))
    if not PROFILE:
        one, one_d2 = sparse[:1].clone(), dist2[:1].clone()
        cases["dist2 9, one frame"] = lambda: ctx.support_distance_dev(one, d_dist2=one_d2, max_radius=9)
        cases["copy6"] = copier(6 * px)
        cases["copy12"] = copier(12 * px)
        cases["occlusion"] = lambda: ctx.sparse_occlusion_dev(sparse, filtered)
    t = alternating(cases)
    for radius in () if PROFILE else RADII:
        line(f"support_distance_dev dist2 alone, R = {radius}", t[f"dist2 {radius}"], 6 * px)
        line(f"support_distance_dev trust mask out of place, R = {radius}", t[f"out {radius}"], 12 * px)
        line(f"support_distance_dev trust mask in place, R = {radius}", t[f"in place {radius}"], int(px * (4 + 4 * share[radius])))
        line(f"device copy of the in-place form's bytes, R = {radius}", t[f"copy in place {radius}"], int(px * (4 + 4 * share[radius])))
    if not PROFILE:
        med, lo, hi = t["dist2 9, one frame"]
        print(f"support_distance_dev dist2 alone, R = 9, ONE frame per call (19 waves in the column pass): {med * 1e3:.2f} us [{lo * 1e3:.2f} .. {hi * 1e3:.2f}]")
        line("device copy (6 B/px)", t["copy6"], 6 * px)
        line("device copy (12 B/px)", t["copy12"], 12 * px)
        line("sparse_occlusion_dev out of place, the defaults", t["occlusion"], 8 * px)
    for radius in () if PROFILE else RADII:
        print(f"R = {radius}: dist2 / copy6 = {t[f'dist2 {radius}'][0] / t['copy6'][0]:.2f}, out of place / copy12 = {t[f'out {radius}'][0] / t['copy12'][0]:.2f}, "
              f"in place / its copy = {t[f'in place {radius}'][0] / t[f'copy in place {radius}'][0]:.2f}, "
              f"dist2 / sparse_occlusion_dev = {t[f'dist2 {radius}'][0] / t['occlusion'][0]:.2f}")
for radius, name, calls, total, avg in split:
    print(f"[profiler child, dist2 alone, R = {radius}] {name}: {calls} calls, {avg / 1e6:.4f} ms each, {total / 1e6:.3f} ms in all")
