"""Eight-path semi-global matching on the device against the four-path call (352x1216, 64 pairs, D = 64, a workspace of 16 frames: four
chunks; the pairs and sizes of tools/time_sgm.py): sgm_dev(paths=8) and sgm_dev(paths=4), both outputs, and a plain device copy of the
bytes of one volume of the 64 frames, in one alternating session.  Medians of REPS alternating repetitions in one process, with the
range.
Then the kernels: the tool starts itself once more as a fresh child process under the kernel trace,
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o sgm -- python3 tools/time_sgm_paths.py --profile
(--profile: only three eight-path calls with both outputs), and prints the mean time of k_sgm_rows, k_sgm_cols, the two k_sgm_diag and
k_sgm_winner per launch, that is per chunk of 16 frames, from DIR's kernel_stats.csv, and each k_sgm_diag against k_sgm_cols, whose
bytes it moves.  --no-kernels leaves that step out."""
import csv, glob, os, shutil, statistics, subprocess, sys, tempfile
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from depth_completion_mt_amd import Context, sgm_workspace_bytes, synth
B, R, C, D, HELD = 64, 352, 1216, 64, 16
REPS = 5
PROFILE = "--profile" in sys.argv[1:]
pairs = [synth.synth_stereo(R, C, seed) for seed in range(4)]
left = torch.from_numpy(np.stack([p[0] for p in pairs])).cuda().repeat(B // 4, 1, 1).contiguous()
right = torch.from_numpy(np.stack([p[1] for p in pairs])).cuda().repeat(B // 4, 1, 1).contiguous()
assert left.dtype == torch.uint8 and tuple(left.shape) == (B, R, C)


def timed(fn, reps=3):
    fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(); a.record()
    for _ in range(reps): fn()
    b.record(); torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def alternating(cases):
    """cases: {name: fn}; REPS rounds, every case once per round in turn.  Returns {name: (median, min, max)} in ms."""
    ms = {k: [] for k in cases}
    for _ in range(REPS):
        for k, fn in cases.items():
            ms[k].append(timed(fn))
    return {k: (statistics.median(v), min(v), max(v)) for k, v in ms.items()}


def line(name, t):
    med, lo, hi = t
    print(f"{name}: {med:.3f} ms [{lo:.3f} .. {hi:.3f}], {med / B:.4f} ms a pair, {B / med * 1e3:.0f} pairs/s")


with Context(0, R, C, B) as ctx:
    work = torch.empty(sgm_workspace_bytes(R, C, D, HELD), dtype=torch.uint8, device="cuda")
    d16 = torch.empty((B, R, C), dtype=torch.int16, device="cuda")
    depth = torch.empty((B, R, C), dtype=torch.float32, device="cuda")
    if PROFILE:
        for _ in range(3):
            ctx.sgm_dev(left, right, d_disp16=d16, d_depth=depth, d_work=work, num_disparities=D, paths=8)
        torch.cuda.synchronize()
        sys.exit(0)
    valid = {}
    for paths in (4, 8):
        ctx.sgm_dev(left, right, d_disp16=d16, d_depth=depth, d_work=work, num_disparities=D, paths=paths)
        valid[paths] = float((d16 >= 0).float().mean())
    volume = 2 * B * R * C * D                                   # bytes of one volume of all 64 frames
    src, dst = work[:volume // 4], work[volume // 4: volume // 2]   # the workspace holds a quarter of them: four copies
    t = alternating({
        "eight": lambda: ctx.sgm_dev(left, right, d_disp16=d16, d_depth=depth, d_work=work, num_disparities=D, paths=8),
        "four": lambda: ctx.sgm_dev(left, right, d_disp16=d16, d_depth=depth, d_work=work, num_disparities=D, paths=4),
        "copy": lambda: [dst.copy_(src) for _ in range(4)],
    })
    print(f"--- {B} pairs of {R} x {C}, D = {D}, workspace of {HELD} frames ({work.numel() / 1e9:.2f} GB); valid pixels: {valid[4]:.3f} with four paths, "
          f"{valid[8]:.3f} with eight")
    line("sgm_dev, eight paths, disp16 + depth", t["eight"])
    line("sgm_dev, four paths, disp16 + depth", t["four"])
    line(f"device copy of one volume ({volume / 1e9:.2f} GB read, as much written)", t["copy"])
    print(f"eight / four = {t['eight'][0] / t['four'][0]:.3f}; the diagonals cost {(t['eight'][0] - t['four'][0]) / (B // HELD) / 2:.3f} ms a launch by difference; "
          f"eight / copy of one volume = {t['eight'][0] / t['copy'][0]:.2f}")


# ---- the kernels, from a kernel trace of a child process (the context above is closed; the child opens its own) ----------------------
if "--no-kernels" not in sys.argv[1:]:
    tracer = shutil.which("rocprofv3")
    if tracer is None:
        print("the kernels: rocprofv3 not found, not measured")
        sys.exit(0)
    with tempfile.TemporaryDirectory() as out:
        r = subprocess.run([tracer, "--kernel-trace", "--stats", "--output-format", "csv", "-d", out, "-o", "sgm", "--", sys.executable,
                            os.path.abspath(__file__), "--profile"], capture_output=True, text=True, timeout=600)
        found = glob.glob(os.path.join(out, "**", "*kernel_stats.csv"), recursive=True)
        if r.returncode != 0 or not found:
            print(f"the kernels: the traced run failed (status {r.returncode})\n{r.stderr[-2000:]}")
            sys.exit(1)
        with open(found[0], newline="") as f:
            rows = [row for row in csv.DictReader(f) if "k_sgm_" in row["Name"]]
    mean = {}
    for row in sorted(rows, key=lambda row: row["Name"]):
        name = row["Name"].split("dcmt::")[1].split("(")[0]
        mean[name] = float(row["AverageNs"]) / 1e6
        print(f"{name}: {mean[name]:.3f} ms a launch ({HELD} frames) [{float(row['MinNs']) / 1e6:.3f} .. {float(row['MaxNs']) / 1e6:.3f}], "
              f"{row['Calls']} launches")
    total = sum(mean.values())
    print(f"the five together: {total:.3f} ms a chunk, {total * (B // HELD):.3f} ms a call of {B // HELD} chunks")
    cols = [v for k, v in mean.items() if "k_sgm_cols" in k]
    for k, v in mean.items():
        if "k_sgm_diag" in k and cols:
            print(f"{k} / k_sgm_cols = {v / cols[0]:.3f}")
