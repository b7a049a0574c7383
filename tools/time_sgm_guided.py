"""LiDAR-guided semi-global matching on the device against the unguided call (352x1216, 64 pairs, D = 64, a workspace of 16 frames: four
chunks; the pairs and sizes of tools/time_sgm_paths.py): sgm_dev(d_guide=) with a sparse guide (about 5 % of the pixels hinted) and with
a dense one (every pixel) against sgm_dev without a guide, with four and with eight paths, both outputs, in one alternating session.
Medians of REPS alternating repetitions in one process, with the range.  The guides hold the depth of a disparity between 1 and 40,
changing from pixel to pixel.
Then the rows kernel: the tool starts itself once more as a fresh child process under the kernel trace,
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o sgm -- python3 tools/time_sgm_guided.py --profile
(--profile: three four-path calls each without a guide, with the sparse and with the dense one), and prints the mean time of
the unguided and the guided instance of k_sgm_rows<NPL, LDS, GUIDED, COST> per launch, that is per chunk of 16 frames, beside the other
kernels, from DIR's kernel_stats.csv.
--no-kernels leaves that step out."""
import csv, glob, os, re, shutil, statistics, subprocess, sys, tempfile
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
rng = np.random.default_rng(0)
bf = np.float32(0.54) * np.float32(9.597910e+02)                 # dcmt_default_sgm_params
dense_np = (bf / rng.uniform(1.0, 40.0, (4, R, C))).astype(np.float32)
sparse_np = np.where(rng.random((4, R, C)) < 0.05, dense_np, np.float32(0))
dense = torch.from_numpy(dense_np).cuda().repeat(B // 4, 1, 1).contiguous()
sparse = torch.from_numpy(sparse_np).cuda().repeat(B // 4, 1, 1).contiguous()
GUIDES = {"none": None, "sparse": sparse, "dense": dense}


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
    run = lambda paths, guide: ctx.sgm_dev(left, right, d_disp16=d16, d_depth=depth, d_work=work, num_disparities=D, paths=paths, d_guide=guide)
    if PROFILE:
        for guide in GUIDES.values():
            for _ in range(3):
                run(4, guide)
        torch.cuda.synchronize()
        sys.exit(0)
    print(f"--- {B} pairs of {R} x {C}, D = {D}, workspace of {HELD} frames ({work.numel() / 1e9:.2f} GB); hinted pixels: "
          f"{float((sparse > 0).float().mean()):.3f} of the sparse guide, {float((dense > 0).float().mean()):.3f} of the dense one")
    t = alternating({(paths, name): (lambda paths=paths, guide=guide: run(paths, guide)) for paths in (4, 8) for name, guide in GUIDES.items()})
    for paths in (4, 8):
        for name in GUIDES:
            line(f"sgm_dev, {paths} paths, guide: {name}, disp16 + depth", t[(paths, name)])
        plain = t[(paths, "none")]
        for name in ("sparse", "dense"):
            print(f"{paths} paths: {name} - none = {t[(paths, name)][0] - plain[0]:+.3f} ms a call, {(t[(paths, name)][0] - plain[0]) / (B // HELD):+.3f} ms a chunk; "
                  f"the unguided call's own range is {plain[2] - plain[1]:.3f} ms")


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
    for k, v in mean.items():
        m = re.fullmatch(r"k_sgm_rows<(.+), true, (\d+)>", k)        # <NPL, LDS, GUIDED, COST>
        plain = mean.get(f"k_sgm_rows<{m.group(1)}, false, {m.group(2)}>") if m else None
        if plain:
            print(f"{k} / its unguided instance = {v / plain:.3f} (sparse and dense launches together), {v - plain:+.3f} ms a launch")
