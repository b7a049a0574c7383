"""Semi-global matching with the census cost on the device against the absolute-difference call (352x1216, 64 pairs, D = 64, a workspace
of 16 frames: four chunks; the pairs and sizes of tools/time_sgm_guided.py; --rows, --cols and --disparities change them: --disparities
128 reaches the instances of k_sgm_rows with two disparities a lane, --cols 4100 with a small --rows those that do not stage their row
in LDS): sgm_dev(cost="census") against sgm_dev(cost="absdiff")
with four and with eight paths, and with a dense guide (every pixel hinted) on both, both outputs, in one alternating session.
Medians of REPS alternating repetitions in one process, with the range.  The comparison partner of every census figure is the
absolute-difference call of the same session.
Then the rows kernel: the tool starts itself once more as a fresh child process under the kernel trace,
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o sgm -- python3 tools/time_sgm_census.py --profile
(--profile: three four-path calls each with absolute differences and with census, without a guide and with the dense one), and prints
the mean time of the four instances of k_sgm_rows<NPL, LDS, GUIDED, COST> per launch, that is per chunk of 16 frames, beside the other
kernels, from DIR's kernel_stats.csv; every census instance beside the absolute-difference instance of the same <NPL, LDS, GUIDED>.
--no-kernels leaves that step out."""
import argparse, csv, glob, os, re, shutil, statistics, subprocess, sys, tempfile
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from depth_completion_mt_amd import Context, sgm_workspace_bytes, synth
ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=352)
ap.add_argument("--cols", type=int, default=1216)
ap.add_argument("--disparities", type=int, default=64)
ap.add_argument("--profile", action="store_true")
ap.add_argument("--no-kernels", action="store_true")
args = ap.parse_args()
B, R, C, D, HELD = 64, args.rows, args.cols, args.disparities, 16
REPS = 5
PROFILE = args.profile
pairs = [synth.synth_stereo(R, C, seed) for seed in range(4)]
left = torch.from_numpy(np.stack([p[0] for p in pairs])).cuda().repeat(B // 4, 1, 1).contiguous()
right = torch.from_numpy(np.stack([p[1] for p in pairs])).cuda().repeat(B // 4, 1, 1).contiguous()
assert left.dtype == torch.uint8 and tuple(left.shape) == (B, R, C)
rng = np.random.default_rng(0)
bf = np.float32(0.54) * np.float32(9.597910e+02)                 # dcmt_default_sgm_params
dense_np = (bf / rng.uniform(1.0, 40.0, (4, R, C))).astype(np.float32)
dense = torch.from_numpy(dense_np).cuda().repeat(B // 4, 1, 1).contiguous()
GUIDES = {"none": None, "dense": dense}
COSTS = ("absdiff", "census")


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
    run = lambda paths, guide, cost: ctx.sgm_dev(left, right, d_disp16=d16, d_depth=depth, d_work=work, num_disparities=D, paths=paths, d_guide=guide,
                                                 cost=cost)
    if PROFILE:
        for guide in GUIDES.values():
            for cost in COSTS:
                for _ in range(3):
                    run(4, guide, cost)
        torch.cuda.synchronize()
        sys.exit(0)
    print(f"--- {B} pairs of {R} x {C}, D = {D}, workspace of {HELD} frames ({work.numel() / 1e9:.2f} GB)")
    valid = {}
    for cost in COSTS:
        run(4, None, cost)
        valid[cost] = float((d16 >= 0).float().mean())
    print(f"valid pixels, four paths, no guide: absdiff {valid['absdiff']:.3f}, census {valid['census']:.3f}")
    t = alternating({(paths, name, cost): (lambda paths=paths, guide=guide, cost=cost: run(paths, guide, cost))
                     for paths in (4, 8) for name, guide in GUIDES.items() for cost in COSTS})
    for paths in (4, 8):
        for name in GUIDES:
            for cost in COSTS:
                line(f"sgm_dev, {paths} paths, guide: {name}, cost: {cost}, disp16 + depth", t[(paths, name, cost)])
            a, c = t[(paths, name, "absdiff")], t[(paths, name, "census")]
            print(f"{paths} paths, guide {name}: census - absdiff = {c[0] - a[0]:+.3f} ms a call ({c[0] / a[0]:.3f} times), "
                  f"{(c[0] - a[0]) / (B // HELD):+.3f} ms a chunk; the absdiff call's own range is {a[2] - a[1]:.3f} ms")


# ---- the kernels, from a kernel trace of a child process (the context above is closed; the child opens its own) ----------------------
if not args.no_kernels:
    tracer = shutil.which("rocprofv3")
    if tracer is None:
        print("the kernels: rocprofv3 not found, not measured")
        sys.exit(0)
    with tempfile.TemporaryDirectory() as out:
        r = subprocess.run([tracer, "--kernel-trace", "--stats", "--output-format", "csv", "-d", out, "-o", "sgm", "--", sys.executable,
                            os.path.abspath(__file__), "--profile", "--rows", str(R), "--cols", str(C), "--disparities", str(D)],
                           capture_output=True, text=True, timeout=600)
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
        m = re.fullmatch(r"k_sgm_rows<(.+), 1>", k)                  # <NPL, LDS, GUIDED, COST>: COST 1 is census, 0 its partner
        partner = mean.get(f"k_sgm_rows<{m.group(1)}, 0>") if m else None
        if partner:
            print(f"{k} / its absolute-difference instance = {v / partner:.3f}, {v - partner:+.3f} ms a launch")
