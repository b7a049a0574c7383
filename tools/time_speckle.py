"""The speckle filter on the device (352x1216, 64 pairs from synth_stereo through sgm_dev, D = 64): filter_speckles_dev with the
disparity map only (out of place) and with the depth plane and the per-frame counts, against the sgm_dev call it follows and a plain
device copy of the filter's own bytes (the int16 plane: 2 B/px read, 2 B/px written).  Medians of REPS alternating repetitions in one
process, with the range; the fraction of the valid pixels the filter removes is printed beside them.
Then the four kernels: the tool starts itself once more as a fresh child process under the kernel trace,
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o speckle -- python3 tools/time_speckle.py --profile
(--profile: the matcher once, then only three filter calls with every output), and prints the mean time of k_spk_local, k_spk_border,
k_conn_flatten and k_spk_apply per launch from DIR's kernel_stats.csv.  --no-kernels leaves that step out."""
import csv, glob, os, shutil, statistics, subprocess, sys, tempfile
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from depth_completion_mt_amd import Context, sgm_workspace_bytes, synth
B, R, C, D, HELD = 64, 352, 1216, 64, 16
REPS = 5
KERNELS = ("k_spk_local", "k_spk_border", "k_conn_flatten", "k_spk_apply")
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
    print(f"{name}: {med:.3f} ms [{lo:.3f} .. {hi:.3f}], {med / B:.4f} ms a frame, {B / med * 1e3:.0f} frames/s")


with Context(0, R, C, B) as ctx:
    work = torch.empty(sgm_workspace_bytes(R, C, D, HELD), dtype=torch.uint8, device="cuda")
    d16 = torch.empty((B, R, C), dtype=torch.int16, device="cuda")
    depth = torch.empty((B, R, C), dtype=torch.float32, device="cuda")
    ctx.sgm_dev(left, right, d_disp16=d16, d_depth=depth, d_work=work, num_disparities=D)
    out = torch.empty_like(d16)
    depth_f = depth.clone()                                      # the filter's in-place plane: a second call stores the same zeros again
    removed = torch.empty((B,), dtype=torch.int32, device="cuda")
    if PROFILE:
        for _ in range(3):
            ctx.filter_speckles_dev(d16, d_depth=depth_f, d_out=out, d_removed=removed)
        torch.cuda.synchronize()
        sys.exit(0)
    scratch = torch.empty_like(d16)
    t = alternating({
        "plain": lambda: ctx.filter_speckles_dev(d16, d_out=out),
        "all": lambda: ctx.filter_speckles_dev(d16, d_depth=depth_f, d_out=out, d_removed=removed),
        "sgm": lambda: ctx.sgm_dev(left, right, d_disp16=d16, d_depth=depth, d_work=work, num_disparities=D),
        "copy": lambda: scratch.copy_(d16),
    })
    valid = int((d16 >= 0).sum())
    gone = int(removed.sum())
    assert gone == int((out != d16).sum()) and bool((depth_f[out != d16] == 0).all())
    print(f"--- {B} frames of {R} x {C} from sgm_dev at D = {D}; {valid / d16.numel():.3f} of the pixels valid, the filter (200, 32) removes "
          f"{gone} of them: {gone / max(valid, 1):.4f} of the valid, {gone / d16.numel():.4f} of all")
    line("filter_speckles_dev, disp16 only", t["plain"])
    line("filter_speckles_dev, disp16 + depth + removed", t["all"])
    line("sgm_dev, disp16 + depth", t["sgm"])
    line(f"device copy of the int16 planes ({2 * d16.numel() / 1e6:.1f} MB read, as much written)", t["copy"])
    print(f"filter / sgm_dev = {t['all'][0] / t['sgm'][0]:.4f} ({t['plain'][0] / t['sgm'][0]:.4f} disp16 only), filter / copy = "
          f"{t['all'][0] / t['copy'][0]:.1f} ({t['plain'][0] / t['copy'][0]:.1f} disp16 only)")


# ---- the four kernels, from a kernel trace of a child process (the context above is closed; the child opens its own) -----------------
if "--no-kernels" not in sys.argv[1:]:
    tracer = shutil.which("rocprofv3")
    if tracer is None:
        print("the four kernels: rocprofv3 not found, not measured")
        sys.exit(0)
    with tempfile.TemporaryDirectory() as outdir:
        r = subprocess.run([tracer, "--kernel-trace", "--stats", "--output-format", "csv", "-d", outdir, "-o", "speckle", "--", sys.executable,
                            os.path.abspath(__file__), "--profile"], capture_output=True, text=True, timeout=600)
        found = glob.glob(os.path.join(outdir, "**", "*kernel_stats.csv"), recursive=True)
        if r.returncode != 0 or not found:
            print(f"the four kernels: the traced run failed (status {r.returncode})\n{r.stderr[-2000:]}")
            sys.exit(1)
        with open(found[0], newline="") as f:
            rows = [row for row in csv.DictReader(f) if any(k in row["Name"] for k in KERNELS)]
    total = sum(float(row["AverageNs"]) for row in rows)
    for row in sorted(rows, key=lambda row: -float(row["AverageNs"])):
        name = row["Name"].split("dcmt::")[1].split("(")[0]
        print(f"{name}: {float(row['AverageNs']) / 1e6:.3f} ms a launch ({B} frames) [{float(row['MinNs']) / 1e6:.3f} .. {float(row['MaxNs']) / 1e6:.3f}], "
              f"{row['Calls']} launches, {float(row['AverageNs']) / total:.2f} of the four")
    print(f"the four together: {total / 1e6:.3f} ms a call")
