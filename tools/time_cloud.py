"""Back-projection and the unmasked Gaussian on the device (dcmt_depth_to_cloud_dev, dcmt_gaussian5_dev, 352x1216): call times at 1024
frames and at batch 1, the bytes the kernels move by the formula of dcmt_kernels_cloud.h -- 4 (count) + 4 (re-read) + 3 (colour) +
16 * v per pixel, v = the share of pixels with depth > 0 taken from the offsets the call returned; the Gaussian 8 B/px (+ 8 for the
copy of an in-place call) -- and that over 8 TB/s.  colorize_dev on the same planes runs alternating with them in the same process
as the comparison (its own 11 B/px).  Medians of REPS alternating repetitions, with the range.  Last: one complete + gaussian5 +
depth_to_cloud step against complete alone on the same stream."""
import os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from depth_completion_mt_amd import Context, make_params, synth
B, R, C = 1024, 352, 1216
REPS = 7
frames = synth.synth_batch(32, R, C, 0)
src = torch.from_numpy(frames).cuda().repeat(B // 32, 1, 1).contiguous()
bgr = torch.randint(0, 256, (B, R, C, 3), dtype=torch.uint8, device="cuda")
out = torch.empty((B, R, C, 3), dtype=torch.uint8, device="cuda")
pts = torch.empty((B * R * C, 4), dtype=torch.float32, device="cuda")
off = torch.empty((B + 1,), dtype=torch.int32, device="cuda")
p = make_params()


def timed(fn, reps=10):
    for _ in range(3): fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(); a.record()
    for _ in range(reps): fn()
    b.record(); torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def alternating(cases, reps_of=None):
    """cases: {name: fn}; REPS rounds, every case once per round in turn.  Returns {name: (median, min, max)} in ms."""
    ms = {k: [] for k in cases}
    for _ in range(REPS):
        for k, fn in cases.items():
            ms[k].append(timed(fn, (reps_of or {}).get(k, 10)))
    return {k: (statistics.median(v), min(v), max(v)) for k, v in ms.items()}


def line(name, t, bytes_moved, note=""):
    med, lo, hi = t
    rate = bytes_moved / (med * 1e-3)
    print(f"{name}: {med:.4f} ms [{lo:.4f} .. {hi:.4f}], {bytes_moved / 1e9:.3f} GB stated -> {rate / 1e12:.2f} TB/s = {rate / 8e12:.3f} of 8 TB/s{note}")


def cloud_bytes(n_frames, total, colour):
    return n_frames * R * C * (8 + (3 if colour else 0)) + 16 * total


with Context(0, R, C, B) as ctx:
    dense = ctx.complete_dev(src, params=p)
    blurred = torch.empty_like(dense)
    scratch = dense.clone()
    for n in (B, 1):
        d, s, c, o = dense[:n], src[:n], bgr[:n], out[:n]
        ctx.depth_to_cloud_dev(d, c, d_points=pts, d_offsets=off[:n + 1])
        v_dense = int(off[n].item())
        ctx.depth_to_cloud_dev(s, c, d_points=pts, d_offsets=off[:n + 1])
        v_sparse = int(off[n].item())
        t = alternating({
            "cloud dense colour": lambda: ctx.depth_to_cloud_dev(d, c, d_points=pts, d_offsets=off[:n + 1]),
            "colorize dense": lambda: ctx.colorize_dev(d, d_bgr=o),
            "cloud dense no colour": lambda: ctx.depth_to_cloud_dev(d, None, d_points=pts, d_offsets=off[:n + 1]),
            "cloud sparse colour": lambda: ctx.depth_to_cloud_dev(s, c, d_points=pts, d_offsets=off[:n + 1]),
            "colorize sparse": lambda: ctx.colorize_dev(s, d_bgr=o),
            "gaussian5": lambda: ctx.gaussian5_dev(d, d_dst=blurred[:n]),
            "gaussian5 in place": lambda: ctx.gaussian5_dev(scratch[:n], d_dst=scratch[:n]),
        }, None if n == B else {k: 100 for k in ("cloud dense colour", "colorize dense", "cloud dense no colour", "cloud sparse colour",
                                                   "colorize sparse", "gaussian5", "gaussian5 in place")})
        px = n * R * C
        print(f"--- {n} frame(s) of {R} x {C}; v = {v_dense / px:.4f} (dense), {v_sparse / px:.4f} (sparse)")
        line("depth_to_cloud_dev, dense, colour", t["cloud dense colour"], cloud_bytes(n, v_dense, True))
        line("depth_to_cloud_dev, dense, no colour", t["cloud dense no colour"], cloud_bytes(n, v_dense, False))
        line("depth_to_cloud_dev, sparse, colour", t["cloud sparse colour"], cloud_bytes(n, v_sparse, True))
        line("colorize_dev, dense (11 B/px)", t["colorize dense"], 11 * px)
        line("colorize_dev, sparse (11 B/px)", t["colorize sparse"], 11 * px)
        line("gaussian5_dev, out of place (8 B/px)", t["gaussian5"], 8 * px)
        line("gaussian5_dev, in place (8 B/px + the copy's 8)", t["gaussian5 in place"], 16 * px)
    dst = torch.empty_like(src)
    t = alternating({
        "complete": lambda: ctx.complete_dev(src, dst, p),
        "chain": lambda: (ctx.complete_dev(src, dst, p), ctx.gaussian5_dev(dst, d_dst=dst),
                          ctx.depth_to_cloud_dev(dst, bgr, d_points=pts, d_offsets=off)),
    })
    a, b = t["complete"], t["chain"]
    print(f"step, {B} frames: complete {a[0]:.3f} ms [{a[1]:.3f} .. {a[2]:.3f}] ({B / a[0] * 1e3:.0f} frames/s); complete + gaussian5 (in place) "
          f"+ depth_to_cloud {b[0]:.3f} ms [{b[1]:.3f} .. {b[2]:.3f}] ({B / b[0] * 1e3:.0f} frames/s, +{(b[0] / a[0] - 1) * 100:.1f} %)")
