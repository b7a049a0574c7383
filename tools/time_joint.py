"""The joint bilateral filter on the device (1024 frames of 352x1216): joint_bilateral_dev on a completed synth.synth_batch cut back by
support_distance_dev at its default radius (so the holes are the pixels further than 9 from a return: the upper third and the gaps),
with a grey and with a three-channel guide, FILL alone and FILL | SMOOTH, at R = 3 and R = 9 (tables of make_joint_tables at that
radius and its default sigmas), against bilateral5_dev and support_distance_dev on the same planes and against plain device copies of
the call's stated bytes (4 + channels read, 4 written per pixel), in one alternating session.  Medians of REPS alternating repetitions
in one process, with the range.  The guide is synthetic: flat regions with edges and integer noise, the same 32 frames repeated; no
real camera frame is timed here.
    python3 tools/time_joint.py [--frames B]"""
import os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np, torch  # noqa: E402
from depth_completion_mt_amd import Context, calib_to_device, make_joint_tables, make_params, synth  # noqa: E402
B = int(sys.argv[sys.argv.index("--frames") + 1]) if "--frames" in sys.argv else 1024
R, C = 352, 1216
REPS, INNER = 7, 3


def timed(fn):
    for _ in range(1): fn()
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


def guide_frames(n, channels):
    """Camera-like frames: flat regions with edges, a ramp and integer noise."""
    g = np.random.Generator(np.random.PCG64(7))
    V, U = np.mgrid[0:R, 0:C]
    out = []
    for f in range(n):
        region = ((U // (37 + f % 5) + V // 23) % 5) * 40 + 30 + (U % 11)
        planes = [np.clip(region * (1.0 + 0.15 * k) + g.integers(-3, 4, (R, C)) + 9 * k, 0, 255).astype(np.uint8) for k in range(channels)]
        out.append(planes[0] if channels == 1 else np.stack(planes, axis=2))
    return np.stack(out)


with Context(0, R, C, B) as ctx:
    rep = B // 32 if B >= 32 else 1
    n0 = min(B, 32)
    sparse = torch.from_numpy(synth.synth_batch(n0, R, C, 0)).cuda().repeat(rep, 1, 1).contiguous()
    dense = ctx.complete_dev(sparse, None, make_params())
    cut, beyond = ctx.support_distance_dev(sparse, dense, beyond=True)
    del dense
    grey = torch.from_numpy(guide_frames(n0, 1)).cuda().repeat(rep, 1, 1).contiguous()
    bgr = torch.from_numpy(guide_frames(n0, 3)).cuda().repeat(rep, 1, 1, 1).contiguous()
    out, scratch = torch.empty_like(cut), torch.empty_like(cut)
    px = B * R * C
    share = float(beyond[:n0].double().mean()) / (R * C)
    torch.cuda.synchronize()
    print(f"--- {B} frames of {R} x {C}: holes (beyond 9 of a return) {share:.4f} of the pixels")
    tabs = {r: calib_to_device(make_joint_tables(r)) for r in (3, 9)}
    cases, filled = {}, {}
    for r in (3, 9):
        for name, guide in (("grey", grey), ("bgr", bgr)):
            for smooth in (False, True):
                key = f"R {r} {name} {'FILL | SMOOTH' if smooth else 'FILL'}"
                cases[key] = lambda r=r, guide=guide, smooth=smooth: ctx.joint_bilateral_dev(cut, guide, tabs[r], d_out=out, radius=r, smooth=smooth)
                _, n = ctx.joint_bilateral_dev(cut, guide, tabs[r], d_out=out, counts=True, radius=r, smooth=smooth)
                filled[key] = float(n[:n0, 0].double().mean()) / (R * C)
    cases["bilateral5"] = lambda: ctx.bilateral5_dev(cut, scratch)
    cases["support"] = lambda: ctx.support_distance_dev(sparse, cut, d_out=scratch)
    cases["copy9"] = copier(9 * px)
    cases["copy11"] = copier(11 * px)
    t = alternating(cases)
    for key in filled:
        ch = 1 if "grey" in key else 3
        line(f"joint_bilateral_dev {key} (fills {filled[key]:.4f} of the pixels)", t[key], (8 + ch) * px)
    line("bilateral5_dev", t["bilateral5"], 8 * px)
    line("support_distance_dev trust mask out of place, R = 9", t["support"], 12 * px)
    line("device copy (9 B/px)", t["copy9"], 9 * px)
    line("device copy (11 B/px)", t["copy11"], 11 * px)
    for key in filled:
        copy = t["copy9" if "grey" in key else "copy11"][0]
        print(f"{key}: / its copy = {t[key][0] / copy:.2f}, / bilateral5_dev = {t[key][0] / t['bilateral5'][0]:.2f}, / support_distance_dev = {t[key][0] / t['support'][0]:.2f}")
