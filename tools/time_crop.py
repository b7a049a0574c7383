"""dcmt_crop_frames_dev and dcmt_depth_to_u16_dev against what bounds them, on one device-resident workload: 1024 frames cycling
through the five KITTI sizes (375x1242, 370x1224, 374x1238, 370x1226, 376x1241), packed back to back, cropped to 352x1216 with the
default origins, once as uint16 and once as BGR; then 1024 dense f32 frames of 352x1216 exported to uint16.

The crop is timed against
    (a) a plain device-to-device copy of as many bytes as the crop writes -- the rate ceiling (it reads what it writes; the crop
        reads a little more: the aligned quads around each row), and
    (b) what the library offered before: one strided copy per frame, dst[f].copy_(view_f), all queued on the same stream;
the export against (a) on the bytes it moves, 4 read + 2 written per pixel.

One process, the candidates of a group alternating: REPS rounds, in every round each timed over `reps` back-to-back calls between
two events.  Per candidate the median and the range over the rounds, and the rate its bytes (read + written) make of the median."""
import os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from depth_completion_mt_amd import Context, api

B, R, C = 1024, 352, 1216
SIZES = [(375, 1242), (370, 1224), (374, 1238), (370, 1226), (376, 1241)]
REPS = 9


def timed(fn, reps):
    for _ in range(2): fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(); a.record()
    for _ in range(reps): fn()
    b.record(); torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def group(title, candidates):
    """candidates: [(name, fn, bytes moved, reps)]"""
    ms = {name: [] for name, *_ in candidates}
    for _ in range(REPS):
        for name, fn, _, reps in candidates:
            ms[name].append(timed(fn, reps))
    print(title)
    for name, _, moved, _ in candidates:
        v = ms[name]
        m = statistics.median(v)
        print(f"    {name}: {m:.4f} ms [{min(v):.4f} .. {max(v):.4f}], {moved / m / 1e9:.2f} TB/s of {moved / 1e6:.0f} MB read + written")
    return {name: statistics.median(v) for name, v in ms.items()}


def crop_group(ctx, elem, name):
    shapes = [SIZES[f % len(SIZES)] for f in range(B)]
    table = api.make_crop_table(shapes, (R, C), elem)
    src_bytes = int(table["offset"][-1]) + shapes[-1][0] * shapes[-1][1] * elem
    table = api.make_crop_table(shapes, (R, C), elem, src_bytes=src_bytes)
    d_src = torch.randint(0, 256, (src_bytes,), dtype=torch.uint8, device="cuda")
    d_table = api.calib_to_device(table)
    out_bytes = B * R * C * elem
    d_dst = torch.empty((B, R, C * elem), dtype=torch.uint8, device="cuda")
    d_ref = torch.empty_like(d_dst)
    d_flat = torch.empty((out_bytes,), dtype=torch.uint8, device="cuda")
    views = []
    for f, (r, c) in enumerate(shapes):
        frame = d_src[int(table["offset"][f]):int(table["offset"][f]) + r * c * elem].view(r, c * elem)
        y0, x0 = int(table["y0"][f]), int(table["x0"][f])
        views.append(frame[y0:y0 + R, x0 * elem:(x0 + C) * elem])

    def per_frame():
        for f in range(B):
            d_ref[f].copy_(views[f])

    def one_launch():
        ctx.crop_frames_dev(d_src, d_table, R, C, elem_bytes=elem, d_dst=d_dst)

    one_launch(); per_frame(); torch.cuda.synchronize()
    assert torch.equal(d_dst, d_ref), f"{name}: the crop and the per-frame copies differ"
    med = group(f"crop, {B} frames of the five KITTI sizes -> {R}x{C}, {name} ({elem} B per element)",
                [("dcmt_crop_frames_dev, one launch", one_launch, 2 * out_bytes, 10),
                 ("(a) plain copy of the output's bytes", lambda: d_flat.copy_(d_dst.view(-1)), 2 * out_bytes, 10),
                 (f"(b) {B} strided copies, one per frame", per_frame, 2 * out_bytes, 2)])
    one, a, b = med.values()
    print(f"    one launch / plain copy {one / a:.2f}, per-frame copies / one launch {b / one:.1f}")


def main():
    assert torch.cuda.is_available(), "no GPU: nothing is measured without one"
    with Context(0, R, C, B) as ctx:
        crop_group(ctx, 2, "uint16")
        crop_group(ctx, 3, "BGR")
        depth = torch.rand((B, R, C), dtype=torch.float32, device="cuda") * 90.0
        out = torch.empty((B, R, C), dtype=torch.int16, device="cuda")
        moved = 6 * B * R * C
        flat_in, flat_out = torch.empty((moved // 2,), dtype=torch.uint8, device="cuda"), torch.empty((moved // 2,), dtype=torch.uint8, device="cuda")
        ctx.depth_to_u16_dev(depth, 256.0, d_out=out); torch.cuda.synchronize()
        want = torch.round(depth * 256.0).clamp(0, 65535).to(torch.int32)
        assert torch.equal(out.to(torch.int32) & 0xffff, want), "the export differs from round(depth * 256)"
        med = group(f"export, {B} frames of {R}x{C}, f32 -> uint16",
                    [("dcmt_depth_to_u16_dev", lambda: ctx.depth_to_u16_dev(depth, 256.0, d_out=out), moved, 10),
                     ("(a) plain copy of 3 B/px (3 read + 3 written)", lambda: flat_out.copy_(flat_in), moved, 10)])
        one, a = med.values()
        print(f"    export / plain copy of the same bytes {one / a:.2f}")


if __name__ == "__main__":
    main()
