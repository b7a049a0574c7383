"""SLIC's two pixel renderings on the device: dcmt_slic_contours_dev / dcmt_slic_cluster_means_dev and their host forms, bit for bit
against the literal restatements of tests/contours_restatement.py (test_contours.py holds those against the closed form of
include/dcmt.h).  Masks, images and sums are integers: every comparison is exact.

Shapes.  The tiles are 64 x 64 pixels and the column pass takes 64 rows per step: 1 x 1, 1 x 70 and 70 x 1 (one row, one column),
65 x 9 and 130 x 3 (one row past a step, two steps and a bit; the alternating runs of test_contours.py cross row 64 and start at row
64 there), 67 x 133 (odd, 2 x 3 tiles); the pipeline's labels at 75 x 131 and 70 x 130."""
import numpy as np
import pytest

import contours_restatement as R
import test_gpu_stream_order as SO
from depth_completion_mt_amd import _lib as L
from depth_completion_mt_amd import api, synth

gpu = pytest.mark.gpu
i32, u8 = np.int32, np.uint8
MAX_ROWS, MAX_COLS, MAX_BATCH = 130, 133, 5
SIZES = [(1, 1), (1, 70), (70, 1), (65, 9), (130, 3), (67, 133)]
RED = (0, 0, 200)


@pytest.fixture(scope="module")
def ctx():
    c = api.Context(0, MAX_ROWS, MAX_COLS, MAX_BATCH)
    yield c
    c.close()


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.cpu().numpy()


_mask, _means = {}, {}


def want_mask(plane):
    """literal_contours(plane), computed once per plane and shared (never modified)."""
    key = (plane.shape, plane.tobytes())
    if key not in _mask:
        _mask[key] = R.literal_contours(plane)
        _mask[key].setflags(write=False)
    return _mask[key]


def want_means(plane, img, n):
    key = (plane.shape, plane.tobytes(), img.tobytes(), n)
    if key not in _means:
        _means[key] = R.literal_means(plane, img, n)
        for a in _means[key]:
            a.setflags(write=False)
    return _means[key]


def images(planes, seed=0):
    return np.stack([R.image_for(planes.shape[1], planes.shape[2], seed + f) for f in range(len(planes))])


def differ(got, want, what):
    neq = got != want
    assert got.shape == want.shape and got.dtype == want.dtype, what
    assert not neq.any(), f"{what}: {int(neq.sum())} elements differ, first at {tuple(np.argwhere(neq)[0])}"


def check_contours(ctx, planes, what, colour=RED):
    """One device call with both outputs on the batch `planes` against the literal restatement of every frame; returns (image, mask)."""
    planes = np.ascontiguousarray(planes, i32)
    img = images(planes)
    d_bgr, d_mask = ctx.slic_contours_dev(dev(planes), dev(img), colour, dev(np.full(planes.shape, 0xA5, u8)))
    bgr, mask = host(d_bgr), host(d_mask)
    for f in range(len(planes)):
        m = want_mask(planes[f])
        differ(mask[f], m, f"{what} frame {f}: mask")
        differ(bgr[f], R.paint(img[f], m, colour), f"{what} frame {f}: image")
    return bgr, mask


def check_means(ctx, planes, n, what, sums=True, img=None):
    planes = np.ascontiguousarray(planes, i32)
    img = images(planes, 50) if img is None else img
    d_bgr, d_sums = ctx.slic_cluster_means_dev(dev(planes), n, dev(img), True if sums else None)
    bgr = host(d_bgr)
    assert (d_sums is None) == (not sums)
    for f in range(len(planes)):
        out, s = want_means(planes[f], img[f], n)
        differ(bgr[f], out, f"{what} frame {f}: image")
        if sums:
            differ(host(d_sums)[f], s, f"{what} frame {f}: sums")
    return bgr


def slic_planes(rows, cols, step, b=2, nc=40):
    """What slic_labels_dev makes of synthetic Lab images, raw and behind slic_connectivity_dev: (raw, connected, n_centers, max_labels)."""
    lab = np.stack([synth.synth_lab(rows, cols, 40 + f) for f in range(b)])
    with api.Context(0, rows, cols, b) as c:
        labels, n = c.slic_labels_dev(dev(lab), step, nc)
        raw = host(labels)
        conn, max_labels, _ = c.slic_connectivity_dev(labels, n)
        return raw, host(conn), n, max_labels


# ------------------------------------------------------------------------------------------------------------- against the restatement
@gpu
@pytest.mark.parametrize("rows,cols", SIZES)
def test_shapes_batch_3_different_frames(ctx, rows, cols):
    cases = R.plane_cases(rows, cols)
    assert {c[0].split()[0] for c in cases} == set(R.PLANES)
    adversarial = np.stack([p for _, p in cases])
    check_contours(ctx, adversarial[:3], f"adversarial {rows}x{cols} (rows, hstripes, checkerboard)")
    check_contours(ctx, adversarial[3:], f"adversarial {rows}x{cols} (vstripes, constant, outofrange)", colour=(1, 255, 77))
    check_contours(ctx, np.stack([R.noise(rows, cols, nv, 90 + nv) for nv in (2, 3, 50)]), f"noise {rows}x{cols}")
    check_means(ctx, adversarial[[0, 3, 5]], 6, f"means {rows}x{cols}, 6 labels")
    check_means(ctx, np.stack([R.noise(rows, cols, 50, 7), R.voronoi(rows, cols), R.out_of_range(rows, cols, 40)]), 40, f"means {rows}x{cols}, 40 labels")


@gpu
@pytest.mark.parametrize("rows,cols,step", [(75, 131, 7), (70, 130, 16)])
def test_labels_of_the_pipeline(rows, cols, step):
    raw, conn, n, max_labels = slic_planes(rows, cols, step)
    assert max_labels == api.slic_connectivity_max_labels(rows, cols, n) and raw.max() < n and conn.max() < max_labels
    with api.Context(0, rows, cols, 2) as c:
        _, mask = check_contours(c, raw, f"slic {rows}x{cols} step {step}, raw")
        _, mask2 = check_contours(c, conn, f"slic {rows}x{cols} step {step}, connected")
        check_means(c, raw, n, "means on raw labels")
        check_means(c, conn, max_labels, "means on connected labels, n_labels = slic_connectivity_max_labels")
        check_means(c, conn, max_labels, "means without d_sums", sums=False)
    print(f"[contours] slic {rows}x{cols} step {step}: {n} centres, max_labels {max_labels}; taken {[(m != 0).mean().round(3) for m in mask]} raw, "
          f"{[(m != 0).mean().round(3) for m in mask2]} connected")


@gpu
def test_labels_far_apart_in_one_tile(ctx):
    """More than kMeansSlots = 512 labels between a tile's smallest and largest: the sums that bypass the LDS table."""
    planes = np.stack([R.noise(67, 133, 4000, 3), R.noise(67, 133, 4000, 4) * (R.checkerboard(67, 133) * 2 - 1)]).astype(i32)
    assert planes[0].max() - planes[0].min() > 3000 and (planes[1] < 0).sum() > 3000
    check_means(ctx, planes, 4000, "4000 labels")
    check_means(ctx, planes, 700, "4000 labels of which 700 are in range")


# ------------------------------------------------------------------------------------------------------------- properties of the call
def five_planes(rows=67, cols=133):
    return np.stack([R.noise(rows, cols, 3, 7), R.rows_own_label(rows, cols), R.out_of_range(rows, cols), R.voronoi(rows, cols), R.checkerboard(rows, cols)])


@gpu
def test_outputs_batch_position_and_repetition(ctx):
    planes = five_planes()
    img = images(planes)
    bgr, mask = check_contours(ctx, planes, "batch of 5")
    # mask only, image only: the same bits as both
    _, m = ctx.slic_contours_dev(dev(planes))
    differ(host(m), mask, "mask only")
    b, none = ctx.slic_contours_dev(dev(planes), dev(img), RED)
    assert none is None
    differ(host(b), bgr, "image only")
    # a frame alone against its position in the batch; another order
    for f in range(5):
        b1, m1 = ctx.slic_contours_dev(dev(planes[f]), dev(img[f]), RED, dev(np.zeros(planes[f].shape, u8)))
        differ(host(b1), bgr[f], f"frame {f} alone: image")
        differ(host(m1), mask[f], f"frame {f} alone: mask")
    order = [4, 2, 0, 3, 1]
    _, m = ctx.slic_contours_dev(dev(planes[order]))
    differ(host(m), mask[order], f"batch in order {order}")
    # a repeated call on the same buffers: identical bits (painting a painted image changes nothing)
    d_lab, d_bgr, d_mask = dev(planes), dev(img), dev(np.zeros(planes.shape, u8))
    for k in range(3):
        ctx.slic_contours_dev(d_lab, d_bgr, RED, d_mask)
        differ(host(d_bgr), bgr, f"call {k}: image")
        differ(host(d_mask), mask, f"call {k}: mask")
    # the means: alone against the batch, repeated out of the same inputs
    means = check_means(ctx, planes, 6, "means, batch of 5")
    for f in (1, 4):
        differ(check_means(ctx, planes[f][None], 6, f"means, frame {f} alone", img=images(planes, 50)[f][None])[0], means[f], f"means frame {f} alone")
    differ(check_means(ctx, planes, 6, "means again"), means, "means again")


@gpu
def test_host_entry_points_and_module_level_calls(ctx):
    plane = R.out_of_range(67, 133)
    img = R.image_for(67, 133, 4)
    m = want_mask(plane)
    got, mask = ctx.slic_contours(plane, img, (9, 8, 7))
    differ(mask, m, "host mask")
    differ(got, R.paint(img, m, (9, 8, 7)), "host image")
    none, mask = ctx.slic_contours(plane)
    assert none is None
    differ(mask, m, "host mask alone")
    wide = np.full((67, 140), 5, i32)
    wide[:, :133] = plane
    differ(ctx.slic_contours(wide[:, :133], img)[0], R.paint(img, m), "pitched labels")
    differ(api.slic_display_contours(plane, img), R.paint(img, m), "slic_display_contours")
    pitched = np.zeros((67, 500), u8)
    pitched[:, :399] = img.reshape(67, 399)
    assert L.lib().dcmt_slic_contours(ctx._h, plane.ctypes.data, 133 * 4, 67, 133, pitched.ctypes.data, 500, bytes(RED), None, 0) == L.OK    # image only, pitched, in place
    differ(pitched[:, :399].reshape(67, 133, 3), R.paint(img, m), "image only, pitched")
    assert (pitched[:, 399:] == 0).all()
    out, sums = want_means(plane, img, 6)
    got, s = ctx.slic_cluster_means(plane, img, 6)
    differ(got, out, "host means")
    differ(s, sums, "host sums")
    differ(api.slic_colour_with_cluster_means(plane, img, 6), out, "slic_colour_with_cluster_means")
    h = img.copy()
    assert L.lib().dcmt_slic_cluster_means(ctx._h, plane.ctypes.data, 133 * 4, 67, 133, 6, h.ctypes.data, 399, None) == L.OK          # no sums
    differ(h, out, "host means without sums")


# ------------------------------------------------------------------------------------------------------------- stream order
def stream_case(rows=40, cols=56, b=3, n_labels=9):
    """Both calls and, behind them on the same context, the labelled completion that reads the same labels."""
    def inputs(which):
        g = np.random.Generator(np.random.PCG64(31 + which))
        return {"labels": SO.salt_and_pepper(g, (b, rows, cols)), "bgr": g.integers(0, 256, (b, rows, cols, 3), dtype=u8),
                "img2": g.integers(0, 256, (b, rows, cols, 3), dtype=u8), "sparse": SO.sparse_frames(b, rows, cols, 400 + 50 * which)}

    def params():
        return api.make_params(spec_fill_iters=SO.SPEC)

    def call(ctx, t, st):
        ctx.slic_contours_dev(t["labels"], t["bgr"], RED, t["mask"], stream=st)
        ctx.slic_cluster_means_dev(t["labels"], n_labels, t["img2"], t["sums"], stream=st)
        ctx.complete_dev(t["sparse"], t["dense"], params(), d_labels=t["labels"], n_labels=n_labels, stream=st)

    def wrap(ctx, t, st):
        with api._on_stream(st, t["labels"]):
            img = t["img2"].clone()                              # the means work in place: every call its own copy of the input
        _, mask = ctx.slic_contours_dev(t["labels"], stream=st)
        _, sums = ctx.slic_cluster_means_dev(t["labels"], n_labels, img, True, stream=st)
        return {"mask": mask, "sums": sums}

    def expect(inp):
        mask = np.stack([want_mask(x) for x in inp["labels"]])
        means = [want_means(inp["labels"][f], inp["img2"][f], n_labels) for f in range(b)]
        dense = []
        for f in range(b):
            y, info = SO.O().interpolate_with_superpixels(inp["sparse"][f], inp["labels"][f], n_labels, return_info=True)
            assert info["rc"] == 0 and info["fill_iters"] < SO.SPEC
            dense.append(y)
        return {"bgr": np.stack([R.paint(inp["bgr"][f], mask[f], RED) for f in range(b)]), "mask": mask, "img2": np.stack([m[0] for m in means]),
                "sums": np.stack([m[1] for m in means]), "dense": np.stack(dense)}

    outs = {"bgr": SO.Out((b, rows, cols, 3), u8), "mask": SO.Out((b, rows, cols), u8), "img2": SO.Out((b, rows, cols, 3), u8),
            "sums": SO.Out((b, n_labels, 4), i32), "dense": SO.Out((b, rows, cols), np.float32)}
    return SO.Case("slic_contours + slic_cluster_means + complete labeled", (rows, cols, b), inputs, outs, call, expect, None, wrap)


@gpu
def test_queued_behind_other_work_on_a_stream():
    """The scheme of tests/test_gpu_stream_order.py: behind a delay on a non-default stream, producer copies, the two calls, a
    labelled completion on the same context and the consumer copies with no host synchronisation between them; the clones hold the
    restatements' and the oracle's bits, so nothing blocked, nothing escaped to the null stream and the completion was not disturbed."""
    SO.run_ordered(stream_case())


@gpu
def test_wrapper_creates_its_outputs_on_the_stream_it_enqueues_on():
    case = stream_case()
    SO.cases()[case.name] = case                             # that test looks its case up by name
    try:
        SO.test_wrapper_creates_its_output_on_the_stream_it_enqueues_on(case.name)
    finally:
        del SO.cases()[case.name]


# ------------------------------------------------------------------------------------------------------------- refusals
@gpu
def test_refusals(ctx):
    import torch
    lib = L.lib()
    r, c, b = 8, 16, 3
    n = r * c * b
    buf = torch.zeros(8 * n, dtype=torch.uint8, device="cuda")
    lab, bgr, mask = torch.zeros(n, dtype=torch.int32, device="cuda"), torch.full((3 * n,), 7, dtype=torch.uint8, device="cuda"), torch.full((n,), 7, dtype=torch.uint8, device="cuda")
    sums = torch.full((b * 4 * 4,), -7, dtype=torch.int32, device="cuda")
    red = bytes(RED)
    P = lambda t, off=0: t.data_ptr() + off

    def cont(l=P(lab), i=P(bgr), m=P(mask), col=red, rows=r, cols=c, batch=b, h=ctx._h):
        return lib.dcmt_slic_contours_dev(h, l, rows, cols, batch, i, col, m, None)

    def mean(l=P(lab), i=P(bgr), s=P(sums), nl=4, rows=r, cols=c, batch=b, h=ctx._h):
        return lib.dcmt_slic_cluster_means_dev(h, l, rows, cols, batch, nl, i, s, None)

    assert cont() == L.OK and cont(i=None) == L.OK and cont(m=None) == L.OK and mean() == L.OK and mean(s=None) == L.OK
    torch.cuda.synchronize()
    assert (host(mask) == 0).all() and (host(bgr) == 7).all()                    # one label: nothing taken, the mean of sevens is seven
    assert host(sums).reshape(b, 4, 4).tolist() == [[[7 * r * c] * 3 + [r * c]] + [[0] * 4] * 3] * b
    bad = [cont(l=None), cont(i=None, m=None), cont(col=None), cont(l=P(lab, 2)),
           cont(l=P(buf), i=P(buf, 4 * n - 1)), cont(l=P(buf, 64), i=P(buf), m=None), cont(l=P(buf), m=P(buf, 4 * n - 1)), cont(l=P(buf, 64), m=P(buf, 63)),
           cont(i=P(buf), m=P(buf, 3 * n - 1)), cont(i=P(buf, 8), m=P(buf)),
           cont(rows=MAX_ROWS + 1), cont(cols=MAX_COLS + 1), cont(batch=MAX_BATCH + 1), cont(rows=0), cont(cols=0), cont(batch=0), cont(h=None),
           mean(l=None), mean(i=None), mean(l=P(lab, 2)), mean(s=P(sums, 2)), mean(nl=0), mean(nl=-4),
           mean(nl=MAX_ROWS * MAX_COLS * MAX_BATCH // (4 * b) + 1), mean(nl=MAX_ROWS * MAX_COLS * MAX_BATCH // (4 * b) + 1, s=None),
           mean(l=P(buf), i=P(buf, 4 * n - 1)), mean(l=P(buf, 64), i=P(buf)), mean(s=P(lab, 4 * n - 4)), mean(s=P(bgr, 8)),
           mean(rows=MAX_ROWS + 1), mean(cols=MAX_COLS + 1), mean(batch=MAX_BATCH + 1), mean(rows=0), mean(batch=0), mean(h=None)]
    assert bad == [L.E_INVALID] * len(bad), bad
    assert cont(l=P(buf), i=P(buf, 4 * n), m=None) == L.OK and cont(i=P(buf), m=P(buf, 3 * n)) == L.OK     # touching is no overlap
    assert mean(nl=MAX_ROWS * MAX_COLS * MAX_BATCH // (4 * b), s=None) == L.OK                              # the bound itself
    torch.cuda.synchronize()
    # the host forms
    hl, hi, hm = np.zeros((r, c), i32), np.full((r, c, 3), 7, u8), np.full((r, c), 7, u8)
    one = lambda *a: lib.dcmt_slic_contours(ctx._h, *a)
    assert one(hl.ctypes.data, c * 4, r, c, hi.ctypes.data, c * 3, red, hm.ctypes.data, c) == L.OK and (hm == 0).all() and (hi == 7).all()
    bad = [one(None, c * 4, r, c, hi.ctypes.data, c * 3, red, hm.ctypes.data, c), one(hl.ctypes.data, c * 4, r, c, None, 0, red, None, 0),
           one(hl.ctypes.data, c * 4, r, c, hi.ctypes.data, c * 3, None, hm.ctypes.data, c), one(hl.ctypes.data, c * 4 - 4, r, c, hi.ctypes.data, c * 3, red, hm.ctypes.data, c),
           one(hl.ctypes.data, c * 4, r, c, hi.ctypes.data, c * 3 - 1, red, hm.ctypes.data, c), one(hl.ctypes.data, c * 4, r, c, hi.ctypes.data, c * 3, red, hm.ctypes.data, c - 1),
           one(hl.ctypes.data, c * 4, MAX_ROWS + 1, c, hi.ctypes.data, c * 3, red, hm.ctypes.data, c)]
    assert bad == [L.E_INVALID] * len(bad), bad
    two = lambda *a: lib.dcmt_slic_cluster_means(ctx._h, *a)
    hs = np.full((4, 4), -7, i32)
    assert two(hl.ctypes.data, c * 4, r, c, 4, hi.ctypes.data, c * 3, hs.ctypes.data) == L.OK and hs[0].tolist() == [7 * r * c] * 3 + [r * c]
    bad = [two(None, c * 4, r, c, 4, hi.ctypes.data, c * 3, hs.ctypes.data), two(hl.ctypes.data, c * 4, r, c, 4, None, c * 3, hs.ctypes.data),
           two(hl.ctypes.data, c * 4, r, c, 0, hi.ctypes.data, c * 3, hs.ctypes.data), two(hl.ctypes.data, c * 4, r, c, 1 << 30, hi.ctypes.data, c * 3, None),
           two(hl.ctypes.data, c * 4 - 4, r, c, 4, hi.ctypes.data, c * 3, hs.ctypes.data), two(hl.ctypes.data, c * 4, r, c, 4, hi.ctypes.data, c * 3 - 1, hs.ctypes.data),
           two(hl.ctypes.data, c * 4, r, MAX_COLS + 1, 4, hi.ctypes.data, c * 3, hs.ctypes.data)]
    assert bad == [L.E_INVALID] * len(bad), bad
    with pytest.raises(api.DcmtError) as e:
        ctx.slic_cluster_means_dev(dev(np.zeros((1, r, c), i32)), 0, dev(np.zeros((1, r, c, 3), u8)))
    assert e.value.status == L.E_INVALID
