"""dcmt_rectify_map_dev, dcmt_rectify_dev and dcmt_rectify on the GPU, bit for bit against tests/rectify_restatement.py (the
definition of include/dcmt.h in numpy): the map of three records, the remap over batches, map counts, index tables, byte offsets
and both routes, the outside rules, one chain queued on a stream, and the host forms."""
import numpy as np
import pytest

import rectify_restatement as R
from depth_completion_mt_amd import _lib as L
from depth_completion_mt_amd import api

gpu = pytest.mark.gpu
ROWS, COLS = 37, 131                        # partial tiles in both directions, three tiles wide
SRC = (41, 150)
SMALL_K = np.array([[120.0, 0.0, 75.3], [0.0, 118.0, 20.6], [0.0, 0.0, 1.0]])
SMALL_P = np.array([[110.0, 0.0, 65.0], [0.0, 112.0, 18.2], [0.0, 0.0, 1.0]])
SMALL_D = np.array([-0.31, 0.12, 1.1e-3, -7e-4, -0.02])
_cache = {}


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.cpu().numpy()


def table9() -> np.ndarray:
    """Nine good records on the 41 x 150 source: record 0 of KITTI's magnitude (its view leaves the small source on the right), 1 a
    30 degree roll about the optical axis, the others smaller rolls with distortion and shifted cameras."""
    recs = [R.record(R.KITTI_K, R.KITTI_D, R.KITTI_R, R.KITTI_P), R.roll_record(30.0, SMALL_K, SMALL_P)]
    for i in range(2, 9):
        rec = R.roll_record(4.0 * i - 20.0, SMALL_K, SMALL_P)
        for k, v in zip(("k1", "k2", "p1", "p2", "k3"), SMALL_D):
            rec[k] = v * (0.5 + 0.1 * i)
        rec["cxp"] += 3.3 * i
        rec["cyp"] -= 1.7 * i
        recs.append(rec)
    return np.concatenate(recs)


def maps9() -> np.ndarray:
    """The restatement's maps of table9, computed once and shared (never modified)."""
    if "maps" not in _cache:
        _cache["maps"] = R.rectify_maps(table9(), ROWS, COLS)
    return _cache["maps"]


def frames(ch: int, b: int = 9) -> np.ndarray:
    key = ("frames", ch)
    if key not in _cache:
        _cache[key] = R.noise((9,) + SRC + ((3,) if ch == 3 else ()), 40 + ch)
    return _cache[key][:b]


@pytest.fixture(scope="module")
def ctx():
    with api.Context(0, 375, 1242, 9) as c:
        yield c


@gpu
def test_map_of_three_records(ctx):
    bad = R.record(R.KITTI_K, R.KITTI_D, R.KITTI_R, R.KITTI_P)
    bad["R"][0][4] = np.inf
    table = np.concatenate([table9()[:2], bad])
    want = R.rectify_maps(table, ROWS, COLS)
    assert (want[2] == R.OUTSIDE).all() and (want[:2] != R.OUTSIDE).all()
    got = host(ctx.rectify_map_dev(api.calib_to_device(table), ROWS, COLS))
    assert got.shape == (3, ROWS, COLS, 2) and got.dtype == np.int32
    assert np.array_equal(got, want)
    # every other way to an all-outside map, and elements that overflow one by one
    others = []
    for name, v in (("fx", np.nan), ("k3", -np.inf), ("cyp", np.inf), ("fxp", 0.0), ("fyp", -0.0)):
        rec = R.record(R.KITTI_K, R.KITTI_D, R.KITTI_R, R.KITTI_P)
        rec[name] = v
        others.append(rec)
    K = SMALL_K.copy()
    K[0, 0] = 1e300                          # finite, but all columns except the principal one land beyond 2^30
    others.append(R.record(K, np.zeros(5), np.eye(3), np.array([[110.0, 0, 65.0], [0, 112.0, 18.0], [0, 0, 1.0]])))
    others.append(R.roll_record(90.0, SMALL_K, np.array([[1e-3, 0, 65.0], [0, 1e-3, 18.0], [0, 0, 1.0]])))     # W stays 1, x and y are huge
    table = np.concatenate(others)
    want = R.rectify_maps(table, ROWS, COLS)
    assert (want[:5] == R.OUTSIDE).all() and (want[5] == R.OUTSIDE).any() and (want[5] != R.OUTSIDE).any()
    assert np.array_equal(host(ctx.rectify_map_dev(api.calib_to_device(table), ROWS, COLS)), want)
    assert np.array_equal(host(ctx.rectify_map_dev(api.calib_to_device(table9()), ROWS, COLS)), maps9())


@gpu
@pytest.mark.parametrize("force", [False, True], ids=["default", "gather"])
@pytest.mark.parametrize("ch", [1, 3], ids=["grey", "bgr"])
def test_remap_batches_maps_index_and_offsets(ctx, ch, force):
    import torch
    maps = maps9()
    d_maps = dev(maps)
    for b in (1, 2, 5, 9):
        src = frames(ch, b)
        d_src = dev(src)
        for n in sorted({1, 2, b}):
            got = host(ctx.rectify_dev(d_src, d_maps[:n].contiguous(), force_gather=force))
            want = R.rectify(src, maps[:n])
            assert got.shape == want.shape and np.array_equal(got, want), (b, n)
            assert want.any() and (want == 0).any()
    assert ("gather" if force else "lds") in ctx.last_path()
    # an index table with one bad index: that frame is zero, its neighbours are what they should be
    src = frames(ch, 5)
    d_maps4 = d_maps[:4].contiguous()
    for index in ([1, 0, 7, 1, 0], [3, -1, 3, 3, 2], [2, 2, 2, 2, -2**31], [0, 1, 2, 4, 3]):
        out = torch.full((5, ROWS, COLS) + ((3,) if ch == 3 else ()), 0xA5, dtype=torch.uint8, device="cuda")
        ctx.rectify_dev(dev(src), d_maps4, out=out, d_map_index=dev(np.array(index, np.int32)), force_gather=force)
        want = R.rectify(src, maps[:4], index=index)
        assert np.array_equal(host(out), want)
        assert sum(not want[f].any() for f in range(5)) == 1
    # d_src and d_dst at every byte offset
    src = frames(ch, 2)
    want = R.rectify(src, maps[:2])
    for so, do in ((1, 3), (2, 2), (3, 1), (0, 1), (1, 0)):
        sbuf = torch.zeros(src.size + 8, dtype=torch.uint8, device="cuda")
        dbuf = torch.full((want.size + 8,), 0xA5, dtype=torch.uint8, device="cuda")
        sbuf[so:so + src.size] = dev(src).reshape(-1)
        d_src, d_dst = sbuf[so:so + src.size].view(src.shape), dbuf[do:do + want.size].view(want.shape)
        assert d_src.data_ptr() % 4 == so and d_dst.data_ptr() % 4 == do
        ctx.rectify_dev(d_src, d_maps[:2].contiguous(), out=d_dst, force_gather=force)
        assert np.array_equal(host(d_dst), want), (so, do)
        edge = host(dbuf)
        assert (edge[:do] == 0xA5).all() and (edge[do + want.size:] == 0xA5).all()


@gpu
def test_routes_are_named_and_identical(ctx):
    # a minifying record: a tile's box is 40 times the tile, far beyond the LDS budget
    rows, cols = 20, 70
    K = np.array([[800.0, 0.0, 1300.0], [0.0, 800.0, 350.0], [0.0, 0.0, 1.0]])
    P = np.array([[20.0, 0.0, 33.0], [0.0, 20.0, 9.0], [0.0, 0.0, 1.0]])
    rec = R.record(K, np.zeros(5), np.eye(3), P)
    m = R.rectify_map(rec, rows, cols)
    src = R.noise((1, 800, 2800), 50)                                   # no box is cut short by the source: every tile overflows
    d_map = ctx.rectify_map_dev(api.calib_to_device(rec), rows, cols)
    assert np.array_equal(host(d_map)[0], m)
    got = host(ctx.rectify_dev(dev(src), d_map))
    assert ctx.last_path() == "k_rectify<gather>"
    assert np.array_equal(got, R.rectify(src, m[None])) and got.any()
    # KITTI's calibration at a full frame: every tile's box fits
    rec = R.record(R.KITTI_K, R.KITTI_D, R.KITTI_R, R.KITTI_P)
    m = R.rectify_map(rec, *R.KITTI_DST)
    d_map = ctx.rectify_map_dev(api.calib_to_device(rec), *R.KITTI_DST)
    assert np.array_equal(host(d_map)[0], m)
    for ch in (1, 3):
        src = R.noise((1,) + R.KITTI_SRC + ((3,) if ch == 3 else ()), 51 + ch)
        d_src = dev(src)
        got = host(ctx.rectify_dev(d_src, d_map))
        assert ctx.last_path() == "k_rectify<lds>"
        forced = host(ctx.rectify_dev(d_src, d_map, force_gather=True))
        assert ctx.last_path() == "k_rectify<gather>"
        assert np.array_equal(got, forced) and np.array_equal(got, R.rectify(src, m[None]))


@gpu
@pytest.mark.parametrize("force", [False, True], ids=["default", "gather"])
def test_outside_rules_and_adversarial_maps(ctx, force):
    import torch
    # a destination view wider than the source: zeros exactly where the restatement has them
    rec = R.record(SMALL_K, SMALL_D, np.eye(3), np.array([[60.0, 0, 65.0], [0, 60.0, 18.0], [0, 0, 1.0]]))
    m = R.rectify_map(rec, ROWS, COLS)
    src = frames(3, 2)
    want = R.rectify(src, m[None])
    assert (want.reshape(2, -1, 3).max(axis=(0, 2)) == 0).sum() > ROWS * COLS // 4 and want.any()
    assert np.array_equal(host(ctx.rectify_dev(dev(src), dev(m[None]), force_gather=force)), want)
    # adversarial elements among good ones, over guard-banded buffers: the destination and its guards are what the restatement
    # says, the source's guards are untouched, the call returns OK
    rng = np.random.default_rng(60)
    adv = np.array([-2**31, 2**31 - 1, 2**30, -2**30, -2**30 - 1, 2**30 + 31, -32, -1, 32 * SRC[1] - 1, 32 * SRC[1], 32 * SRC[0] - 33], np.int64)
    m = maps9()[2:4].copy()
    pick = rng.random(m.shape) < 0.3
    m[pick] = rng.choice(adv, size=int(pick.sum())).astype(np.int32)
    m[0, :16, :64] = np.array([-2**31, -2**31], np.int32)               # a whole tile outside
    m[1, 16:32, 64:128, 0] = 2**31 - 1
    for ch in (1, 3):
        src = frames(ch, 5)
        want = R.rectify(src, m)
        g = 4096
        sbuf = torch.full((src.size + 2 * g,), 0x5A, dtype=torch.uint8, device="cuda")
        dbuf = torch.full((want.size + 2 * g,), 0xA5, dtype=torch.uint8, device="cuda")
        sbuf[g:g + src.size] = dev(src).reshape(-1)
        ctx.rectify_dev(sbuf[g:g + src.size].view(src.shape), dev(m), out=dbuf[g:g + want.size].view(want.shape), force_gather=force)
        got, s_after = host(dbuf), host(sbuf)
        assert np.array_equal(got[g:g + want.size].reshape(want.shape), want)
        assert (got[:g] == 0xA5).all() and (got[g + want.size:] == 0xA5).all()
        assert (s_after[:g] == 0x5A).all() and (s_after[g + src.size:] == 0x5A).all() and np.array_equal(s_after[g:g + src.size], src.reshape(-1))
    # all of it outside: zeros
    out = host(ctx.rectify_dev(dev(frames(1, 2)), dev(np.full((1, ROWS, COLS, 2), -2**31, np.int32)), force_gather=force))
    assert out.shape == (2, ROWS, COLS) and not out.any()


@gpu
def test_refused_arguments_on_the_device(ctx):
    import torch
    lib = L.lib()
    src, mp, out = dev(frames(1, 2)), dev(maps9()[:2]), torch.zeros((2, ROWS, COLS), dtype=torch.uint8, device="cuda")
    idx = dev(np.zeros(2, np.int32))
    ok = lambda **kw: lib.dcmt_rectify_dev(ctx._h, kw.get("src", src.data_ptr()), kw.get("sr", SRC[0]), kw.get("sc", SRC[1]), kw.get("ch", 1),
                                           kw.get("mp", mp.data_ptr()), kw.get("n", 2), kw.get("idx", idx.data_ptr()), kw.get("flags", 0),
                                           kw.get("dst", out.data_ptr()), kw.get("rows", ROWS), kw.get("cols", COLS), kw.get("b", 2), None)
    assert ok() == L.OK
    for bad in (dict(src=None), dict(mp=None), dict(dst=None), dict(ch=2), dict(ch=4), dict(n=0), dict(flags=2), dict(flags=1 << 31), dict(sr=0),
                dict(sc=16385), dict(rows=376), dict(cols=1243), dict(b=10), dict(b=0), dict(mp=mp.data_ptr() + 4), dict(idx=idx.data_ptr() + 2),
                dict(dst=src.data_ptr() + 5), dict(dst=mp.data_ptr() + 16), dict(dst=idx.data_ptr())):
        assert ok(**bad) == L.E_INVALID, bad
    assert ok(idx=None) == L.OK
    table = api.calib_to_device(table9()[:2])
    okm = lambda **kw: lib.dcmt_rectify_map_dev(ctx._h, kw.get("t", table.data_ptr()), kw.get("n", 2), kw.get("rows", ROWS), kw.get("cols", COLS),
                                                kw.get("mp", mp.data_ptr()), None)
    assert okm() == L.OK
    for bad in (dict(t=None), dict(mp=None), dict(n=0), dict(t=table.data_ptr() + 4), dict(mp=mp.data_ptr() + 4), dict(rows=0), dict(cols=1243),
                dict(mp=table.data_ptr())):
        assert okm(**bad) == L.E_INVALID, bad
    torch.cuda.synchronize()


@gpu
def test_chain_queued_on_a_stream_equals_the_synchronised_chain(ctx):
    """rectify_dev -> bgr_convert_dev(gray=True) for both cameras, then sgm_dev, on a non-default stream behind other work, the inputs
    arriving on that stream too, with no host synchronisation between the calls."""
    import torch
    rows, cols, D = 48, 160, 32
    K = np.array([[150.0, 0.0, 90.2], [0.0, 149.0, 30.4], [0.0, 0.0, 1.0]])
    P = np.array([[140.0, 0.0, 80.0], [0.0, 140.0, 24.0], [0.0, 0.0, 1.0]])
    table = np.concatenate([R.roll_record(1.5, K, P), R.roll_record(-1.0, K, P)])
    table["k1"] = (-0.2, -0.18)
    rng = np.random.default_rng(70)
    base = rng.integers(0, 256, size=(60, 200 + 8, 3), dtype=np.uint8)
    base = np.repeat(np.repeat(base[::2, ::2], 2, axis=0), 2, axis=1)                       # some structure for the matcher
    pair = np.stack([base[:, 8:], base[:, :-8]])                                            # left, right: interleaved frames of two maps
    decoy = R.noise(pair.shape, 71)
    d_table = api.calib_to_device(table)

    def chain(d_in, stream):
        d_maps = ctx.rectify_map_dev(d_table, rows, cols, stream=stream)
        rect = ctx.rectify_dev(d_in, d_maps, stream=stream)
        grey = ctx.bgr_convert_dev(rect, lab=False, gray=True, stream=stream)
        return rect, ctx.sgm_dev(grey[0:1], grey[1:2], num_disparities=D, stream=stream)

    want_rect, want_disp = (host(t) for t in chain(dev(pair), None))
    torch.cuda.synchronize()
    assert np.array_equal(want_rect, R.rectify(pair, R.rectify_maps(table, rows, cols)))
    s = torch.cuda.Stream()
    d_in, d_real = dev(decoy), dev(pair)
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        busy = torch.zeros(1 << 26, dtype=torch.float32, device="cuda")
        for _ in range(8):
            busy.add_(1.0)                                                                  # work the chain has to queue behind
        d_in.copy_(d_real, non_blocking=True)
    rect, disp = chain(d_in, s.cuda_stream)
    with torch.cuda.stream(s):
        rect_c, disp_c = rect.clone(), disp.clone()
        d_in.copy_(dev(decoy), non_blocking=True)
    s.synchronize()
    assert np.array_equal(host(rect_c), want_rect) and np.array_equal(host(disp_c), want_disp)
    assert (want_disp >= 0).any()


@gpu
def test_host_forms_give_the_same_bytes(ctx):
    rec = table9()[3]
    K = np.array([[rec["fx"], 0, rec["cx"]], [0, rec["fy"], rec["cy"]], [0, 0, 1.0]])
    D = np.array([rec[k] for k in ("k1", "k2", "p1", "p2", "k3")])
    Rm = rec["R"].reshape(3, 3)
    P = np.array([[rec["fxp"], 0, rec["cxp"], 0.0], [0, rec["fyp"], rec["cyp"], 0.0], [0, 0, 1.0, 0.0]])
    for ch in (1, 3):
        src = frames(ch, 1)[0]
        want = R.remap(src, maps9()[3])
        assert np.array_equal(ctx.rectify(src, K, D, Rm, P, (ROWS, COLS)), want)
        wide = np.zeros((SRC[0], SRC[1] + 5) + src.shape[2:], np.uint8)                     # a pitched source
        wide[:, :SRC[1]] = src
        assert np.array_equal(ctx.rectify(wide[:, :SRC[1]], K, D, Rm, P, (ROWS, COLS)), want)
        assert np.array_equal(host(ctx.rectify(dev(src), K, D, Rm, P, (ROWS, COLS))), want)
        assert np.array_equal(api.undistort_rectify(src, K, D, Rm, P, (ROWS, COLS)), want)
        assert np.array_equal(host(api.undistort_rectify(dev(src), K, D, Rm, P, (ROWS, COLS))), want)
