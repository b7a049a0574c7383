"""In-place and overlapping device calls (include/dcmt.h, "In place"): d_dst == d_src, or d_dst shifted against d_src by a frame,
a row or one element, on every completion entry point (f32, uint16, labeled), dispatch path and stop_after stage.  Every cell is
compared bit for bit with the oracle run on a host copy of the input, and asserts the kernels the library reports (dcmt_last_path),
so that no cell tests another path than it names.  The cells in which one kernel both reads the frames and writes the probe run on
16 frames of 352 x 1216: thousands of workgroups, far more than the GPU holds at once, so a read-after-write race between them
cannot hide.  Every cell runs once; a test reports all of its failing cells, not only the first."""
import concurrent.futures
import ctypes

import numpy as np
import pytest

from conftest import assert_bit_equal
from depth_completion_mt_amd import _lib as L
from depth_completion_mt_amd import api, synth
from test_gpu_fuzz import _frame, _grid_frame, _labels

pytestmark = pytest.mark.gpu

R, C, B = 352, 1216, 16
FILL = 16                                   # max_fill_iters == spec_fill_iters: the device result is complete
LAYOUTS = ("same", "dst one frame behind", "dst one frame ahead", "dst one row ahead", "dst one element ahead", "dst one element behind")
STAGES = range(L.STAGE_INVERT, L.STAGE_FINAL + 1)

_POOL = concurrent.futures.ThreadPoolExecutor(8)    # the oracle's C calls release the GIL


@pytest.fixture(scope="module")
def O():
    from oracle import oracle
    return oracle


def _full_frames(cols=C, seed=820):
    f = synth.synth_batch(B, R, cols, seed)           # depths on the 1/256 m grid
    f[3, 150:230] = 0                                 # a gap the 31x31 fill closes in three applications: the hole-closure loop runs
    f[5, 120:170, 400:520] = 0
    f[7] = 0                                          # an empty frame
    f[9, :, : cols // 2] = 0                          # left half empty
    return f


def _full_labels():
    """SLIC-like labels, a band of labels 400 columns wide (the label stage walks boxes wider than a wave in column chunks) and
    unlabeled pixels"""
    lab, n = synth.synth_labels(R, C, 1200, 5)
    lab[:, 300:700] = n + np.arange(R)[:, None] // 90
    n += (R + 89) // 90
    lab[np.random.Generator(np.random.PCG64(5)).random((R, C)) < 0.03] = -1
    return lab.astype(np.int32), n


_CACHE = {}


def _oracle(O, frames, stop, k0="as_compiled", blur="gaussian", norm=None, labels=None, n_labels=0, key=None):
    """(outputs, fill_iters) of every frame; fill_iters -1 where the loop hit FILL (what dcmt_last_fill_iters reports).
    key: names the frames (and labels): the result is kept for every later test that asks for the same"""
    ck = (key, stop, k0, blur, norm, n_labels)
    if key is not None and ck in _CACHE:
        return _CACHE[ck]
    op = O.default_params(k0=k0, blur=blur, stop_after=max(stop, L.STAGE_INVERT), max_fill_iters=FILL)

    def one(x):
        if norm is not None:
            x = O.normalize_minmax(x, *norm)
        if stop == L.STAGE_NORMALIZE:
            return x, 0
        if labels is None:
            y, info = O.img_completion(x, op, return_info=True)
        else:
            y, info = O.interpolate_with_superpixels(x, labels, n_labels, op, return_info=True)
        return y, info["fill_iters"] if info["rc"] == 0 else -1

    res = list(_POOL.map(one, list(frames)))
    out = np.stack([r[0] for r in res]), [r[1] for r in res]
    if key is not None:
        _CACHE[ck] = out
    return out


def _offsets(layout, rows, cols):
    """(src, dst) offsets in f32 elements into one buffer"""
    fe = rows * cols
    return {"same": (0, 0), "dst one frame behind": (fe, 0), "dst one frame ahead": (0, fe), "dst one row ahead": (0, cols),
            "dst one element ahead": (0, 1), "dst one element behind": (1, 0)}[layout]


def _overlapping(layout, b, rows, cols):
    """does dst overlap src at all (one frame shifted by a whole frame does not: a control cell)"""
    so, do = _offsets(layout, rows, cols)
    return abs(so - do) < b * rows * cols


def _dev_labels(lab, b):
    import torch
    return torch.from_numpy(np.stack([lab] * b)).cuda()


def _views(frames, layout):
    """src and dst: views into one fresh device buffer, overlapping as `layout` says; src holds the frames, the rest is NaN"""
    import torch
    b, r, c = frames.shape
    so, do = _offsets(layout, r, c)
    n = b * r * c
    buf = torch.full((n + max(so, do),), float("nan"), dtype=torch.float32, device="cuda")
    src, dst = buf[so:so + n].view(b, r, c), buf[do:do + n].view(b, r, c)
    src.copy_(torch.from_numpy(np.ascontiguousarray(frames)))
    return src, dst


def _u16_views(u16, where):
    """d_src16 = the front or the back half of the f32 d_dst buffer's bytes (decode into the output buffer)"""
    import torch
    b, r, c = u16.shape
    n = b * r * c
    dst = torch.full((b, r, c), float("nan"), dtype=torch.float32, device="cuda")
    halves = dst.view(-1).view(torch.int16)
    src = (halves[:n] if where == "front" else halves[n:]).view(b, r, c)
    src.copy_(torch.from_numpy(u16.view(np.int16)))
    return src, dst


def _kernels(path):
    """dcmt_last_path as a list of kernel names ("copy": the result went through scratch into the overlapping dst)"""
    return [k.split(" ")[0] for k in path.split(" + ")]


def _staged(stop, pre="k_pre_v1", copy=True):
    return [pre, "k_fill31_v1", "k_post_v1"] + (["copy"] if copy and stop <= L.STAGE_FILL7 else [])


def _fused(stop, pre="k_pre_p", fp="k_fp_s"):
    return [pre] + (["copy"] if stop == L.STAGE_EXTEND else [fp] if stop == L.STAGE_FINAL else [])


def _call(ctx, src, dst, params, labels=None, n_labels=0, u16=False):
    import torch
    if u16:
        ctx.complete_u16_dev(src, 1.0 / 256.0, dst, params)
    else:
        ctx.complete_dev(src, dst, params, d_labels=labels, n_labels=n_labels)
    torch.cuda.synchronize()
    return dst.cpu().numpy()


def _check(ctx, what, got, want, path, stop, iters=None):
    for f in range(len(got)):
        assert_bit_equal(got[f], want[f], f"{what}, frame {f}")
    assert _kernels(ctx.last_path()) == path, (what, ctx.last_path(), path)
    if stop == L.STAGE_FINAL:
        got_iters, st = ctx.last_fill_iters(len(got))
        assert got_iters == list(iters) and st == (L.OK if min(iters) > 0 else L.E_NOT_CONVERGED), (what, got_iters, st, iters)


def _run_cells(cells):
    """cells: (what, thunk); runs each once, then fails with every failing cell"""
    failed = []
    for what, cell in cells:
        try:
            cell()
        except AssertionError as e:
            failed.append(f"{what}: {str(e)[:400]}")
    assert not failed, f"{len(failed)} of {len(cells)} cells fail:\n" + "\n".join(failed)


def _params(stop, **kw):
    return api.make_params(stop_after=stop, max_fill_iters=FILL, spec_fill_iters=FILL, **kw)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_staged_f32(O, layout):
    """The staged tile kernels: batch 1 and 2 (default dispatch) and 16 full-size frames (force_staged), every stop_after.
    k_pre_v1 writes the probes of stages 2..5 itself while other workgroups still read their halo from d_src."""
    frames = _full_frames()
    want = {st: _oracle(O, frames, st, key=C) for st in STAGES}
    cells = []
    with api.Context(0, R, C, B) as c:
        for b, force in ((1, False), (2, False), (B, True)):
            for st in STAGES:
                def cell(b=b, force=force, st=st):
                    src, dst = _views(frames[:b], layout)
                    got = _call(c, src, dst, _params(st, force_staged=force))
                    _check(c, f"{layout}, batch {b}, stage {st}", got, want[st][0][:b], _staged(st, copy=_overlapping(layout, b, R, C)), st,
                           want[st][1][:b])
                cells.append((f"batch {b} stage {st}", cell))
        _run_cells(cells)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_fused_f32(O, layout):
    """The streaming kernels on 16 full-size frames, stop_after EXTEND..FINAL: k_pre_p (even width, 8-byte aligned frames) and
    k_pre_s (odd width, or frames one element off).  At EXTEND k_pre writes the probe itself while other waves read their strips."""
    cells = []
    with api.Context(0, R, C, B) as c:
        for cols in (C, C - 1):
            frames = _full_frames(cols)
            want = {st: _oracle(O, frames, st, key=cols) for st in range(L.STAGE_EXTEND, L.STAGE_FINAL + 1)}
            pre = "k_pre_p" if cols % 2 == 0 and _offsets(layout, R, cols)[0] % 2 == 0 else "k_pre_s"
            for st in range(L.STAGE_EXTEND, L.STAGE_FINAL + 1):
                def cell(frames=frames, want=want, pre=pre, st=st, cols=cols):
                    src, dst = _views(frames, layout)
                    got = _call(c, src, dst, _params(st))
                    _check(c, f"{layout}, {R}x{cols}, stage {st}", got, want[st][0], _fused(st, pre), st, want[st][1])
                cells.append((f"{R}x{cols} stage {st}", cell))
        _run_cells(cells)


def test_16_bit_attempt_f32_and_labeled(O, monkeypatch):
    """DCMT_Q16_MIN_WAVES=0: the 16-bit attempt at 16 frames.  Separate buffers take it (the control); overlapping ones must not,
    on a batch with a frame off the 1/256 m grid (the attempt's gated f32 rerun would read d_src after k_fp_q wrote d_dst).  The
    labeled entry point takes it whatever d_dst overlaps: its attempt and rerun read the label stage's output in scratch."""
    import torch
    monkeypatch.setenv("DCMT_Q16_MIN_WAVES", "0")
    grid = _full_frames()
    mixed = grid.copy()
    mixed[2][mixed[2] > 0] += np.float32(0.001)       # off the grid
    mixed[11, 100, 100] = 120.0                       # on the grid, beyond the code range
    want_grid, want_mixed = _oracle(O, grid, 11, key=C), _oracle(O, mixed, 11)
    lab, nl = _full_labels()
    want_lab = _oracle(O, mixed, 11, labels=lab, n_labels=nl)
    d_lab = _dev_labels(lab, B)
    cells = []
    with api.Context(0, R, C, B) as c:
        def control():
            src = torch.from_numpy(grid).cuda()
            got = _call(c, src, torch.full_like(src, float("nan")), _params(11))
            _check(c, "separate buffers", got, want_grid[0], ["k_pre_p<Q16OUT>", "k_fp_q"], 11, want_grid[1])
        cells.append(("control", control))
        for layout in LAYOUTS:
            def cell(layout=layout):
                src, dst = _views(mixed, layout)
                pre = "k_pre_s" if _offsets(layout, R, C)[0] % 2 else "k_pre_p"
                _check(c, layout, _call(c, src, dst, _params(11)), want_mixed[0], [pre, "k_fp_s"], 11, want_mixed[1])
            cells.append((layout, cell))
        _run_cells(cells)
    cells = []
    for layout in ("same", "dst one frame behind", "dst one row ahead"):
        def lcell(layout=layout):
            with api.Context(0, R, C, B) as c:      # fresh: a raised flag makes a context skip its next 63 attempts
                src, dst = _views(mixed, layout)
                got = _call(c, src, dst, _params(11), labels=d_lab, n_labels=nl)
                _check(c, f"labeled, {layout}", got, want_lab[0], ["k_label_bbox", "k_label_stage", "k_pre_p<Q16OUT>", "k_fp_q"], 11,
                       want_lab[1])
        cells.append((f"labeled {layout}", lcell))
    _run_cells(cells)


@pytest.mark.parametrize("where", ("front", "back"))
def test_u16_into_its_own_output_buffer(O, monkeypatch, where):
    """dcmt_complete_u16_dev with d_src16 inside d_dst's bytes, every stop_after: the staged kernels (stages 2..5: the payload is
    converted into scratch first), the streaming ones (6..11), and at FINAL the 16-bit attempt -- taken with separate buffers, never
    when d_src16 overlaps d_dst (payloads > 30719 raise the attempt's flag: its gated f32 rerun would read d_src16 after k_fp_q
    wrote d_dst).  The control shows the flag is raised: the context skips the attempt on its next call."""
    import torch
    monkeypatch.setenv("DCMT_Q16_MIN_WAVES", "0")
    u16 = np.round(_full_frames() * 256.0).astype(np.uint16)
    u16[1, 200, 300] = 65535
    u16[6, 200:260, 400:480] = 40000                  # 156.25 m, a block: X6 keeps values with no 16-bit code (the flag is raised)
    as_f32 = (u16.astype(np.float32) * np.float32(1.0 / 256.0)).astype(np.float32)
    want = {st: _oracle(O, as_f32, st, key="u16") for st in STAGES}

    def control():
        with api.Context(0, R, C, B) as c:
            src = torch.from_numpy(u16.view(np.int16)).cuda()
            got = _call(c, src, torch.full(src.shape, float("nan"), dtype=torch.float32, device="cuda"), _params(11), u16=True)
            _check(c, "u16, separate buffers", got, want[11][0], ["k_pre_p<U16,Q16OUT>", "k_fp_q"], 11, want[11][1])
            got = _call(c, src, torch.full(src.shape, float("nan"), dtype=torch.float32, device="cuda"), _params(11), u16=True)
            _check(c, "u16, separate buffers, the next call", got, want[11][0], ["k_pre_p<U16>", "k_fp_s"], 11, want[11][1])

    def final():
        with api.Context(0, R, C, B) as c:
            src, dst = _u16_views(u16, where)
            _check(c, f"u16 {where}, stage 11", _call(c, src, dst, _params(11), u16=True), want[11][0], ["k_pre_p<U16>", "k_fp_s"], 11,
                   want[11][1])
    cells = [("control", control), ("stage 11", final)]
    with api.Context(0, R, C, B) as c:
        for st in range(L.STAGE_INVERT, L.STAGE_FINAL):
            def cell(st=st):
                src, dst = _u16_views(u16, where)
                path = _staged(st, copy=False) if st < L.STAGE_EXTEND else _fused(st, "k_pre_p<U16>")
                _check(c, f"u16 {where}, stage {st}", _call(c, src, dst, _params(st), u16=True), want[st][0], path, st)
            cells.append((f"stage {st}", cell))
        _run_cells(cells)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_labeled(O, layout):
    """dcmt_complete_labeled_f32_dev at CLOSE5 and FINAL: the fast path (bounding boxes + label stage, 16 frames), the staged kernels
    (batch 2, and 16 frames with force_staged).  At CLOSE5 the label stage writes X4 -- the probe -- while it reads d_src."""
    frames = _full_frames()
    lab, nl = _full_labels()
    d_lab = _dev_labels(lab, B)
    want = {st: _oracle(O, frames, st, labels=lab, n_labels=nl, key=C) for st in (L.STAGE_CLOSE5, L.STAGE_FINAL)}
    fast = {L.STAGE_CLOSE5: ["k_label_bbox", "k_label_stage", "copy"],
            L.STAGE_FINAL: ["k_label_bbox", "k_label_stage", "k_pre_p<START4>", "k_fp_s"]}
    cells = []
    with api.Context(0, R, C, B) as c:
        for b, force in ((B, False), (2, False), (B, True)):
            for st in (L.STAGE_CLOSE5, L.STAGE_FINAL):
                def cell(b=b, force=force, st=st):
                    src, dst = _views(frames[:b], layout)
                    got = _call(c, src, dst, _params(st, force_staged=force), labels=d_lab[:b], n_labels=nl)
                    path = fast[st] if b >= 3 and not force else _staged(st, "k_pre_labeled_v1")
                    _check(c, f"{layout}, batch {b}, stage {st}", got, want[st][0][:b], path, st, want[st][1][:b])
                cells.append((f"batch {b}{' staged' if force else ''} stage {st}", cell))
        _run_cells(cells)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_normalize(O, layout):
    """DCMT_FLAG_NORMALIZE (0, 80) on 16 full-size frames, every stop_after: the normalised frames themselves (k_norm_write, a
    grid-stride pass), the staged probes, the streaming kernels."""
    frames = _full_frames()
    cells = []
    with api.Context(0, R, C, B) as c:
        for st in range(L.STAGE_NORMALIZE, L.STAGE_FINAL + 1):
            def cell(st=st):
                want, iters = _oracle(O, frames, st, norm=(0, 80), key=C)
                src, dst = _views(frames, layout)
                got = _call(c, src, dst, _params(st, normalize=(0, 80)))
                pre = "k_pre_s" if _offsets(layout, R, C)[0] % 2 else "k_pre_p<NORM>"
                path = (["k_minmax", "k_norm_coef", "k_norm_write", "copy"] if st == L.STAGE_NORMALIZE else
                        _staged(st) if st < L.STAGE_EXTEND else _fused(st, pre))
                _check(c, f"{layout}, normalize, stage {st}", got, want, path, st, iters)
            cells.append((f"stage {st}", cell))
        _run_cells(cells)


def test_seeded_fuzz(O, monkeypatch):
    """40 seeded draws of (path, stage, layout, shape, k0, blur) at small shapes, DCMT_Q16_MIN_WAVES=0, a fresh context each."""
    import torch
    monkeypatch.setenv("DCMT_Q16_MIN_WAVES", "0")
    g = np.random.Generator(np.random.PCG64(4242))
    routes = ("staged", "fused", "u16", "labeled fast", "labeled staged", "normalize")
    cells = []
    for case in range(40):
        route = routes[case % len(routes)] if case < len(routes) else routes[int(g.integers(0, len(routes)))]
        rows, cols = int(g.integers(8, 120)), int(g.integers(8, 300))
        k0 = ("as_compiled", "diamond")[g.integers(0, 2)]
        blur = ("gaussian", "none")[g.integers(0, 2)]
        layout = ("front", "back")[g.integers(0, 2)] if route == "u16" else LAYOUTS[g.integers(0, len(LAYOUTS))]
        kw, norm, lab, nl, u16 = {}, None, None, 0, False
        if route == "staged":
            batch = int(g.choice([1, 2, 4]))
            kw["force_staged"] = batch == 4
            stop = int(g.integers(2, 12))
        elif route in ("fused", "u16"):
            batch = int(g.choice([1, 3, 5]))
            kw["force_fused"] = True
            stop = int(g.integers(6, 12))
            u16 = route == "u16"
            if u16:
                cols += cols % 2 * int(g.integers(0, 2))  # mostly even widths: k_pre_p<U16>
        elif route.startswith("labeled"):
            batch = 4 if route == "labeled fast" else int(g.choice([1, 2]))
            stop = int(g.choice([4, 11]))
            lab, nl = _labels(g, rows, cols)
        else:
            batch = int(g.choice([1, 4]))
            stop = int(g.integers(1, 12))
            norm = kw["normalize"] = (0, 80)
        if norm is None and route != "normalize" and g.random() < 0.25 and not u16:
            norm = kw["normalize"] = (0, 100)
        frames = np.stack([(_grid_frame if u16 or g.random() < 0.5 else _frame)(g, rows, cols) for _ in range(batch)])
        what = f"case {case}: {route} {rows}x{cols} b{batch} stop {stop} {layout} {k0} {blur} norm {norm}"

        def cell(route=route, rows=rows, cols=cols, batch=batch, stop=stop, k0=k0, blur=blur, layout=layout, kw=kw, norm=norm, lab=lab,
                 nl=nl, u16=u16, frames=frames, what=what):
            p = _params(stop, k0=k0, blur_type=blur, **kw)
            with api.Context(0, rows, cols, batch) as c:
                if u16:
                    payload = np.round(frames * 256.0).astype(np.uint16)
                    frames = (payload.astype(np.float32) * np.float32(1.0 / 256.0)).astype(np.float32)
                    src, dst = _u16_views(payload, layout)
                    in_off = 0 if layout == "front" else 2 * frames.size      # bytes from dst
                    dst_off = 0
                else:
                    src, dst = _views(frames, layout)
                    so, do = _offsets(layout, rows, cols)
                    in_off, dst_off = 4 * so, 4 * do
                d_lab = None if lab is None else _dev_labels(lab, batch)
                got = _call(c, src, dst, p, labels=d_lab, n_labels=nl, u16=u16)
                want, iters = _oracle(O, frames, stop, k0, blur, norm, lab, nl)
                pair = cols % 2 == 0 and cols >= 8
                ov = u16 or _overlapping(layout, batch, rows, cols)
                if stop == L.STAGE_NORMALIZE:
                    path = ["k_minmax", "k_norm_coef", "k_norm_write"] + ["copy"] * ov
                elif route == "labeled fast":               # (the label stage's output in scratch is what the 16-bit attempt reads)
                    q16 = pair and norm is None and dst_off % 8 == 0
                    path = (["k_label_bbox", "k_label_stage", "copy"] if stop == 4 else
                            ["k_label_bbox", "k_label_stage", "k_pre_p<Q16OUT>" if q16 else "k_pre_p<START4>" if pair else "k_pre_s",
                             "k_fp_q" if q16 else "k_fp_s"])
                elif route in ("fused", "u16") or (route == "normalize" and batch >= 3 and stop >= L.STAGE_EXTEND):
                    pair = pair and in_off % (4 if u16 else 8) == 0 and (ov or stop != L.STAGE_EXTEND or dst_off % 8 == 0)
                    if stop == L.STAGE_FINAL and pair and norm is None and not ov and dst_off % 8 == 0:
                        path = ["k_pre_p<Q16OUT>", "k_fp_q"]  # (one frame shifted by a whole frame: separate memory)
                    else:
                        path = _fused(stop, ("k_pre_p<U16>" if u16 else "k_pre_p<NORM>" if norm else "k_pre_p") if pair else "k_pre_s")
                        path = path[:1] if stop == L.STAGE_EXTEND and not ov else path
                else:
                    path = _staged(stop, "k_pre_labeled_v1" if lab is not None else "k_pre_v1", copy=ov)
                _check(c, what, got, want, path, stop, iters)
        cells.append((what, cell))
    _run_cells(cells)


def test_host_entry_points_in_place(O):
    """dcmt_complete_f32 / dcmt_complete_labeled_f32 with src == dst, one host pointer, contiguous and padded rows: they stage through
    device buffers of their own.  The padding is left alone."""
    rows, cols, b = 96, 200, 3
    frames = synth.synth_batch(b, rows, cols, 40)
    frames[1, 40:70] = 0
    lab, nl = synth.synth_labels(rows, cols, 80, 4)
    labs = np.stack([lab] * b)
    cells = []
    with api.Context(0, rows, cols, b) as c:
        for pad in (0, 7):
            for labeled in (False, True):
                for st in (L.STAGE_CLOSE5, L.STAGE_FINAL):
                    def cell(pad=pad, labeled=labeled, st=st):
                        buf = np.full((b, rows, cols + pad), 12345.0, np.float32)
                        buf[:, :, :cols] = frames
                        want, iters = _oracle(O, frames, st, labels=lab if labeled else None, n_labels=nl)
                        p = api.make_params(stop_after=st)
                        ptr, rs, fs = buf.ctypes.data, buf.strides[1], buf.strides[0]
                        if labeled:
                            rc = L.lib().dcmt_complete_labeled_f32(c._h, ptr, rs, fs, labs.ctypes.data, labs.strides[1], labs.strides[0], nl,
                                                                   ptr, rs, fs, rows, cols, b, ctypes.byref(p), 1)
                        else:
                            rc = L.lib().dcmt_complete_f32(c._h, ptr, rs, fs, ptr, rs, fs, rows, cols, b, ctypes.byref(p))
                        assert rc == L.OK, rc
                        for f in range(b):
                            assert_bit_equal(buf[f, :, :cols], want[f], f"pad {pad} labeled {labeled} stage {st} frame {f}")
                        assert (buf[:, :, cols:] == 12345.0).all(), "padding written"
                        assert "copy" not in _kernels(c.last_path()), c.last_path()
                        if st == L.STAGE_FINAL:
                            assert c.last_fill_iters(b) == (iters, L.OK)
                    cells.append((f"pad {pad} labeled {labeled} stage {st}", cell))
        _run_cells(cells)
