"""Batches past 2^31 / 2^32 bytes and at the largest batch dcmt_create admits: the three geometries, how such a batch is made from
a handful of frames, how its output is verified on the device, and one case per *_dev entry point.  A plain module:
tests/test_large_batch.py checks it without a GPU, tests/test_gpu_large_batch.py runs the cases.

The geometries are the smallest at which each boundary exists (the batch cap is 65535, so the frames are as small as it allows):
    A  65535 x  96 x  176   f32 / int32 planes pass 2^32 bytes, u8 x 3 planes 2^31 bytes; the largest batch = the largest grid y / z
    B   2512 x 352 x 1216   f32 planes pass 2^32 bytes at the production shape; batch % 8 == 0 (XCD map on)
    C  65535 x 128 x  260   more than 2^31 and 0x7fff0000 pixels: the three segmented entry points run two segments
Their figures are recomputed and asserted below.

A batch: K = 5 distinct frames tiled over the batch (frame f holds source f % K; 5 divides neither 4 nor 8, so no tile or XCD
period lines up with it) and one UNIQUE source at frame 0, at the last frame, and at every frame that holds a boundary of a plane
the entry point touches (byte 2^31 and 2^32 of planes of 4, 2, 1 and 3 bytes per pixel; pixel marks such as 2^31 and a segment
start) and at the frame behind it.  Layout.index maps a frame to its source.  The device batch is src[index]: no host array has
the size of a batch.

The expectation of a frame is the reference's result for its source -- the references are the ones the small tests use -- so the
whole output is compared, bit for bit and on the device, with expectation[index], in chunks (mismatched_frames).  A kernel that
wrapped a 32-bit offset reads or writes another frame: the frame it should have written keeps the sentinel every output starts
with, and the frame it wrote instead holds another source's result, which differs (assert_distinct).  Where the project states a
bound instead of bit equality (bilateral5 against f64, the evaluation sums against fsum) the bound is checked on one frame per
source and every other frame is compared with that frame's bits."""
import time

import numpy as np

from depth_completion_mt_amd import _lib as L
from depth_completion_mt_amd import api, synth

f32 = np.float32
P31, P32 = 1 << 31, 1 << 32
SEG_PX = 0x7fff0000             # kBgrSegPx, kU16SegPx (csrc/dcmt_tiles.h, csrc/dcmt_crop.h)
COLOR_PX_PER_WG = 4096          # kColorPxPerWg
K_TILED = 5
SPEC = 16                       # spec_fill_iters of every completion call here (the frame with a 40-row gap needs fewer: asserted)
CAP_BYTES = 40 * 10 ** 9        # no test may need more device memory than this
SENT_F32 = 0x7FC5A5A5           # a NaN no kernel produces
SENT_F64 = 0x7FF8A5A5A5A5A5A5
SENT_BYTE = 0xA5
SENT_LABEL = -2


class Geometry:
    def __init__(self, name, batch, rows, cols):
        self.name, self.batch, self.rows, self.cols = name, batch, rows, cols
        self.px = rows * cols
        self.total_px = batch * self.px

    def __repr__(self):
        return f"{self.name} ({self.batch} x {self.rows} x {self.cols})"


A = Geometry("A", 65535, 96, 176)
B = Geometry("B", 2512, 352, 1216)
C = Geometry("C", 65535, 128, 260)
GEOMETRIES = {"A": A, "B": B, "C": C}


def color_seg_frames(g):
    """Frames per segment of dcmt_colorize_dev (plan_colorize, csrc/dcmt_plan_side.h), restated."""
    cap = (P31 - COLOR_PX_PER_WG) // g.px
    seg = min(g.batch, cap)
    if 4 <= seg < g.batch:
        seg &= ~3
    return seg


def check_geometries():
    """The table of the module docstring, recomputed."""
    assert A.px == 16896 and A.total_px == 1_107_279_360 and 4 * A.total_px == 4_429_117_440 > P32
    assert P32 // (4 * A.px) == 63550 and P32 - 63550 * 4 * A.px == 4096 and P31 // (4 * A.px) == 31775 and P31 % (4 * A.px) != 0
    assert P31 < 3 * A.total_px < P32 and A.total_px < P31 and A.batch == 65535
    assert B.px == 428032 and B.total_px == 1_075_216_384 and 4 * B.total_px == 4_300_865_536 > P32
    assert P32 // (4 * B.px) == 2508 and P32 % (4 * B.px) != 0 and P31 // (4 * B.px) == 1254 and B.batch % 8 == 0 and B.total_px < P31
    assert C.px == 33280 and C.total_px == 2_181_004_800 > P31 > SEG_PX and P31 // C.px == 64527 and P31 % C.px != 0
    assert P31 < C.total_px < P32 < 3 * C.total_px and C.total_px > 2 ** 31 - 1
    for g in (A, B, C):
        assert g.px <= 0x1FFFFFF0 and g.batch <= 65535                                     # what dcmt_create admits
    assert -(-C.total_px // SEG_PX) == 2 and color_seg_frames(C) == 64524 and -(-C.batch // color_seg_frames(C)) == 2
    assert color_seg_frames(A) == A.batch and color_seg_frames(B) == B.batch and A.total_px < SEG_PX and B.total_px < SEG_PX


check_geometries()


# ---------------------------------------------------------------------------------------------------------------- boundaries
def boundary_frames(g, elem_bytes=(), px_marks=()):
    """The frames a unique source goes to beside frame 0 and the last one.  elem_bytes: bytes per pixel of every plane the entry
    point touches; for each, byte 2^31 and byte 2^32 of the [batch][px] plane, where the plane reaches that far.  px_marks: pixel
    positions in the batch's flat pixel run (2^31, a segment's first pixel).  Per boundary: the frame that holds the byte or pixel
    AT the boundary, the frame behind it, and -- where the boundary is a frame's first byte -- the frame in front."""
    marks = [(b, e * g.px) for e in elem_bytes for b in (P31, P32)] + [(p, g.px) for p in px_marks]
    out = set()
    for pos, unit in marks:
        if pos >= unit * g.batch:
            continue
        h = pos // unit
        out.update(f for f in ((h - 1) if pos % unit == 0 else h, h, h + 1) if 0 <= f < g.batch)
    return sorted(out)


def boundary_frames_brute(g, elem_bytes=(), px_marks=()):
    """The same set stated frame by frame: frame f occupies [f * unit, (f + 1) * unit)."""
    f = np.arange(g.batch, dtype=np.int64)
    out = set()
    for unit, pos in [(e * g.px, b) for e in elem_bytes for b in (P31, P32)] + [(g.px, p) for p in px_marks]:
        holds = (f * unit <= pos) & (pos < (f + 1) * unit)
        ends_at = (f + 1) * unit == pos                          # the frame whose last byte is in front of the boundary
        for h in np.flatnonzero(holds):
            out.add(int(h))
            if h + 1 < g.batch:
                out.add(int(h) + 1)
            out.update(int(e) for e in np.flatnonzero(ends_at))
    return sorted(out)


class Layout:
    """index [batch]: the source of every frame.  Sources 0 .. k-1 are the tiled ones, k .. n_src-1 the unique ones in frame order
    (source k is frame 0's, source n_src - 1 the last frame's).  reps [n_src]: the first frame that holds each source.  Pixel 2^31
    of the batch is a mark of every layout (geometry C has it)."""

    def __init__(self, g, elem_bytes=(4,), px_marks=(), extra=(), k=K_TILED):
        assert k % 2 == 1 and 4 % k and 8 % k and g.batch > 4 * k
        self.g, self.k = g, k
        self.unique = sorted({0, g.batch - 1} | set(boundary_frames(g, elem_bytes, tuple(px_marks) + (P31,))) | {int(f) for f in extra})
        self.index = np.arange(g.batch, dtype=np.int64) % k
        self.index[self.unique] = k + np.arange(len(self.unique))
        self.n_src = k + len(self.unique)
        self.reps = np.array([self.tiled_rep(s) for s in range(k)] + self.unique, dtype=np.int64)
        assert (self.index[self.reps] == np.arange(self.n_src)).all()

    def tiled_rep(self, s):
        f = s
        while f in self.unique:
            f += self.k
        return f

    def source_of(self, frame):
        return int(self.index[frame])


# ---------------------------------------------------------------------------------------------------------------- bits
def _as_words_np(a):
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def is_sentinel_frame(a, label=False):
    """A host frame that is nothing but the fill its output buffer starts with."""
    w = _as_words_np(a)
    if label:
        return bool((np.ascontiguousarray(a) == SENT_LABEL).all())
    if a.dtype == np.float32:
        return bool((w == SENT_F32).all())
    if a.dtype == np.float64:
        return bool((w == SENT_F64).all())
    return bool((np.ascontiguousarray(a).view(np.uint8) == SENT_BYTE).all())


def assert_distinct(name, exp, label=False):
    """The condition on the inputs: the expectations of the sources differ pairwise, bit for bit, and none is the sentinel -- a
    frame that holds another frame's result, or was never written, cannot look right."""
    exp = np.ascontiguousarray(exp)
    seen = {}
    for s in range(exp.shape[0]):
        key = exp[s].tobytes()
        assert key not in seen, f"{name}: sources {seen[key]} and {s} have the same expectation"
        seen[key] = s
        assert not is_sentinel_frame(exp[s], label), f"{name}: the expectation of source {s} is the sentinel"


def fill_sentinel(t, label=False):
    import torch
    if label:
        t.fill_(SENT_LABEL)
    elif t.dtype == torch.float32:
        t.view(torch.int32).fill_(SENT_F32)
    elif t.dtype == torch.float64:
        t.view(torch.int64).fill_(SENT_F64)
    else:
        t.view(torch.uint8).fill_(SENT_BYTE)
    return t


def sentinel(shape, dtype, device="cuda", label=False):
    """An output buffer as every test hands it to the call."""
    import torch
    return fill_sentinel(torch.empty(tuple(shape), dtype=dtype, device=device), label)


def torch_dtype(np_dtype):
    import torch
    return {"float32": torch.float32, "float64": torch.float64, "int32": torch.int32, "uint8": torch.uint8, "int16": torch.int16,
            "int64": torch.int64}[np.dtype(np_dtype).name]


def words(t):
    """A tensor's bit patterns as integers torch can compare."""
    import torch
    view = {torch.float32: torch.int32, torch.float64: torch.int64, torch.uint16: torch.int16}.get(t.dtype)
    return t if view is None else t.view(view)


def mismatched_frames(out, exp, index, chunk_bytes=256 << 20):
    """out [n][...], exp [n_src][...] of the same dtype and trailing shape, index int64 [n], all on one device: (the number of
    frames f whose bits differ from exp[index[f]], the first few of them).  Chunked: the gathered expectation and the comparison
    of one chunk stay below about three times chunk_bytes."""
    import torch
    o, e = words(out), words(exp)
    n = o.shape[0]
    assert o.dtype == e.dtype and tuple(o.shape[1:]) == tuple(e.shape[1:]) and index.numel() == n, (o.dtype, e.dtype, o.shape, e.shape, index.shape)
    frame_bytes = max(1, o[0].numel() * o.element_size())
    step = max(1, chunk_bytes // frame_bytes)
    count, first = 0, []
    for s in range(0, n, step):
        t = min(n, s + step)
        neq = (o[s:t] != e[index[s:t]]).reshape(t - s, -1).any(dim=1)
        c = int(neq.sum())
        if c:
            count += c
            if len(first) < 8:
                first += (torch.nonzero(neq).flatten()[:8 - len(first)] + s).tolist()
    return count, first


def describe_frame(out, exp, index, f, label=False):
    """What the first wrong frame holds: the sentinel, another source's expectation, the expectation moved, or neither."""
    got = out[f].cpu().numpy()
    want = exp[int(index[f])].cpu().numpy()
    if is_sentinel_frame(got, label):
        return "it still holds the sentinel: never written"
    e = exp.cpu().numpy()
    for s in range(e.shape[0]):
        if got.tobytes() == e[s].tobytes():
            return f"it holds the expectation of source {s}: another frame's result"
    gw, ww = _as_words_np(got).ravel(), _as_words_np(want).ravel()
    neq = np.flatnonzero(gw != ww)
    return f"{len(neq)} of {gw.size} words differ, the first at {int(neq[0])}: {gw[neq[0]]:#x} vs {ww[neq[0]]:#x}"


def assert_frames(name, out, exp, index, label=False):
    count, first = mismatched_frames(out, exp, index)
    if count:
        f = first[0]
        raise AssertionError(f"{name}: {count} of {out.shape[0]} frames differ from the expectation of their source; the first are {first} "
                             f"(sources {[int(index[i]) for i in first]}); frame {f}: {describe_frame(out, exp, index, f, label)}")


# ---------------------------------------------------------------------------------------------------------------- the device side
def dev(a):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a if a.flags.writeable else a.copy()).cuda()


def check_memory(name, need):
    """need: the bytes the test allocates on the device.  Skips only where another tenant leaves less than need + a quarter free."""
    import pytest
    import torch
    assert need < CAP_BYTES, f"{name}: needs {need / 1e9:.1f} GB, the cap of this module is {CAP_BYTES / 1e9:.0f} GB"
    free, _ = torch.cuda.mem_get_info()
    if free < need * 1.25:
        pytest.skip(f"{name}: needs {need / 1e9:.1f} GB + a quarter, {free / 1e9:.1f} GB are free on this device")


class Timer:
    def __init__(self):
        self.t, self.phases = time.perf_counter(), []

    def phase(self, name):
        import torch
        torch.cuda.synchronize()
        now = time.perf_counter()
        self.phases.append((name, now - self.t))
        self.t = now

    def __str__(self):
        return ", ".join(f"{n} {s:.2f} s" for n, s in self.phases) + f", in all {sum(s for _, s in self.phases):.2f} s"


def report(name, need, timer):
    import torch
    print(f"[large-batch] {name}: stated need {need / 1e9:.2f} GB, torch peak {torch.cuda.max_memory_allocated() / 1e9:.2f} GB (the context's "
          f"scratch comes on top); {timer}")


class FrameCase:
    """An entry point whose outputs are per frame and depend on that frame's inputs alone.
    g: the geometry; planes: bytes per pixel of every plane the call touches; px_marks / extra: Layout's.
    sources(lay) -> {name: array [n_src][...]}: the inputs, one entry per source.
    reference(src, lay) -> {name: array [n_src][...]}: what the references give for every source; keys with a leading underscore
        are host values for `after`.
    outputs: {name: (trailing shape, numpy dtype)}; a name that is also an input is written in place (no sentinel).
    call(ctx, t, o, lay): the call(s); t the batch-sized inputs, o the outputs, filled with the sentinel.
    bounds: {output name: check(got [n_src][...], src, lay)}: outputs the project states a bound for instead of bit equality -- the
        check runs on one frame per source, every other frame is compared with those frames' bits (reference leaves them out, or
        gives them for the distinctness check alone).
    after(ctx, ref, lay): host-side checks behind the call.  scratch: bytes of context scratch beyond its two planes.
    labels: names of outputs whose sentinel is -2.  aux: outputs too small to differ between all sources (a count per frame): they
    ride along with an output that does.  tables(lay) -> {name: tensor}: further device inputs (calibration tables)."""

    def __init__(self, name, g, planes, sources, reference, outputs, call, bounds=None, after=None, scratch=0, px_marks=(), extra=(),
                 labels=(), tables=None, aux=()):
        self.name, self.g, self.planes, self.sources, self.reference, self.outputs, self.call = name, g, planes, sources, reference, outputs, call
        self.bounds, self.after, self.scratch, self.px_marks, self.extra, self.labels = bounds or {}, after, scratch, px_marks, extra, labels
        self.tables, self.aux = tables, aux
        self._prep = None

    def layout(self):
        return Layout(self.g, self.planes, self.px_marks, self.extra)

    def prepare(self):
        """(layout, sources, reference): host work only, computed once and left unchanged."""
        if self._prep is None:
            lay = self.layout()
            src = {k: np.ascontiguousarray(v) for k, v in self.sources(lay).items()}
            for v in src.values():
                assert v.shape[0] == lay.n_src
                v.setflags(write=False)
            ref = self.reference(src, lay)
            for name in self.outputs:
                if name not in self.aux:
                    assert_distinct(f"{self.name}: {name}", ref[name], name in self.labels)
            assert len(self.aux) < len(self.outputs)
            self._prep = (lay, src, ref)
        return self._prep

    def need_bytes(self):
        lay, src, _ = self.prepare()
        per_frame = sum(v[0].nbytes for v in src.values())
        per_frame += sum(int(np.prod(shape, dtype=np.int64)) * np.dtype(dt).itemsize for n, (shape, dt) in self.outputs.items() if n not in src)
        return 2 * 4 * self.g.total_px + self.scratch + per_frame * self.g.batch + (1 << 30)      # + the comparison's chunks

    def run(self):
        import torch
        lay, src, ref = self.prepare()
        need = self.need_bytes()
        check_memory(self.name, need)
        torch.cuda.reset_peak_memory_stats()
        tm = Timer()
        g = self.g
        index = dev(lay.index)
        with api.Context(0, g.rows, g.cols, g.batch) as ctx:
            tm.phase("context")
            t = {k: dev(v)[index] for k, v in src.items()}
            if self.tables:
                t.update(self.tables(lay))
            o = {n: sentinel((g.batch,) + tuple(shape), torch_dtype(dt), label=n in self.labels) for n, (shape, dt) in self.outputs.items() if n not in src}
            tm.phase("tile and fill")
            self.call(ctx, t, o, lay)
            tm.phase("call")
            if self.after:
                self.after(ctx, ref, lay)
            reps = dev(lay.reps)
            for name in self.outputs:
                got = o[name] if name in o else t[name]
                if name in self.bounds:
                    at_reps = got[reps]
                    self.bounds[name](at_reps.cpu().numpy(), src, lay)
                    exp = at_reps
                else:
                    want = np.ascontiguousarray(ref[name], dtype=self.outputs[name][1])
                    exp = dev(want)
                assert_frames(f"{self.name}: {name}", got, exp, index, name in self.labels)
                del exp
            tm.phase("compare")
        report(self.name, need, tm)


# ---------------------------------------------------------------------------------------------------------------- inputs
def O():
    from oracle import oracle
    return oracle


def sparse_sources(lay, seed, gap=True, empty=True, off_grid=False):
    """Sparse depth frames, multiples of 1/256 m (off_grid: every valid pixel moved off that grid).  gap: the last frame's source
    has a 40-row gap under a valid band, so that the hole-closure loop has to run there; empty: the source of the first boundary
    frame (or of frame 0) is all zero."""
    g = lay.g
    x = synth.synth_batch(lay.n_src, g.rows, g.cols, seed)
    if off_grid:
        x = np.where(x > 0, x + f32(0.001), f32(0)).astype(f32)
    if gap:
        x[-1, 0:2] = f32(40.0) + f32(seed % 64) / f32(4.0) + (f32(0.001) if off_grid else f32(0))
        x[-1, 4:44] = 0
    if empty:
        x[lay.k + 1 if lay.n_src > lay.k + 2 else lay.k] = 0
    return x


def dense_sources(lay, seed, lo=0.5, hi=80.0):
    g = lay.g
    return np.random.default_rng(seed).uniform(lo, hi, (lay.n_src, g.rows, g.cols)).astype(f32)


def stack(frames):
    return np.stack([np.ascontiguousarray(f) for f in frames])


# ---------------------------------------------------------------------------------------------------------------- completion
COMPLETE_VARIANTS = ("default", "off_grid", "force_staged", "normalize", "stop_normalize", "stop_extend", "no_extrapolate", "bilateral_clone")


def complete_params(variant):
    kw = {"force_staged": dict(force_staged=True), "normalize": dict(normalize=(0.0, 80.0)),
          "stop_normalize": dict(normalize=(0.0, 80.0), stop_after=L.STAGE_NORMALIZE), "stop_extend": dict(stop_after=L.STAGE_EXTEND),
          "no_extrapolate": dict(extrapolate=False), "bilateral_clone": dict(blur_type="bilateral_clone", stop_after=L.STAGE_BLUR)}.get(variant, {})
    return api.make_params(spec_fill_iters=SPEC, **kw)


def complete_paths(variant):
    """What dcmt_last_path must say at these batch sizes (csrc/dcmt_plan.h: plan_call)."""
    return {"default": ("k_pre_p<Q16OUT> + k_fp_q",), "off_grid": ("k_pre_p<Q16OUT> + k_fp_q", "k_pre_p + k_fp_s"),
            "force_staged": ("k_pre_v1 + k_fill31_v1 + k_post_v1 (staged tile kernels)",), "normalize": ("k_pre_p<NORM> + k_fp_s",),
            "stop_normalize": ("k_minmax + k_norm_coef + k_norm_write",), "stop_extend": ("k_pre_p",), "no_extrapolate": ("k_local",),
            "bilateral_clone": ("k_pre_p + bilateral5",)}[variant]


def complete_reference(x, variant):
    """(the oracle's plane, its info or None) for one frame."""
    o = O()
    if variant in ("default", "off_grid", "force_staged"):
        return o.img_completion(x, return_info=True)
    if variant == "normalize":
        return o.img_completion(o.normalize_minmax(x, 0.0, 80.0), return_info=True)
    if variant == "stop_normalize":
        return o.normalize_minmax(x, 0.0, 80.0), None
    if variant == "stop_extend":
        return o.img_completion(x, o.default_params(stop_after=L.STAGE_EXTEND)), None
    if variant == "no_extrapolate":
        import no_extrapolate_restatement as NE
        return NE.restatement_oracle(x), None
    assert variant == "bilateral_clone"
    import bilateral_restatement as BR
    med = o.img_completion(x, o.default_params(blur="none", stop_after=L.STAGE_MEDIAN5))
    return BR.restatement_f64(med), None


BILATERAL_TOL = 2e-5            # tests/test_gpu_bilateral.py: the project's stated bound against the f64 restatement


def bound_f64(name, want64):
    def check(got, src, lay):
        e = float(np.abs(got.astype(np.float64) - want64).max())
        print(f"[large-batch] {name}: max |device - f64| over the {len(got)} source frames = {e:.3g}")
        assert e <= BILATERAL_TOL, (name, e)
    return check


def complete_case(g, variant, seed=100):
    name = f"complete_dev {variant} {g.name}"
    loop = variant in ("default", "off_grid", "force_staged", "normalize")

    def sources(lay):
        return {"src": sparse_sources(lay, seed, off_grid=variant == "off_grid")}

    def reference(src, lay):
        res = [complete_reference(x, variant) for x in src["src"]]
        ref = {"dst": stack([r[0] for r in res]).astype(f32 if variant != "bilateral_clone" else np.float64)}
        if loop:
            for s, (_, info) in enumerate(res):
                assert info["rc"] == 0 and info["fill_iters"] < SPEC, (name, s, info)
            ref["_iters"] = [r[1]["fill_iters"] for r in res]
            ref["_holes"] = [r[1]["holes_after_extend"] for r in res]
            assert ref["_iters"][-1] > 1, (name, ref["_iters"])          # the gap frame does need the loop
        if variant == "bilateral_clone":
            ref["_f64"] = ref["dst"]
            ref["dst"] = ref["dst"].astype(f32)                      # for the distinctness check alone
        return ref

    def call(ctx, t, o, lay):
        import torch
        ctx.complete_dev(t["src"], o["dst"], complete_params(variant))
        assert ctx.last_path() == complete_paths(variant)[0], ctx.last_path()
        if variant == "off_grid":
            # the 16-bit attempt failed and the gated f32 rerun gave the result; the context has seen it: its next call goes
            # straight to the f32 kernels, as a launch of k_fp_s of its own
            torch.cuda.synchronize()
            first = o["dst"].clone()
            fill_sentinel(o["dst"])
            ctx.complete_dev(t["src"], o["dst"], complete_params(variant))
            assert ctx.last_path() == complete_paths(variant)[1], ctx.last_path()
            torch.cuda.synchronize()
            assert torch.equal(first.view(torch.int32), o["dst"].view(torch.int32)), "the gated rerun and k_fp_s differ"

    def after(ctx, ref, lay):
        if not loop and variant != "no_extrapolate":
            return
        iters, st = ctx.last_fill_iters(g.batch)
        holes = ctx.last_holes_after_extend(g.batch)
        if variant == "no_extrapolate":
            assert st == L.OK and not any(iters) and not any(holes)
            return
        want_i = np.array(ref["_iters"])[lay.index]
        assert st == L.OK and np.array_equal(np.array(iters), want_i), (name, [(f, iters[f], int(want_i[f])) for f in np.flatnonzero(np.array(iters) != want_i)[:8]])
        want_h = np.array(ref["_holes"])[lay.index]
        assert np.array_equal(np.array(holes), want_h), (name, [(f, holes[f], int(want_h[f])) for f in np.flatnonzero(np.array(holes) != want_h)[:8]])

    case = FrameCase(name, g, (4,), sources, reference, {"dst": ((g.rows, g.cols), f32)}, call, None, after,
                     scratch={"default": 2 * g.total_px, "off_grid": 2 * g.total_px + 4 * g.total_px, "bilateral_clone": 4 * g.total_px,
                              "force_staged": 2 * 4 * g.cols * ((g.rows + 15) // 16) * g.batch}.get(variant, 0))
    if variant == "bilateral_clone":
        case.bounds = {"dst": lambda got, src, lay: bound_f64(name, case.prepare()[2]["_f64"])(got, src, lay)}
    return case


def complete_u16_case(g, seed=300, staged=False):
    """staged: DCMT_FLAG_FORCE_STAGED, where the payload is converted by k_u16_to_f32, a flat run over the whole batch."""
    name = f"complete_u16_dev {'force_staged ' if staged else ''}{g.name}"

    def sources(lay):
        return {"src": np.round(sparse_sources(lay, seed) * 256.0).astype(np.uint16).view(np.int16)}

    def reference(src, lay):
        res = [O().img_completion((x.view(np.uint16).astype(f32) * f32(1.0 / 256.0)).astype(f32), return_info=True) for x in src["src"]]
        return {"dst": stack([r[0] for r in res]), "_iters": [r[1]["fill_iters"] for r in res]}

    def call(ctx, t, o, lay):
        ctx.complete_u16_dev(t["src"], 1.0 / 256.0, o["dst"], api.make_params(spec_fill_iters=SPEC, force_staged=staged))
        assert ctx.last_path() == (complete_paths("force_staged")[0] if staged else "k_pre_p<U16,Q16OUT> + k_fp_q"), ctx.last_path()

    def after(ctx, ref, lay):
        iters, st = ctx.last_fill_iters(g.batch)
        assert st == L.OK and np.array_equal(np.array(iters), np.array(ref["_iters"])[lay.index])

    # scratch: the 16-bit plane, or the staged kernels' column statistics (two ints per column and tile row, tiles of 16 rows or more)
    return FrameCase(name, g, (4, 2), sources, reference, {"dst": ((g.rows, g.cols), f32)}, call, None, after,
                     scratch=2 * 4 * g.cols * ((g.rows + 15) // 16) * g.batch if staged else 2 * g.total_px)


def labeled_case(g, kind, seed=400):
    """kind "lds": few enough labels that k_label_bbox keeps its boxes in LDS; "global": a label count beyond that (16 bytes per
    label in 48 KiB: 3072); "synth": synth.synth_labels at the production shape."""
    name = f"complete_dev labels {kind} {g.name}"
    if kind == "synth":
        n_labels = synth.synth_labels(g.rows, g.cols, 1200, 0)[1]
    else:
        n_labels = 40 if kind == "lds" else 3500

    def sources(lay):
        if kind == "synth":
            lab = stack([synth.synth_labels(g.rows, g.cols, 1200, 7 + s)[0] for s in range(lay.n_src)])
        else:
            # a jittered grid whose cells carry labels spread over [0, n_labels), some pixels unlabeled
            lab = stack([synth.synth_labels(g.rows, g.cols, 40, 7 + s)[0] for s in range(lay.n_src)])
            n_grid = synth.synth_labels(g.rows, g.cols, 40, 0)[1]
            if kind == "global":
                lab = np.where(lab >= 0, lab * ((n_labels - 1) // max(n_grid - 1, 1)), -1).astype(np.int32)
            else:
                lab = np.where(lab >= n_labels, -1, lab).astype(np.int32)
        assert lab.max() < n_labels
        return {"src": sparse_sources(lay, seed), "labels": lab.astype(np.int32)}

    def reference(src, lay):
        res = [O().interpolate_with_superpixels(x, lab, n_labels, return_info=True) for x, lab in zip(src["src"], src["labels"])]
        for s, (_, info) in enumerate(res):
            assert info["rc"] == 0 and info["fill_iters"] < SPEC, (name, s, info)
        return {"dst": stack([r[0] for r in res]), "_iters": [r[1]["fill_iters"] for r in res]}

    def call(ctx, t, o, lay):
        ctx.complete_dev(t["src"], o["dst"], api.make_params(spec_fill_iters=SPEC), d_labels=t["labels"], n_labels=n_labels)
        assert ctx.last_path().startswith("k_label_bbox + k_label_stage + k_pre_p"), ctx.last_path()

    def after(ctx, ref, lay):
        iters, st = ctx.last_fill_iters(g.batch)
        assert st == L.OK and np.array_equal(np.array(iters), np.array(ref["_iters"])[lay.index])

    return FrameCase(name, g, (4,), sources, reference, {"dst": ((g.rows, g.cols), f32)}, call, None, after,
                     scratch=2 * g.total_px + 2 * 4 * 2 * g.batch * n_labels)


# ---------------------------------------------------------------------------------------------------------------- per-pixel entry points
def gaussian_case(g):
    def sources(lay):
        return {"src": (np.random.default_rng(40).standard_normal((lay.n_src, g.rows, g.cols)) * 20.0).astype(f32)}

    return FrameCase(f"gaussian5_dev {g.name}", g, (4,), sources, lambda src, lay: {"dst": stack([O().gaussian5(x) for x in src["src"]])},
                     {"dst": ((g.rows, g.cols), f32)}, lambda ctx, t, o, lay: ctx.gaussian5_dev(t["src"], o["dst"]))


def bilateral_case(g):
    import bilateral_restatement as BR
    name = f"bilateral5_dev {g.name}"

    def sources(lay):
        rng = np.random.Generator(np.random.PCG64(1000 * g.rows + g.cols))
        yy, xx = np.mgrid[0:g.rows, 0:g.cols]
        out = []
        for s in range(lay.n_src):       # tests/test_gpu_bilateral.py's three kinds of plane, in turn
            kind = s % 3
            out.append(30.0 + 0.4 * xx + 0.7 * yy + rng.normal(0.0, 1.0, xx.shape) if kind == 0 else
                       20.0 + 3.0 * ((xx // 5 + yy // 3) % 4) + rng.normal(0.0, 0.3, xx.shape) if kind == 1 else rng.uniform(-20.0, 100.0, xx.shape))
        return {"src": stack(out).astype(f32)}

    def reference(src, lay):
        w = stack([BR.restatement_f64(x) for x in src["src"]])
        return {"dst": w.astype(f32), "_f64": w}

    case = FrameCase(name, g, (4,), sources, reference, {"dst": ((g.rows, g.cols), f32)}, lambda ctx, t, o, lay: ctx.bilateral5_dev(t["src"], o["dst"]))
    case.bounds = {"dst": lambda got, src, lay: bound_f64(name, case.prepare()[2]["_f64"])(got, src, lay)}
    return case


def depth_to_u16_case(g):
    import crop_restatement as CR

    def sources(lay):
        x = dense_sources(lay, 61, 0.0, 300.0)
        x[:, 0, :9] = np.array(CR.EXPORT_PROBES, f32)
        return {"depth": x}

    px_marks = (SEG_PX, P31)
    return FrameCase(f"depth_to_u16_dev {g.name}", g, (4, 2), sources, lambda src, lay: {"out": stack([CR.depth_to_u16(x) for x in src["depth"]]).view(np.int16)},
                     {"out": ((g.rows, g.cols), np.int16)}, lambda ctx, t, o, lay: ctx.depth_to_u16_dev(t["depth"], 256.0, o["out"]), px_marks=px_marks)


def colorize_case(g):
    import test_colorize as TC

    def sources(lay):
        base = synth.synth_batch(lay.n_src, g.rows, g.cols, 70)
        rng = np.random.default_rng(71)
        out = np.empty_like(base)
        for s in range(lay.n_src):       # test_colorize.frames_for's kinds, without the constant frame (its image is one colour)
            kind = s % 5
            out[s] = (base[s] if kind == 0 else base[s] + f32(0.37) if kind == 1 else base[s] * f32(3.0) - f32(40.0) if kind == 2 else
                      f32(50.0) + (rng.random((g.rows, g.cols)) * 1e-3).astype(f32) if kind == 3 else base[s] * f32(1e4) + f32(1.0))
        return {"src": out}

    seg = color_seg_frames(g)
    return FrameCase(f"colorize_dev {g.name}", g, (4, 3), sources, lambda src, lay: {"bgr": stack([TC.np_colorize(x) for x in src["src"]])},
                     {"bgr": ((g.rows, g.cols, 3), np.uint8)}, lambda ctx, t, o, lay: ctx.colorize_dev(t["src"], o["bgr"]),
                     px_marks=(seg * g.px, P31) if seg < g.batch else (P31,))


def bgr_convert_case(g):
    import bgr_restatement as BG

    def sources(lay):
        return {"bgr": np.random.default_rng(700).integers(0, 256, (lay.n_src, g.rows, g.cols, 3), dtype=np.uint8)}

    def reference(src, lay):
        return {"lab": stack([BG.bgr_to_lab(x) for x in src["bgr"]]), "gray": stack([BG.bgr_to_gray(x) for x in src["bgr"]])}

    return FrameCase(f"bgr_convert_dev lab + grey {g.name}", g, (3, 1), sources, reference,
                     {"lab": ((g.rows, g.cols, 3), np.uint8), "gray": ((g.rows, g.cols), np.uint8)},
                     lambda ctx, t, o, lay: ctx.bgr_convert_dev(t["bgr"], d_lab=o["lab"], d_gray=o["gray"]), px_marks=(SEG_PX, P31))


def evaluate_case(g, u16):
    """The sums have the project's stated bound against math.fsum (tests/test_evaluate.py: check_sums); the counts are exact."""
    import test_evaluate as TE
    name = f"evaluate_dev {'uint16' if u16 else 'f32'} ground truth {g.name}"

    def sources(lay):
        rng = np.random.default_rng(500)
        pred = dense_sources(lay, 510)
        gt = np.where(rng.random(pred.shape) < 0.3, pred + rng.normal(0, 1.5, pred.shape), 0.0).clip(0, 200)
        gt = np.round(gt * 256.0).astype(np.uint16)
        return {"gt": gt.view(np.int16) if u16 else (gt.astype(f32) / f32(256.0)).astype(f32), "pred": pred}

    def gt_of(x):
        return (x.view(np.uint16).astype(f32) * f32(1.0 / 256.0)).astype(f32) if u16 else x

    def reference(src, lay):
        # for the distinctness check: the counts and the fsum of the absolute error differ between the sources
        rows = []
        for gt, pred in zip(src["gt"], src["pred"]):
            n, t3, n_inv, t2 = TE.np_terms(gt_of(gt), pred, 0.0, "both")
            rows.append([n, float(t3[0].astype(np.float64).sum()), float(t3[1].astype(np.float64).sum()), float(t3[2].astype(np.float64).sum()),
                         n_inv, float(t2[0].sum()), float(t2[1].sum())])
        return {"sums": np.array(rows, np.float64)}

    def check(got, src, lay):
        for s in range(lay.n_src):
            TE.check_sums(got[s], gt_of(src["gt"][s]), src["pred"][s], 0.0, "both", f"{name}: source {s}")

    return FrameCase(name, g, (4, 2) if u16 else (4,), sources, reference, {"sums": ((7,), np.float64)},
                     lambda ctx, t, o, lay: ctx.evaluate_dev(t["gt"], t["pred"], 0.0, "both", d_out=o["sums"]), {"sums": check},
                     scratch=0)


# ---------------------------------------------------------------------------------------------------------------- stereo, reprojection
def stereo_case(g, calib):
    name = f"stereo_refine{'_calib' if calib else ''}_dev {g.name}"

    def recs(lay):
        return [dict(baseline=0.54 * (1 + 0.05 * (s % 4)), focal=80.0 * (1 + 0.1 * (s % 3))) if calib else dict(baseline=0.54, focal=80.0) for s in range(lay.n_src)]

    def sources(lay):
        l, r, d = zip(*[synth.synth_stereo(g.rows, g.cols, 70 + s, focal=80.0) for s in range(lay.n_src)])
        return {"depth": stack(d), "left": stack(l), "right": stack(r)}

    def reference(src, lay):
        rec = recs(lay)
        return {"out": stack([O().stereo_refine(src["depth"][s], src["left"][s], src["right"][s], iterations=4, **rec[s]) for s in range(lay.n_src)])}

    def tables(lay):
        if not calib:
            return {}
        rec = recs(lay)
        return {"table": api.calib_to_device(api.make_stereo_calib(np.array([r["baseline"] for r in rec])[lay.index], np.array([r["focal"] for r in rec])[lay.index]))}

    def call(ctx, t, o, lay):
        if calib:
            ctx.stereo_refine_calib_dev(t["depth"], t["left"], t["right"], t["table"], o["out"], iterations=4)
        else:
            ctx.stereo_refine_dev(t["depth"], t["left"], t["right"], o["out"], iterations=4, focal=80.0)

    return FrameCase(name, g, (4, 1), sources, reference, {"out": ((g.rows, g.cols), f32)}, call, tables=tables)


def reproject_case(g, calib, nearest):
    import calib_cases as CC
    import nearest_restatement as NR
    from test_reproject import np_reproject
    name = f"reproject_depth{'_nearest' if nearest else ''}{'_calib' if calib else ''}_dev {g.name}"
    n_rec = 3

    def records():
        return CC.reproject_records(n_rec, g.rows, g.cols, g.rows, g.cols)

    def rec_of(s):
        return s % n_rec if calib else 1

    def sources(lay):
        return {"depth": CC.depth_frames(lay.n_src, g.rows, g.cols, 900)}

    def reference(src, lay):
        M, K, kw = records()
        out = []
        for s, d in enumerate(src["depth"]):
            r = rec_of(s)
            out.append(NR.reproject_frame(d, g.rows, g.cols, dict(M=M[r], K=K[r], **kw[r])) if nearest else np_reproject(d, g.rows, g.cols, M=M[r], K=K[r], **kw[r]))
        return {"out": stack(out)}

    def tables(lay):
        if not calib:
            return {}
        M, K, kw = records()
        r = lay.index % n_rec
        return {"table": api.calib_to_device(api.make_reproject_calib(M[r], K[r], *[np.array([k[n] for k in kw])[r] for n in ("fx", "fy", "cx", "cy")]))}

    def call(ctx, t, o, lay):
        if calib:
            ctx.reproject_depth_calib_dev(t["depth"], g.rows, g.cols, t["table"], o["out"], nearest=nearest)
        else:
            M, K, kw = records()
            ctx.reproject_depth_dev(t["depth"], g.rows, g.cols, api.make_reproject_params(M=M[1], K=K[1], **kw[1]), o["out"], nearest=nearest)

    return FrameCase(name, g, (4,), sources, reference, {"out": ((g.rows, g.cols), f32)}, call, tables=tables, scratch=0 if nearest else 4 * g.total_px)


# ---------------------------------------------------------------------------------------------------------------- stereo matching
SGM_D, SGM_SLOTS = 16, 4096          # disparities; frames the workspace holds
SGM_KW = dict(num_disparities=SGM_D, focal=80.0)        # baseline * focal = 43.2: no disparity from 1 px on is clamped to max_depth


def sgm_figures(g):
    """The chunking of dcmt_sgm_dev at SGM_D disparities through a workspace of SGM_SLOTS frames (plan_sgm, csrc/dcmt_sgm.h), restated:
    (bytes of one frame's two volumes, chunks, frames of the last chunk, the slot that holds byte 2^32 of the workspace)."""
    one = 4 * g.px * SGM_D
    n_chunks = -(-g.batch // SGM_SLOTS)
    return one, n_chunks, g.batch - (n_chunks - 1) * SGM_SLOTS, P32 // one


def check_sgm_figures():
    one, n_chunks, last, slot = sgm_figures(A)
    assert one == 1_081_344 and SGM_SLOTS * one == 4_429_185_024 > P32 and (n_chunks, last) == (16, 4095)
    assert slot == 3971 and slot * one < P32 < (slot + 1) * one and slot + 1 < last         # the boundary lies inside slot 3971, in every chunk
    assert 2 * A.total_px > P31 and 4 * A.total_px > P32                                  # disp16 passes 2^31 bytes, depth 2^32


check_sgm_figures()


def sgm_extra_frames(g):
    """Beside the plane boundaries: in the first, a middle and the last chunk the frames whose slots hold byte 2^32 of the workspace
    and the slot behind it, and both sides of the first, a middle and the last chunk seam."""
    one, n_chunks, last, slot = sgm_figures(g)
    chunks = (0, n_chunks // 2, n_chunks - 1)
    frames = [c * SGM_SLOTS + s for c in chunks for s in (slot, slot + 1)]
    frames += [c * SGM_SLOTS + e for c in (1, n_chunks // 2, n_chunks - 1) for e in (-1, 0)]
    assert all(0 <= f < g.batch for f in frames) and len(set(frames)) == 12
    return frames


def sgm_case(g):
    """dcmt_sgm_dev, both outputs: the chunk loop's offsets into four planes, a workspace that passes 2^32 bytes itself, frames in
    grid y.  Sources: shifted pairs, exact and half in turn, every one with a seed and (in turn) a shift of its own."""
    import sgm_restatement as SR
    name = f"sgm_dev {g.name}"
    one = sgm_figures(g)[0]
    assert api.sgm_workspace_bytes(g.rows, g.cols, SGM_D, 1) == one

    def sources(lay):
        pairs = [SR.shifted_pair(g.rows, g.cols, 2600 + s, 1 + s % 14, half=s % 2 == 1) for s in range(lay.n_src)]
        return {"left": stack([p[0] for p in pairs]), "right": stack([p[1] for p in pairs])}

    def reference(src, lay):
        res = [SR.vectorised(l, r, **SGM_KW) for l, r in zip(src["left"], src["right"])]
        return {"disp16": stack([r[0] for r in res]), "depth": stack([r[1] for r in res])}

    def call(ctx, t, o, lay):
        import torch
        work = torch.empty(SGM_SLOTS * one, dtype=torch.uint8, device="cuda")
        assert work.numel() > P32
        ctx.sgm_dev(t["left"], t["right"], d_disp16=o["disp16"], d_depth=o["depth"], d_work=work, **SGM_KW)

    return FrameCase(name, g, (1, 2, 4), sources, reference, {"disp16": ((g.rows, g.cols), np.int16), "depth": ((g.rows, g.cols), f32)}, call,
                     scratch=SGM_SLOTS * one, extra=sgm_extra_frames(g))


# ---------------------------------------------------------------------------------------------------------------- SLIC
SLIC_STEP, SLIC_NC = 16, 40


def lab_sources(lay):
    g = lay.g
    return stack([synth.synth_lab(g.rows, g.cols, 40 + s) for s in range(lay.n_src)])


_slic = {}


def slic_of(lay):
    """(labels [n_src][rows][cols], n_centers, centres [n_src][n][5]) of lab_sources, from the oracle; shared by the SLIC cases."""
    key = (lay.g.name, lay.n_src)
    if key not in _slic:
        res = [O().slic(x, SLIC_STEP, SLIC_NC, return_centers=True) for x in lab_sources(lay)]
        assert all(r[1] == res[0][1] for r in res)
        _slic[key] = (stack([r[0] for r in res]), res[0][1], stack([r[2] for r in res]))
    return _slic[key]


def slic_labels_case(g):
    name = f"slic_labels_dev {g.name}"

    def reference(src, lay):
        labels, n, cent = slic_of(lay)
        return {"labels": labels, "centers": cent}

    def check_centres(got, src, lay):
        want = slic_of(lay)[2]
        live = ~np.isnan(want)                   # a centre that owns no pixel: the oracle's value is NaN and nothing is compared
        assert got.shape == want.shape and np.array_equal(got.view(np.uint64)[live], want.view(np.uint64)[live]), name

    def call(ctx, t, o, lay):
        n = slic_of(lay)[1]
        labels, n_dev, cent = ctx.slic_labels_dev(t["lab"], SLIC_STEP, SLIC_NC, o["labels"], return_centers=True)
        assert n_dev == n
        o["centers"] = cent.contiguous()

    n = L.lib().dcmt_slic_num_centers(g.rows, g.cols, SLIC_STEP)
    case = FrameCase(name, g, (3, 4), lambda lay: {"lab": lab_sources(lay)}, reference, {"labels": ((g.rows, g.cols), np.int32)}, call,
                     labels=("labels",),
                     scratch=g.batch * (8 * (2 * 5 + 6) * n + 4 * 2 * (5 * ((g.cols - 1) // SLIC_STEP + 1) * ((g.rows - 1) // SLIC_STEP + 1) + 1)))
    case.outputs["centers"] = ((n, 5), np.float64)
    case.bounds = {"centers": check_centres}
    return case


def connectivity_case(g):
    import connectivity_restatement as CN

    def sources(lay):
        return {"labels": slic_of(lay)[0]}

    def reference(src, lay):
        n = slic_of(lay)[1]
        res = [CN.components(x, n) for x in src["labels"]]
        return {"out": stack([r[0] for r in res]), "counts": np.array([r[1] for r in res], np.int32)}

    def call(ctx, t, o, lay):
        ctx.slic_connectivity_dev(t["labels"], slic_of(lay)[1], o["out"], o["counts"])

    return FrameCase(f"slic_connectivity_dev {g.name}", g, (4,), sources, reference, {"out": ((g.rows, g.cols), np.int32), "counts": ((), np.int32)}, call,
                     labels=("out",), aux=("counts",))


def contours_case(g):
    import contours_restatement as CT

    def sources(lay):
        return {"labels": slic_of(lay)[0], "bgr": stack([CT.image_for(g.rows, g.cols, s) for s in range(lay.n_src)])}

    def reference(src, lay):
        masks = [CT.closed_contours(x) for x in src["labels"]]
        return {"mask": stack(masks), "bgr": stack([CT.paint(img, m) for img, m in zip(src["bgr"], masks)])}

    return FrameCase(f"slic_contours_dev {g.name}", g, (4, 3, 1), sources, reference, {"mask": ((g.rows, g.cols), np.uint8), "bgr": ((g.rows, g.cols, 3), np.uint8)},
                     lambda ctx, t, o, lay: ctx.slic_contours_dev(t["labels"], t["bgr"], d_mask=o["mask"]))


def cluster_means_case(g):
    import contours_restatement as CT

    def sources(lay):
        return {"labels": slic_of(lay)[0], "bgr": stack([CT.image_for(g.rows, g.cols, s) for s in range(lay.n_src)])}

    def reference(src, lay):
        n = slic_of(lay)[1]
        res = [CT.closed_means(x, img, n) for x, img in zip(src["labels"], src["bgr"])]
        return {"bgr": stack([r[0] for r in res]), "sums": stack([r[1] for r in res])}

    n = L.lib().dcmt_slic_num_centers(g.rows, g.cols, SLIC_STEP)
    return FrameCase(f"slic_cluster_means_dev {g.name}", g, (4, 3), sources, reference, {"bgr": ((g.rows, g.cols, 3), np.uint8), "sums": ((n, 4), np.int32)},
                     lambda ctx, t, o, lay: ctx.slic_cluster_means_dev(t["labels"], slic_of(lay)[1], t["bgr"], o["sums"]))


# ---------------------------------------------------------------------------------------------------------------- projection
class ProjectCase:
    """dcmt_project_points*_dev: the unique frames and a handful of tiled ones have a sweep of points, every other sweep is empty
    and its plane must come out zero.  Source 0 is the empty sweep; source 1 + j is sweep j."""

    def __init__(self, g, calib, nearest):
        self.g, self.calib, self.nearest = g, calib, nearest
        self.name = f"project_points{'_nearest' if nearest else ''}{'_calib' if calib else ''}_dev {g.name}"
        self._prep = None

    def prepare(self):
        if self._prep is None:
            import nearest_restatement as NR
            g = self.g
            lay = Layout(g, (4,))
            with_points = sorted(set(lay.unique) | {1, 2, 7, g.batch // 2, g.batch - 2})
            n_sw = len(with_points)
            T = synth.KITTI_T_VELO_TO_CAM
            P = [np.array([[60.0 + 3 * j, 0, g.cols / 2, 3.0], [0, 60.0, g.rows / 2, 0.01], [0, 0, 1, 0.002]], f32) if self.calib else
                 np.array([[60.0, 0, g.cols / 2, 3.0], [0, 60.0, g.rows / 2, 0.01], [0, 0, 1, 0.002]], f32) for j in range(n_sw)]
            sweeps = [synth.synth_points(600 + 37 * j, 300 + j) for j in range(n_sw)]
            rule = (lambda p, Pm: NR.project_frame(p, T, Pm, g.rows, g.cols)) if self.nearest else (lambda p, Pm: O().project_points(p, T, Pm, g.rows, g.cols))
            exp = stack([np.zeros((g.rows, g.cols), f32)] + [rule(sweeps[j], P[j]) for j in range(n_sw)])
            for j in range(n_sw):
                assert np.count_nonzero(exp[1 + j]) > 20, (self.name, j)
            assert len({e.tobytes() for e in exp}) == len(exp), f"{self.name}: two sweeps have the same expectation"
            index = np.zeros(g.batch, np.int64)
            index[with_points] = 1 + np.arange(n_sw)
            counts = np.zeros(g.batch, np.int64)
            counts[with_points] = [len(s) for s in sweeps]
            offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
            self._prep = dict(index=index, exp=exp, points=np.concatenate(sweeps), offsets=offsets, T=T, P=P, with_points=with_points)
        return self._prep

    def need_bytes(self):
        g = self.g
        return 2 * 4 * g.total_px + 4 * g.total_px + (0 if self.nearest else 4 * g.total_px) + (1 << 30)

    def run(self):
        import torch
        p, g = self.prepare(), self.g
        need = self.need_bytes()
        check_memory(self.name, need)
        torch.cuda.reset_peak_memory_stats()
        tm = Timer()
        with api.Context(0, g.rows, g.cols, g.batch) as ctx:
            tm.phase("context")
            out = sentinel((g.batch, g.rows, g.cols), torch.float32)
            pts, off = dev(p["points"]), dev(p["offsets"])
            tm.phase("fill")
            if self.calib:
                Tb = np.broadcast_to(p["T"], (g.batch, 4, 4))
                Pb = np.stack([p["P"][0]] + p["P"])[p["index"]]            # (an empty sweep's record is never applied to a point)
                ctx.project_points_calib_dev(pts, off, api.calib_to_device(api.make_project_calib(Tb, Pb)), g.rows, g.cols, out, nearest=self.nearest)
            else:
                ctx.project_points_dev(pts, off, p["T"], p["P"][0], g.rows, g.cols, out, nearest=self.nearest)
            tm.phase("call")
            assert_frames(self.name, out, dev(p["exp"]), dev(p["index"]))
            tm.phase("compare")
        report(self.name, need, tm)


# ---------------------------------------------------------------------------------------------------------------- point cloud
class CloudCase:
    """dcmt_depth_to_cloud*_dev: the records are packed in batch order, so the expectation of the whole output is built from the
    per-source records: offsets = the host's cumulative sum of the per-source counts, and record j of frame f is record j of
    frame f's source.  Rows behind offsets[batch] must keep the sentinel."""

    def __init__(self, g, calib):
        self.g, self.calib = g, calib
        self.name = f"depth_to_cloud{'_calib' if calib else ''}_dev {g.name}"
        self._prep = None

    def recs(self, n):
        g = self.g
        return [dict(fx=0.9 * g.cols * (1 + 0.2 * (s % 3)), fy=0.8 * g.rows * (1 + 0.3 * (s % 3)), cx=g.cols / 2 + 0.5 * (s % 3), cy=g.rows / 2 - 0.25 * (s % 3))
                if self.calib else dict(fx=0.9 * g.cols, fy=0.8 * g.rows, cx=g.cols / 2, cy=g.rows / 2) for s in range(n)]

    def prepare(self):
        if self._prep is None:
            from test_cloud import np_cloud, words as rec_words
            g = self.g
            lay = Layout(g, (4, 3))
            depth = sparse_sources(lay, 800, gap=False)                      # about 4 % valid: the packed records stay far below 2 GB
            bgr = None if self.calib else np.random.default_rng(810).integers(0, 256, (lay.n_src, g.rows, g.cols, 3), dtype=np.uint8)
            rec = self.recs(lay.n_src)
            recs = [rec_words(np_cloud(depth[s], None if bgr is None else bgr[s], **rec[s])) for s in range(lay.n_src)]
            counts = np.array([len(r) for r in recs], np.int64)
            assert len({r.tobytes() for r in recs}) == lay.n_src and (counts == 0).sum() == 1
            offsets = np.concatenate([[0], np.cumsum(counts[lay.index])])
            assert offsets[-1] * 16 < P31 and offsets[-1] < 2 ** 31
            self._prep = dict(lay=lay, depth=depth, bgr=bgr, rec=rec, recs=recs, counts=counts, offsets=offsets.astype(np.int32))
        return self._prep

    def need_bytes(self):
        p, g = self.prepare(), self.g
        return 2 * 4 * g.total_px + 4 * g.total_px + (0 if self.calib else 3 * g.total_px) + 16 * int(p["offsets"][-1]) + (2 << 30)

    def run(self):
        import torch
        p, g = self.prepare(), self.g
        lay = p["lay"]
        need = self.need_bytes()
        check_memory(self.name, need)
        torch.cuda.reset_peak_memory_stats()
        tm = Timer()
        total, slack = int(p["offsets"][-1]), 4096
        index = dev(lay.index)
        with api.Context(0, g.rows, g.cols, g.batch) as ctx:
            tm.phase("context")
            depth = dev(p["depth"])[index]
            bgr = None if p["bgr"] is None else dev(p["bgr"])[index]
            points = sentinel((total + slack, 4), torch.float32)
            offsets = sentinel((g.batch + 1,), torch.int32)
            tm.phase("tile and fill")
            if self.calib:
                rec = p["rec"]
                table = api.make_cloud_calib(*[np.array([r[n] for r in rec])[lay.index] for n in ("fx", "fy", "cx", "cy")])
                ctx.depth_to_cloud_calib_dev(depth, api.calib_to_device(table), None, points, offsets, capacity=total + slack)
            else:
                ctx.depth_to_cloud_dev(depth, bgr, api.make_cloud_params(**p["rec"][0]), points, offsets, capacity=total + slack)
            tm.phase("call")
            got_off = offsets.cpu().numpy()
            bad = np.flatnonzero(got_off != p["offsets"])
            assert not len(bad), f"{self.name}: offsets differ from the host's cumulative sum, first at frame {bad[0]}: {got_off[bad[0]]} vs {p['offsets'][bad[0]]}"
            # expected row j: frame f = the frame whose range holds j, record j - offsets[f] of source index[f]
            flat = dev(np.concatenate([r for r in p["recs"] if len(r)]).view(np.int32))
            start = dev(np.concatenate([[0], np.cumsum(p["counts"])[:-1]]))
            off64 = dev(p["offsets"].astype(np.int64))
            got = points.view(torch.int32)
            step = 8 << 20
            for s in range(0, total, step):
                e = min(total, s + step)
                j = torch.arange(s, e, device="cuda")
                f = torch.searchsorted(off64, j, right=True) - 1
                want = flat[start[index[f]] + (j - off64[f])]
                neq = (got[s:e] != want).any(dim=1)
                if bool(neq.any()):
                    r = int(torch.nonzero(neq)[0]) + s
                    raise AssertionError(f"{self.name}: record {r} (frame {int(f[r - s])}) differs: {got[r].tolist()} vs {want[r - s].tolist()}")
            tail = points[total:].cpu().numpy()
            assert is_sentinel_frame(tail), f"{self.name}: rows behind offsets[batch] were written"
            tm.phase("compare")
        report(self.name, need, tm)


# ---------------------------------------------------------------------------------------------------------------- ragged crop
class CropCase:
    """dcmt_crop_frames_dev: ragged sources packed back to back in one buffer of more than 2^32 bytes, so that the records hold
    offsets above 2^32.  A frame's size and window origin follow f % K (a unique source has the size of the tiled one it replaces),
    so the buffer is K frames repeated, built on the device, with the unique frames' bytes written over it."""

    def __init__(self, g, elem):
        self.g, self.elem = g, elem
        self.name = f"crop_frames_dev {elem} B elements {g.name}"
        self._prep = None

    def prepare(self):
        if self._prep is None:
            import crop_restatement as CR
            g, elem, k = self.g, self.elem, K_TILED
            grow = 1 if elem == 4 else 160                                   # 1-byte elements: frames large enough to pass 2^32 bytes
            sizes = [(g.rows + grow + 2 * i, g.cols + grow + 3 * ((i * 2) % k)) for i in range(k)]
            origins = [(i % (sizes[i][0] - g.rows + 1), (2 * i + 1) % (sizes[i][1] - g.cols + 1)) for i in range(k)]
            nbytes = np.array([r * c * elem for r, c in sizes], np.int64)
            kind = np.arange(g.batch) % k
            offsets = np.concatenate([[0], np.cumsum(nbytes[kind])])
            src_bytes = int(offsets[-1])
            assert src_bytes > P32 and g.batch % k == 0
            # the frames that hold byte 2^31 and 2^32 of the SOURCE buffer and of the output get a unique source, and their neighbours
            marks = set()
            for pos in (P31, P32):
                h = int(np.searchsorted(offsets, pos, side="right")) - 1
                marks.update(f for f in (h - 1, h, h + 1) if 0 <= f < g.batch)
            lay = Layout(g, (elem,), extra=marks)
            frames = [CR.noise(sizes[int(kind[lay.reps[s]])] + ((elem,) if elem > 1 else ()), np.uint8, 50 + s) for s in range(lay.n_src)]
            exp = []
            for s, fr in enumerate(frames):
                (y0, x0) = origins[int(kind[lay.reps[s]])]
                exp.append(fr.reshape(fr.shape[0], -1)[y0:y0 + g.rows, x0 * elem:(x0 + g.cols) * elem])
            exp = stack(exp)
            assert_distinct(self.name, exp)
            table = np.zeros(g.batch, api.CROP_SRC_DTYPE)
            table["offset"] = offsets[:-1]
            table["rows"], table["cols"] = np.array(sizes)[kind].T
            table["row_stride"] = table["cols"] * elem
            table["y0"], table["x0"] = np.array(origins)[kind].T
            assert int(table["offset"].max()) > P32
            # the restatement's record test on the records of the frames a unique source sits at
            for f in lay.unique:
                assert CR.record_ok(table[f], elem, g.rows, g.cols, src_bytes), f
            self._prep = dict(lay=lay, frames=frames, exp=exp, table=table, offsets=offsets, src_bytes=src_bytes, nbytes=nbytes)
        return self._prep

    def need_bytes(self):
        p, g = self.prepare(), self.g
        return 2 * 4 * g.total_px + p["src_bytes"] + g.total_px * self.elem + (1 << 30)

    def run(self):
        import torch
        p, g, k = self.prepare(), self.g, K_TILED
        lay = p["lay"]
        need = self.need_bytes()
        check_memory(self.name, need)
        torch.cuda.reset_peak_memory_stats()
        tm = Timer()
        with api.Context(0, g.rows, g.cols, g.batch) as ctx:
            tm.phase("context")
            block = torch.cat([dev(p["frames"][s].reshape(-1)) for s in range(k)])
            src = block.repeat(g.batch // k)
            assert src.numel() == p["src_bytes"]
            for s in range(k, lay.n_src):
                at = int(p["offsets"][lay.reps[s]])
                fr = dev(p["frames"][s].reshape(-1))
                src[at:at + fr.numel()] = fr
            dst = sentinel((g.batch, g.rows, g.cols * self.elem), torch.uint8)
            tm.phase("tile and fill")
            ctx.crop_frames_dev(src, api.calib_to_device(p["table"]), g.rows, g.cols, elem_bytes=self.elem, d_dst=dst)
            tm.phase("call")
            assert_frames(self.name, dst, dev(p["exp"]), dev(lay.index))
            tm.phase("compare")
        report(self.name, need, tm)


# ---------------------------------------------------------------------------------------------------------------- the refusal
class CloudRefusalCase:
    """dcmt_depth_to_cloud_dev states a limit of INT32_MAX pixels per call: beyond it the call must answer DCMT_E_INVALID and leave
    its outputs as they were."""

    def __init__(self, g):
        self.g, self.name = g, f"depth_to_cloud_dev refuses {g.name}"

    def prepare(self):
        assert self.g.total_px > 2 ** 31 - 1
        return {}

    def need_bytes(self):
        return 2 * 4 * self.g.total_px + 4 * self.g.total_px + (1 << 30)

    def run(self):
        import torch
        g = self.g
        need = self.need_bytes()
        check_memory(self.name, need)
        tm = Timer()
        with api.Context(0, g.rows, g.cols, g.batch) as ctx:
            depth = torch.ones((g.batch, g.rows, g.cols), dtype=torch.float32, device="cuda")
            points = sentinel((1 << 16, 4), torch.float32)
            offsets = sentinel((g.batch + 1,), torch.int32)
            try:
                ctx.depth_to_cloud_dev(depth, None, None, points, offsets, capacity=1 << 16)
            except api.DcmtError as e:
                assert e.status == L.E_INVALID, e
            else:
                raise AssertionError(f"{self.name}: a batch of {g.total_px} pixels was accepted")
            torch.cuda.synchronize()
            assert is_sentinel_frame(points.cpu().numpy()) and is_sentinel_frame(offsets.cpu().numpy()), f"{self.name}: a refused call wrote its outputs"
            tm.phase("all")
        report(self.name, need, tm)


# ---------------------------------------------------------------------------------------------------------------- the table
_cases = {}


def cases():
    """Every case, by name, built once (building is cheap: inputs and expectations are made by prepare())."""
    if not _cases:
        made = [complete_case(A, v) for v in COMPLETE_VARIANTS]
        made += [complete_u16_case(A), labeled_case(A, "lds"), labeled_case(A, "global")]
        made += [ProjectCase(A, calib, nearest) for nearest in (False, True) for calib in (False, True)]
        made += [slic_labels_case(A), connectivity_case(A), contours_case(A), cluster_means_case(A)]
        made += [stereo_case(A, False), stereo_case(A, True), evaluate_case(A, False), evaluate_case(A, True), colorize_case(A)]
        made += [CloudCase(A, False), CloudCase(A, True), gaussian_case(A), bilateral_case(A)]
        made += [reproject_case(A, calib, nearest) for nearest in (False, True) for calib in (False, True)]
        made += [bgr_convert_case(A), depth_to_u16_case(A), CropCase(A, 4), CropCase(A, 1), sgm_case(A)]
        made += [complete_case(B, "default"), complete_b_one_off_grid(), complete_u16_case(B), labeled_case(B, "synth")]
        made += [colorize_case(C), bgr_convert_case(C), depth_to_u16_case(C), CloudRefusalCase(C), evaluate_case(C, False)]
        # beyond 2^31 pixels also: the kernels that take the whole batch as ONE flat run (k_norm_write, k_u16_to_f32, k_project_resolve,
        # k_nearest_fixup and the 8.7 GB memset in front of it) and one kernel with the frame in its grid's y
        made += [complete_case(C, "stop_normalize"), complete_u16_case(C, staged=True), ProjectCase(C, False, False), ProjectCase(C, False, True),
                 gaussian_case(C)]
        for c in made:
            assert c.name not in _cases, c.name
            _cases[c.name] = c
    return _cases


def complete_b_one_off_grid():
    """Geometry B with ONE frame off the 1/256 m grid, behind the 2^32-byte boundary: the 16-bit attempt raises its flag and the
    gated f32 rerun recomputes the whole batch."""
    case = complete_case(B, "default", seed=150)
    case.name = "complete_dev one off-grid frame B"
    inner = case.sources

    def sources(lay):
        x = inner(lay)["src"].copy()
        s = lay.source_of(P32 // (4 * B.px) + 1)
        x[s] = np.where(x[s] > 0, x[s] + f32(0.001), f32(0))
        return {"src": x}

    case.sources = sources
    case.scratch = 2 * B.total_px
    return case
