"""The *_dev entry points the way they are measured and documented: queued on a torch.cuda.Stream() behind work that is still
running, with no host synchronisation between the calls (include/dcmt.h: "DEVICE pointers, stream-ordered, asynchronous ... Never
synchronises; never allocates"; INTEGRATION.md section 3: one thread, one context, one stream per GPU).

The scheme, one helper (run_ordered) for every case.  Each input buffer has a REAL and a DECOY content, both valid inputs of the
call; outputs start with a recognisable finite fill.  After a warm-up on the decoys (code objects, documented first-use
allocations) everything below is enqueued on a stream `s` without the host ever waiting:
    delay kernel, marker event, copy real -> inputs, the call(s) under test (stream=s), clone of every output,
    copy decoy -> inputs, fill -> outputs;            then one s.synchronize().
The clones must be, bit for bit, the expectation for the REAL inputs.  A kernel, memset or copy that left the stream ran either
too early (it saw the decoys or the fill) or too late (it saw the restored decoys, or wrote over the restored fill) and gives
a wrong clone; a call that blocked the host on the stream finds the marker complete when it returns.  Every case asserts that the
marker is still pending right behind the last call under test: a delay that was too short fails the test, it is no pass.
`s` is not any stream: streams that share a hardware queue run one after the other, and an escape to such a stream would be
serialised behind the delay and look right.  scheme_streams() picks `s` so that it runs beside the null stream -- where a launch
that lost its stream argument lands -- and the two controls at the end show that an escaped call is seen on that very stream.

Expectations: the oracle where it has the operation; for evaluate, colorize, depth_to_cloud, reproject_depth and bgr_convert --
whose restatements live in their own test files, which pin these calls -- the bits of the same call made alone, synchronised, on
the default stream and on a fresh context.  expectation(real) != expectation(decoy) != fill is asserted for every compared frame
(for the oracle-backed cases also in a test that needs no GPU), so a stale read cannot look right."""
import time

import numpy as np
import pytest

from depth_completion_mt_amd import _lib as L
from depth_completion_mt_amd import api, synth

gpu = pytest.mark.gpu
f32 = np.float32

SPEC = 16                   # spec_fill_iters of every completion call here: enough for a frame with a 40-row gap (asserted)
D_START_MS, D_CAP_MS = 100.0, 1000.0
FILLS = {"f": -7.0, "i": -7, "u": 0xA5}


def fill_of(dtype):
    return FILLS[np.dtype(dtype).kind]


class Out:
    """One output buffer of a case.  per_frame: its first axis is the batch (real / decoy / fill are told apart frame by frame);
    returned: the wrapper creates it (no buffer of ours: it is cloned, never refilled)."""

    def __init__(self, shape, dtype, per_frame=True, returned=False):
        self.shape, self.dtype, self.per_frame, self.returned = tuple(shape), np.dtype(dtype), per_frame, returned


class Case:
    """name; dims: (max_rows, max_cols, max_batch) of the context; inputs(which) -> {name: array} (0 the real set, 1 the decoys,
    2.. further real sets); outputs {name: Out} (a name that is also an input: in place, no fill); call(ctx, t, stream) with t
    {name: tensor} makes the call(s) on `stream` (None: torch's current stream) and returns {name: tensor} of returned outputs or
    None; expect(inputs) -> {name: array} from the oracle (keys with a leading underscore: host values), None = the call made alone;
    after(ctx, expectation): host-side checks right behind the enqueue; wrap(ctx, t, stream) -> {name: tensor}: the same call with
    every output left to the wrapper."""

    def __init__(self, name, dims, inputs, outputs, call, expect=None, after=None, wrap=None):
        self.name, self.dims, self._inputs, self.outputs = name, dims, inputs, outputs
        self.call, self.expect, self.after, self.wrap = call, expect, after, wrap
        self._in, self._exp, self.rows = {}, {}, {}

    def inputs(self, which):
        if which not in self._in:
            self._in[which] = {k: np.ascontiguousarray(v) for k, v in self._inputs(which).items()}
        return self._in[which]

    def expectation(self, which):
        """Computed once per input set and shared (never modified)."""
        if which not in self._exp:
            self._exp[which] = self.expect(self.inputs(which)) if self.expect else alone(self, self.inputs(which))
        return self._exp[which]


# ---------------------------------------------------------------------------------------------------------------- comparing
def _words(a):
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(_words(a), _words(b))


def assert_same(got, want, what, name=None):
    """Bit for bit.  name "centers" (the SLIC centres only): where the oracle's value is NaN -- a centre that owns no pixel --
    nothing is compared; name "points": cloud records, whose fourth word holds colour bytes (read as a float: NaN, alpha being 255);
    every other expectation must be free of NaN."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, f"{what}: {got.dtype}{got.shape} vs {want.dtype}{want.shape}"
    neq = _words(got) != _words(want)
    if want.dtype.kind == "f":
        if name == "centers":
            neq &= ~np.isnan(want)
        elif name != "points":
            assert not np.isnan(want).any(), f"{what}: the expectation holds NaN"
    if neq.any():
        first = tuple(np.argwhere(neq)[0])
        raise AssertionError(f"{what}: {int(neq.sum())} of {want.size} elements differ bitwise; first at {first}: {got[first]!r} vs {want[first]!r}")


def check_distinct(case, e_real, e_decoy):
    """The condition on the inputs: per compared frame expectation(real) differs bitwise from expectation(decoy) and from the fill."""
    for name, o in case.outputs.items():
        a, b = e_real[name], e_decoy[name]
        assert a.shape == o.shape and a.dtype == o.dtype, (case.name, name, a.shape, a.dtype)
        n = o.shape[0] if o.per_frame else 1
        for f in range(n):
            fa, fb = (a[f], b[f]) if o.per_frame else (a, b)
            assert not same_bits(fa, fb), f"{case.name}: {name} frame {f}: real and decoy expectations are the same bits"
            if not o.returned and name not in case.inputs(0):
                assert not (fa == fill_of(o.dtype)).all(), f"{case.name}: {name} frame {f}: the expectation is the fill"


# ---------------------------------------------------------------------------------------------------------------- device side
def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.cpu().numpy()


def buffers(case, inp):
    """The case's device buffers: inputs holding `inp`, outputs holding their fill."""
    t = {k: dev(v) for k, v in inp.items()}
    for name, o in case.outputs.items():
        if not o.returned and name not in t:
            t[name] = dev(np.full(o.shape, fill_of(o.dtype), o.dtype))
    return t


def refill(case, t):
    for name, o in case.outputs.items():
        if not o.returned and name not in case.inputs(0):
            t[name].fill_(fill_of(o.dtype))


def alone(case, inp):
    """The bits of the call made alone: a fresh context, torch's default stream, synchronised."""
    import torch
    with api.Context(0, *case.dims) as ctx:
        t = buffers(case, inp)
        torch.cuda.synchronize()
        ret = case.call(ctx, t, None) or {}
        torch.cuda.synchronize()
        return {name: host(ret[name] if o.returned else t[name]) for name, o in case.outputs.items()}


_cycles_per_ms = []


def cycles_per_ms():
    """torch.cuda._sleep spins for a number of clock ticks: how many make a millisecond, measured once with events."""
    import torch
    if not _cycles_per_ms:
        n, ms = 1_000_000, 0.0
        for _ in range(6):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            torch.cuda._sleep(n)
            e1.record()
            torch.cuda.synchronize()
            ms = e0.elapsed_time(e1)
            if ms >= 5.0:
                break
            n *= 8
        assert ms >= 5.0, f"torch.cuda._sleep({n}) took {ms} ms: unusable as a delay"
        _cycles_per_ms.append(n / ms)
    return _cycles_per_ms[0]


def delay_for(t_call):
    """D: 100 ms, raised up to the 1 s cap until D >= 20 * t_call."""
    return min(D_CAP_MS, max(D_START_MS, 20.0 * t_call * 1e3))


def delayed(stream, d_ms):
    """Enqueues the delay kernel and records the marker behind it; returns the marker."""
    import torch
    with torch.cuda.stream(stream):
        torch.cuda._sleep(int(d_ms * cycles_per_ms()))
        marker = torch.cuda.Event()
        marker.record(stream)
    return marker


def overlaps(busy, c):
    """One probe: does a small piece of work on stream `c` finish while `busy` is held up by a 20 ms delay?"""
    import torch
    marker = delayed(busy, 20.0)
    with torch.cuda.stream(c):
        torch.zeros(16, device="cuda")
    c.synchronize()
    ran = not marker.query()
    busy.synchronize()
    return ran


_streams = []


def scheme_streams():
    """(s, s2): the stream every scheme of this module runs on, and the second stream of the tests that are about two.  HIP spreads a
    process's streams over a few hardware queues (four by default) and streams on one queue run one after the other; a launch that
    escaped from `s` to the null stream (or to s2) would then be serialised behind the delay and the producer copy, and its clone
    would come out right: the scheme would be blind.  So, once per module, eight streams of torch's pool are surveyed -- each probed
    once -- and `s` is one that runs while the null stream is busy, s2 one that runs while the null stream and while `s` is busy.
    The two controls at the end of the module show that an escape to either is seen on exactly these streams."""
    import torch
    if not _streams:
        null = torch.cuda.default_stream()
        cand = {c.cuda_stream: c for c in (torch.cuda.Stream() for _ in range(8))}
        free = [c for c in cand.values() if c.cuda_stream != null.cuda_stream and overlaps(null, c)]
        assert free, "none of eight streams ran while the null stream was busy: an escaped launch could not be seen here"
        others = [c for c in free[1:] if overlaps(free[0], c)]
        assert others, "no second stream ran while the scheme's stream was busy: nothing about two streams can be tested here"
        print(f"[stream-order] streams: {len(free)} of {len(cand)} surveyed ran beside the null stream, {len(others)} of the other {len(free) - 1} beside the chosen one")
        _streams.extend([free[0], others[0]])
    return _streams


def report(name, t_call, d_ms, **kw):
    print(f"[stream-order] {name}: t_call {t_call * 1e3:.3f} ms, D {d_ms:.0f} ms" + "".join(f", {k} {v}" for k, v in kw.items()))


def warm_up(case, ctx, t, s):
    """Once on `s` with the decoys in place (code objects, first-use allocations), then a second, timed call: t_call."""
    import torch
    decoy = {k: dev(v) for k, v in case.inputs(1).items()}
    torch.cuda.synchronize()
    t_call = 0.0
    for _ in range(2):
        t0 = time.perf_counter()
        case.call(ctx, t, s.cuda_stream)
        t_call = time.perf_counter() - t0
        s.synchronize()
        with torch.cuda.stream(s):
            for k in decoy:
                t[k].copy_(decoy[k])
            refill(case, t)
        s.synchronize()
    return decoy, t_call


def run_ordered(case, check_marker=True):
    """The scheme of the module docstring on one case; returns the clones as host arrays."""
    import torch
    e_real, e_decoy = case.expectation(0), case.expectation(1)
    check_distinct(case, e_real, e_decoy)
    real = {k: dev(v) for k, v in case.inputs(0).items()}
    s = scheme_streams()[0]
    t0 = time.perf_counter()
    with api.Context(0, *case.dims) as ctx:
        t = buffers(case, case.inputs(1))
        decoy, t_call = warm_up(case, ctx, t, s)
        d_ms = delay_for(t_call)
        marker = delayed(s, d_ms)
        with torch.cuda.stream(s):
            for k in real:
                t[k].copy_(real[k])
            ret = case.call(ctx, t, s.cuda_stream) or {}
            pending = not marker.query()
            if case.after:
                case.after(ctx, e_real)
            clones = {name: (ret[name] if o.returned else t[name]).clone() for name, o in case.outputs.items()}
            for k in decoy:
                t[k].copy_(decoy[k])
            refill(case, t)
        s.synchronize()
        got = {k: host(v) for k, v in clones.items()}
    report(case.name, t_call, d_ms, test_s=f"{time.perf_counter() - t0:.2f}")
    if check_marker:
        assert pending, f"{case.name}: the marker behind a {d_ms:.0f} ms delay was complete when the call returned (t_call {t_call * 1e3:.3f} ms): the call blocked on its stream, or the delay was too short"
    for name in case.outputs:
        assert_same(got[name], e_real[name], f"{case.name}: {name} behind the delay", name)
    return got


# ---------------------------------------------------------------------------------------------------------------- the cases
def O():
    from oracle import oracle
    return oracle


def sparse_frames(b, rows, cols, seed, gap=False):
    x = synth.synth_batch(b, rows, cols, seed)
    if gap:                                      # a 40-row gap under a valid band: the hole-closure loop has to run
        x[b - 1, 0:2] = f32(40.0) + f32(seed % 64) / f32(4.0)
        x[b - 1, 4:44] = 0
    return x


def salt_and_pepper(g, shape):
    """tests/test_gpu_fuzz.py's generator: every pixel its own neighbourhood of labels 0..8, some unlabeled."""
    lab = g.integers(0, 9, shape).astype(np.int32)
    lab[g.random(shape) < 0.03] = -1
    return lab


def complete_case(name, rows, cols, b, gap=True, norm=None, labeled=False, u16=False, iters=False, **pkw):
    def inputs(which):
        x = sparse_frames(b, rows, cols, 100 + 50 * which, gap)
        d = {"src": np.round(x * 256.0).astype(np.uint16).view(np.int16) if u16 else x}
        if labeled:
            d["labels"] = salt_and_pepper(np.random.Generator(np.random.PCG64(9 + which)), (b, rows, cols))
        return d

    def params():
        return api.make_params(spec_fill_iters=SPEC, normalize=norm, **pkw)

    def call(ctx, t, st):
        if u16:
            ctx.complete_u16_dev(t["src"], 1.0 / 256.0, t["dst"], params(), stream=st)
        else:
            ctx.complete_dev(t["src"], t["dst"], params(), d_labels=t.get("labels"), n_labels=9 if labeled else 0, stream=st)

    def wrap(ctx, t, st):
        if u16:
            return {"dst": ctx.complete_u16_dev(t["src"], 1.0 / 256.0, None, params(), stream=st)}
        return {"dst": ctx.complete_dev(t["src"], None, params(), d_labels=t.get("labels"), n_labels=9 if labeled else 0, stream=st)}

    def expect(inp):
        out, its = [], []
        for f in range(b):
            x = inp["src"][f]
            if u16:
                x = (x.view(np.uint16).astype(f32) * f32(1.0 / 256.0)).astype(f32)
            if norm is not None:
                x = O().normalize_minmax(x, *norm)
            if labeled:
                y, info = O().interpolate_with_superpixels(x, inp["labels"][f], 9, return_info=True)
            else:
                y, info = O().img_completion(x, return_info=True)
            assert info["rc"] == 0 and info["fill_iters"] < SPEC, (name, f, info)
            out.append(y)
            its.append(info["fill_iters"])
        if gap:
            assert max(its) > 1, (name, its)      # the gap frame does need the loop
        return {"dst": np.stack(out), "_iters": its}

    def after(ctx, e):
        # dcmt_last_fill_iters "synchronises with the last call's stream": right behind the enqueue, with no torch synchronisation
        got, st = ctx.last_fill_iters(b)
        assert st == L.OK and got == e["_iters"], (name, got, e["_iters"])

    return Case(name, (rows, cols, b), inputs, {"dst": Out((b, rows, cols), f32)}, call, expect, after if iters else None, wrap)


def project_case(name="project_points 40x133 ragged", rows=40, cols=133, n=6000):
    T = synth.KITTI_T_VELO_TO_CAM
    P = np.array([[60.0, 0, cols / 2, 3.0], [0, 60.0, rows / 2, 0.01], [0, 0, 1, 0.002]], f32)
    parts = {0: [0, 2500, 2500, n], 1: [0, 1000, n, n], 2: [0, 0, 3000, n], 3: [0, 4000, 5000, n]}     # each with an empty sweep but [3]

    def inputs(which):
        return {"pts": synth.synth_points(n, 300 + which), "off": np.array(parts[which], np.int32)}

    def call(ctx, t, st):
        ctx.project_points_dev(t["pts"], t["off"], T, P, rows, cols, t["sparse"], stream=st)

    def wrap(ctx, t, st):
        return {"sparse": ctx.project_points_dev(t["pts"], t["off"], T, P, rows, cols, None, stream=st)}

    def expect(inp):
        o = inp["off"]
        return {"sparse": np.stack([O().project_points(inp["pts"][o[f]:o[f + 1]], T, P, rows, cols) for f in range(3)])}

    return Case(name, (rows, cols, 3), inputs, {"sparse": Out((3, rows, cols), f32)}, call, expect, None, wrap)


def slic_case(rows, cols, step, b=2, nc=40):
    def inputs(which):
        return {"lab": np.stack([synth.synth_lab(rows, cols, 40 + 10 * which + f) for f in range(b)])}

    def call(ctx, t, st):
        _, _, cent = ctx.slic_labels_dev(t["lab"], step, nc, t["labels"], return_centers=True, stream=st)
        return {"centers": cent}

    def wrap(ctx, t, st):
        lab, _, cent = ctx.slic_labels_dev(t["lab"], step, nc, None, return_centers=True, stream=st)
        return {"labels": lab, "centers": cent}

    def expect(inp):
        res = [O().slic(inp["lab"][f], step, nc, return_centers=True) for f in range(b)]
        assert all(r[1] == res[0][1] for r in res)
        return {"labels": np.stack([r[0] for r in res]), "centers": np.stack([r[2] for r in res])}

    case = Case(f"slic_labels {rows}x{cols} step {step}", (rows, cols, b), inputs, {"labels": Out((b, rows, cols), np.int32)}, call, expect, None, wrap)
    n = O().slic(case.inputs(0)["lab"][0], step, nc)[1]
    case.outputs["centers"] = Out((b, n, 5), np.float64, returned=True)
    return case


def stereo_case(iterations, rows=48, cols=64, b=2):
    kw = dict(focal=80.0)

    def inputs(which):
        l, r, d = zip(*[synth.synth_stereo(rows, cols, 70 + 7 * which + f, focal=80.0) for f in range(b)])
        return {"depth": np.stack(d), "left": np.stack(l), "right": np.stack(r)}

    def call(ctx, t, st):
        ctx.stereo_refine_dev(t["depth"], t["left"], t["right"], t["out"], iterations=iterations, stream=st, **kw)

    def wrap(ctx, t, st):
        return {"out": ctx.stereo_refine_dev(t["depth"], t["left"], t["right"], None, iterations=iterations, stream=st, **kw)}

    def expect(inp):
        it = 4 if iterations is None else iterations
        return {"out": np.stack([O().stereo_refine(inp["depth"][f], inp["left"][f], inp["right"][f], iterations=it, **kw) for f in range(b)])}

    return Case(f"stereo_refine 48x64 iterations={iterations}", (rows, cols, b), inputs, {"out": Out((b, rows, cols), f32)}, call, expect, None, wrap)


def gaussian_case(in_place, rows=48, cols=64, b=3):
    def inputs(which):
        return {"src": (np.random.default_rng(40 + which).standard_normal((b, rows, cols)) * 20.0).astype(f32)}

    def call(ctx, t, st):
        ctx.gaussian5_dev(t["src"], t["src"] if in_place else t["dst"], stream=st)

    def wrap(ctx, t, st):
        return {"dst": ctx.gaussian5_dev(t["src"], None, stream=st)}

    def expect(inp):
        return {"src" if in_place else "dst": np.stack([O().gaussian5(inp["src"][f]) for f in range(b)])}

    return Case(f"gaussian5 {'in place' if in_place else 'out of place'}", (rows, cols, b), inputs,
                {"src" if in_place else "dst": Out((b, rows, cols), f32)}, call, expect, None, None if in_place else wrap)


def dense_frames(b, rows, cols, seed):
    g = np.random.default_rng(seed)
    return g.uniform(0.5, 80.0, (b, rows, cols)).astype(f32)


def evaluate_case(u16, rows=48, cols=64, b=3):
    def inputs(which):
        g = np.random.default_rng(500 + which)
        pred = dense_frames(b, rows, cols, 510 + which)
        gt = np.where(g.random(pred.shape) < 0.3, pred + g.normal(0, 1.5, pred.shape), 0.0).clip(0, 200)
        gt = np.round(gt * 256.0).astype(np.uint16)
        return {"gt": gt.view(np.int16) if u16 else (gt.astype(f32) / f32(256.0)).astype(f32), "pred": pred}

    def call(ctx, t, st):
        ctx.evaluate_dev(t["gt"], t["pred"], 0.0, "both", d_out=t["sums"], stream=st)

    def wrap(ctx, t, st):
        return {"sums": ctx.evaluate_dev(t["gt"], t["pred"], 0.0, "both", stream=st)}

    return Case(f"evaluate {'uint16' if u16 else 'f32'} ground truth", (rows, cols, b), inputs, {"sums": Out((b, 7), np.float64)}, call, None, None, wrap)


def colorize_case(rows=48, cols=64, b=3):
    def call(ctx, t, st):
        ctx.colorize_dev(t["src"], t["bgr"], stream=st)

    def wrap(ctx, t, st):
        return {"bgr": ctx.colorize_dev(t["src"], None, stream=st)}

    return Case("colorize", (rows, cols, b), lambda which: {"src": dense_frames(b, rows, cols, 600 + which)},
                {"bgr": Out((b, rows, cols, 3), np.uint8)}, call, None, None, wrap)


def bgr_case(mode, rows=40, cols=56, b=3):
    outs = {"lab": {"lab": Out((b, rows, cols, 3), np.uint8)}, "gray": {"gray": Out((b, rows, cols), np.uint8)},
            "both": {"lab": Out((b, rows, cols, 3), np.uint8), "gray": Out((b, rows, cols), np.uint8)},
            "in place": {"bgr": Out((b, rows, cols, 3), np.uint8)}}[mode]

    def call(ctx, t, st):
        if mode == "in place":
            ctx.bgr_convert_dev(t["bgr"], d_lab=t["bgr"], stream=st)
        else:
            ctx.bgr_convert_dev(t["bgr"], lab=False, d_lab=t.get("lab"), d_gray=t.get("gray"), stream=st)

    def wrap(ctx, t, st):
        lab, gray = ctx.bgr_convert_dev(t["bgr"], lab=True, gray=True, stream=st)
        return {"lab": lab, "gray": gray}

    return Case(f"bgr_convert {mode}", (rows, cols, b), lambda which: {"bgr": np.random.default_rng(700 + which).integers(0, 256, (b, rows, cols, 3), dtype=np.uint8)},
                outs, call, None, None, wrap if mode == "both" else None)


def cloud_case(colour, rows=48, cols=64, b=3):
    def inputs(which):
        d = {"depth": sparse_frames(b, rows, cols, 800 + 20 * which)}
        if colour:
            d["bgr"] = np.random.default_rng(810 + which).integers(0, 256, (b, rows, cols, 3), dtype=np.uint8)
        return d

    def call(ctx, t, st):
        ctx.depth_to_cloud_dev(t["depth"], t.get("bgr"), d_points=t["points"], d_offsets=t["offsets"], stream=st)

    def wrap(ctx, t, st):
        pts, off = ctx.depth_to_cloud_dev(t["depth"], t.get("bgr"), stream=st)
        return {"points": pts, "offsets": off}

    # records from offsets[batch] on are not written: they keep the fill, in the call made alone as behind the delay; in points
    # that the wrapper creates (torch.empty) they are anything, and only the rows in front of them are compared
    case = Case(f"depth_to_cloud {'with' if colour else 'without'} colour", (rows, cols, b), inputs,
                {"points": Out((b * rows * cols, 4), f32, per_frame=False), "offsets": Out((b + 1,), np.int32, per_frame=False)}, call, None, None, wrap)
    case.rows["points"] = lambda e: int(e["offsets"][-1])
    return case


def reproject_case(rows=48, cols=64, orows=40, ocols=70, b=3):
    M = np.eye(4, dtype=f32)
    M[0, 3] = 0.5                                 # a shift along x: columns move by 0.5 * fx / z, some collide, some leave the image

    def call(ctx, t, st):
        ctx.reproject_depth_dev(t["depth"], orows, ocols, api.make_reproject_params(M=M), t["out"], stream=st)

    def wrap(ctx, t, st):
        return {"out": ctx.reproject_depth_dev(t["depth"], orows, ocols, api.make_reproject_params(M=M), None, stream=st)}

    return Case("reproject_depth 48x64 -> 40x70", (max(rows, orows), max(cols, ocols), b), lambda which: {"depth": dense_frames(b, rows, cols, 900 + which)},
                {"out": Out((b, orows, ocols), f32)}, call, None, None, wrap)


_cases = {}


def cases():
    """Every case of part 1, built once (the oracle-backed ones need no GPU to build)."""
    if not _cases:
        for c in (complete_case("complete staged 48x64 batch 2", 48, 64, 2),
                  complete_case("complete streaming 64x96 batch 8", 64, 96, 8, force_fused=True),
                  complete_case("complete normalize=(0, 80) staged", 48, 64, 2, norm=(0, 80)),
                  complete_case("complete normalize=(0, 80) streaming", 64, 96, 8, norm=(0, 80), force_fused=True),
                  complete_case("complete labeled 40x56 batch 2", 40, 56, 2, gap=False, labeled=True),
                  complete_case("complete labeled 40x56 batch 8", 40, 56, 8, gap=False, labeled=True),
                  complete_case("complete_u16 64x96 batch 8", 64, 96, 8, u16=True),
                  complete_case("last_fill_iters behind complete 64x96 batch 8", 64, 96, 8, iters=True, force_fused=True),
                  project_case(), slic_case(75, 131, 7), slic_case(70, 130, 16), stereo_case(0), stereo_case(None),
                  gaussian_case(False), gaussian_case(True),
                  evaluate_case(False), evaluate_case(True), colorize_case(), bgr_case("lab"), bgr_case("gray"), bgr_case("both"),
                  bgr_case("in place"), cloud_case(True), cloud_case(False), reproject_case()):
            _cases[c.name] = c
    return _cases


ORACLE_BACKED = ["complete staged 48x64 batch 2", "complete streaming 64x96 batch 8", "complete normalize=(0, 80) staged",
                 "complete normalize=(0, 80) streaming", "complete labeled 40x56 batch 2", "complete labeled 40x56 batch 8",
                 "complete_u16 64x96 batch 8", "last_fill_iters behind complete 64x96 batch 8", "project_points 40x133 ragged",
                 "slic_labels 75x131 step 7", "slic_labels 70x130 step 16", "stereo_refine 48x64 iterations=0",
                 "stereo_refine 48x64 iterations=None", "gaussian5 out of place", "gaussian5 in place"]
ALONE_BACKED = ["evaluate f32 ground truth", "evaluate uint16 ground truth", "colorize", "bgr_convert lab", "bgr_convert gray",
                "bgr_convert both", "bgr_convert in place", "depth_to_cloud with colour", "depth_to_cloud without colour",
                "reproject_depth 48x64 -> 40x70"]
WRAPPED = ["complete staged 48x64 batch 2", "complete streaming 64x96 batch 8", "complete labeled 40x56 batch 8", "complete_u16 64x96 batch 8",
           "project_points 40x133 ragged", "slic_labels 70x130 step 16", "stereo_refine 48x64 iterations=None", "gaussian5 out of place",
           "reproject_depth 48x64 -> 40x70", "evaluate f32 ground truth", "colorize", "bgr_convert both", "depth_to_cloud with colour",
           "depth_to_cloud without colour"]


def test_case_lists_name_every_case():
    assert sorted(ORACLE_BACKED + ALONE_BACKED) == sorted(cases())
    assert all(cases()[n].expect is not None for n in ORACLE_BACKED) and all(cases()[n].expect is None for n in ALONE_BACKED)
    assert all(cases()[n].wrap is not None for n in WRAPPED)


@pytest.mark.parametrize("name", ORACLE_BACKED)
def test_real_and_decoy_expectations_differ(name):
    """No GPU: for the oracle-backed cases expectation(real), expectation(decoy) and the fill differ in every compared frame."""
    case = cases()[name]
    check_distinct(case, case.expectation(0), case.expectation(1))


def test_deep_queue_inputs_have_distinct_expectations():
    """No GPU: the two distinct inputs of the deep-queue test (and their decoys) give four different results."""
    exp = [ring_expectation(x) for x in ring_inputs()]
    for i in range(4):
        for j in range(i):
            for f in range(8):
                if not (f != 5 and {i, j} in ({0, 1}, {2, 3})):      # grid and off-grid differ in frame 5 only
                    assert not same_bits(exp[i][f], exp[j][f]), (i, j, f)
    assert not same_bits(exp[0][5], exp[1][5]) and not same_bits(exp[2][5], exp[3][5])


# ---------------------------------------------------------------------------------------------------------------- 1. alone
@gpu
@pytest.mark.parametrize("name", ORACLE_BACKED + ALONE_BACKED)
def test_entry_point_alone_behind_the_delay(name):
    run_ordered(cases()[name])


# ---------------------------------------------------------------------------------------------------------------- 2. deep queue
def ring_inputs():
    """(grid, off-grid, decoy of grid, decoy of off-grid): the batches of test_16_bit_flag_ring_over_many_calls, and another seed."""
    res = []
    for seed in (21, 61):
        grid = synth.synth_batch(8, 64, 96, seed)
        grid[2, 20:60, 10:80] = 0                 # one frame that needs the hole-closure loop
        off = grid.copy()
        off[5][off[5] > 0] += f32(0.003)
        res += [grid, off]
    return res


_ring_exp = {}


def ring_expectation(x):
    key = x.tobytes()
    if key not in _ring_exp:
        _ring_exp[key] = np.stack([O().img_completion(f) for f in x])
    return _ring_exp[key]


@gpu
def test_16_bit_form_under_a_deep_queue(monkeypatch):
    """141 calls queued behind one delay on one context: 70 on the 1/256 m grid, one off it, 70 more of which every fifth is off it.
    The host never sees a raised flag in time (q16_seen is read at the start of a later call, the device is a whole queue behind),
    so it keeps attempting the 16-bit form and every off-grid call is rescued by the device-side gate alone.  Then the same
    sequence on the same context with a synchronise after every call: the regime the ring was tested in so far."""
    import torch
    monkeypatch.setenv("DCMT_Q16_MIN_WAVES", "0")            # read by dcmt_create
    grid, off, grid_decoy, off_decoy = ring_inputs()
    want = {False: ring_expectation(grid), True: ring_expectation(off)}
    seq = [False] * 70 + [True] + [k % 5 == 0 for k in range(70)]
    real = {False: dev(grid), True: dev(off)}
    decoy = {False: dev(grid_decoy), True: dev(off_decoy)}
    buf = {False: decoy[False].clone(), True: decoy[True].clone()}
    out = dev(np.full((len(seq), 8, 64, 96), -7.0, f32))      # every call its own slice: 27 MB
    s = scheme_streams()[0]
    with api.Context(0, 64, 96, 8) as other:                 # the f32 rerun's code objects, loaded through another context ...
        other.complete_dev(buf[True], out[0], stream=s.cuda_stream)
        s.synchronize()
    with api.Context(0, 64, 96, 8) as ctx:
        t_call = 0.0
        for _ in range(2):                                   # ... so that this context's warm-up (the 16-bit plane) raises no flag
            t0 = time.perf_counter()
            ctx.complete_dev(buf[False], out[0], stream=s.cuda_stream)
            t_call = time.perf_counter() - t0
            s.synchronize()
        assert "k_fp_q" in ctx.last_path(), ctx.last_path()
        out[0].fill_(-7.0)
        torch.cuda.synchronize()
        d_ms = delay_for(t_call * len(seq))
        marker = delayed(s, d_ms)
        paths = []
        with torch.cuda.stream(s):
            for k in buf:
                buf[k].copy_(real[k])
            t0 = time.perf_counter()
            for i, is_off in enumerate(seq):
                ctx.complete_dev(buf[is_off], out[i], stream=s.cuda_stream)
                paths.append(ctx.last_path())
            t_all = time.perf_counter() - t0
            pending = not marker.query()
            for k in buf:
                buf[k].copy_(decoy[k])
        s.synchronize()
        report("16-bit form, deep queue (141 calls)", t_call, d_ms, t_141_calls_ms=f"{t_all * 1e3:.2f}")
        assert pending, f"the marker behind a {d_ms:.0f} ms delay was complete after 141 enqueues ({t_all * 1e3:.1f} ms on the host)"
        assert any("k_fp_q" in p for p in paths), set(paths)
        got = host(out)
        for i, is_off in enumerate(seq):
            assert_same(got[i], want[is_off], f"deep queue, call {i} ({'off-grid' if is_off else 'grid'}, {paths[i]})")
        # the same sequence, synchronised after every call: the host sees each raised flag at once and skips the next 63 attempts
        with torch.cuda.stream(s):
            for k in buf:
                buf[k].copy_(real[k])
            out.fill_(-7.0)
        s.synchronize()
        paths2 = []
        for i, is_off in enumerate(seq):
            ctx.complete_dev(buf[is_off], out[i], stream=s.cuda_stream)
            s.synchronize()
            paths2.append(ctx.last_path())
        got2 = host(out)
        for i, is_off in enumerate(seq):
            assert_same(got2[i], want[is_off], f"synchronised, call {i} ({'off-grid' if is_off else 'grid'}, {paths2[i]})")
        assert any("k_fp_s" in p for p in paths2), set(paths2)     # the skipped attempts
        queued, synced = sum("k_fp_q" in p for p in paths), sum("k_fp_q" in p for p in paths2)
        print(f"[stream-order] deep queue: {queued} attempts queued, {synced} synchronised")
        # the two regimes: queued, the host saw no flag in time and attempted every call (the 15 off-grid ones included: rescued on
        # the device alone); synchronised, every raised flag stops the next 63 attempts
        assert queued == len(seq) and synced < queued - 63, (queued, synced)


# ---------------------------------------------------------------------------------------------------------------- 3. pipelines
def alone_on(dims, fn):
    """fn(ctx) made alone: fresh context, default stream, synchronised; returns its tensors as host arrays."""
    import torch
    with api.Context(0, *dims) as ctx:
        torch.cuda.synchronize()
        res = fn(ctx)
        torch.cuda.synchronize()
        return [host(r) for r in res]


def run_pipeline(name, dims, input_sets, decoy, outputs, calls, expectations, decoy_expectation):
    """Three input sets through the SAME device buffers, all iterations queued behind one delay, clones taken per iteration.
    outputs: {name: (shape, dtype, per_frame)}.  The condition on the inputs, per compared frame as in check_distinct: an iteration's
    expectation differs from the decoys', from the iteration before's (what a stale read would show) and from the fill."""
    import torch
    frames = lambda a, per_frame: list(a) if per_frame else [a]
    for i, e in enumerate(expectations):
        stale = [("the decoys", decoy_expectation)] + ([("the iteration before", expectations[i - 1])] if i else [])
        for k, (shape, dtype, per_frame) in outputs.items():
            assert e[k].shape == tuple(shape) and e[k].dtype == np.dtype(dtype), (name, i, k, e[k].shape, e[k].dtype)
            for f, fa in enumerate(frames(e[k], per_frame)):
                assert not (fa == fill_of(dtype)).all(), f"{name}: iteration {i}: {k} frame {f}: the expectation is the fill"
                for what, o in stale:
                    assert not same_bits(fa, frames(o[k], per_frame)[f]), f"{name}: iteration {i}: {k} frame {f}: the same bits as {what}"
    real = [{k: dev(v) for k, v in inp.items()} for inp in input_sets]
    d_decoy = {k: dev(v) for k, v in decoy.items()}
    s = scheme_streams()[0]
    t0 = time.perf_counter()
    with api.Context(0, *dims) as ctx:
        t = {k: v.clone() for k, v in d_decoy.items()}
        for k, (shape, dtype, _) in outputs.items():
            t[k] = dev(np.full(shape, fill_of(dtype), dtype))
        fills = {k: t[k].clone() for k in outputs}
        t_call = 0.0
        for _ in range(2):
            tc = time.perf_counter()
            calls(ctx, t, s.cuda_stream)
            t_call = time.perf_counter() - tc
            s.synchronize()
            with torch.cuda.stream(s):
                for k in fills:
                    t[k].copy_(fills[k])
            s.synchronize()
        d_ms = delay_for(t_call * len(input_sets))
        marker = delayed(s, d_ms)
        clones = []
        with torch.cuda.stream(s):
            for inp in real:
                for k in inp:
                    t[k].copy_(inp[k])
                calls(ctx, t, s.cuda_stream)
                clones.append({k: t[k].clone() for k in outputs})
            pending = not marker.query()
            for k in d_decoy:
                t[k].copy_(d_decoy[k])
            for k in fills:
                t[k].copy_(fills[k])
        s.synchronize()
        got = [{k: host(v) for k, v in c.items()} for c in clones]
    report(name, t_call, d_ms, test_s=f"{time.perf_counter() - t0:.2f}")
    assert pending, f"{name}: the marker behind a {d_ms:.0f} ms delay was complete after the last call returned"
    for i, e in enumerate(expectations):
        for k in e:
            assert_same(got[i][k], e[k], f"{name}: iteration {i}: {k}", k)


class Pipeline:
    """A chain of calls through one set of buffers: what run_pipeline takes (tests/test_gpu_graph_replay.py replays the same
    chains from a captured graph).  inputs(k) -> {name: array}; outputs {name: (shape, dtype, per_frame)}; calls(ctx, t, stream);
    expect(inputs) -> {name: array}."""

    def __init__(self, name, dims, inputs, outputs, calls, expect):
        self.name, self.dims, self.inputs, self.outputs, self.calls, self.expect = name, dims, inputs, outputs, calls, expect


def lidar_camera_pipeline():
    """bgr_convert -> slic_labels -> complete(d_labels) -> evaluate."""
    rows, cols, b, step, nc = 70, 130, 2, 16, 40
    dims = (rows, cols, b)
    nl = L.lib().dcmt_slic_num_centers(rows, cols, step)
    p = lambda: api.make_params(spec_fill_iters=SPEC)

    def inputs(k):
        g = np.random.default_rng(1000 + k)
        lab = np.stack([synth.synth_lab(rows, cols, 200 + 10 * k + f) for f in range(b)])      # smooth regions: as camera bytes
        sparse = sparse_frames(b, rows, cols, 1100 + 10 * k)
        gt = np.where(g.random(sparse.shape) < 0.3, g.uniform(1.0, 80.0, sparse.shape), 0.0).astype(f32)
        return {"bgr": lab, "sparse": sparse, "gt": gt}

    def calls(ctx, t, st):
        ctx.bgr_convert_dev(t["bgr"], d_lab=t["lab"], stream=st)
        ctx.slic_labels_dev(t["lab"], step, nc, t["labels"], stream=st)
        ctx.complete_dev(t["sparse"], t["dense"], p(), d_labels=t["labels"], n_labels=nl, stream=st)
        ctx.evaluate_dev(t["gt"], t["dense"], 0.0, "both", d_out=t["sums"], stream=st)

    def expect(inp):
        lab, = alone_on(dims, lambda c: [c.bgr_convert_dev(dev(inp["bgr"]))])
        res = [O().slic(lab[f], step, nc) for f in range(b)]
        assert all(r[1] == nl for r in res)
        labels = np.stack([r[0] for r in res])
        dense = []
        for f in range(b):
            y, info = O().interpolate_with_superpixels(inp["sparse"][f], labels[f], nl, return_info=True)
            assert info["rc"] == 0 and info["fill_iters"] < SPEC
            dense.append(y)
        dense = np.stack(dense)
        sums, = alone_on(dims, lambda c: [c.evaluate_dev(dev(inp["gt"]), dev(dense), 0.0, "both")])
        return {"lab": lab, "labels": labels, "dense": dense, "sums": sums}

    outs = {"lab": ((b, rows, cols, 3), np.uint8, True), "labels": ((b, rows, cols), np.int32, True), "dense": ((b, rows, cols), f32, True),
            "sums": ((b, 7), np.float64, True)}
    return Pipeline("pipeline lidar + camera", dims, inputs, outs, calls, expect)


def run_repeated(p):
    """The pipeline three times through the same buffers behind one delay: input sets 0..2, set 3 the decoys."""
    sets = [p.inputs(k) for k in range(3)]
    run_pipeline(p.name, p.dims, sets, p.inputs(3), p.outputs, p.calls, [p.expect(i) for i in sets], p.expect(p.inputs(3)))


@gpu
def test_lidar_camera_pipeline_repeated_in_reused_buffers():
    """bgr_convert -> slic_labels -> complete(d_labels) -> evaluate, three times through the same buffers behind one delay."""
    run_repeated(lidar_camera_pipeline())


def stereo_lidar_pipeline():
    """project_points -> complete(normalize) -> bgr_convert(gray) left, right -> stereo_refine -> reproject_depth -> evaluate ->
    gaussian5 in place -> colorize -> depth_to_cloud.  The cloud is made of the warped plane (zero where nothing landed, so its counts
    differ from set to set) with the colourised refined plane as its colours."""
    rows, cols, b, n = 40, 133, 3, 6000
    dims = (rows, cols, b)
    pc = project_case()
    T = synth.KITTI_T_VELO_TO_CAM
    P = np.array([[60.0, 0, cols / 2, 3.0], [0, 60.0, rows / 2, 0.01], [0, 0, 1, 0.002]], f32)
    M = np.eye(4, dtype=f32)
    M[0, 3] = 0.5
    rp = lambda: api.make_reproject_params(M=M)
    p = lambda: api.make_params(spec_fill_iters=SPEC, normalize=(0, 100))

    def inputs(k):
        g = np.random.default_rng(1200 + k)
        d = dict(pc.inputs((0, 2, 3, 1)[k]))
        d["bgr_l"] = g.integers(0, 256, (b, rows, cols, 3), dtype=np.uint8)
        d["bgr_r"] = np.ascontiguousarray(np.roll(d["bgr_l"], -2 - k, axis=2))
        d["gt"] = np.where(g.random((b, rows, cols)) < 0.3, g.uniform(1.0, 80.0, (b, rows, cols)), 0.0).astype(f32)
        return d

    def calls(ctx, t, st):
        ctx.project_points_dev(t["pts"], t["off"], T, P, rows, cols, t["sparse"], stream=st)
        ctx.complete_dev(t["sparse"], t["dense"], p(), stream=st)
        ctx.bgr_convert_dev(t["bgr_l"], lab=False, d_gray=t["gray_l"], stream=st)
        ctx.bgr_convert_dev(t["bgr_r"], lab=False, d_gray=t["gray_r"], stream=st)
        ctx.stereo_refine_dev(t["dense"], t["gray_l"], t["gray_r"], t["refined"], stream=st, focal=80.0)
        ctx.reproject_depth_dev(t["dense"], rows, cols, rp(), t["warped"], stream=st)
        ctx.evaluate_dev(t["gt"], t["warped"], 2.0, "both", d_out=t["sums"], stream=st)
        ctx.gaussian5_dev(t["refined"], t["refined"], stream=st)
        ctx.colorize_dev(t["refined"], t["colour"], stream=st)
        ctx.depth_to_cloud_dev(t["warped"], t["colour"], d_points=t["points"], d_offsets=t["offsets"], stream=st)

    def expect(inp):
        sparse = pc.expect(inp)["sparse"]
        dense = []
        for f in range(b):
            y, info = O().img_completion(O().normalize_minmax(sparse[f], 0, 100), return_info=True)
            assert info["rc"] == 0 and info["fill_iters"] < SPEC
            dense.append(y)
        dense = np.stack(dense)
        gl, gr = alone_on(dims, lambda c: [c.bgr_convert_dev(dev(inp["bgr_l"]), lab=False, gray=True), c.bgr_convert_dev(dev(inp["bgr_r"]), lab=False, gray=True)])
        refined = np.stack([O().stereo_refine(dense[f], gl[f], gr[f], focal=80.0) for f in range(b)])
        blurred = np.stack([O().gaussian5(refined[f]) for f in range(b)])

        def rest(c):
            warped = c.reproject_depth_dev(dev(dense), rows, cols, rp())
            sums = c.evaluate_dev(dev(inp["gt"]), warped, 2.0, "both")
            colour = c.colorize_dev(dev(blurred))
            pts = dev(np.full((b * rows * cols, 4), -7.0, f32))
            _, offs = c.depth_to_cloud_dev(warped, colour, d_points=pts)
            return [warped, sums, colour, pts, offs]
        warped, sums, colour, pts, offs = alone_on(dims, rest)
        return {"sparse": sparse, "dense": dense, "gray_l": gl, "gray_r": gr, "refined": blurred, "warped": warped, "sums": sums,
                "colour": colour, "points": pts, "offsets": offs}

    img, px = ((b, rows, cols), f32, True), ((b, rows, cols), np.uint8, True)
    outs = {"sparse": img, "dense": img, "gray_l": px, "gray_r": px, "refined": img, "warped": img, "sums": ((b, 7), np.float64, True),
            "colour": ((b, rows, cols, 3), np.uint8, True), "points": ((b * rows * cols, 4), f32, False), "offsets": ((b + 1,), np.int32, False)}
    return Pipeline("pipeline stereo + lidar", dims, inputs, outs, calls, expect)


@gpu
def test_stereo_lidar_pipeline_repeated_in_reused_buffers():
    """project_points -> complete(normalize) -> bgr_convert(gray) left, right -> stereo_refine -> reproject_depth -> evaluate ->
    gaussian5 in place -> colorize -> depth_to_cloud, three times through the same buffers behind one delay."""
    run_repeated(stereo_lidar_pipeline())


# ---------------------------------------------------------------------------------------------------------------- 4. growth
@gpu
def test_growth_behind_a_pending_queue():
    """Calls queued behind the delay, then a call that needs more than any before it: several times the labels (bounding-box tables),
    a smaller SLIC step (cells and centres), a larger projection target (winner plane).  The header documents that these may
    synchronise and allocate: no marker check, only every queued result and the growing call's."""
    import torch
    rows, cols, b = 70, 130, 2
    g = np.random.default_rng(77)
    sparse = sparse_frames(b, rows, cols, 1300)
    lab9 = salt_and_pepper(g, (b, rows, cols))
    lab500 = g.integers(0, 500, (b, rows, cols)).astype(np.int32)
    img = np.stack([synth.synth_lab(rows, cols, 1310 + f) for f in range(b)])
    pc = project_case()
    pin = pc.inputs(0)
    pts, off = pin["pts"], np.array([0, 2500, 6000], np.int32)
    T = synth.KITTI_T_VELO_TO_CAM
    Pm = lambda r, c: np.array([[60.0, 0, c / 2, 3.0], [0, 60.0, r / 2, 0.01], [0, 0, 1, 0.002]], f32)
    p = lambda: api.make_params(spec_fill_iters=SPEC)
    want = {}
    for k, (lab, nl) in {"dense9": (lab9, 9), "dense500": (lab500, 500)}.items():
        res = [O().interpolate_with_superpixels(sparse[f], lab[f], nl, return_info=True) for f in range(b)]
        assert all(info["rc"] == 0 and info["fill_iters"] < SPEC for _, info in res)
        want[k] = np.stack([y for y, _ in res])
    for k, step in {"slic16": 16, "slic7": 7}.items():
        want[k] = np.stack([O().slic(img[f], step, 40)[0] for f in range(b)])
    for k, (r, c) in {"small": (40, 64), "large": (rows, cols)}.items():
        want[k] = np.stack([O().project_points(pts[off[f]:off[f + 1]], T, Pm(r, c), r, c) for f in range(b)])
    d = {k: dev(v) for k, v in dict(sparse=sparse, lab9=lab9, lab500=lab500, img=img, pts=pts, off=off).items()}
    out = {k: dev(np.full(v.shape, fill_of(v.dtype), v.dtype)) for k, v in want.items()}
    s = scheme_streams()[0]
    with api.Context(0, rows, cols, b) as ctx:
        st = s.cuda_stream

        def small_calls():
            ctx.complete_dev(d["sparse"], out["dense9"], p(), d_labels=d["lab9"], n_labels=9, stream=st)
            ctx.slic_labels_dev(d["img"], 16, 40, out["slic16"], stream=st)
            ctx.project_points_dev(d["pts"], d["off"], T, Pm(40, 64), 40, 64, out["small"], stream=st)
        small_calls()                                          # warm-up: code objects and the first, small allocations
        s.synchronize()
        with torch.cuda.stream(s):
            for k in ("dense9", "slic16", "small"):
                out[k].fill_(fill_of(want[k].dtype))
        s.synchronize()
        delayed(s, D_START_MS)
        with torch.cuda.stream(s):
            small_calls()
            clones = {k: out[k].clone() for k in ("dense9", "slic16", "small")}
            ctx.complete_dev(d["sparse"], out["dense500"], p(), d_labels=d["lab500"], n_labels=500, stream=st)     # grows the bbox tables
            small_calls()
            ctx.slic_labels_dev(d["img"], 7, 40, out["slic7"], stream=st)                                           # grows cells and centres
            small_calls()
            ctx.project_points_dev(d["pts"], d["off"], T, Pm(rows, cols), rows, cols, out["large"], stream=st)      # grows the winner plane
            small_calls()
        s.synchronize()
        for k in clones:
            assert_same(host(clones[k]), want[k], f"growth: {k} queued in front of the growing calls")
        for k in want:
            assert_same(host(out[k]), want[k], f"growth: {k}")


# ---------------------------------------------------------------------------------------------------------------- 5. two contexts
@gpu
def test_two_contexts_on_two_streams_interleaved_from_one_thread():
    """ctx A on sA behind the delay, ctx B on sB without one, calls alternating: B finishes (results right) while A's marker is
    still pending -- one context's calls never wait on another context's stream -- and A is right after its synchronise."""
    import torch
    case = cases()["complete streaming 64x96 batch 8"]
    e_real, e_decoy = case.expectation(0), case.expectation(1)
    real = {k: dev(v) for k, v in case.inputs(0).items()}
    sA, sB = scheme_streams()
    with api.Context(0, *case.dims) as A, api.Context(0, *case.dims) as B:
        tA, tB = buffers(case, case.inputs(1)), buffers(case, case.inputs(1))
        decoy, t_call = warm_up(case, A, tA, sA)
        warm_up(case, B, tB, sB)
        outsA = [dev(np.full((8, 64, 96), -7.0, f32)) for _ in range(3)]
        outsB = [dev(np.full((8, 64, 96), -7.0, f32)) for _ in range(3)]
        torch.cuda.synchronize()
        d_ms = delay_for(6 * t_call)
        markerA = delayed(sA, d_ms)
        with torch.cuda.stream(sA):
            tA["src"].copy_(real["src"])
        with torch.cuda.stream(sB):
            tB["src"].copy_(real["src"])
        for i in range(3):
            case.call(A, dict(tA, dst=outsA[i]), sA.cuda_stream)
            case.call(B, dict(tB, dst=outsB[i]), sB.cuda_stream)
        sB.synchronize()
        a_pending = not markerA.query()                     # B has run dry: A's delay must not have been in its way
        gotB = [host(o) for o in outsB]
        with torch.cuda.stream(sA):
            tA["src"].copy_(decoy["src"])
        sA.synchronize()
        gotA = [host(o) for o in outsA]
    report("two contexts, two streams", t_call, d_ms)
    assert a_pending, f"context B's calls were only through when context A's {d_ms:.0f} ms delay had run out"
    for i in range(3):
        assert_same(gotB[i], e_real["dst"], f"context B (no delay), call {i}")
        assert_same(gotA[i], e_real["dst"], f"context A (behind the delay), call {i}")


# ---------------------------------------------------------------------------------------------------------------- 6. the wrappers
@gpu
@pytest.mark.parametrize("name", WRAPPED)
def test_wrapper_creates_its_output_on_the_stream_it_enqueues_on(name):
    """stream= given while torch's current stream is another one, which is busy: the output the wrapper creates (and fills with NaN
    or -7) must be ordered on `stream`, in front of the kernels -- read after both streams have run dry it is the result, never the fill."""
    import torch
    case = cases()[name]
    e_real = case.expectation(0)
    s = scheme_streams()[0]                                  # runs beside torch's default stream
    with api.Context(0, *case.dims) as ctx:
        t = buffers(case, case.inputs(0))
        torch.cuda.synchronize()
        t_call = 0.0
        for _ in range(2):
            t0 = time.perf_counter()
            case.wrap(ctx, t, s.cuda_stream)
            t_call = time.perf_counter() - t0
            torch.cuda.synchronize()
        d_ms = delay_for(t_call)
        marker = delayed(torch.cuda.default_stream(), d_ms)      # torch's current stream is busy; s is idle
        ret = case.wrap(ctx, t, s.cuda_stream)
        pending = not marker.query()
        s.synchronize()
        torch.cuda.synchronize()
        got = {k: host(v) for k, v in ret.items()}
    report("wrapper: " + name, t_call, d_ms)
    assert pending, f"{name}: torch's current stream was idle again when the wrapper returned ({d_ms:.0f} ms delay)"
    for k, v in got.items():
        n = case.rows[k](e_real) if k in case.rows else len(v)     # (rows that the call leaves unwritten are not compared)
        assert n > 0
        assert_same(v[:n], e_real[k][:n], f"wrapper {name}: {k} created by default", k)


# ---------------------------------------------------------------------------------------------------------------- 7. the controls
def escaped_call(s, escape_to):
    """The scheme on a deliberate misuse: the producer copy on `s` behind the delay, the call on `escape_to`, which is idle (valid
    data, nothing out of range).  Returns what the call made, expectation(decoy), expectation(real) and whether the delay on `s` was
    still running when the call was through."""
    import torch
    case = cases()["complete streaming 64x96 batch 8"]
    e_real, e_decoy = case.expectation(0), case.expectation(1)
    check_distinct(case, e_real, e_decoy)
    real = {k: dev(v) for k, v in case.inputs(0).items()}
    with api.Context(0, *case.dims) as ctx:
        t = buffers(case, case.inputs(1))
        decoy, t_call = warm_up(case, ctx, t, escape_to)
        d_ms = delay_for(t_call)
        marker = delayed(s, d_ms)
        with torch.cuda.stream(s):
            for k in real:
                t[k].copy_(real[k])
        with torch.cuda.stream(escape_to):
            case.call(ctx, t, escape_to.cuda_stream)
            clone = t["dst"].clone()
        escape_to.synchronize()
        pending = not marker.query()
        s.synchronize()
        got = host(clone)
    report("control", t_call, d_ms)
    return got, e_decoy["dst"], e_real["dst"], pending


@gpu
def test_control_a_call_that_escapes_to_the_null_stream_is_seen():
    """Where a launch or copy that lost its stream argument lands: the null stream.  On the stream every scheme here runs on, such
    a call reads the decoys: its result is expectation(decoy) exactly, which the scheme's comparison with expectation(real) rejects."""
    import torch
    got, e_decoy, e_real, pending = escaped_call(scheme_streams()[0], torch.cuda.default_stream())
    assert pending, "the delay on `s` was over before the call on the null stream had finished"
    assert_same(got, e_decoy, "control: a call on the null stream reads the decoys")
    assert not same_bits(got, e_real)


@gpu
def test_control_a_call_that_escapes_to_another_stream_is_seen():
    """The same with the call on a second stream (the one the two-context test gives to context B)."""
    s, s2 = scheme_streams()
    got, e_decoy, e_real, pending = escaped_call(s, s2)
    assert pending, "the delay on `s` was over before the call on the idle stream had finished"
    assert_same(got, e_decoy, "control: a call on another stream than its producer reads the decoys")
    assert not same_bits(got, e_real)
