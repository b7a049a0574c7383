"""Every *_dev entry point captured into a graph once and replayed on new inputs (include/dcmt.h, "Graph capture").

A replay runs the captured kernels with the arguments the host computed at capture time: whatever a call derives on the host from
state that advances per call -- the winner plane's generation, the slot of the 16-bit attempt's flag -- is frozen in the graph,
while the context goes on advancing under the eager calls made beside it.  The scheme, one helper (run_replayed) for every case,
built on the machinery of tests/test_gpu_stream_order.py (Case, Out, buffers, refill, assert_same, check_distinct) and on the case
builders of the other GPU test files, imported, with the shapes they have there:

    a fresh Context; static buffers holding input set 1 (the decoys) and outputs holding the fill; ONE eager warm-up call on a side
    stream `s` (code objects, the documented first-use allocations); the buffers restored;
    g = torch.cuda.CUDAGraph(); with torch.cuda.graph(g, stream=s): the call, on torch's current stream.  The default capture error
    mode is the strict one: an allocation or a synchronisation by the library fails the capture, and with it the test.  One stream,
    no fork or join: every graph here is a straight line of nodes;
    after the capture nothing has run (the outputs hold the fill) and dcmt_last_path names the captured route;
    for the input sets 0, 2, 3, 0: copy the set into the static inputs on `s`, refill the outputs, g.replay(), clone the outputs,
    synchronise; every clone is, bit for bit, case.expectation(set): the oracle (or the file's restatement) where the case has one,
    else the same call made alone on a fresh context.  Returning to set 0 shows that nothing of sets 2 and 3 survives;
    then, on the same context and graph: replay(0), eager(1), replay(2), eager(3), replay(0), the eager calls on the same buffers
    and stream -- where the graph's frozen state and the context's advancing state meet.  All five results are compared;
    where the case reports (last_fill_iters), the counts after every step are the oracle's for that step's inputs.

check_distinct runs on every pair of the four expectations, so a stale result cannot pass.  A failing case reports every step that
differs, not the first one only.  The last test is the control: the same comparison on a captured "call" whose argument is a Python
counter rejects the second replay."""
import time

import numpy as np
import pytest

import test_gpu_stream_order as SO
from depth_completion_mt_amd import _lib as L
from depth_completion_mt_amd import api, synth

gpu = pytest.mark.gpu
f32, i16, i32, u8 = np.float32, np.int16, np.int32, np.uint8

ORDER = (0, 2, 3, 0)                                         # the replays of the first part
MIXED = (("replay", 0), ("eager", 1), ("replay", 2), ("eager", 3), ("replay", 0))
SETS = (0, 1, 2, 3)
SPEC = SO.SPEC


# ---------------------------------------------------------------------------------------------------------------- the scheme
def expectations(case):
    """The four expectations of a case, told apart pairwise and from the fill."""
    exp = {w: case.expectation(w) for w in SETS}
    for a in SETS:
        for b in SETS:
            if a != b:
                SO.check_distinct(case, exp[a], exp[b])
    return exp


def differences(case, got, want, what):
    """SO.assert_same on every output; the messages of those that differ."""
    out = []
    for name in case.outputs:
        try:
            SO.assert_same(got[name], want[name], f"{case.name}: {what}: {name}", name)
        except AssertionError as e:
            out.append(str(e))
    return out


class Replayed:
    """A case on a fresh context, warmed up once and captured: step("replay" | "eager", which) loads input set `which` into the static
    buffers, refills the outputs, replays the graph or makes the call eagerly, and returns the clones as host arrays."""

    def __init__(self, case):
        import torch
        self.case, self.s = case, SO.scheme_streams()[0]
        self.sets = {w: {k: SO.dev(v) for k, v in case.inputs(w).items()} for w in SETS}
        self.ctx = api.Context(0, *case.dims)
        self.t = SO.buffers(case, case.inputs(1))
        torch.cuda.synchronize()
        case.call(self.ctx, self.t, self.s.cuda_stream)      # the one warm-up
        self.s.synchronize()
        self.load(1)
        self.s.synchronize()
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph, stream=self.s):
            self.ret = case.call(self.ctx, self.t, torch.cuda.current_stream().cuda_stream) or {}
        torch.cuda.synchronize()

    def load(self, which):
        import torch
        with torch.cuda.stream(self.s):
            for k, v in self.sets[which].items():
                self.t[k].copy_(v)
            SO.refill(self.case, self.t)

    def untouched(self):
        """Capturing runs nothing: the outputs hold the fill, an in-place output its input."""
        for name, o in self.case.outputs.items():
            if o.returned:
                continue
            got = SO.host(self.t[name])
            if name in self.case.inputs(1):
                assert SO.same_bits(got, self.case.inputs(1)[name]), f"{self.case.name}: {name} was written during the capture"
            else:
                assert (got == SO.fill_of(o.dtype)).all(), f"{self.case.name}: {name} was written during the capture"

    def step(self, kind, which):
        import torch
        self.load(which)
        with torch.cuda.stream(self.s):
            if kind == "replay":
                self.graph.replay()
                ret = self.ret
            else:
                ret = self.case.call(self.ctx, self.t, self.s.cuda_stream) or {}
            clones = {name: (ret[name] if o.returned else self.t[name]).clone() for name, o in self.case.outputs.items()}
        self.s.synchronize()
        return {k: SO.host(v) for k, v in clones.items()}

    def close(self):
        import torch
        torch.cuda.synchronize()
        self.graph = self.ret = None
        self.ctx.close()


def run_replayed(case, path=None, not_path=None):
    """The scheme of the module docstring on one case.  path / not_path: what dcmt_last_path must (not) contain after the capture."""
    exp = expectations(case)
    t0 = time.perf_counter()
    r = Replayed(case)
    try:
        r.untouched()
        if path is not None:
            p = r.ctx.last_path()
            assert path in p and (not_path is None or not_path not in p), f"{case.name}: the captured route is {p!r}"
        bad = []
        steps = [("replay", w, f"replay {i} (set {w})") for i, w in enumerate(ORDER)]
        steps += [(kind, w, f"mixed step {i}: {kind} (set {w})") for i, (kind, w) in enumerate(MIXED)]
        for kind, w, what in steps:
            got = r.step(kind, w)
            bad += differences(case, got, exp[w], what)
            if case.after:                                   # the completion cases with iters=True: the counts of THIS step's inputs
                try:
                    case.after(r.ctx, exp[w])
                except AssertionError as e:
                    bad.append(f"{case.name}: {what}: last_fill_iters: {e}")
    finally:
        r.close()
    print(f"[graph-replay] {case.name}: {len(steps)} steps, {len(bad)} differences, test_s {time.perf_counter() - t0:.2f}")
    assert not bad, "\n".join(bad)


# ---------------------------------------------------------------------------------------------------------------- cases of this file
def grid_frames(b, rows, cols, seed):
    """Frames on the 1/256 m grid (what the 16-bit form takes) with one frame that needs the hole-closure loop."""
    x = SO.sparse_frames(b, rows, cols, seed, gap=True)
    return (np.round(x * 256.0) / 256.0).astype(f32)


def q16_case():
    """The 16-bit form (k_pre_p<Q16OUT> + k_fp_q; DCMT_Q16_MIN_WAVES=0 when the context is created).  Sets 0, 1 and 3 lie on the grid;
    set 2 has one frame off it, as tests/test_gpu_fuzz.py makes one: the replays see on-grid, off-grid, on-grid, on-grid."""
    b, rows, cols = 8, 64, 96

    def inputs(which):
        x = grid_frames(b, rows, cols, 2100 + 50 * which)
        if which == 2:
            x[5] = (x[5] * f32(1.003)).astype(f32)
        return {"src": x}

    def call(ctx, t, st):
        ctx.complete_dev(t["src"], t["dst"], api.make_params(spec_fill_iters=SPEC), stream=st)

    def expect(inp):
        out = []
        for f in range(b):
            y, info = SO.O().img_completion(inp["src"][f], return_info=True)
            assert info["rc"] == 0 and info["fill_iters"] < SPEC, (f, info)
            out.append(y)
        return {"dst": np.stack(out)}

    return SO.Case("complete 16-bit form 64x96 batch 8", (rows, cols, b), inputs, {"dst": SO.Out((b, rows, cols), f32)}, call, expect)


def iters_case():
    """tests/test_gpu_stream_order.py's last_fill_iters case with the frame that needs the hole-closure loop at another place in
    every input set, so that every set has counts of its own: a report that stayed with the capture's, or an earlier replay's, differs."""
    base = SO.cases()["last_fill_iters behind complete 64x96 batch 8"]
    case = SO.Case("last_fill_iters behind a replay 64x96 batch 8", base.dims, lambda which: {"src": np.roll(base.inputs(which)["src"], 2 * which, axis=0)},
                   base.outputs, base.call, base.expect, base.after)
    counts = [tuple(case.expectation(w)["_iters"]) for w in SETS]
    assert len(set(counts)) == len(SETS), counts
    return case


def in_place_case():
    """An in-place call whose result goes to scratch first (" + copy to dst"): the cascade without the extrapolation, dst = src."""
    import no_extrapolate_restatement as R
    import test_gpu_no_extrapolate as NE
    b, rows, cols = 3, 64, 250

    def call(ctx, t, st):
        ctx.complete_dev(t["src"], t["src"], NE.p(), stream=st)

    def expect(inp):
        return {"src": np.stack([R.restatement_oracle(f) for f in inp["src"]])}

    return SO.Case("complete without extrapolation in place 64x250 batch 3", (rows, cols, b), lambda which: {"src": SO.sparse_frames(b, rows, cols, 2300 + 50 * which)},
                   {"src": SO.Out((b, rows, cols), f32)}, call, expect)


def payload(x):
    """A depth plane as the KITTI uint16 payload (metres * 256), as int16 bits: what torch holds."""
    return np.round(x * 256.0).astype(np.uint16).view(i16)


def occlusion_u16_case(rows=40, cols=133, b=3):
    import occlusion_restatement as R

    def inputs(which):
        return {"sparse": payload(np.stack([R.sparse_plane(rows, cols, 0.3, 900 + 10 * which + f, specials=False) for f in range(b)]))}

    def call(ctx, t, st):
        ctx.sparse_occlusion_dev(t["sparse"], t["out"], d_removed=t["removed"], u16=True, stream=st)

    return SO.Case("sparse_occlusion uint16", (rows, cols, b), inputs, {"out": SO.Out((b, rows, cols), i16), "removed": SO.Out((b,), i32)}, call)


def support_u16_case(rows=40, cols=133, b=3):
    import support_restatement as R

    def inputs(which):
        g = np.random.Generator(np.random.PCG64(950 + which))
        return {"sparse": payload(np.stack([R.sparse_plane(rows, cols, 0.01, 900 + 10 * which + f, specials=False) for f in range(b)])),
                "dense": g.uniform(1.0, 90.0, (b, rows, cols)).astype(f32), "fallback": g.uniform(1.0, 90.0, (b, rows, cols)).astype(f32)}

    def call(ctx, t, st):
        ctx.support_distance_dev(t["sparse"], t["dense"], t["fallback"], d_out=t["out"], d_dist2=t["dist2"], d_beyond=t["beyond"], u16=True, stream=st)

    outs = {"out": SO.Out((b, rows, cols), f32), "dist2": SO.Out((b, rows, cols), i16), "beyond": SO.Out((b,), i32)}
    return SO.Case("support_distance uint16", (rows, cols, b), inputs, outs, call)


def normals_calib_case(rows=40, cols=133, b=3):
    import normals_restatement as N
    ref = api.make_cloud_params()

    def inputs(which):
        k = [1.0 + 0.1 * f + 0.03 * which for f in range(b)]
        tab = api.make_normals_calib([ref.fx * x for x in k], [ref.fy * x for x in k], [ref.cx + 2.0 * f for f in range(b)], ref.cy)
        return {"depth": np.stack([N.holey_plane(rows, cols, 900 + 10 * which + f, specials=False) for f in range(b)]),
                "calib": tab.view(u8).reshape(b, -1)}

    def call(ctx, t, st):
        ctx.depth_normals_calib_dev(t["depth"], t["calib"], d_normals=t["normals"], d_out=t["out"], d_counts=t["counts"], stream=st, min_plane_dist=3.0)

    outs = {"normals": SO.Out((b, rows, cols, 4), f32), "out": SO.Out((b, rows, cols), f32), "counts": SO.Out((b, 2), i32)}
    return SO.Case("depth_normals_calib", (rows, cols, b), inputs, outs, call)


def photo_calib_case(rows=65, cols=257, b=3, window=2):
    import test_gpu_photo_error as PE
    base = PE.photo_case(rows, cols, b, window)

    def inputs(which):
        d = dict(base.inputs(which))
        tab = api.make_stereo_calib([0.54 * (1.0 + 0.1 * f) for f in range(b)], [959.791 * (1.0 + 0.05 * which + 0.02 * f) for f in range(b)])
        d["calib"] = tab.view(u8).reshape(b, -1)
        return d

    def call(ctx, t, st):
        ctx.photo_error_calib_dev(t["depth"], t["left"], t["right"], t["calib"], d_err=t["err"], d_stats=t["stats"], stream=st, window=window)

    return SO.Case("photo_error_calib 65x257", (rows, cols, b), inputs, dict(base.outputs), call)


def sgm_case(kind, rows=9, cols=65, D=48, b=3):
    """The four forms of the matcher on one small shape of tests/test_gpu_sgm.py, both outputs, the workspace given (one frame in
    flight: the batch goes through it in three chunks)."""
    import test_gpu_sgm as G
    kw = dict(num_disparities=D, focal=80.0)
    kw.update({"4 paths": {}, "8 paths": {"paths": 8}, "guided": {}, "census": {"cost": "census"}}[kind])
    work = api.sgm_workspace_bytes(rows, cols, D, 1)
    assert work > 0

    def inputs(which):
        pairs = [G.pair("shifted", rows, cols, D, seed=1000 + 10 * which + f) for f in range(b)]
        d = {"left": np.stack([p[0] for p in pairs]), "right": np.stack([p[1] for p in pairs]), "work": np.zeros(work, u8)}
        if kind == "guided":
            g = np.random.default_rng(1100 + which)
            d["guide"] = np.where(g.random((b, rows, cols)) < 0.3, g.uniform(1.0, 40.0, (b, rows, cols)), 0.0).astype(f32)
        return d

    def call(ctx, t, st):
        ctx.sgm_dev(t["left"], t["right"], d_disp16=t["disp"], d_depth=t["depth"], d_work=t["work"], d_guide=t.get("guide"), stream=st, **kw)

    return SO.Case(f"sgm {kind} 9x65 D=48", (rows, cols, b), inputs, {"disp": SO.Out((b, rows, cols), i16), "depth": SO.Out((b, rows, cols), f32)}, call)


def speckle_case(rows=17, cols=65, b=3):
    import speckle_restatement as R

    def inputs(which):
        g = np.random.default_rng(1200 + which)
        return {"disp": np.stack([R.random_plane(rows, cols, 3, 0.6, 1200 + 10 * which + f, -16) for f in range(b)]),
                "depth": g.uniform(1.0, 80.0, (b, rows, cols)).astype(f32)}

    def call(ctx, t, st):
        ctx.filter_speckles_dev(t["disp"], d_depth=t["depth"], d_out=t["out"], d_removed=t["removed"], stream=st, max_size=5, max_diff=16)

    outs = {"out": SO.Out((b, rows, cols), i16), "depth": SO.Out((b, rows, cols), f32), "removed": SO.Out((b,), i32)}
    return SO.Case("filter_speckles 17x65", (rows, cols, b), inputs, outs, call)


def rectify_map_case(b=3):
    import test_gpu_rectify as RT

    def inputs(which):
        return {"table": np.ascontiguousarray(RT.table9()[2 * which:2 * which + b]).view(u8).reshape(b, -1)}

    def call(ctx, t, st):
        ctx.rectify_map_dev(t["table"], RT.ROWS, RT.COLS, t["map"], stream=st)

    return SO.Case("rectify_map 37x131", (RT.ROWS, RT.COLS, b), inputs, {"map": SO.Out((b, RT.ROWS, RT.COLS, 2), i32)}, call)


def rectify_case(b=3):
    import rectify_restatement as R
    import test_gpu_rectify as RT

    def inputs(which):
        return {"src": R.noise((b,) + RT.SRC + (3,), 1300 + which), "map": np.ascontiguousarray(RT.maps9()[2 * which:2 * which + b])}

    def call(ctx, t, st):
        ctx.rectify_dev(t["src"], t["map"], out=t["dst"], stream=st)

    return SO.Case("rectify 41x150 -> 37x131", (max(RT.ROWS, RT.SRC[0]), max(RT.COLS, RT.SRC[1]), b), inputs,
                   {"dst": SO.Out((b, RT.ROWS, RT.COLS, 3), u8)}, call)


def pipeline_case(p):
    """A tests/test_gpu_stream_order.py Pipeline (its body and its expectations) as a case: the whole chain is one captured graph."""
    outs = {k: SO.Out(shape, dtype, per_frame) for k, (shape, dtype, per_frame) in p.outputs.items()}
    return SO.Case(p.name, p.dims, p.inputs, outs, lambda ctx, t, st: p.calls(ctx, t, st), p.expect)


def lidar_chain_case(rows=40, cols=133, b=3):
    """project (nearest wins) -> occlusion filter in place -> completion -> trust mask in place -> joint bilateral -> normals -> cloud,
    one graph.  Every link has its own restatement in its own file; here the chain replayed equals the chain made alone."""
    import joint_restatement as J
    pc = SO.project_case()
    T = synth.KITTI_T_VELO_TO_CAM
    P = np.array([[60.0, 0, cols / 2, 3.0], [0, 60.0, rows / 2, 0.01], [0, 0, 1, 0.002]], f32)
    tab = J.as_record(*J.tables(3, **J.SIGMAS)).view(u8).reshape(1, -1)

    def inputs(which):
        d = dict(pc.inputs(which))
        d["guide"] = np.stack([J.guide_plane(rows, cols, 3, 1400 + 10 * which + f) for f in range(b)])
        d["tables"] = tab
        return d

    def call(ctx, t, st):
        ctx.project_points_dev(t["pts"], t["off"], T, P, rows, cols, t["sparse"], stream=st, nearest=True)
        ctx.sparse_occlusion_dev(t["sparse"], t["sparse"], d_removed=t["removed"], stream=st)
        ctx.complete_dev(t["sparse"], t["dense"], api.make_params(spec_fill_iters=SPEC), stream=st)
        ctx.support_distance_dev(t["sparse"], t["dense"], None, d_out=t["dense"], d_beyond=t["beyond"], stream=st, max_radius=6)
        ctx.joint_bilateral_dev(t["dense"], t["guide"], t["tables"], d_out=t["filled"], stream=st, radius=3, smooth=True)
        ctx.depth_normals_dev(t["filled"], d_normals=t["normals"], d_out=t["kept"], stream=st, min_plane_dist=1.0)
        ctx.depth_to_cloud_dev(t["kept"], t["guide"], d_points=t["points"], d_offsets=t["offsets"], stream=st)

    img = SO.Out((b, rows, cols), f32)
    outs = {"sparse": img, "removed": SO.Out((b,), i32), "dense": img, "beyond": SO.Out((b,), i32), "filled": img,
            "normals": SO.Out((b, rows, cols, 4), f32), "kept": img, "points": SO.Out((b * rows * cols, 4), f32, per_frame=False),
            "offsets": SO.Out((b + 1,), i32, per_frame=False)}
    return SO.Case("chain lidar + camera", (rows, cols, b), inputs, outs, call)


def stereo_chain_case(rows=24, cols=70, D=16, b=2):
    """BGR -> grey (left, right) -> SGM -> speckle filter -> refinement -> reprojection, one graph; replayed = made alone."""
    import test_gpu_sgm as G
    work = api.sgm_workspace_bytes(rows, cols, D, 1)
    M = np.eye(4, dtype=f32)
    M[0, 3] = 0.5
    kw = dict(num_disparities=D, focal=80.0)

    def inputs(which):
        pairs = [G.pair("shifted", rows, cols, D, seed=1500 + 10 * which + f) for f in range(b)]
        grey = lambda k: np.stack([p[k] for p in pairs])
        return {"bgr_l": np.ascontiguousarray(np.repeat(grey(0)[..., None], 3, axis=3)), "bgr_r": np.ascontiguousarray(np.repeat(grey(1)[..., None], 3, axis=3)),
                "work": np.zeros(work, u8)}

    def call(ctx, t, st):
        ctx.bgr_convert_dev(t["bgr_l"], lab=False, d_gray=t["gray_l"], stream=st)
        ctx.bgr_convert_dev(t["bgr_r"], lab=False, d_gray=t["gray_r"], stream=st)
        ctx.sgm_dev(t["gray_l"], t["gray_r"], d_disp16=t["disp"], d_depth=t["depth"], d_work=t["work"], stream=st, **kw)
        ctx.filter_speckles_dev(t["disp"], d_depth=t["depth"], d_out=t["disp"], stream=st, max_size=5, max_diff=16)
        ctx.stereo_refine_dev(t["depth"], t["gray_l"], t["gray_r"], t["refined"], stream=st, focal=80.0)
        ctx.reproject_depth_dev(t["refined"], rows, cols, api.make_reproject_params(M=M, fx=80.0, fy=80.0, cx=cols / 2, cy=rows / 2,
                                                                                    K=[[80.0, 0, cols / 2], [0, 80.0, rows / 2], [0, 0, 1]]), t["warped"], stream=st)

    img, px = SO.Out((b, rows, cols), f32), SO.Out((b, rows, cols), u8)
    outs = {"gray_l": px, "gray_r": px, "disp": SO.Out((b, rows, cols), i16), "depth": img, "refined": img, "warped": img}
    return SO.Case("chain stereo", (rows, cols, b), inputs, outs, call)


# ---------------------------------------------------------------------------------------------------------------- the case list
def _so(name):
    return lambda: SO.cases()[name]


def _mod(module, fn, *a):
    def make():
        import importlib
        return getattr(importlib.import_module(module), fn)(*a)
    return make


def _nearest(key):
    def make():
        import test_gpu_nearest as NR
        return NR.STREAM_CASES[key]()
    return make


def _pipeline(fn):
    return lambda: pipeline_case(getattr(SO, fn)())


# id: (maker, the entry points of include/dcmt.h the case calls, what dcmt_last_path holds after the capture, what it must not hold)
CASES = {
    # the cascade, every route of plan_call
    "complete staged": (_so("complete staged 48x64 batch 2"), ["dcmt_complete_f32_dev"], "staged tile kernels", None),
    "complete streaming f32": (_so("complete streaming 64x96 batch 8"), ["dcmt_complete_f32_dev"], "k_fp_s", "k_fp_q"),
    "complete labeled streaming": (_so("complete labeled 40x56 batch 8"), ["dcmt_complete_labeled_f32_dev"], "k_label_bbox + k_label_stage + k_pre_", None),
    "complete labeled staged": (_so("complete labeled 40x56 batch 2"), ["dcmt_complete_labeled_f32_dev"], "k_pre_labeled_v1", None),
    "complete uint16": (_so("complete_u16 64x96 batch 8"), ["dcmt_complete_u16_dev"], "U16", None),
    "complete normalize in front": (_so("complete normalize=(0, 80) streaming"), ["dcmt_complete_f32_dev"], "k_pre_p<NORM>", None),
    "complete no_extrapolate + cloud": (_mod("test_gpu_no_extrapolate", "cloud_case"), ["dcmt_complete_f32_dev", "dcmt_depth_to_cloud_dev"], "k_local", "copy to dst"),
    "complete bilateral finish": (_mod("test_gpu_bilateral", "cascade_case"), ["dcmt_complete_f32_dev"], " + bilateral5", None),
    "complete gaussian_valid finish": (_mod("test_gpu_gauss_valid", "extrapolating_case"), ["dcmt_complete_f32_dev"], " + gauss5_valid", None),
    "complete gaussian_valid k_local": (_mod("test_gpu_gauss_valid", "local_case"), ["dcmt_complete_f32_dev"], "k_local<VALID>", None),
    "complete 16-bit form": (q16_case, ["dcmt_complete_f32_dev"], "k_fp_q", None),
    "complete in place": (in_place_case, ["dcmt_complete_f32_dev"], " + copy to dst", None),
    "last_fill_iters": (iters_case, ["dcmt_complete_f32_dev"], "k_fp_s", None),
    # the winner plane
    "project_points": (_so("project_points 40x133 ragged"), ["dcmt_project_points_dev"], None, None),
    "reproject_depth": (_so("reproject_depth 48x64 -> 40x70"), ["dcmt_reproject_depth_dev"], None, None),
    "project_points_calib": (_mod("test_gpu_calib", "stream_order_case", "project"), ["dcmt_project_points_calib_dev"], None, None),
    "reproject_depth_calib": (_mod("test_gpu_calib", "stream_order_case", "reproject"), ["dcmt_reproject_depth_calib_dev"], None, None),
    # the rest
    "depth_to_cloud_calib": (_mod("test_gpu_calib", "stream_order_case", "cloud"), ["dcmt_depth_to_cloud_calib_dev"], None, None),
    "stereo_refine_calib": (_mod("test_gpu_calib", "stream_order_case", "stereo"), ["dcmt_stereo_refine_calib_dev"], None, None),
    "project nearest": (_nearest("project uniform"), ["dcmt_project_points_nearest_dev"], None, None),
    "project nearest calib": (_nearest("project table"), ["dcmt_project_points_nearest_calib_dev"], None, None),
    "reproject nearest": (_nearest("reproject uniform"), ["dcmt_reproject_depth_nearest_dev"], None, None),
    "reproject nearest calib": (_nearest("reproject table"), ["dcmt_reproject_depth_nearest_calib_dev"], None, None),
    "slic_labels": (_so("slic_labels 70x130 step 16"), ["dcmt_slic_labels_dev"], None, None),
    "slic_connectivity": (_mod("test_gpu_connectivity", "stream_case", False), ["dcmt_slic_connectivity_dev"], None, None),
    "slic_connectivity in place": (_mod("test_gpu_connectivity", "stream_case", True), ["dcmt_slic_connectivity_dev"], None, None),
    "slic renderings + labeled": (_mod("test_gpu_contours", "stream_case"), ["dcmt_slic_contours_dev", "dcmt_slic_cluster_means_dev", "dcmt_complete_labeled_f32_dev"],
                                  "k_label_bbox", None),
    "superpixel_planes": (_mod("test_gpu_planes", "stream_case"), ["dcmt_superpixel_planes_dev"], None, None),
    "stereo_refine": (_so("stereo_refine 48x64 iterations=None"), ["dcmt_stereo_refine_dev"], None, None),
    "gaussian5": (_so("gaussian5 out of place"), ["dcmt_gaussian5_dev"], None, None),
    "gaussian5 in place": (_so("gaussian5 in place"), ["dcmt_gaussian5_dev"], None, None),
    "gaussian5_valid": (_mod("test_gpu_gauss_valid", "stand_alone_case", False), ["dcmt_gaussian5_valid_dev"], None, None),
    "bilateral5": (_mod("test_gpu_bilateral", "stand_alone_case", False), ["dcmt_bilateral5_dev"], None, None),
    "evaluate": (_so("evaluate f32 ground truth"), ["dcmt_evaluate_dev"], None, None),
    "evaluate uint16": (_so("evaluate uint16 ground truth"), ["dcmt_evaluate_u16_dev"], None, None),
    "colorize": (_so("colorize"), ["dcmt_colorize_dev"], None, None),
    "bgr_convert": (_so("bgr_convert both"), ["dcmt_bgr_convert_dev"], None, None),
    "bgr_convert in place": (_so("bgr_convert in place"), ["dcmt_bgr_convert_dev"], None, None),
    "depth_to_cloud": (_so("depth_to_cloud with colour"), ["dcmt_depth_to_cloud_dev"], None, None),
    "crop_frames": (_mod("test_gpu_crop_export", "crop_case"), ["dcmt_crop_frames_dev"], None, None),
    "depth_to_u16": (_mod("test_gpu_crop_export", "export_case"), ["dcmt_depth_to_u16_dev"], None, None),
    "photo_error": (_mod("test_gpu_photo_error", "photo_case", 65, 257, 3, 2), ["dcmt_photo_error_dev"], None, None),
    "photo_error_calib": (photo_calib_case, ["dcmt_photo_error_calib_dev"], None, None),
    "sgm": (lambda: sgm_case("4 paths"), ["dcmt_sgm_dev"], None, None),
    "sgm_paths": (lambda: sgm_case("8 paths"), ["dcmt_sgm_paths_dev"], None, None),
    "sgm_guided": (lambda: sgm_case("guided"), ["dcmt_sgm_guided_dev"], None, None),
    "sgm_cost": (lambda: sgm_case("census"), ["dcmt_sgm_cost_dev"], None, None),
    "filter_speckles": (speckle_case, ["dcmt_filter_speckles_dev"], None, None),
    "rectify_map": (rectify_map_case, ["dcmt_rectify_map_dev"], None, None),
    "rectify": (rectify_case, ["dcmt_rectify_dev"], "k_rectify", None),
    "sparse_occlusion": (_mod("test_gpu_occlusion", "stream_case", False), ["dcmt_sparse_occlusion_dev"], None, None),
    "sparse_occlusion in place": (_mod("test_gpu_occlusion", "stream_case", True), ["dcmt_sparse_occlusion_dev"], None, None),
    "sparse_occlusion uint16": (occlusion_u16_case, ["dcmt_sparse_occlusion_u16_dev"], None, None),
    "support_distance": (_mod("test_gpu_support", "stream_case", False), ["dcmt_support_distance_dev"], None, None),
    "support_distance in place": (_mod("test_gpu_support", "stream_case", True), ["dcmt_support_distance_dev"], None, None),
    "support_distance uint16": (support_u16_case, ["dcmt_support_distance_u16_dev"], None, None),
    "joint_bilateral": (_mod("test_gpu_joint", "stream_case"), ["dcmt_joint_bilateral_dev"], None, None),
    "depth_normals": (_mod("test_gpu_normals", "stream_case", False), ["dcmt_depth_normals_dev"], None, None),
    "depth_normals in place": (_mod("test_gpu_normals", "stream_case", True), ["dcmt_depth_normals_dev"], None, None),
    "depth_normals_calib": (normals_calib_case, ["dcmt_depth_normals_calib_dev"], None, None),
    # whole pipelines, each one graph
    "pipeline lidar + camera": (_pipeline("lidar_camera_pipeline"), ["dcmt_bgr_convert_dev", "dcmt_slic_labels_dev", "dcmt_complete_labeled_f32_dev", "dcmt_evaluate_dev"], None, None),
    "pipeline stereo + lidar": (_pipeline("stereo_lidar_pipeline"),
                                ["dcmt_project_points_dev", "dcmt_complete_f32_dev", "dcmt_bgr_convert_dev", "dcmt_stereo_refine_dev", "dcmt_reproject_depth_dev",
                                 "dcmt_evaluate_dev", "dcmt_gaussian5_dev", "dcmt_colorize_dev", "dcmt_depth_to_cloud_dev"], None, None),
    "chain lidar + camera": (lidar_chain_case, ["dcmt_project_points_nearest_dev", "dcmt_sparse_occlusion_dev", "dcmt_complete_f32_dev", "dcmt_support_distance_dev",
                                                "dcmt_joint_bilateral_dev", "dcmt_depth_normals_dev", "dcmt_depth_to_cloud_dev"], None, None),
    "chain stereo": (stereo_chain_case, ["dcmt_bgr_convert_dev", "dcmt_sgm_dev", "dcmt_filter_speckles_dev", "dcmt_stereo_refine_dev", "dcmt_reproject_depth_dev"], None, None),
}
Q16 = ("complete 16-bit form",)                              # cases whose context is created with DCMT_Q16_MIN_WAVES=0

_made = {}


def case_of(cid):
    """Built once per process: the expectations are cached on the case."""
    if cid not in _made:
        _made[cid] = CASES[cid][0]()
    return _made[cid]


# ---------------------------------------------------------------------------------------------------------------- without a GPU
def test_case_lists_name_every_case():
    """Every *_dev entry point include/dcmt.h declares (the names depth_completion_mt_amd/_lib.py checks the library's exports
    against) is called by at least one case: a new entry point cannot go in without one.  And no case names anything else."""
    declared = {n for n in L.EXPORTS if n.endswith("_dev")}
    named = {n for _, entries, _, _ in CASES.values() for n in entries}
    assert declared - named == set(), f"entry points without a graph-replay case: {sorted(declared - named)}"
    assert named - declared == set(), f"cases name what include/dcmt.h does not declare: {sorted(named - declared)}"
    assert len(declared) >= 45
    assert all(cid in CASES for cid in Q16)


def winners(landed, flat, index, n_px):
    """The winner plane one call leaves on a cleared plane: per pixel the largest index that landed there, -1 where none did."""
    w = np.full(n_px, -1, np.int64)
    np.maximum.at(w, flat[landed], index[landed])
    return w


def projection_planes(inp, rows, cols):
    """numpy's statement of N2 as oracle/np_restatement.py makes it, per input set: (winner plane of global point indices over the
    batch, depth of every point).  The depth of pixel px is z[winner[px]], 0 where the winner is -1."""
    T = np.asarray(synth.KITTI_T_VELO_TO_CAM, f32).reshape(4, 4)
    P = np.array([[60.0, 0, cols / 2, 3.0], [0, 60.0, rows / 2, 0.01], [0, 0, 1, 0.002]], f32)
    pts, off = inp["pts"], inp["off"]
    x, y, z = pts[:, 0], pts[:, 1], pts[:, 2]
    dot = lambda m, a, b, c: ((m[0] * a + m[1] * b) + m[2] * c) + m[3]
    tx, ty, tz = dot(T[0], x, y, z), dot(T[1], x, y, z), dot(T[2], x, y, z)
    px, py, pz = dot(P[0], tx, ty, tz), dot(P[1], tx, ty, tz), dot(P[2], tx, ty, tz)
    with np.errstate(divide="ignore", invalid="ignore"):
        uf, vf = px / pz, py / pz
        ok = (tz > 0) & (uf >= 0) & (uf < f32(cols)) & (vf >= 0) & (vf < f32(rows))
    frame = np.searchsorted(off, np.arange(len(pts)), side="right") - 1
    ok &= (frame >= 0) & (frame < len(off) - 1)
    flat = np.zeros(len(pts), np.int64)
    flat[ok] = (frame[ok] * rows + vf[ok].astype(np.int64)) * cols + uf[ok].astype(np.int64)
    return winners(ok, flat, np.arange(len(pts)), (len(off) - 1) * rows * cols), pz


def reprojection_planes(frames, orows, ocols, M):
    """tests/test_reproject.py's restatement with its winners kept: (winner plane of frame-local source pixel indices, t_2 of every
    source pixel), per frame."""
    import test_reproject as TR
    ws, zs = [], []
    for d in frames:
        uf, vf, t2 = TR._project(d, M, TR.CAMERA_MAT, TR.FX, TR.FY, TR.CX, TR.CY)
        with np.errstate(invalid="ignore"):
            land = ((t2 > 0) & (uf >= 0) & (uf < f32(ocols)) & (vf >= 0) & (vf < f32(orows))).ravel()
        flat = np.zeros(land.size, np.int64)
        flat[land] = vf.ravel()[land].astype(np.int64) * ocols + uf.ravel()[land].astype(np.int64)
        ws.append(winners(land, flat, np.arange(land.size), orows * ocols))
        zs.append(t2.ravel())
    return ws, zs


def resolve(w, z):
    return np.where(w >= 0, z[np.maximum(w, 0)], f32(0.0)).astype(f32)


def stale_report(w_before, w_now, z_now):
    """The model of "the plane was not cleared between two calls at one generation": the second call's atomicMax meets the first
    call's tags, the resolve reads the SECOND call's inputs at the index that survives.  Returns (pixels where that differs from the
    right answer, pixels that kept a larger earlier index, pixels that kept a winner although nothing landed now)."""
    right, stale = resolve(w_now, z_now), resolve(np.maximum(w_before, w_now), z_now)
    differ = right.view(np.uint32) != stale.view(np.uint32)
    return int(differ.sum()), int(((w_now >= 0) & (w_before > w_now)).sum()), int(((w_now < 0) & (w_before >= 0)).sum())


def test_projection_sets_make_stale_winners_visible():
    """No GPU.  For project_points and reproject_depth the input sets are such that a winner plane that is not cleared between two
    replays gives a wrong plane: from set 0 to set 2 (and along the rest of 0, 2, 3, 0) some pixels get a lower index than before,
    some that were hit stay empty, and the model's plane differs from the right one on at least 1 % of the pixels."""
    case = case_of("project_points")
    rows, cols, b = case.dims
    planes = {w: projection_planes(case.inputs(w), rows, cols) for w in SETS}
    for w in SETS:                                           # the model restates the oracle: its right answer is the oracle's
        SO.assert_same(resolve(*planes[w]).reshape(b, rows, cols), case.expectation(w)["sparse"], f"the numpy model of project_points, set {w}")
    for a, c in zip(ORDER, ORDER[1:]):
        differ, lower, left = stale_report(planes[a][0], *planes[c])
        print(f"[graph-replay] project_points, set {a} -> set {c}: the stale plane differs on {differ} of {b * rows * cols} pixels ({lower} kept a larger index, {left} kept a winner where nothing landed)")
        assert lower > 0 and left > 0 and differ >= 0.01 * b * rows * cols, (a, c, differ, lower, left)
    case = case_of("reproject_depth")
    orows, ocols = 40, 70
    M = np.eye(4, dtype=f32)
    M[0, 3] = 0.5
    import test_reproject as TR
    planes = {w: reprojection_planes(case.inputs(w)["depth"], orows, ocols, M) for w in SETS}
    for w in SETS:
        for f, d in enumerate(case.inputs(w)["depth"]):      # the model restates test_reproject.py's restatement
            SO.assert_same(resolve(planes[w][0][f], planes[w][1][f]).reshape(orows, ocols), TR.np_reproject(d, orows, ocols, M=M), f"the numpy model of reproject_depth, set {w} frame {f}")
    for a, c in zip(ORDER, ORDER[1:]):
        rep = [stale_report(planes[a][0][f], planes[c][0][f], planes[c][1][f]) for f in range(len(planes[c][0]))]
        differ, lower, left = (sum(r[k] for r in rep) for k in range(3))
        n = len(rep) * orows * ocols
        print(f"[graph-replay] reproject_depth, set {a} -> set {c}: the stale plane differs on {differ} of {n} pixels ({lower} kept a larger index, {left} kept a winner where nothing landed)")
        assert lower > 0 and left > 0 and differ >= 0.01 * n, (a, c, differ, lower, left)


# ---------------------------------------------------------------------------------------------------------------- the replays
@gpu
@pytest.mark.parametrize("cid", list(CASES))
def test_entry_point_replayed_from_a_captured_graph(cid, monkeypatch):
    if cid in Q16:
        monkeypatch.setenv("DCMT_Q16_MIN_WAVES", "0")        # read by dcmt_create
    _, _, path, not_path = CASES[cid]
    run_replayed(case_of(cid), path, not_path)


# ---------------------------------------------------------------------------------------------------------------- the refusals
def capture(s, body):
    """body() captured on `s` with the default (strict) error mode; returns the graph."""
    import torch
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        body(torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return g


@gpu
def test_reports_refuse_while_their_stream_is_capturing_and_follow_the_replays():
    """dcmt_last_fill_iters and dcmt_last_holes_after_extend: DCMT_E_INVALID while the stream of the last call is capturing (they
    would have to synchronise it), the capture goes on undisturbed; after a replay and a synchronise of the stream it was launched
    on they give THAT replay's counts -- also where the replay ran on another stream than the one it was captured on."""
    import ctypes
    import torch
    case = case_of("last_fill_iters")
    b = case.dims[2]
    exp = {w: case.expectation(w) for w in (0, 2)}
    assert exp[0]["_iters"] != exp[2]["_iters"], "the two input sets need different counts"
    s, s2 = SO.scheme_streams()
    seen = {}
    with api.Context(0, *case.dims) as ctx:
        t = SO.buffers(case, case.inputs(1))
        torch.cuda.synchronize()
        case.call(ctx, t, s.cuda_stream)
        s.synchronize()

        def body(st):
            case.call(ctx, t, st)
            out = (ctypes.c_int * b)()                       # (the C functions: the wrappers raise on a status)
            seen["iters"] = L.lib().dcmt_last_fill_iters(ctx._h, out, b)
            seen["holes"] = L.lib().dcmt_last_holes_after_extend(ctx._h, out, b)
        g = capture(s, body)
        assert seen == {"iters": L.E_INVALID, "holes": L.E_INVALID}, seen
        for which, stream in ((0, s), (2, s2), (0, s2), (2, s)):
            src = SO.dev(case.inputs(which)["src"])
            torch.cuda.synchronize()
            with torch.cuda.stream(stream):
                t["src"].copy_(src)
                g.replay()
            stream.synchronize()
            SO.assert_same(SO.host(t["dst"]), exp[which]["dst"], f"replay of set {which} on {'the capture stream' if stream is s else 'another stream'}")
            got, st = ctx.last_fill_iters(b)
            assert st == L.OK and got == exp[which]["_iters"], (which, got, exp[which]["_iters"])
            holes = ctx.last_holes_after_extend(b)
            assert len(holes) == b and all(h >= 0 for h in holes) and (max(holes) > 0) == (max(exp[which]["_iters"]) > 1), (which, holes)
        torch.cuda.synchronize()
        del g


@gpu
def test_kernel_timing_and_verbose_refuse_a_capturing_call():
    """With dcmt_set_kernel_timing on, or verbose set, a completion call on a capturing stream returns DCMT_E_INVALID before it has
    enqueued anything -- an event recorded, or a line printed, once at capture time would mean nothing for the replays.  The capture
    stays valid, the same calls made eagerly are taken, and without the aids the call is captured."""
    import torch
    case = SO.cases()["complete streaming 64x96 batch 8"]
    want = case.expectation(0)["dst"]
    s = SO.scheme_streams()[0]
    verbose = api.make_params(spec_fill_iters=SPEC, force_fused=True)
    verbose.verbose = 2
    with api.Context(0, *case.dims) as ctx:
        t = SO.buffers(case, case.inputs(0))
        torch.cuda.synchronize()
        case.call(ctx, t, s.cuda_stream)
        s.synchronize()
        SO.refill(case, t)
        torch.cuda.synchronize()
        status = []

        def refused(fn):
            try:
                fn()
                status.append(L.OK)
            except api.DcmtError as e:
                status.append(e.status)

        def body(st):
            ctx.set_kernel_timing(True)
            refused(lambda: case.call(ctx, t, st))
            ctx.set_kernel_timing(False)
            refused(lambda: ctx.complete_dev(t["src"], t["dst"], verbose, stream=st))
            t["dst"].add_(1.0)                               # the graph's only node
        g = capture(s, body)
        assert status == [L.E_INVALID, L.E_INVALID], status
        with torch.cuda.stream(s):
            g.replay()
        s.synchronize()
        assert bool((t["dst"] == SO.fill_of(f32) + 1.0).all()), "a refused call left something in the graph"
        ctx.set_kernel_timing(True)
        case.call(ctx, t, s.cuda_stream)                     # eager: taken, with the events
        s.synchronize()
        SO.assert_same(SO.host(t["dst"]), want, "eager call with kernel timing on")
        assert len(ctx.last_kernel_times()) > 0
        ctx.set_kernel_timing(False)
        SO.refill(case, t)
        ctx.complete_dev(t["src"], t["dst"], verbose, stream=s.cuda_stream)
        s.synchronize()
        SO.assert_same(SO.host(t["dst"]), want, "eager call with verbose set")
        SO.refill(case, t)
        torch.cuda.synchronize()
        g2 = capture(s, lambda st: case.call(ctx, t, st))
        with torch.cuda.stream(s):
            g2.replay()
        s.synchronize()
        SO.assert_same(SO.host(t["dst"]), want, "captured without the aids")
        del g, g2


# ---------------------------------------------------------------------------------------------------------------- the control
@gpu
def test_control_a_value_frozen_at_capture_time_is_seen():
    """The scheme on a "call" that is a torch op whose argument is a Python counter, advanced per call: dst = src + counter.  Eager
    calls add 1, 2, 3, ...; the captured one adds, on every replay, what the counter was when it was captured.  The comparison with
    what the eager calls would have given takes the first replay and rejects the second."""
    import torch
    rows, cols, b = 48, 64, 3
    counter = [0]

    def call(ctx, t, st):
        counter[0] += 1
        torch.add(t["src"], float(counter[0]), out=t["dst"])

    case = SO.Case("control: a Python counter", (rows, cols, b), lambda which: {"src": SO.dense_frames(b, rows, cols, 1600 + which)},
                   {"dst": SO.Out((b, rows, cols), f32)}, call, lambda inp: {"dst": inp["src"]})
    r = Replayed(case)                                       # the warm-up is call 1, the capture call 2
    try:
        r.untouched()
        assert counter[0] == 2
        bad = []
        for i, w in enumerate(ORDER[:2]):
            want = {"dst": (case.inputs(w)["src"] + f32(2 + i)).astype(f32)}      # what eager call 2 + i gives
            bad.append(differences(case, r.step("replay", w), want, f"replay {i}"))
    finally:
        r.close()
    assert bad[0] == [], bad[0]
    assert len(bad[1]) == 1 and "elements differ bitwise" in bad[1][0], bad[1]
