"""Inputs and expectations of the per-frame calibration table tests (test_calib.py without a GPU, test_gpu_calib.py with one).

Every case is a batch whose frames carry visibly different records -- a small rotation and translation per frame, focal lengths
spread by tens of per cent -- and an expectation computed frame by frame, with the frame's own record, from the restatements that
already pin the uniform calls: oracle.project_points, oracle.stereo_refine, np_reproject (test_reproject.py), np_cloud
(test_cloud.py).  They are imported, not copied.  An expectation is computed once per case and shared (never modified).

power(case) is what makes the GPU comparison decisive: for every frame that has any input, the restatement's result with the
frame's own record differs, bit for bit, from its result with each other frame's record -- a kernel that picked another frame's
record cannot pass.  (A frame without input -- an empty sweep, an all-zero plane of the cloud -- gives the empty result under
every record and is left out; the cases say which.)"""
import numpy as np

from depth_completion_mt_amd import api, synth
from test_cloud import np_cloud, words
from test_reproject import np_reproject, rot

f32 = np.float32


def O():
    from oracle import oracle
    return oracle


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


class Case:
    """name; b frames; table: the make_*_calib array; frame(f, g) -> the restatement's result for frame f's input with record g
    (an array); empty: frames without input.  want(f) = frame(f, f), cached."""

    def __init__(self, name, b, table, frame, empty=(), **data):
        self.name, self.b, self.table, self.frame, self.empty = name, b, table, frame, tuple(empty)
        self.__dict__.update(data)
        self._want = {}

    def want(self, f):
        if f not in self._want:
            self._want[f] = self.frame(f, f)
        return self._want[f]


def power(case):
    for f in range(case.b):
        if f in case.empty:
            continue
        for g in range(case.b):
            if g != f:
                assert not same_bits(case.frame(f, g), case.want(f)), f"{case.name}: frame {f} gives the same bits with record {g} as with its own"


# ---------------------------------------------------------------------------------------------------------------- projection
def project_records(b, rows, cols):
    T = np.stack([rot(0.02 * (f + 1), -0.015 * (f + 1), (0.05 * f, -0.03 * f, 0.1 + 0.07 * f)) for f in range(b)])
    P = np.zeros((b, 3, 4), f32)
    for f in range(b):
        fx, fy = 0.5 * cols * (1 + 0.15 * f), 0.55 * rows * (1 + 0.2 * f)
        P[f] = [[fx, 0, cols / 2, 0.5 + 0.1 * f], [0, fy, rows / 2, -0.25], [0, 0, 1, 0.01 * (f + 1)]]
    return T, P


def project_case(name, rows, cols, sweeps, seed):
    """Points in camera-like coordinates, spread so that most of a sweep lands in the image under its OWN record; the image is tiny,
    so many pixels are decided by the last writer."""
    b = len(sweeps)
    T, P = project_records(b, rows, cols)
    g = np.random.default_rng(seed)
    parts = []
    for f, n in enumerate(sweeps):
        pts = np.empty((n, 4), f32)
        z = g.uniform(1.0, 40.0, n)
        pts[:, 2] = z
        pts[:, 0] = g.uniform(-0.5, 0.5, n) * (cols / P[f, 0, 0]) * z
        pts[:, 1] = g.uniform(-0.5, 0.5, n) * (rows / P[f, 1, 1]) * z
        pts[:, 3] = g.uniform(0, 1, n)
        if n == 1:
            pts[0, :3] = [0.02, -0.01, 7.0]                    # a sweep of one point: in the image under every record
        parts.append(pts)
    points = np.concatenate(parts)
    offsets = np.concatenate([[0], np.cumsum(sweeps)]).astype(np.int32)

    def frame(f, gidx):
        return O().project_points(points[offsets[f]:offsets[f + 1]], T[gidx], P[gidx], rows, cols)

    return Case(name, b, api.make_project_calib(T, P), frame, [f for f, n in enumerate(sweeps) if n == 0],
                points=points, offsets=offsets, T=T, P=P, rows=rows, cols=cols)


# ---------------------------------------------------------------------------------------------------------------- reprojection
def reproject_records(b, rows, cols, orows, ocols):
    M = np.stack([rot(0.01 * (f + 1), -0.02 * (f + 1), (0.1 * f, -0.05 * f, 0.2 + 0.1 * f)) for f in range(b)])
    K = np.zeros((b, 3, 3), f32)
    kw = []
    for f in range(b):
        K[f] = [[ocols * (1 + 0.3 * f), 0, ocols / 2], [0, orows * (1 + 0.25 * f), orows / 2], [0, 0, 1]]     # the source covers the whole destination
        kw.append(dict(fx=0.9 * cols * (1 + 0.2 * f), fy=0.9 * rows * (1 + 0.15 * f), cx=cols / 2 + 0.25 * f, cy=rows / 2 - 0.5 * f))
    return M, K, kw


def depth_frames(b, rows, cols, seed, zeros=0.15):
    g = np.random.default_rng(seed)
    x = g.uniform(0.5, 60.0, (b, rows, cols)).astype(f32)
    x[g.random(x.shape) < zeros] = 0.0
    return x


def reproject_table(M, K, kw):
    return api.make_reproject_calib(M, K, *[[k[n] for k in kw] for n in ("fx", "fy", "cx", "cy")])


def reproject_case(name, b, rows, cols, orows, ocols, seed, records=None, frames=None):
    M, K, kw = records or reproject_records(b, rows, cols, orows, ocols)
    frames = depth_frames(b, rows, cols, seed) if frames is None else frames

    def frame(f, g):
        return np_reproject(frames[f], orows, ocols, M=M[g], K=K[g], **kw[g])

    return Case(name, b, reproject_table(M, K, kw), frame, frames=frames, M=M, K=K, kw=kw, rows=rows, cols=cols, orows=orows, ocols=ocols)


# ---------------------------------------------------------------------------------------------------------------- cloud
def cloud_records(b, rows, cols):
    return [dict(fx=0.9 * cols * (1 + 0.2 * f), fy=-0.8 * rows * (1 + 0.3 * f) if f == 1 else 0.8 * rows * (1 + 0.3 * f),
                 cx=cols / 2 + 0.5 * f, cy=rows / 2 - 0.25 * f) for f in range(b)]


def cloud_table(kw):
    return api.make_cloud_calib(*[[k[n] for k in kw] for n in ("fx", "fy", "cx", "cy")])


def cloud_case(name, b, rows, cols, seed, colour, zero_frame=None, kw=None, frames=None):
    kw = kw or cloud_records(b, rows, cols)
    frames = depth_frames(b, rows, cols, seed, zeros=0.5) if frames is None else frames
    if zero_frame is not None:
        frames[zero_frame] = 0
    bgr = np.random.default_rng(seed + 1).integers(0, 256, frames.shape + (3,), dtype=np.uint8) if colour else None

    def frame(f, g):
        return words(np_cloud(frames[f], None if bgr is None else bgr[f], **kw[g]))

    return Case(name, b, cloud_table(kw), frame, [] if zero_frame is None else [zero_frame], frames=frames, bgr=bgr, kw=kw, rows=rows, cols=cols)


def cloud_want(case):
    """(records uint32 [total][4], offsets int32 [b + 1]) of the whole batch."""
    recs = [case.want(f) for f in range(case.b)]
    return np.concatenate(recs), np.concatenate([[0], np.cumsum([len(r) for r in recs])]).astype(np.int32)


# ---------------------------------------------------------------------------------------------------------------- stereo
def stereo_case(name, b, rows, cols, seed, iterations):
    rec = [dict(baseline=0.54 * (1 + 0.1 * f), focal=80.0 * (1 + 0.25 * f)) for f in range(b)]
    l, r, d = zip(*[synth.synth_stereo(rows, cols, seed + f, **rec[f]) for f in range(b)])

    def frame(f, g):
        return O().stereo_refine(d[f], l[f], r[f], iterations=iterations, **rec[g])

    return Case(name, b, api.make_stereo_calib([k["baseline"] for k in rec], [k["focal"] for k in rec]), frame,
                depth=np.stack(d), left=np.stack(l), right=np.stack(r), rec=rec, iterations=iterations, rows=rows, cols=cols)


# ---------------------------------------------------------------------------------------------------------------- stream order
STREAM_KINDS = ("project", "cloud", "reproject", "stereo")
STREAM_ROWS, STREAM_COLS, STREAM_B, STREAM_OUT = 24, 40, 3, (20, 36)


def rolled(case, name, by):
    """The case with its table rolled by `by` records: frame f carries record (f - by) % b of the original."""
    data = {k: v for k, v in case.__dict__.items() if k not in ("name", "b", "table", "frame", "empty", "_want")}
    return Case(name, case.b, np.roll(case.table, by), lambda f, g: case.frame(f, (g - by) % case.b), case.empty, **data)


def stream_case(kind, which):
    """Input set `which` (0 the real one, 1 the decoy) of the stream-order test of `kind`: its own seed, and the table rolled by `which`
    records, so that the real and the decoy table differ in every record."""
    r, c, b = STREAM_ROWS, STREAM_COLS, STREAM_B
    base = {"project": lambda: project_case("p", r, c, (400, 250, 350), 60 + which),
            "cloud": lambda: cloud_case("c", b, r, c, 90 + 3 * which, True),
            "reproject": lambda: reproject_case("r", b, r, c, STREAM_OUT[0], STREAM_OUT[1], 70 + which),
            "stereo": lambda: stereo_case("s", b, r, c, 80 + 5 * which, 4)}[kind]()
    return rolled(base, f"stream {kind} 24x40 {'decoy' if which else 'real'}", which)


# ---------------------------------------------------------------------------------------------------------------- the sets
_cases = {}


def cases():
    """Every input set test_gpu_calib.py compares against a restatement, built once."""
    if not _cases:
        kitti = ([np.linalg.inv(rot(0.0151, -0.0028)).astype(f32), rot(-0.009, 0.004, (0.02, -0.01, 0.0))],
                 np.array([[[959.791, 0, 696.0217], [0, 956.9251, 224.1806], [0, 0, 1]], [[721.5377, 0, 609.5593], [0, 721.5377, 172.854], [0, 0, 1]]], f32),
                 [dict(fx=959.791, fy=956.9251, cx=696.0217, cy=224.1806), dict(fx=721.5377, fy=721.5377, cx=609.5593, cy=172.854)])
        full = depth_frames(2, 352, 1216, 77, zeros=0.3)
        for c in (
            # sweep boundaries at points 100, 400, 437, 693 of three workgroups (inside a workgroup and inside a wave), one empty sweep
            project_case("project sweeps 16x24", 16, 24, (100, 0, 300, 37, 256, 1), 1),
            # 4 x 35 pixels: with PW == 4 the thread of pixels 32..35 has three of frame 0 and one of frame 1
            project_case("project straddle 5x7", 5, 7, (60, 60, 60, 60), 2),
            # 600 pixels a frame: waves of the resolve inside a frame and across pixels 600 and 1200 at every store width; a sweep boundary
            # inside a wave, one empty sweep (test_gpu_geo_instances.py)
            project_case("project 20x30", 20, 30, (300, 0, 200), 3),
            reproject_case("reproject 6x9 -> 5x7", 4, 6, 9, 5, 7, 25),
            reproject_case("reproject 40x50 -> 33x41", 4, 40, 50, 33, 41, 8),          # two scatter workgroups per frame
            reproject_case("reproject 352x1216 pair", 2, 352, 1216, 352, 1216, 0, records=kitti, frames=full),
            cloud_case("cloud 96x96 colour", 4, 96, 96, 5, True, zero_frame=2),        # two 8192-pixel chunks per frame
            cloud_case("cloud 96x96", 4, 96, 96, 6, False, zero_frame=2),
            cloud_case("cloud 352x1216 pair", 2, 352, 1216, 7, True, kw=kitti[2], frames=full.copy()),
            stereo_case("stereo 6x300 iterations 4", 3, 6, 300, 8, 4),                 # a thread walks more than one column
            stereo_case("stereo 6x300 iterations 0", 3, 6, 300, 8, 0),
            stereo_case("stereo 3x49160", 2, 3, 49160, 9, 4),                          # the row does not fit LDS: k_stereo_refine<false>
            # the sets of the bad-record test (frame 1 of 3 is made bad there) and of the winner-plane test.  Sweeps of 256, 300 and 100
            # points: workgroup 1 (points 256..511) starts in frame 1 and all four of its waves lie in it (the record of the workgroup's
            # first frame, on the scalar path); wave 0 of workgroup 2 holds the boundary at point 556 (the per-lane path)
            project_case("project 3 sweeps 12x20", 12, 20, (256, 300, 100), 10),
            reproject_case("reproject 12x20 -> 10x18 batch 3", 3, 12, 20, 10, 18, 11),
            cloud_case("cloud 12x20 batch 3", 3, 12, 20, 12, True),
            stereo_case("stereo 8x40 batch 3", 3, 8, 40, 13, 4),
        ):
            _cases[c.name] = c
        for kind in STREAM_KINDS:
            for which in (0, 1):
                c = stream_case(kind, which)
                _cases[c.name] = c
    return _cases
