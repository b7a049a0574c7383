"""Numpy restatements of the two scatter calls under the NEAREST-wins rule (dcmt_project_points_nearest*, dcmt_reproject_depth_nearest*)
and the tiny inputs tests/test_nearest.py (no GPU) and tests/test_gpu_nearest.py share.

The arithmetic is not restated here: a point's landing pixel and value are what oracle/np_restatement.project_points -- the last-wins
restatement -- gives for that point ALONE (one point cannot collide), and a source pixel's uf, vf, t_2 are test_reproject._project's,
with np_reproject's acceptance test.  Only the collision rule is new: the smallest value per pixel in the total order of finite f32
with -0 below +0, chosen through the usual sign-flip map of f32 bits to unsigned order and np.minimum.at; the *_loop forms keep a
running minimum with float compares instead and must agree bit for bit."""
import math

import numpy as np

import test_reproject as TR
from oracle import np_restatement as NP

f32 = np.float32
u32 = np.uint32


_memo = {}          # inputs and per-point landings, computed once and shared (never modified)


# ---------------------------------------------------------------- the order
def ord_of(v):
    """f32 -> uint32 with the order of the floats, -0 below +0."""
    b = np.ascontiguousarray(v, dtype=f32).view(u32)
    return np.where(b >> u32(31), ~b, b ^ u32(0x80000000)).astype(u32)


def unord(o):
    o = np.asarray(o, dtype=u32)
    return np.where(o >> u32(31), o ^ u32(0x80000000), ~o).astype(u32).view(f32)


def key_of(v):
    """The device's key (csrc/dcmt_depth_key.h): ~ord, so that an integer max keeps the smallest float."""
    return ~ord_of(v)


def below(a, b):
    """a < b in the total order: the float compare, and -0 below +0."""
    return a < b or (a == b and math.copysign(1.0, a) < math.copysign(1.0, b))


def nearest_of(flat, values, n_px):
    """Per pixel the smallest of the values that land on it (flat: their pixels), 0 where none does."""
    best = np.full(n_px, 0xFFFFFFFF, u32)
    np.minimum.at(best, flat, ord_of(values))
    out = np.zeros(n_px, f32)
    hit = np.zeros(n_px, bool)
    hit[flat] = True
    out[hit] = unord(best[hit])
    return out


def nearest_of_loop(flat, values, n_px):
    out, seen = np.zeros(n_px, f32), np.zeros(n_px, bool)
    for p, v in zip(flat, values):
        if not seen[p] or below(float(v), float(out[p])):
            out[p] = v
        seen[p] = True
    return out


def last_of(flat, values, n_px):
    out = np.zeros(n_px, f32)
    for p, v in zip(flat, values):
        out[p] = v
    return out


# ---------------------------------------------------------------- projection
def project_landings(points, T, P, rows, cols):
    """(pixel, value) of every point that lands, in file order: the last-wins restatement on each point alone.  A point that lands
    stores p.z != 0 (p.z == 0 fails the bounds), so the one word of the plane that is not zero tells both."""
    pts = np.asarray(points, dtype=f32).reshape(-1, 4)
    memo = ("l", pts.tobytes(), np.asarray(T, f32).tobytes(), np.asarray(P, f32).tobytes(), rows, cols)
    if memo in _memo:
        return _memo[memo]
    flat, values = [], []
    for i in range(len(pts)):
        plane = NP.project_points(pts[i:i + 1], T, P, rows, cols).ravel()
        nz = np.flatnonzero(plane.view(u32))
        assert len(nz) <= 1
        if len(nz):
            flat.append(int(nz[0]))
            values.append(plane[nz[0]])
    _memo[memo] = (np.array(flat, np.int64), np.array(values, f32))
    return _memo[memo]


def record_ok(*arrays):
    return all(np.isfinite(np.asarray(a, np.float64)).all() for a in arrays)


def project_frame(points, T, P, rows, cols, rule=nearest_of):
    """One sweep.  A record with a non-finite entry (of T's rows 0..2 and P) gives the zero plane, as the table calls do."""
    if not record_ok(np.asarray(T, f32).reshape(4, 4)[:3], P):
        return np.zeros((rows, cols), f32)
    flat, values = project_landings(points, T, P, rows, cols)
    return rule(flat, values, rows * cols).reshape(rows, cols)


def project_batch(points, offsets, Ts, Ps, rows, cols, rule=nearest_of):
    """Ts, Ps: one matrix for all sweeps or a list with one per sweep."""
    b = len(offsets) - 1
    one = np.asarray(Ts).ndim == 2
    return np.stack([project_frame(points[offsets[f]:offsets[f + 1]], Ts if one else Ts[f], Ps if one else Ps[f], rows, cols, rule)
                     for f in range(b)])


def project_last(points, offsets, Ts, Ps, rows, cols):
    """The last-wins restatement itself, frame by frame (what the default rule gives)."""
    b = len(offsets) - 1
    one = np.asarray(Ts).ndim == 2
    out = []
    for f in range(b):
        T, P = (Ts, Ps) if one else (Ts[f], Ps[f])
        ok = record_ok(np.asarray(T, f32).reshape(4, 4)[:3], P)
        out.append(NP.project_points(points[offsets[f]:offsets[f + 1]], T, P, rows, cols) if ok else np.zeros((rows, cols), f32))
    return np.stack(out)


# ---------------------------------------------------------------- reprojection
def reproject_landings(d, orows, ocols, M, K, fx, fy, cx, cy):
    uf, vf, t2 = TR._project(d, M, K, fx, fy, cx, cy)
    with np.errstate(invalid="ignore"):
        land = (t2 > 0) & (uf >= 0) & (uf < f32(ocols)) & (vf >= 0) & (vf < f32(orows))      # np_reproject's test
    idx = np.flatnonzero(land.ravel())                                                   # row-major source order
    flat = vf.ravel()[idx].astype(np.int64) * ocols + uf.ravel()[idx].astype(np.int64)
    return flat, t2.ravel()[idx]


def reproject_frame(d, orows, ocols, rec, rule=nearest_of):
    """rec: dict(M, K, fx, fy, cx, cy).  A record the uniform call would refuse gives the zero plane."""
    M, K = np.asarray(rec["M"], f32).reshape(4, 4), np.asarray(rec["K"], f32).reshape(3, 3)
    if not record_ok(M[:3], K[:2], [rec["fx"], rec["fy"], rec["cx"], rec["cy"]]) or rec["fx"] == 0 or rec["fy"] == 0:
        return np.zeros((orows, ocols), f32)
    flat, values = reproject_landings(d, orows, ocols, M, K, rec["fx"], rec["fy"], rec["cx"], rec["cy"])
    return rule(flat, values, orows * ocols).reshape(orows, ocols)


def reproject_batch(frames, orows, ocols, recs, rule=nearest_of):
    """recs: one record for all frames or a list with one per frame."""
    return np.stack([reproject_frame(d, orows, ocols, recs if isinstance(recs, dict) else recs[f], rule) for f, d in enumerate(frames)])


def reproject_last(frames, orows, ocols, recs):
    out = []
    for f, d in enumerate(frames):
        r = recs if isinstance(recs, dict) else recs[f]
        ok = record_ok(np.asarray(r["M"], f32).reshape(4, 4)[:3], np.asarray(r["K"], f32).reshape(3, 3)[:2], [r["fx"], r["fy"], r["cx"], r["cy"]])
        out.append(TR.np_reproject(d, orows, ocols, **r) if ok else np.zeros((orows, ocols), f32))
    return np.stack(out)


# ---------------------------------------------------------------- the tiny inputs
PROJECT_SHAPES = ((5, 7), (6, 7), (8, 16))       # odd pixel count (scalar fix-up), 2-wide, 4-wide; x 3 frames
PROJECT_OFFSETS = np.array([0, 800, 800, 1500], np.int32)      # ~800 points; an EMPTY sweep; a sweep that starts inside the workgroup
                                                               # of points 768..1023, so the wave of 768..831 spans two frames


def project_record(rows, cols, k=0):
    """T with a translation (the velodyne behind and above the camera), P with a third-row translation of -0.5: a point with
    0 < t.z < 0.5 has p.z < 0.  k = 0, 1, 2: three different records."""
    T = TR.rot(0.01 + 0.004 * k, 0.02 - 0.003 * k, (0.05 + 0.01 * k, -0.08, -0.27 + 0.02 * k))
    f = 0.9 * cols + 0.2 * k
    P = np.array([[f, 0, cols / 2.0, 0.3 + 0.1 * k], [0, f, rows / 2.0 + 0.1 * k, 0.02], [0, 0, 1, -0.5]], f32)
    return T, P


def _points_for(g, T, P, uf, vf, tz):
    """Points whose f64 image under (T, P) is (uf, vf) at t.z = tz -- where the f32 arithmetic puts them is the restatement's business."""
    T, P = T.astype(np.float64), P.astype(np.float64)
    pz = tz + P[2, 3]
    tx = (uf * pz - P[0, 2] * tz - P[0, 3]) / P[0, 0]
    ty = (vf * pz - P[1, 2] * tz - P[1, 3]) / P[1, 1]
    t = np.stack([tx, ty, tz], axis=1) - T[:3, 3]
    xyz = t @ T[:3, :3]                                          # R^T (t - translation), row-wise
    return np.concatenate([xyz, g.random((len(xyz), 1))], axis=1).astype(f32)


def _sweep(g, n, T, P, rows, cols):
    """n points in random order: 80 % aimed into the image at depths 2..60 (4-6 and more per pixel), 7 % aimed beside it, 5 % behind
    the camera (t.z <= 0), 5 % with 0 < t.z < 0.5 aimed into the image (p.z < 0 lands in bounds), 3 % exact copies of earlier points
    (equal depth on the same pixel)."""
    n_in, n_out, n_behind, n_neg = int(0.80 * n), int(0.07 * n), int(0.05 * n), int(0.05 * n)
    inside = lambda m: (g.random(m) * cols, g.random(m) * rows)
    parts = [_points_for(g, T, P, *inside(n_in), 2.0 + 58.0 * g.random(n_in)),
             _points_for(g, T, P, g.random(n_out) * cols + g.choice([-1.5, 1.5], n_out) * cols, g.random(n_out) * rows, 2.0 + 58.0 * g.random(n_out)),
             _points_for(g, T, P, *inside(n_behind), -30.0 * g.random(n_behind)),
             _points_for(g, T, P, *inside(n_neg), 0.05 + 0.4 * g.random(n_neg))]
    pts = np.concatenate(parts)
    pts = np.concatenate([pts, pts[g.integers(0, len(pts), n - len(pts))]])
    return pts[g.permutation(n)]


def project_inputs(rows, cols, seed=0):
    """{points [1500][4], offsets, records [(T, P)] * 3}: sweep f is aimed with record f (the uniform tests use record 0 for all, so
    the other sweeps land a little differently -- any finite input is a valid one)."""
    key = ("p", rows, cols, seed)
    if key not in _memo:
        g = np.random.default_rng(7000 + 100 * rows + cols + seed)
        recs = [project_record(rows, cols, k) for k in range(3)]
        o = PROJECT_OFFSETS
        pts = np.concatenate([_sweep(g, int(o[f + 1] - o[f]), *recs[f], rows, cols) for f in range(3)])
        assert pts.shape == (1500, 4) and pts.dtype == f32 and np.isfinite(pts).all()
        pts.setflags(write=False)
        _memo[key] = dict(points=pts, offsets=o, records=recs)
    return _memo[key]


REPROJECT_SHAPES = (((9, 13), (5, 7)), ((16, 24), (8, 16)))
REPROJECT_MATS = {"identity": TR.EYE, "small": TR.rot(0.02, -0.015), "shift": TR.rot(0.01, 0.02, (0.3, -0.2, 1.5)),
                  "behind": TR.rot(0.1, math.radians(65.0))}


def reproject_record(src, dst, mat="identity", k=0):
    """Intrinsics at the scale of the source, K at the scale of the destination: some three source pixels fall into one destination pixel."""
    (r, c), (orows, ocols) = src, dst
    fx, fy = 0.9 * c + 0.3 * k, 0.9 * c
    K = np.array([[fx * ocols / c, 0, ocols / 2.0], [0, fy * orows / r, orows / 2.0 + 0.05 * k], [0, 0, 1]], f32)
    return dict(M=REPROJECT_MATS[mat] if isinstance(mat, str) else mat, K=K, fx=fx, fy=fy, cx=c / 2.0 - 0.25, cy=r / 2.0 + 0.25 * k)


def reproject_inputs(src, seed=0):
    """[3][rows][cols]: depths that GROW in row-major order (with noise), so that of the source pixels that share a destination pixel
    the nearer come earlier and last-wins keeps a farther one; zeros, negatives and -0.0 among them; frame 1 all zero."""
    key = ("r", src, seed)
    if key not in _memo:
        r, c = src
        g = np.random.default_rng(9000 + 100 * r + c + seed)
        ramp = np.arange(r * c, dtype=np.float64).reshape(r, c) / (r * c)
        x = (2.0 + 40.0 * ramp[None] + 6.0 * g.random((3, r, c))).astype(f32)
        x[g.random(x.shape) < 0.06] = 0.0
        x[g.random(x.shape) < 0.04] = -0.0
        neg = g.random(x.shape) < 0.05
        x[neg] = -x[neg]
        x[1] = 0
        x.setflags(write=False)
        _memo[key] = x
    return _memo[key]


def compare_rules(near, last):
    """(occupied pixels, pixels where the rules differ), after asserting what must hold between them: the same occupancy (a stored
    value is never +0: p.z == 0 is rejected, t_2 > 0) and nearest <= last everywhere."""
    nb, lb = near.view(u32), last.view(u32)
    assert np.array_equal(nb != 0, lb != 0), "occupancy differs between the two rules"
    assert (ord_of(near) <= ord_of(last)).all(), "a nearest value above the last-wins value"
    return int((lb != 0).sum()), int((nb != lb).sum())
