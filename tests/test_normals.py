"""Surface normals and the flying-pixel filter without a GPU: the two restatements of tests/normals_restatement.py against each other,
the formula itself in f64 on exactly affine inverse depths, what the statement promises at its edges (ties, a clean step, a
one-pixel column, min_plane_dist = 0, the counts), the bounds claim of include/dcmt.h over the extreme inputs, the default measured on
the oracle's cascade, the launch plan (tests/plan_normals_test.cpp, built against the headers alone), the makers' refusals, the struct
layouts and exports, and the PCD round trip."""
import ctypes
import itertools

import numpy as np
import pytest

import bilateral_restatement as B
import normals_restatement as N
import occlusion_restatement as OR
from depth_completion_mt_amd import _lib as L
from depth_completion_mt_amd import api
from test_plan import _build_and_run

f32, f64, u32 = np.float32, np.float64, np.uint32
SHAPES = [(1, 1), (1, 2), (2, 1), (1, 65), (17, 1), (5, 3), (70, 131), (33, 64)]


def both(depth, what, **kw):
    """The two restatements agree bit for bit; returns the literal one's (normals, out, removed, none)."""
    lit, vec = N.literal(depth, **kw), N.vectorised(depth, **kw)
    for a, b in zip(lit[:2], vec[:2]):
        assert a.dtype == f32 and a.shape == b.shape and a.tobytes() == b.tobytes(), what
    assert lit[2:] == vec[2:], f"{what}: {lit[2:]} against {vec[2:]}"
    return lit


def check_counts(depth, res, what, **kw):
    """The counts add up: removed = the pixels whose bytes changed, all of them to +0.0; none = the valid pixels with a zero record;
    every other pixel keeps its four bytes."""
    normals, out, removed, none = res
    lo, hi = (int(np.array(kw.get(k, N.DEFAULTS[k]), f32).view(u32)) for k in ("valid_thresh", "max_depth"))
    zb = depth.view(u32)
    valid = (zb >= lo) & (zb <= hi)
    changed = out.view(u32) != zb
    assert removed == int(changed.sum()) and (out.view(u32)[changed] == 0).all() and valid[changed].all(), what
    blank = (normals.view(u32) == 0).all(-1)
    assert blank[~valid].all() and none == int((valid & blank).sum()), what
    assert not blank[changed].any(), what                          # only a pixel with a normal is removed
    ln = np.sqrt((normals[..., :3].astype(f64) ** 2).sum(-1))[~blank]
    assert np.abs(ln - 1.0).max(initial=0.0) < 1e-6, what            # unit normals


@pytest.mark.parametrize("rows,cols", SHAPES)
def test_restatements_agree(rows, cols):
    """Planes with 40 % holes and the specials, a dense smooth plane, the tie planes; default, zero and large min_plane_dist."""
    planes = [("holes", N.holey_plane(rows, cols, 7)), ("smooth", N.smooth_plane(rows, cols, 8))] + list(zip(("lin", "peak"), N.tie_planes(rows, cols)))
    for name, z in planes:
        for dmin in (0.4, 0.0, 30.0):
            for intr in ({}, N.KITTI):
                what = f"{name} {rows}x{cols} min_plane_dist {dmin} {intr}"
                check_counts(z, both(z, what, min_plane_dist=dmin, **intr), what)
    if rows * cols >= 60:
        z = N.holey_plane(rows, cols, 7)
        assert np.isnan(z).any() and np.isinf(z).any() and (z.view(u32) == 0x80000000).any() and (z < 0).any()
        assert min(rows, cols) == 1 or N.vectorised(z, min_plane_dist=30.0)[2] > 0


def test_restatements_agree_on_a_full_frame():
    """352 x 1216, the planes tests/test_gpu_normals.py runs on the device at that size."""
    for z, dmin in ((N.holey_plane(352, 1216, 3), 2.0), (N.smooth_plane(352, 1216, 4), 0.4)):
        check_counts(z, both(z, "352x1216", min_plane_dist=dmin, **N.KITTI), "352x1216")


def test_one_row_or_column_has_no_normal():
    """A gradient that was not observed is not taken for zero: a frame of one row or one column has no normal at all."""
    for shape in ((1, 65), (17, 1), (1, 1)):
        z = N.smooth_plane(*shape, 3)
        normals, out, removed, none = both(z, str(shape))
        assert not normals.any() and removed == 0 and none == z.size and out.tobytes() == z.tobytes()


PLANES = [("ground at 1.65 m", (0.0, 1.0, 0.0), 1.65), ("frontal wall at 30 m", (0.0, 0.0, 1.0), 30.0),
          ("oblique wall", (np.sin(np.deg2rad(50)), 0.0, np.cos(np.deg2rad(50))), 12.0)]


def plane_errors():
    """For each of PLANES under KITTI's intrinsics on 24 x 40 pixels below the horizon: (name, the f64 statement's largest errors in
    the normal and in the distance, the f32 restatement's largest angular error in degrees and distance error in metres)."""
    rows, cols, rows0 = 24, 40, 200
    out = []
    for name, m, d in PLANES:
        k = dict(N.KITTI, cy=N.KITTI["cy"] - rows0, cx=N.KITTI["cx"] - 500)            # the window's rows and columns in the full frame
        w = N.plane_inverse_depth(m, d, rows, cols, **k)
        assert (w > 0.01).all()
        n64, d64 = N.exact(w, **k)
        e_n, e_d = np.abs(n64 + np.asarray(m)).max(), np.abs(d64 - d).max()            # the normal points TOWARDS the camera: -m
        z = (1.0 / w).astype(f32)
        nrm = N.vectorised(z, min_plane_dist=0.0, **k)[0][1:-1, 1:-1].astype(f64)
        cosang = np.clip(-(nrm[..., :3] * np.asarray(m)).sum(-1), -1, 1)
        out.append((name, e_n, e_d, float(np.degrees(np.arccos(cosang)).max()), float(np.abs(nrm[..., 3] - d).max())))
    return out


def test_formula_in_f64():
    """On an exactly affine inverse depth the f64 evaluation of the statement returns the plane's unit normal (towards the camera) and
    its distance to 1e-9.  The f32 restatement's errors on the same planes are printed (DESIGN.md section 38 records them)."""
    for name, e_n, e_d, ang, dd in plane_errors():
        print(f"{name}: f64 normal error {e_n:.2e}, distance error {e_d:.2e}; f32 largest angular error {ang:.4f} deg, distance error {dd:.4f} m")
        assert e_n < 1e-9 and e_d < 1e-9, name


def test_ties_take_F():
    lin, peak = N.tie_planes(12, 20)
    ties = N.linear_ties(lin)
    assert ties.sum() > 40
    nl = both(lin, "lin", min_plane_dist=0.0, **N.KITTI)[0]
    step = f32(1.0 / 1024.0)
    for y, x in np.argwhere(ties)[:30]:
        a = f32(N.KITTI["fx"]) * step
        assert nl[y, x, 0] == -a * nl[y, x, 3]                              # gx = F = B = 1 / 1024
    npk = both(peak, "peak", min_plane_dist=0.0, **N.KITTI)[0]
    inner = npk[1:-1, 1:-1]
    hi = (np.add.outer(np.arange(1, 11), np.arange(1, 19)) % 2 == 0)       # w = 0.5: F = -0.25 = -B, so gx = gy = -0.25 and nx, ny > 0
    assert (inner[hi][:, 0] > 0).all() and (inner[hi][:, 1] > 0).all()
    assert (inner[~hi][:, 0] < 0).all() and (inner[~hi][:, 1] < 0).all()  # w = 0.25: F = +0.25


def step_scene(rows=40, cols=64, near=6.0, far=30.0):
    """A fronto-parallel box at `near` m in front of a fronto-parallel wall at `far` m, the step clean."""
    z = np.full((rows, cols), far, f32)
    z[10:30, 20:44] = near
    return z


def test_clean_step_removes_nothing():
    """Up to the nearer surface's own plane distance: a fronto-parallel surface at depth z has dist = z."""
    z = step_scene()
    for dmin in (0.4, 0.8, 1.6, 5.99):                       # (at 6.0 itself the rounding of len2 * dmin2 decides)
        normals, out, removed, none = both(z, f"step {dmin}", min_plane_dist=dmin, **N.KITTI)
        assert removed == 0 and none == 0 and out.tobytes() == z.tobytes()
    assert np.allclose(normals[..., 3], z, rtol=4e-7, atol=0) and (normals[..., 2] == -1).all()      # two divisions and a root, half an ulp each
    assert both(z, "step 6.5", min_plane_dist=6.5, **N.KITTI)[2] == 20 * 24        # beyond it the box goes, whole


def test_one_pixel_column_is_removed():
    """What the statement gives (dcmt.h says so): both row differences of a column one pixel wide cross the step."""
    z = np.full((40, 64), 30.0, f32)
    z[:, 31] = 6.0
    out, removed = both(z, "column", **N.KITTI)[1:3]
    assert removed == 40 and (out[:, 31] == 0).all() and np.array_equal(np.delete(out, 31, 1), np.delete(z, 31, 1))
    z[:, 32] = 6.0                                                          # two pixels wide: kept
    assert both(z, "two columns", **N.KITTI)[2] == 0


def test_blurred_step_loses_its_veil():
    """The 5x5 Gaussian of the step writes the ramp 28.5, 22.5, 13.5, 7.5 m between the wall and the box.  Along the straight parts of
    the edge a ramp pixel more than 2 m from both surfaces has both neighbours across the edge on the ramp as well: even its smaller
    difference of w is at least 1 / 22.5 - 1 / 28.5 = 0.0094, a plane closer than 1 / (721.5 * 0.0094) = 0.15 m: all of them go at the
    default.  Every pixel the blur did not touch stays, and a larger min_plane_dist removes a superset."""
    from oracle import oracle as O
    z = step_scene()
    blurred = O.gaussian5(z)
    out = both(blurred, "blurred step", **N.KITTI)[1]
    V, U = np.mgrid[0:40, 0:64]
    straight = ((V >= 13) & (V <= 26)) | ((U >= 23) & (U <= 40))            # three pixels and more from the box's corners
    deep = straight & (np.abs(blurred - 6.0) > 2) & (np.abs(blurred - 30.0) > 2)
    assert deep.sum() > 100 and (out[deep] == 0).all()
    untouched = blurred == z
    assert untouched.sum() > 1000 and (out[untouched] == z[untouched]).all()
    wider = both(blurred, "blurred step 0.8", min_plane_dist=0.8, **N.KITTI)[1]
    assert ((wider == 0) | (out != 0)).all() and (wider == 0).sum() > (out == 0).sum()


def test_zero_removes_nothing():
    for z in (N.holey_plane(70, 131, 7), N.smooth_plane(33, 64, 8)):
        out, removed = both(z, "zero", min_plane_dist=0.0)[1:3]
        assert removed == 0 and out.tobytes() == z.tobytes()


# ------------------------------------------------------------------------------------------------------------------- the bounds
EXEMPT = {"cc", "dmin2", "rem"}                    # the three products dcmt.h names: their underflow changes no bit


def test_no_overflow_and_no_subnormal_over_the_extremes():
    """dcmt.h's claim: under the enforced bounds every intermediate is finite, and with |cx|, |cy| zero or at least 2^-60 none but
    c * c, dmin * dmin and len2 * dmin2 is subnormal."""
    tiny = float(np.finfo(f32).tiny)
    seen = {}

    def watch(name, v):
        a = abs(float(v))
        assert np.isfinite(a), (name, v)
        assert name in EXEMPT or a == 0.0 or a >= tiny, (name, v)
        lo, hi = seen.get(name, (np.inf, 0.0))
        seen[name] = (min(lo, a) if a > 0 else lo, max(hi, a))

    zlo, zhi = f32(0.0625), f32(16384.0)
    vals = np.array([zlo, np.nextafter(zlo, f32(1)), zhi, np.nextafter(zhi, f32(0)), 1.0, 2.0, 4.0, 3.0, 1000.0], f32)
    g = np.random.Generator(np.random.PCG64(11))
    planes = [vals[g.integers(0, len(vals), (5, 6))] for _ in range(3)]
    chess = np.where(np.add.outer(np.arange(5), np.arange(6)) % 2 == 0, zlo, zhi).astype(f32)       # the largest differences of w
    cancel = np.array([[1.0, 2.0, 4.0]] * 3, f32)          # at (1, 1) under cx = 3: w = 0.5, gx = -0.25, dx = -2, so c1 = 0 and c = 0
    focal = (2.0 ** -10, -2.0 ** -10, 2.0 ** 20, -2.0 ** 20)
    centre = (0.0, 2.0 ** -60, -2.0 ** -60, 2.0 ** 20, -2.0 ** 20, 3.0)
    for z in planes + [chess, cancel]:
        for fx, cx in itertools.product(focal, centre):
            for dmin in (0.0, 2.0 ** -70, 0.8, 1024.0):
                N.literal(z, watch=watch, fx=fx, fy=-fx, cx=cx, cy=-cx, min_plane_dist=dmin, valid_thresh=0.0625, max_depth=16384.0)
    assert seen["w"] == (2.0 ** -14, 16.0) and seen["a"][1] <= 2.0 ** 24 and seen["c"][1] < 2.0 ** 27 and seen["len2"][1] < 2.0 ** 55
    assert seen["F"][0] >= 2.0 ** -37 and seen["len2"][0] >= 2.0 ** -94 and 2.0 ** -28 < seen["dist"][0] and seen["dist"][1] <= 2.0 ** 47
    n = N.literal(cancel, fx=2.0 ** 20, fy=1.0, cx=3.0, cy=0.0, min_plane_dist=0.0)[0]
    assert n[1, 1, 2] == 0 and n[1, 1, 0] == 1.0                                   # c cancelled exactly: the normal lies along x


# ------------------------------------------------------------------------------------------------------------------- the default
def completed_scene(boxes, blur):
    """lidar_scene completed by the oracle's cascade (blur "gaussian": the default; "bilateral_clone": the bilateral finish on the plane
    behind the median), the ray-cast truth, and the mask of the pixels whose truth is a box."""
    from oracle import oracle as O
    sparse = OR.lidar_scene(boxes=boxes)[0]
    if blur == "gaussian":
        dense = O.img_completion(sparse)
    else:
        dense = B.invert(B.restatement_f32(O.img_completion(sparse, O.default_params(blur="none", stop_after=9))))
    V, U = np.mgrid[0:OR.ROWS, 0:OR.COLS]
    rays = np.stack([(U - OR.CX) / OR.F, (V - OR.CY) / OR.F, np.ones(U.shape)], -1).reshape(-1, 3)
    truth = OR._cast(np.zeros(3), rays, boxes).reshape(OR.ROWS, OR.COLS)
    ground = np.isclose(truth * (V - OR.CY) / OR.F, OR.GROUND_Y)
    return np.ascontiguousarray(dense, f32), truth, ground


def default_table():
    """Rows of (scene, blur, min_plane_dist, veil pixels, removed among them, other valid pixels, removed among them, the smallest dist
    on the ground among the pixels within 0.25 m of the truth)."""
    rows = []
    intr = dict(fx=OR.F, fy=OR.F, cx=OR.CX, cy=OR.CY)
    for boxes in (True, False):
        for blur in ("gaussian", "bilateral_clone"):
            dense, truth, ground = completed_scene(boxes, blur)
            for dmin in (0.4, 0.8, 1.6):
                normals, out, removed, none = N.vectorised(dense, min_plane_dist=dmin, **intr)
                valid = (dense >= f32(0.1)) & (dense <= f32(100.0))
                veil = valid & (np.abs(dense.astype(f64) - truth) > 0.25)
                gone = (out == 0) & valid
                good_ground = valid & ~veil & ground & (normals[..., 3] > 0)
                rows.append(("boxes" if boxes else "no boxes", blur, dmin, int(veil.sum()), int((gone & veil).sum()), int((valid & ~veil).sum()),
                             int((gone & ~veil).sum()), float(normals[..., 3][good_ground].min())))
    return rows


def test_default_on_the_cascade():
    """The one assertion: without the boxes the default min_plane_dist removes no pixel of the ground or the wall whose completed
    depth is within 0.25 m of the truth.  The whole table is printed (DESIGN.md section 38 records it)."""
    table = default_table()
    for r in table:
        print("%-8s %-15s min_plane_dist %.1f: veil %6d removed %6d; others %6d removed %5d; smallest ground dist %.4f" % r)
    default = float(api.make_normals_params().min_plane_dist)
    for scene, blur, dmin, n_veil, gone_veil, n_other, gone_other, gmin in table:
        if scene == "no boxes" and abs(dmin - default) < 1e-6:
            assert gone_other == 0, (blur, gone_other)


# ------------------------------------------------------------------------------------------------------------------- the host side
def test_launch_plan_as_compiled(tmp_path):
    """tests/plan_normals_test.cpp against the headers alone: the routes and their launches, the grids, every refusal, the bounds."""
    _build_and_run(tmp_path, "plan_normals_test")


def test_layouts_defaults_and_exports():
    assert ctypes.sizeof(L.NormalsParams) == 12
    p = api.make_normals_params()
    assert (f32(p.min_plane_dist), f32(p.valid_thresh), f32(p.max_depth)) == (f32(0.4), f32(0.1), f32(100.0))
    for name in ("dcmt_default_normals_params", "dcmt_depth_normals_dev", "dcmt_depth_normals_calib_dev", "dcmt_depth_normals"):
        assert name in L.EXPORTS and hasattr(L.lib(), name)
    header = open(L.HEADER).read() if hasattr(L, "HEADER") else ""
    assert not header or "dcmt_depth_normals_calib_dev" in header


@pytest.mark.parametrize("kw", [dict(min_plane_dist=-0.1), dict(min_plane_dist=1024.5), dict(min_plane_dist=np.nan), dict(min_plane_dist=np.inf),
                                dict(valid_thresh=0.05), dict(valid_thresh=np.nan), dict(max_depth=20000.0), dict(max_depth=0.05),
                                dict(max_depth=np.inf), dict(valid_thresh=5.0, max_depth=4.0)])
def test_params_refused(kw):
    with pytest.raises(ValueError):
        api.make_normals_params(**kw)


def test_params_accepted_at_the_bounds():
    for kw in (dict(min_plane_dist=0.0), dict(min_plane_dist=1024.0), dict(valid_thresh=0.0625, max_depth=16384.0), dict(valid_thresh=7.0, max_depth=7.0)):
        api.make_normals_params(**kw)


@pytest.mark.parametrize("bad", [dict(fx=0.0), dict(fx=2.0 ** -11), dict(fy=-2.0 ** 21), dict(fy=np.nan), dict(cx=np.inf), dict(cx=2.0 ** 20 + 1),
                                 dict(cy=-2.0 ** 20 - 1), dict(cy=np.nan)])
def test_tables_and_intrinsics_refused(bad):
    good = dict(fx=[721.5, 700.0, 2.0 ** -10], fy=[721.5, -2.0 ** 20, 5.0], cx=[0.0, 2.0 ** 20, -3.0], cy=[176.0, -2.0 ** 20, 1e-300])
    assert len(api.make_normals_calib(**good)) == 3
    k = dict(good)
    (name, v), = bad.items()
    k[name] = [good[name][0], v, good[name][2]]
    with pytest.raises(ValueError):
        api.make_normals_calib(**k)
    with pytest.raises(ValueError):
        api._normals_intrinsics_or_raise(**dict(dict(fx=721.5, fy=721.5, cx=608.0, cy=176.0), **bad))


def test_pcd_round_trip(tmp_path):
    g = np.random.Generator(np.random.PCG64(5))
    pts = np.zeros(37, api.CLOUD_DTYPE)
    for k in ("x", "y", "z"):
        pts[k] = g.normal(size=37).astype(f32)
    for k in ("b", "g", "r", "a"):
        pts[k] = g.integers(0, 256, 37)
    nrm = g.normal(size=(37, 4)).astype(f32)
    plain, with_n = str(tmp_path / "plain.pcd"), str(tmp_path / "normals.pcd")
    api.write_pcd(plain, pts)
    assert np.array_equal(api.read_pcd(plain), pts)
    with pytest.raises(ValueError):
        api.read_pcd(plain, normals=True)
    api.write_pcd(with_n, pts, nrm)
    back, nb = api.read_pcd(with_n, normals=True)
    assert np.array_equal(back, pts) and nb.tobytes() == nrm[:, :3].tobytes()
    assert np.array_equal(api.read_pcd(with_n), pts)
    blob = open(with_n, "rb").read()
    assert b"FIELDS x y z rgb normal_x normal_y normal_z curvature\n" in blob and b"SIZE 4 4 4 4 4 4 4 4\n" in blob
    body = np.frombuffer(blob[blob.index(b"DATA binary\n") + 12:], f32).reshape(37, 8)
    assert not body[:, 7].any()                                              # curvature: written as 0
    api.write_pcd(with_n, pts, nrm[:, :3])                                   # [n][3] is taken as well
    assert api.read_pcd(with_n, normals=True)[1].tobytes() == nrm[:, :3].tobytes()
    with pytest.raises(ValueError):
        api.write_pcd(with_n, pts, nrm[:5])
