"""The point-cloud stage on the GPU (tsbb15_amd.cloud, csrc/cloud.hip) against the numpy
restatement tests/cloud_ref.py on the clouds of tests/cloud_fixture.py.

Bars.  evals: 1e-12 r^2 -- the rounding of a k-term mean of terms bounded by r^2 is a few
eps r^2, which leaves about three orders of margin.  Normals of ok rows, sign-aligned: 1e-9 per
component -- Davis-Kahan with |dM| <= 1e-14 r^2 and a gap >= 1e-4 r^2 (asserted by the fixture)
gives 2e-10.  count / ok / the NaN pattern: equal, the fixture keeps every pair at least
1e-9 r away from the predicate's boundary.  Colours and view normals: 1e-13 of the row's
largest magnitude (sums of at most a dozen terms of that size).
"""
import io

import numpy as np
import pytest

import cloud_fixture as cf
import cloud_ref as cr
from tsbb15_amd import _ffi, cloud
from tsbb15_amd import tables as gt

pytestmark = pytest.mark.gpu

EVAL_BAR = 1e-12       # times r^2
NORMAL_BAR = 1e-9
ATTR_BAR = 1e-13


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64) if a.dtype == np.float64 else a


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _check(got, ref, radius, rows=None):
    """count, ok and the NaN pattern equal; evals to the bar; sign-aligned normals to the bar on
    `rows` (default: every ok row).  Prints every figure before it asserts."""
    normals, ok, count, evals, info = got
    rn, rok, rcount, revals = ref
    assert count.dtype == np.int32 and ok.dtype == bool
    assert np.array_equal(count, rcount)
    assert np.array_equal(ok, rok)
    assert np.array_equal(np.isnan(normals), np.isnan(rn))
    assert np.array_equal(np.isnan(evals), np.isnan(revals))
    assert np.array_equal(np.isnan(normals).any(axis=1), ~ok)
    assert info["neighbours_found"] == int(rcount.sum())
    assert info["rows_not_ok"] == int((~rok).sum())
    assert info["pairs_tested"] >= info["neighbours_found"]
    rows = rok if rows is None else rows & rok
    de = float(np.abs(evals[rok] - revals[rok]).max() / radius ** 2) if rok.any() else 0.0
    sign = np.sign((normals[rows] * rn[rows]).sum(axis=1))[:, None]
    dn = float(np.abs(sign * normals[rows] - rn[rows]).max()) if rows.any() else 0.0
    print(f"n={len(count)} r={radius}: d evals / r^2 {de:.2e}, d normals {dn:.2e}, info {info}")
    assert de <= EVAL_BAR
    assert dn <= NORMAL_BAR
    if rok.any():
        assert np.all(np.diff(evals[rok], axis=1) >= 0.0)
        assert np.abs(np.linalg.norm(normals[rok], axis=1) - 1.0).max() <= 1e-14
    return de, dn


def _against_ref(pts, radius, ctx, orient=None):
    """A cloud without the fixture's gap guarantee: normals are compared on the rows whose gap
    is at least the fixture's; the boundary margin is asserted."""
    assert cr.boundary_margin(pts, radius) >= cf.MARGIN
    ref = cr.surface_normals(pts, radius, orient)
    with np.errstate(invalid="ignore"):
        rows = (ref[3][:, 1] - ref[3][:, 0]) >= cf.GAP * radius ** 2
    got = cloud.surface_normals(pts, radius, orient=orient, ctx=ctx)
    _check(got, ref, radius, rows)
    return got, ref


# ------------------------------------------------------------------------------------------
# surface_normals against cloud_ref
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["dino0.1", "dino0.2", "sphere"])
def test_surface_normals_match_the_reference(ctx, name):
    pts, radius, _, ref = cf.reference(name)
    got = cloud.surface_normals(pts, radius, ctx=ctx)
    _check(got, ref, radius)                      # every ok row: the fixture asserts the gap
    normals, ok = got[0], got[1]
    # the default sign: the component of largest magnitude is positive
    big = np.abs(normals[ok]).argmax(axis=1)
    assert np.all(normals[ok][np.arange(int(ok.sum())), big] > 0.0)
    # and it is the reference's sign wherever the two largest magnitudes are not a near tie
    mag = np.sort(np.abs(ref[0][ok]), axis=1)
    clear = mag[:, 2] - mag[:, 1] > 1e-6
    assert np.abs(normals[ok][clear] - ref[0][ok][clear]).max() <= NORMAL_BAR
    info = got[4]
    assert 1 <= info["largest_cell"] <= len(pts)
    assert 1 <= info["cells_occupied"] <= len(pts)


@pytest.mark.parametrize("name", ["dino0.1", "dino0.2"])
def test_orient_decides_the_sign(ctx, name):
    pts, radius, orient, ref = cf.reference(name)
    normals, ok, count, evals, _ = cloud.surface_normals(pts, radius, orient=orient, ctx=ctx)
    dots = (normals[ok] * orient[ok]).sum(axis=1)
    print(f"{name}: smallest dot(normal, orient) {dots.min():.3e}")
    assert np.all(dots > 0.0)
    plain = cloud.surface_normals(pts, radius, ctx=ctx)
    assert _same_bits(np.abs(normals), np.abs(plain[0]))      # only signs differ
    assert _same_bits(evals, plain[3]) and np.array_equal(count, plain[2])
    # a zero or non-finite orient row falls back to the default rule
    o2 = np.array(orient)
    o2[0], o2[1] = 0.0, (np.nan, 1.0, 0.0)
    n2 = cloud.surface_normals(pts, radius, orient=o2, ctx=ctx)[0]
    assert _same_bits(n2[:2], plain[0][:2]) and _same_bits(n2[2:], normals[2:])


def test_sphere_normals_are_radial(ctx):
    pts, radius, _, _ = cf.reference("sphere")
    normals, ok, _, _, _ = cloud.surface_normals(pts, radius, ctx=ctx)
    radial = pts / np.linalg.norm(pts, axis=1, keepdims=True)
    cos = np.abs((normals * radial).sum(axis=1))
    print(f"sphere: smallest |cos| to the radial direction {cos.min():.4f}")
    assert ok.all() and cos.min() >= 0.99


# ------------------------------------------------------------------------------------------
# reproducibility
# ------------------------------------------------------------------------------------------
def test_identical_calls_give_identical_bits(ctx):
    pts, radius, orient, _ = cf.reference("dino0.1")
    a = cloud.surface_normals(pts, radius, orient=orient, ctx=ctx)
    b = cloud.surface_normals(pts, radius, orient=orient, ctx=ctx)
    for x, y in zip(a[:4], b[:4]):
        assert _same_bits(x, y)
    assert a[4] == b[4]
    pts, radius, _, _ = cf.reference("sphere")
    a = cloud.surface_normals(pts, radius, ctx=ctx)
    b = cloud.surface_normals(pts, radius, ctx=ctx)
    for x, y in zip(a[:4], b[:4]):
        assert _same_bits(x, y)


def test_permuted_cloud(ctx):
    pts, radius, _, _ = cf.reference("sphere")
    perm = np.random.default_rng(1).permutation(len(pts))
    a = cloud.surface_normals(pts, radius, ctx=ctx)
    b = cloud.surface_normals(pts[perm], radius, ctx=ctx)
    assert np.array_equal(b[2], a[2][perm])
    de = np.abs(b[3] - a[3][perm]).max() / radius ** 2
    print(f"permuted: d evals / r^2 {de:.2e}")
    assert de <= EVAL_BAR


# ------------------------------------------------------------------------------------------
# edge shapes
# ------------------------------------------------------------------------------------------
def test_empty_one_and_two_points(ctx):
    normals, ok, count, evals, info = cloud.surface_normals(np.zeros((0, 3)), 0.1, ctx=ctx)
    assert normals.shape == (0, 3) and count.shape == (0,) and info["pairs_tested"] == 0
    for pts in (np.array([[1.0, -2.0, 3.0]]), np.array([[0.0, 0.0, 0.0], [0.05, 0.0, 0.0]]),
                np.array([[0.0, 0.0, 0.0], [5.0, 0.0, 0.0]])):
        normals, ok, count, evals, info = cloud.surface_normals(pts, 0.1, ctx=ctx)
        ref = cr.surface_normals(pts, 0.1)
        assert np.array_equal(count, ref[2]) and not ok.any()
        assert np.isnan(normals).all() and np.isnan(evals).all()
        assert info["rows_not_ok"] == len(pts)


def test_three_collinear_points(ctx):
    pts = np.array([[0.0, 0.0, 0.0], [0.03, 0.03, 0.0], [0.06, 0.06, 0.0]])
    r = 0.1
    normals, ok, count, evals, _ = cloud.surface_normals(pts, r, ctx=ctx)
    assert ok.all() and np.array_equal(count, [3, 3, 3])
    print(f"collinear: evals / r^2 {evals / r ** 2}")
    assert np.abs(evals[:, :2]).max() <= EVAL_BAR * r * r
    assert np.abs(evals[:, 2] - 2.0 * 0.03 ** 2 * 2.0 / 3.0).max() <= EVAL_BAR * r * r
    line = np.array([1.0, 1.0, 0.0]) / np.sqrt(2.0)
    assert np.abs(normals @ line).max() <= 1e-9             # normal to the line
    assert np.abs(np.linalg.norm(normals, axis=1) - 1.0).max() <= 1e-14


def test_one_wave_plus_one(ctx):
    _against_ref(cf.sphere(65, seed=8), 0.8, ctx)


def test_one_crowded_cell_with_duplicates(ctx):
    r = 0.5
    pts = np.random.default_rng(9).uniform(0.0, 0.9 * r, (300, 3))
    pts[0] = 0.0                                            # the minimum corner is a point
    pts[10] = pts[3]
    pts[200] = pts[3]
    got, ref = _against_ref(pts, r, ctx)
    assert got[4]["cells_occupied"] == 1 and got[4]["largest_cell"] == 300
    assert got[4]["pairs_tested"] == 300 * 300
    assert _same_bits(got[3][3], got[3][10]) and _same_bits(got[3][3], got[3][200])


def test_negative_coordinates(ctx):
    _against_ref(cf.sphere(400, seed=10) * 2.0 - np.array([3.0, 7.0, 0.5]), 0.5, ctx)


def test_radius_below_every_distance(ctx):
    pts = cf.sphere(200, seed=11)
    normals, ok, count, evals, info = cloud.surface_normals(pts, 1e-6, ctx=ctx)
    assert np.all(count == 1) and not ok.any() and np.isnan(normals).all()
    assert info["neighbours_found"] == 200 and info["rows_not_ok"] == 200
    assert info["cells_occupied"] == 200 and info["largest_cell"] == 1


def test_two_distant_copies(ctx):
    pts, radius, _, _ = cf.reference("sphere")
    far = pts + np.array([1e5 * radius, 0.0, 0.0])
    assert cr.boundary_margin(far, radius) >= cf.MARGIN
    a = cloud.surface_normals(pts, radius, ctx=ctx)
    b = cloud.surface_normals(far, radius, ctx=ctx)
    both = cloud.surface_normals(np.vstack([pts, far]), radius, ctx=ctx)
    n = len(pts)
    assert np.array_equal(both[2][:n], a[2]) and np.array_equal(both[2][n:], b[2])
    de = max(np.abs(both[3][:n] - a[3]).max(), np.abs(both[3][n:] - b[3]).max()) / radius ** 2
    print(f"two copies: d evals / r^2 {de:.2e}")
    assert de <= EVAL_BAR
    assert both[4]["neighbours_found"] == a[4]["neighbours_found"] + b[4]["neighbours_found"]


def test_too_wide_a_cloud_is_a_value_error(ctx):
    pts, radius, _, _ = cf.reference("sphere")
    wide = np.vstack([pts[:100], pts[:100] + np.array([0.0, 3e6 * radius, 0.0])])
    with pytest.raises(ValueError, match="2097152"):
        cloud.surface_normals(wide, radius, ctx=ctx)
    # the context is still good
    assert cloud.surface_normals(pts[:100], radius, ctx=ctx)[2].sum() >= 100


def test_non_finite_points_are_ignored(ctx):
    clean = cf.sphere(300, seed=12)
    r = 0.4
    pts = np.insert(clean, [5, 100], [[np.nan, 0.0, 0.0], [np.inf, 1.0, 1.0]], axis=0)
    bad = np.array([5, 101])
    keep = np.setdiff1d(np.arange(len(pts)), bad)
    assert np.array_equal(pts[keep], clean)
    a = cloud.surface_normals(clean, r, ctx=ctx)
    b = cloud.surface_normals(pts, r, ctx=ctx)
    assert np.all(b[2][bad] == 0) and not b[1][bad].any()
    assert np.isnan(b[0][bad]).all() and np.isnan(b[3][bad]).all()
    for x, y in zip(a[:4], b[:4]):
        assert _same_bits(x, y[keep])
    assert b[4]["rows_not_ok"] == a[4]["rows_not_ok"] + 2
    # nothing but non-finite points
    c = cloud.surface_normals(np.full((3, 3), np.nan), r, ctx=ctx)
    assert np.all(c[2] == 0) and np.isnan(c[0]).all() and c[4]["cells_occupied"] == 0


# ------------------------------------------------------------------------------------------
# point_attributes and the table drop-in
# ------------------------------------------------------------------------------------------
def _rel(got, ref):
    return float((np.abs(got - ref).max(axis=1) / np.abs(ref).max(axis=1)).max())


def test_point_attributes_match_the_reference(ctx):
    T = cf.table()
    pts, rc, rn = cr.table_attributes(T)
    ep, eo = cr.table_entries(T)
    cams = np.array([v.camera_pose.GetCameraMatrix() for v in T.T_views])
    ov = np.array([o.view_index for o in T.T_obs])
    col = np.array([o.color for o in T.T_obs])
    colors, normals = cloud.point_attributes(cams, pts, ep, eo, ov, col, ctx=ctx)
    print(f"attributes: colours {_rel(colors, rc):.2e}, view normals {_rel(normals, rn):.2e}")
    assert _rel(colors, rc) <= ATTR_BAR and _rel(normals, rn) <= ATTR_BAR
    # a point without an entry gets NaN; the others do not change
    c2, n2 = cloud.point_attributes(cams, pts, ep[ep != 4], eo[ep != 4], ov, col, ctx=ctx)
    assert np.isnan(c2[4]).all() and np.isnan(n2[4]).all()
    rest = np.arange(len(pts)) != 4
    assert _same_bits(c2[rest], colors[rest]) and _same_bits(n2[rest], normals[rest])
    with pytest.raises(ValueError, match="entry_obs"):
        cloud.point_attributes(cams, pts, ep, eo + len(ov), ov, col, ctx=ctx)
    with pytest.raises(ValueError, match="non-decreasing"):
        cloud.point_attributes(cams, pts, ep[::-1], eo, ov, col, ctx=ctx)


def test_table_dropin(ctx):
    T = cf.table()
    rp, rc, rn = cr.table_attributes(T)
    points, colors, normals = gt.get3DPointsColorsAndNormals(T, ctx=ctx)
    assert np.array_equal(points, rp)
    assert _rel(colors, rc) <= ATTR_BAR and _rel(normals, rn) <= ATTR_BAR
    # the single-entry point: observation 0's colour / 255 and the direction to its camera
    o = T.T_obs[0]
    v = T.T_views[o.view_index].camera_pose
    assert np.abs(colors[-1] - o.color / 255.0).max() <= ATTR_BAR
    assert _rel(normals[-1:], (-1.0 * (v.R.T @ v.t) - rp[-1])[None]) <= ATTR_BAR


def test_table_dropin_with_radius(ctx, tmp_path):
    T = cf.table()
    radius = 0.08
    rp, rc, rn = cr.table_attributes(T)
    assert cr.boundary_margin(rp, radius) >= cf.MARGIN
    ref_n, ok, _, ref_e = cr.surface_normals(rp, radius, orient=rn)
    assert ok.sum() >= 10 and (~ok).sum() >= 5              # both kinds of row
    assert ((ref_e[ok, 1] - ref_e[ok, 0]) >= cf.GAP * radius ** 2).all()
    points, colors, normals = gt.get3DPointsColorsAndNormals(T, radius=radius, ctx=ctx)
    assert np.abs(normals[ok] - ref_n[ok]).max() <= NORMAL_BAR
    assert np.all((normals[ok] * rn[ok]).sum(axis=1) > 0.0)
    unit = rn / np.linalg.norm(rn, axis=1, keepdims=True)
    assert np.abs(normals[~ok] - unit[~ok]).max() <= 2.0 * ATTR_BAR
    assert np.abs(np.linalg.norm(normals, axis=1) - 1.0).max() <= 1e-14
    # the export parses back to the same arrays
    path = tmp_path / "cloud.txt"
    cloud.save_txt(path, points, colors, normals)
    back = np.loadtxt(path)
    assert back.shape == (len(points), 10) and np.all(back[:, 3] == 1.0)
    assert np.array_equal(back[:, :3], points) and np.array_equal(back[:, 4:7], colors)
    assert np.array_equal(back[:, 7:], normals)
    out = io.BytesIO()
    cloud.save_txt(out, points, colors, normals)
    assert out.getvalue() == open(path, "rb").read()


# ------------------------------------------------------------------------------------------
# rs_cloud_timing
# ------------------------------------------------------------------------------------------
def _timed(ms, names):
    return all(np.isfinite(ms[k]) and 0.0 < ms[k] < 1e3 for k in names)


def test_timing_slots():
    """Slots start at -1; rs_cloud_normals fills grid / scan / sort / normals and
    rs_cloud_attributes fills attributes alone; a call after disabling changes nothing; timed
    and untimed results are bit-equal.  A context of its own, so that no earlier call has timed."""
    pts, radius, orient, _ = cf.reference("dino0.1")
    T = cf.table()
    tp, _, _ = cr.table_attributes(T)
    ep, eo = cr.table_entries(T)
    cams = np.array([v.camera_pose.GetCameraMatrix() for v in T.T_views])
    ov = np.array([o.view_index for o in T.T_obs])
    col = np.array([o.color for o in T.T_obs])
    normals_of = lambda c: cloud.surface_normals(pts, radius, orient=orient, ctx=c)
    attrs_of = lambda c: cloud.point_attributes(cams, tp, ep, eo, ov, col, ctx=c)
    stages = _ffi.CLOUD_STAGES[:4]
    own = _ffi.Context()
    try:
        plain_n, plain_a = normals_of(own), attrs_of(own)
        assert cloud.timing(1, ctx=own) == dict.fromkeys(_ffi.CLOUD_STAGES, -1.0)
        timed_n = normals_of(own)
        ms = cloud.timing(1, ctx=own)
        print("after surface_normals:", ms)
        assert _timed(ms, stages) and ms["attributes"] == -1.0
        timed_a = attrs_of(own)
        ms2 = cloud.timing(0, ctx=own)
        print("after point_attributes:", ms2)
        assert _timed(ms2, ["attributes"])
        assert all(ms2[k] == ms[k] for k in stages)
        again_n, again_a = normals_of(own), attrs_of(own)
        assert cloud.timing(0, ctx=own) == ms2
        for a, b, c in zip(plain_n[:4], timed_n[:4], again_n[:4]):
            assert _same_bits(a, b) and _same_bits(a, c)
        assert plain_n[4] == timed_n[4] == again_n[4]
        for a, b, c in zip(plain_a, timed_a, again_a):
            assert _same_bits(a, b) and _same_bits(a, c)
    finally:
        own.close()
