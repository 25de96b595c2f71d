"""The point-cloud stage without a GPU: the facts of tests/cloud_fixture.py pinned on the numpy
reference tests/cloud_ref.py alone, cloud_ref's attributes against the reference's three loops
written out, the export against the reference's own file, and the bookkeeping of
tsbb15_amd.tables.get3DPointsColorsAndNormals with stubs in place of the two kernels.

Fixture facts, measured with cloud_ref:
                  nearest pair to the boundary   smallest gap / r^2   rows with k < 3
  Dino, r = 0.1   5.7e-7                         2.7e-3               3
  Dino, r = 0.2   8.7e-6                         3.4e-3               0
  sphere, r=0.25  1.2e-5                         5.7e-2               0
The smallest |cos| between a PCA normal and the golden view normal is 2.2e-3 (r = 0.1) and
1.4e-3 (r = 0.2); on the sphere the smallest |cos| to the radial direction is 0.9959.
"""
import ctypes
import io

import numpy as np
import pytest

import cloud_fixture as cf
import cloud_ref as cr
from tsbb15_amd import _ffi, cloud
from tsbb15_amd import tables as gt

FACTS = {"dino0.1": (5.6e-7, 5.8e-7, 2.6e-3, 3), "dino0.2": (8.6e-6, 8.8e-6, 3.4e-3, 0),
         "sphere": (1.2e-5, 1.3e-5, 5.7e-2, 0)}


@pytest.mark.parametrize("name", sorted(FACTS))
def test_fixture_facts(name):
    pts, radius, orient, ref = cf.reference(name)
    margin, gap, bad = cf.check_cloud(pts, radius, ref)
    print(f"{name}: margin {margin:.3e}, gap {gap:.3e}, rows not ok {bad}")
    lo, hi, g, nbad = FACTS[name]
    assert lo <= margin <= hi
    assert gap >= g
    assert bad == nbad
    normals, ok, count, evals = ref
    assert np.array_equal(np.isnan(normals).any(axis=1), ~ok)
    assert np.allclose(np.linalg.norm(normals[ok], axis=1), 1.0, atol=1e-14)
    assert np.all(count >= 1)                       # every point is its own neighbour
    assert np.all(evals[ok, 0] >= -1e-15 * radius ** 2)


def test_fixture_orientation_is_unambiguous():
    for name, least in (("dino0.1", 2.2e-3), ("dino0.2", 1.4e-3)):
        pts, radius, orient, (normals, ok, _, _) = cf.reference(name)
        cos = (normals[ok] * orient[ok]).sum(axis=1) / np.linalg.norm(orient[ok], axis=1)
        assert np.abs(cos).min() >= least
    pts, radius, _, (normals, ok, _, _) = cf.reference("sphere")
    radial = pts / np.linalg.norm(pts, axis=1, keepdims=True)
    assert ok.all() and np.abs((normals * radial).sum(axis=1)).min() >= 0.9958


def test_sign_rules():
    v = np.array([0.5, -0.5, 0.1])
    assert cr.orient_sign(v) == 1.0                         # the first of the largest
    assert cr.orient_sign(-v) == -1.0
    assert cr.orient_sign(v, np.array([0.0, 1.0, 0.0])) == -1.0
    assert cr.orient_sign(v, np.zeros(3)) == 1.0            # zero: the default rule
    assert cr.orient_sign(v, np.array([np.nan, 1.0, 0.0])) == 1.0


def _reference_loops(T):
    """tables.py:189-226 written out: three loops of np.concatenate, the mean unless the index
    holds one entry.  (The reference leaves `normal` unbound in that case; the single-entry
    point is not passed through here.)"""
    def colour_of(point):
        colour = np.zeros([0, 3], dtype='float')
        for o in point.observations_index:
            colour = np.concatenate((colour, [T.T_obs[o].color]), axis=0)
        if len(point.observations_index) != 1:
            colour = np.mean(colour, axis=0)
        return colour / 255.0

    def normal_of(point):
        vectors = np.zeros([0, 3])
        for o in point.observations_index:
            view = T.T_views[T.T_obs[o].view_index]
            position = -1.0 * (view.camera_pose.R.T @ view.camera_pose.t)
            vectors = np.concatenate((vectors, [position - point.point]), axis=0)
        if len(point.observations_index) != 1:
            normal = np.average(vectors, axis=0)
        return normal

    points, colours, normals = np.zeros([0, 3]), np.zeros([0, 3]), np.zeros([0, 3])
    for p in T.T_points:
        points = np.concatenate((points, [p.point]), axis=0)
        colours = np.concatenate((colours, [colour_of(p)]), axis=0)
        normals = np.concatenate((normals, [normal_of(p)]), axis=0)
    return points, colours, normals


def test_ref_attributes_equal_the_reference_loops():
    T = cf.table()
    pts, colors, normals = cr.table_attributes(T)
    single = len(T.T_points) - 1
    with pytest.raises((UnboundLocalError, ValueError)):   # the reference's own failure
        _reference_loops(T)
    T.T_points = T.T_points[:single]
    p0, c0, n0 = _reference_loops(T)
    assert np.array_equal(p0, pts[:single])
    assert np.allclose(c0, colors[:single], rtol=1e-14, atol=0)
    assert np.allclose(n0, normals[:single], rtol=1e-13, atol=1e-15)
    # every mean includes observation 0 once more than the point's own observations
    ep, eo = cr.table_entries(cf.table())
    assert np.all(eo[np.r_[0, np.flatnonzero(np.diff(ep)) + 1]] == 0)
    # the single-entry point: observation 0's colour / 255, the direction to its view
    o = T.T_obs[0]
    v = T.T_views[o.view_index].camera_pose
    assert np.allclose(colors[single], o.color / 255.0, rtol=1e-15)
    assert np.allclose(normals[single], -1.0 * (v.R.T @ v.t) - pts[single], rtol=1e-15)


def test_save_txt_reproduces_the_reference_file():
    d = cf.dino()
    out = io.BytesIO()
    cloud.save_txt(out, d["points"], d["colors"], d["normals"])
    lines = out.getvalue().split(b"\n")
    assert len(lines) == 689 and lines[-1] == b""
    assert d["txt_head"].count(b"\n") == 20
    assert b"\n".join(lines[:20]) + b"\n" == d["txt_head"]
    assert all(len(l.split(b" ")) == 10 for l in lines[:-1])


def test_save_txt_reflectance_and_shapes(tmp_path):
    d = cf.dino()
    path = tmp_path / "cloud.txt"
    cloud.save_txt(path, d["points"][:5], d["colors"][:5], d["normals"][:5], reflectance=0.25)
    back = np.loadtxt(path)
    assert back.shape == (5, 10) and np.all(back[:, 3] == 0.25)
    assert np.array_equal(back[:, :3], d["points"][:5])
    with pytest.raises(ValueError, match="colors"):
        cloud.save_txt(path, d["points"][:5], d["colors"][:4], d["normals"][:5])


def test_binding_matches_the_header():
    assert ctypes.sizeof(_ffi.CloudInfo) == 40
    assert _ffi.CloudInfo.pairs_tested.offset == 16 and _ffi.CloudInfo.rows_not_ok.offset == 32
    header = open(_ffi.HEADER_PATH).read()
    assert f"#define RS_CLOUD_TIMING_SLOTS {len(_ffi.CLOUD_STAGES)}\n" in header
    assert "#define RS_CLOUD_MAX_CELLS (1LL << 21)" in header and _ffi.CLOUD_MAX_CELLS == 1 << 21
    for name in ("rs_cloud_attributes", "rs_cloud_normals", "rs_cloud_timing"):
        assert name in _ffi._SIGS and hasattr(_ffi.lib(), name)


def test_value_errors_and_empty_cloud():
    pts = cf.sphere(10)
    for radius in (0.0, -1.0, np.inf, np.nan):
        with pytest.raises(ValueError, match="radius"):
            cloud.surface_normals(pts, radius)
    with pytest.raises(ValueError, match=r"\(n, 3\)"):
        cloud.surface_normals(pts[:, :2], 0.1)
    with pytest.raises(ValueError, match="orient"):
        cloud.surface_normals(pts, 0.1, orient=pts[:5])
    with pytest.raises(ValueError, match=r"\(nP, 3\)"):
        cloud.point_attributes(np.zeros((1, 3, 4)), np.zeros((4, 2)), [], [], [], np.zeros((0, 3)))
    with pytest.raises(ValueError, match="entry_obs"):
        cloud.point_attributes(np.zeros((1, 3, 4)), pts, [0, 1], [0], [0], np.zeros((1, 3)))
    with pytest.raises(ValueError, match="colour"):
        cloud.point_attributes(np.zeros((1, 3, 4)), pts, [0], [0], [0, 0], np.zeros((1, 3)))
    with pytest.raises(ValueError, match="integers"):
        cloud.point_attributes(np.zeros((1, 3, 4)), pts, [0.5], [0], [0], np.zeros((1, 3)))
    # n == 0: empty arrays, no context, no launch
    normals, ok, count, evals, info = cloud.surface_normals(np.zeros((0, 3)), 0.1)
    assert normals.shape == evals.shape == (0, 3) and ok.shape == count.shape == (0,)
    assert ok.dtype == bool and count.dtype == np.int32
    assert info == dict(cells_occupied=0, largest_cell=0, pairs_tested=0, neighbours_found=0,
                        rows_not_ok=0)


# ------------------------------------------------------------------------------------------
# bookkeeping of get3DPointsColorsAndNormals(T, ...) with both kernels stubbed
# ------------------------------------------------------------------------------------------
def _stubs(monkeypatch, ok):
    seen = {}

    def point_attributes(cams, pts, entry_point, entry_obs, obs_view, obs_color, ctx=None):
        seen["attr"] = dict(cams=np.array(cams), pts=np.array(pts), ep=np.array(entry_point),
                            eo=np.array(entry_obs), ov=np.array(obs_view),
                            col=np.array(obs_color))
        return cr.point_attributes(cams, pts, entry_point, entry_obs, obs_view, obs_color)

    def surface_normals(pts, radius, orient=None, ctx=None):
        seen["normals"] = dict(pts=np.array(pts), radius=radius, orient=np.array(orient))
        n = len(pts)
        pca = np.tile([0.0, 0.0, 1.0], (n, 1))
        pca[~ok] = np.nan
        return pca, ok.copy(), np.where(ok, 5, 1).astype(np.int32), np.zeros((n, 3)), {}

    monkeypatch.setattr(cloud, "point_attributes", point_attributes)
    monkeypatch.setattr(cloud, "surface_normals", surface_normals)
    return seen


def test_dropin_gathers_the_table(monkeypatch):
    T = cf.table()
    nP = len(T.T_points)
    seen = _stubs(monkeypatch, np.ones(nP, bool))
    before = [np.array(p.observations_index) for p in T.T_points]
    points, colors, normals = gt.get3DPointsColorsAndNormals(T)
    assert "normals" not in seen                           # no radius, no PCA call
    assert points.shape == colors.shape == normals.shape == (nP, 3)
    a = seen["attr"]
    ep, eo = cr.table_entries(T)
    assert np.array_equal(a["ep"], ep) and np.array_equal(a["eo"], eo)
    assert a["ep"].dtype == np.int32 and a["eo"].dtype == np.int32
    # the spurious 0 leads every point's entries; the last point has nothing else
    for j, p in enumerate(T.T_points):
        own = a["eo"][a["ep"] == j]
        assert own[0] == 0 and np.array_equal(own, p.observations_index)
    assert (a["ep"] == nP - 1).sum() == 1
    assert np.array_equal(a["ov"], [o.view_index for o in T.T_obs])
    assert np.array_equal(a["col"], [o.color for o in T.T_obs])
    assert np.array_equal(a["cams"][2][:, :3], T.T_views[2].camera_pose.R)
    assert np.array_equal(a["cams"][2][:, 3], T.T_views[2].camera_pose.t)
    p0, c0, n0 = cr.table_attributes(T)
    assert np.array_equal(points, p0) and np.array_equal(colors, c0)
    assert np.array_equal(normals, n0)
    after = [np.array(p.observations_index) for p in T.T_points]
    assert all(np.array_equal(x, y) for x, y in zip(before, after))   # the table is only read


def test_dropin_falls_back_to_the_view_normal(monkeypatch):
    T = cf.table()
    nP = len(T.T_points)
    ok = np.ones(nP, bool)
    ok[[1, 7, nP - 1]] = False
    seen = _stubs(monkeypatch, ok)
    points, colors, normals = gt.get3DPointsColorsAndNormals(T, radius=0.3)
    _, _, view = cr.table_attributes(T)
    s = seen["normals"]
    assert s["radius"] == 0.3 and np.array_equal(s["pts"], points)
    assert np.array_equal(s["orient"], view)               # oriented by the view normals
    assert np.array_equal(normals[ok], np.tile([0.0, 0.0, 1.0], (int(ok.sum()), 1)))
    unit = view / np.linalg.norm(view, axis=1, keepdims=True)
    assert np.array_equal(normals[~ok], unit[~ok])
    assert np.isfinite(normals).all()
    assert points.shape == colors.shape == normals.shape == (nP, 3)
