"""The surface from oriented points without a GPU: the numpy restatement tests/points_ref.py on
the cases of tests/points_fixture.py, through tests/surface_ref.py to a mesh, and the host part
of tsbb15_amd.surface.points_volume, points_field and from_points.

Bars.  Plane: the field of a flat, regularly sampled sheet is the height above it; with unit
weights summing to sw the error is a few roundings of terms of size |z| <= 0.25, bar 1e-15
(measured 8.3e-17).  Sphere: the mesh is closed, of Euler characteristic 2 and in one component,
and no vertex is further than a quarter voxel (0.025) from the unit sphere (measured 0.0130).
"""
import numpy as np
import pytest

import points_fixture as pf
import points_ref as pr
import surface_ref as sr
from tsbb15_amd import surface


def test_plane_is_the_height():
    c = pf.plane()
    tsdf, weight, (value, count, sat) = pf.volume("plane")
    z = sr.node_positions(c["origin"], c["voxel"], c["dims"]).reshape(-1, 3)[:, 2]
    err = float(np.abs(value - z).max())
    print(f"plane: defined {int(np.isfinite(value).sum())}, saturated {int(sat.sum())}, "
          f"max |f - z| {err:.2e}")
    assert np.isfinite(value).all() and len(value) == 729
    assert int(sat.sum()) == 355
    assert err <= 1e-15
    assert tsdf.dtype == np.float32 and weight.dtype == np.float32
    assert np.array_equal(weight.reshape(-1), count.astype(np.float32))
    # positive on the side the normals point to, clamped at trunc = radius
    assert np.all(np.sign(tsdf.reshape(-1)) == np.sign(z))
    assert float(np.abs(tsdf).max()) <= 1.0


def test_sphere_closes():
    c = pf.sphere()
    assert c["dims"] == (25, 25, 25)
    _, _, (value, count, sat) = pf.volume("sphere")
    v, f = pf.mesh("sphere")
    radial = float(np.abs(np.linalg.norm(v, axis=1) - 1.0).max())
    print(f"sphere: {len(v)} vertices, {len(f)} faces, Euler {sr.euler(v, f)}, radial error "
          f"{radial:.4f}, saturated {int(sat.sum())}")
    assert (len(v), len(f)) == (5732, 11460)
    assert int(sat.sum()) == 3285
    assert sr.is_closed(f)
    assert sr.euler(v, f) == 2
    assert pf.components(len(v), f) == 1
    assert radial < 0.025
    assert sr.signed_volume(v, f) > 0.0          # the faces look along the cloud's normals


def test_restatement_edges():
    L = pf.lattice()
    pts, nrm = L["points"], L["normals"]
    # a node on a point: d2 = 0, w = 1, dot = 0; alone within the radius the field is +0
    value, count, _, _ = pr.field(pts, nrm, pts[62:63], 0.5, 16)
    assert count[0] == 1 and value[0] == 0.0
    # every neighbour exactly on the rim: counted, weight 0, NaN
    value, count, _, _ = pr.field(pts, nrm, [[2.0, 2.0, 2.5]], 0.5, 16)
    assert count[0] == 2 and np.isnan(value[0])
    # the rim joins a list without moving the value
    inner = pr.field(pts, nrm, [[2.0, 2.0, 2.25]], 0.5, 16)
    rim = pr.field(pts, nrm, [[2.0, 2.0, 2.25]], 0.75, 16)
    assert (inner[1][0], rim[1][0]) == (1, 2) and inner[0][0] == 0.25 and rim[0][0] == 0.25
    # normals as given: a scaled normal scales f
    twice = pr.field(pts, 2.0 * nrm, [[2.0, 2.0, 2.25]], 0.5, 16)
    assert twice[0][0] == 0.5
    # a point with a non-finite normal is out
    bad = np.array(nrm)
    bad[62, 0] = np.nan
    value, count, _, _ = pr.field(pts, bad, pts[62:63], 0.5, 16)
    assert count[0] == 0 and np.isnan(value[0])
    # no point at all
    value, count, color, _ = pr.field(np.zeros((0, 3)), np.zeros((0, 3)), pts[:3], 0.5, 4,
                                      colors=np.zeros((0, 3)))
    assert np.all(count == 0) and np.isnan(value).all() and np.isnan(color).all()
    # one colour everywhere comes back wherever the field is defined
    col = np.tile([[0.25, 0.5, 0.75]], (len(pts), 1))
    value, count, color, _ = pr.field(pts, nrm, pts + 0.3, 1.0, 8, colors=col)
    assert np.abs(color[np.isfinite(value)] - col[0]).max() <= 1e-15


def test_oriented_cloud_drops_rows():
    rng = np.random.default_rng(5)
    pts, nrm = rng.normal(size=(12, 3)), rng.normal(size=(12, 3)) * 5.0
    col = rng.uniform(0, 1, (12, 3))
    pts[1, 2] = np.nan
    nrm[3] = 0.0
    nrm[4, 0] = np.inf
    nrm[7] = np.nan
    col[9, 1] = np.nan
    p, u, c, keep = surface.oriented_cloud(pts, nrm, col)
    assert keep.tolist() == [i not in (1, 3, 4, 7, 9) for i in range(12)]
    assert np.array_equal(p, pts[keep]) and np.array_equal(c, col[keep])
    assert np.abs(np.linalg.norm(u, axis=1) - 1.0).max() <= 1e-15
    assert np.all((u * nrm[keep]).sum(axis=1) > 0.0)
    p, u, c, keep = surface.oriented_cloud(pts, nrm)
    assert c is None and keep.sum() == 8
    p, u, c, keep = surface.oriented_cloud(pts, nrm, (np.nan_to_num(col) * 255).astype(np.uint8))
    assert c.max() <= 1.0 and keep.sum() == 8                # uint8 colours: 0..255 -> [0, 1]
    assert np.array_equal(p, pts[keep])
    d = pf.dino()
    length = np.linalg.norm(d["raw"]["normals"], axis=1)
    assert 4.0 < length.min() and length.max() < 7.0         # averaged view normals, not unit
    assert d["kept"] == 688
    with pytest.raises(ValueError, match="no finite point"):
        surface.from_points(np.full((4, 3), np.nan), np.ones((4, 3)), 0.1, 0.2)
    with pytest.raises(ValueError, match="no finite point"):
        surface.from_points(np.ones((4, 3)), np.zeros((4, 3)), 0.1, 0.2)


def test_wrapper_errors():
    c = pf.plane()
    pts, nrm = c["points"], c["normals"]
    ok = dict(origin=c["origin"], voxel=c["voxel"], dims=c["dims"], radius=c["radius"])

    def vol(points=pts, normals=nrm, **kw):
        a = dict(ok, **kw)
        return surface.points_volume(points, normals, a.pop("origin"), a.pop("voxel"),
                                     a.pop("dims"), a.pop("radius"), **a)

    for kw in ({"k": 0}, {"k": 65}, {"k": 2.5}, {"k": True}, {"radius": 0.0}, {"radius": -1.0},
               {"radius": np.nan}, {"radius": np.inf}, {"trunc": 0.0}, {"trunc": np.nan},
               {"trunc": np.inf}, {"cell": -1.0}, {"cell": np.nan}, {"cell": np.inf},
               {"voxel": 0.0}, {"voxel": np.nan}, {"origin": [0.0, np.inf, 0.0]},
               {"origin": [0.0, 0.0]}, {"dims": (9, 9)}, {"dims": (0, 9, 9)},
               {"dims": (2049, 1, 1)}, {"dims": (1024, 1024, 256)}, {"points": pts[:, :2]},
               {"points": pts.reshape(-1)}, {"normals": nrm[:5]}):
        with pytest.raises(ValueError):
            vol(**kw)
    with pytest.raises(ValueError, match="64"):
        vol(k=65)
    with pytest.raises(ValueError, match="radius"):
        vol(radius=0.0)
    Q = pts[:4] + 0.1
    for kw in ({"k": 0}, {"k": 65}, {"radius": 0.0}, {"radius": np.nan}, {"cell": -1.0},
               {"colors": nrm[:5]}, {"queries": Q[:, :2]}, {"queries": Q.reshape(-1)}):
        a = dict(queries=Q, radius=0.3)
        a.update(kw)
        with pytest.raises(ValueError):
            surface.points_field(pts, nrm, a.pop("queries"), a.pop("radius"), **a)
    with pytest.raises(ValueError):
        surface.points_field(pts[:, :2], nrm, Q, 0.3)
    with pytest.raises(ValueError):
        surface.from_points(pts, nrm, 0.0, 0.3)
    with pytest.raises(ValueError):
        surface.from_points(pts, nrm[:5], 0.1, 0.3)
    with pytest.raises(ValueError):
        surface.from_points(pts, nrm, 0.1, 0.3, colors=nrm[:5])
    assert surface.POINTS_STAGES == ("box", "grid", "scan", "scatter", "field")
