"""Clouds and a table for tests/test_cloud_cpu.py and tests/test_gpu_cloud.py.  Test
infrastructure.

  * dino()    the reference's own saved cloud (tests/golden/cloud.npz): 688 points, colours and
              averaged view normals; used at radius 0.1 (3Dvisualization.py:96) and 0.2
  * sphere()  1500 unit vectors from default_rng(7), each scaled by 1 + 0.002 N(0, 1);
              radius 0.25
  * table()   a small synthetic table on the tests/wash_fixture.py scheme: every
              observations_index carries the reference's spurious leading 0, every observation a
              colour, and one extra point has a single entry (the spurious 0 alone)

check_cloud asserts what every comparison of a GPU result with cloud_ref needs of its input: no
pair within 1e-9 * r of the predicate's boundary (so count cannot depend on the last bit of the
distance) and lambda1 - lambda0 >= 1e-4 r^2 on every ok row (so the normal is well defined).
"""
from __future__ import annotations

import numpy as np

import cloud_ref as cr
import wash_fixture as wf
from conftest import golden

DINO_RADII = (0.1, 0.2)
SPHERE_N, SPHERE_RADIUS = 1500, 0.25
MARGIN = 1e-9        # relative distance of the nearest pair from the boundary
GAP = 1e-4           # (lambda1 - lambda0) / r^2 on ok rows

_cache = {}


def dino():
    """dict(points, colors, normals), each (688, 3), read-only."""
    if "dino" not in _cache:
        z = golden("cloud.npz")
        d = {k: np.array(z[k], dtype=np.float64) for k in ("points", "colors", "normals")}
        d["txt_head"] = z["txt_head"].tobytes()
        for k in ("points", "colors", "normals"):
            d[k].setflags(write=False)
        _cache["dino"] = d
    return _cache["dino"]


def sphere(n=SPHERE_N, seed=7, noise=0.002):
    """(n, 3): unit vectors scaled by 1 + noise N(0, 1)."""
    rng = np.random.default_rng(seed)
    v = rng.standard_normal((n, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    return v * (1.0 + noise * rng.standard_normal(n))[:, None]


def check_cloud(pts, radius, ref=None):
    """Assert the two fixture conditions; returns (margin, smallest gap / r^2, rows not ok)."""
    normals, ok, count, evals = ref if ref is not None else cr.surface_normals(pts, radius)
    margin = cr.boundary_margin(pts, radius)
    assert margin >= MARGIN, margin
    gap = float(((evals[ok, 1] - evals[ok, 0]) / radius ** 2).min()) if ok.any() else np.inf
    assert gap >= GAP, gap
    return margin, gap, int((~ok).sum())


def reference(name):
    """(pts, radius, orient, (normals, ok, count, evals) of cloud_ref without orient), computed
    once and read-only.  name: 'dino0.1', 'dino0.2', 'sphere'."""
    if name not in _cache:
        if name == "sphere":
            pts, radius, orient = sphere(), SPHERE_RADIUS, None
        else:
            pts, radius, orient = dino()["points"], float(name[4:]), dino()["normals"]
        ref = cr.surface_normals(pts, radius)
        check_cloud(pts, radius, ref)
        for a in ref:
            a.setflags(write=False)
        pts = np.array(pts)
        pts.setflags(write=False)
        _cache[name] = (pts, radius, orient, ref)
    return _cache[name]


def table(nC=5, nP=24, seed=2):
    """A MiniTables with colours: the table of wash_fixture.table(nC, nP, seed) (no
    displacement), a colour of three integers in 0..255 per observation, and one more point
    without any observation of its own, whose observations_index is the spurious [0]."""
    W = wf.table(nC, nP, seed, displaced=False)
    T = wf.mini_tables(W)
    rng = np.random.RandomState(4000 + seed)
    for o in T.T_obs:
        o.color = rng.randint(0, 256, 3).astype(np.float64)
    T.addPoint(np.array([0.1, -0.2, 0.3]))
    wf.check_table(T)
    assert len(T.T_points[len(T.T_points) - 1].observations_index) == 1
    return T
