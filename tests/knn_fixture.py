"""Clouds for tests/test_knn_cpu.py and tests/test_gpu_knn.py.  Test infrastructure.

  * sphere(), dino()   the clouds of tests/cloud_fixture.py (1 500 and 688 points)
  * lattice()          the 5 x 5 x 5 integer lattice, index (x * 5 + y) * 5 + z: every d2 is exact
                       in fp64 and full of ties, so the tie rule alone decides the order
  * planted()          the sphere plus 30 points drawn uniformly in [-1.5, 1.5]^3 from
                       default_rng(11), keeping those at least 0.2 from the unit sphere

check_gaps asserts what a comparison of index lists needs: the smallest gap between consecutive
sorted d2 within the first k + 1 of every row is positive (no tie decides an index).  check_normals
asserts (lambda1 - lambda0) / d2_k >= cloud_fixture.GAP on ok rows, so the normal is well defined.
References are computed once, shared and read-only.
"""
from __future__ import annotations

import numpy as np

import cloud_fixture as cf
import knn_ref as kr

OUTLIER_STD_RATIO = 1.0      # with 2.0 the planted points inflate the deviation and 4 survive
N_PLANTED = 30

_cache = {}


def _frozen(*arrays):
    for a in arrays:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return arrays


def sphere():
    if "sphere" not in _cache:
        _cache["sphere"] = _frozen(cf.sphere())[0]
    return _cache["sphere"]


def dino():
    return cf.dino()["points"]


def lattice(side=5):
    if ("lattice", side) not in _cache:
        g = np.arange(float(side))
        L = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)
        _cache[("lattice", side)] = _frozen(np.ascontiguousarray(L))[0]
    return _cache[("lattice", side)]


def planted():
    """(cloud (1530, 3), is_planted (1530,) bool): the planted points come last."""
    if "planted" not in _cache:
        rng = np.random.default_rng(11)
        X = []
        while len(X) < N_PLANTED:
            x = rng.uniform(-1.5, 1.5, 3)
            if abs(np.linalg.norm(x) - 1.0) >= 0.2:
                X.append(x)
        A = np.vstack([sphere(), np.array(X)])
        mask = np.arange(len(A)) >= len(sphere())
        _cache["planted"] = _frozen(A, mask)
    return _cache["planted"]


def cloud(name):
    return {"sphere": sphere, "dino": dino, "lattice": lattice}[name]()


def lists(name, k):
    """knn_ref.knn(cloud(name), k), self query: (idx, d2, count), computed once."""
    key = ("lists", name, k)
    if key not in _cache:
        _cache[key] = _frozen(*kr.knn(cloud(name), k))
    return _cache[key]


def check_gaps(name, k):
    """The smallest gap between consecutive d2 within k + 1 over all rows; asserted positive."""
    _, d2, count = lists(name, k + 1)
    assert np.all(count == k + 1)
    gap = float(np.diff(d2, axis=1).min())
    assert gap > 0.0, gap
    return gap


def normals(name, k):
    """knn_ref.knn_normals(cloud(name), k) without orient, computed once, the gap asserted:
    (normals, ok, count, evals, d2k)."""
    key = ("normals", name, k)
    if key not in _cache:
        ref = kr.knn_normals(cloud(name), k, lists=lists(name, k))
        check_normals(ref)
        _cache[key] = _frozen(*ref)
    return _cache[key]


def check_normals(ref):
    """(lambda1 - lambda0) / d2_k on ok rows, asserted >= cloud_fixture.GAP."""
    _, ok, _, evals, d2k = ref
    gap = float(((evals[ok, 1] - evals[ok, 0]) / d2k[ok]).min()) if ok.any() else np.inf
    assert gap >= cf.GAP, gap
    return gap


def outliers(k):
    """knn_ref.remove_outliers(planted cloud, k, OUTLIER_STD_RATIO), computed once."""
    key = ("outliers", k)
    if key not in _cache:
        _cache[key] = _frozen(*kr.remove_outliers(planted()[0], k, OUTLIER_STD_RATIO))
    return _cache[key]
