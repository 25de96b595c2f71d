"""The restatement tests/knn_ref.py and the clouds of tests/knn_fixture.py, without a GPU: the
brute force against hand answers and scipy's kd-tree, the grid walk against the brute force, the
plane fit against the radial direction, and the margins every GPU comparison relies on."""
import numpy as np
import pytest
from scipy.spatial import cKDTree

import knn_fixture as kf
import knn_ref as kr


def test_lattice_hand_answers():
    L = kf.lattice()
    idx, d2, count = kr.knn(L, 7)
    assert idx.dtype == np.int32 and count.dtype == np.int32
    assert idx[62].tolist() == [62, 37, 57, 61, 63, 67, 87]      # the centre (2, 2, 2)
    assert d2[62].tolist() == [0.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0]
    assert idx[0].tolist() == [0, 1, 5, 25, 6, 26, 30]           # the corner (0, 0, 0)
    assert d2[0].tolist() == [0.0, 1.0, 1.0, 1.0, 2.0, 2.0, 2.0]
    assert np.all(count == 7)
    # max_dist is inclusive: exactly the six neighbours at distance 1 and the point itself
    idx, d2, count = kr.knn(L, 27, max_dist=1.0)
    assert count[62] == 7 and count[0] == 4
    assert idx[62, 7:].tolist() == [-1] * 20 and np.all(np.isinf(d2[62, 7:]))


def test_sizes_and_non_finite():
    P = np.arange(12.0).reshape(4, 3)
    idx, d2, count = kr.knn(P, 6)
    assert np.all(count == 4) and np.all(idx[:, 4:] == -1) and np.all(np.isinf(d2[:, 4:]))
    Q = P.copy()
    Q[1, 0] = np.nan
    Q[2, 2] = np.inf
    idx, d2, count = kr.knn(Q, 3)
    assert count.tolist() == [2, 0, 0, 2]
    assert idx[0].tolist() == [0, 3, -1] and idx[3].tolist() == [3, 0, -1]
    idx, d2, count = kr.knn(np.zeros((0, 3)), 2, queries=P)
    assert np.all(count == 0) and np.all(idx == -1)


@pytest.mark.parametrize("name,k", [("sphere", 8), ("sphere", 16), ("sphere", 32),
                                    ("sphere", 15), ("dino", 15)])
def test_brute_force_matches_the_kd_tree(name, k):
    pts = kf.cloud(name)
    gap = kf.check_gaps(name, k)
    idx, d2, count = kf.lists(name, k)
    dd, ii = cKDTree(pts).query(pts, k)
    print(f"{name} k={k}: smallest gap between consecutive d2 {gap:.2e}")
    assert np.array_equal(ii, idx)
    assert np.abs(dd * dd - d2).max() <= 4 * np.finfo(float).eps * d2.max()


def test_fixture_gaps_are_what_was_measured():
    assert kf.check_gaps("sphere", 8) >= 3e-7
    assert kf.check_gaps("sphere", 16) >= 3e-8
    assert kf.check_gaps("sphere", 32) >= 3e-8


@pytest.mark.parametrize("G", [1, 6, 8, 11, 16])
@pytest.mark.parametrize("k", [8, 32])
def test_grid_walk_equals_brute_force(G, k):
    pts = kf.sphere()
    rng = np.random.default_rng(5)
    _, lo, hi = kr.default_cell(pts)
    cell = float((hi - lo).max()) / G
    inside = pts[:120]
    outside = lo + (hi - lo) * rng.uniform(-0.5, 1.5, (60, 3))
    on_cells = lo + cell * rng.integers(0, G + 1, (40, 3))        # on cell boundaries
    far = hi + 100.0 * (hi - lo) * np.array([[1.0, 0.0, 0.0], [1.0, 1.0, 1.0], [0.0, -2.0, 0.0]])
    Q = np.vstack([inside, outside, on_cells, far])
    ref = kr.knn(pts, k, queries=Q)
    got = kr.knn_grid(pts, k, queries=Q, cell=cell)
    for a, b in zip(got[:3], ref):
        assert np.array_equal(a, b)
    info = got[3]
    assert info["cells"] == int(np.prod(info["dims"])) and max(info["dims"]) in (G, G + 1)
    per_query = info["tested"] / len(Q)
    print(f"G={G} k={k}: tested per query {per_query:.0f}, largest cell {info['largest_cell']}")
    if G > 1:                                             # G = 1: two cells on the longest axis
        # k = 32 of 1 500 points lie within a quarter of the box of any query in or near it, so
        # with six or more cells an axis the walk stops long before it has seen half the cloud
        assert per_query < len(pts) / 2


def test_grid_walk_default_cell_tests_a_fraction():
    pts = kf.sphere()
    # the figures the design records for the first 300 points as queries: tests per query at the
    # default G = 11, to the nearest whole number, and 208 as the largest over G = 6, 8, 11, 16
    for k, per_query in ((8, 46), (16, 95), (32, 118)):
        idx, d2, count, info = kr.knn_grid(pts, k, queries=pts[:300])
        ref = kf.lists("sphere", k)
        assert np.array_equal(idx, ref[0][:300]) and np.array_equal(d2, ref[1][:300])
        assert max(info["dims"]) == 11 or max(info["dims"]) == 12     # G = 11
        assert info["tested"] / 300 < 375                             # a quarter of 1 500
        assert round(info["tested"] / 300) == per_query
    _, lo, hi = kr.default_cell(pts)
    for G in (6, 8, 16):
        for k in (8, 16, 32):
            cell = float((hi - lo).max()) / G
            idx, d2, count, info = kr.knn_grid(pts, k, queries=pts[:300], cell=cell)
            assert np.array_equal(idx, kf.lists("sphere", k)[0][:300])
            assert round(info["tested"] / 300) <= 208
    # with max_dist and with ties: the same lists as the brute force
    L = kf.lattice()
    for kw in ({}, {"max_dist": 1.0}, {"max_dist": np.sqrt(2.0)}, {"cell": 0.75}):
        got = kr.knn_grid(L, 27, **kw)
        ref = kr.knn(L, 27, max_dist=kw.get("max_dist", np.inf))
        for a, b in zip(got[:3], ref):
            assert np.array_equal(a, b)


@pytest.mark.parametrize("k,worst", [(8, 9.0), (16, 5.8), (32, 4.3)])
def test_normals_on_the_sphere(k, worst):
    pts = kf.sphere()
    normals, ok, count, evals, d2k = kf.normals("sphere", k)      # asserts the eigen-gap
    assert ok.all() and np.all(count == k)
    radial = pts / np.linalg.norm(pts, axis=1, keepdims=True)
    angle = np.degrees(np.arccos(np.clip(np.abs((normals * radial).sum(axis=1)), 0.0, 1.0)))
    print(f"k={k}: worst angle {angle.max():.2f} deg")
    assert angle.max() <= worst + 0.1
    # eigh against the definition: M v = lambda v, ascending, unit
    i = 17
    idx = kf.lists("sphere", k)[0][i]
    d = pts[idx] - pts[i]
    M = d.T @ d / k - np.outer(d.mean(axis=0), d.mean(axis=0))
    assert np.abs(M @ normals[i] - evals[i, 0] * normals[i]).max() <= 1e-15
    assert np.all(np.diff(evals, axis=1) >= 0.0)
    big = np.abs(normals).argmax(axis=1)
    assert np.all(normals[np.arange(len(pts)), big] > 0.0)


def test_normals_on_dino_are_well_defined():
    normals, ok, count, evals, d2k = kf.normals("dino", 15)
    assert ok.all()


def test_mean_dist_branches():
    # one point 40 times: most rows do not hold themselves and lose their last entry
    P = np.tile([[0.5, -1.0, 2.0]], (40, 1))
    md, count = kr.mean_dist(P, 8)
    assert np.all(md == 0.0) and np.all(count == 9)
    # two points: the other one is the only neighbour
    md, count = kr.mean_dist(np.array([[0.0, 0.0, 0.0], [3.0, 4.0, 0.0]]), 5)
    assert md.tolist() == [5.0, 5.0] and count.tolist() == [2, 2]
    md, _ = kr.mean_dist(np.array([[1.0, 2.0, 3.0]]), 1)
    assert np.isnan(md[0])
    L = kf.lattice()
    md, _ = kr.mean_dist(L, 6)
    assert md[62] == 1.0


@pytest.mark.parametrize("k,planted_margin,sphere_margin", [(8, 1.2, 0.93), (16, 1.15, 0.93)])
def test_outlier_fixture_margins(k, planted_margin, sphere_margin):
    A, is_planted = kf.planted()
    keep, md, threshold = kf.outliers(k)
    print(f"k={k}: nearest planted {md[is_planted].min() / threshold:.3f}, farthest sphere "
          f"{md[~is_planted].max() / threshold:.3f} of the threshold")
    assert np.array_equal(keep, ~is_planted)
    assert md[is_planted].min() >= planted_margin * threshold
    assert md[~is_planted].max() <= sphere_margin * threshold
    # the reason the fixture does not use 2.0
    keep2, _, _ = kr.remove_outliers(A, k, 2.0)
    assert keep2[~is_planted].all() and 0 < int(keep2[is_planted].sum()) < 30
