"""The point-cloud stage (HIP kernels of cloud.hip): what main.py does last (main.py:175-176) and
the export of 3Dvisualization.py.

  * ``point_attributes``  the arithmetic of Tables.getColorFor3DPoint / getNormalFor3DPoint
                          (tables.py:189-214) for every point at once: the mean colour / 255 and
                          the mean direction to the cameras that see the point
  * ``surface_normals``   the plane fit 3Dvisualization.py attempts and leaves commented out
                          (3Dvisualization.py:16-31, :96-113), by its mathematics: fixed-radius
                          neighbourhoods, the smallest eigenvector of the neighbourhood's
                          covariance, a sign
  * ``knn``               exact k nearest neighbours (cloud_knn.hip), what GetKNeighbours asks a
                          kd-tree for (3Dvisualization.py:33-69); ``knn_normals`` fits the plane
                          to them, ``knn_mean_dist`` and ``remove_outliers`` clean a cloud up
  * ``save_txt``          the ten-column file of 3Dvisualization.py:139-145 (host only)

The contract of the kernels stands in include/rsamd.h.  The table-level drop-in is
``tsbb15_amd.tables.get3DPointsColorsAndNormals``.
"""
from __future__ import annotations

import numpy as np

from . import _ffi

_d = _ffi.C.c_double
_i32 = _ffi.C.c_int32


def _ctx(ctx):
    return (ctx or _ffi.default_context()).handle


def _index(a, name):
    a = np.asarray(a)
    if a.size and not np.issubdtype(a.dtype, np.integer):
        raise ValueError(f'{name} must hold integers')
    return _ffi.i32c(a, name).reshape(-1)


def point_attributes(cams, pts, entry_point, entry_obs, obs_view, obs_color, ctx=None):
    """Colours and view normals of a cloud (rs_cloud_attributes).

    cams (nC, 3, 4) [R | t], pts (nP, 3); the flat entry list (entry_point[i], entry_obs[i])
    names the observations every point averages over, grouped by point (entry_point
    non-decreasing) and, within a point, in the order to be summed; obs_view (nObs) and
    obs_color (nObs, 3) describe the observations.  Returns (colors, normals), both (nP, 3):
    the mean of the listed colours divided by 255, and the mean of centre(view) - point with
    centre = -R^T t, not normalised, as the reference.  A point without an entry gets NaN.
    ValueError for bad shapes and indices out of range."""
    cams = _ffi.f64c(cams).reshape(-1, 3, 4)
    pts = _ffi.f64c(pts)
    if pts.ndim != 2 or pts.shape[1] != 3:
        raise ValueError('pts must be (nP, 3)')
    ep, eo = _index(entry_point, 'entry_point'), _index(entry_obs, 'entry_obs')
    ov = _index(obs_view, 'obs_view')
    col = _ffi.f64c(obs_color).reshape(-1, 3)
    if len(ep) != len(eo):
        raise ValueError('one entry_obs per entry_point')
    if len(col) != len(ov):
        raise ValueError('one colour per observation')
    colors, normals = np.empty_like(pts), np.empty_like(pts)
    if len(pts) == 0 and len(ep) == 0:
        return colors, normals
    _ffi.check(_ffi.lib().rs_cloud_attributes(
        _ctx(ctx), _ffi.ptr(cams, _d), len(cams), _ffi.ptr(pts, _d), len(pts),
        _ffi.ptr(ep, _i32), _ffi.ptr(eo, _i32), len(ep), _ffi.ptr(ov, _i32), _ffi.ptr(col, _d),
        len(ov), _ffi.ptr(colors, _d), _ffi.ptr(normals, _d)))
    return colors, normals


def surface_normals(pts, radius, orient=None, ctx=None):
    """Surface normals from fixed-radius neighbourhoods (rs_cloud_normals).

    The neighbourhood of point i is every j with |p_j - p_i|^2 <= radius^2 (i included);
    count[i] is its size; evals[i] are the ascending eigenvalues of the covariance of the
    neighbourhood about p_i's own mean, normals[i] the unit eigenvector of the smallest.
    ok[i] = count[i] >= 3; rows that are not ok hold NaN in normals and evals.  With ``orient``
    (n, 3) the sign of normal i is the one with dot(normal, orient[i]) >= 0 (where orient[i] is
    finite and non-zero); otherwise the component of largest magnitude is positive.  A
    non-finite point has count 0 and is nobody's neighbour.

    Returns (normals, ok, count, evals, info); info = dict(cells_occupied, largest_cell,
    pairs_tested, neighbours_found, rows_not_ok).  n == 0 returns empty arrays without a launch.
    ValueError: pts not (n, 3), orient of another shape, radius not finite or <= 0, or a cloud so
    wide that (p - min corner) / radius reaches 2^21 on an axis.  The cost grows with the points
    per cell: a radius that swallows the whole cloud makes the call quadratic."""
    pts = _ffi.f64c(pts)
    if pts.ndim != 2 or pts.shape[1] != 3:
        raise ValueError('pts must be (n, 3)')
    radius = float(radius)
    if not np.isfinite(radius) or not radius > 0.0:
        raise ValueError('radius must be finite and positive')
    n = len(pts)
    op = None
    if orient is not None:
        orient = _ffi.f64c(orient)
        if orient.shape != pts.shape:
            raise ValueError('orient must have the shape of pts')
        op = _ffi.ptr(orient, _d)
    normals, evals = np.empty((n, 3)), np.empty((n, 3))
    count = np.zeros(n, dtype=np.int32)
    info = _ffi.CloudInfo()
    if n > 0:
        _ffi.check(_ffi.lib().rs_cloud_normals(
            _ctx(ctx), _ffi.ptr(pts, _d), n, radius, op, _ffi.ptr(normals, _d),
            _ffi.ptr(count, _i32), _ffi.ptr(evals, _d), _ffi.C.byref(info)))
    return normals, count >= 3, count, evals, {
        "cells_occupied": info.cells_occupied, "largest_cell": info.largest_cell,
        "pairs_tested": info.pairs_tested, "neighbours_found": info.neighbours_found,
        "rows_not_ok": info.rows_not_ok}


def timing(enable, ctx=None):
    """Enable / disable HIP events between the stages of the next point-cloud calls
    (rs_cloud_timing); returns the last timed call's {stage: device ms}, -1 where none."""
    ctx = ctx or _ffi.default_context()
    ms = np.zeros(len(_ffi.CLOUD_STAGES))
    _ffi.check(_ffi.lib().rs_cloud_timing(ctx.handle, int(enable), _ffi.ptr(ms, _d)))
    return dict(zip(_ffi.CLOUD_STAGES, ms.tolist()))


def _knn_args(pts, k, kmax, cell):
    pts = _ffi.f64c(pts)
    if pts.ndim != 2 or pts.shape[1] != 3:
        raise ValueError('pts must be (n, 3)')
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)):
        raise ValueError('k must be an integer')
    if not 1 <= k <= kmax:
        raise ValueError(f'k must be in 1..{kmax} (RS_CLOUD_KNN_MAX_K = {_ffi.CLOUD_KNN_MAX_K})')
    if len(pts) > _ffi.CLOUD_MAX_POINTS:
        raise ValueError('more points than RS_CLOUD_MAX_POINTS = 2^28')
    cell = 0.0 if cell is None else float(cell)
    if not np.isfinite(cell) or cell < 0.0:
        raise ValueError('cell must be finite and >= 0 (None or 0: the default)')
    return pts, int(k), cell


def _knn_info(info):
    return {"cells": info.cells, "largest_cell": info.largest_cell, "tested": info.tested,
            "found": info.found, "rows_short": info.rows_short}


def knn(pts, k, queries=None, max_dist=np.inf, cell=None, ctx=None):
    """Exact k nearest neighbours (rs_cloud_knn): what ``cKDTree(pts).query(queries, k)`` returns,
    as squared distances.

    pts (n, 3); queries (m, 3), or None for the points themselves (a point is then its own
    first neighbour unless duplicates with lower indices come before it).  d2 of a pair is
    dx*dx + dy*dy + dz*dz of the fp64 differences, bit for bit numpy's; a row holds the k
    smallest pairs (d2, index) in ascending order, the lower index first where two d2 are
    bit-equal, over the finite points with d2 <= max_dist^2.  count is the number found; the
    slots past it hold idx -1 and d2 +inf.  A non-finite point is nobody's neighbour, a
    non-finite query has count 0.  The result depends neither on ``cell`` (None: the largest
    extent / round(cbrt(n))) nor on anything else about the grid.

    Returns (idx (m, k) int32, d2 (m, k), count (m,) int32, info); info = dict(cells,
    largest_cell, tested, found, rows_short).  ValueError: pts or queries not (., 3), k outside
    1..64, max_dist NaN or negative, cell negative or not finite, or a cell that needs more than
    2^24 cells."""
    pts, k, cell = _knn_args(pts, k, _ffi.CLOUD_KNN_MAX_K, cell)
    max_dist = float(max_dist)
    if not max_dist >= 0.0:
        raise ValueError('max_dist must be >= 0 (inf: none)')
    qp, m = None, len(pts)
    if queries is not None:
        queries = _ffi.f64c(queries)
        if queries.ndim != 2 or queries.shape[1] != 3:
            raise ValueError('queries must be (m, 3)')
        if len(queries) > _ffi.CLOUD_MAX_POINTS:
            raise ValueError('more queries than RS_CLOUD_MAX_POINTS = 2^28')
        qp, m = _ffi.ptr(queries, _d), len(queries)
    idx = np.full((m, k), -1, dtype=np.int32)
    d2 = np.full((m, k), np.inf)
    count = np.zeros(m, dtype=np.int32)
    info = _ffi.KnnInfo()
    _ffi.check(_ffi.lib().rs_cloud_knn(
        _ctx(ctx), _ffi.ptr(pts, _d), len(pts), qp, m, k, max_dist, cell, _ffi.ptr(idx, _i32),
        _ffi.ptr(d2, _d), _ffi.ptr(count, _i32), _ffi.C.byref(info)))
    return idx, d2, count, _knn_info(info)


def knn_normals(pts, k, orient=None, cell=None, ctx=None):
    """Surface normals from every point's own k nearest (rs_cloud_knn_normals): the plane fit of
    GetNormalOfPlaneFromPoints(points[NN_index]) (3Dvisualization.py:33-69), by its mathematics.
    The neighbourhood adapts to the density, which a fixed radius cannot.

    The list of point i is ``knn(pts, k)``'s row i (i itself included).  evals[i] are the
    ascending eigenvalues of the list's covariance about p_i's own mean, normals[i] the unit
    eigenvector of the smallest, signed as ``surface_normals`` signs it.  ok[i] = count[i] >= 3;
    the other rows hold NaN.  Two calls give the same bits.

    Returns (normals, ok, count, evals, info), the shape of ``surface_normals``; info as
    ``knn``'s."""
    pts, k, cell = _knn_args(pts, k, _ffi.CLOUD_KNN_MAX_K, cell)
    n = len(pts)
    op = None
    if orient is not None:
        orient = _ffi.f64c(orient)
        if orient.shape != pts.shape:
            raise ValueError('orient must have the shape of pts')
        op = _ffi.ptr(orient, _d)
    normals, evals = np.empty((n, 3)), np.empty((n, 3))
    count = np.zeros(n, dtype=np.int32)
    info = _ffi.KnnInfo()
    _ffi.check(_ffi.lib().rs_cloud_knn_normals(
        _ctx(ctx), _ffi.ptr(pts, _d), n, k, cell, op, _ffi.ptr(normals, _d), _ffi.ptr(evals, _d),
        _ffi.ptr(count, _i32), _ffi.C.byref(info)))
    return normals, count >= 3, count, evals, _knn_info(info)


def knn_mean_dist(pts, k, cell=None, ctx=None):
    """The mean distance from every point to its k nearest other points
    (rs_cloud_knn_mean_dist), 1 <= k <= 63: of the k + 1 nearest the point itself is dropped
    (the last entry where more than k duplicates with lower indices hide it), the square roots of
    the rest are summed in list order and divided by their number.  NaN for a non-finite point
    and where nothing remains.  Returns (mean_dist (n,), count (n,) int32, info)."""
    pts, k, cell = _knn_args(pts, k, _ffi.CLOUD_KNN_MAX_K - 1, cell)
    n = len(pts)
    mean = np.full(n, np.nan)
    count = np.zeros(n, dtype=np.int32)
    info = _ffi.KnnInfo()
    _ffi.check(_ffi.lib().rs_cloud_knn_mean_dist(
        _ctx(ctx), _ffi.ptr(pts, _d), n, k, cell, _ffi.ptr(mean, _d), _ffi.ptr(count, _i32),
        _ffi.C.byref(info)))
    return mean, count, _knn_info(info)


def remove_outliers(pts, k=16, std_ratio=2.0, cell=None, ctx=None):
    """Statistical outlier removal: a point stays when its mean distance to its k nearest other
    points (``knn_mean_dist``) is at most mean + std_ratio * std of the finite such distances
    (np.mean and np.std on the host).  Returns (keep (n,) bool, mean_dist (n,), threshold);
    rows whose mean_dist is NaN are dropped.  It belongs between ``dense.fuse`` and
    ``save_txt`` / ``surface.integrate``."""
    std_ratio = float(std_ratio)
    if not np.isfinite(std_ratio):
        raise ValueError('std_ratio must be finite')
    mean, _, _ = knn_mean_dist(pts, k, cell=cell, ctx=ctx)
    fin = mean[np.isfinite(mean)]
    threshold = float(np.mean(fin) + std_ratio * np.std(fin)) if len(fin) else np.nan
    with np.errstate(invalid='ignore'):
        keep = mean <= threshold
    return keep, mean, threshold


def knn_timing(enable, ctx=None):
    """Enable / disable HIP events between the stages of the next k-NN calls
    (rs_cloud_knn_timing); returns the last timed call's {stage: device ms}, -1 where none."""
    ctx = ctx or _ffi.default_context()
    ms = np.zeros(len(_ffi.CLOUD_KNN_STAGES))
    _ffi.check(_ffi.lib().rs_cloud_knn_timing(ctx.handle, int(enable), _ffi.ptr(ms, _d)))
    return dict(zip(_ffi.CLOUD_KNN_STAGES, ms.tolist()))


def fpfh(points, normals, k=32, cell=None, ctx=None):
    """Fast point feature histograms over k-NN neighbourhoods (rs_cloud_fpfh, where every order of
    operations is written down): 3 x 11 bins per point, the descriptor ``match_features`` and
    ``evaluation.global_register`` work on.

    The neighbours of point i are ``knn(points, k + 1)``'s row i with i dropped by the rule of
    ``knn_mean_dist``; neighbours by number and not by radius make the descriptor invariant to
    scale for clouds of comparable sampling.  A pair (i, j) is counted unless d2 = 0, a normal
    is not finite, or p_j - p_i is parallel to n_i; the third feature is a diamond pseudo-angle
    in place of atan2, so that every bit can be restated (tests/global_ref.py).  1 <= k <= 63.

    Returns (fpfh (n, 33), count (n,) int32, info): count the number of counted pairs, info as
    ``knn``'s.  A row without a counted pair, or whose neighbours have none, is NaN.  The result
    does not depend on ``cell``."""
    points, k, cell = _knn_args(points, k, _ffi.CLOUD_KNN_MAX_K - 1, cell)
    normals = _ffi.f64c(normals)
    if normals.shape != points.shape:
        raise ValueError('normals must have the shape of points')
    n = len(points)
    out = np.full((n, _ffi.FPFH_BINS), np.nan)
    count = np.zeros(n, dtype=np.int32)
    info = _ffi.KnnInfo()
    _ffi.check(_ffi.lib().rs_cloud_fpfh(
        _ctx(ctx), _ffi.ptr(points, _d), _ffi.ptr(normals, _d), n, k, cell, _ffi.ptr(out, _d),
        _ffi.ptr(count, _i32), _ffi.C.byref(info)))
    return out, count, _knn_info(info)


def match_features(fa, fb, mutual=False, ctx=None):
    """For every row of fa (n, D) the nearest row of fb (m, D) by brute force (rs_feature_match),
    D <= 64: idx (n,) int32 the lowest index among the rows with the smallest
    d2 = sum_c (a_c - b_c)^2 (summed left to right), d2 (n,) that value.  A row with a NaN matches
    nothing and is nobody's match: idx = -1, d2 = +inf; so is every row when m = 0.

    ``mutual=True`` is a host-side filter on two calls: idx[i] stays only where the nearest row
    of fa to fb[idx[i]] is i again; the others become -1 / +inf.  Returns (idx, d2)."""
    fa, fb = _ffi.f64c(fa), _ffi.f64c(fb)
    if fa.ndim != 2 or fb.ndim != 2 or fa.shape[1] != fb.shape[1]:
        raise ValueError('fa and fb must be (n, D) and (m, D)')
    D = fa.shape[1]
    if not 1 <= D <= _ffi.FEATURE_MATCH_MAX_D:
        raise ValueError(f'D must be in 1..{_ffi.FEATURE_MATCH_MAX_D}')
    if max(len(fa), len(fb)) > _ffi.CLOUD_MAX_POINTS:
        raise ValueError('more rows than RS_CLOUD_MAX_POINTS = 2^28')

    def one(a, b):
        idx = np.full(len(a), -1, dtype=np.int32)
        d2 = np.full(len(a), np.inf)
        _ffi.check(_ffi.lib().rs_feature_match(
            _ctx(ctx), _ffi.ptr(a, _d), len(a), _ffi.ptr(b, _d), len(b), D, _ffi.ptr(idx, _i32),
            _ffi.ptr(d2, _d)))
        return idx, d2

    idx, d2 = one(fa, fb)
    if mutual:
        back, _ = one(fb, fa)
        keep = idx >= 0
        keep[keep] = back[idx[keep]] == np.flatnonzero(keep)
        idx, d2 = np.where(keep, idx, -1).astype(np.int32), np.where(keep, d2, np.inf)
    return idx, d2


def global_timing(enable, ctx=None):
    """Enable / disable HIP events around the kernels of the next fpfh, match_features and
    evaluation.ransac_similarity calls (rs_global_timing); returns the last timed calls'
    {stage: device ms}, -1 where none."""
    ctx = ctx or _ffi.default_context()
    ms = np.zeros(len(_ffi.GLOBAL_STAGES))
    _ffi.check(_ffi.lib().rs_global_timing(ctx.handle, int(enable), _ffi.ptr(ms, _d)))
    return dict(zip(_ffi.GLOBAL_STAGES, ms.tolist()))


def save_txt(path, points, colors, normals, reflectance=1.0):
    """The export of 3Dvisualization.py:139-145: one row per point -- x y z, reflectance, r g b,
    nx ny nz -- through np.savetxt(..., delimiter=' ')."""
    points, colors, normals = (np.asarray(a, dtype=np.float64) for a in (points, colors, normals))
    n = len(points)
    for name, a in (('points', points), ('colors', colors), ('normals', normals)):
        if a.shape != (n, 3):
            raise ValueError(f'{name} must be (n, 3)')
    refl = np.empty((n, 1))
    refl[:] = np.asarray(reflectance, dtype=np.float64).reshape(-1, 1) \
        if np.ndim(reflectance) else float(reflectance)
    result = np.append(points, refl, axis=1)
    result = np.append(result, colors, axis=1)
    result = np.append(result, normals, axis=1)
    np.savetxt(path, result, delimiter=' ')
