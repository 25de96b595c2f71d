"""The point-cloud stage (HIP kernels of cloud.hip): what main.py does last (main.py:175-176) and
the export of 3Dvisualization.py.

  * ``point_attributes``  the arithmetic of Tables.getColorFor3DPoint / getNormalFor3DPoint
                          (tables.py:189-214) for every point at once: the mean colour / 255 and
                          the mean direction to the cameras that see the point
  * ``surface_normals``   the plane fit 3Dvisualization.py attempts and leaves commented out
                          (3Dvisualization.py:16-31, :96-113), by its mathematics: fixed-radius
                          neighbourhoods, the smallest eigenvector of the neighbourhood's
                          covariance, a sign
  * ``save_txt``          the ten-column file of 3Dvisualization.py:139-145 (host only)

The contract of both kernels stands in include/rsamd.h.  The table-level drop-in is
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
