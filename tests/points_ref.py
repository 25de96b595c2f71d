"""numpy restatement of the surface from oriented points (include/rsamd.h:
rs_surface_points_volume, rs_surface_points_eval) for tests/test_points_cpu.py and
tests/test_gpu_points.py.  Test infrastructure: small clouds and volumes only.

  * field    the lists of knn_ref.knn (brute force) over the points that are not out, then the
             slot loop vectorised over the queries: slot s of every list is added before slot
             s + 1 of any, so each query's sums run in list order, one operation at a time
  * volume   field on the nodes of surface_ref.node_positions, the clamp and the float32 cast
"""
from __future__ import annotations

import numpy as np

import knn_ref as kr
import surface_ref as sr


BLOCK = 8192     # queries per brute-force table


def field(pts, normals, queries, radius, k, colors=None):
    """(value (m,), count (m,) int32, color (m, 3) or None, saturated (m,) bool)."""
    X = np.asarray(queries, dtype=np.float64).reshape(-1, 3)
    if len(X) > BLOCK:
        parts = [_field(pts, normals, X[at:at + BLOCK], radius, k, colors)
                 for at in range(0, len(X), BLOCK)]
        return tuple(None if p[0] is None else np.concatenate(p) for p in zip(*parts))
    return _field(pts, normals, X, radius, k, colors)


def _field(pts, normals, X, radius, k, colors):
    pts = np.asarray(pts, dtype=np.float64).reshape(-1, 3)
    normals = np.asarray(normals, dtype=np.float64).reshape(-1, 3)
    m, radius = len(X), float(radius)
    out_pts = np.where(np.isfinite(normals).all(axis=1)[:, None], pts, np.nan)   # out: no neighbour
    idx, d2, count = kr.knn(out_pts, k, queries=X, max_dist=radius)
    acc, sw, cacc = np.zeros(m), np.zeros(m), np.zeros((m, 3))
    with np.errstate(invalid="ignore", over="ignore"):
        for s in range(k if len(pts) else 0):
            on = s < count
            j = np.where(on, idx[:, s], 0)
            d = X - pts[j]
            u = np.minimum(np.sqrt(np.where(on, d2[:, s], 0.0)) / radius, 1.0)
            a = 1.0 - u
            a2 = a * a
            w = (a2 * a2) * (4.0 * u + 1.0)
            nj = normals[j]
            dot = d[:, 0] * nj[:, 0] + d[:, 1] * nj[:, 1] + d[:, 2] * nj[:, 2]
            acc = np.where(on, acc + w * dot, acc)
            sw = np.where(on, sw + w, sw)
            if colors is not None:
                cacc = np.where(on[:, None], cacc + w[:, None] * np.asarray(colors)[j], cacc)
    some = sw > 0.0
    with np.errstate(invalid="ignore", divide="ignore"):
        value = np.where(some, acc / sw, np.nan)
        color = None if colors is None else np.where(some[:, None], cacc / sw[:, None], np.nan)
    return value, count, color, count == k


def volume(pts, normals, origin, voxel, dims, radius, k, trunc=None):
    """(tsdf, weight) float32 (nz, ny, nx), and (value, count, saturated) per node, flat."""
    X = sr.node_positions(origin, float(voxel), dims).reshape(-1, 3)
    value, count, _, sat = field(pts, normals, X, radius, k)
    trunc = float(radius if trunc is None else trunc)
    with np.errstate(invalid="ignore"):
        t = value / trunc
        t = np.where(t > 1.0, 1.0, t)
        t = np.where(t < -1.0, -1.0, t)
    tsdf = np.where(np.isnan(value), np.float32(np.nan), t.astype(np.float32)).astype(np.float32)
    return tsdf.reshape(dims), count.astype(np.float32).reshape(dims), (value, count, sat)
