"""numpy restatement of the point-cloud stage (include/rsamd.h, rs_cloud_attributes and
rs_cloud_normals) for tests/test_cloud_cpu.py and tests/test_gpu_cloud.py.  Test
infrastructure: brute force, small clouds only.

surface_normals: neighbourhoods from the full (n, n) table of squared distances, evaluated as
dx*dx + dy*dy + dz*dz in float64; M = S/k - (s/k)(s/k)^T about the query point; np.linalg.eigh;
the two sign rules.  point_attributes: the loops of tables.py:189-226 over a flat entry list,
including whatever the list holds of the reference's spurious 0.
"""
from __future__ import annotations

import numpy as np


def squared_distances(pts):
    """(n, n) |p_j - p_i|^2; NaN rows and columns for non-finite points."""
    d = pts[None, :, :] - pts[:, None, :]
    with np.errstate(invalid="ignore", over="ignore"):
        return d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]


def boundary_margin(pts, radius):
    """The smallest | |p_j - p_i| / radius - 1 | over all pairs of finite points: how far the
    nearest pair stays from the predicate's boundary."""
    fin = np.isfinite(pts).all(axis=1)
    d2 = squared_distances(pts[fin])
    return float(np.abs(np.sqrt(d2) / radius - 1.0).min())


def orient_sign(v, o=None):
    """+1 or -1: the factor that gives v the contract's sign."""
    if o is not None and np.isfinite(o).all() and np.any(o != 0.0):
        return -1.0 if float(np.dot(v, o)) < 0.0 else 1.0
    big = int(np.argmax(np.abs(v)))        # the first of the largest
    return -1.0 if v[big] < 0.0 else 1.0


def surface_normals(pts, radius, orient=None):
    """(normals, ok, count, evals): the contract of rs_cloud_normals, row by row."""
    pts = np.asarray(pts, dtype=np.float64).reshape(-1, 3)
    n = len(pts)
    fin = np.isfinite(pts).all(axis=1)
    d2 = squared_distances(pts)
    with np.errstate(invalid="ignore"):
        near = (d2 <= radius * radius) & fin[:, None] & fin[None, :]
    count = near.sum(axis=1).astype(np.int32)
    ok = count >= 3
    normals, evals = np.full((n, 3), np.nan), np.full((n, 3), np.nan)
    for i in np.flatnonzero(ok):
        d = pts[near[i]] - pts[i]          # ascending j
        k = float(count[i])
        mean = d.sum(axis=0) / k
        M = (d[:, :, None] * d[:, None, :]).sum(axis=0) / k - np.outer(mean, mean)
        w, V = np.linalg.eigh(M)
        v = V[:, 0] / np.linalg.norm(V[:, 0])
        evals[i] = w
        normals[i] = orient_sign(v, None if orient is None else orient[i]) * v
    return normals, ok, count, evals


def point_attributes(cams, pts, entry_point, entry_obs, obs_view, obs_color):
    """(colors, normals): per point, over its entries in list order, the mean colour / 255 and
    the mean of centre(view) - point with centre = -R^T t.  NaN for a point without an entry."""
    cams = np.asarray(cams, dtype=np.float64).reshape(-1, 3, 4)
    pts = np.asarray(pts, dtype=np.float64).reshape(-1, 3)
    centres = np.array([-1.0 * (c[:, :3].T @ c[:, 3]) for c in cams]).reshape(-1, 3)
    colors, normals = np.full(pts.shape, np.nan), np.full(pts.shape, np.nan)
    for j in range(len(pts)):
        own = np.asarray(entry_obs)[np.asarray(entry_point) == j]
        if len(own) == 0:
            continue
        col, vec = np.zeros(3), np.zeros(3)
        for o in own:
            col = col + np.asarray(obs_color[o], dtype=np.float64)
            vec = vec + (centres[obs_view[o]] - pts[j])
        colors[j] = col / len(own) / 255.0
        normals[j] = vec / len(own)
    return colors, normals


def table_entries(T):
    """The flat entry list of a table: every point's observations_index as it stands."""
    idx = [np.asarray(p.observations_index, dtype=np.int64).ravel() for p in T.T_points]
    entry_point = np.repeat(np.arange(len(idx)), [len(i) for i in idx])
    return entry_point, (np.concatenate(idx) if idx else np.zeros(0, np.int64))


def table_attributes(T):
    """(points, colors, normals) of a table through point_attributes."""
    cams = np.array([np.hstack([v.camera_pose.R, np.reshape(v.camera_pose.t, (3, 1))])
                     for v in T.T_views])
    pts = np.array([p.point for p in T.T_points], dtype=np.float64).reshape(-1, 3)
    ov = np.array([o.view_index for o in T.T_obs])
    col = np.array([o.color for o in T.T_obs], dtype=np.float64).reshape(-1, 3)
    ep, eo = table_entries(T)
    colors, normals = point_attributes(cams, pts, ep, eo, ov, col)
    return pts, colors, normals
