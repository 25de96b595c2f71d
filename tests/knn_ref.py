"""numpy restatement of the k-NN calls of the point-cloud stage (include/rsamd.h: rs_cloud_knn,
rs_cloud_knn_normals, rs_cloud_knn_mean_dist) for tests/test_knn_cpu.py and
tests/test_gpu_knn.py.  Test infrastructure: small clouds only.

  * knn            brute force: the (m, n) table of d2 = dx*dx + dy*dy + dz*dz with d = q - p_j in
                   float64 and a stable sort, which orders by (d2, index)
  * knn_grid       the same result through the grid and the walk over Chebyshev rings the header
                   describes, in plain Python; also the grid's figures and the number of
                   candidates tested, which the GPU's info must equal
  * knn_normals    the plane fit over a point's own list, np.linalg.eigh as the independent solver
  * mean_dist, remove_outliers
"""
from __future__ import annotations

import numpy as np

SHRINK = 1.0 - 2.0 ** -20
FAR = 2.0 ** 29
MAX_CELLS = 2 ** 24


def squared_distances(pts, queries):
    """(m, n) d2(q_i, p_j); NaN where a point or a query is not finite."""
    with np.errstate(invalid="ignore", over="ignore"):
        d = queries[:, None, :] - pts[None, :, :]
        return d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]


def _arrays(pts, queries):
    pts = np.asarray(pts, dtype=np.float64).reshape(-1, 3)
    queries = pts if queries is None else np.asarray(queries, dtype=np.float64).reshape(-1, 3)
    return pts, queries


def knn(pts, k, queries=None, max_dist=np.inf):
    """(idx (m, k) int32, d2 (m, k), count (m,) int32): the contract of rs_cloud_knn."""
    pts, queries = _arrays(pts, queries)
    m, n = len(queries), len(pts)
    idx = np.full((m, k), -1, dtype=np.int32)
    out = np.full((m, k), np.inf)
    count = np.zeros(m, dtype=np.int32)
    if n == 0 or m == 0:
        return idx, out, count
    fin_p, fin_q = np.isfinite(pts).all(axis=1), np.isfinite(queries).all(axis=1)
    d2 = squared_distances(pts, queries)
    with np.errstate(invalid="ignore"):
        cand = (d2 <= max_dist * max_dist) & fin_p[None, :] & fin_q[:, None]
    key = np.where(cand, d2, np.nan)                 # a NaN sorts last, behind a +inf
    order = np.argsort(key, axis=1, kind="stable")   # ties: the lower index first
    count[:] = np.minimum(cand.sum(axis=1), k)
    w = min(k, n)
    take = np.arange(w)[None, :] < count[:, None]
    idx[:, :w] = np.where(take, order[:, :w], -1)
    out[:, :w] = np.where(take, np.take_along_axis(d2, order[:, :w], axis=1), np.inf)
    return idx, out, count


def default_cell(pts):
    """The cell rs_cloud_knn picks for cell = 0, and the box [lo, hi] of the finite points."""
    fin = pts[np.isfinite(pts).all(axis=1)]
    lo, hi = fin.min(axis=0), fin.max(axis=0)
    ext = float((hi - lo).max())
    mag = float(max(np.abs(lo).max(), np.abs(hi).max()))
    g = min(max(np.floor(np.cbrt(float(len(fin))) + 0.5), 1.0), 256.0)
    cell = max(ext / g, mag / 2.0 ** 24)
    if not ext > 0.0 or not cell > 0.0:
        cell = mag if mag > 0.0 else 1.0
    return cell, lo, hi


def _coord(x, lo, cell, limit):
    with np.errstate(invalid="ignore", over="ignore"):
        q = np.floor((x - lo) / cell)
    return np.where(q >= -limit, np.minimum(q, limit), -limit)


def knn_grid(pts, k, queries=None, max_dist=np.inf, cell=None):
    """(idx, d2, count, info): knn's result through the grid; info = dict(cells, largest_cell,
    tested, dims).  Ring by ring: all candidates of a ring's cells, then the k smallest pairs
    (d2, index) of the list so far and them."""
    pts, queries = _arrays(pts, queries)
    m = len(queries)
    idx = np.full((m, k), -1, dtype=np.int32)
    out = np.full((m, k), np.inf)
    count = np.zeros(m, dtype=np.int32)
    fin = np.flatnonzero(np.isfinite(pts).all(axis=1))
    if len(fin) == 0 or m == 0:
        return idx, out, count, {"cells": 0, "largest_cell": 0, "tested": 0, "dims": (0, 0, 0)}
    dcell, lo, hi = default_cell(pts)
    cell = dcell if cell is None or cell == 0.0 else float(cell)
    dims = (np.floor((hi - lo) / cell) + 1.0).astype(np.int64)
    assert int(np.prod(dims)) <= MAX_CELLS
    pc = np.maximum(_coord(pts[fin], lo, cell, (dims - 1).astype(np.float64)), 0.0).astype(np.int64)
    cid = (pc[:, 2] * dims[1] + pc[:, 1]) * dims[0] + pc[:, 0]
    order = np.argsort(cid, kind="stable")
    members = fin[order]                                      # point indices by cell
    ncell = int(np.prod(dims))
    start = np.searchsorted(cid[order], np.arange(ncell + 1))
    tested = 0
    md2 = max_dist * max_dist
    for i in np.flatnonzero(np.isfinite(queries).all(axis=1)):
        q = queries[i]
        c = _coord(q, lo, cell, FAR).astype(np.int64)
        r0 = int(max(0, np.max(np.maximum(-c, c - (dims - 1)))))
        rmax = int(max(0, np.max(np.maximum(c, dims - 1 - c))))
        best_d, best_j = np.zeros(0), np.zeros(0, dtype=np.int64)
        for r in range(r0, rmax + 1):
            if r > 0:
                bound = float(r - 1) * cell * SHRINK
                if (len(best_d) == k and best_d[-1] <= bound * bound) or bound > max_dist:
                    break
            ax = [np.arange(max(c[a] - r, 0), min(c[a] + r, dims[a] - 1) + 1) for a in range(3)]
            X, Y, Z = np.meshgrid(ax[0], ax[1], ax[2], indexing="ij")
            shell = np.maximum(np.maximum(np.abs(X - c[0]), np.abs(Y - c[1])), np.abs(Z - c[2])) == r
            ids = ((Z * dims[1] + Y) * dims[0] + X)[shell]
            ids = ids[start[ids + 1] > start[ids]]
            if len(ids) == 0:
                continue
            js = np.concatenate([members[start[t]:start[t + 1]] for t in ids])
            d = q - pts[js]
            d2 = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]
            tested += len(js)
            ok = d2 <= md2
            all_d, all_j = np.concatenate([best_d, d2[ok]]), np.concatenate([best_j, js[ok]])
            o = np.lexsort((all_j, all_d))[:k]
            best_d, best_j = all_d[o], all_j[o]
        count[i] = len(best_d)
        idx[i, :len(best_d)] = best_j
        out[i, :len(best_d)] = best_d
    info = {"cells": ncell, "largest_cell": int(np.diff(start).max()), "tested": int(tested),
            "dims": tuple(int(x) for x in dims)}
    return idx, out, count, info


def orient_sign(v, o=None):
    """+1 or -1: the factor that gives v the contract's sign (that of rs_cloud_normals)."""
    if o is not None and np.isfinite(o).all() and np.any(o != 0.0):
        return -1.0 if float(np.dot(v, o)) < 0.0 else 1.0
    big = int(np.argmax(np.abs(v)))
    return -1.0 if v[big] < 0.0 else 1.0


def knn_normals(pts, k, orient=None, lists=None):
    """(normals, ok, count, evals, d2k): the contract of rs_cloud_knn_normals row by row; d2k is
    the d2 of the row's last entry (NaN where the row is empty)."""
    pts = np.asarray(pts, dtype=np.float64).reshape(-1, 3)
    n = len(pts)
    idx, d2, count = lists if lists is not None else knn(pts, k)
    ok = count >= 3
    normals, evals, d2k = np.full((n, 3), np.nan), np.full((n, 3), np.nan), np.full(n, np.nan)
    for i in range(n):
        c = int(count[i])
        if c > 0:
            d2k[i] = d2[i, c - 1]
        if c < 3:
            continue
        d = pts[idx[i, :c]] - pts[i]
        mean = d.sum(axis=0) / c
        M = (d[:, :, None] * d[:, None, :]).sum(axis=0) / c - np.outer(mean, mean)
        w, V = np.linalg.eigh(M)
        v = V[:, 0] / np.linalg.norm(V[:, 0])
        evals[i] = w
        normals[i] = orient_sign(v, None if orient is None else orient[i]) * v
    return normals, ok, count, evals, d2k


def mean_dist(pts, k, lists=None):
    """(mean_dist (n,), count (n,)): the contract of rs_cloud_knn_mean_dist; the sum runs in
    list order (np.cumsum adds one term after the other, np.sum does not)."""
    pts = np.asarray(pts, dtype=np.float64).reshape(-1, 3)
    idx, d2, count = lists if lists is not None else knn(pts, k + 1)
    out = np.full(len(pts), np.nan)
    for i in range(len(pts)):
        c = int(count[i])
        if c <= 1:
            continue
        own = np.flatnonzero(idx[i, :c] == i)
        drop = int(own[0]) if len(own) else c - 1
        rest = np.sqrt(np.delete(d2[i, :c], drop))
        out[i] = np.cumsum(rest)[-1] / float(c - 1)
    return out, count


def remove_outliers(pts, k=16, std_ratio=2.0):
    """(keep, mean_dist, threshold)."""
    md, _ = mean_dist(pts, k)
    fin = md[np.isfinite(md)]
    threshold = float(np.mean(fin) + std_ratio * np.std(fin)) if len(fin) else np.nan
    with np.errstate(invalid="ignore"):
        return md <= threshold, md, threshold
