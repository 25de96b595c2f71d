"""Numpy restatement of the evaluation stage's kernel (include/rsamd.h, rs_eval_mesh_distance): a
brute force over all (query, face) pairs with the closest-point routine in the header's order of
operations -- every product and sum spelled out, no np.dot, no einsum, so nothing is fused or
reordered -- and restatements of the host functions of tsbb15_amd.evaluation that are not trivial.
``dtype=np.longdouble`` runs the same operations in extended precision; the difference between
the two runs is the error the fp64 routine itself has.
"""
import numpy as np


def _dot(u, v):
    return u[0] * v[0] + u[1] * v[1] + u[2] * v[2]


def face_valid(vertices, faces):
    """(nf) bool: nine finite coordinates and a cross product that is not exactly zero (fp64)."""
    v = np.asarray(vertices, dtype=np.float64)
    f = np.asarray(faces).reshape(-1, 3)
    a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    finite = np.isfinite(a).all(axis=1) & np.isfinite(b).all(axis=1) & np.isfinite(c).all(axis=1)
    with np.errstate(invalid='ignore', over='ignore'):
        ab, ac = (b - a).T, (c - a).T
        n0 = ab[1] * ac[2] - ab[2] * ac[1]
        n1 = ab[2] * ac[0] - ab[0] * ac[2]
        n2 = ab[0] * ac[1] - ab[1] * ac[0]
    return finite & ~((n0 == 0.0) & (n1 == 0.0) & (n2 == 0.0))


def closest_point(p, a, b, c):
    """The header's ClosestPtPointTriangle on broadcastable arrays (..., 3) of one dtype.
    Returns (q (..., 3), d2 (...)).  Every branch is evaluated and the first rule that holds is
    selected, which gives the bits of the branching code."""
    p, a, b, c = (np.moveaxis(np.asarray(x), -1, 0) for x in np.broadcast_arrays(p, a, b, c))
    with np.errstate(all='ignore'):
        ab, ac, ap = b - a, c - a, p - a
        d1, d2 = _dot(ab, ap), _dot(ac, ap)
        bp = p - b
        d3, d4 = _dot(ab, bp), _dot(ac, bp)
        cp = p - c
        d5, d6 = _dot(ab, cp), _dot(ac, cp)
        vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
        e43, e56 = d4 - d3, d5 - d6
        s = (va + vb) + vc
        rules = [
            ((d1 <= 0) & (d2 <= 0), a),
            ((d3 >= 0) & (d4 <= d3), b),
            ((d6 >= 0) & (d5 <= d6), c),
            ((vc <= 0) & (d1 >= 0) & (d3 <= 0), a + (d1 / (d1 - d3)) * ab),
            ((vb <= 0) & (d2 >= 0) & (d6 <= 0), a + (d2 / (d2 - d6)) * ac),
            ((va <= 0) & (e43 >= 0) & (e56 >= 0), b + (e43 / (e43 + e56)) * (c - b)),
        ]
        q = (a + (vb / s) * ab) + (vc / s) * ac
        for cond, val in reversed(rules):
            q = np.where(cond, val, q)
        e = p - q
        dd = _dot(e, e)
    return np.moveaxis(q, 0, -1), dd


def pair_d2(pts, vertices, faces, dtype=np.float64, chunk=256):
    """(n, nf) squared distances and the valid-face mask; an invalid face's column is +inf, and
    so is a NaN (it never wins)."""
    pts = np.asarray(pts, dtype=np.float64)
    f = np.asarray(faces).reshape(-1, 3)
    valid = face_valid(vertices, f)
    v = np.asarray(vertices, dtype=np.float64).astype(dtype)
    a, b, c = v[f[:, 0]][None], v[f[:, 1]][None], v[f[:, 2]][None]
    out = np.empty((len(pts), len(f)), dtype=dtype)
    for at in range(0, len(pts), chunk):
        p = pts[at:at + chunk].astype(dtype)[:, None, :]
        out[at:at + chunk] = closest_point(p, a, b, c)[1]
    out[:, ~valid] = np.inf
    out[np.isnan(out)] = np.inf
    return out, valid


def mesh_distance(pts, vertices, faces, max_dist=np.inf, dtype=np.float64, return_pairs=False):
    """(d2, face, closest) of rs_eval_mesh_distance, by brute force, in ``dtype``."""
    pts = np.asarray(pts, dtype=np.float64).reshape(-1, 3)
    f = np.asarray(faces).reshape(-1, 3)
    n = len(pts)
    pairs, valid = pair_d2(pts, vertices, f, dtype)
    d2 = np.full(n, np.inf, dtype=dtype)
    face = np.full(n, -1, dtype=np.int32)
    closest = np.full((n, 3), np.nan, dtype=dtype)
    if len(f):
        best = pairs.argmin(axis=1)          # the first, so the lowest, index of the minimum
        d2 = pairs[np.arange(n), best]
        won = np.isfinite(d2)
        face = np.where(won, best, -1).astype(np.int32)
        v = np.asarray(vertices, dtype=np.float64).astype(dtype)
        tri = v[f[best]]
        closest = closest_point(pts.astype(dtype), tri[:, 0], tri[:, 1], tri[:, 2])[0]
    md = dtype(max_dist)
    beyond = ~(d2 <= md * md)
    bad = ~np.isfinite(pts).all(axis=1)
    d2 = np.where(beyond, dtype(np.inf), d2)
    d2 = np.where(bad, dtype(np.nan), d2)
    face = np.where(beyond | bad, -1, face).astype(np.int32)
    closest = np.where((face < 0)[:, None], dtype(np.nan), closest)
    if return_pairs:
        return d2, face, closest, pairs
    return d2, face, closest


def grid_entries(vertices, faces, cell):
    """(dims, entries, largest_cell) of the header's grid: the box of the faces with finite
    coordinates, floor((hi - lo) / cell) + 1 cells per axis, every valid face registered in every
    cell its own box overlaps."""
    v = np.asarray(vertices, dtype=np.float64)
    f = np.asarray(faces).reshape(-1, 3)
    tri = v[f]
    finite = np.isfinite(tri).all(axis=(1, 2)) if len(f) else np.zeros(0, bool)
    if not finite.any():
        return (1, 1, 1), 0, 0
    lo, hi = tri[finite].min(axis=(0, 1)), tri[finite].max(axis=(0, 1))
    dims = (np.floor((hi - lo) / cell) + 1).astype(np.int64)
    t = tri[face_valid(v, f)]
    c0 = np.clip(np.floor((t.min(axis=1) - lo) / cell), 0, dims - 1).astype(np.int64)
    c1 = np.clip(np.floor((t.max(axis=1) - lo) / cell), 0, dims - 1).astype(np.int64)
    count = np.zeros(tuple(dims), dtype=np.int64)
    for (x0, y0, z0), (x1, y1, z1) in zip(c0, c1):
        count[x0:x1 + 1, y0:y1 + 1, z0:z1 + 1] += 1
    return tuple(int(d) for d in dims), int(count.sum()), int(count.max()) if len(t) else 0


def barycentric(points, a, b, c):
    """Barycentric coordinates (n, 3) of points in the planes of the triangles (a, b, c), by the
    normal equations in longdouble; for a point of the triangle all three lie in [0, 1]."""
    p, a, b, c = (np.asarray(x, dtype=np.longdouble) for x in (points, a, b, c))
    u, v, w = b - a, c - a, p - a
    uu, uv, vv = (u * u).sum(-1), (u * v).sum(-1), (v * v).sum(-1)
    wu, wv = (w * u).sum(-1), (w * v).sum(-1)
    den = uu * vv - uv * uv
    s, t = (wu * vv - wv * uv) / den, (wv * uu - wu * uv) / den
    return np.stack([1 - s - t, s, t], axis=-1)


# ---- host functions ----------------------------------------------------------------------------

def kth_smallest(dist, fraction):
    """accuracy by a full sort."""
    d = np.sort(np.asarray(dist, dtype=np.float64))
    k = int(np.ceil(np.round(fraction * len(d), 9)))
    return float(d[max(k, 1) - 1])


def umeyama(src, dst, with_scale=True):
    """Umeyama (1991), eqs. 34-43, written from the paper: dst ~ s R src + t."""
    src, dst = np.asarray(src, float), np.asarray(dst, float)
    n = len(src)
    mx, my = src.sum(0) / n, dst.sum(0) / n
    sx2 = ((src - mx) ** 2).sum() / n
    cov = np.zeros((3, 3))
    for x, y in zip(src - mx, dst - my):
        cov += np.outer(y, x) / n
    U, D, Vt = np.linalg.svd(cov)
    S = np.eye(3)
    if np.linalg.det(cov) < 0:
        S[2, 2] = -1
    R = U @ S @ Vt
    s = np.trace(np.diag(D) @ S) / sx2 if with_scale else 1.0
    return s, R, my - s * R @ mx


def rotation_angle_deg(A, B):
    """The angle of A B^T for two rotations."""
    c = (np.trace(A @ B.T) - 1.0) / 2.0
    return float(np.degrees(np.arccos(min(1.0, max(-1.0, c)))))
