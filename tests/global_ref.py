"""Numpy restatement of the global registration (include/rsamd.h, "Global registration"), written
from the header: rs_cloud_fpfh, rs_feature_match, rs_sim3_ransac and evaluation.global_register's
orchestration.  Every expression keeps the header's order of operations -- numpy's elementwise
fp64 operations round once each and fuse nothing -- so the GPU's outputs are compared with these
bit for bit.
"""
import numpy as np

import eval_ref
import knn_ref
import philox_ref
import register_ref

BINS = 33
CHUNK = 1 << 20          # RS_SIM3_CHUNK
TILE = 96                # RS_FEATURE_MATCH_TILE


def dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1],
                     a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def pseudo_angle(x, y):
    """The diamond angle in [0, 4] of (x, y), 0 unless |x| + |y| > 0."""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    with np.errstate(invalid='ignore', divide='ignore'):
        den = np.abs(x) + np.abs(y)
        r = y / den
        a = np.where(x >= 0.0, 1.0 + r, np.where(y >= 0.0, 3.0 - r, (-1.0 - r) + 4.0))
        return np.where(den > 0.0, a, 0.0)


def bin11(q):
    """0 unless floor(q) >= 0, 10 where floor(q) > 10, else floor(q)."""
    with np.errstate(invalid='ignore'):
        f = np.floor(q)
        return np.where(f >= 0.0, np.where(f > 10.0, 10.0, f), 0.0).astype(np.int64)


def neighbour_lists(points, k):
    """(idx (n, k + 1), d2, use (n, k + 1) bool): rs_cloud_knn's rows of the k + 1 nearest and the
    entries that remain after the drop of rs_cloud_knn_mean_dist."""
    idx, d2, count = knn_ref.knn(points, k + 1)
    n, K = idx.shape
    e = np.arange(K)[None, :]
    listed = e < count[:, None]
    own = listed & (idx == np.arange(n)[:, None])
    drop = np.where(own.any(axis=1), own.argmax(axis=1), count - 1)
    return idx, d2, listed & (e != drop[:, None])


def pair_features(points, normals, idx, d2, use):
    """(counted (n, K) bool, f1, f2, a) of every listed pair; the features hold garbage where the
    pair is not counted."""
    n, K = idx.shape
    j = np.where(use, idx, 0)
    with np.errstate(invalid='ignore', divide='ignore', over='ignore'):
        u = np.broadcast_to(normals[:, None, :], (n, K, 3))
        nj = normals[j]
        d = points[j] - points[:, None, :]
        cr = cross(d, u)
        cc = dot(cr, cr)
        counted = (use & (d2 > 0.0) & np.isfinite(u).all(axis=2) & np.isfinite(nj).all(axis=2)
                   & (cc > 0.0))
        v = cr / np.sqrt(cc)[..., None]
        w = cross(u, v)
        f1 = dot(v, nj)
        f2 = dot(u, d) / np.sqrt(d2)
        a = pseudo_angle(dot(u, nj), dot(w, nj))
    return counted, f1, f2, a


def spfh(points, normals, k, lists=None):
    """(SPFH (n, 33) int32, c (n,) int32, lists)."""
    points = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    normals = np.asarray(normals, dtype=np.float64).reshape(-1, 3)
    idx, d2, use = lists or neighbour_lists(points, k)
    counted, f1, f2, a = pair_features(points, normals, idx, d2, use)
    hist = np.zeros((len(points), BINS), dtype=np.int32)
    rows = np.nonzero(counted)[0]
    np.add.at(hist, (rows, bin11((f1[counted] + 1.0) * 5.5)), 1)
    np.add.at(hist, (rows, 11 + bin11((f2[counted] + 1.0) * 5.5)), 1)
    np.add.at(hist, (rows, 22 + bin11(a[counted] * 2.75)), 1)
    return hist, counted.sum(axis=1).astype(np.int32), (idx, d2, use)


def fpfh(points, normals, k=32):
    """(fpfh (n, 33), count (n,) int32): the contract of rs_cloud_fpfh."""
    hist, c, (idx, d2, use) = spfh(points, normals, k)
    n, K = idx.shape
    A, W = np.zeros((n, BINS)), np.zeros(n)
    anyj = np.zeros(n, dtype=bool)
    for e in range(K):                        # list order
        j = np.where(use[:, e], idx[:, e], 0)
        with np.errstate(invalid='ignore', divide='ignore'):
            on = use[:, e] & (d2[:, e] > 0.0) & (c[j] > 0) & (c > 0)
            w = 1.0 / np.sqrt(d2[:, e])
            term = (w[:, None] * hist[j].astype(np.float64)) / c[j].astype(np.float64)[:, None]
        A = A + np.where(on[:, None], term, 0.0)
        W = W + np.where(on, w, 0.0)
        anyj |= on
    with np.errstate(invalid='ignore', divide='ignore'):
        out = hist.astype(np.float64) / c.astype(np.float64)[:, None] + A / W[:, None]
    out[~anyj] = np.nan
    return out, c


def match(fa, fb):
    """(idx (n,) int32, d2 (n,)): the contract of rs_feature_match."""
    fa, fb = np.asarray(fa, dtype=np.float64), np.asarray(fb, dtype=np.float64)
    n, m = len(fa), len(fb)
    if m == 0 or n == 0:
        return np.full(n, -1, dtype=np.int32), np.full(n, np.inf)
    with np.errstate(invalid='ignore', over='ignore'):
        e = fa[:, None, 0] - fb[None, :, 0]
        D2 = e * e
        for c in range(1, fa.shape[1]):
            e = fa[:, None, c] - fb[None, :, c]
            D2 = D2 + e * e
        key = np.where(D2 < np.inf, D2, np.inf)
    idx = key.argmin(axis=1)                   # the first of the smallest
    best = key[np.arange(n), idx]
    none = ~(best < np.inf)
    return np.where(none, -1, idx).astype(np.int32), np.where(none, np.inf, best)


def match_mutual(fa, fb):
    idx, d2 = match(fa, fb)
    back, _ = match(fb, fa)
    keep = idx >= 0
    keep[keep] = back[idx[keep]] == np.flatnonzero(keep)
    return np.where(keep, idx, -1).astype(np.int32), np.where(keep, d2, np.inf)


def _frame(p0, p1, p2):
    e1, e2 = p1 - p0, p2 - p0
    x = e1 / np.sqrt(dot(e1, e1))[:, None]
    g = cross(e1, e2)
    z = g / np.sqrt(dot(g, g))[:, None]
    return x, cross(z, x), z


def _dist(p, q):
    d = p - q
    return np.sqrt(dot(d, d))


def triple_model(a, b, with_scale=True):
    """The closed form on triples a, b (H, 3, 3): (model (H, 13), la (H, 3), lb (H, 3))."""
    with np.errstate(invalid='ignore', divide='ignore', over='ignore'):
        la = np.stack([_dist(a[:, 0], a[:, 1]), _dist(a[:, 0], a[:, 2]), _dist(a[:, 1], a[:, 2])], 1)
        lb = np.stack([_dist(b[:, 0], b[:, 1]), _dist(b[:, 0], b[:, 2]), _dist(b[:, 1], b[:, 2])], 1)
        ca = ((a[:, 0] + a[:, 1]) + a[:, 2]) / 3.0
        cb = ((b[:, 0] + b[:, 1]) + b[:, 2]) / 3.0
        sa = [dot(a[:, q] - ca, a[:, q] - ca) for q in range(3)]
        sb = [dot(b[:, q] - cb, b[:, q] - cb) for q in range(3)]
        if with_scale:
            s = np.sqrt((sb[0] + sb[1]) + sb[2]) / np.sqrt((sa[0] + sa[1]) + sa[2])
        else:
            s = np.ones(len(a))
        xa, ya, za = _frame(a[:, 0], a[:, 1], a[:, 2])
        xb, yb, zb = _frame(b[:, 0], b[:, 1], b[:, 2])
        R = ((xb[:, :, None] * xa[:, None, :] + yb[:, :, None] * ya[:, None, :])
             + zb[:, :, None] * za[:, None, :])
        t = cb - s[:, None] * ((R[:, :, 0] * ca[:, None, 0] + R[:, :, 1] * ca[:, None, 1])
                               + R[:, :, 2] * ca[:, None, 2])
    return np.concatenate([s[:, None], R.reshape(-1, 9), t], axis=1), la, lb


def count_inliers(model, src, dst, inlier_dist):
    """The score of every model (S, 13) over the correspondences."""
    chunk = max(1, min(512, 20000000 // max(len(src), 1)))      # memory only
    thr2 = inlier_dist * inlier_dist
    out = np.zeros(len(model), dtype=np.int64)
    x, y, z = src[None, :, 0], src[None, :, 1], src[None, :, 2]
    for lo in range(0, len(model), chunk):
        m = model[lo:lo + chunk]
        d = []
        with np.errstate(invalid='ignore', over='ignore'):
            for r in range(3):
                p = (m[:, 0, None] * ((m[:, 1 + 3 * r, None] * x + m[:, 2 + 3 * r, None] * y)
                                      + m[:, 3 + 3 * r, None] * z) + m[:, 10 + r, None])
                d.append(p - dst[None, :, r])
            d2 = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
            out[lo:lo + chunk] = (d2 <= thr2).sum(axis=1)
    return out


def ransac(src, dst, H, inlier_dist, seed=0, with_scale=True, scale=None, edge_tol=0.15,
           min_edge=0.0, candidates=32):
    """The contract of rs_sim3_ransac: dict(h, count, s, R, t, info) as
    evaluation.ransac_similarity returns it, and ``survivors`` (h, count, model) of all of them."""
    src = np.asarray(src, dtype=np.float64).reshape(-1, 3)
    dst = np.asarray(dst, dtype=np.float64).reshape(-1, 3)
    lo, hi = (0.0, np.inf) if scale is None else (float(scale[0]), float(scale[1]))
    M = len(src)
    passed = np.zeros(5, dtype=np.int64)
    hs, models = [], []
    for h0 in range(0, H, CHUNK):
        tup = philox_ref.floyd_tuples(seed, h0, min(CHUNK, H - h0), M, 3)
        a, b = src[tup], dst[tup]
        model, la, lb = triple_model(a, b, with_scale)
        same = lambda p, q: (p == q).all(axis=1)      # noqa: E731
        g = ~same(b[:, 0], b[:, 1]) & ~same(b[:, 0], b[:, 2]) & ~same(b[:, 1], b[:, 2])
        passed[0] += g.sum()
        with np.errstate(invalid='ignore', divide='ignore', over='ignore'):
            g = g & (la > min_edge).all(axis=1)
            passed[1] += g.sum()
            r = lb / la
            up = 1.0 + edge_tol
            g = g & ~np.isnan(r).any(axis=1) & (r.max(axis=1) <= up * r.min(axis=1))
            if not with_scale:
                g = g & (r >= 1.0 / up).all(axis=1) & (r <= up).all(axis=1)
            passed[2] += g.sum()
            g = g & (model[:, 0] >= lo) & (model[:, 0] <= hi)
            passed[3] += g.sum()
            g = g & np.isfinite(model).all(axis=1)
            passed[4] += g.sum()
        hs.append(np.flatnonzero(g) + h0)
        models.append(model[g])
    hs, models = np.concatenate(hs), np.concatenate(models)
    count = count_inliers(models, src, dst, inlier_dist)
    order = np.lexsort((hs, -count))[:candidates]
    c = len(order)
    return {"h": hs[order].astype(np.int64), "count": count[order], "s": models[order, 0],
            "R": models[order, 1:10].reshape(c, 3, 3), "t": models[order, 10:13],
            "info": {"hypotheses": H, "passed": passed, "tests": len(hs) * M, "found": c},
            "survivors": (hs, count, models)}


def face_normals(vertices, faces):
    tri = np.asarray(vertices, dtype=np.float64)[np.asarray(faces).reshape(-1, 3)]
    cr = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    with np.errstate(invalid='ignore', divide='ignore'):
        return cr / np.sqrt((cr * cr).sum(axis=1))[:, None]


def rms_radius(points):
    p = np.asarray(points, dtype=np.float64)
    return float(np.sqrt(((p - p.mean(axis=0)) ** 2).sum(axis=1).mean()))


def mesh_d2(pts, vertices, faces):
    """The d2 of eval_ref.mesh_distance (max_dist = +inf) for finite points and a mesh of valid
    faces, by the same pair expression on fewer pairs: a face can hold the minimum only if its
    centroid lies within (the distance to the nearest vertex) + (the largest face radius) of the
    point.  A minimum over a superset of its minimiser is the same number, so every bit agrees
    with the brute force (tests/test_global_cpu.py checks that)."""
    from scipy.spatial import cKDTree
    pts = np.asarray(pts, dtype=np.float64).reshape(-1, 3)
    v = np.asarray(vertices, dtype=np.float64)
    f = np.asarray(faces).reshape(-1, 3)
    assert eval_ref.face_valid(v, f).all() and np.isfinite(pts).all()
    tri = v[f]
    cen = tri.mean(axis=1)
    rad = np.sqrt(((tri - cen[:, None, :]) ** 2).sum(axis=2)).max()
    ub = cKDTree(v[np.unique(f)]).query(pts)[0]
    near = cKDTree(cen).query_ball_point(pts, (ub + rad) * (1.0 + 1e-6) + 1e-300)
    sizes = np.array([len(c) for c in near])
    rows = np.repeat(np.arange(len(pts)), sizes)
    cols = np.concatenate([np.asarray(c, dtype=np.int64) for c in near])
    d2 = eval_ref.closest_point(pts[rows], tri[cols, 0], tri[cols, 1], tri[cols, 2])[1]
    d2 = np.where(np.isnan(d2), np.inf, d2)
    return np.minimum.reduceat(d2, np.concatenate(([0], np.cumsum(sizes)[:-1])))


def trimmed_rms(points, vertices, faces, s, R, t, keep):
    """The rms evaluation.step_rms("point", ...) reports for MeshIndex.step(s, R, t, keep=keep,
    metric="point") on finite points: register_ref.step's, with mesh_d2 for the distances."""
    d2 = mesh_d2(register_ref.transform(points, s, R, t), vertices, faces)
    k = register_ref.trim_rank(keep, len(d2))
    mask = d2 <= np.sort(d2)[k - 1]
    total = register_ref.ordered_sum(np.where(mask, d2, 0.0)[:, None])[0]
    return float(np.sqrt(total / mask.sum()))


def coarse(points, normals, vertices, faces, target, target_fpfh, k=32, H=100000, candidates=32,
           keep=0.75, seed=0, with_scale=True, edge_tol=0.15, min_edge=0.0, verify=True):
    """evaluation.global_register up to its verified coarse pose.  ``target`` and ``target_fpfh``
    are the mesh's samples and their descriptors (the same for every cloud of a mesh).  Returns
    dict(candidates, src, dst, scale, inlier_dist, rms, chosen, coarse)."""
    fa, _ = fpfh(points, normals, k)
    idx, _ = match(fa, target_fpfh)
    ok = idx >= 0
    src, dst = points[ok], target[idx[ok]]
    ratio = rms_radius(target) / rms_radius(points)
    scale = (0.5 * ratio, 2.0 * ratio)
    origin, diagonal = register_ref.mesh_box(vertices, faces)
    inlier_dist = 0.03 * diagonal
    cand = ransac(src, dst, H, inlier_dist, seed, with_scale, scale, edge_tol, min_edge,
                  candidates)
    out = {"candidates": cand, "src": src, "dst": dst, "scale": scale,
           "inlier_dist": inlier_dist}
    if verify:
        rms = np.full(len(cand["h"]), np.inf)
        for c in range(len(rms)):
            rms[c] = trimmed_rms(points, vertices, faces, cand["s"][c], cand["R"][c],
                                 cand["t"][c], keep)
        best = int(np.argmin(rms))
        out.update(rms=rms, chosen=best,
                   coarse=(float(cand["s"][best]), cand["R"][best], cand["t"][best]))
    return out
