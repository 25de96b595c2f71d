"""Plain numpy restatement of the wash step (rs_wash_points / rs_triangulate_nview of wash.hip):
robust N-view re-triangulation of every point from its own track and removal of the
observations and points that do not fit.  Test infrastructure: the reference the GPU kernels
are compared with, written from the algorithm's description in include/rsamd.h.

Per point, with its track in ascending observation index and t2 = thresh^2:

  1. every pair a < b of the track in two different views gives a hypothesis X_ab: the
     inhomogeneous linear triangulation (rows (u c3 - c1).[X;1] = 0, (v c3 - c2).[X;1] = 0)
     through the 3x3 normal equations and Cholesky; a non-positive / NaN pivot or a non-finite
     X makes it invalid.  It is scored by (inliers over the track, sum of their e_i in track
     order), e_i = |uv_i - proj(X)|^2, inlier = e_i <= t2 and the sign of the depth as asked.
  2. the winner has >= 2 inliers and is best under (larger count, smaller sum, smaller pair
     ordinal); none: the point fails.
  3. twice: Levenberg-Marquardt on X over the inlier set (Marquardt damping, lam0 = 1e-3,
     Nielsen's update, <= 20 linearisations, stop at a gain <= 1e-15 cost or lam > 1e32), then
     the inlier set again; fewer than 2 inliers before a refit: the point fails.
  4. kept = not failed, X finite, >= min_views final inliers.
"""
from __future__ import annotations

import numpy as np

MAX_LIN = 20
LAM0 = 1e-3
FTOL = 1e-15
LAM_MAX = 1e32


def chol3_solve(N, g):
    """N (..., 6) symmetric as 00 01 02 11 12 22, g (..., 3) -> (X (..., 3), ok (...))."""
    N, g = np.asarray(N, dtype=np.float64), np.asarray(g, dtype=np.float64)
    a00, a01, a02, a11, a12, a22 = np.moveaxis(N, -1, 0)
    g0, g1, g2 = np.moveaxis(g, -1, 0)
    with np.errstate(all="ignore"):
        ok = a00 > 0.0
        l00 = np.sqrt(a00)
        l10, l20 = a01 / l00, a02 / l00
        d1 = a11 - l10 * l10
        ok = ok & (d1 > 0.0)
        l11 = np.sqrt(d1)
        l21 = (a12 - l20 * l10) / l11
        d2 = a22 - l20 * l20 - l21 * l21
        ok = ok & (d2 > 0.0)
        l22 = np.sqrt(d2)
        y0 = g0 / l00
        y1 = (g1 - l10 * y0) / l11
        y2 = (g2 - l20 * y0 - l21 * y1) / l22
        x2 = y2 / l22
        x1 = (y1 - l21 * x2) / l11
        x0 = (y0 - l10 * x1 - l20 * x2) / l00
    X = np.stack([x0, x1, x2], axis=-1)
    return X, ok & np.isfinite(X).all(axis=-1)


def rows(cams, uv):
    """The two linear equations of every observation: (m, 2, 4)."""
    return uv[:, :, None] * cams[:, None, 2, :] - cams[:, :2, :]


def normal_terms(R):
    """Rows R (..., 4) -> (N (..., 6), g (..., 3)) of one equation: A^T A and -A^T b."""
    A, b = R[..., :3], R[..., 3]
    N = np.stack([A[..., 0] * A[..., 0], A[..., 0] * A[..., 1], A[..., 0] * A[..., 2],
                  A[..., 1] * A[..., 1], A[..., 1] * A[..., 2], A[..., 2] * A[..., 2]], axis=-1)
    return N, -A * b[..., None]


def _ordered_sum(terms, axis):
    """Left-to-right sum along `axis` (np.sum adds pairwise)."""
    return np.take(np.cumsum(terms, axis=axis), -1, axis=axis)


def errors(cams, uv, X):
    """X (..., 3) against the whole track -> (e (..., m), w (..., m))."""
    with np.errstate(all="ignore"):
        y = np.einsum("mij,...j->...mi", cams[:, :, :3], X) + cams[:, :, 3]
        w = y[..., 2]
        ru = uv[:, 0] - y[..., 0] / w
        rv = uv[:, 1] - y[..., 1] / w
        return ru * ru + rv * rv, w


def inliers(e, w, t2, depth_sign):
    with np.errstate(invalid="ignore"):
        ok = e <= t2
        if depth_sign > 0:
            ok = ok & (w > 0.0)
        elif depth_sign < 0:
            ok = ok & (w < 0.0)
    return ok


def refit(cams, uv, X):
    """Levenberg-Marquardt on X over the given observations, from X."""
    def cost_of(Y):
        e, _ = errors(cams, uv, Y)
        return 0.5 * float(_ordered_sum(e, 0)) if len(e) else 0.0

    X = np.array(X, dtype=np.float64)
    cost = cost_of(X)
    lam, nu = LAM0, 2.0
    for _ in range(MAX_LIN):
        with np.errstate(all="ignore"):
            y = cams[:, :, :3] @ X + cams[:, :, 3]
            a, b, w = y[:, 0], y[:, 1], y[:, 2]
            r = np.stack([uv[:, 0] - a / w, uv[:, 1] - b / w], axis=1)
            iw2 = (1.0 / w) * (1.0 / w)
            j0 = -(cams[:, 0, :3] * w[:, None] - a[:, None] * cams[:, 2, :3]) * iw2[:, None]
            j1 = -(cams[:, 1, :3] * w[:, None] - b[:, None] * cams[:, 2, :3]) * iw2[:, None]
            V = np.stack([j0[:, 0] * j0[:, 0] + j1[:, 0] * j1[:, 0],
                          j0[:, 0] * j0[:, 1] + j1[:, 0] * j1[:, 1],
                          j0[:, 0] * j0[:, 2] + j1[:, 0] * j1[:, 2],
                          j0[:, 1] * j0[:, 1] + j1[:, 1] * j1[:, 1],
                          j0[:, 1] * j0[:, 2] + j1[:, 1] * j1[:, 2],
                          j0[:, 2] * j0[:, 2] + j1[:, 2] * j1[:, 2]], axis=1)
            V = _ordered_sum(V, 0)
            g = _ordered_sum(j0 * r[:, :1] + j1 * r[:, 1:], 0)
        dV = V[[0, 3, 5]]
        stop = False
        while True:
            Vd = V.copy()
            Vd[[0, 3, 5]] += lam * dV
            dx, ok = chol3_solve(Vd, -g)
            cost_n = cost_of(X + dx) if ok else np.nan
            pred = 0.5 * float(np.sum(lam * dx * dV * dx - dx * g)) if ok else 0.0
            if ok and np.isfinite(cost_n) and cost_n < cost and pred > 0.0:
                rho = (cost - cost_n) / pred
                small = (cost - cost_n) <= FTOL * cost
                X, cost = X + dx, cost_n
                t = 2.0 * rho - 1.0
                lam *= max(1.0 / 3.0, 1.0 - t * t * t)
                nu = 2.0
                stop = small
                break
            lam *= nu
            nu *= 2.0
            if lam > LAM_MAX:
                stop = True
                break
        if stop:
            break
    return X


def wash_track(cams, uv, views, thresh, min_views=2, depth_sign=0):
    """One point.  cams (m, 3, 4), uv (m, 2), views (m,) of its track, in track order.
    Returns dict(X or None, keep (m,) bool, err2 (m,), failed, kept, hypotheses)."""
    m = len(views)
    t2 = float(thresh) * float(thresh)
    out = dict(X=None, keep=np.zeros(m, bool), err2=np.full(m, np.nan), failed=True, kept=False,
               hypotheses=0)
    if m < 2:
        return out
    ia, ib = np.triu_indices(m, 1)            # a-major, b-minor
    use = views[ia] != views[ib]
    ia, ib = ia[use], ib[use]
    if len(ia) == 0:
        return out
    R = rows(cams, uv)                         # (m, 2, 4)
    Nt, gt = normal_terms(R)                   # (m, 2, 6), (m, 2, 3)
    N = ((Nt[ia, 0] + Nt[ia, 1]) + Nt[ib, 0]) + Nt[ib, 1]
    g = ((gt[ia, 0] + gt[ia, 1]) + gt[ib, 0]) + gt[ib, 1]
    Xh, ok = chol3_solve(N, g)
    out["hypotheses"] = int(ok.sum())
    e, w = errors(cams, uv, Xh)                # (P, m)
    inl = inliers(e, w, t2, depth_sign) & ok[:, None]
    cnt = inl.sum(axis=1)
    ssum = _ordered_sum(np.where(inl, e, 0.0), 1)
    cand = np.flatnonzero(cnt >= 2)
    if len(cand) == 0:
        return out
    best = cand[np.lexsort((cand, ssum[cand], -cnt[cand]))[0]]
    X = Xh[best]
    e, w = errors(cams, uv, X)
    S = inliers(e, w, t2, depth_sign)
    for _ in range(2):
        if S.sum() < 2:
            return out
        X = refit(cams[S], uv[S], X)
        e, w = errors(cams, uv, X)
        S = inliers(e, w, t2, depth_sign)
    out["failed"] = False
    out["err2"] = e
    out["X"] = X
    out["kept"] = bool(np.isfinite(X).all() and S.sum() >= min_views)
    if out["kept"]:
        out["keep"] = S
    return out


def _tracks(op, nP):
    order = np.argsort(op, kind="stable")
    cuts = np.searchsorted(op[order], np.arange(nP + 1))
    return [order[cuts[j]:cuts[j + 1]] for j in range(nP)]


def wash_points(cams, pts, obs_view, obs_point, uv, thresh, min_views=2, depth_sign=0):
    """-> (pts, obs_keep (bool), point_keep (bool), err2, info dict), as tables.wash_points."""
    cams = np.asarray(cams, dtype=np.float64).reshape(-1, 3, 4)
    pts = np.array(pts, dtype=np.float64).reshape(-1, 3)
    ov, op = np.asarray(obs_view), np.asarray(obs_point)
    uv = np.asarray(uv, dtype=np.float64).reshape(-1, 2)
    n, nP = len(ov), len(pts)
    obs_keep, point_keep = np.zeros(n, bool), np.zeros(nP, bool)
    err2 = np.full(n, np.nan)
    hyp = failed = 0
    for j, tr in enumerate(_tracks(op, nP)):
        r = wash_track(cams[ov[tr]], uv[tr], ov[tr], thresh, min_views, depth_sign)
        hyp += r["hypotheses"]
        failed += r["failed"]
        err2[tr] = r["err2"]
        if r["kept"]:
            point_keep[j] = True
            obs_keep[tr] = r["keep"]
            pts[j] = r["X"]
    info = dict(hypotheses=hyp, obs_removed=int(n - obs_keep.sum()),
                points_removed=int(nP - point_keep.sum()), points_failed=int(failed))
    return pts, obs_keep, point_keep, err2, info


def triangulate_nview(cams, pts, obs_view, obs_point, uv):
    """-> (pts, ok (bool)): every point from all its observations, no robustness."""
    cams = np.asarray(cams, dtype=np.float64).reshape(-1, 3, 4)
    pts = np.array(pts, dtype=np.float64).reshape(-1, 3)
    ov, op = np.asarray(obs_view), np.asarray(obs_point)
    uv = np.asarray(uv, dtype=np.float64).reshape(-1, 2)
    ok = np.zeros(len(pts), bool)
    for j, tr in enumerate(_tracks(op, len(pts))):
        if len(tr) < 2:
            continue
        c, y = cams[ov[tr]], uv[tr]
        Nt, gt = normal_terms(rows(c, y))
        N = _ordered_sum(Nt.reshape(-1, 6), 0)
        g = _ordered_sum(gt.reshape(-1, 3), 0)
        X, good = chol3_solve(N, g)
        if not good:
            continue
        X = refit(c, y, X)
        if np.isfinite(X).all():
            pts[j], ok[j] = X, True
    return pts, ok
