"""Numpy restatement of the registration step (include/rsamd.h, rs_eval_index_step) on top of
tests/eval_ref.py's brute-force mesh distance, and of the loop tsbb15_amd.evaluation.register
drives with it.  Every product and sum is spelled out in the header's order; tau comes from a full
sort; the moments are summed in the header's order -- lane, fold by halving, blocks -- in fp64 or,
with ``dtype=np.longdouble``, in extended precision from the same fp64 points, which shows the
error the fp64 terms and their sum have.
"""
import numpy as np

import eval_ref

BLOCK = 2048          # RS_EVAL_REG_BLOCK
LANES = 256
SLOTS = 40            # RS_EVAL_REG_SLOTS
NS = {"point": 17, "plane": 37}
RMS_SLOT = {"point": 16, "plane": 35}


def transform(pts, s, R, t):
    """p'_r = s ((R_r0 x + R_r1 y) + R_r2 z) + t_r."""
    p = np.asarray(pts, dtype=np.float64)
    R, t = np.asarray(R, dtype=np.float64), np.asarray(t, dtype=np.float64)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    s = np.float64(s)
    with np.errstate(all='ignore'):
        return np.stack([s * ((R[r, 0] * x + R[r, 1] * y) + R[r, 2] * z) + t[r]
                         for r in range(3)], axis=1)


def trim_rank(keep, m):
    """k = ceil(keep m - 1e-9) clamped to 1..m; 0 for m = 0."""
    if m == 0:
        return 0
    k = np.ceil(np.float64(keep) * np.float64(m) - np.float64(1e-9))
    return int(min(max(k, 1.0), float(m)))


def terms(metric, moved, closest, d2, face, vertices, faces, origin, kept, dtype=np.float64):
    """(n, NS) the kept points' terms in the header's slots, +0.0 in the rows not kept."""
    with np.errstate(all='ignore'):
        p, q = (np.asarray(a, dtype=np.float64).astype(dtype).T for a in (moved, closest))
        o = np.asarray(origin, dtype=np.float64).astype(dtype)
        d = np.asarray(d2, dtype=np.float64).astype(dtype)
        x0, x1, x2 = p[0] - o[0], p[1] - o[1], p[2] - o[2]
        if metric == "point":
            y = [q[0] - o[0], q[1] - o[1], q[2] - o[2]]
            w = [x0, x1, x2] + y
            for i in range(3):
                w += [y[i] * x0, y[i] * x1, y[i] * x2]
            w += [(x0 * x0 + x1 * x1) + x2 * x2, d]
        else:
            f = np.asarray(faces).reshape(-1, 3)
            tri = np.asarray(vertices, dtype=np.float64).astype(dtype)[f[face]]   # -1: masked
            a, b, c = tri[:, 0].T, tri[:, 1].T, tri[:, 2].T
            u0, u1, u2 = b[0] - a[0], b[1] - a[1], b[2] - a[2]
            v0, v1, v2 = c[0] - a[0], c[1] - a[1], c[2] - a[2]
            N0, N1, N2 = u1 * v2 - u2 * v1, u2 * v0 - u0 * v2, u0 * v1 - u1 * v0
            ln = np.sqrt((N0 * N0 + N1 * N1) + N2 * N2)
            n0, n1, n2 = N0 / ln, N1 / ln, N2 / ln
            e0, e1, e2 = p[0] - q[0], p[1] - q[1], p[2] - q[2]
            r = (n0 * e0 + n1 * e1) + n2 * e2
            J = [x1 * n2 - x2 * n1, x2 * n0 - x0 * n2, x0 * n1 - x1 * n0, n0, n1, n2,
                 (x0 * n0 + x1 * n1) + x2 * n2]
            w = [J[i] * J[j] for i in range(7) for j in range(i, 7)]
            w += [J[i] * r for i in range(7)] + [r * r, d]
        w = np.stack(w, axis=1)
    return np.where(np.asarray(kept)[:, None], w, dtype(0.0))


def ordered_sum(w):
    """The header's order over the rows of w (n, ns): block i // BLOCK, lane (i % BLOCK) % LANES
    adds its rows in ascending index from +0.0, the lanes fold by halving, the blocks' partials
    are added in ascending order from +0.0."""
    n, ns = w.shape
    nb = (n + BLOCK - 1) // BLOCK
    pad = np.zeros((nb * BLOCK, ns), dtype=w.dtype)
    pad[:n] = w
    a = pad.reshape(nb, BLOCK // LANES, LANES, ns)
    lane = np.zeros((nb, LANES, ns), dtype=w.dtype)
    for j in range(BLOCK // LANES):
        lane = lane + a[:, j]
    h = LANES // 2
    while h > 0:
        lane = lane[:, :h] + lane[:, h:2 * h]
        h //= 2
    total = np.zeros(ns, dtype=w.dtype)
    for b in range(nb):
        total = total + lane[b, 0]
    return total


def step(pts, vertices, faces, s, R, t, origin, keep=1.0, max_dist=np.inf, metric="plane",
         dtype=np.float64):
    """One step: dict(matched, kept, k, tau, moments (SLOTS, dtype), scale (SLOTS) the sum of the
    terms' magnitudes, moved, d2, face, closest, mask).  The points, the query and tau are fp64
    whatever ``dtype``; the terms and their sum are in ``dtype``."""
    moved = transform(pts, s, R, t)
    d2, face, closest = eval_ref.mesh_distance(moved, vertices, faces, max_dist)
    matched = face >= 0
    m = int(matched.sum())
    k = trim_rank(keep, m)
    tau = float(np.sort(d2[matched])[k - 1]) if m else float('nan')
    with np.errstate(invalid='ignore'):
        mask = matched & (d2 <= tau)
    w = terms(metric, moved, closest, d2, face, vertices, faces, origin, mask, dtype)
    moments, scale = np.zeros(SLOTS, dtype=dtype), np.zeros(SLOTS)
    moments[:w.shape[1]] = ordered_sum(w)
    scale[:w.shape[1]] = np.abs(w).sum(axis=0).astype(np.float64)
    return {"matched": m, "kept": int(mask.sum()), "k": k, "tau": tau, "moments": moments,
            "scale": scale, "moved": moved, "d2": d2, "face": face, "closest": closest,
            "mask": mask}


def rodrigues(w):
    w = np.asarray(w, dtype=np.float64)
    th = float(np.sqrt((w * w).sum()))
    K = np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])
    if th < 1e-8:
        a, b = 1.0 - th * th / 6.0, 0.5 - th * th / 24.0
    else:
        a, b = np.sin(th) / th, (1.0 - np.cos(th)) / (th * th)
    return np.eye(3) + a * K + b * (K @ K)


def update(metric, moments, kept, origin, with_scale=True):
    """(ds, dR, dt) from a step's moments, about ``origin``."""
    mom = np.asarray(moments, dtype=np.float64)
    origin = np.asarray(origin, dtype=np.float64)
    if metric == "point":
        N = float(kept)
        mx, my = mom[0:3] / N, mom[3:6] / N
        cov = mom[6:15].reshape(3, 3) / N - np.outer(my, mx)
        var = mom[15] / N - float((mx * mx).sum())
        U, D, Vt = np.linalg.svd(cov)
        S = np.array([1.0, 1.0, 1.0 if np.linalg.det(U) * np.linalg.det(Vt) >= 0.0 else -1.0])
        dR = (U * S) @ Vt
        ds = float((D * S).sum() / var) if with_scale and var > 0.0 else 1.0
        u = my - ds * dR @ mx
    else:
        A = np.zeros((7, 7))
        A[np.triu_indices(7)] = mom[0:28]
        A = A + np.triu(A, 1).T
        m = 7 if with_scale else 6
        z = np.linalg.lstsq(A[:m, :m], -mom[28:28 + m], rcond=None)[0]
        dR, u = rodrigues(z[0:3]), z[3:6]
        ds = 1.0 + float(z[6]) if with_scale else 1.0
    return ds, dR, origin + u - ds * dR @ origin


def mesh_box(vertices, faces):
    tri = np.asarray(vertices)[np.asarray(faces).reshape(-1, 3)]
    tri = tri[np.isfinite(tri).all(axis=(1, 2))]
    lo, hi = tri.min(axis=(0, 1)), tri.max(axis=(0, 1))
    return (lo + hi) / 2.0, float(np.sqrt(((hi - lo) ** 2).sum()))


def register(pts, vertices, faces, metric="plane", keep=1.0, with_scale=True, init=None,
             max_dist=np.inf, max_iter=50, rtol=1e-6, atol=None):
    """evaluation.register's loop around ``step``.  Also returns ``transforms``, the (s, R, t)
    every step was evaluated under."""
    origin, diag = mesh_box(vertices, faces)
    atol = 1e-12 * diag if atol is None else atol
    s, R, t = (1.0, np.eye(3), np.zeros(3)) if init is None else init
    s, R, t = float(s), np.array(R, dtype=np.float64), np.array(t, dtype=np.float64)
    rms, kept, matched, tau, transforms = [], [], [], [], []
    converged = False
    for it in range(max_iter):
        rec = step(pts, vertices, faces, s, R, t, origin, keep, max_dist, metric)
        if rec["matched"] == 0:
            raise ValueError(f'step {it} matched no point')
        transforms.append((s, R, t))
        rms.append(float(np.sqrt(rec["moments"][RMS_SLOT[metric]] / rec["kept"])))
        kept.append(rec["kept"]), matched.append(rec["matched"]), tau.append(rec["tau"])
        if rms[-1] <= atol or (it > 0 and abs(rms[-2] - rms[-1]) <= rtol * rms[-2]):
            converged = True
            break
        if it == max_iter - 1:
            break
        ds, dR, dt = update(metric, rec["moments"], rec["kept"], origin, with_scale)
        s, R, t = ds * s, dR @ R, ds * dR @ t + dt
    return {"s": s, "R": R, "t": t, "iterations": len(rms), "converged": converged,
            "rms": np.array(rms), "kept": np.array(kept, dtype=np.int64),
            "matched": np.array(matched, dtype=np.int64), "tau": np.array(tau),
            "dist": np.sqrt(rec["d2"]), "mask": rec["mask"], "transforms": transforms}
