"""CPU numpy restatement of the rigid-camera bundle adjustment (rs_bundle_adjust_rigid of ba.hip,
tsbb15_amd.tables.bundle_adjust_rigid).  Test infrastructure, the role tests/wash_ref.py has for
the wash step; the reference project has no such step (its BundleAdjustment2 frees all 12
entries of every camera, oracle/tables_ref.bundle_adjust_lm).

Objective: oracle.tables_ref.ba_residuals.  Camera k is [R | t], Xc = R X + t = (x, y, z),
a = x / z, b = y / z, iz = 1 / z, r = (u - a, v - b).  The local update delta = (omega, tau) acts
on the left: R+ = Exp(omega) R, t+ = Exp(omega) t + tau, so Xc+ = Exp(omega) Xc + tau and

    Jc = d r / d delta = -[[-ab, 1 + a^2, -b, iz, 0, -a iz], [-(1 + b^2), ab, a, 0, iz, -b iz]]
    Jp = d r / d X     = -iz [[1, 0, -a], [0, 1, -b]] R

The LM rules are those of oracle.tables_ref.bundle_adjust_lm: lam = 1e-3, nu = 2, Marquardt
diagonal damping, accept iff cost_new < cost and pred > 0, Nielsen's update, stop on ftol,
lam > 1e32 or max_iter.  The free cameras are cameras 1.. with an observation; points without
an observation stay out.  ``solver="schur"`` eliminates the points as the GPU does;
``solver="dense"`` solves the same damped normal equations as one dense system.
"""
from __future__ import annotations

import numpy as np

from oracle import tables_ref as tr


def hat(w):
    return np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])


def exp_so3(w):
    """I + A K + B K^2, A = sin th / th, B = (sin(th/2) / (th/2))^2 / 2; series below th^2 = 1e-12."""
    w = np.asarray(w, dtype=np.float64)
    t2 = float(w @ w)
    if t2 < 1e-12:
        A, B = 1.0 - t2 / 6.0, 0.5 - t2 / 24.0
    else:
        t = np.sqrt(t2)
        A = np.sin(t) / t
        B = 0.5 * (np.sin(0.5 * t) / (0.5 * t)) ** 2
    K = hat(w)
    return np.eye(3) + A * K + B * (K @ K)


def retract(cams, dc):
    """cams (nC, 3, 4), dc (nC, 6): [R | t] <- Exp(omega) [R | t] + [0 | tau]; a zero row of dc
    leaves its camera bit for bit."""
    out = cams.copy()
    for k in range(len(cams)):
        if not dc[k].any():
            continue
        out[k] = exp_so3(dc[k, :3]) @ cams[k]
        out[k, :, 3] += dc[k, 3:]
    return out


def jacobian(cams, pts, obs_view, obs_point):
    """Per observation Jc (n, 2, 6) at delta = 0 and Jp (n, 2, 3)."""
    c = cams[obs_view]
    Xc = np.einsum('nij,nj->ni', c[:, :, :3], pts[obs_point]) + c[:, :, 3]
    iz = 1.0 / Xc[:, 2]
    a, b = Xc[:, 0] * iz, Xc[:, 1] * iz
    z, o = np.zeros_like(a), np.ones_like(a)
    Jc = -np.stack([np.stack([-a * b, 1 + a * a, -b, iz, z, -a * iz], axis=1),
                    np.stack([-(1 + b * b), a * b, a, z, iz, -b * iz], axis=1)], axis=1)
    Pi = iz[:, None, None] * np.stack([np.stack([o, z, -a], axis=1),
                                       np.stack([z, o, -b], axis=1)], axis=1)
    Jp = -np.einsum('nij,njk->nik', Pi, c[:, :, :3])
    return Jc, Jp


def free_cameras(nC, obs_view):
    seen = np.bincount(obs_view, minlength=nC) > 0
    return np.array([k for k in range(1, nC) if seen[k]], dtype=np.int64)


def normal_blocks(Jc, Jp, r, obs_view, obs_point, nC, nP):
    rr = r.reshape(-1, 2)
    U, gc = np.zeros((nC, 6, 6)), np.zeros((nC, 6))
    V, gp = np.zeros((nP, 3, 3)), np.zeros((nP, 3))
    np.add.at(U, obs_view, np.einsum('nki,nkj->nij', Jc, Jc))
    np.add.at(gc, obs_view, np.einsum('nki,nk->ni', Jc, rr))
    np.add.at(V, obs_point, np.einsum('nki,nkj->nij', Jp, Jp))
    np.add.at(gp, obs_point, np.einsum('nki,nk->ni', Jp, rr))
    W = np.einsum('nki,nkj->nij', Jc, Jp)                 # (n, 6, 3)
    return U, gc, V, gp, W


def schur_step(U, gc, V, gp, W, lam, obs_view, obs_point):
    """(dc (nC, 6), dx (nP, 3)) of (H + lam diag H) delta = -g with the points eliminated."""
    nC, nP = len(U), len(V)
    free = free_cameras(nC, obs_view)
    nf = len(free)
    pos = -np.ones(nC, dtype=np.int64)
    pos[free] = np.arange(nf)
    seen = np.bincount(obs_point, minlength=nP) > 0
    Vs = V + lam * np.einsum('pi,ij->pij', np.einsum('pii->pi', V), np.eye(3))
    Vi = np.zeros_like(V)
    Vi[seen] = np.linalg.inv(Vs[seen])
    S = np.zeros((nf, 6, nf, 6))
    rhs = np.zeros((nf, 6))
    for k, c in enumerate(free):
        S[k, :, k, :] += U[c] + lam * np.diag(np.diag(U[c]))
        rhs[k] -= gc[c]
    order = np.argsort(obs_point, kind="stable")
    bounds = np.searchsorted(obs_point[order], np.arange(nP + 1))
    for p in range(nP):
        idx = [i for i in order[bounds[p]:bounds[p + 1]] if pos[obs_view[i]] >= 0]
        if not idx:
            continue
        Y = W[idx] @ Vi[p]                                # (m, 6, 3)
        blocks = np.einsum('aik,bjk->abij', Y, W[idx])
        for ai, i in enumerate(idx):
            rhs[pos[obs_view[i]]] += Y[ai] @ gp[p]
            for bi, j in enumerate(idx):
                S[pos[obs_view[i]], :, pos[obs_view[j]], :] -= blocks[ai, bi]
    dc = np.zeros((nC, 6))
    if nf:
        dc[free] = np.linalg.solve(S.reshape(6 * nf, 6 * nf), rhs.ravel()).reshape(nf, 6)
    gx = gp.copy()
    np.add.at(gx, obs_point, np.einsum('nij,ni->nj', W, dc[obs_view]))
    dx = -np.einsum('pij,pj->pi', Vi, gx)
    return dc, dx


def dense_step(Jc, Jp, r, lam, obs_view, obs_point, nC, nP):
    """The same damped normal equations through the dense (2n, 6 nf + 3 nP') Jacobian."""
    free = free_cameras(nC, obs_view)
    nf = len(free)
    pos = -np.ones(nC, dtype=np.int64)
    pos[free] = np.arange(nf)
    seen = np.flatnonzero(np.bincount(obs_point, minlength=nP) > 0)
    ppos = -np.ones(nP, dtype=np.int64)
    ppos[seen] = np.arange(len(seen))
    J = np.zeros((2 * len(obs_view), 6 * nf + 3 * len(seen)))
    for i, (c, p) in enumerate(zip(obs_view, obs_point)):
        if pos[c] >= 0:
            J[2 * i:2 * i + 2, 6 * pos[c]:6 * pos[c] + 6] = Jc[i]
        J[2 * i:2 * i + 2, 6 * nf + 3 * ppos[p]:6 * nf + 3 * ppos[p] + 3] = Jp[i]
    H = J.T @ J
    H += lam * np.diag(np.diag(H))
    d = np.linalg.solve(H, -(J.T @ r))
    dc, dx = np.zeros((nC, 6)), np.zeros((nP, 3))
    dc[free] = d[:6 * nf].reshape(nf, 6)
    dx[seen] = d[6 * nf:].reshape(-1, 3)
    return dc, dx


def bundle_adjust_rigid_lm(cams, pts, obs_view, obs_point, u, v, max_iter=200, ftol=1e-15,
                           solver="schur"):
    """Returns (cams, pts, info); info has the keys of tsbb15_amd.tables.bundle_adjust."""
    cams, pts = cams.copy(), pts.copy()
    obs_view = np.asarray(obs_view, dtype=np.int64)
    obs_point = np.asarray(obs_point, dtype=np.int64)
    nC, nP = len(cams), len(pts)
    lam, nu = 1e-3, 2.0

    def cost_of(cm, pt):
        r = tr.ba_residuals(cm, pt, obs_view, obs_point, u, v)
        return 0.5 * float(r @ r), r

    cost, r = cost_of(cams, pts)
    cost0, it, rejected = cost, 0, 0

    def info(status):
        return dict(cost_init=cost0, cost=cost, iterations=it, status=status, rejected=rejected,
                    **{"lambda": float(lam)})

    for it in range(1, max_iter + 1):
        Jc, Jp = jacobian(cams, pts, obs_view, obs_point)
        U, gc, V, gp, W = normal_blocks(Jc, Jp, r, obs_view, obs_point, nC, nP)
        free = free_cameras(nC, obs_view)
        while True:
            if solver == "schur":
                dc, dx = schur_step(U, gc, V, gp, W, lam, obs_view, obs_point)
            else:
                dc, dx = dense_step(Jc, Jp, r, lam, obs_view, obs_point, nC, nP)
            dU, dV = np.einsum('cii->ci', U), np.einsum('pii->pi', V)
            pred = 0.5 * (lam * ((dc[free] * dU[free] * dc[free]).sum() + (dx * dV * dx).sum())
                          - (dc[free] * gc[free]).sum() - (dx * gp).sum())
            cams_n, pts_n = retract(cams, dc), pts + dx
            cost_n, r_n = cost_of(cams_n, pts_n)
            if np.isfinite(cost_n) and cost_n < cost and pred > 0:
                rho = (cost - cost_n) / pred
                small = (cost - cost_n) <= ftol * cost
                cams, pts, cost, r = cams_n, pts_n, cost_n, r_n
                t = 2 * rho - 1
                lam *= max(1 / 3, 1 - t ** 3)
                nu = 2.0
                if small:
                    return cams, pts, info(1)
                break
            rejected += 1
            lam *= nu
            nu *= 2
            if lam > 1e32:
                return cams, pts, info(2)
    return cams, pts, info(0)
