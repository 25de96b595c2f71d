"""CPU numpy restatement of bundle adjustment under a robust loss (rs_bundle_adjust_robust of
ba.hip, the ``loss=`` / ``f_scale=`` keywords of tsbb15_amd.tables.bundle_adjust and
bundle_adjust_rigid), for both camera models.  Test infrastructure, the role ba_rigid_ref.py has
for the rigid adjustment.  The reference project reaches the same switch through
scipy.optimize.least_squares(loss=, f_scale=).

Objective.  Per observation i with the residual (ru, rv) of oracle.tables_ref.ba_residuals:
s_i = ru^2 + rv^2, z_i = s_i / C^2, C = f_scale, cost = 0.5 C^2 sum rho(z_i) with

    linear   rho = z                                   w = rho' = 1
    soft_l1  rho = 2 (sqrt(1 + z) - 1)                 w = 1 / sqrt(1 + z)
    huber    rho = z (z <= 1), 2 sqrt(z) - 1 (z > 1)   w = 1 (z <= 1), 1 / sqrt(z)
    cauchy   rho = log1p(z)                            w = 1 / (1 + z)

scipy's names and forms, but rho acts on the observation's squared norm, not on ru and rv
separately as scipy's does.

Iteration.  The LM of oracle.tables_ref.bundle_adjust_lm / ba_rigid_ref.bundle_adjust_rigid_lm,
rule for rule, on the re-weighted problem (IRLS, Triggs' first-order form: no rho'' term).  At
every linearisation w_i comes from the residuals of the accepted state; r, Jc and Jp of
observation i are scaled by sqrt(w_i); U, V, W, the gradients, the step and the predicted
reduction are the linear formulas in the scaled quantities.  The weights stay fixed over the
rejected trials of one linearisation; a trial's cost is the robust cost of the trial state.  A
singular point block or reduced system, or a non-finite step or cost, is a rejected trial, as a
non-positive pivot is on the GPU.  ``solver="schur"`` eliminates the points (ba_rigid_ref.
schur_step for the rigid model); ``solver="dense"`` solves the same damped normal equations
as one dense system.
"""
from __future__ import annotations

import numpy as np

import ba_rigid_ref as rr
from oracle import tables_ref as tr

LOSSES = ("linear", "soft_l1", "huber", "cauchy")


def rho(loss, z):
    z = np.asarray(z, dtype=np.float64)
    if loss == "linear":
        return z.copy()
    if loss == "soft_l1":
        return 2.0 * z / (np.sqrt(1.0 + z) + 1.0)
    if loss == "huber":
        return np.where(z <= 1.0, z, 2.0 * np.sqrt(z) - 1.0)
    if loss == "cauchy":
        return np.log1p(z)
    raise ValueError(loss)


def weight(loss, z):
    """rho'(z)."""
    z = np.asarray(z, dtype=np.float64)
    if loss == "linear":
        return np.ones_like(z)
    if loss == "soft_l1":
        return 1.0 / np.sqrt(1.0 + z)
    if loss == "huber":
        return np.where(z <= 1.0, 1.0, 1.0 / np.sqrt(np.maximum(z, 1.0)))
    if loss == "cauchy":
        return 1.0 / (1.0 + z)
    raise ValueError(loss)


def z_of(r, f_scale):
    rr2 = r.reshape(-1, 2)
    return (rr2[:, 0] ** 2 + rr2[:, 1] ** 2) / f_scale ** 2


def robust_cost(r, loss, f_scale):
    """(0.5 C^2 sum rho(z), w (n,)) of the interleaved residual vector r (2n,)."""
    z = z_of(r, f_scale)
    return 0.5 * f_scale ** 2 * float(rho(loss, z).sum()), weight(loss, z)


def jacobian(cams, pts, obs_view, obs_point, rigid):
    """(Jc (n, 2, D), Jp (n, 2, 3)): D = 6 of ba_rigid_ref, D = 12 of oracle.tables_ref."""
    if rigid:
        return rr.jacobian(cams, pts, obs_view, obs_point)
    return tr.ba_jacobian(cams, pts, obs_view, obs_point)


def retract(cams, dc, rigid):
    return rr.retract(cams, dc) if rigid else cams + dc.reshape(len(cams), 3, 4)


def scaled(Jc, Jp, r, w):
    """(Jc~, Jp~, r~) = sqrt(w) (Jc, Jp, r), observation by observation."""
    sq = np.sqrt(w)
    return Jc * sq[:, None, None], Jp * sq[:, None, None], r * np.repeat(sq, 2)


def normal_blocks(Jc, Jp, r, obs_view, obs_point, nC, nP):
    """ba_rigid_ref.normal_blocks for any camera block width."""
    D = Jc.shape[2]
    r2 = r.reshape(-1, 2)
    U, gc = np.zeros((nC, D, D)), np.zeros((nC, D))
    V, gp = np.zeros((nP, 3, 3)), np.zeros((nP, 3))
    np.add.at(U, obs_view, np.einsum('nki,nkj->nij', Jc, Jc))
    np.add.at(gc, obs_view, np.einsum('nki,nk->ni', Jc, r2))
    np.add.at(V, obs_point, np.einsum('nki,nkj->nij', Jp, Jp))
    np.add.at(gp, obs_point, np.einsum('nki,nk->ni', Jp, r2))
    return U, gc, V, gp, np.einsum('nki,nkj->nij', Jc, Jp)


def schur_step12(U, gc, V, gp, W, lam, obs_view, obs_point):
    """ba_rigid_ref.schur_step with 12-wide camera blocks."""
    nC, nP, D = len(U), len(V), 12
    free = rr.free_cameras(nC, obs_view)
    nf = len(free)
    pos = -np.ones(nC, dtype=np.int64)
    pos[free] = np.arange(nf)
    seen = np.bincount(obs_point, minlength=nP) > 0
    Vs = V + lam * np.einsum('pi,ij->pij', np.einsum('pii->pi', V), np.eye(3))
    Vi = np.zeros_like(V)
    Vi[seen] = np.linalg.inv(Vs[seen])
    S = np.zeros((nf, D, nf, D))
    rhs = np.zeros((nf, D))
    for k, c in enumerate(free):
        S[k, :, k, :] += U[c] + lam * np.diag(np.diag(U[c]))
        rhs[k] -= gc[c]
    order = np.argsort(obs_point, kind="stable")
    bounds = np.searchsorted(obs_point[order], np.arange(nP + 1))
    for p in range(nP):
        idx = [i for i in order[bounds[p]:bounds[p + 1]] if pos[obs_view[i]] >= 0]
        if not idx:
            continue
        Y = W[idx] @ Vi[p]
        blocks = np.einsum('aik,bjk->abij', Y, W[idx])
        for ai, i in enumerate(idx):
            rhs[pos[obs_view[i]]] += Y[ai] @ gp[p]
            for bi, j in enumerate(idx):
                S[pos[obs_view[i]], :, pos[obs_view[j]], :] -= blocks[ai, bi]
    dc = np.zeros((nC, D))
    if nf:
        dc[free] = np.linalg.solve(S.reshape(D * nf, D * nf), rhs.ravel()).reshape(nf, D)
    gx = gp.copy()
    np.add.at(gx, obs_point, np.einsum('nij,ni->nj', W, dc[obs_view]))
    return dc, -np.einsum('pij,pj->pi', Vi, gx)


def dense_step(Jc, Jp, r, lam, obs_view, obs_point, nC, nP):
    """ba_rigid_ref.dense_step for any camera block width."""
    D = Jc.shape[2]
    free = rr.free_cameras(nC, obs_view)
    nf = len(free)
    pos = -np.ones(nC, dtype=np.int64)
    pos[free] = np.arange(nf)
    seen = np.flatnonzero(np.bincount(obs_point, minlength=nP) > 0)
    ppos = -np.ones(nP, dtype=np.int64)
    ppos[seen] = np.arange(len(seen))
    J = np.zeros((2 * len(obs_view), D * nf + 3 * len(seen)))
    for i, (c, p) in enumerate(zip(obs_view, obs_point)):
        if pos[c] >= 0:
            J[2 * i:2 * i + 2, D * pos[c]:D * pos[c] + D] = Jc[i]
        J[2 * i:2 * i + 2, D * nf + 3 * ppos[p]:D * nf + 3 * ppos[p] + 3] = Jp[i]
    H = J.T @ J
    H += lam * np.diag(np.diag(H))
    d = np.linalg.solve(H, -(J.T @ r))
    dc, dx = np.zeros((nC, D)), np.zeros((nP, 3))
    dc[free] = d[:D * nf].reshape(nf, D)
    dx[seen] = d[D * nf:].reshape(-1, 3)
    return dc, dx


def bundle_adjust_robust_lm(cams, pts, obs_view, obs_point, u, v, loss="linear", f_scale=1.0,
                            rigid=False, max_iter=200, ftol=1e-15, solver="schur"):
    """Returns (cams, pts, info); info has the keys of tsbb15_amd.tables.bundle_adjust plus
    "weights", w_i (n,) at the returned state (ones for "linear")."""
    if loss not in LOSSES:
        raise ValueError(f"unknown loss {loss!r}")
    if not (np.isfinite(f_scale) and f_scale > 0):
        raise ValueError("f_scale must be finite and > 0")
    cams, pts = cams.copy(), pts.copy()
    obs_view = np.asarray(obs_view, dtype=np.int64)
    obs_point = np.asarray(obs_point, dtype=np.int64)
    nC, nP = len(cams), len(pts)
    lam, nu = 1e-3, 2.0

    def cost_of(cm, pt):
        with np.errstate(all='ignore'):
            r = tr.ba_residuals(cm, pt, obs_view, obs_point, u, v)
            cost, w = robust_cost(r, loss, f_scale)
        return cost, r, w

    cost, r, w = cost_of(cams, pts)
    cost0, it, rejected = cost, 0, 0

    def info(status):
        return dict(cost_init=cost0, cost=cost, iterations=it, status=status, rejected=rejected,
                    weights=w.copy(), **{"lambda": float(lam)})

    free = rr.free_cameras(nC, obs_view)
    for it in range(1, max_iter + 1):
        Jc, Jp = jacobian(cams, pts, obs_view, obs_point, rigid)
        Jc, Jp, rt = scaled(Jc, Jp, r, w)
        U, gc, V, gp, W = normal_blocks(Jc, Jp, rt, obs_view, obs_point, nC, nP)
        while True:
            try:
                with np.errstate(all='ignore'):
                    if solver == "dense":
                        dc, dx = dense_step(Jc, Jp, rt, lam, obs_view, obs_point, nC, nP)
                    elif rigid:
                        dc, dx = rr.schur_step(U, gc, V, gp, W, lam, obs_view, obs_point)
                    else:
                        dc, dx = schur_step12(U, gc, V, gp, W, lam, obs_view, obs_point)
                ok = bool(np.isfinite(dc).all() and np.isfinite(dx).all())
            except np.linalg.LinAlgError:
                ok = False
            if ok:
                dU, dV = np.einsum('cii->ci', U), np.einsum('pii->pi', V)
                pred = 0.5 * (lam * ((dc[free] * dU[free] * dc[free]).sum() + (dx * dV * dx).sum())
                              - (dc[free] * gc[free]).sum() - (dx * gp).sum())
                cams_n, pts_n = retract(cams, dc, rigid), pts + dx
                cost_n, r_n, w_n = cost_of(cams_n, pts_n)
            if ok and np.isfinite(cost_n) and cost_n < cost and pred > 0:
                gain = (cost - cost_n) / pred
                small = (cost - cost_n) <= ftol * cost
                cams, pts, cost, r, w = cams_n, pts_n, cost_n, r_n, w_n
                t = 2 * gain - 1
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
