"""Bundle-adjustment problems for tests/test_gpu_ba*.py, built from committed data only
(tests/golden/dino_pnp_kat.npz: the Dino cameras R, t and points3d).  Test infrastructure.

The scene is moved into camera 0's frame (camera 0 = [I | 0], as the pipeline's first view).
Point j has a track of length 2 + j % (nC - 1) starting at view j % nC and wrapping around;
the observations are shuffled by a seeded permutation; uv is the exact projection (normalised
cameras, depths w ~ -1 in this data set) plus 1e-4 N(0, 1).  A start perturbs cameras 1.. and
the points by sigma N(0, 1).
"""
from __future__ import annotations

import numpy as np

from conftest import golden


def dino_scene(nC, nP):
    """(cams (nC, 3, 4), pts (nP, 3)) of the first nC views / nP points, in camera 0's frame."""
    z = golden("dino_pnp_kat.npz")
    R, t, X = z["R"][:nC], z["t"][:nC], z["points3d"][:nP]
    R0, t0 = R[0], t[0]
    cams = np.empty((nC, 3, 4))
    for k in range(nC):
        Rk = R[k] @ R0.T
        cams[k, :, :3] = Rk
        cams[k, :, 3] = t[k] - Rk @ t0
    cams[0] = np.hstack([np.eye(3), np.zeros((3, 1))])
    return cams, X @ R0.T + t0


def project(cams, pts, ov, op):
    xh = np.hstack([pts[op], np.ones((len(op), 1))])
    y = np.einsum('nij,nj->ni', cams[ov], xh)
    return y[:, :2] / y[:, 2:3]


def sparse_tracks(nC, nP):
    ov, op = [], []
    for j in range(nP):
        for s in range(2 + j % (nC - 1)):
            ov.append((j % nC + s) % nC)
            op.append(j)
    return np.array(ov, dtype=np.int32), np.array(op, dtype=np.int32)


def problem(nC, nP, seed=0, noise=1e-4, full=False):
    """dict(cams, pts: the true scene; ov, op, uv: the shuffled noisy observations)."""
    cams, pts = dino_scene(nC, nP)
    if full:
        ov = np.repeat(np.arange(nC, dtype=np.int32), nP)
        op = np.tile(np.arange(nP, dtype=np.int32), nC)
    else:
        ov, op = sparse_tracks(nC, nP)
    rng = np.random.RandomState(1000 + seed)
    perm = rng.permutation(len(ov))
    ov, op = ov[perm], op[perm]
    uv = project(cams, pts, ov, op) + noise * rng.standard_normal((len(ov), 2))
    return dict(cams=cams, pts=pts, ov=ov, op=op, uv=uv)


def start(prob, sigma, seed=0):
    """(cams0, pts0): cameras 1.. and the points perturbed by sigma N(0, 1)."""
    rng = np.random.RandomState(2000 + seed)
    cams0, pts0 = prob["cams"].copy(), prob["pts"].copy()
    cams0[1:] += sigma * rng.standard_normal(cams0[1:].shape)
    pts0 += sigma * rng.standard_normal(pts0.shape)
    return cams0, pts0
