"""Rigid-camera bundle-adjustment problems for tests/test_ba_rigid_cpu.py and
tests/test_gpu_ba_rigid.py, built from tests/ba_fixture.py (committed data only).  Test
infrastructure.
"""
from __future__ import annotations

import numpy as np

import ba_fixture as bf
import ba_rigid_ref as rr


def rigid_start(prob, sigma, seed=0):
    """(cams0, pts0) of a ``ba_fixture.problem``: cameras 1.. moved to Exp(sigma n) R,
    t + sigma n, the points to X + sigma n, every n standard normal.  Every R stays a rotation."""
    rng = np.random.RandomState(3000 + seed)
    cams0, pts0 = prob["cams"].copy(), prob["pts"].copy()
    for k in range(1, len(cams0)):
        cams0[k, :, :3] = rr.exp_so3(sigma * rng.standard_normal(3)) @ cams0[k, :, :3]
        cams0[k, :, 3] += sigma * rng.standard_normal(3)
    pts0 += sigma * rng.standard_normal(pts0.shape)
    return cams0, pts0


def ring_problem(nC=42, nP=60, seed=0, noise=1e-4):
    """nC cameras on a closed curve around the first nP Dino points, each looking at their
    centroid (positive depths), the scene expressed in camera 0's frame; tracks are
    ``ba_fixture.sparse_tracks``, shuffled; uv is the exact projection plus noise N(0, 1).
    Same dict as ``ba_fixture.problem``."""
    _, X = bf.dino_scene(2, nP)
    ctr = X.mean(axis=0)
    rad = np.linalg.norm(X - ctr, axis=1).max()
    cams = np.empty((nC, 3, 4))
    for k in range(nC):
        phi = 2 * np.pi * k / nC
        pos = ctr + 3.3 * rad * np.array([np.cos(phi), np.sin(phi), 0.35 * np.sin(2 * phi)])
        z = (ctr - pos) / np.linalg.norm(ctr - pos)
        x = np.cross([0.0, 0.0, 1.0], z)
        x /= np.linalg.norm(x)
        R = np.stack([x, np.cross(z, x), z])
        cams[k, :, :3], cams[k, :, 3] = R, -R @ pos
    R0, t0 = cams[0, :, :3].copy(), cams[0, :, 3].copy()
    for k in range(nC):
        Rk = cams[k, :, :3] @ R0.T
        cams[k, :, 3] -= Rk @ t0
        cams[k, :, :3] = Rk
    cams[0] = np.hstack([np.eye(3), np.zeros((3, 1))])
    pts = X @ R0.T + t0
    ov, op = bf.sparse_tracks(nC, nP)
    rng = np.random.RandomState(4000 + seed)
    perm = rng.permutation(len(ov))
    ov, op = ov[perm], op[perm]
    uv = bf.project(cams, pts, ov, op) + noise * rng.standard_normal((len(ov), 2))
    return dict(cams=cams, pts=pts, ov=ov, op=op, uv=uv)


# The rings of tests/test_ba_shapes_cpu.py and tests/test_gpu_ba_large.py: cameras -> (points,
# observations).  nP >= nC - 1, so every track length 2 .. nC occurs.  Each camera count is the
# smallest that reaches a branch of k_ba_chol / k_ba_final (or the largest that stays below it);
# test_ba_shapes_cpu.py has the table.
LARGE_RINGS = {22: (40, 461), 23: (40, 464), 43: (60, 1134), 44: (60, 1159), 45: (60, 1186),
               88: (100, 4019), 128: (130, 8264)}
LARGE_FREE12 = (22, 23, 45, 88, 128)
LARGE_RIGID = (43, 44, 88, 128)
_rings = {}


def large_ring(nC):
    """``ring_problem(nC, LARGE_RINGS[nC][0])``, built once and read-only."""
    if nC not in _rings:
        P = ring_problem(nC, LARGE_RINGS[nC][0])
        for a in P.values():
            a.setflags(write=False)
        _rings[nC] = P
    return _rings[nC]


def short_track_ring(nC, keep=4):
    """``large_ring(nC)`` with every track cut to its first ``keep`` views (point j starts at
    view j % nC): a chain around the ring in which most pairs of cameras share no point, so most
    pair blocks of the reduced system are zero.  Every camera is still observed."""
    P = large_ring(nC)
    sel = (P["ov"].astype(np.int64) - P["op"] % nC) % nC < keep
    out = dict(cams=P["cams"], pts=P["pts"], ov=P["ov"][sel], op=P["op"][sel], uv=P["uv"][sel])
    for a in out.values():
        a.setflags(write=False)
    return out


def depths(prob):
    c = prob["cams"][prob["ov"]]
    return np.einsum('nj,nj->n', c[:, 2, :3], prob["pts"][prob["op"]]) + c[:, 2, 3]


def rotation_defect(cams):
    """max |R^T R - I| over the cameras."""
    R = cams[:, :, :3]
    return float(np.abs(np.einsum('kji,kjl->kil', R, R) - np.eye(3)).max())


def scale_fixed(cams, like):
    """cams with every t scaled so that |t_1| equals that of ``like`` (the one gauge freedom a
    rigid reconstruction with camera 0 fixed has left)."""
    out = cams.copy()
    out[:, :, 3] *= np.linalg.norm(like[1, :, 3]) / np.linalg.norm(cams[1, :, 3])
    return out


def pose_error(cams, truth):
    """(max |R - R_true|, max |t - t_true|) with the scale fixed by |t_1|."""
    c = scale_fixed(cams, truth)
    return (float(np.abs(c[:, :, :3] - truth[:, :, :3]).max()),
            float(np.abs(c[:, :, 3] - truth[:, :, 3]).max()))


def own_move(prob, sigma, rel=1e-13, seed=0):
    """How far the reference (ba_rigid_ref, Schur route, converged) moves when the start points
    are perturbed by ``rel`` relative: dict(cost: relative, R: max |dR|, t: max |dt| with the
    scale fixed by |t_1|, ref: the unperturbed (cams, pts, info)).  Input-level rounding of this
    size is what separates any two correct implementations of the same iteration."""
    ov, op, uv = prob["ov"], prob["op"], prob["uv"]
    c0, p0 = rigid_start(prob, sigma)
    rng = np.random.RandomState(5000 + seed)
    p0b = p0 * (1.0 + rel * rng.standard_normal(p0.shape))
    a = rr.bundle_adjust_rigid_lm(c0, p0, ov, op, uv[:, 0], uv[:, 1])
    b = rr.bundle_adjust_rigid_lm(c0, p0b, ov, op, uv[:, 0], uv[:, 1])
    ca, cb = scale_fixed(a[0], prob["cams"]), scale_fixed(b[0], prob["cams"])
    return dict(cost=abs(a[2]["cost"] - b[2]["cost"]) / a[2]["cost"],
                R=float(np.abs(ca[:, :, :3] - cb[:, :, :3]).max()),
                t=float(np.abs(ca[:, :, 3] - cb[:, :, 3]).max()), ref=a)
