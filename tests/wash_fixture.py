"""Tables with known outliers for tests/test_wash_cpu.py and tests/test_gpu_wash.py, built on
ba_fixture.problem (noise 1e-4, scene scale ~ 1, tracks of 2 .. nC observations, shuffled).
Test infrastructure.

For j % 3 == 0 one randomly chosen observation of point j is displaced by 0.02 in a random
direction; for j % 3 == 1 with a track of >= 5 observations, two are.  The points start at
truth + 0.05 N(0, 1); the cameras are the true ones.  thresh = 1e-3 is 10 sigma.

``ring(nC)`` is the other extreme: three points seen by every one of nC cameras, for the longest
track (128) and the track lengths around the 64-lane wave (RING_EDGES).
"""
from __future__ import annotations

import numpy as np

import ba_fixture as bf

THRESH = 1e-3
DISPLACEMENT = 0.02
RING_EDGES = (63, 64, 65, 127)   # ring(nC): tracks on either side of the 64-lane wave, and 2 x 64 - 1


def table(nC, nP, seed, displaced=True):
    """dict(cams, pts (truth), pts0 (start), ov, op, uv, bad (n,) bool: displaced,
    track_len (n,): the length of each observation's track, thresh)."""
    P = bf.problem(nC, nP, seed)
    rng = np.random.RandomState(3000 + seed)
    ov, op, uv = P["ov"], P["op"], P["uv"].copy()
    bad = np.zeros(len(ov), bool)
    count = np.bincount(op, minlength=nP)
    for j in range(nP):
        tr = np.flatnonzero(op == j)
        k = 1 if j % 3 == 0 else (2 if j % 3 == 1 and len(tr) >= 5 else 0)
        pick = rng.choice(len(tr), k, replace=False)
        ang = rng.uniform(0.0, 2.0 * np.pi, k)
        if displaced:
            uv[tr[pick]] += DISPLACEMENT * np.stack([np.cos(ang), np.sin(ang)], axis=1)
            bad[tr[pick]] = True
    pts0 = P["pts"] + 0.05 * rng.standard_normal(P["pts"].shape)
    return dict(cams=P["cams"], pts=P["pts"], pts0=pts0, ov=ov, op=op, uv=uv, bad=bad,
                track_len=count[op], thresh=THRESH)


def ring(nC):
    """nC cameras on a wavy circle of radius 4 looking at the origin, 3 points near it seen by
    all of them, noise 1e-4, 5 observations of each point displaced by 0.02."""
    th = 2.0 * np.pi * np.arange(nC) / nC
    C = 4.0 * np.stack([np.cos(th), 0.3 * np.sin(3.0 * th), np.sin(th)], axis=1)
    z = -C / np.linalg.norm(C, axis=1, keepdims=True)
    x = np.cross([0.0, 1.0, 0.0], z)
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    y = np.cross(z, x)
    R = np.stack([x, y, z], axis=1)
    cams = np.concatenate([R, -np.einsum("kij,kj->ki", R, C)[:, :, None]], axis=2)
    pts = np.array([[0.3, 0.1, -0.2], [-0.25, 0.3, 0.15], [0.05, -0.35, 0.3]])
    rng = np.random.RandomState(77)
    perm = rng.permutation(3 * nC)
    ov = np.tile(np.arange(nC), 3)[perm].astype(np.int32)
    op = np.repeat(np.arange(3), nC)[perm].astype(np.int32)
    yh = np.einsum("nij,nj->ni", cams[ov], np.hstack([pts[op], np.ones((len(op), 1))]))
    uv = yh[:, :2] / yh[:, 2:3] + 1e-4 * rng.standard_normal((len(op), 2))
    bad = np.zeros(len(op), bool)
    for j in range(3):
        pick = rng.choice(np.flatnonzero(op == j), 5, replace=False)
        ang = rng.uniform(0.0, 2.0 * np.pi, 5)
        uv[pick] += 0.02 * np.stack([np.cos(ang), np.sin(ang)], axis=1)
        bad[pick] = True
    pts0 = pts + 0.05 * rng.standard_normal(pts.shape)
    return cams, pts, pts0, ov, op, uv, bad


def mini_tables(W):
    """A tables_fixture.MiniTables holding the table W (views, points at pts0, observations in
    order, image_coordinates = (u, v, 1))."""
    from tables_fixture import MiniTables, Pose
    T = MiniTables(np.eye(3))
    for k, c in enumerate(W["cams"]):
        T.addView(k, Pose(c[:, :3].copy(), c[:, 3].copy()))
    for p in W["pts0"]:
        T.addPoint(p.copy())
    for y, v, p in zip(W["uv"], W["ov"], W["op"]):
        T.addObs(np.array([y[0], y[1], 1.0]), int(v), int(p))
    return T


def check_table(T):
    """The bookkeeping invariants of a Tables object: every index points at the right object,
    every observations_index starts with the literal 0 and lists its own observations in
    ascending order, exactly once."""
    nO, nV, nP = len(T.T_obs), len(T.T_views), len(T.T_points)
    for o in T.T_obs:
        assert 0 <= o.view_index < nV and 0 <= o.point_3D_index < nP
    for kind, recs in (("view_index", T.T_views), ("point_3D_index", T.T_points)):
        seen = np.zeros(nO, int)
        for k, rec in enumerate(recs):
            idx = np.asarray(rec.observations_index)
            assert idx[0] == 0
            own = idx[1:]
            assert np.all(np.diff(own) > 0)
            assert np.all((own >= 0) & (own < nO))
            for i in own:
                assert getattr(T.T_obs[i], kind) == k
            seen[own] += 1
        assert np.all(seen == 1)
