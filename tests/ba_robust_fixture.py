"""Bundle-adjustment problems with known outliers for tests/test_ba_robust_cpu.py and
tests/test_gpu_ba_robust.py: the problems of ba_fixture.py and ba_rigid_fixture.py made dirty by
the rule of wash_fixture.table.  Test infrastructure.

For j % 3 == 0 one randomly chosen observation of point j is displaced by 0.02 in a random
direction; for j % 3 == 1 with a track of >= 5 observations, two are.
"""
from __future__ import annotations

import numpy as np

import ba_fixture as bf
import ba_rigid_fixture as rf
import ba_robust_ref as br
import wash_fixture as wf

F_SCALE = 3e-4       # 3 sigma of the fixtures' noise (1e-4); a displaced observation has z ~ 4400
# the tables of wash_fixture.table (nC, nP, seed) on which the motive is pinned, and the bar on
# the Cauchy pose error there: 3 times the reference's worst (1.94e-2), 5 times below the best
# linear result (0.32); tests/test_ba_robust_cpu.py has the table
TABLES = [(4, 30, 0), (4, 30, 1), (6, 40, 0), (6, 40, 1), (7, 70, 0), (7, 70, 1)]
POSE_BAR = 0.06


def dirty(P, seed=0):
    """A copy of the problem dict P with displaced observations and ``bad`` (n,) bool."""
    rng = np.random.RandomState(6000 + seed)
    op, uv = P["op"], P["uv"].copy()
    bad = np.zeros(len(op), bool)
    for j in range(len(P["pts"])):
        tr = np.flatnonzero(op == j)
        k = 1 if j % 3 == 0 else (2 if j % 3 == 1 and len(tr) >= 5 else 0)
        pick = rng.choice(len(tr), k, replace=False)
        ang = rng.uniform(0.0, 2.0 * np.pi, k)
        uv[tr[pick]] += wf.DISPLACEMENT * np.stack([np.cos(ang), np.sin(ang)], axis=1)
        bad[tr[pick]] = True
    out = dict(P)
    out["uv"], out["bad"] = uv, bad
    return out


def dirty_problem(nC, nP, seed=0):
    return dirty(bf.problem(nC, nP, seed), seed)


def dirty_ring(nC=42, nP=60, seed=0):
    return dirty(rf.ring_problem(nC, nP, seed), seed)


def dirty_full(nC=3, nP=676, seed=0):
    """Fully visible: camera rows of nP observations, longer than a 256-observation LDS tile."""
    return dirty(bf.problem(nC, nP, seed, full=True), seed)


def start(P, sigma, rigid, seed=0):
    """The start of either model: rotations stay rotations for the rigid one."""
    return rf.rigid_start(P, sigma, seed) if rigid else bf.start(P, sigma, seed)


def own_move(prob, sigma, loss, f_scale=F_SCALE, rigid=True, rel=1e-13, seeds=(0, 1), **kw):
    """ba_rigid_fixture.own_move for ba_robust_ref: how far the reference moves when the start
    points are perturbed by ``rel`` relative: dict(cost: relative, R, t (scale fixed by |t_1|),
    weights: max |dw|, ref: the unperturbed (cams, pts, info)).  The move depends on which
    trials the last iterations accept (one draw may happen to follow the unperturbed run trial
    for trial and show 1e-13 where the next shows 1e-9), so it is the larger over two draws, as
    the rigid fixtures take the larger over their two starts."""
    ov, op, uv = prob["ov"], prob["op"], prob["uv"]
    c0, p0 = start(prob, sigma, rigid)
    run = lambda p: br.bundle_adjust_robust_lm(c0, p, ov, op, uv[:, 0], uv[:, 1], loss=loss,
                                               f_scale=f_scale, rigid=rigid, **kw)
    a = run(p0)
    ca = rf.scale_fixed(a[0], prob["cams"])
    out = dict(cost=0.0, R=0.0, t=0.0, weights=0.0, ref=a)
    for seed in seeds:
        rng = np.random.RandomState(5000 + seed)
        b = run(p0 * (1.0 + rel * rng.standard_normal(p0.shape)))
        cb = rf.scale_fixed(b[0], prob["cams"])
        out["cost"] = max(out["cost"], abs(a[2]["cost"] - b[2]["cost"]) / a[2]["cost"])
        out["R"] = max(out["R"], float(np.abs(ca[:, :, :3] - cb[:, :, :3]).max()))
        out["t"] = max(out["t"], float(np.abs(ca[:, :, 3] - cb[:, :, 3]).max()))
        out["weights"] = max(out["weights"],
                             float(np.abs(a[2]["weights"] - b[2]["weights"]).max()))
    return out
