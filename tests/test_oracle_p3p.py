"""The oracle's P3P restatement (oracle/pnp_ref.py p3p_lambda_twist, the n = 3 branch of
ransac.py:81-82) on the CPU: exact poses recovered from noise-free triples, the mirrored twins
put the three points behind the camera, and the RANSAC restatement finds the pose."""
import random

import numpy as np
import pytest

from oracle import pnp_ref


def _rot(w):
    th = np.linalg.norm(w)
    k = w / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K


def test_p3p_recovers_the_pose():
    rs = np.random.RandomState(0)
    found = 0
    for _ in range(200):
        R = _rot(rs.normal(0, 0.5, 3))
        t = np.array([rs.uniform(-1, 1), rs.uniform(-1, 1), rs.uniform(4, 9)])
        X = rs.uniform(-1.5, 1.5, (3, 3))
        Y = X @ R.T + t
        sols = pnp_ref.p3p_lambda_twist(X, pnp_ref.bearings(Y / Y[:, 2:]))
        assert len(sols) <= 8
        for Rs, ts, mirrored in sols:
            assert np.allclose(Rs @ Rs.T, np.eye(3), atol=1e-8) and np.linalg.det(Rs) > 0
            z = (X @ Rs.T + ts)[:, 2]
            assert np.all(z < 0) if mirrored else np.all(z > 0)
        err = min(np.abs(Rs - R).max() + np.abs(ts - t).max() for Rs, ts, m in sols if not m)
        found += err < 1e-8
    assert found >= 198, found


def test_ransac_p3p_restatement():
    rs = np.random.RandomState(2)
    R = _rot(np.array([0.1, 0.3, -0.2]))
    t = np.array([0.2, -0.1, 6.0])
    X = rs.uniform(-2, 2, (150, 3))
    Y = X @ R.T + t
    y = Y / Y[:, 2:]
    y[100:, :2] += rs.uniform(-0.2, 0.2, (50, 2))
    Rb, tb, im, ih, best, pose, counts = pnp_ref.ransac_pnp_p3p(
        y, X, y, X, 60, 1e-12, rng=random.Random(1), trace=True)
    assert best >= 0 and counts.max() == len(im) == 100
    assert np.array_equal(im, np.arange(100))
    np.testing.assert_allclose(Rb, R, atol=1e-8)


def test_consensus_arithmetic_emulation_equals_the_oracle():
    """tests/pnp_exact.errors_exact (the dgemm FMA chain, then pi / diff / dot in order) is the
    oracle's pose_errors bit for bit on the build container's BLAS: it is the truth the GPU
    consensus counts are checked against at the threshold (test_gpu_pnp.py)."""
    import pytest
    from conftest import trace_blas_matches
    from tsbb15_amd import synth
    import pnp_exact
    same, desc = trace_blas_matches()
    if not same:
        pytest.skip("numpy's dgemm order is the build container's: " + desc)
    X, _, y, R, t, _ = synth.pnp_scene(300, 0.3, seed=3)
    rs = np.random.RandomState(0)
    for _ in range(4):
        Rp, tp = R + rs.normal(0, 1e-3, (3, 3)), t + rs.normal(0, 1e-3, 3)
        e = pnp_exact.errors_exact(np.concatenate([Rp.ravel(), tp]), X, y)
        assert np.array_equal(e, pnp_ref.pose_errors(Rp, tp, X, y))


def _dist(R, t, Rr, tr):
    return max(np.abs(R - Rr).max(), np.abs(t - tr).max() / np.abs(tr).max())


def test_p3p_pose4_recovers_the_pose():
    """Three points solve, the fourth chooses: the exact pose on noise-free data, in front of
    the camera and (a negative-scale camera, every depth negated) behind it."""
    rs = np.random.RandomState(3)
    found = 0
    for trial in range(100):
        R = _rot(rs.normal(0, 0.5, 3))
        t = np.array([rs.uniform(-1, 1), rs.uniform(-1, 1), rs.uniform(4, 9)])
        X = rs.uniform(-1.5, 1.5, (4, 3))
        for tz in (t, t * np.array([1.0, 1.0, -1.0])):
            Y = X @ R.T + tz
            out = pnp_ref.p3p_pose4(X, Y / Y[:, 2:])
            found += out is not None and _dist(out[0], out[1], R, tz) < 1e-7 and out[2] < 1e-8
    assert found >= 196, found


def test_mirror_wins_rule():
    inf, nan = float("inf"), float("nan")
    assert pnp_ref.mirror_wins(0.9e-2, 1.0) and not pnp_ref.mirror_wins(1.1e-2, 1.0)
    assert pnp_ref.mirror_wins(5.0, inf) and not pnp_ref.mirror_wins(inf, inf)
    assert pnp_ref.mirror_wins(1.0, nan) and not pnp_ref.mirror_wins(nan, nan)
    assert not pnp_ref.mirror_wins(nan, 1.0)


def test_ransac_pnp_tuples_is_the_loop_with_given_samples():
    """ransac_pnp_tuples = ransac_pnp fed the same samples; ransac_pnp_p3p(tuples=) likewise."""
    from tsbb15_amd import synth
    X, _, y, _, _, _ = synth.pnp_scene(80, 0.2, seed=3, sigma=0.05)
    thr = (1.5 / 800.0) ** 2
    rng = random.Random(4)
    tup = np.array([pnp_ref.gen_rnd_indices(80, 6, rng) for _ in range(60)])
    tup[40] = tup[3]                        # a repeated tuple: scored once, counted twice
    a = pnp_ref.ransac_pnp(y[:50], X[:50], y, X, 60, thr, 6, rng=pnp_ref._PrefixRng(tup),
                           trace=True)
    b = pnp_ref.ransac_pnp_tuples(y[:50], X[:50], y, X, tup, thr)
    assert a[4] == b[4] >= 0 and np.array_equal(a[5], b[5])
    for u, v in zip(a[:4], b[:4]):
        assert np.array_equal(u, v)
    c = pnp_ref.ransac_pnp_p3p(y, X, y, X, 60, thr, rng=pnp_ref._PrefixRng(tup[:, :3]),
                               trace=True)
    d = pnp_ref.ransac_pnp_p3p(y, X, y, X, 60, thr, trace=True, tuples=tup[:, :3])
    assert c[4:6] == d[4:6] and np.array_equal(c[6], d[6])
    for u, v in zip(c[:4], d[:4]):
        assert np.array_equal(u, v)
    # nothing reaches the threshold: no winner
    e = pnp_ref.ransac_pnp_tuples(y, X, y, X, tup, 1e-30)
    assert e[4] == -1 and e[0] is None and not e[5].any()


@pytest.mark.parametrize("key", ["p3p_front", "p3p_dino", "p3p_dino_fine"])
def test_p3p_pose4_float64_run_reproduces_the_golden_floors(key):
    """The float64 restatement against the 50-digit poses recorded in
    tests/golden/pnp_minimal.npz (make_golden_pnp_minimal.py): at most 5 % of the samples are
    left out as ill-conditioned (floor above 1e-9) and the float64 run stays within the bar the
    recorded floors set for tests/test_gpu_pnp_edges.py.  (BAdino2's true poses are the
    mirrored-depth ones, but under 0.8 px of noise the mirrored candidate's fourth-point error
    is never below 1e-2 of its front-facing twin's: all 50 samples exercise the rule's "no"
    side; p3p_dino_fine, the same views under 0.01 px, has the mirrored pose win in 32 of 50.)"""
    from conftest import golden
    z = golden("pnp_minimal.npz")
    X, y, Rg, tg, floor = (z[f"{key}_{s}"] for s in ("X", "y", "R", "t", "floor"))
    keep = floor <= 1e-9
    assert 1.0 - keep.mean() <= 0.05
    bar = max(4.0 * floor[keep].max(), 16.0 * np.finfo(np.float64).eps)
    mirrored = 0
    for i in np.flatnonzero(keep):
        R, t, _ = pnp_ref.p3p_pose4(X[i], y[i])
        assert _dist(R, t, Rg[i], tg[i]) <= bar, (key, i)
        mirrored += bool(((X[i] @ R.T + t)[:3, 2] < 0).all())
    assert mirrored == (32 if key == "p3p_dino_fine" else 0)
