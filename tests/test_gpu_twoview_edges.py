"""The two-view kernels (twoview.hip) at their size boundaries and at hard geometry.

tests/test_gpu_twoview.py pins them to the reference's goldens on the Dino ring and one
sideways synthetic pair.  Here:

  * optimal triangulation (k_triangulate_optimal) against the exact answer of the reference's
    formulas (tests/golden/twoview_edges.npz, mpmath at 50 digits) for sideways and forward
    motion, nearly rectified cameras and a tiny baseline, in pixel and C-normalised units;
  * relative pose (k_relative_pose) on batches whose last workgroup is mostly padding quads,
    with every one of the four candidates winning somewhere, against the oracle pair by pair;
  * the LM gold standard (k_gold_standard) at every inlier count where its code changes path
    (one wave up to 64, 256 threads above; 1, 2, 3 points per thread; underdetermined below 8),
    against oracle/twoview_ref.gold_standard_lm at the end point and after exactly one step.

Bars: BASELINE.json's 1e-6 on triangulated points where the oracle itself is exact to 1e-11,
else ten times the oracle's own error; 1e-9 on closed forms, start costs and single steps.
"""
import numpy as np
import pytest

from conftest import golden
from oracle import ransac_ref
from oracle import twoview_ref as tvr
from tsbb15_amd import synth, twoview

pytestmark = pytest.mark.gpu
nF = ransac_ref.normalize_F

WELL = ("sideways", "forward")          # the oracle is exact to 1e-11: the 1e-6 bar applies
ILL = ("nearrect", "tiny")              # the reference's formulas are ill-conditioned
KINDS = ("px", "nm")


def _rel_err(X, ref):
    return np.abs(X - ref).max(axis=1) / np.abs(ref).max(axis=1)


def _cfg(z, name, kind):
    p = f"{name}_{kind}_"
    return z[p + "C1"], z[p + "C2"], z[p + "x1"], z[p + "x2"], z[p + "X"], z[p + "err_oracle"]


# ---- optimal triangulation -----------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", WELL)
def test_triangulate_exact_sideways_and_forward(ctx, name, kind):
    """257 points in one launch (two full 128-thread groups and one live lane), 1e-6 relative
    per point against the exact X."""
    C1, C2, x1, x2, X, _ = _cfg(golden("twoview_edges.npz"), name, kind)
    assert x1.shape == (2, 257)
    G = twoview.triangulate_optimal_batch(C1, C2, x1, x2)
    err = _rel_err(G, X)
    print(f"\n[{name}_{kind}] largest GPU error {err.max():.3g} (point {int(err.argmax())})")
    assert np.all(np.isfinite(G))
    assert err.max() < 1e-6, (err.max(), int(err.argmax()))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", ILL)
def test_triangulate_ill_conditioned_within_oracle_error(ctx, name, kind):
    """Nearly rectified cameras and a tiny baseline: the reference's formulation (f1 = f2 = 1,
    dehomogenised epipole) loses digits in float64 whoever evaluates it, so the GPU is held to
    ten times the numpy oracle's own error against the exact X (1e-6 where that is smaller).
    The factor is room for another root finder and null-vector method, not for a wrong root."""
    C1, C2, x1, x2, X, eo = _cfg(golden("twoview_edges.npz"), name, kind)
    assert x1.shape == (2, 65)
    G = twoview.triangulate_optimal_batch(C1, C2, x1, x2)
    err = _rel_err(G, X)
    ratio = err / eo
    print(f"\n[{name}_{kind}] largest GPU error {err.max():.3g}, oracle {eo.max():.3g}; "
          f"GPU / oracle per point: median {np.median(ratio):.3g}, largest {ratio.max():.3g}")
    assert np.all(np.isfinite(G))
    bound = np.maximum(1e-6, 10.0 * eo)
    bad = np.flatnonzero(~(err <= bound))
    assert bad.size == 0, (bad, err[bad], eo[bad])


def test_triangulate_mixed_launch_all_configurations(ctx):
    """All eight configurations in one call, a camera index per point and the points
    interleaved across configurations: bit for bit the per-configuration calls."""
    z = golden("twoview_edges.npz")
    cfgs = [_cfg(z, n, k) for n in WELL + ILL for k in KINDS]
    C1s = np.stack([c[0] for c in cfgs])
    C2s = np.stack([c[1] for c in cfgs])
    x1 = np.hstack([c[2] for c in cfgs])
    x2 = np.hstack([c[3] for c in cfgs])
    cam = np.concatenate([np.full(c[2].shape[1], i, np.int32) for i, c in enumerate(cfgs)])
    perm = np.random.RandomState(5).permutation(cam.size)
    assert cam.size == 4 * 257 + 4 * 65 and np.any(np.diff(cam[perm][:64]) != 0)
    G = twoview.triangulate_optimal_batch(C1s, C2s, np.ascontiguousarray(x1[:, perm]),
                                          np.ascontiguousarray(x2[:, perm]), cam=cam[perm])
    each = np.vstack([twoview.triangulate_optimal_batch(c[0], c[1], c[2], c[3]) for c in cfgs])
    np.testing.assert_array_equal(G, each[perm])


# ---- relative pose -------------------------------------------------------------------------
def _rodrigues(axis, ang):
    k = tvr.cross_matrix(axis / np.linalg.norm(axis))
    return np.eye(3) + np.sin(ang) * k + (1.0 - np.cos(ang)) * (k @ k)


def pose_batch(B, seed):
    """B pairs: a rotation of 0.05-0.6 rad about a random axis, a random unit t, one point at
    depth 3-8, E of that pose times a random scale in [0.1, 10] and a random sign.  The first
    correspondence rotates through four kinds: exact; the point mirrored behind both cameras;
    y2 displaced by sigma = 0.3; both displaced by 1e-3.  Returns E (B,3,3), y1, y2 (B,2)."""
    rs = np.random.RandomState(seed)
    E, y1, y2 = np.empty((B, 3, 3)), np.empty((B, 2)), np.empty((B, 2))
    for i in range(B):
        R = _rodrigues(rs.randn(3), rs.uniform(0.05, 0.6))
        t = rs.randn(3)
        t /= np.linalg.norm(t)
        X = np.array([rs.uniform(-1.0, 1.0), rs.uniform(-1.0, 1.0), rs.uniform(3.0, 8.0)])
        C2 = np.hstack([R, t.reshape(3, 1)])
        scale = rs.uniform(0.1, 10.0) * rs.choice([-1.0, 1.0])
        E[i] = tvr.fmatrix_from_cameras(tvr.I34, C2) * scale
        kind = i % 4
        if kind == 1:
            X = -X
        a = X[:2] / X[2]
        b = R @ X + t
        b = b[:2] / b[2]
        if kind == 2:
            b = b + rs.normal(0.0, 0.3, 2)
        elif kind == 3:
            a = a + rs.normal(0.0, 1e-3, 2)
            b = b + rs.normal(0.0, 1e-3, 2)
        y1[i], y2[i] = a, b
    return E, y1, y2


def oracle_pose_candidates(E, y1, y2):
    """tvr.relative_camera_pose's loop with its bookkeeping exposed: the 1-based index of the
    first passing candidate (0: none), how many pass and the smallest absolute depth seen."""
    U, _, VT = tvr.specSVD(E)
    V = VT.T
    W = np.array([[0., 1., 0.], [-1., 0., 0.], [0., 0., 1.]])
    Ra, Rb, v3 = V @ W @ U.T, V @ W.T @ U.T, V[:, -1]
    first, npass, dmin = 0, 0, np.inf
    for k, (R, t) in enumerate(((Ra, v3), (Rb, v3), (Ra, -v3), (Rb, -v3))):
        x1 = tvr.triangulate_optimal(tvr.I34, np.hstack([R, t.reshape(3, 1)]), y1, y2)
        x2 = R @ x1 + t
        dmin = min(dmin, abs(x1[-1]), abs(x2[-1]))
        if x1[-1] > 0 and x2[-1] > 0:
            npass += 1
            first = first or k + 1
    return first, npass, dmin


POSE_BATCHES = {33: 4, 97: 5}      # pairs: seed (33 pairs = 132 lanes: one live quad and 31
                                   # padding quads in the second workgroup)


@pytest.fixture(scope="module")
def pose_cases():
    out = {}
    for B, seed in POSE_BATCHES.items():
        E, y1, y2 = pose_batch(B, seed)
        ref = [tvr.relative_camera_pose(E[i], y1[i], y2[i]) for i in range(B)]
        cand = [oracle_pose_candidates(E[i], y1[i], y2[i]) for i in range(B)]
        out[B] = (E, y1, y2, ref, cand)
    return out


@pytest.mark.parametrize("B", sorted(POSE_BATCHES))
def test_relative_pose_every_candidate_wins_with_padding_quads(ctx, pose_cases, B):
    E, y1, y2, ref, cand = pose_cases[B]
    # the recipe decides: exactly one candidate passes in the oracle, away from zero depth,
    # and each of the four wins somewhere in the batch
    assert all(r is not None for r in ref)
    assert all(c[1] == 1 for c in cand), [c for c in cand if c[1] != 1]
    assert min(c[2] for c in cand) > 0.1
    hist_o = np.bincount([c[0] for c in cand], minlength=5)
    assert np.all(hist_o[1:] > 0) and hist_o[0] == 0, hist_o
    R, t, found = twoview.relative_camera_pose_batch(E, y1, y2)
    hist_g = np.bincount(found, minlength=5)
    print(f"\n[pose B={B}] found histogram (0..4): GPU {hist_g.tolist()}, oracle {hist_o.tolist()}")
    assert np.all(found > 0), np.flatnonzero(found <= 0)
    # poses, never indices: the candidate order follows the SVD's sign freedom
    np.testing.assert_allclose(R, np.array([r[0] for r in ref]), rtol=0, atol=1e-9)
    np.testing.assert_allclose(t, np.array([r[1] for r in ref]), rtol=0, atol=1e-9)
    assert np.all(hist_g[1:5] > 0) and hist_g[5:].sum() == 0, hist_g


def test_relative_pose_nan_pair_leaves_neighbours_alone(ctx, pose_cases):
    """An all-NaN E in the middle of a batch: found 0 and a NaN pose for that pair, every
    other pair bit for bit what it is in the batch without it."""
    E, y1, y2, _, _ = pose_cases[33]
    R0, t0, f0 = twoview.relative_camera_pose_batch(E, y1, y2)
    k = 16
    E1 = np.insert(E, k, np.full((3, 3), np.nan), axis=0)
    R1, t1, f1 = twoview.relative_camera_pose_batch(E1, np.insert(y1, k, y1[k], axis=0),
                                                    np.insert(y2, k, y2[k], axis=0))
    assert f1[k] == 0 and np.all(np.isnan(R1[k])) and np.all(np.isnan(t1[k]))
    keep = np.arange(34) != k
    np.testing.assert_array_equal(R1[keep], R0)
    np.testing.assert_array_equal(t1[keep], t0)
    np.testing.assert_array_equal(f1[keep], f0)


# ---- gold standard -------------------------------------------------------------------------
GS_SIZES = (1, 2, 5, 7, 8, 9, 63, 64, 65, 128, 255, 256, 257, 513, 700)
GS_ONE_STEP = (64, 65, 513)


@pytest.fixture(scope="module")
def gs_case():
    """700 noisy inliers of the synth scene, the true F perturbed by 1e-3 relative and put back
    to rank 2, and the oracle's LM from that start on the first n points, for every size."""
    p1, p2, _ = synth.two_view(700, 0.0, 21, sigma=0.5)
    K = synth.K_SYNTH
    Ft = tvr.fmatrix_from_cameras(K @ tvr.I34, K @ np.hstack([synth.rot_y(synth.ANGLE),
                                                              synth.T_SYNTH.reshape(3, 1)]))
    rs = np.random.RandomState(22)
    U, s, Vt = np.linalg.svd(Ft * (1.0 + 1e-3 * rs.randn(3, 3)))
    F0 = U @ np.diag([s[0], s[1], 0.0]) @ Vt
    oracle = {n: tvr.gold_standard_lm(F0, p1[:, :n], p2[:, :n]) for n in GS_SIZES}
    step = {n: tvr.gold_standard_lm(F0, p1[:, :n], p2[:, :n], max_iter=1) for n in GS_ONE_STEP}
    return p1, p2, F0, oracle, step


def _gs_batch(F0, p1, p2, ns, max_iter=twoview.MAX_ITER):
    off = np.concatenate([[0], np.cumsum(ns)]).astype(np.int64)
    pl = np.hstack([p1[:, :n] for n in ns] + [np.zeros((2, 0))])
    pr = np.hstack([p2[:, :n] for n in ns] + [np.zeros((2, 0))])
    return twoview.gold_standard_arrays(np.repeat(F0[None], len(ns), axis=0), pl, pr, off,
                                        max_iter=max_iter)


@pytest.fixture(scope="module")
def gs_gpu(ctx, gs_case):
    """Every size in one launch, in a shuffled order with two empty pairs among them."""
    p1, p2, F0, _, _ = gs_case
    ns = list(np.random.RandomState(23).permutation(GS_SIZES))
    ns.insert(4, 0)
    ns.insert(11, 0)
    F, C1, X, info = _gs_batch(F0, p1, p2, ns)
    return ns, F, C1, X, info


@pytest.mark.parametrize("n", GS_SIZES)
def test_gold_standard_every_size(ctx, gs_case, gs_gpu, n):
    p1, p2, F0, oracle, _ = gs_case
    ns, F, _, _, info = gs_gpu
    b = ns.index(n)
    a, c = p1[:, :n], p2[:, :n]
    Fo, io = oracle[n]
    g, Fg = info[b], F[b]
    assert io["status"] in (1, 2)          # the oracle converges at every size
    print(f"\n[gs n={n}] status {int(g['status'])} (oracle {io['status']}), iterations "
          f"{int(g['iterations'])} (oracle {io['iterations']}), cost {float(g['cost'])!r}, "
          f"cost - oracle cost {float(g['cost']) - io['cost']:.3g}, cost_init rel. diff "
          f"{abs(float(g['cost_init']) - io['cost_init']) / max(io['cost_init'], 1e-300):.3g}")
    assert int(g["n"]) == n
    assert np.all(np.isfinite(Fg))
    assert float(g["cost"]) <= float(g["cost_init"])
    assert float(g["cost_init"]) == pytest.approx(io["cost_init"], rel=1e-9, abs=1e-16)
    # one workgroup per pair: the batch's arithmetic is the single call's
    F1, _, _, i1 = _gs_batch(F0, p1, p2, [n])
    np.testing.assert_array_equal(F1[0], Fg)
    assert i1[0] == g
    if n >= 9:
        assert float(g["cost"]) <= io["cost"] * (1 + 1e-9)
        assert tvr.gs_objective(Fg, a, c) <= float(g["cost"]) * (1 + 1e-9)
        np.testing.assert_allclose(nF(Fg), nF(Fo), atol=1e-6)
    else:
        # the minimum is not unique (or nearly so): no end point to compare, but a rank-2 F
        # and a convergence exit (the ok / lam > 1e32 exits are what end the loop here)
        assert abs(np.linalg.det(Fg)) <= 1e-12 * np.linalg.norm(Fg) ** 3
        assert int(g["status"]) in (1, 2)


def test_gold_standard_empty_pairs_in_the_batch(ctx, gs_gpu):
    ns, F, _, _, info = gs_gpu
    for b in (i for i, n in enumerate(ns) if n == 0):
        assert int(info[b]["n"]) == 0 and float(info[b]["cost"]) == 0.0
        assert np.all(np.isfinite(F[b]))


@pytest.mark.parametrize("n", GS_ONE_STEP)
def test_gold_standard_one_step_matches_oracle(ctx, gs_case, n):
    """max_iter = 1: both stop after the first accepted step of the same damping schedule, so
    the Schur complement and the unrolled 12 x 12 Cholesky are compared before convergence can
    hide a wrong but still descending step."""
    p1, p2, F0, _, step = gs_case
    Fo, io = step[n]
    assert io["iterations"] == 1 and io["status"] == 0
    F, _, _, info = _gs_batch(F0, p1, p2, [n], max_iter=1)
    g = info[0]
    dF = np.abs(F[0] - Fo).max() / np.abs(Fo).max()
    print(f"\n[gs one step n={n}] cost_init {float(g['cost_init'])!r} (oracle "
          f"{io['cost_init']!r}), cost {float(g['cost'])!r} (oracle {io['cost']!r}), "
          f"|dF| / |F| {dF:.3g}")
    assert int(g["iterations"]) == 1 and int(g["status"]) == 0
    assert float(g["cost_init"]) == pytest.approx(io["cost_init"], rel=1e-9)
    assert float(g["cost"]) == pytest.approx(io["cost"], rel=1e-9)
    assert dF <= 1e-9, dF
