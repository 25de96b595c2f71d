"""The five-point solver and E-RANSAC (essential.hip) at the sizes where their kernels change
shape, on bad and hard samples, and replayed sample by sample.

tests/test_gpu_essential.py pins the solver at two batch sizes and one geometry and E-RANSAC by
properties.  Here:

  * every batch size around the kernels' group sizes (64 lanes per workgroup in k_e5_build /
    k_e5_polys, two samples per wave in k_e5_gj, four 16-lane rows per wave and sixteen per
    workgroup in k_e5_roots): a sample's result may not depend on its wave-mates;
  * NaN, rank-deficient and coincident samples among good ones;
  * exact data at hard geometry against the oracle (oracle/essential_ref.py), the GPU held to
    max(1e-8, 10 x the oracle's own distance to the true E);
  * E-RANSAC replayed: the sampled indices are known on the CPU (tests/philox_ref.py), so the
    per-slot counts, c*, the candidates and the winner's consensus set are recomputed in numpy,
    also past the switch to the two-level scan (k_e5_bsum / k_e5_bscan) and with the winner in
    the last workgroup of samples;
  * the two-phase root finder (RSAMD_E5_SPLIT) in a child process against one phase.
"""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import philox_ref as pr
from oracle import essential_ref as er
from oracle import ransac_ref
from tsbb15_amd import essential, synth

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG_DIR = os.path.join(REPO, "tsbb15-3d-reconstruction-project_amd")
K = synth.K_SYNTH
KI = np.linalg.inv(K)

POOL, POOL_SEED = 257, 4
SIZES = (1, 2, 3, 4, 5, 15, 16, 17, 31, 32, 33, 63, 64, 65, 255, 256, 257)


def _normalise(p):
    return (KI @ np.vstack([p, np.ones(p.shape[1])])).T


@functools.lru_cache(maxsize=None)
def _pool():
    """257 noisy samples, made as test_gpu_essential.test_five_point_solution_sets_match_oracle
    makes its 120."""
    p1, p2, _ = synth.two_view(5 * POOL, 0.0, seed=POOL_SEED, sigma=0.7)
    return _normalise(p1).reshape(POOL, 5, 3), _normalise(p2).reshape(POOL, 5, 3)


@functools.lru_cache(maxsize=None)
def _pool_gpu():
    y1, y2 = _pool()
    return essential.five_point_batch(y1, y2)


def _e_dist(E, Et):
    """The metric of er.same_e: largest entry difference after scale and sign."""
    a, b = E / np.linalg.norm(E), Et / np.linalg.norm(Et)
    return min(np.abs(a - b).max(), np.abs(a + b).max())


# ------------------------------------------------------------------------------------------
# batch sizes
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", SIZES)
def test_five_point_every_batch_size(ctx, S):
    y1, y2 = _pool()
    Efull, nfull = _pool_gpu()
    E, ns = essential.five_point_batch(y1[:S], y2[:S])
    assert np.array_equal(ns, nfull[:S])
    assert E.tobytes() == Efull[:S].tobytes()


def test_five_point_pool_matches_oracle(ctx):
    """The rule of test_five_point_solution_sets_match_oracle on the 257-sample pool: solutions
    one for one at 1e-7, at most 7 of 257 samples (3 of 120, scaled) off.  Measured: the list
    printed below."""
    y1, y2 = _pool()
    E, ns = _pool_gpu()
    off, dist = [], []
    for s in range(POOL):
        ref = er.five_point(y1[s], y2[s])
        got = list(E[s, :ns[s]])
        assert np.isnan(E[s, ns[s]:]).all() and np.isfinite(E[s, :ns[s]]).all()
        if len(ref) != len(got):
            off.append(s)
            continue
        for r in ref:
            d = min(min(np.abs(r - g).max(), np.abs(r + g).max()) for g in got)
            dist.append(d)
            if d > 1e-7:
                off.append(s)
    dist = np.array(dist)
    print(f"\n{len(dist)} solutions, distance p50 {np.median(dist):.2e} max {dist.max():.2e}; "
          f"samples off: {sorted(set(off))}")
    assert len(set(off)) <= 7, sorted(set(off))
    assert np.median(dist) < 1e-10


# ------------------------------------------------------------------------------------------
# bad samples among good ones
# ------------------------------------------------------------------------------------------
def test_bad_samples_do_not_disturb_their_neighbours(ctx):
    y1, y2 = (a[:33].copy() for a in _pool())
    nan_s, rep_s, same_s = 5, 18, 32      # three different waves of k_e5_roots, the last row
    y1[nan_s, :, :2] = np.nan
    y2[nan_s, :, :2] = np.nan
    y1[rep_s, 4], y2[rep_s, 4] = y1[rep_s, 0], y2[rep_s, 0]     # rank 4
    y1[same_s], y2[same_s] = y1[same_s, 0], y2[same_s, 0]       # five identical points
    E, ns = essential.five_point_batch(y1, y2)
    for s in range(33):
        if s in (nan_s, rep_s, same_s):
            continue
        Es, n1 = essential.five_point_batch(y1[s:s + 1], y2[s:s + 1])
        assert n1[0] == ns[s] and Es[0].tobytes() == E[s].tobytes(), s
    assert ns[nan_s] == 0 and np.isnan(E[nan_s]).all()
    for s in (rep_s, same_s):
        finite = np.isfinite(E[s]).all(axis=(1, 2))
        assert (np.isnan(E[s]).all(axis=(1, 2)) | finite).all()
        assert ns[s] == finite.sum() and finite[:ns[s]].all()
        nrm = np.linalg.norm(E[s, finite].reshape(-1, 9), axis=1)
        print(f"\nsample {s}: {ns[s]} solutions, norms {nrm}")
        assert np.allclose(nrm, 1.0, atol=1e-12)


# ------------------------------------------------------------------------------------------
# hard geometry, exact data
# ------------------------------------------------------------------------------------------
def _rot(axis, a):
    axis = np.asarray(axis, float) / np.linalg.norm(axis)
    Kx = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(a) * Kx + (1 - np.cos(a)) * Kx @ Kx


GEOMETRIES = ("sideways", "forward", "rot170", "planar", "tiny_baseline", "deep")
GEO_SEED = {"sideways": 1, "forward": 2, "rot170": 3, "planar": 4, "tiny_baseline": 25, "deep": 6}


@functools.lru_cache(maxsize=None)
def _geometry(name):
    """64 exact five-point samples: (y1, y2 (64, 5, 3), true E).  x2 = R x1 + t."""
    rs = np.random.RandomState(GEO_SEED[name])
    n = 64 * 5
    X = np.column_stack([rs.uniform(-1, 1, n), rs.uniform(-1, 1, n), rs.uniform(4, 8, n)])
    R, t = synth.rot_y(synth.ANGLE), synth.T_SYNTH.copy()
    if name == "forward":                 # t along the optical axis: the epipole in the image
        R, t = _rot([0.2, 1.0, 0.1], 0.05), np.array([0.0, 0.0, 0.8])
    elif name == "rot170":                # the second camera looks back at the scene
        R, t = _rot([0.05, 1.0, 0.02], np.deg2rad(170.0)), np.array([0.5, 0.1, 12.0])
    elif name == "planar":
        X[:, 2] = 6.0 + 0.3 * X[:, 0] + 0.2 * X[:, 1]
    elif name == "tiny_baseline":
        # 1e-4 of the depth.  Every [t']_x R nearly fits such data, so the cubic constraints
        # tell the true t apart only at third order in the parallax: over the +-1 field of view
        # of the other sets the oracle itself is off by more than 1e-4 on 47 of 64 samples, under
        # any seed.  Over a narrow field of view (+-0.1 at depth 4-8) it stays within 1.6e-6 on
        # all 64 (median 1.6e-10)
        X[:, :2] *= 0.1
        R, t = _rot([1.0, 0.0, 0.0], 0.3), 6e-4 * np.array([1.0, 0.5, 0.7]) / np.sqrt(1.74)
    elif name == "deep":                  # depths 1 : 1000, the same field of view
        z = np.exp(rs.uniform(0.0, np.log(1000.0), n))
        X = np.column_stack([X[:, 0] / 6 * z, X[:, 1] / 6 * z, z])
    X2 = X @ R.T + t
    assert (X2[:, 2] > 0).all()
    y1 = (X / X[:, 2:]).reshape(64, 5, 3)
    y2 = (X2 / X2[:, 2:]).reshape(64, 5, 3)
    return y1, y2, er.e_from_cameras(np.eye(3), np.zeros(3), R, t)


def _quality(sols, y1, y2):
    """Largest epipolar residual and singular-value defects over a sample's solutions."""
    ep = sv01 = sv2 = 0.0
    for e in sols:
        ep = max(ep, np.abs(np.einsum("ia,ab,ib->i", y1, e, y2)).max())
        sv = np.linalg.svd(e, compute_uv=False)
        sv01, sv2 = max(sv01, abs(sv[0] - sv[1])), max(sv2, sv[2])
    return np.array([ep, sv01, sv2])


@functools.lru_cache(maxsize=None)
def _geometry_oracle(name):
    """Per sample: the oracle's distance to the true E (inf: no solution); and the oracle's worst
    (epipolar, s0 - s1, s2) over the geometry."""
    y1, y2, Et = _geometry(name)
    dist, worst = np.full(64, np.inf), np.zeros(3)
    for s in range(64):
        sols = er.five_point(y1[s], y2[s])
        if sols:
            dist[s] = min(_e_dist(e, Et) for e in sols)
            worst = np.maximum(worst, _quality(sols, y1[s], y2[s]))
    return dist, worst


@pytest.mark.parametrize("name", GEOMETRIES)
def test_five_point_hard_geometry(ctx, name):
    """Measured GPU / oracle figures: DESIGN.md 2.2, "Five-point edges"."""
    y1, y2, Et = _geometry(name)
    d_or, worst_or = _geometry_oracle(name)
    keep = d_or <= 1e-4
    assert (~keep).sum() <= 3, f"the oracle alone misses {(~keep).sum()} of 64 (cap 5 %)"
    E, ns = essential.five_point_batch(y1, y2)
    d_gpu, worst = np.full(64, np.inf), np.zeros(3)
    for s in range(64):
        sols = list(E[s, :ns[s]])
        assert np.isnan(E[s, ns[s]:]).all() and np.isfinite(E[s, :ns[s]]).all()
        if sols:
            d_gpu[s] = min(_e_dist(e, Et) for e in sols)
            worst = np.maximum(worst, _quality(sols, y1[s], y2[s]))
    bar = np.maximum(1e-8, 10.0 * d_or)
    ratio = d_gpu[keep] / np.maximum(d_or[keep], 1e-300)
    print(f"\n[{name}] kept {keep.sum()} of 64; distance to the true E: GPU max "
          f"{d_gpu[keep].max():.2e} oracle max {d_or[keep].max():.2e}; GPU / oracle p50 "
          f"{np.median(ratio):.2f} max {ratio.max():.2f}; epipolar, s0 - s1, s2: GPU "
          f"{worst[0]:.1e} {worst[1]:.1e} {worst[2]:.1e} oracle {worst_or[0]:.1e} "
          f"{worst_or[1]:.1e} {worst_or[2]:.1e}")
    bad = np.flatnonzero(keep & ~(d_gpu <= bar))
    assert len(bad) == 0, (bad, d_gpu[bad], d_or[bad])
    bars = np.maximum(np.array([1e-9, 1e-7, 1e-7]), 10.0 * worst_or)
    assert (worst <= bars).all(), (worst, bars)


# ------------------------------------------------------------------------------------------
# E-RANSAC replayed
# ------------------------------------------------------------------------------------------
def _distances(F, p1, p2):
    """ransac_ref.inlier_distance for a stack of models F (M, 3, 3): (M, n)."""
    x = np.vstack([p1, np.ones(p1.shape[1])])
    y = np.vstack([p2, np.ones(p2.shape[1])])
    l1 = F @ y
    l2 = F.transpose(0, 2, 1) @ x
    res1 = (l1 * x).sum(axis=1) / np.sqrt(l1[:, 0] ** 2 + l1[:, 1] ** 2)
    res2 = (l2 * y).sum(axis=1) / np.sqrt(l2[:, 0] ** 2 + l2[:, 1] ** 2)
    return np.maximum(np.abs(res1), np.abs(res2))


def _replay(p1, p2, seed, S, thresh, vectorised=False):
    """E-RANSAC sample by sample: the Philox five-point samples from the CPU restatement, their
    solutions by five_point_batch, F = K^-T E K^-1, the reference's distance per slot.  Returns
    (E (S, 10, 3, 3), d (S, 10, n) with NaN for empty slots, counts (S, 10))."""
    n = p1.shape[1]
    tup = pr.floyd_tuples(seed, 0, S, n, 5)
    y1, y2 = _normalise(p1), _normalise(p2)
    E, ns = essential.five_point_batch(y1[tup], y2[tup])
    real = np.arange(10)[None, :] < ns[:, None]
    F = KI.T @ E[real] @ KI
    d = np.full((S, 10, n), np.nan)
    if vectorised:
        d[real] = _distances(F, p1, p2)
    else:
        d[real] = np.array([ransac_ref.inlier_distance(f, p1, p2) for f in F]).reshape(-1, n)
    with np.errstate(invalid="ignore"):
        counts = (d < thresh).sum(axis=2)
    return E, d, counts


def _check_replay(r, E, d, counts, thresh):
    """ransac_e's result r against the replay; returns the winner's sample."""
    cstar = int(counts.max())
    assert cstar > 0
    # precondition: no decision that matters hangs on the last bits of a distance
    near = counts >= cstar - 1
    with np.errstate(invalid="ignore"):
        assert not (np.abs(d[near] - thresh) <= 1e-9 * thresh).any()
    cands = list(zip(*np.nonzero(counts == cstar)))
    norms = {c: np.linalg.norm(d[c]) for c in cands}
    won = (r.best_sample, r.best_solution)
    print(f"\nS {len(counts)}: c* {cstar}, candidates {cands[:8]}{'...' if len(cands) > 8 else ''}"
          f", winner {won}")
    assert r.count == cstar
    assert won in cands
    assert er.same_e(r.E, E[won], 1e-9), _e_dist(r.E, E[won])
    assert np.array_equal(r.inliers, np.flatnonzero(d[won] < thresh))
    # the smallest ||d|| wins, as far as 1e-9 relative tells the candidates apart
    assert norms[won] <= min(norms.values()) * (1 + 1e-9)
    return r.best_sample


ERANSAC_SEED = 3


@functools.lru_cache(maxsize=None)
def _eransac_points():
    return synth.two_view(120, 0.3, seed=6)[:2]


@pytest.mark.parametrize("S", [1, 16, 17, 300])
def test_ransac_e_replayed(ctx, S):
    p1, p2 = _eransac_points()
    r = essential.ransac_e(p1, p2, K, samples=S, seed=ERANSAC_SEED)
    _check_replay(r, *_replay(p1, p2, ERANSAC_SEED, S, 1.5), 1.5)


def test_ransac_e_replayed_float64_counting(ctx, monkeypatch):
    p1, p2 = _eransac_points()
    monkeypatch.setenv("RSAMD_E5_FP64", "1")
    r = essential.ransac_e(p1, p2, K, samples=300, seed=ERANSAC_SEED)
    monkeypatch.delenv("RSAMD_E5_FP64")
    _check_replay(r, *_replay(p1, p2, ERANSAC_SEED, 300, 1.5), 1.5)


S_SCAN = 128 * 256 + 1       # one sample past the inline reduction of k_e5_pack
SCAN_SEED = 5


def test_ransac_e_replayed_past_two_level_scan(ctx):
    p1, p2, _ = synth.two_view(60, 0.3, seed=8)
    r = essential.ransac_e(p1, p2, K, samples=S_SCAN, seed=SCAN_SEED)
    _check_replay(r, *_replay(p1, p2, SCAN_SEED, S_SCAN, 1.5, vectorised=True), 1.5)


# 9 exact correspondences among 51 random ones and a 0.05 px threshold: only a sample of five of
# the nine reaches c* = 9.  Under LAST_SEED the one such sample of the S_SCAN is the last
# (philox_ref.floyd_tuples; asserted below), alone in the last workgroup of k_e5_pack, whose
# base comes from the scanned workgroup sums.
LAST_SEED = 154205
LAST_INLIERS, LAST_THRESH = 9, 0.05


def _last_points():
    p1, p2, _ = synth.two_view(60, 0.0, seed=9, sigma=0.0)
    rs = np.random.RandomState(90)
    p2[0, LAST_INLIERS:] = rs.uniform(0.0, 640.0, 60 - LAST_INLIERS)
    p2[1, LAST_INLIERS:] = rs.uniform(0.0, 480.0, 60 - LAST_INLIERS)
    return p1, p2


def test_ransac_e_winner_in_last_workgroup(ctx):
    p1, p2 = _last_points()
    tup = pr.floyd_tuples(LAST_SEED, 0, S_SCAN, 60, 5)
    assert np.flatnonzero((tup < LAST_INLIERS).all(axis=1)).tolist() == [S_SCAN - 1]
    r = essential.ransac_e(p1, p2, K, samples=S_SCAN, seed=LAST_SEED, thresh=LAST_THRESH)
    E, d, counts = _replay(p1, p2, LAST_SEED, S_SCAN, LAST_THRESH, vectorised=True)
    assert _check_replay(r, E, d, counts, LAST_THRESH) == S_SCAN - 1
    assert r.count >= LAST_INLIERS


# ------------------------------------------------------------------------------------------
# two-phase root finder
# ------------------------------------------------------------------------------------------
_CHILD = """
import sys
import numpy as np
from tsbb15_amd import essential
z = np.load(sys.argv[1])
E, ns = essential.five_point_batch(z["y1"], z["y2"])
np.savez(sys.argv[2], E=E, ns=ns)
"""


@pytest.mark.parametrize("split", [6, 99])
def test_two_phase_root_finder_equals_one_phase(ctx, tmp_path, split):
    """RSAMD_E5_SPLIT is read once per process, so the two-phase run is a child process."""
    y1, y2 = _pool()
    Efull, nfull = _pool_gpu()
    np.savez(tmp_path / "in.npz", y1=y1, y2=y2)
    env = dict(os.environ, RSAMD_E5_SPLIT=str(split),
               PYTHONPATH=os.pathsep.join([REPO, PKG_DIR, os.environ.get("PYTHONPATH", "")]))
    subprocess.run([sys.executable, "-c", _CHILD, str(tmp_path / "in.npz"),
                    str(tmp_path / "out.npz")], env=env, check=True, timeout=120)
    z = np.load(tmp_path / "out.npz")
    assert np.array_equal(z["ns"], nfull)
    assert z["E"].tobytes() == Efull.tobytes()
