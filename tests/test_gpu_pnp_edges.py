"""The PnP path at its size boundaries (pnp_kernels.hip, pnp_minimal.h) against the oracle.

  1  planted winners (tuple mode): pnp_select_block's int4 reads, its scalar tail of H mod 4
     counts, the 8 x 1024-quad stride and the "lowest index wins" rule across lanes, waves and
     strides, for the DLT branch and the P3P branch (8 models a trial);
  2  CPython-stream parity of ransac.ransac_pnp across the 512 / 1024 boundaries of
     pnp_inliers_block (one-pass fast path, chunked ordered_compact), with D_med and D_high of
     different sizes and sample sizes up to 16 (the streaming blk_add_point loop);
  3  the cv path: the K = 5 and K = 4 Philox samplers of k_pnp_solve_min replayed on the CPU,
     and k_pnp_inliers_px beyond one chunk of 1024 points;
  4  the minimal solvers p3p_pose and epnp_pose on noisy data against the restatements
     oracle/pnp_ref.p3p_pose4 and oracle/epnp_ref.epnp, with bars measured from the
     restatements' own fp64 error (tests/golden/pnp_minimal.npz, see the table below);
  5  k_pnp_lm's strided block reduction at point counts around kLmThreads = 256.

Section 4: bars and measured figures.  ``floor`` is the distance between the fp64 restatement and
the same restatement evaluated with mpmath at 50 digits (make_golden_pnp_minimal.py); a sample
whose floor exceeds 1e-9 is an ill-conditioned minimal sample and is left out (cap: 5 % per
solver); the bar is 4 x the largest remaining floor, at least 16 eps.  Distances are
max(max |dR|, max |dt| / max |t|).

  solver / samples            left out   largest floor   bar        largest GPU distance (MI355X)
  P3P front-facing, 200       0 (0 %)    5.94e-13        2.38e-12   5.21e-13
  P3P BAdino2 0.8 px, 50      0 (0 %)    2.02e-10        8.06e-10   3.06e-10
  P3P BAdino2 0.01 px, 50     0 (0 %)    3.33e-10        1.33e-09   1.47e-10
  EPnP m = 6, 40              0 (0 %)    1.42e-14        5.67e-14   1.00e-14
  EPnP m = 7, 40              0 (0 %)    1.13e-14        4.53e-14   1.49e-14   (5.95e-14 before)
  EPnP m = 64, 40             0 (0 %)    8.02e-15        3.21e-14   2.16e-15
  EPnP m = 65, 40             0 (0 %)    7.16e-15        2.86e-14   5.72e-15
  EPnP m = 257, 40            0 (0 %)    7.27e-15        2.91e-14   3.08e-15

"before": test_epnp_pose_equals_restatement_on_noisy_points[7] failed on one sample until
sym_jacobi (pnp_minimal.h) took one more sweep after its stop test first passes; the test is
relative to the whole diagonal and left the eigenvectors of the smallest eigenvalues, the ones
EPnP uses, short of converged (reproduced on the CPU by running the restatement with that stop
rule: 5.99e-14 on the same sample, 9.6e-15 with the further sweep).
"""
import ctypes as C
import functools
import random

import numpy as np
import pytest

import philox_ref as pr
from conftest import golden
from oracle import epnp_ref, pnp_ref
from tsbb15_amd import _ffi, cv, ransac, synth

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps


# ------------------------------------------------------------------------------------------
# 1. planted winners
# ------------------------------------------------------------------------------------------
THR_EXACT = (0.5 / 800.0) ** 2


def _ransac_tuples(ctx, Xm, ym, Xh, yh, k, tuples, thresh):
    """rs_pnp_ransac in tuple mode: everything it returns."""
    d, i64 = C.c_double, C.c_int64
    Xm, ym, Xh, yh = (_ffi.f64c(a) for a in (Xm, ym, Xh, yh))
    tuples = np.ascontiguousarray(tuples, dtype=np.int32)
    res = _ffi.PnpResult()
    im, ih = np.full(len(Xm), -1, np.int64), np.full(len(Xh), -1, np.int64)
    km, kh = i64(0), i64(0)
    _ffi.check(_ffi.lib().rs_pnp_ransac(
        ctx.handle, _ffi.ptr(Xm, d), _ffi.ptr(ym, d), len(Xm), _ffi.ptr(Xh, d), _ffi.ptr(yh, d),
        len(Xh), k, len(tuples), _ffi.SAMPLER_TUPLES, 0, _ffi.ptr(tuples, C.c_int32), thresh,
        C.byref(res), _ffi.ptr(im, i64), C.byref(km), _ffi.ptr(ih, i64), C.byref(kh)))
    return {"best_index": int(res.best_index), "count": int(res.best_count),
            "R": np.array(res.R[:]).reshape(3, 3), "t": np.array(res.t[:]),
            "inl_med": im[:km.value].copy(), "inl_high": ih[:kh.value].copy()}


@functools.lru_cache(maxsize=None)
def _exact_scene(m, k):
    """synth.pnp_scene(m, 0.3, seed=31, sigma=0): exact inliers, gross outliers.  Returns X, y,
    eight clean k-tuples and 40 k-tuples holding one outlier each."""
    X, _, y, _, _, inl = synth.pnp_scene(m, 0.3, seed=31, sigma=0.0)
    good, bad = np.flatnonzero(inl), np.flatnonzero(~inl)
    rs = np.random.RandomState(5)
    clean = np.array([rs.choice(good, k, replace=False) for _ in range(8)], np.int32)
    dirty = np.array([np.r_[rs.choice(good, k - 1, replace=False), bad[j]] for j in range(40)],
                     np.int32)
    for row in dirty:       # the outlier at a varying place of the tuple
        row[:] = np.roll(row, int(row[-1]) % k)
    return X, y, clean, dirty, int(inl.sum())


def _planted_tuples(dirty, clean, H, at):
    tup = dirty[np.arange(H) % len(dirty)].copy()
    for j, pos in enumerate(at):
        tup[pos] = clean[j]
    return tup


Q = 16  # H = 4 Q + 1, 2, 3 = 65, 66, 67
HS = 4 * (8192 + 3) + 3
PLANTED = [
    # (m, H, clean tuples at, the winner)
    pytest.param(513, 4 * Q + 1, (4 * Q,), 4 * Q, id="tail-only-H65"),
    pytest.param(513, 4 * Q + 2, (4 * Q + 1,), 4 * Q + 1, id="tail-only-H66"),
    pytest.param(513, 4 * Q + 3, (4 * Q + 2,), 4 * Q + 2, id="tail-only-H67"),
    pytest.param(513, 1, (0,), 0, id="tail-only-H1"),
    pytest.param(513, 2, (1,), 1, id="tail-only-H2"),
    pytest.param(513, 3, (2,), 2, id="tail-only-H3"),
    pytest.param(513, 4 * Q + 3, (4 * Q,), 4 * Q, id="tail-first"),
    pytest.param(513, 4 * Q + 3, (5, 4 * Q + 1), 5, id="tie-vector-tail"),
    pytest.param(1025, 4 * Q + 3, (4 * Q + 1, 5), 5, id="tie-vector-tail-m1025"),
    # quads 3 and 70: lanes of waves 0 and 1 of the 1024-thread block
    pytest.param(513, 4 * 80 + 3, (4 * 3 + 1, 4 * 70 + 2), 13, id="tie-waves"),
    pytest.param(513, 4 * 80 + 3, (4 * 70 + 2, 4 * 3 + 1), 13, id="tie-waves-swapped"),
    # quads 1024 + 3 (wave 0, second unrolled load) and 70 (wave 1): the lower index in the
    # higher wave
    pytest.param(513, 4 * 1100 + 3, (4 * 1027 + 1, 4 * 70 + 2), 282, id="tie-unroll"),
    # the outer loop's stride of 8 x 1024 quads: H = 4 (8192 + 3) + 3, so that quads 8193 and
    # 8194 (a thread's second trip) exist and three counts are left to the tail; and H = 32 771,
    # the largest H mod 4 = 3 that a single trip covers
    pytest.param(513, HS, (4 * 8192 + 5, 9), 9, id="tie-stride"),
    pytest.param(513, HS, (5, 4 * 8192 + 9), 5, id="tie-stride-reversed"),
    pytest.param(513, HS, (HS - 1, 4 * 8192 + 5), 4 * 8192 + 5, id="tie-stride-tail"),
    pytest.param(513, 32771, (32770,), 32770, id="tail-only-H32771"),
    pytest.param(513, 4 * Q + 3, (), -1, id="nothing-wins"),
    pytest.param(513, 2, (), -1, id="nothing-wins-H2"),
]


@pytest.mark.parametrize("m, H, at, winner", PLANTED)
def test_planted_winner_dlt(ctx, m, H, at, winner):
    """Every tuple holds an outlier (count 0 for the oracle) but those planted: the winner is
    the first of the largest counts, wherever pnp_select_block reads it.  The oracle counts
    every inlier for a clean tuple (359 of 513, 717 of 1025; largest inlier error 2e-27,
    smallest outlier error 2.9e-4, threshold 3.9e-7), so no count hangs on rounding."""
    X, y, clean, dirty, n_inl = _exact_scene(m, 6)
    tup = _planted_tuples(dirty, clean, H, at)
    Ro, to, imo, iho, besto, counts = pnp_ref.ransac_pnp_tuples(y, X, y, X, tup, THR_EXACT)
    assert besto == winner                       # the case is what its name says
    assert sorted(np.flatnonzero(counts)) == sorted(at) and (counts[list(at)] == n_inl).all()
    got = _ransac_tuples(ctx, X, y, X, y, 6, tup, THR_EXACT)
    assert got["best_index"] == besto
    if besto < 0:
        assert got["count"] == 0 and len(got["inl_med"]) == 0 and len(got["inl_high"]) == 0
        return
    assert got["count"] == counts[besto] == n_inl
    assert np.array_equal(got["inl_med"], imo) and np.array_equal(got["inl_high"], iho)
    np.testing.assert_allclose(got["R"], Ro, atol=1e-6)
    np.testing.assert_allclose(got["t"], to, rtol=1e-6, atol=1e-6)


@pytest.mark.parametrize("at, winner", [((4098,), 4098), ((4098, 7), 7)],
                         ids=["last-trial", "duplicate"])
def test_planted_winner_p3p(ctx, at, winner):
    """The P3P branch (k = 3, mirrored flags read as uchar4, 8 models a trial): r = 4099 trials,
    8 r = 32 792 > 4 x 8192 models, one clean triple at the last trial, or the same triple at
    trials 7 and r - 1 (7 wins).  For the oracle alone the clean triple's best pose counts
    all 359 inliers of the 513 points and no pose of the 40 contaminated triples counts more
    than 4, so the winner is planted, not found."""
    r = 4099
    X, y, clean, dirty, n_inl = _exact_scene(513, 3)
    tup = dirty[np.arange(r) % len(dirty)].copy()
    tup[list(at)] = clean[0]
    Ro, to, imo, iho, besto, poseo, counts = pnp_ref.ransac_pnp_p3p(
        y, X, y, X, r, THR_EXACT, trace=True, tuples=tup)
    assert besto == winner and counts[besto, poseo] == n_inl
    rest = np.delete(counts, list(at), axis=0)
    print(f"\nclean triple {n_inl}, contaminated triples at most {rest.max()}")
    assert rest.max() < n_inl
    got = _ransac_tuples(ctx, X, y, X, y, 3, tup, THR_EXACT)
    assert got["best_index"] == besto and got["count"] == n_inl
    assert np.array_equal(got["inl_med"], imo) and np.array_equal(got["inl_high"], iho)
    np.testing.assert_allclose(got["R"], Ro, atol=1e-9)
    np.testing.assert_allclose(got["t"], to, rtol=1e-9, atol=1e-9)


# ------------------------------------------------------------------------------------------
# 2. stream parity across the compaction boundaries, med != high, n up to 16
# ------------------------------------------------------------------------------------------
STREAM = [
    # m_med, m_high, n, r, (oracle winner, count, |inl_high|) where recorded, same arrays
    (512, 513, 6, 399, (28, 410, 410), False),
    (513, 513, 6, 401, (28, 410, 410), False),      # equal shapes, two distinct copies
    (1025, 700, 6, 403, (303, 820, 559), False),
    (300, 1025, 7, 402, (16, 242, 820), False),
    (2049, 600, 16, 203, (6, 1639, 463), False),
    (513, 512, 6, 397, None, False),
    (1024, 1024, 6, 400, None, True),               # the very same arrays: the `same` shortcut
    (1, 6, 6, 50, None, False),                     # a single med point
]


@pytest.mark.parametrize("m_med, m_high, n, r, figures, same", STREAM)
def test_stream_parity_across_compaction_boundaries(ctx, m_med, m_high, n, r, figures, same):
    """ransac.ransac_pnp = pnp_ref.ransac_pnp on random.Random(0)'s stream: winner, count, both
    consensus sets, pose, and the stream state after the call.  For the oracle the winner's
    errors keep a relative gap of at least 0.4 from the threshold in every case (0.7 in those
    with recorded figures; asserted below at 1e-6), so the sets do not hang on the last bits.
    In the (1, 6) case every sample is a permutation of D_high's six noisy points, whose DLT
    misses the single D_med point: nothing wins, on both sides."""
    X, _, y, *_ = synth.pnp_scene(max(m_med, m_high), 0.2, seed=3, sigma=0.05)
    thr = (1.5 / 800.0) ** 2
    Xm, ym = X[:m_med].copy(), y[:m_med].copy()
    Xh, yh = (Xm, ym) if same else (X[:m_high].copy(), y[:m_high].copy())
    rng_g, rng_o = random.Random(0), random.Random(0)
    Ro, to, imo, iho, besto, counts = pnp_ref.ransac_pnp(ym, Xm, yh, Xh, r, thr, n, rng=rng_o,
                                                         trace=True)
    R, t, im, ih, best, cnt = ransac.ransac_pnp(Xm, ym, Xh, yh, r, thr, n, rng=rng_g, ctx=ctx)
    assert rng_g.getstate() == rng_o.getstate()
    if besto < 0:
        assert (m_med, m_high) == (1, 6) and counts.max() == 0
        assert best == -1 and cnt == 0 and len(im) == 0 and len(ih) == 0
        return
    ties = int(np.count_nonzero(counts == counts.max()))
    e = np.concatenate([pnp_ref.pose_errors(Ro, to, Xm, ym), pnp_ref.pose_errors(Ro, to, Xh, yh)])
    gap = np.abs(e - thr).min() / thr
    print(f"\n({m_med}, {m_high}, n {n}, r {r}): winner {besto} count {counts.max()} ties {ties} "
          f"|inl_high| {len(iho)} gap {gap:.3g}")
    assert gap > 1e-6
    if figures is not None:
        assert (besto, int(counts.max()), len(iho)) == figures
    assert best == besto and cnt == counts.max()
    assert np.array_equal(im, imo) and np.array_equal(ih, iho)
    assert len(ih) == len(iho)
    np.testing.assert_allclose(R, Ro, atol=1e-6)
    np.testing.assert_allclose(t, to, rtol=1e-6, atol=1e-6)


# ------------------------------------------------------------------------------------------
# 3. the cv path
# ------------------------------------------------------------------------------------------
K_ANISO = np.array([[800.0, 0.5, 640.0], [0.0, 1200.0, 480.0], [0.0, 0.0, 1.0]])


def _cv_pose():
    R, _ = cv.Rodrigues(np.array([0.1, -0.2, 0.05]))
    return R, np.array([0.2, -0.1, 6.0])


@functools.lru_cache(maxsize=None)
def _noisy_cv_scene(seed=4):
    """1025 correspondences under the anisotropic, skewed camera: 820 with 0.5 px Gaussian
    noise, 205 gross outliers (>= 60 px)."""
    rs = np.random.RandomState(seed)
    R, t = _cv_pose()
    X = rs.uniform(-2, 2, (1025, 3))
    uv = cv.project_points(X, cv.Rodrigues(R)[0], t, K_ANISO)
    uv[:820] += rs.normal(0.0, 0.5, (820, 2))
    uv[820:] += rs.choice([-1, 1], (205, 2)) * rs.uniform(60, 200, (205, 2))
    return X, uv


def _pose_gap(a, b):
    if a is None or b is None:
        return np.inf
    return max(np.abs(a[0] - b[0]).max(), np.abs(a[1] - b[1]).max())


@pytest.mark.parametrize("guess", [False, True], ids=["no-guess", "wrong-guess"])
@pytest.mark.parametrize("flags", [cv.SOLVEPNP_EPNP, cv.SOLVEPNP_P3P, cv.SOLVEPNP_ITERATIVE],
                         ids=["EPNP", "P3P", "ITERATIVE"])
def test_cv_sampler_pin(ctx, flags, guess):
    """The winner of cv.solvePnPRansac is the minimal pose of the tuple floyd_sample<K> draws
    for its hypothesis number (K = 5: EPnP, also behind SOLVEPNP_ITERATIVE; K = 4: P3P),
    points in draw order; with an extrinsic guess hypothesis 0 is the guess and sample h still
    uses counter h.  The neighbouring hypotheses' tuples and the other K's tuple give poses
    more than 1e-3 away, so 1e-6 pins the tuple.  The replay solves with rs_pnp_minimal, the
    same epnp_pose / p3p_pose in another kernel.  (cv.solvePnPRansac never takes the
    six-point DLT kernel, so there is no K = 6 case on this path.)"""
    X, uv = _noisy_cv_scene()
    m = len(X)
    kw = {}
    if guess:
        R0, t0 = _cv_pose()
        kw = dict(rvec=-cv.Rodrigues(R0)[0], tvec=t0.reshape(3, 1) + 1.0, useExtrinsicGuess=True)
    ok, *_ = cv.solvePnPRansac(X, uv, K_ANISO, None, iterationsCount=300, confidence=1.0,
                               flags=flags, ctx=ctx, **kw)
    assert ok
    rr = dict(cv.last_ransac)
    assert rr["iterations"] == 300 + (1 if guess else 0)
    h = rr["best_index"]
    assert h >= (1 if guess else 0)
    Ks = 4 if flags == cv.SOLVEPNP_P3P else 5
    method = {4: _ffi.PNP_P3P, 5: _ffi.PNP_EPNP5}

    # the pixels normalised by the expressions rs_pnp_ransac_cv uses (K upper triangular,
    # K[2][2] = 1), so both sides solve from the same numbers: a 5-point EPnP has an exact
    # two-dimensional null space whose basis -- and with it the pose, at the noise level --
    # turns on the last bit of its input
    y1 = (uv[:, 1] - K_ANISO[1, 2]) / K_ANISO[1, 1]
    yn = np.column_stack([(uv[:, 0] - K_ANISO[0, 2] - K_ANISO[0, 1] * y1) / K_ANISO[0, 0], y1,
                          np.ones(m)])

    def pose(hyp, k):
        T = pr.floyd_tuple(cv.CV_RANSAC_SEED, hyp, m, k)[0]
        R, t, err = _minimal(ctx, X[T], yn[T], method[k])
        return (R, t) if np.isfinite(err) else None

    won = pose(h, Ks)
    assert won is not None
    others = {"h-1": pose(h - 1, Ks), "h+1": pose(h + 1, Ks), "other K": pose(h, 9 - Ks)}
    gaps = {k: _pose_gap(won, v) for k, v in others.items()}
    print(f"\nflags {flags} guess {guess}: h {h}, gaps to other tuples {gaps}")
    assert min(gaps.values()) > 1e-3, gaps
    np.testing.assert_allclose(rr["R"], won[0], atol=1e-6)
    np.testing.assert_allclose(rr["t"], won[1], rtol=1e-6, atol=1e-6)


@pytest.mark.parametrize("m", [1024, 1025, 2049])
def test_cv_pixel_consensus_beyond_one_chunk(ctx, m):
    """k_pnp_inliers_px's ordered_compact over more than one chunk of 1024 points: exact
    projections, a tenth moved 7 px along u (inliers at 8 px), a tenth 9 px along v (not), a
    fifth gross outliers (>= 60 px), interleaved over the whole index range."""
    rs = np.random.RandomState(m)
    R, t = _cv_pose()
    X = rs.uniform(-2, 2, (m, 3))
    uv = cv.project_points(X, cv.Rodrigues(R)[0], t, K_ANISO)
    kind = rs.permutation(m) % 10           # 0: +-7 px u, 1: +-9 px v, 2 and 3: gross
    sgn = rs.choice([-1.0, 1.0], m)
    uv[kind == 0, 0] += 7.0 * sgn[kind == 0]
    uv[kind == 1, 1] += 9.0 * sgn[kind == 1]
    gross = (kind == 2) | (kind == 3)
    uv[gross] += rs.choice([-1, 1], (gross.sum(), 2)) * rs.uniform(60, 200, (gross.sum(), 2))
    ok, rvec, tvec, inl = cv.solvePnPRansac(X, uv, K_ANISO, None, iterationsCount=300,
                                            confidence=1.0, flags=cv.SOLVEPNP_P3P, ctx=ctx)
    assert ok
    inl = inl[:, 0]
    rr = cv.last_ransac
    e = np.linalg.norm(cv.project_points(X, cv.Rodrigues(rr["R"])[0], rr["t"], K_ANISO) - uv,
                       axis=1)
    print(f"\nm {m}: {len(inl)} inliers, nearest error to 8 px: {np.abs(e - 8.0).min():.3g}")
    assert np.abs(e - 8.0).min() > 1e-6
    np.testing.assert_array_equal(inl, np.flatnonzero(e <= 8.0))
    assert (np.diff(inl) > 0).all()
    assert len(inl) >= int(0.6 * m) and inl.max() >= m - 10   # the set spans every chunk


# ------------------------------------------------------------------------------------------
# 4. minimal solvers against their restatements on noisy data
# ------------------------------------------------------------------------------------------
def _dist(R, t, Rr, tr):
    return max(np.abs(R - Rr).max(), np.abs(t - tr).max() / np.abs(tr).max())


def _minimal(ctx, X, y, method):
    """rs_pnp_minimal on C-normalised points: (R, t, err)."""
    d = C.c_double
    X, y = _ffi.f64c(X), _ffi.f64c(y)
    R, t, err = np.empty(9), np.empty(3), d(0.0)
    _ffi.check(_ffi.lib().rs_pnp_minimal(ctx.handle, _ffi.ptr(X, d), _ffi.ptr(y, d), len(X),
                                         int(method), _ffi.ptr(R, d), _ffi.ptr(t, d),
                                         C.byref(err)))
    return R.reshape(3, 3), t, err.value


def _against_golden(ctx, z, key, method, label, m=None):
    if m is None:
        X, y = z[f"{key}_X"], z[f"{key}_y"]
    else:                   # the first m points of each of the 40 sets
        X, y = z["epnp_X"][:, :m], z["epnp_y"][:, :m]
    Rg, tg, floor = (z[f"{key}_{s}"] for s in ("R", "t", "floor"))
    keep = floor <= 1e-9
    assert 1.0 - keep.mean() <= 0.05
    bar = max(4.0 * floor[keep].max(), 16.0 * EPS)
    worst, at = 0.0, -1
    for i in np.flatnonzero(keep):
        R, t, err = _minimal(ctx, X[i], y[i], method)
        assert np.isfinite(err), (label, i)
        dgpu = _dist(R, t, Rg[i], tg[i])
        if dgpu > worst:
            worst, at = dgpu, i
    print(f"\n{label}: {int(keep.sum())} of {len(keep)} samples, largest floor "
          f"{floor[keep].max():.3g}, bar {bar:.3g}, largest GPU distance {worst:.3g} (sample "
          f"{at}, its own floor {floor[at]:.3g})")
    assert worst <= bar, (label, worst, bar)


@pytest.mark.parametrize("key", ["p3p_front", "p3p_dino", "p3p_dino_fine"])
def test_p3p_pose_equals_restatement_on_noisy_samples(ctx, key):
    """p3p_pose (three points solve, the fourth chooses, kMirrorWins) = pnp_ref.p3p_pose4 in
    50-digit arithmetic, on 200 four-point samples of a positive-depth scene and 50 of BAdino2
    views (negative-scale cameras), 0.8 px noise.  Under that noise the mirrored candidate of a
    BAdino2 sample is never below 1e-2 of its front-facing twin, so all 50 take the rule's "no"
    side; p3p_dino_fine, 50 more under 0.01 px, has the mirrored pose win in 32."""
    _against_golden(ctx, golden("pnp_minimal.npz"), key, _ffi.PNP_P3P, key)


@pytest.mark.parametrize("m", [6, 7, 64, 65, 257])
def test_epnp_pose_equals_restatement_on_noisy_points(ctx, m):
    """epnp_pose over m noisy correspondences (k_pnp_minimal_all: solvePnP(EPNP) and the EPNP
    refinement of solvePnPRansac) = epnp_ref.epnp in 50-digit arithmetic, 40 point sets per m."""
    _against_golden(ctx, golden("pnp_minimal.npz"), f"epnp{m}", _ffi.PNP_EPNP5, f"EPnP m={m}",
                    m)


@pytest.mark.parametrize("m", [4, 5])
def test_epnp_pose_invariants_at_4_and_5_points(ctx, m):
    """With 4 or 5 points the 2m x 12 system has an exact null space of dimension 4 or 2; Jacobi
    and LAPACK return different bases of it and the linearisations depend on the basis, so pose
    parity is undefined.  What holds for any basis: R is a rotation (1e-12), the returned error
    is the mean reprojection error of the returned pose (1e-12 relative), and on positive-depth
    data the pose is front-facing."""
    z = golden("pnp_minimal.npz")
    X, y = z["epnp_X"][:, :m], z["epnp_y"][:, :m]
    for i in range(len(X)):
        R, t, err = _minimal(ctx, X[i], y[i], _ffi.PNP_EPNP5)
        assert np.isfinite(err), i
        np.testing.assert_allclose(R.T @ R, np.eye(3), atol=1e-12)
        assert abs(np.linalg.det(R) - 1.0) < 1e-12
        q = X[i] @ R.T + t
        assert (q[:, 2] > 0).all(), i
        e = np.mean(np.linalg.norm(q[:, :2] / q[:, 2:] - y[i][:, :2] / y[i][:, 2:], axis=1))
        assert err == pytest.approx(e, rel=1e-12), i


# ------------------------------------------------------------------------------------------
# 5. LM refinement at the block's edges
# ------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _lm_scene():
    rs = np.random.RandomState(17)
    R, t = _cv_pose()
    X = rs.uniform(-2, 2, (513, 3))
    rv = cv.Rodrigues(R)[0]
    uv = cv.project_points(X, rv, t, K_ANISO) + rs.normal(0.0, 1.0, (513, 2))
    r0 = rv + rs.normal(0.0, 0.02, (3, 1))
    t0 = t.reshape(3, 1) * (1.0 + rs.normal(0.0, 0.02, (3, 1)))
    return X, uv, r0, t0


@pytest.mark.parametrize("m", [6, 255, 256, 257, 513])
def test_refine_lm_at_block_edges(ctx, m):
    """k_pnp_lm (kLmThreads = 256 threads striding over the points) on the first m points of
    one noisy scene against scipy's MINPACK LM from the same perturbed start: cost to 1e-9
    relative, pose to 1e-6 (the bars of test_refine_lm_gpu_reaches_the_least_squares_pose).  A
    dropped or doubled point moves the minimum far beyond that."""
    from scipy.optimize import least_squares
    X, uv, r0, t0 = _lm_scene()
    X, uv = np.ascontiguousarray(X[:m]), np.ascontiguousarray(uv[:m])

    def res(x):
        return (cv.project_points(X, x[:3], x[3:], K_ANISO) - uv).ravel()

    x0 = np.concatenate((r0.ravel(), t0.ravel()))
    ref = least_squares(res, x0, method="lm", xtol=1e-15, ftol=1e-15, gtol=1e-15)
    rv, tv = cv._refine_lm(X, uv, K_ANISO, r0, t0, ctx)
    c_gpu = 0.5 * float(np.sum(res(np.concatenate((rv.ravel(), tv.ravel()))) ** 2))
    print(f"\nm {m}: cost {c_gpu:.12g} scipy {ref.cost:.12g}")
    assert c_gpu <= 0.5 * float(res(x0) @ res(x0))
    assert cv.last_lm["cost"] == pytest.approx(c_gpu, rel=1e-9)
    assert c_gpu == pytest.approx(ref.cost, rel=1e-9), (m, c_gpu, ref.cost)
    np.testing.assert_allclose(rv.ravel(), ref.x[:3], atol=1e-6)
    np.testing.assert_allclose(tv.ravel(), ref.x[3:], rtol=1e-6, atol=1e-6)
