"""The device sampler (device_math.h: philox4x32_10, floyd_sample<K>) against its CPU restatement
(tests/philox_ref.py), through every entry point that has both a Philox and a tuple mode.

The sampled indices cannot be read back, but the code after them is the same in both modes: a
Philox-mode call and the tuple-mode call fed with philox_ref.floyd_tuples must return the same
bytes.  A wrong round constant, a dropped high word of the hypothesis number or of the seed, a
slip in Lemire's rejection loop, in the block refill or in Floyd's duplicate rule changes the
tuples and with them the models."""
import ctypes as C

import numpy as np
import pytest

import philox_ref as pr
from tsbb15_amd import _ffi, pairs, synth

pytestmark = pytest.mark.gpu

HIGH_SEED = 0x9E3779B97F4A7C15


# ------------------------------------------------------------------------------------------
# F plan
# ------------------------------------------------------------------------------------------
def _plan_outputs(plan, H):
    r, inl = plan.result()
    return {"result": bytes(r), "inliers": inl.tobytes(), "models": plan.models(H).tobytes(),
            "counts": plan.counts(H).tobytes(),
            "candidates": [bytes(c) for c in plan.candidates()]}, r


def _plan_both_modes(plan, n, H, seed, off):
    plan.run(H, mode=_ffi.SAMPLER_PHILOX, seed=seed, hyp_offset=off)
    got, r = _plan_outputs(plan, H)
    tup = pr.floyd_tuples(seed, off, H, n, 8)
    plan.run(H, mode=_ffi.SAMPLER_TUPLES, tuples=tup)
    want, _ = _plan_outputs(plan, H)
    for key in want:
        assert got[key] == want[key], (key, n, H, seed, off)
    return r


@pytest.mark.parametrize("n, H, seed, off", [
    (8, 1, 0, 0),
    (9, 63, 1234, 1),
    (37, 65, HIGH_SEED, 2**32 - 3),      # crosses into the high counter word
    (257, 64, 1234, 2**40 + 7),
    (2000, 4097, HIGH_SEED, 0),
    (2000, 65, 0, 2**40 + 7),
    (37, 4097, 0, 1),
])
def test_f_plan_philox_equals_tuple_mode(ctx, n, H, seed, off):
    p1, p2, _ = synth.two_view(n, 0.3, seed=n)
    plan = _ffi.F8Plan(ctx, n, H)
    plan.set_points(p1, p2)
    r = _plan_both_modes(plan, n, H, seed, off)
    print(f"\nn {n} H {H}: best {r.best_index} count {r.best_count} candidates {r.n_candidates}")
    if n >= 37:
        assert r.best_index >= 0 and r.best_count >= 8
    plan.close()


@pytest.mark.parametrize("n, hs", [(pr.REJECT_N, pr.REJECT_H), (pr.EDGE_N, pr.EDGE_H8)])
def test_f_plan_rejected_and_threshold_draws(ctx, n, hs):
    """Windows of 64 hypotheses around those that reject a bounded draw (a ninth word: the
    second refill) and around those whose last draw sits exactly on Lemire's threshold."""
    p1, p2, _ = synth.two_view(n, 0.3, seed=3)
    plan = _ffi.F8Plan(ctx, n, 64)
    plan.set_points(p1, p2)
    for h in hs:
        _plan_both_modes(plan, n, 64, pr.REJECT_SEED, h - 32)
    plan.close()


# ------------------------------------------------------------------------------------------
# pairs
# ------------------------------------------------------------------------------------------
def _pair_bytes(r):
    return (r.F.tobytes(), r.inliers.tobytes(), r.best_index, r.count,
            np.array([r.std, r.norm]).tobytes(), r.n_candidates)


@pytest.mark.parametrize("ids", [None, [5, 0, 2**33]])
def test_pairs_philox_equals_tuple_mode(ctx, ids):
    ns, H, seed_base = (8, 37, 130), 65, 1000
    prs = [synth.two_view(n, 0.3, seed=40 + n)[:2] for n in ns]
    got = pairs.ransac_pairs(prs, H, ids=ids, ctx=ctx)
    streams = ids if ids is not None else range(len(ns))
    tup = np.stack([pr.floyd_tuples(seed_base + s, 0, H, n, 8) for s, n in zip(streams, ns)])
    want = pairs.ransac_pairs(prs, H, tuples=tup, ctx=ctx)
    for b, (g, w) in enumerate(zip(got, want)):
        print(f"\npair {b}: best {g.best_index} count {g.count}")
        assert _pair_bytes(g) == _pair_bytes(w), b
    assert got[1].best_index >= 0 and got[2].best_index >= 0


# ------------------------------------------------------------------------------------------
# PnP
# ------------------------------------------------------------------------------------------
def _pnp(ctx, X, y, k, H, thresh, mode, seed=0, tuples=None):
    """rs_pnp_ransac as ransac.ransac_pnp calls it (D_med = D_high): everything it returns."""
    d, i64 = C.c_double, C.c_int64
    res = _ffi.PnpResult()
    m = len(X)
    im, ih = np.full(m, -1, np.int64), np.full(m, -1, np.int64)
    km, kh = i64(0), i64(0)
    tp = None if tuples is None else _ffi.ptr(tuples, C.c_int32)
    _ffi.check(_ffi.lib().rs_pnp_ransac(
        ctx.handle, _ffi.ptr(X, d), _ffi.ptr(y, d), m, _ffi.ptr(X, d), _ffi.ptr(y, d), m, k, H,
        mode, seed, tp, thresh, C.byref(res), _ffi.ptr(im, i64), C.byref(km), _ffi.ptr(ih, i64),
        C.byref(kh)))
    found = res.best_index >= 0
    return {"R": bytes(res.R) if found else b"", "t": bytes(res.t) if found else b"",
            "inl_med": im[:km.value].tobytes() if found else b"",
            "inl_high": ih[:kh.value].tobytes() if found else b"",
            "best_index": int(res.best_index), "count": int(res.best_count) if found else 0}


@pytest.mark.parametrize("k, m", [(6, 6), (6, 7), (6, 500), (3, 4), (3, 500)])
def test_pnp_philox_equals_tuple_mode(ctx, k, m):
    # (exact data in the small sets: the 6-point DLT does not survive pixel noise, and a pose
    # without a consensus would leave nothing but the index -1 to compare)
    if m == 500:
        X, _, y, _, _, _ = synth.pnp_scene(m, 0.2, seed=10 + m)
    else:
        X, _, y, _, _, _ = synth.pnp_scene(m, 0.0, seed=10 + m, sigma=0.0)
    X, y = _ffi.f64c(X), _ffi.f64c(y)
    H, thr = 65, (3.0 / 800.0) ** 2
    got = _pnp(ctx, X, y, k, H, thr, _ffi.SAMPLER_PHILOX, seed=HIGH_SEED)
    tup = np.ascontiguousarray(pr.floyd_tuples(HIGH_SEED, 0, H, m, k))
    want = _pnp(ctx, X, y, k, H, thr, _ffi.SAMPLER_TUPLES, tuples=tup)
    print(f"\nk {k} m {m}: best {got['best_index']} count {got['count']}")
    for key in want:
        assert got[key] == want[key], key
    assert got["best_index"] >= 0 and got["count"] >= min(m, 100)
