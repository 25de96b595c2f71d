"""The screening prefix stage of the F plan's pruned count (f8_kernels.hip above k_f8_count32q):
past the sample a hypothesis is dropped when K minus its certified outliers among the first K
points, plus the n - K points left, cannot reach L - 1; the others are counted in full.  The rule
is checked on every hypothesis through stage_counts() (the stages' own counts) against counts()
(the full recount), and everything the plan returns against the RSAMD_PRUNE=0 plan, bit for
bit."""
import numpy as np
import pytest

from tsbb15_amd import _ffi, synth

pytestmark = pytest.mark.gpu

N, H = 257, 4096   # as test_gpu_f8_prune.py: n is no multiple of 8, 64 hypothesis groups
G0 = 32            # hypothesis groups of the default sample


def _plan(ctx, monkeypatch, prune, pts, **env):
    env = {"RSAMD_PRUNE": "1" if prune else "0", **{k: str(v) for k, v in env.items()}}
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    plan = _ffi.F8Plan(ctx, pts[0].shape[1], H)
    plan.set_points(*pts)
    for k in env:
        monkeypatch.delenv(k, raising=False)
    return plan


def _rec(plan, h=H):
    """Everything the plan returns for its last run, floats as bytes (NaN compares equal)."""
    r, inl = plan.result()
    head = (int(r.best_index), int(r.best_count), int(r.max_count_fast), int(r.n_candidates),
            int(r.guard_mismatch), np.array([*r.F[:], r.best_std, r.best_norm]).tobytes())
    cands = sorted((c.index, c.count, np.array([c.std_d, c.norm_d, *c.F[:]]).tobytes())
                   for c in plan.candidates())
    return (head, inl.tolist(), cands, plan.counts(h).tobytes(), plan.models(h).tobytes())


def _both(ctx, monkeypatch, pts, body, **env):
    """body(plan) on the pruned plan (with env) and on the unpruned one."""
    out = []
    for prune in (True, False):
        plan = _plan(ctx, monkeypatch, prune, pts, **(env if prune else {}))
        try:
            out.append(body(plan))
        finally:
            plan.close()
    return out


def _sound(raw, full, st, g0):
    """The rule on every hypothesis; returns the number that must have been counted in full."""
    n, K, L = N, st["K"], st["L"]
    assert K < st["npad"], st            # the run was screened
    h0 = 64 * g0
    assert np.array_equal(raw[:h0], full[:h0])            # the sample: full counts
    assert L == full[:h0].max()
    r, f = raw[h0:].astype(np.int64), full[h0:].astype(np.int64)
    hopeless = r + (n - K) < L - 1
    # a survivor has its full count; everybody else is below the bar with an upper bound
    assert np.all((r == f) | (hopeless & (f <= r + (n - K))))
    assert np.all(f[hopeless] < L - 1)
    return int(np.count_nonzero(~hopeless))


@pytest.mark.parametrize("g0,env", [
    (G0, {}),
    # one group as the sample: a weak L (36, the best of the run's first 64 hypotheses), and so
    # a long prefix, K = roundup8(257 - 36 + 24) = 248 of 264, with many survivors
    (1, {"RSAMD_PRUNE_SAMPLE": 1, "RSAMD_PRUNE_MARGIN": 24, "RSAMD_PRUNE_MINSKIP": 8}),
])
def test_soundness_on_every_hypothesis(ctx, monkeypatch, g0, env):
    p1, p2, _ = synth.two_view(N, 0.30, seed=3)

    def body(plan):
        plan.run(H, mode=_ffi.SAMPLER_PHILOX, seed=5)
        return plan.stage_counts(H), plan.prune_stats(), plan.counts(H), _rec(plan)

    (raw, st, full, got), (raw0, st0, full0, want) = _both(ctx, monkeypatch, (p1, p2), body, **env)
    print(env, st, "survivors at least", _sound(raw, full, st, g0))
    assert _sound(raw, full, st, g0) <= st["survivors"] <= H - 64 * g0
    assert st0["K"] == st0["npad"] and np.array_equal(raw0, full0)   # unpruned: no recount
    assert np.array_equal(full, full0)
    assert got == want


def test_inliers_first(ctx, monkeypatch):
    """60 % outliers, the inliers first, a one-group sample, m = 0 and a least skip of 8 points:
    L is weak (the best of 64 hypotheses), K = roundup8(n - L) is far above c*, and the upper
    bound c' = K - certified outliers of a good hypothesis can exceed c* -- a group maximum of
    c' folded into c* would change max_count_fast and the candidates.  The pair seed is 3:
    `python tools/screen_model.py inliers-first 3` gives, for 8 runs of 4096 numpy-sampled
    hypotheses, L 11-29, K 232-248 of npad 264, c* 53-89, and in 4 of the 8 runs K > c* with
    max c' = c* + 1 (seeds 4, 5, 6: 2, 3, 2 of 8); the kernel's fp32 guard band certifies a
    little less than the float64 model, so its c' are no smaller."""
    p1, p2, mask = synth.two_view(N, 0.60, seed=3)
    order = np.argsort(~mask, kind="stable")
    pts = (np.ascontiguousarray(p1[:, order]), np.ascontiguousarray(p2[:, order]))

    def body(plan):
        out, stats = [], []
        for i in range(8):
            plan.run(H, mode=_ffi.SAMPLER_PHILOX, seed=5, hyp_offset=i * H)
            out.append(_rec(plan))
            stats.append(plan.prune_stats())
        return out, stats

    (got, stats), (want, _) = _both(ctx, monkeypatch, pts, body, RSAMD_PRUNE_SAMPLE=1,
                                    RSAMD_PRUNE_MARGIN=0, RSAMD_PRUNE_MINSKIP=8)
    cstar = [w[0][2] for w in want]
    print([(s["L"], s["K"], s["survivors"], c) for s, c in zip(stats, cstar)])
    assert any(s["K"] < s["npad"] and s["K"] > c for s, c in zip(stats, cstar))
    assert got == want


def test_nan_models_past_the_sample(ctx, monkeypatch):
    # tuples of one index eight times: the solve returns a NaN model, which certifies no point
    # (NaN fails Q > S), so it survives, is recounted over the whole window and ends with 0
    p1, p2, _ = synth.two_view(N, 0.30, seed=3)
    tup, _, _ = _ffi.np_choice_tuples(*_ffi.np_seed(3), N, 8, H)
    tup = tup.copy()
    deg = np.array([5, 64 * G0, 64 * G0 + 63, 64 * G0 + 64, 3000, H - 1])
    tup[deg] = (deg % N)[:, None]

    def body(plan):
        plan.run(H, mode=_ffi.SAMPLER_TUPLES, tuples=tup)
        return plan.stage_counts(H), plan.prune_stats(), plan.counts(H), _rec(plan)

    (raw, st, full, got), (_, _, full0, want) = _both(ctx, monkeypatch, (p1, p2), body)
    models = np.frombuffer(got[4]).reshape(H, 9)
    assert (~np.isfinite(models[deg])).any(axis=1).all()
    _sound(raw, full, st, G0)
    # a dropped NaN model would hold c' = K, a survivor holds its full count
    assert np.all(raw[deg] == 0) and np.all(full[deg] == 0)
    assert np.array_equal(full, full0)
    assert got == want
