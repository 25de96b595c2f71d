"""The F plan's pruned count (RSAMD_PRUNE=1, f8_plan.hip: a full count of the first hypothesis
groups, the prefix [0, K) of the others, the rest of those that can still reach L - 1) against
the single whole-window launch (RSAMD_PRUNE=0): every comparison is exact (bit) equality of
what the two plans return for the same calls; prune_stats() says what the pruned plan did."""
import numpy as np
import pytest

from tsbb15_amd import _ffi, synth

pytestmark = pytest.mark.gpu

N, H = 257, 4096   # n is no multiple of 8; the CPU model of this pair: K = 104, 6.6 % survive
G0 = 32            # hypothesis groups of the default sample


def _pair(n=N, seed=3):
    p1, p2, _ = synth.two_view(n, 0.30, seed=seed)
    return p1, p2


def _plan(ctx, monkeypatch, prune, pts, max_hyp=H, **env):
    env = {"RSAMD_PRUNE": "1" if prune else "0", **{k: str(v) for k, v in env.items()}}
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    plan = _ffi.F8Plan(ctx, pts[0].shape[1], max_hyp)
    plan.set_points(*pts)
    for k in env:
        monkeypatch.delenv(k, raising=False)
    return plan


def _rec(plan, h):
    """Everything the plan returns for its last run, floats as bytes (NaN compares equal)."""
    r, inl = plan.result()
    head = (int(r.best_index), int(r.best_count), int(r.max_count_fast), int(r.n_candidates),
            int(r.guard_mismatch), np.array([*r.F[:], r.best_std, r.best_norm]).tobytes())
    cands = sorted((c.index, c.count, np.array([c.std_d, c.norm_d, *c.F[:]]).tobytes())
                   for c in plan.candidates())
    return (head, inl.tolist(), cands, plan.counts(h).tobytes(), plan.models(h).tobytes())


def _philox(plan, h=H, i=0):
    plan.run(h, mode=_ffi.SAMPLER_PHILOX, seed=5, hyp_offset=i * H)


_REF = {}


def _unpruned(ctx, monkeypatch, key, pts, body, max_hyp=H):
    """body(plan) on a RSAMD_PRUNE=0 plan, computed once per key and shared."""
    if key not in _REF:
        plan = _plan(ctx, monkeypatch, False, pts, max_hyp=max_hyp)
        try:
            _REF[key] = body(plan)
            st = plan.prune_stats()
            assert st["K"] == st["npad"] and st["survivors"] == 0
        finally:
            plan.close()
    return _REF[key]


def _one_run(plan):
    _philox(plan)
    return _rec(plan, H)


def _check(ctx, monkeypatch, key, pts, body, max_hyp=H, **env):
    """body on a pruned plan equals body on the unpruned one; returns the pruned plan's stats."""
    plan = _plan(ctx, monkeypatch, True, pts, max_hyp=max_hyp, **env)
    try:
        got = body(plan)
        st = plan.prune_stats()
    finally:
        plan.close()
    want = _unpruned(ctx, monkeypatch, key, pts, body, max_hyp=max_hyp)
    assert got == want
    print(key, env, st)
    return st


def test_pruning_engages(ctx, monkeypatch):
    st = _check(ctx, monkeypatch, "pair", _pair(), _one_run)
    assert st["K"] < st["npad"]
    assert 0 < st["survivors"] < H / 2


def test_against_the_float64_kernel(ctx, monkeypatch):
    pts = _pair()
    out = []
    for fp64 in (False, True):
        plan = _plan(ctx, monkeypatch, True, pts)
        try:
            plan.set_count_precision(fp64)
            out.append(_one_run(plan))
            st = plan.prune_stats()
            assert (st["K"] == st["npad"]) == fp64   # the float64 path is not pruned
        finally:
            plan.close()
    assert out[0] == out[1]


@pytest.mark.parametrize("h", [64, 100])
def test_no_prefix_stage(ctx, monkeypatch, h):
    # H <= 64 G0: the sample is the whole run (h = 100: a ragged last group)
    def body(plan):
        _philox(plan, h)
        return _rec(plan, h)
    st = _check(ctx, monkeypatch, f"h{h}", _pair(), body)
    assert st["K"] == st["npad"] and st["survivors"] == 0


def test_no_pruning_possible(ctx, monkeypatch):
    # unrelated correspondences: L stays near 8, so too few points could be skipped
    rs = np.random.RandomState(4)
    pts = (rs.uniform(0, 1000, (2, 64)), rs.uniform(0, 1000, (2, 64)))
    st = _check(ctx, monkeypatch, "random64", pts, _one_run)
    assert st["K"] == st["npad"] and st["survivors"] == 0


def test_smallest_plan(ctx, monkeypatch):
    def body(plan):
        _philox(plan, 1)
        return _rec(plan, 1)
    st = _check(ctx, monkeypatch, "n8", _pair(8), body, max_hyp=1)
    assert st["K"] == st["npad"]


def test_margin_zero(ctx, monkeypatch):
    # K = roundup8(n - L) leaves n - K = L - s points, s = K - (n - L) in [0, 7]: a hypothesis
    # needs s - 1 inliers among the first K to stay able to reach L - 1.  The run is chosen, by
    # the unpruned plan's counts, so that s <= 1: then every hypothesis past the sample survives
    # (a sample of 16 groups, a quarter of the run, so that they are more than H / 2)
    pts, g0 = _pair(), 16
    probe = _plan(ctx, monkeypatch, False, pts)
    try:
        for i in range(32):
            _philox(probe, i=i)
            L = int(probe.counts(64 * g0).max())
            if (N - L) % 8 in (0, 7):
                break
        else:
            raise AssertionError("no run with n - L = 0 or 7 (mod 8)")
    finally:
        probe.close()

    def body(plan):
        _philox(plan, i=i)
        return _rec(plan, H)
    st = _check(ctx, monkeypatch, f"pair_run{i}", pts, body, RSAMD_PRUNE_MARGIN=0,
                RSAMD_PRUNE_SAMPLE=g0)
    assert st["L"] == L and st["K"] == (N - L + 7) // 8 * 8 < st["npad"]
    assert st["survivors"] == H - 64 * g0 > H / 2


def test_large_margin(ctx, monkeypatch):
    # a long prefix, a rest stage of a few points for a handful of hypotheses
    st = _check(ctx, monkeypatch, "pair", _pair(), _one_run, RSAMD_PRUNE_MARGIN=120)
    assert st["K"] < st["npad"] <= st["K"] + 64
    assert st["survivors"] > 0


def test_weak_sample(ctx, monkeypatch):
    st = _check(ctx, monkeypatch, "pair", _pair(), _one_run, RSAMD_PRUNE_SAMPLE=1)
    assert st["survivors"] <= H - 64


def test_rotation(ctx, monkeypatch):
    # nine runs reuse the four buffer sets (words, survivor lists, finish counters) on both
    # lanes: read back after every run, then after nine back to back
    def body(plan):
        out = []
        for i in range(9):
            _philox(plan, i=i)
            out.append(_rec(plan, H))
        for i in range(9):
            _philox(plan, i=9 + i)
        out.append(_rec(plan, H))
        return out
    _check(ctx, monkeypatch, "rotation", _pair(), body)


def test_tuple_mode_with_a_tie(ctx, monkeypatch):
    # host tuples with the best hypothesis twice (once inside the sample, once past it): the
    # count tie at c* must produce the same replay winner
    pts = _pair()
    tup, _, _ = _ffi.np_choice_tuples(*_ffi.np_seed(3), N, 8, H)
    probe = _plan(ctx, monkeypatch, False, pts)
    try:
        probe.run(H, mode=_ffi.SAMPLER_TUPLES, tuples=tup)
        best = int(probe.result()[0].best_index)
    finally:
        probe.close()
    tup = tup.copy()
    tup[70] = tup[best]
    tup[H - 3] = tup[best]

    def body(plan):
        plan.run(H, mode=_ffi.SAMPLER_TUPLES, tuples=tup)
        return _rec(plan, H)
    st = _check(ctx, monkeypatch, "tuples", pts, body)
    assert st["K"] < st["npad"]


def test_bookkeeping(ctx, monkeypatch):
    plan = _plan(ctx, monkeypatch, True, _pair())
    try:
        _philox(plan)
        st = plan.prune_stats()
        counts = plan.counts(H)
    finally:
        plan.close()
    assert st["npad"] == (N + 7) // 8 * 8
    assert st["K"] % 8 == 0 and 0 < st["K"] <= st["npad"]
    assert 0 <= st["survivors"] <= H - 64 * G0
    assert st["L"] == counts[:64 * G0].max()
