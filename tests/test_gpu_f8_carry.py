"""The F plan's carried bound (f8_kernels.hip above k_f8_count32q, "Carried bound"): a run on a
stream lane whose previous run had the same H and threshold over the same points has no sample
stage; it screens every hypothesis against L = (that run's c*) - gap and counts everything again
when the best full count among its survivors does not reach L.  Every comparison is exact (bit)
equality of what a carrying plan and an RSAMD_PRUNE=0 plan return for the same calls;
carry_stats() and prune_stats() say what the carrying plan did."""
import numpy as np
import pytest

from tsbb15_amd import _ffi, synth

pytestmark = pytest.mark.gpu

N, H = 257, 4096   # as test_gpu_f8_prune.py: n is no multiple of 8, 64 hypothesis groups
G0 = 32            # hypothesis groups of the default sample
HS = 3072          # another H that still has hypotheses past the sample (H > 64 G0)
GAP = max(16, N // 50)  # the default gap (f8_plan.hip kCarryGapMin, kCarryGapDiv)
NPAD = (N + 7) // 8 * 8
FALL = {"RSAMD_CARRY_GAP": -1000}   # L far above any count: every carried run falls back


def _pair(outliers=0.30):
    p1, p2, _ = synth.two_view(N, outliers, seed=3)
    return p1, p2


def _plan(ctx, monkeypatch, prune, pts, **env):
    env = {"RSAMD_PRUNE": "1" if prune else "0", "RSAMD_CARRY": "1",
           **{k: str(v) for k, v in env.items()}}
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
    """body(plan) on the carrying plan (with env) and on the unpruned one: (got, want)."""
    out = []
    for prune in (True, False):
        plan = _plan(ctx, monkeypatch, prune, pts, **(env if prune else {}))
        try:
            out.append(body(plan, prune))
        finally:
            plan.close()
    return out


def _philox(plan, i=0, h=H, thresh=1.5):
    plan.run(h, mode=_ffi.SAMPLER_PHILOX, seed=5, hyp_offset=i * H, thresh=thresh)


def _sound(raw, full, st):
    """The stage rule of a carried run on every hypothesis (no sample: g0 = 0)."""
    K, L = st["K"], st["L"]
    assert K < st["npad"], st
    r, f = raw.astype(np.int64), full.astype(np.int64)
    hopeless = r + (N - K) < L - 1
    # a survivor has its full count; everybody else is below the bar with an upper bound
    assert np.all((r == f) | (hopeless & (f <= r + (N - K))))
    assert np.all(f[hopeless] < L - 1)
    return int(np.count_nonzero(~hopeless))


def _tuples(seed=3):
    return _ffi.np_choice_tuples(*_ffi.np_seed(seed), N, 8, H)[0].copy()


def _rotation(plan, prune):
    """Nine runs read back one by one (all on lane 0), then nine back to back (both lanes)."""
    out = []
    for i in range(9):
        _philox(plan, i)
        out.append(_rec(plan))
    for i in range(9):
        _philox(plan, 9 + i)
    out.append(_rec(plan))
    return out, (plan.carry_stats(), plan.lane_waits()) if prune else None


def test_back_to_back(ctx, monkeypatch):
    (got, (cs, waits)), (want, _) = _both(ctx, monkeypatch, _pair(), _rotation)
    print(cs)
    assert got == want
    # every run but the first on each lane: lane 0 alone could have carried 8 + 5 of them
    assert cs["carried"] == 16 and cs["last_carried"]
    assert cs["fallbacks"] <= cs["carried"]
    assert waits == 0


def test_forced_fallback(ctx, monkeypatch):
    (got, (cs, waits)), (want, _) = _both(ctx, monkeypatch, _pair(), _rotation, **FALL)
    assert got == want
    assert cs["carried"] == 16 and cs["fallbacks"] == 16
    assert cs["last_carried"] and cs["last_fell_back"]
    assert waits == 0


def test_stage_rule(ctx, monkeypatch):
    def body(plan, prune):
        _philox(plan, 0)
        first = _rec(plan)
        _philox(plan, 1)
        return (first, _rec(plan), plan.stage_counts(H), plan.counts(H), plan.prune_stats(),
                plan.carry_stats() if prune else None)

    (f1, got, raw, full, st, cs), (w1, want, raw0, full0, _, _) = _both(ctx, monkeypatch, _pair(),
                                                                        body)
    assert (f1, got) == (w1, want)
    assert cs["last_carried"] and cs["carried"] == 1
    assert st["L"] == w1[0][2] - GAP           # the first run's c* less the gap
    cstar = want[0][2]
    assert cs["last_fell_back"] == (cstar < st["L"])
    if not cs["last_fell_back"]:
        print(st, "survivors at least", _sound(raw, full, st))
        assert _sound(raw, full, st) <= st["survivors"] <= H
    assert np.array_equal(raw0, full0) and np.array_equal(full, full0)


def test_fallback_stage_counts_are_full(ctx, monkeypatch):
    def body(plan, prune):
        _philox(plan, 0)
        plan.result()      # the next run follows it on lane 0
        _philox(plan, 1)
        return plan.stage_counts(H), plan.counts(H), plan.prune_stats()

    (raw, full, st), (raw0, full0, _) = _both(ctx, monkeypatch, _pair(), body, **FALL)
    assert st["K"] < st["npad"] and st["L"] > full0.max()
    assert np.array_equal(raw, full0) and np.array_equal(full, full0)


def test_set_points_drops_the_carry(ctx, monkeypatch):
    # the same N with 60 % outliers: c* is far lower, the carried guess would be above it
    weak = _pair(0.60)

    def body(plan, prune):
        _philox(plan, 0)
        out = [_rec(plan)]
        plan.set_points(*weak)
        _philox(plan, 1)
        out.append(_rec(plan))
        return out, plan.prune_stats(), plan.counts(64 * G0), plan.carry_stats() if prune else None

    (got, st, head, cs), (want, _, _, _) = _both(ctx, monkeypatch, _pair(), body)
    assert got == want
    assert want[1][0][2] < want[0][0][2] - GAP   # the guess would indeed have been too high
    assert cs == {"carried": 0, "fallbacks": 0, "last_carried": False, "last_fell_back": False}
    assert st["L"] == head.max()                 # a sample run


def test_guess_above_cstar_with_host_tuples(ctx, monkeypatch):
    # run 1: numpy tuples with the best hypothesis twice; run 2 on the same lane: the worse half
    # of those hypotheses, twice over, so its c* is the median count of run 1
    pts, tup = _pair(), _tuples()
    probe = _plan(ctx, monkeypatch, False, pts)
    try:
        probe.run(H, mode=_ffi.SAMPLER_TUPLES, tuples=tup)
        best = int(probe.result()[0].best_index)
        worse = np.argsort(probe.counts(H), kind="stable")[:H // 2]
    finally:
        probe.close()
    tup2 = np.ascontiguousarray(np.concatenate([tup[worse], tup[worse]]))
    tup[H - 3] = tup[best]

    def body(plan, prune):
        plan.run(H, mode=_ffi.SAMPLER_TUPLES, tuples=tup)
        out = [_rec(plan)]
        plan.run(H, mode=_ffi.SAMPLER_TUPLES, tuples=tup2)
        out.append(_rec(plan))
        return out, plan.prune_stats(), plan.carry_stats() if prune else None

    (got, st, cs), (want, _, _) = _both(ctx, monkeypatch, pts, body)
    assert got == want
    c1, c2 = want[0][0][2], want[1][0][2]
    assert st["L"] == c1 - GAP and c2 < st["L"] and st["K"] < st["npad"]
    assert cs["last_carried"] and cs["last_fell_back"] and cs["fallbacks"] == 1


def test_parameter_changes_end_the_carry(ctx, monkeypatch):
    def body(plan, prune):
        out, carried = [], []

        def step(h=H, thresh=1.5):
            _philox(plan, len(out), h, thresh)
            out.append(_rec(plan, h))
            carried.append(plan.carry_stats()["last_carried"] if prune else None)

        step()                 # 0 the plan's first run
        step()                 # 1 carried
        step(thresh=2.0)       # 2 another threshold
        step(thresh=2.0)       # 3 carried
        step(h=HS)         # 4 another H
        step(h=HS)         # 5 carried
        plan.set_count_precision(True)
        step(h=HS)         # 6 the float64 kernel
        plan.set_count_precision(False)
        step(h=HS)         # 7 back on fp32: a sample first
        step(h=HS)         # 8 carried
        for h in (64, 64, 100, 100):   # 9-12: H <= 64 G0, the sample is the whole run
            step(h=h)
        return out, carried

    (got, carried), (want, _) = _both(ctx, monkeypatch, _pair(), body)
    assert got == want
    assert carried == [False, True, False, True, False, True, False, False, True,
                       False, False, False, False]


@pytest.mark.parametrize("env", [{}, {"RSAMD_CARRY_GAP": 0}])
def test_no_pruning_possible(ctx, monkeypatch, env):
    # unrelated correspondences: c* stays near 8, too few points could be skipped, K = npad;
    # nothing is dropped, so the run is valid whatever the carried bound
    rs = np.random.RandomState(4)
    pts = (rs.uniform(0, 1000, (2, 64)), rs.uniform(0, 1000, (2, 64)))

    def body(plan, prune):
        _philox(plan, 0)
        out = [_rec(plan)]
        _philox(plan, 1)
        out.append(_rec(plan))
        return out, plan.prune_stats(), plan.carry_stats() if prune else None

    (got, st, cs), (want, _, _) = _both(ctx, monkeypatch, pts, body, **env)
    assert got == want
    assert st["K"] == st["npad"] == 64 and st["survivors"] == 0
    assert cs["last_carried"] and not cs["last_fell_back"] and cs["fallbacks"] == 0


def test_nan_models(ctx, monkeypatch):
    # tuples of one index eight times give NaN models, inside the first 32 groups too: they
    # certify no point, survive the carried run's screen and end with a full count of 0
    tup = _tuples()
    deg = np.array([5, 70, 2047, 64 * G0, 64 * G0 + 63, 64 * G0 + 64, 3000, H - 1])
    tup[deg] = (deg % N)[:, None]

    def body(plan, prune):
        plan.run(H, mode=_ffi.SAMPLER_TUPLES, tuples=tup)
        first = _rec(plan)
        plan.run(H, mode=_ffi.SAMPLER_TUPLES, tuples=tup)
        return (first, _rec(plan), plan.stage_counts(H), plan.counts(H), plan.prune_stats(),
                plan.carry_stats() if prune else None)

    (f1, got, raw, full, st, cs), (w1, want, _, full0, _, _) = _both(ctx, monkeypatch, _pair(), body)
    assert (f1, got) == (w1, want)
    models = np.frombuffer(got[4]).reshape(H, 9)
    assert (~np.isfinite(models[deg])).any(axis=1).all()
    assert cs["last_carried"] and not cs["last_fell_back"]   # the same run again: c* - gap < c*
    _sound(raw, full, st)
    assert np.all(raw[deg] == 0) and np.all(full[deg] == 0)
    assert np.array_equal(full, full0)


def test_tie_at_cstar(ctx, monkeypatch):
    # the best hypothesis twice, one copy inside the first 32 groups: the same replay winner
    pts, tup = _pair(), _tuples()
    probe = _plan(ctx, monkeypatch, False, pts)
    try:
        probe.run(H, mode=_ffi.SAMPLER_TUPLES, tuples=tup)
        best = int(probe.result()[0].best_index)
    finally:
        probe.close()
    tup[70] = tup[best]
    tup[H - 3] = tup[best]

    def body(plan, prune):
        out = []
        for _ in range(2):
            plan.run(H, mode=_ffi.SAMPLER_TUPLES, tuples=tup)
            out.append(_rec(plan))
        return out, plan.prune_stats(), plan.carry_stats() if prune else None

    (got, st, cs), (want, _, _) = _both(ctx, monkeypatch, pts, body)
    assert got == want
    assert got[1][0][3] >= 2                    # the tie is among the candidates
    assert cs["last_carried"] and not cs["last_fell_back"] and st["K"] < st["npad"]


def test_parity_entry_point_between_philox_runs(ctx, monkeypatch):
    def body(plan, prune):
        out = []
        _philox(plan, 0)
        out.append(_rec(plan))
        key, pos = plan.run_np(H, *_ffi.np_seed(3))
        out.append((_rec(plan), key.tobytes(), pos))
        _philox(plan, 1)
        out.append(_rec(plan))
        _philox(plan, 2)
        _philox(plan, 3)
        out.append(_rec(plan))
        return out, plan.carry_stats() if prune else None

    (got, cs), (want, _) = _both(ctx, monkeypatch, _pair(), body)
    assert got == want
    assert cs["carried"] >= 2
