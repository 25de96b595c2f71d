"""The F plan's deferred recount (f8_plan.hip, plan_recount; f8_kernels.hip above k_f8_count32q,
"Carried bound"): a carried run is two count launches, prefix and rest.  When its bound turns out
to be above c* the run's tail selects nothing and marks the run's pinned header; the run is counted
again in full only inside the flush that reads it.  A fallen-back run that is never read is never
recounted, and leaves its lane a lower guess.  Every comparison of results is exact (bit) equality
of what a carrying plan and an RSAMD_PRUNE=0 plan return for the same calls; recount_stats(),
carry_stats() and prune_stats() say what the carrying plan did.

The recount figure of the rotation: its runs 0 and 10 are the first runs of lanes 0 and 1, sample
runs that cannot fall back, which is why 16 of the 18 runs are carried and fall back.  Ten runs
are read, the first of them run 0, so nine of the runs read fell back: nine recounts, a tenth
after the three further runs."""
import numpy as np
import pytest

from tsbb15_amd import _ffi, synth

pytestmark = pytest.mark.gpu

N, H = 257, 4096   # as test_gpu_f8_carry.py: n is no multiple of 8, 64 hypothesis groups
G0 = 32            # hypothesis groups of the default sample
HS = 3072          # another H that still has hypotheses past the sample
GAP = max(16, N // 50)
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


def _head(plan):
    r, inl = plan.result()
    return ((int(r.best_index), int(r.best_count), int(r.max_count_fast), int(r.n_candidates),
             int(r.guard_mismatch), np.array([*r.F[:], r.best_std, r.best_norm]).tobytes()),
            inl.tolist())


def _cands(plan):
    return sorted((c.index, c.count, np.array([c.std_d, c.norm_d, *c.F[:]]).tobytes())
                  for c in plan.candidates())


def _rec(plan, h=H):
    """Everything the plan returns for its last run, floats as bytes (NaN compares equal)."""
    return (*_head(plan), _cands(plan), plan.counts(h).tobytes(), plan.models(h).tobytes())


def _both(ctx, monkeypatch, pts, body, common=None, **env):
    """body(plan, prune) on the carrying plan (with env) and on the unpruned one; `common` is the
    environment of both."""
    out = []
    for prune in (True, False):
        plan = _plan(ctx, monkeypatch, prune, pts, **{**(common or {}), **(env if prune else {})})
        try:
            out.append(body(plan, prune))
        finally:
            plan.close()
    return out


def _philox(plan, i=0, h=H, thresh=1.5):
    plan.run(h, mode=_ffi.SAMPLER_PHILOX, seed=5, hyp_offset=i * H, thresh=thresh)


def _tuples(seed=3):
    return _ffi.np_choice_tuples(*_ffi.np_seed(seed), N, 8, H)[0].copy()


def test_forced_fallback_rotation(ctx, monkeypatch):
    def body(plan, prune):
        out, rc = [], []
        for i in range(9):          # read one by one: all on lane 0
            _philox(plan, i)
            out.append(_rec(plan))
            rc.append(plan.recount_stats()[0] if prune else None)
        for i in range(9):          # back to back: both lanes, the last one read
            _philox(plan, 9 + i)
        out.append(_rec(plan))
        rc.append(plan.recount_stats()[0] if prune else None)
        cs = plan.carry_stats() if prune else None
        for i in range(3):          # a recount after a recount on the same buffer sets
            _philox(plan, 18 + i)
        out.append(_rec(plan))
        rc.append(plan.recount_stats()[0] if prune else None)
        return out, rc, cs, (plan.carry_stats() if prune else None), plan.lane_waits()

    (got, rc, cs, cs2, waits), (want, _, _, _, waits0) = _both(ctx, monkeypatch, _pair(), body,
                                                               **FALL)
    print(rc, cs, cs2)
    assert got == want
    # one recount per read of a run that fell back: run 0 is lane 0's sample run
    assert rc == [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10]
    assert cs["carried"] == 16 and cs["fallbacks"] == 16
    assert cs["last_carried"] and cs["last_fell_back"]
    assert cs2["carried"] == 19 and cs2["fallbacks"] == 19 and cs2["last_fell_back"]
    assert waits == waits0 == 0


def test_launch_counts(ctx, monkeypatch):
    def body(plan, prune):
        out = []
        _philox(plan, 0)                     # lane 0's first run
        out.append(plan.recount_stats()[1])
        _philox(plan, 1)                     # lane 1's first run
        out.append(plan.recount_stats()[1])
        _philox(plan, 2)                     # carried
        out.append(plan.recount_stats()[1])
        fell = [plan.carry_stats()["last_fell_back"]]
        _philox(plan, 3)                     # carried, on lane 0 after the read
        out.append(plan.recount_stats()[1])
        fell.append(plan.carry_stats()["last_fell_back"])
        return out, plan.recount_stats()[0], sum(fell), plan.carry_stats()

    (got, rc, fell, cs), (want, rc0, _, _) = _both(ctx, monkeypatch, _pair(), body)
    assert got == [3, 3, 2, 2] and want == [1, 1, 1, 1]
    assert cs["carried"] == 2
    assert rc == fell == cs["fallbacks"] and rc0 == 0   # both carried runs were read


def test_unread_fallback_between_good_runs(ctx, monkeypatch):
    # host tuples as in test_gpu_f8_carry.test_guess_above_cstar_with_host_tuples: `tup` holds the
    # best hypothesis, tup2 the worse half twice over, so its c* is the median count of tup.  Lane
    # 1 needs a run before B for B to be carried there: two good runs first, then A, B, C, D, all
    # back to back, so that B and D are on lane 1; only D is read
    pts, tup = _pair(), _tuples()
    probe = _plan(ctx, monkeypatch, False, pts)
    try:
        probe.run(H, mode=_ffi.SAMPLER_TUPLES, tuples=tup)
        best = int(probe.result()[0].best_index)
        worse = np.argsort(probe.counts(H), kind="stable")[:H // 2]
        tup2 = np.ascontiguousarray(np.concatenate([tup[worse], tup[worse]]))
        tup[H - 3] = tup[best]
        probe.run(H, mode=_ffi.SAMPLER_TUPLES, tuples=tup)
        c1 = int(probe.result()[0].max_count_fast)
        probe.run(H, mode=_ffi.SAMPLER_TUPLES, tuples=tup2)
        c2 = int(probe.result()[0].max_count_fast)
        counts_b = set(probe.counts(H).tolist())
    finally:
        probe.close()
    assert c2 < c1 - GAP      # B's guess, c1 - GAP, is above its c*

    def body(plan, prune):
        for t in (tup, tup, tup, tup2, tup, tup):     # lanes 0 1 0 1 0 1
            plan.run(H, mode=_ffi.SAMPLER_TUPLES, tuples=t)
        rec = _rec(plan)
        return (rec, plan.prune_stats(), plan.recount_stats(),
                plan.carry_stats() if prune else None, plan.lane_waits())

    (got, st, rs, cs, waits), (want, _, _, _, waits0) = _both(ctx, monkeypatch, pts, body)
    print(st, rs, cs, c1, c2)
    assert got == want
    assert rs == (0, 2) and waits == waits0 == 0
    assert cs["carried"] == 4 and cs["fallbacks"] == 1
    assert cs["last_carried"] and not cs["last_fell_back"]
    # D's bound: B's best survivor count (a full count of one of B's hypotheses, at most B's c*)
    # less the gap, or from 0: nothing pruned.  Never the c1 - GAP of the run before B
    if st["L"] + GAP > 0:
        assert st["L"] + GAP in counts_b and st["L"] + GAP <= c2
    else:
        assert st["L"] <= 1 and st["K"] == st["npad"] == NPAD


def test_unread_fallback_leaves_its_best_survivor(ctx, monkeypatch):
    # the same six runs with a fallen-back B whose c_f is positive and known: t is the best count
    # below c1 among the good tuples' hypotheses, B's hypotheses are those with a count of at most
    # t, and the gap is c1 - t - 1, so B is screened against L = t + 1.  Its best hypothesis has
    # the full count t = L - 1: it survives whatever the screen certifies (the survivor rule), and
    # nothing of B counts more, so c_f = t < L: B falls back and leaves t, D is screened against
    # t less the gap
    pts, tup = _pair(), _tuples()
    probe = _plan(ctx, monkeypatch, False, pts)
    try:
        probe.run(H, mode=_ffi.SAMPLER_TUPLES, tuples=tup)
        counts = probe.counts(H)
    finally:
        probe.close()
    c1 = int(counts.max())
    t = int(counts[counts < c1].max())
    gap = c1 - t - 1
    tup2 = np.ascontiguousarray(np.resize(tup[counts <= t], (H, 8)))

    def body(plan, prune):
        for x in (tup, tup, tup, tup2, tup, tup):     # lanes 0 1 0 1 0 1
            plan.run(H, mode=_ffi.SAMPLER_TUPLES, tuples=x)
        rec = _rec(plan)
        return (rec, plan.prune_stats(), plan.recount_stats(),
                plan.carry_stats() if prune else None)

    (got, st, rs, cs), (want, _, _, _) = _both(ctx, monkeypatch, pts, body, RSAMD_CARRY_GAP=gap)
    print(st, rs, cs, c1, t, gap)
    assert got == want and want[0][2] == c1
    assert rs == (0, 2)
    assert cs["carried"] == 4 and cs["fallbacks"] == 1 and not cs["last_fell_back"]
    assert st["L"] == t - gap


ACCESSORS = ["result", "candidates", "counts", "stage_counts", "models", "prune_stats",
             "carry_stats", "kernel_ms"]


def _access(plan, name):
    if name == "result":
        return _head(plan)
    if name == "candidates":
        return _cands(plan)
    if name in ("counts", "stage_counts"):
        return getattr(plan, name)(H).tobytes()
    if name == "models":
        return plan.models(H).tobytes()
    return getattr(plan, name)()


def test_each_accessor_first(ctx, monkeypatch):
    def body(plan, prune):
        _philox(plan, 0)
        plan.result()
        out = []
        for i, first in enumerate(ACCESSORS):
            _philox(plan, 1 + i)             # on lane 0, carried: falls back
            before = plan.recount_stats()[0]
            rec = {first: _access(plan, first)}
            mid = plan.recount_stats()[0]
            for name in ACCESSORS:
                if name != first:
                    rec[name] = _access(plan, name)
            out.append((rec, mid - before, plan.recount_stats()[0] - before))
        return out

    got, want = _both(ctx, monkeypatch, _pair(), body, **FALL)
    for (g, d1, d2), (w, _, _), first in zip(got, want, ACCESSORS):
        assert (d1, d2) == (1, 1), first      # the first accessor recounts, no other one does
        for name in ("result", "candidates", "counts", "stage_counts", "models"):
            assert g[name] == w[name], (first, name)
        assert g["stage_counts"] == g["counts"]
        cstar = g["result"][0][2]
        st, cs = g["prune_stats"], g["carry_stats"]
        assert st["K"] < st["npad"] == NPAD and st["L"] > cstar, first
        assert cs["last_carried"] and cs["last_fell_back"], first
        assert g["kernel_ms"]["count_ms"] > 0.0
    assert got[-1][0]["carry_stats"]["fallbacks"] == len(ACCESSORS)


def test_dropped_unread(ctx, monkeypatch):
    pts = _pair()

    def body(plan, prune):
        out, rc = [], []
        _philox(plan, 0)
        plan.result()
        _philox(plan, 1)                      # carried on lane 0, falls back, unread
        plan.set_points(*pts)
        rc.append(plan.recount_stats())
        if prune:
            with pytest.raises(ValueError):   # that run has no result
                plan.result()
        _philox(plan, 2)
        rc.append(plan.recount_stats())
        out.append(_rec(plan))
        _philox(plan, 3)                      # carried, falls back, unread
        plan.set_count_precision(True)
        plan.set_count_precision(False)
        rc.append(plan.recount_stats())
        _philox(plan, 4)
        rc.append(plan.recount_stats())
        out.append(_rec(plan))
        cs = plan.carry_stats() if prune else None
        _philox(plan, 5)                      # carried, falls back, unread
        return out, rc, cs, plan.recount_stats()   # ... and the caller closes the plan

    (got, rc, cs, end), (want, _, _, _) = _both(ctx, monkeypatch, pts, body, **FALL)
    assert got == want
    # no recount anywhere: the runs read are sample runs (three launches), the others were dropped
    assert [r[0] for r in rc] == [0, 0, 0, 0] and end == (0, 2)
    assert [r[1] for r in rc] == [2, 3, 2, 3]
    assert not cs["last_carried"] and not cs["last_fell_back"]
    assert cs["carried"] == 2 and cs["fallbacks"] == 2


def test_run_np_after_unread_fallback_on_lane1(ctx, monkeypatch):
    def body(plan, prune):
        for i in range(4):                   # lanes 0 1 0 1: the last two carried, fallen back
            _philox(plan, i)
        key, pos = plan.run_np(H, *_ffi.np_seed(3))   # waits for lane 1, runs on lane 0
        rec = (_rec(plan), key.tobytes(), pos)
        return (rec, plan.lane_waits(), plan.recount_stats()[0],
                plan.carry_stats() if prune else None)

    (got, waits, rc, cs), (want, waits0, _, _) = _both(ctx, monkeypatch, _pair(), body, **FALL)
    assert got == want
    assert waits == waits0 == 1
    assert cs["carried"] == 3 and cs["fallbacks"] == 3 and cs["last_fell_back"]
    assert rc == 1                           # the parity run itself, when it was read


def test_one_lane_forced_fallback(ctx, monkeypatch):
    def body(plan, prune):
        out = []
        for i in range(3):
            _philox(plan, i)
            out.append(_rec(plan))
        for i in range(5):
            _philox(plan, 3 + i)
        out.append(_rec(plan))
        return (out, plan.lane_waits(), plan.recount_stats()[0],
                plan.carry_stats() if prune else None)

    (got, waits, rc, cs), (want, waits0, _, _) = _both(ctx, monkeypatch, _pair(), body,
                                                       common={"RSAMD_OVERLAP": 0}, **FALL)
    assert got == want
    assert waits == waits0 == 0
    assert cs["carried"] == 7 and cs["fallbacks"] == 7 and rc == 3


def test_nan_models_forced_fallback(ctx, monkeypatch):
    # tuples of one index eight times give NaN models: they certify no point, survive the screen
    # and end with a full count of 0, after the recount too
    tup = _tuples()
    deg = np.array([5, 70, 2047, 64 * G0, 64 * G0 + 63, 64 * G0 + 64, 3000, H - 1])
    tup[deg] = (deg % N)[:, None]

    def body(plan, prune):
        plan.run(H, mode=_ffi.SAMPLER_TUPLES, tuples=tup)
        first = _rec(plan)
        plan.run(H, mode=_ffi.SAMPLER_TUPLES, tuples=tup)
        return (first, _rec(plan), plan.stage_counts(H), plan.counts(H), plan.recount_stats()[0],
                plan.carry_stats() if prune else None)

    (f1, got, raw, full, rc, cs), (w1, want, _, full0, _, _) = _both(ctx, monkeypatch, _pair(),
                                                                     body, **FALL)
    assert (f1, got) == (w1, want)
    models = np.frombuffer(got[4]).reshape(H, 9)
    assert (~np.isfinite(models[deg])).any(axis=1).all()
    assert cs["last_carried"] and cs["last_fell_back"] and rc == 1
    assert np.all(raw[deg] == 0) and np.all(full[deg] == 0)
    assert np.array_equal(full, full0) and np.array_equal(raw, full0)
