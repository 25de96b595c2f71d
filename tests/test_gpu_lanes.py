"""The F plan's two stream lanes (RSAMD_OVERLAP=1, f8_plan.hip: consecutive runs alternate
between the context's stream and a stream of the plan, each lane a serial chain tail + solve ->
count, no cross-stream event on the hot path) against the one-lane plan (RSAMD_OVERLAP=0):
every comparison is exact (bit) equality of what the two plans return for the same calls."""
import math

import numpy as np
import pytest

from tsbb15_amd import _ffi, synth

pytestmark = pytest.mark.gpu

N, H = 600, 4000


def _plan(ctx, monkeypatch, lanes, n=N, max_hyp=H, seed=21):
    monkeypatch.setenv("RSAMD_OVERLAP", "1" if lanes == 2 else "0")
    p1, p2, _ = synth.two_view(n, 0.3, seed=seed)
    plan = _ffi.F8Plan(ctx, n, max_hyp)
    plan.set_points(p1, p2)
    monkeypatch.delenv("RSAMD_OVERLAP", raising=False)
    return plan


def _rec(plan, h):
    """Everything the plan returns for its last run, floats as bytes (NaN compares equal)."""
    r, inl = plan.result()
    head = (int(r.best_index), int(r.best_count), int(r.max_count_fast), int(r.n_candidates),
            int(r.guard_mismatch), np.array([*r.F[:], r.best_std, r.best_norm]).tobytes())
    cands = sorted((c.index, c.count, np.array([c.std_d, c.norm_d, *c.F[:]]).tobytes())
                   for c in plan.candidates())
    return (head, inl.tolist(), cands, plan.counts(h).tobytes(), plan.models(h).tobytes())


def _both(ctx, monkeypatch, body, **kw):
    """body(plan) -> records, on a two-lane and on a one-lane plan; asserts they are equal."""
    out = []
    for lanes in (2, 1):
        plan = _plan(ctx, monkeypatch, lanes, **kw)
        try:
            out.append(body(plan))
        finally:
            plan.close()
    assert len(out[0]) == len(out[1]) and len(out[0]) > 0
    for k, (x, y) in enumerate(zip(*out)):
        assert x == y, k


def _philox(plan, i, h=H, seed=5):
    plan.run(h, mode=_ffi.SAMPLER_PHILOX, seed=seed, hyp_offset=i * H)


def test_wrap_around(ctx, monkeypatch):
    # j runs back to back, then everything of the last one: j > 8 wraps the four buffer sets and
    # pinned slots twice; the tails of the last two runs are flushed alone, one per lane
    def body(plan):
        out, i = [], 0
        for j in range(1, 11):
            for _ in range(j):
                _philox(plan, i)
                i += 1
            out.append(_rec(plan, H))
        return out
    _both(ctx, monkeypatch, body)


def test_result_after_every_run(ctx, monkeypatch):
    # the flush path with one pending tail: every run starts on an idle plan (lane 0)
    def body(plan):
        out = []
        for i in range(10):
            _philox(plan, i)
            out.append(_rec(plan, H))
        return out
    _both(ctx, monkeypatch, body)


def test_flush_with_a_tail_on_either_lane(ctx, monkeypatch):
    # result() after an even and after an odd number of runs in flight: the last run's tail
    # (the one result() returns) is pending on lane 1 and on lane 0 in turn
    def body(plan):
        out, i = [], 0
        for j in (2, 3, 2, 5, 4, 1):
            for _ in range(j):
                _philox(plan, i)
                i += 1
            out.append(plan.result()[1].tolist())
        out.append(_rec(plan, H))
        return out
    _both(ctx, monkeypatch, body)


def test_no_host_wait_in_philox_and_tuple_sequences(ctx, monkeypatch):
    # The set guard must not fire when the host has already waited for the set's last run: a
    # result() after an odd number of runs swaps lane and set parity for the next sequence.
    # Any host wait for a lane outside result() would serialise the two lanes.
    plan = _plan(ctx, monkeypatch, 2)
    try:
        i = 0
        for _ in range(6):               # 3 runs + result(), in a loop
            for _ in range(3):
                _philox(plan, i)
                i += 1
            plan.result()
        for batch in (5, 20, 1, 7, 2):   # the driver's 5 warm-up + 20 timed runs, other odd sizes
            for _ in range(batch):
                _philox(plan, i)
                i += 1
            plan.result()
        key, pos = _ffi.np_seed(3)
        for batch in (3, 5):             # host tuples, mixed with Philox runs
            for k in range(batch):
                tup, key, pos = _ffi.np_choice_tuples(key, pos, N, 8, H)
                plan.run(H, mode=_ffi.SAMPLER_TUPLES, tuples=tup)
                _philox(plan, i + k)
            plan.result()
        plan.set_timing(2, 3)            # exclusive timed runs wait on the device, not the host
        for k in range(9):
            _philox(plan, k)
        plan.result()
        assert plan.lane_waits() == 0
        # the counter does count: a parity run behind a run in flight on lane 1 waits for it
        _philox(plan, 0)
        _philox(plan, 1)
        nkey, npos = _ffi.np_seed(0)
        plan.run_np(H, nkey, npos)
        plan.result()
        assert plan.lane_waits() == 1
    finally:
        plan.close()


def test_mixed_h_and_modes(ctx, monkeypatch):
    # the parity entry points run on lane 0 behind their parse and break the alternation: the
    # next runs meet buffer sets the other lane used last (the set guard)
    def body(plan):
        out = []
        tkey, tpos = _ffi.np_seed(3)
        nkey, npos = _ffi.np_seed(0)
        _philox(plan, 0)
        _philox(plan, 1, h=65)
        tup, tkey, tpos = _ffi.np_choice_tuples(tkey, tpos, N, 8, H)
        plan.run(H, mode=_ffi.SAMPLER_TUPLES, tuples=tup)
        nkey, npos = plan.run_np(H, nkey, npos)
        out.append((npos, nkey.tolist()))
        _philox(plan, 2)
        skey, spos = plan.run_np_slice(H, 1000, 1000, nkey, npos)
        out.append((spos, skey.tolist()))
        tup, tkey, tpos = _ffi.np_choice_tuples(tkey, tpos, N, 8, H)
        plan.run(H, mode=_ffi.SAMPLER_TUPLES, tuples=tup)
        for i in range(3, 6):
            _philox(plan, i)
        out.append(_rec(plan, H))
        # and read back after each kind of run in the same order (a run_np_slice's own result)
        _philox(plan, 6, h=65)
        out.append(_rec(plan, 65))
        skey, spos = plan.run_np_slice(H, 1000, 1000, nkey, npos)
        out.append(_rec(plan, 1000) + (spos, skey.tolist()))
        return out
    _both(ctx, monkeypatch, body)


def test_state_changes_mid_sequence(ctx, monkeypatch):
    q1, q2, _ = synth.two_view(N, 0.3, seed=22)

    def body(plan):
        out, i = [], 0
        for _ in range(3):
            _philox(plan, i)
            i += 1
        plan.set_points(q1, q2)      # flushes both lanes, then new points
        for _ in range(3):
            _philox(plan, i)
            i += 1
        out.append(_rec(plan, H))
        _philox(plan, i)
        plan.set_count_precision(True)   # with one run in flight
        for _ in range(5):
            i += 1
            _philox(plan, i)
        out.append(_rec(plan, H))
        _philox(plan, i + 1)
        plan.set_count_precision(False)
        for k in range(3):
            _philox(plan, i + 2 + k)
        out.append(_rec(plan, H))
        return out
    _both(ctx, monkeypatch, body)


@pytest.mark.parametrize("level,every", [(1, 2), (2, 3)])
def test_timed_runs(ctx, monkeypatch, level, every):
    # a run that records timing events counts alone (two waits and a record); results equal,
    # and the events give finite positive times
    def body(plan):
        plan.set_timing(level, every)
        for i in range(9):
            _philox(plan, i)
        rec = _rec(plan, H)
        km = plan.kernel_ms(last_n=9)
        print(f"timing level {level} every {every}: {km}")
        assert math.isfinite(km["count_ms"]) and km["count_ms"] > 0.0
        if level == 2:
            assert math.isfinite(km["solve_ms"]) and km["solve_ms"] > 0.0
            assert math.isfinite(km["total_ms"]) and km["total_ms"] >= km["count_ms"]
        return [rec]
    _both(ctx, monkeypatch, body)


def test_two_plans_on_one_context(ctx, monkeypatch):
    # two two-lane plans interleaved on one context (lane 0 of both is the context's stream)
    # against each plan run alone on one lane
    def six(plan, seed):
        for i in range(6):
            _philox(plan, i, seed=seed)

    a = _plan(ctx, monkeypatch, 2, seed=21)
    b = _plan(ctx, monkeypatch, 2, seed=22)
    try:
        for i in range(6):
            _philox(a, i, seed=7)
            _philox(b, i, seed=8)
        got = [_rec(a, H), _rec(b, H)]
    finally:
        a.close()
        b.close()
    want = []
    for pts_seed, seed in ((21, 7), (22, 8)):
        plan = _plan(ctx, monkeypatch, 1, seed=pts_seed)
        try:
            six(plan, seed)
            want.append(_rec(plan, H))
        finally:
            plan.close()
    assert got[0] == want[0]
    assert got[1] == want[1]


@pytest.mark.parametrize("n,h", [(8, 1), (9, 65)])
def test_edge_shapes(ctx, monkeypatch, n, h):
    def body(plan):
        out = []
        for i in range(5):
            plan.run(h, mode=_ffi.SAMPLER_PHILOX, seed=9, hyp_offset=i * h)
        out.append(_rec(plan, h))
        for i in range(5):
            plan.run(h, mode=_ffi.SAMPLER_PHILOX, seed=9, hyp_offset=(5 + i) * h)
            out.append(plan.result()[1].tolist())
        return out
    _both(ctx, monkeypatch, body, n=n, max_hyp=h)
