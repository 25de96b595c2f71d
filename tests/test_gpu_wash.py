"""The GPU wash step (tsbb15_amd.tables.wash_points / triangulate_nview / wash, rs_wash_points
and rs_triangulate_nview of wash.hip) against its numpy restatement tests/wash_ref.py, against
ground truth, and through a table into BundleAdjustment2.

Tables come from tests/wash_fixture.py; every one used for a mask comparison satisfies the
stability condition of tests/test_wash_cpu.py (the reference's masks are identical at
thresh (1 +- 1e-6)), and no final e_i of (6, 40, 3), (12, 120, 4) or (16, 60, 6) lies within a
factor 1 +- 0.05 of t^2.

Bars.  Masks, point_keep and the hypothesis count must be equal.  Kept points: 1e-8 absolute.
The reference's own variation, measured with numpy on (12, 120, 4): 2.8e-10 when its last refit
starts 1e-4 away, 2.7e-10 with every track reversed (the LM stops where a step gains less than
1e-15 of the cost); the bar is about 30 times that and is not to be widened.  err2: 1e-6
relative + 1e-8 t^2 absolute where finite, NaN in the same places.

Measured on the MI355X, GPU against the reference: kept points differ by 3.7e-11 (6x40),
2.7e-10 (12x120), 6.0e-11 (16x60), 6.3e-12 (the three 128-view tracks), 1.7e-11 / 1.9e-11 /
2.1e-11 / 1.2e-15 (the tracks of 63 / 64 / 65 / 127 views, err2 at most 0.059 of its bar);
triangulate_nview on the clean 12x120 by 6.0e-10; err2 at most 0.69 of its bar (12x120).  Kept
points of tracks >= 4 lie within 6.7e-4 / 1.0e-3 / 5.8e-4 of truth.  End to end on 6x40: 27
observations and 3 points removed, then BundleAdjustment2 from 6.1e-9 to 4.3e-9 per kept
observation.
"""
import numpy as np
import pytest

import wash_fixture as wf
import wash_ref as wr
from tsbb15_amd import _ffi
from tsbb15_amd import tables as gt

pytestmark = pytest.mark.gpu

POINT_BAR = 1e-8
CASES = {"6x40": (6, 40, 3), "12x120": (12, 120, 4), "16x60": (16, 60, 6)}
_cache = {}


def _table(name, displaced=True):
    key = ("table", name, displaced)
    if key not in _cache:
        _cache[key] = wf.table(*CASES[name], displaced=displaced)
    return _cache[key]


def _ref(key, fn, *args, **kw):
    """A reference result, computed once per key and never modified."""
    if key not in _cache:
        res = fn(*args, **kw)
        for a in res:
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _cache[key] = res
    return _cache[key]


def _args(W):
    return W["cams"], W["pts0"], W["ov"], W["op"], W["uv"]


def _compare(gpu, ref, t2, what):
    pts, ok, pk, e2, info = gpu
    rpts, rok, rpk, re2, rinfo = ref
    assert ok.dtype == bool and pk.dtype == bool
    np.testing.assert_array_equal(ok, rok)
    np.testing.assert_array_equal(pk, rpk)
    assert info == rinfo, (info, rinfo)
    np.testing.assert_array_equal(np.isnan(e2), np.isnan(re2))
    fin = np.isfinite(re2)
    assert np.array_equal(np.isfinite(e2), fin)
    dp = np.abs(pts[pk] - rpts[pk]).max() if pk.any() else 0.0
    de = (np.abs(e2[fin] - re2[fin]) / (1e-6 * np.abs(re2[fin]) + 1e-8 * t2)).max() \
        if fin.any() else 0.0
    print(f"{what}: kept points differ by {dp:.2e} (bar {POINT_BAR:.0e}); err2 at {de:.2e} of "
          f"its bar; info {info}")
    assert dp <= POINT_BAR, dp
    assert de <= 1.0, de


# ------------------------------------------------------------------------------------------
# 1. parity with the reference
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_parity_with_reference(ctx, name):
    W = _table(name)
    ref = _ref(("wash", name), wr.wash_points, *_args(W), W["thresh"])
    pts0_in = W["pts0"].copy()
    gpu = gt.wash_points(*_args(W), W["thresh"], ctx=ctx)
    _compare(gpu, ref, W["thresh"] ** 2, f"parity {name}")
    np.testing.assert_array_equal(W["pts0"], pts0_in)          # the inputs are not modified
    assert gpu[0][~gpu[2]].tobytes() == W["pts0"][~gpu[2]].tobytes()


@pytest.mark.parametrize("name", ["6x40", "12x120"])
def test_parity_on_the_clean_table(ctx, name):
    W = _table(name, displaced=False)
    ref = _ref(("wash-clean", name), wr.wash_points, *_args(W), W["thresh"])
    gpu = gt.wash_points(*_args(W), W["thresh"], ctx=ctx)
    _compare(gpu, ref, W["thresh"] ** 2, f"clean {name}")
    assert gpu[1].all() and gpu[2].all()


# ------------------------------------------------------------------------------------------
# 2. ground truth
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_ground_truth(ctx, name):
    W = _table(name)
    pts, ok, pk, e2, info = gt.wash_points(*_args(W), W["thresh"], ctx=ctx)
    long = W["track_len"] >= 4
    assert np.array_equal(ok[long], ~W["bad"][long])
    lens = np.bincount(W["op"], minlength=len(pts))
    kept_long = pk & (lens >= 4)
    assert kept_long.sum() == (lens >= 4).sum()
    d = np.linalg.norm(pts[kept_long] - W["pts"][kept_long], axis=1).max()
    print(f"truth {name}: kept points of tracks >= 4 within {d:.2e} of truth")
    assert d < 2e-3


# ------------------------------------------------------------------------------------------
# 3. triangulate_nview
# ------------------------------------------------------------------------------------------
def test_triangulate_nview_matches_reference(ctx):
    W = _table("12x120", displaced=False)
    rpts, rok = _ref(("nview", "12x120"), wr.triangulate_nview, *_args(W))
    pts, ok = gt.triangulate_nview(*_args(W), ctx=ctx)
    assert ok.dtype == bool and ok.all() and rok.all()
    d = np.abs(pts - rpts).max()
    print(f"nview 12x120: differs from the reference by {d:.2e}; "
          f"{np.linalg.norm(pts - W['pts'], axis=1).max():.2e} from truth")
    assert d <= POINT_BAR


def test_triangulate_nview_leaves_a_single_observation_alone(ctx):
    W = _table("6x40", displaced=False)
    cams, pts0, ov, op, uv = _args(W)
    pts0 = np.vstack([pts0, [[0.1, 0.2, 0.3]], [[0.4, 0.5, 0.6]]])
    ov = np.r_[ov, 2].astype(np.int32)
    op = np.r_[op, 40].astype(np.int32)                       # point 40: one, point 41: none
    uv = np.vstack([uv, [[0.01, 0.02]]])
    pts, ok = gt.triangulate_nview(cams, pts0, ov, op, uv, ctx=ctx)
    assert ok[:40].all() and not ok[40] and not ok[41]
    assert pts[40:].tobytes() == pts0[40:].tobytes()
    rpts, rok = wr.triangulate_nview(cams, pts0, ov, op, uv)
    assert np.array_equal(ok, rok) and np.abs(pts - rpts).max() <= POINT_BAR


# ------------------------------------------------------------------------------------------
# 4. the longest track
# ------------------------------------------------------------------------------------------
def test_longest_track(ctx):
    assert _ffi.WASH_MAX_TRACK == 128
    cams, truth, pts0, ov, op, uv, bad = wf.ring(128)
    pts, ok, pk, e2, info = gt.wash_points(cams, pts0, ov, op, uv, 1e-3, ctx=ctx)
    assert np.array_equal(ok, ~bad) and pk.all()
    assert info["hypotheses"] == 3 * 8128 and info["obs_removed"] == 15
    assert np.linalg.norm(pts - truth, axis=1).max() < 2e-3
    ref = _ref(("ring",), wr.wash_points, cams, pts0, ov, op, uv, 1e-3)
    _compare((pts, ok, pk, e2, info), ref, 1e-6, "ring 128")
    with pytest.raises(ValueError):                            # a 129th observation
        gt.wash_points(cams, pts0, np.r_[ov, 0].astype(np.int32), np.r_[op, 1].astype(np.int32),
                       np.vstack([uv, [[0.0, 0.0]]]), 1e-3, ctx=ctx)
    with pytest.raises(ValueError):
        gt.triangulate_nview(cams, pts0, np.r_[ov, 0].astype(np.int32),
                             np.r_[op, 1].astype(np.int32), np.vstack([uv, [[0.0, 0.0]]]),
                             ctx=ctx)


@pytest.mark.parametrize("nC", wf.RING_EDGES)
def test_track_lengths_around_the_wave_width(ctx, nC):
    """The pair walk of the 64-lane class (ordinal p on lane p % 64, `while (b >= m)`) with a
    track one short of the wave, equal to it, one past it and one short of two waves: a lane
    then crosses no row, one row or several rows of the pair triangle in one stride."""
    cams, truth, pts0, ov, op, uv, bad = wf.ring(nC)
    gpu = gt.wash_points(cams, pts0, ov, op, uv, wf.THRESH, ctx=ctx)
    ref = _ref(("ring", nC), wr.wash_points, cams, pts0, ov, op, uv, wf.THRESH)
    _compare(gpu, ref, wf.THRESH ** 2, f"ring {nC}")
    pts, ok, pk, e2, info = gpu
    assert np.array_equal(ok, ~bad) and pk.all()
    assert info["hypotheses"] == 3 * nC * (nC - 1) // 2


# ------------------------------------------------------------------------------------------
# 5. depth_sign
# ------------------------------------------------------------------------------------------
def test_depth_sign(ctx):
    W = _table("6x40")
    zero = gt.wash_points(*_args(W), W["thresh"], depth_sign=0, ctx=ctx)
    neg = gt.wash_points(*_args(W), W["thresh"], depth_sign=-1, ctx=ctx)
    for a, b in zip(zero[:4], neg[:4]):                       # depths are negative in this data
        assert a.tobytes() == b.tobytes()
    assert zero[4] == neg[4]
    pts, ok, pk, e2, info = gt.wash_points(*_args(W), W["thresh"], depth_sign=1, ctx=ctx)
    assert not ok.any() and not pk.any() and np.isnan(e2).all()
    assert info["points_removed"] == 40 == info["points_failed"]
    assert info["obs_removed"] == len(ok) and info["hypotheses"] == zero[4]["hypotheses"]
    assert pts.tobytes() == W["pts0"].tobytes()


# ------------------------------------------------------------------------------------------
# 6. structure
# ------------------------------------------------------------------------------------------
def test_points_with_too_few_observations(ctx):
    W = _table("6x40")
    cams, pts0, ov, op, uv = _args(W)
    # point 40: none; 41: one; 42: two in the same view; 43: three, two of them in one view
    pts0 = np.vstack([pts0, W["pts"][:4]])
    eo = np.array([41, 42, 42, 43, 43, 43])
    ev = np.array([1, 3, 3, 0, 2, 2])
    y = wf.bf.project(cams, W["pts"][:4], ev, eo - 40)
    ov, op = np.r_[ov, ev].astype(np.int32), np.r_[op, eo].astype(np.int32)
    uv = np.vstack([uv, y])
    gpu = gt.wash_points(cams, pts0, ov, op, uv, W["thresh"], ctx=ctx)
    ref = wr.wash_points(cams, pts0, ov, op, uv, W["thresh"])
    _compare(gpu, ref, W["thresh"] ** 2, "few observations")
    pts, ok, pk, e2, info = gpu
    base = gt.wash_points(*_args(W), W["thresh"], ctx=ctx)
    assert list(pk[40:]) == [False, False, False, True]
    assert not ok[op == 41].any() and not ok[op == 42].any() and ok[op == 43].all()
    assert np.isnan(e2[(op == 41) | (op == 42)]).all()
    assert pts[40:43].tobytes() == pts0[40:43].tobytes()
    assert info["points_failed"] == base[4]["points_failed"] + 3
    assert info["hypotheses"] == base[4]["hypotheses"] + 2    # the same-view pairs give none
    assert np.array_equal(ok[:len(base[1])], base[1])


def test_min_views(ctx):
    W = _table("6x40")
    two = gt.wash_points(*_args(W), W["thresh"], min_views=2, ctx=ctx)
    three = gt.wash_points(*_args(W), W["thresh"], min_views=3, ctx=ctx)
    ref = _ref(("wash-mv3", "6x40"), wr.wash_points, *_args(W), W["thresh"], min_views=3)
    _compare(three, ref, W["thresh"] ** 2, "min_views 3")
    n_in = np.bincount(W["op"], weights=two[1], minlength=40)
    assert (two[2] & (n_in == 2)).any()
    assert np.array_equal(three[2], two[2] & (n_in >= 3))
    assert np.array_equal(three[1], two[1] & three[2][W["op"]])
    assert three[4]["points_failed"] == two[4]["points_failed"]
    assert three[0][~three[2]].tobytes() == W["pts0"][~three[2]].tobytes()


def test_nan_observation_leaves_alone(ctx):
    W = _table("12x120", displaced=False)
    cams, pts0, ov, op, uv = _args(W)
    j = int(np.flatnonzero(np.bincount(op) == 9)[0])
    i = int(np.flatnonzero(op == j)[4])
    uv = uv.copy()
    uv[i, 1] = np.nan
    pts, ok, pk, e2, info = gt.wash_points(cams, pts0, ov, op, uv, W["thresh"], ctx=ctx)
    assert pk.all() and info["obs_removed"] == 1 and not ok[i] and np.isnan(e2[i])
    assert np.isfinite(np.delete(e2, i)).all()
    ref = wr.wash_points(cams, pts0, ov, op, uv, W["thresh"])
    _compare((pts, ok, pk, e2, info), ref, W["thresh"] ** 2, "NaN observation")
    assert info["hypotheses"] == _ref(("wash-clean", "12x120"), wr.wash_points, *_args(W),
                                      W["thresh"])[4]["hypotheses"] - 8


def test_observation_order_between_points_does_not_matter(ctx):
    """Grouping the observations by point (a stable sort: every track keeps its own order, so
    every sum keeps its order) must not change one bit."""
    W = _table("12x120")
    cams, pts0, ov, op, uv = _args(W)
    order = np.argsort(op, kind="stable")
    assert not np.array_equal(order, np.arange(len(op)))
    a = gt.wash_points(cams, pts0, ov, op, uv, W["thresh"], ctx=ctx)
    b = gt.wash_points(cams, pts0, ov[order], op[order], uv[order], W["thresh"], ctx=ctx)
    assert a[0].tobytes() == b[0].tobytes() and a[2].tobytes() == b[2].tobytes()
    assert a[1][order].tobytes() == b[1].tobytes()
    assert a[3][order].tobytes() == b[3].tobytes()
    assert a[4] == b[4]
    pa, oka = gt.triangulate_nview(cams, pts0, ov, op, uv, ctx=ctx)
    pb, okb = gt.triangulate_nview(cams, pts0, ov[order], op[order], uv[order], ctx=ctx)
    assert pa.tobytes() == pb.tobytes() and np.array_equal(oka, okb)


def test_two_calls_give_the_same_bits(ctx):
    W = _table("16x60")
    a = gt.wash_points(*_args(W), W["thresh"], ctx=ctx)
    b = gt.wash_points(*_args(W), W["thresh"], ctx=ctx)
    for x, y in zip(a[:4], b[:4]):
        assert x.tobytes() == y.tobytes()
    assert a[4] == b[4]


# ------------------------------------------------------------------------------------------
# 7. errors
# ------------------------------------------------------------------------------------------
def test_errors(ctx):
    W = _table("6x40")
    cams, pts0, ov, op, uv = _args(W)
    t = W["thresh"]
    bad_ov, bad_op = ov.copy(), op.copy()
    bad_ov[3], bad_op[5] = 6, 40
    neg_ov, neg_op = ov.copy(), op.copy()
    neg_ov[0], neg_op[0] = -1, -1
    calls = [
        lambda: gt.wash_points(cams, pts0, bad_ov, op, uv, t, ctx=ctx),
        lambda: gt.wash_points(cams, pts0, ov, bad_op, uv, t, ctx=ctx),
        lambda: gt.wash_points(cams, pts0, neg_ov, op, uv, t, ctx=ctx),
        lambda: gt.wash_points(cams, pts0, ov, neg_op, uv, t, ctx=ctx),
        lambda: gt.wash_points(cams, pts0, ov[:-1], op, uv, t, ctx=ctx),
        lambda: gt.wash_points(cams, pts0, ov, op, uv[:-1], t, ctx=ctx),
        lambda: gt.wash_points(cams[:0], pts0, ov, op, uv, t, ctx=ctx),
        lambda: gt.wash_points(cams, pts0, ov[:0], op[:0], uv[:0], t, ctx=ctx),
        lambda: gt.wash_points(cams, pts0, ov, op, uv, 0.0, ctx=ctx),
        lambda: gt.wash_points(cams, pts0, ov, op, uv, -1e-3, ctx=ctx),
        lambda: gt.wash_points(cams, pts0, ov, op, uv, np.nan, ctx=ctx),
        lambda: gt.wash_points(cams, pts0, ov, op, uv, np.inf, ctx=ctx),
        lambda: gt.wash_points(cams, pts0, ov, op, uv, t, min_views=1, ctx=ctx),
        lambda: gt.wash_points(cams, pts0, ov, op, uv, t, depth_sign=2, ctx=ctx),
        lambda: gt.wash_points(cams, pts0, ov, op, uv, t, depth_sign=-2, ctx=ctx),
        lambda: gt.triangulate_nview(cams, pts0, bad_ov, op, uv, ctx=ctx),
        lambda: gt.triangulate_nview(cams, pts0, ov, bad_op, uv, ctx=ctx),
        lambda: gt.triangulate_nview(cams, pts0, ov[:-1], op, uv, ctx=ctx),
        lambda: gt.triangulate_nview(cams[:0], pts0, ov, op, uv, ctx=ctx),
        lambda: gt.triangulate_nview(cams, pts0, ov[:0], op[:0], uv[:0], ctx=ctx),
    ]
    for k, call in enumerate(calls):
        try:
            call()
        except ValueError:
            continue
        pytest.fail(f"call {k} raised no ValueError")


# ------------------------------------------------------------------------------------------
# 8. end to end: wash, then the bundle adjustment
# ------------------------------------------------------------------------------------------
def test_wash_then_bundle_adjustment(ctx):
    W = _table("6x40")
    T = wf.mini_tables(W)
    info = gt.wash(T, W["thresh"], ctx=ctx)
    wf.check_table(T)
    ref = _ref(("wash", "6x40"), wr.wash_points, *_args(W), W["thresh"])
    assert np.array_equal(info["obs_map"] >= 0, ref[1])
    assert np.array_equal(info["point_map"] >= 0, ref[2])
    assert len(T.T_obs) == ref[1].sum() and len(T.T_points) == ref[2].sum()
    assert len(T.T_views) == 6
    ba = gt.BundleAdjustment2(T, max_iter=60, ctx=ctx)
    per = ba["cost"] / len(T.T_obs)
    print(f"end to end 6x40: {info['obs_removed']} observations and {info['points_removed']} "
          f"points removed; BA {ba['cost_init'] / len(T.T_obs):.2e} -> {per:.2e} per kept "
          f"observation in {ba['iterations']} linearisations")
    assert per <= 1e-7
    wf.check_table(T)
