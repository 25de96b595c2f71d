"""The wash step without a GPU: the facts of tests/wash_fixture.py pinned on the numpy
reference tests/wash_ref.py alone, the payoff for the bundle adjustment that follows it
(oracle.tables_ref.bundle_adjust_lm), and the bookkeeping of tsbb15_amd.tables.wash with a stub
in place of the kernel.

Fixture facts, measured with wash_ref at (nC, nP, seed) = (6, 40, 3), (12, 120, 4), (8, 64, 5):
clean table: nothing removed, largest final error 6.5e-8 .. 1.4e-7 (squared; 2.5e-4 .. 3.7e-4
in length) against t^2 = 1e-6.  With the displacements: every observation of every track of
length >= 4 classified exactly (0 mismatches); the only removed points are 2-view tracks with a
displaced observation (3, 4, 3 of them).  A 2-view track whose displacement lies along the
epipolar line is kept at a wrong depth -- two views cannot detect it -- so truth is not tested
there.  Payoff on 6 x 40: the washed table starts BA at 6.1e-9 per kept observation and ends at
4.3e-9 (sigma^2 = 1e-8); the dirty table still stands at 1.1e-5 per observation after 60
linearisations.
"""
import numpy as np
import pytest

import wash_fixture as wf
import wash_ref as wr
from oracle import tables_ref as tr
from tsbb15_amd import tables as gt

CASES = [(6, 40, 3), (12, 120, 4), (8, 64, 5)]
_cache = {}


def _ref(case, displaced=True, scale=1.0):
    """(table, reference result), computed once and never modified."""
    key = (case, displaced, scale)
    if key not in _cache:
        W = wf.table(*case, displaced=displaced)
        res = wr.wash_points(W["cams"], W["pts0"], W["ov"], W["op"], W["uv"],
                             W["thresh"] * scale)
        for a in res[:4]:
            a.setflags(write=False)
        _cache[key] = (W, res)
    return _cache[key]


@pytest.mark.parametrize("case", CASES)
def test_clean_table_loses_nothing(case):
    W, (pts, obs_keep, point_keep, err2, info) = _ref(case, displaced=False)
    print(f"clean {case}: largest final error {np.sqrt(err2.max()):.2e}, info {info}")
    assert obs_keep.all() and point_keep.all()
    assert info["obs_removed"] == 0 == info["points_removed"] == info["points_failed"]
    assert err2.max() < 0.25 * W["thresh"] ** 2


@pytest.mark.parametrize("case", CASES)
def test_displaced_observations_are_found_exactly(case):
    W, (pts, obs_keep, point_keep, err2, info) = _ref(case)
    long = W["track_len"] >= 4
    mism = int((obs_keep[long] == W["bad"][long]).sum())
    lens = np.bincount(W["op"], minlength=len(pts))
    print(f"displaced {case}: {mism} mismatches of {int(long.sum())}, removed tracks "
          f"{lens[~point_keep]}, info {info}")
    assert mism == 0
    # only 2-view tracks with a displaced observation lose their point
    assert np.all(lens[~point_keep] == 2)
    for j in np.flatnonzero(~point_keep):
        assert W["bad"][W["op"] == j].any()
    kept_long = point_keep & (lens >= 4)
    assert np.linalg.norm(pts[kept_long] - W["pts"][kept_long], axis=1).max() < 2e-3
    assert info["points_removed"] == int((~point_keep).sum())
    assert info["obs_removed"] == int((~obs_keep).sum())


@pytest.mark.parametrize("case", CASES + [(16, 60, 6)])
def test_masks_are_stable_around_the_threshold(case):
    """The condition every fixture of a GPU mask comparison must satisfy."""
    _, (_, ok0, pk0, _, _) = _ref(case)
    for scale in (1.0 - 1e-6, 1.0 + 1e-6):
        _, (_, ok, pk, _, _) = _ref(case, scale=scale)
        assert np.array_equal(ok, ok0) and np.array_equal(pk, pk0)


@pytest.mark.parametrize("nC", wf.RING_EDGES)
def test_ring_masks_are_stable_around_the_threshold(nC):
    """The same condition for the rings of tests/test_gpu_wash.py whose tracks lie around the
    wave width, and what that test asserts of the GPU, here of the reference alone: exactly the
    15 displaced observations removed, every point kept, every pair a hypothesis."""
    cams, truth, pts0, ov, op, uv, bad = wf.ring(nC)
    res = {s: wr.wash_points(cams, pts0, ov, op, uv, wf.THRESH * s)
           for s in (1.0, 1.0 - 1e-6, 1.0 + 1e-6)}
    pts, ok0, pk0, err2, info = res[1.0]
    for s in (1.0 - 1e-6, 1.0 + 1e-6):
        assert np.array_equal(res[s][1], ok0) and np.array_equal(res[s][2], pk0)
    assert np.array_equal(ok0, ~bad) and bad.sum() == 15 and pk0.all()
    assert info["hypotheses"] == 3 * nC * (nC - 1) // 2 and info["obs_removed"] == 15
    ratio = err2 / wf.THRESH ** 2
    print(f"ring {nC}: {info['hypotheses']} hypotheses, final errors nearest to t^2 at factors "
          f"{ratio[ratio < 1].max():.3f} and {ratio[ratio >= 1].min():.1f}")
    assert ratio[ratio < 1].max() < 1 / 6 and ratio[ratio >= 1].min() > 6


def test_wash_pays_off_in_bundle_adjustment():
    W, (pts, obs_keep, point_keep, _, _) = _ref(CASES[0])
    ov, op, uv = W["ov"], W["op"], W["uv"]
    pmap = np.cumsum(point_keep) - 1
    k = obs_keep
    _, _, washed = tr.bundle_adjust_lm(W["cams"], pts[point_keep], ov[k], pmap[op[k]],
                                       uv[k, 0], uv[k, 1], max_iter=60)
    _, _, dirty = tr.bundle_adjust_lm(W["cams"], W["pts0"], ov, op, uv[:, 0], uv[:, 1],
                                      max_iter=60)
    nk, n = int(k.sum()), len(ov)
    print(f"washed: {washed['cost_init'] / nk:.2e} -> {washed['cost'] / nk:.2e} per kept "
          f"observation; dirty ends at {dirty['cost'] / n:.2e} per observation")
    assert washed["cost_init"] / nk <= 1e-7
    assert washed["cost"] / nk <= 1e-7
    assert dirty["cost"] / n > 1e-6


def test_binding_matches_the_header():
    import ctypes
    from tsbb15_amd import _ffi
    assert ctypes.sizeof(_ffi.WashInfo) == 24
    assert _ffi.WashInfo.obs_removed.offset == 8 and _ffi.WashInfo.points_failed.offset == 16
    header = open(_ffi.HEADER_PATH).read()
    assert f"#define RS_WASH_MAX_TRACK {_ffi.WASH_MAX_TRACK} " in header
    for name in ("rs_wash_points", "rs_triangulate_nview"):
        assert name in _ffi._SIGS and hasattr(_ffi.lib(), name)


# ------------------------------------------------------------------------------------------
# bookkeeping of wash(T, ...) with prescribed masks
# ------------------------------------------------------------------------------------------
def _stub(obs_keep, point_keep, new_pts):
    def wash_points(cams, pts, ov, op, uv, thresh, min_views=2, depth_sign=0, ctx=None):
        info = dict(hypotheses=7, obs_removed=int((~obs_keep).sum()),
                    points_removed=int((~point_keep).sum()), points_failed=0)
        return new_pts.copy(), obs_keep.copy(), point_keep.copy(), np.zeros(len(ov)), info
    return wash_points


def test_wash_rewrites_the_table(monkeypatch):
    W = wf.table(4, 9, 0)
    T = wf.mini_tables(W)
    wf.check_table(T)
    ov, op = W["ov"], W["op"]
    n, nP = len(ov), len(W["pts0"])
    point_keep = np.ones(nP, bool)
    point_keep[[0, 4]] = False
    obs_keep = point_keep[op].copy()
    obs_keep[np.flatnonzero(op == 7)[0]] = False        # one observation of a kept point
    obs_keep[(ov == 2) & (op != 7)] = False             # view 2 loses (nearly) everything
    obs_keep[ov == 2] = False                           # ... everything
    new_pts = W["pts0"] + 1.0
    old_obs, old_pts, old_views = list(T.T_obs), list(T.T_points), list(T.T_views)
    old_coords = [o.image_coordinates.copy() for o in old_obs]
    monkeypatch.setattr(gt, "wash_points", _stub(obs_keep, point_keep, new_pts))
    info = gt.wash(T, 1e-3)

    assert info["hypotheses"] == 7 and info["points_removed"] == 2
    assert len(T.T_views) == 4 and list(T.T_views) == old_views      # views never leave
    # survivors keep their relative order and are the same objects
    assert list(T.T_obs) == [o for o, k in zip(old_obs, obs_keep) if k]
    assert list(T.T_points) == [p for p, k in zip(old_pts, point_keep) if k]
    pm, om = info["point_map"], info["obs_map"]
    assert np.array_equal(pm >= 0, point_keep) and np.array_equal(om >= 0, obs_keep)
    assert np.array_equal(pm[point_keep], np.arange(point_keep.sum()))
    assert np.array_equal(om[obs_keep], np.arange(obs_keep.sum()))
    for i in np.flatnonzero(obs_keep):
        o = T.T_obs[om[i]]
        assert o is old_obs[i]
        assert o.point_3D_index == pm[op[i]] and o.view_index == ov[i]
        assert np.array_equal(o.image_coordinates, old_coords[i])
    for j in np.flatnonzero(point_keep):
        assert np.array_equal(T.T_points[pm[j]].point, new_pts[j])
        own = np.flatnonzero(obs_keep & (op == j))
        assert np.array_equal(T.T_points[pm[j]].observations_index, np.r_[0, om[own]])
    for v in range(4):
        own = np.flatnonzero(obs_keep & (ov == v))
        assert np.array_equal(T.T_views[v].observations_index, np.r_[0, om[own]])
    assert np.array_equal(T.T_views[2].observations_index, [0])       # left with nothing
    wf.check_table(T)


def test_wash_with_nothing_removed_changes_only_the_points(monkeypatch):
    W = wf.table(4, 9, 1)
    T = wf.mini_tables(W)
    before = [np.array(r.observations_index) for r in list(T.T_views) + list(T.T_points)]
    n, nP = len(W["ov"]), len(W["pts0"])
    monkeypatch.setattr(gt, "wash_points", _stub(np.ones(n, bool), np.ones(nP, bool), W["pts"]))
    info = gt.wash(T, 1e-3, min_views=3, depth_sign=-1)
    after = [np.array(r.observations_index) for r in list(T.T_views) + list(T.T_points)]
    assert all(np.array_equal(a, b) for a, b in zip(before, after))
    assert np.array_equal(info["obs_map"], np.arange(n))
    assert np.array_equal(info["point_map"], np.arange(nP))
    assert np.array_equal(np.array([p.point for p in T.T_points]), W["pts"])
    assert [o.point_3D_index for o in T.T_obs] == list(W["op"])
    wf.check_table(T)
