"""The GPU bundle adjustment (tsbb15_amd.tables.bundle_adjust / BundleAdjustment2, rs_bundle_adjust
of ba.hip) against the CPU oracle oracle/tables_ref.bundle_adjust_lm, which
tests/test_oracle_tables.py pins to the reference's scipy result.

Problems come from tests/ba_fixture.py (the Dino scene of tests/golden/dino_pnp_kat.npz with a
sparse visibility pattern) and from the reference's own run in tests/golden/tables.npz.

Bars.  One step (and the 3-step run on the fully visible problem): the step must equal the
oracle's to 1e-8 of the largest step component -- the oracle's Schur route and a dense solve of
the same damped normal equations differ by 1.1e-11 / 7e-13 at condition number 5e6; the bar is
1000 times that.  Converged runs: the final cost within 1e-10 relative of the oracle's (the
oracle itself moves by 1e-14 .. 1.3e-13 under a 1e-13 perturbation of the start or a
permutation of the observations); costs are compared, not parameters, because a projective
gauge remains with only camera 0 fixed.  A cost recomputed from the same parameters (a sum of
at most a few thousand squares in another order) must agree to 1e-12 relative.
"""
import numpy as np
import pytest

import ba_fixture as bf
from conftest import golden
from oracle import tables_ref as tr
from tables_fixture import MiniTables, Pose
from tsbb15_amd import _ffi, cloud, dense, features
from tsbb15_amd import tables as gt

pytestmark = pytest.mark.gpu

STEP_BAR = 1e-8
COST_BAR = 1e-10
SIZES = {"5x40": (5, 40), "7x70": (7, 70)}
_cache = {}


def _problem(size):
    if size not in _cache:
        _cache[size] = bf.problem(*SIZES[size])
    return _cache[size]


def _oracle(key, cams0, pts0, ov, op, uv, **kw):
    """The oracle's (cams, pts, info), computed once per key and never modified."""
    if key not in _cache:
        c, p, info = tr.bundle_adjust_lm(cams0, pts0, ov, op, uv[:, 0], uv[:, 1], **kw)
        c.setflags(write=False)
        p.setflags(write=False)
        _cache[key] = (c, p, info)
    return _cache[key]


def _cost(cams, pts, ov, op, uv):
    r = tr.ba_residuals(cams, pts, ov, op, uv[:, 0], uv[:, 1])
    return 0.5 * float(r @ r)


def _step_error(new, old, ref_new):
    step, ref = new - old, ref_new - old
    return np.abs(step - ref).max() / np.abs(ref).max()


def _golden_problem(tag):
    z = golden("tables.npz")
    g = lambda k: z[f"{tag}_{k}"]
    nC, nP = int(g("ba_n_views")), int(g("ba_n_points"))
    x0 = g("ba_x0")
    return (x0[:12 * nC].reshape(nC, 3, 4).copy(), x0[12 * nC:].reshape(nP, 3).copy(),
            g("ba_obs_view").astype(np.int32), g("ba_obs_point").astype(np.int32),
            np.ascontiguousarray(g("ba_obs_coords")[:, :2]), float(g("ba_cost_final")))


# ------------------------------------------------------------------------------------------
# 1. one-step parity
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", list(SIZES))
def test_one_step_matches_oracle(ctx, size):
    P = _problem(size)
    ov, op, uv = P["ov"], P["op"], P["uv"]
    c0, p0 = bf.start(P, 1e-3)
    cr, pr, iref = _oracle((size, "step"), c0, p0, ov, op, uv, max_iter=1)
    c1, p1, info = gt.bundle_adjust(c0, p0, ov, op, uv, max_iter=1)
    ec, ep = _step_error(c1, c0, cr), _step_error(p1, p0, pr)
    print(f"one step {size}: camera step error {ec:.3e}, point step error {ep:.3e} "
          f"(of the largest step component)")
    assert info["iterations"] == 1 == iref["iterations"] and info["status"] == 0
    assert ec < STEP_BAR and ep < STEP_BAR, (ec, ep)
    assert info["cost"] == pytest.approx(iref["cost"], rel=1e-9)


# ------------------------------------------------------------------------------------------
# 2. convergence
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sigma", [1e-3, 5e-2])
@pytest.mark.parametrize("size", list(SIZES))
def test_converges_to_the_oracle_cost(ctx, size, sigma):
    P = _problem(size)
    ov, op, uv = P["ov"], P["op"], P["uv"]
    c0, p0 = bf.start(P, sigma)
    c0_in, p0_in = c0.copy(), p0.copy()
    _, _, iref = _oracle((size, sigma), c0, p0, ov, op, uv)
    c1, p1, info = gt.bundle_adjust(c0, p0, ov, op, uv)
    rel = abs(info["cost"] - iref["cost"]) / iref["cost"]
    print(f"convergence {size} sigma {sigma}: cost {info['cost']:.13e} oracle "
          f"{iref['cost']:.13e} rel {rel:.2e}; iterations {info['iterations']} "
          f"(oracle {iref['iterations']}), rejected {info['rejected']}, status {info['status']}")
    np.testing.assert_array_equal(c0, c0_in)          # the inputs are not modified
    np.testing.assert_array_equal(p0, p0_in)
    assert set(info) == set(iref) | {"rejected", "lambda"}
    assert rel < COST_BAR, rel
    assert info["cost_init"] == pytest.approx(iref["cost_init"], rel=1e-12)
    assert c1[0].tobytes() == c0[0].tobytes()
    assert _cost(c1, p1, ov, op, uv) == pytest.approx(info["cost"], rel=1e-12)
    assert info["status"] in (1, 2)
    assert info["cost"] < info["cost_init"]
    if sigma == 5e-2:
        assert info["rejected"] >= 1


# ------------------------------------------------------------------------------------------
# 3. the reference's own problem
# ------------------------------------------------------------------------------------------
def test_reference_problem_not_worse_than_scipy(ctx):
    c0, p0, ov, op, uv, cost_final = _golden_problem("noisy")
    _, _, iref = _oracle("golden_noisy", c0, p0, ov, op, uv)
    c1, p1, info = gt.bundle_adjust(c0, p0, ov, op, uv)
    rel = abs(info["cost"] - iref["cost"]) / iref["cost"]
    print(f"reference problem: cost {info['cost']:.13e} oracle {iref['cost']:.13e} rel {rel:.2e} "
          f"scipy {cost_final:.13e}")
    assert info["cost"] <= cost_final
    assert rel < COST_BAR, rel
    assert c1[0].tobytes() == c0[0].tobytes()


def test_reference_problem_already_converged(ctx):
    """clean_ba_*: the initial cost is 4e-23; nothing to gain, nothing may break."""
    c0, p0, ov, op, uv, _ = _golden_problem("clean")
    c1, p1, info = gt.bundle_adjust(c0, p0, ov, op, uv)
    assert np.isfinite(c1).all() and np.isfinite(p1).all()
    assert np.isfinite(info["cost"]) and info["cost"] <= info["cost_init"]
    assert info["cost_init"] < 1e-20


# ------------------------------------------------------------------------------------------
# 4. determinism and order
# ------------------------------------------------------------------------------------------
def test_bitwise_reproducible_and_order_independent(ctx):
    P = _problem("7x70")
    ov, op, uv = P["ov"], P["op"], P["uv"]
    c0, p0 = bf.start(P, 5e-2)
    a = gt.bundle_adjust(c0, p0, ov, op, uv)
    b = gt.bundle_adjust(c0, p0, ov, op, uv)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    assert a[2] == b[2]
    perm = np.random.RandomState(9).permutation(len(ov))
    c = gt.bundle_adjust(c0, p0, ov[perm], op[perm], uv[perm])
    rel = abs(c[2]["cost"] - a[2]["cost"]) / a[2]["cost"]
    print(f"permuted observations: cost moves by {rel:.2e} relative")
    assert rel < COST_BAR, rel


# ------------------------------------------------------------------------------------------
# 5. structure
# ------------------------------------------------------------------------------------------
def _with_extra_point(P, views, seed):
    """The 5x40 problem plus point 40, observed (with noise) by `views`."""
    rng = np.random.RandomState(seed)
    X = P["pts"].mean(axis=0) + 0.01 * rng.standard_normal(3)
    pts = np.vstack([P["pts"], X])
    xv = np.array(views, dtype=np.int32)
    xp = np.full(len(views), 40, dtype=np.int32)
    uvx = bf.project(P["cams"], pts, xv, xp) + 1e-4 * rng.standard_normal((len(views), 2))
    return pts, np.r_[P["ov"], xv], np.r_[P["op"], xp], np.vstack([P["uv"], uvx])


def test_unobserved_point_and_camera_stay_out(ctx):
    """The oracle cannot run here (V or S is singular); the observed part must do exactly what
    it does with the unobserved point and camera deleted."""
    P = _problem("5x40")
    ov, op, uv = P["ov"], P["op"], P["uv"]
    c0, p0 = bf.start(P, 1e-3)
    base_c, base_p, base_info = gt.bundle_adjust(c0, p0, ov, op, uv)
    cx = np.concatenate([c0, np.array([[[-0.0, 1.5, 2.5, 3.5], [0.1, -0.0, 7.0, 1e-300],
                                        [3.0, 2.0, -1.0, 0.25]]])])
    px = np.vstack([p0, [-0.0, 0.1234567, -9.5]])
    c1, p1, info = gt.bundle_adjust(cx, px, ov, op, uv)
    assert c1[5].tobytes() == cx[5].tobytes() and p1[40].tobytes() == px[40].tobytes()
    assert c1[:5].tobytes() == base_c.tobytes() and p1[:40].tobytes() == base_p.tobytes()
    assert info == base_info


@pytest.mark.parametrize("views", [(0, 2), (3,)], ids=["camera0_and_one_other", "single_obs"])
def test_weakly_observed_point(ctx, views):
    P = _problem("5x40")
    pts, ov, op, uv = _with_extra_point(P, views, seed=77)
    c0, _ = bf.start(P, 1e-3)
    p0 = pts + 1e-3 * np.random.RandomState(3).standard_normal(pts.shape)
    _, _, iref = _oracle(("extra", views), c0, p0, ov, op, uv)
    c1, p1, info = gt.bundle_adjust(c0, p0, ov, op, uv)
    rel = abs(info["cost"] - iref["cost"]) / iref["cost"]
    print(f"extra point seen by {views}: cost rel {rel:.2e}")
    assert rel < COST_BAR, rel
    assert c1[0].tobytes() == c0[0].tobytes()
    assert _cost(c1, p1, ov, op, uv) == pytest.approx(info["cost"], rel=1e-12)


def test_single_camera_refines_points_only(ctx):
    """nC == 1: camera 0 sees every point twice (two noisy observations)."""
    P = _problem("5x40")
    rng = np.random.RandomState(41)
    cams = P["cams"][:1].copy()
    ov = np.zeros(80, dtype=np.int32)
    op = np.tile(np.arange(40, dtype=np.int32), 2)
    uv = bf.project(cams, P["pts"], ov, op) + 1e-4 * rng.standard_normal((80, 2))
    p0 = P["pts"] + 1e-3 * rng.standard_normal(P["pts"].shape)
    _, _, iref = _oracle("nC1", cams, p0, ov, op, uv)
    c1, p1, info = gt.bundle_adjust(cams, p0, ov, op, uv)
    rel = abs(info["cost"] - iref["cost"]) / iref["cost"]
    print(f"nC == 1: cost rel {rel:.2e}")
    assert c1.tobytes() == cams.tobytes()
    assert rel < COST_BAR, rel
    assert info["cost_init"] == pytest.approx(iref["cost_init"], rel=1e-12)
    assert not np.array_equal(p1, p0)


def test_fully_visible_long_rows(ctx):
    """3 views x 676 points, all visible (2028 observations): camera rows longer than any
    workgroup, counts no multiple of 64."""
    key = "full"
    if key not in _cache:
        _cache[key] = bf.problem(3, 676, full=True)
    P = _cache[key]
    ov, op, uv = P["ov"], P["op"], P["uv"]
    c0, p0 = bf.start(P, 1e-3)
    cr, pr, iref = _oracle("full3", c0, p0, ov, op, uv, max_iter=3)
    c1, p1, info = gt.bundle_adjust(c0, p0, ov, op, uv, max_iter=3)
    ec, ep = _step_error(c1, c0, cr), _step_error(p1, p0, pr)
    print(f"3 x 676 fully visible, 3 iterations: camera step error {ec:.3e}, point step "
          f"error {ep:.3e}")
    assert info["iterations"] == iref["iterations"] == 3
    assert ec < STEP_BAR and ep < STEP_BAR, (ec, ep)
    assert info["cost"] == pytest.approx(iref["cost"], rel=1e-9)


# ------------------------------------------------------------------------------------------
# 6. errors
# ------------------------------------------------------------------------------------------
def test_bad_input_raises_value_error(ctx):
    P = _problem("5x40")
    ov, op, uv = P["ov"], P["op"], P["uv"]
    c0, p0 = bf.start(P, 1e-3)
    for bad_ov in (np.r_[ov[:-1], 5], np.r_[ov[:-1], -1]):
        with pytest.raises(ValueError):
            gt.bundle_adjust(c0, p0, bad_ov.astype(np.int32), op, uv)
    for bad_op in (np.r_[op[:-1], 40], np.r_[op[:-1], -1]):
        with pytest.raises(ValueError):
            gt.bundle_adjust(c0, p0, ov, bad_op.astype(np.int32), uv)
    with pytest.raises(ValueError):
        gt.bundle_adjust(c0, p0, ov[:-1], op, uv)
    with pytest.raises(ValueError):
        gt.bundle_adjust(c0, p0, ov, op, uv[:-1])
    with pytest.raises(ValueError):
        gt.bundle_adjust(c0, p0, ov[:0], op[:0], uv[:0])
    nan_uv = uv.copy()
    nan_uv[17, 1] = np.nan
    with pytest.raises(ValueError):
        gt.bundle_adjust(c0, p0, ov, op, nan_uv)
    with pytest.raises(ValueError):
        gt.bundle_adjust(np.zeros((129, 3, 4)), p0, ov, op, uv)   # above the camera cap
    # and the context still works afterwards
    assert gt.bundle_adjust(c0, p0, ov, op, uv, max_iter=1)[2]["iterations"] == 1


# ------------------------------------------------------------------------------------------
# 7. drop-in
# ------------------------------------------------------------------------------------------
def test_bundle_adjustment2_on_a_table(ctx):
    z = golden("tables.npz")
    g = lambda k: z[f"noisy_{k}"]
    c0, p0, ov, op, uv, cost_final = _golden_problem("noisy")
    T = MiniTables(g("K"))
    for v in range(len(c0)):
        T.addView(v, Pose(c0[v, :, :3].copy(), c0[v, :, 3].copy()))
    for p in p0:
        T.addPoint(p.copy())
    for c, v, p in zip(g("ba_obs_coords"), g("ba_obs_view"), g("ba_obs_point")):
        T.addObs(c.copy(), int(v), int(p))
    info = gt.BundleAdjustment2(T)
    assert info["cost"] <= cost_final
    assert all(isinstance(v.camera_pose, Pose) for v in T.T_views)
    np.testing.assert_array_equal(T.T_views[0].camera_pose.GetCameraMatrix(), c0[0])
    assert not np.array_equal(T.T_views[1].camera_pose.GetCameraMatrix(), c0[1])
    pts = np.array([p.point for p in T.T_points])
    assert pts.shape == p0.shape and not np.array_equal(pts, p0)
    cams = np.array([v.camera_pose.GetCameraMatrix() for v in T.T_views])
    assert _cost(cams, pts, ov, op, uv) == pytest.approx(info["cost"], rel=1e-12)
    # the table is still a table: the next view registers on it
    n_views = T.T_views.size
    gt.add_new_view(T, g("K"), 2, g("match_queries"), g("match_y2_hom"), g("match_y1"),
                    g("match_y2"))
    assert T.T_views.size == n_views + 1


# ------------------------------------------------------------------------------------------
# rs_ba_timing
# ------------------------------------------------------------------------------------------
def test_timing_slots():
    """The sums per kernel start at 0; a timed call fills them and counts its trials; the next
    timed call starts from zero again; a call after disabling changes nothing; timed and
    untimed results are bit-equal.  A context of its own, so that no earlier call has timed."""
    P = _problem("5x40")
    ov, op, uv = P["ov"], P["op"], P["uv"]
    c0, p0 = bf.start(P, 1e-3)
    run = lambda it: gt.bundle_adjust(c0, p0, ov, op, uv, max_iter=it, ctx=own)
    cost = _ffi.BA_KERNELS[-1]
    own = _ffi.Context()
    try:
        plain = run(3)
        assert _ffi.ba_timing(own, 1) == (dict.fromkeys(_ffi.BA_KERNELS, 0.0), 0)
        timed = run(3)
        ms, trials = _ffi.ba_timing(own, 1)
        print("3 iterations:", ms, trials)
        assert trials >= 1 and ms[cost] > 0.0
        assert all(np.isfinite(v) and 0.0 <= v < 1e3 for v in ms.values())
        # the same call again: the same trials, not the two calls' together
        run(3)
        assert _ffi.ba_timing(own, 1)[1] == trials
        # no iteration at all: only the first cost is timed, nothing of the calls before stays
        run(0)
        ms0, trials0 = _ffi.ba_timing(own, 0)
        print("0 iterations:", ms0, trials0)
        assert trials0 == 0 and 0.0 < ms0[cost] < 1e3
        assert all(v == 0.0 for k, v in ms0.items() if k != cost)
        again = run(3)
        assert _ffi.ba_timing(own, 0) == (ms0, trials0)
        for a, b, c in zip(plain[:2], timed[:2], again[:2]):
            assert a.tobytes() == b.tobytes() == c.tobytes()
        assert plain[2] == timed[2] == again[2]
    finally:
        own.close()


def test_context_with_every_timer_enabled_is_destroyed():
    P = _problem("5x40")
    c0, p0 = bf.start(P, 1e-3)
    own = _ffi.Context()
    _ffi.pnp_timing(own, 1)
    _ffi.ba_timing(own, 1)
    features.timing(1, ctx=own)
    cloud.timing(1, ctx=own)
    dense.timing(1, ctx=own)
    gt.bundle_adjust(c0, p0, P["ov"], P["op"], P["uv"], max_iter=1, ctx=own)   # BA's events exist
    own.close()
    with pytest.raises(RuntimeError):
        own.handle
