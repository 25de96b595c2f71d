"""GPU bundle adjustment under a robust loss (rs_bundle_adjust_robust of ba.hip, the ``loss=`` /
``f_scale=`` keywords of tsbb15_amd.tables.bundle_adjust / bundle_adjust_rigid /
BundleAdjustment2 / BundleAdjustmentRigid) against its numpy restatement tests/ba_robust_ref.py,
which tests/test_ba_robust_cpu.py checks against finite differences, a dense solve and the two
linear references.

Shapes (dirty: ba_robust_fixture, wash_fixture's displacement rule).  2x20: one free camera.
4x30: three free cameras, an odd count, a padded rigid system.  7x70.  Ring 42x60, rigid: 246
columns padded to 252, one full 240-column Cholesky tile (the second pass over the tile is run by
tests/test_gpu_ba_large.py, 44 cameras).  3x676 fully visible: camera rows longer than the
256-observation LDS tile, so the weights of k_ba_camera<6, true> are staged over three tiles.

Bars.  Steps (max_iter 1 and 3, start sigma 1e-3, f_scale 3e-4): STEP_BAR = 1e-8 of the largest
step component, cost 1e-9 relative, weights 1e-8 absolute, the bars of test_gpu_ba_rigid.py;
under a 1e-13 perturbation of the start the reference itself moves by at most 4.8e-14 in cost and
3.2e-11 in weights over 3 iterations (dirty 7x70, both models, three losses).  Converged Cauchy on
wash_fixture.table: cost within COST_BAR = 1e-10 relative (the reference's own move is at most
1.8e-14), R, the scale-fixed t and the weights within 100 times the reference's own move for that
table (ba_robust_fixture.own_move, the larger over two draws: R 7.9e-10 .. 6.5e-9, t 1.5e-9 ..
1.1e-8, weights 1.7e-7 .. 3.0e-7).  Huber and soft-L1 get no converged test on dirty tables (the
reference is still moving after 200 linearisations there); on the clean 7x70 problem the
reference's own move is 6.6e-14 (soft_l1) and 7.9e-14 (huber) in cost, below 1e-12, so one
converged run each is held to COST_BAR.

Huber's kink.  The step cases the issue sets (start sigma 1e-3, f_scale 3e-4) were to assert
first that each branch, z <= 1 and z > 1, holds at least 10 % of the observations at the start.
It does not: a start 1e-3 off leaves 0.1 % .. 7.5 % of the observations inside z <= 1 (2x20 2.5 /
7.5 %, 4x30 3.3 %, 7x70 2.3 %, ring 0.1 %, 3x676 1.4 %; rigid / 12-parameter where they differ).
The kink is still exercised by those cases, at the later linearisations of the 3-iteration runs:
the weights of linearisations 2 and 3 find 27 .. 64 % and 60 .. 86 % inside.  So the assertion is
made where Huber weights are formed with both branches in play: at linearisations 2 and 3 of every
3-iteration case, and at the start of an added one-step case per shape from a start 1e-4 off
(18 .. 65 % inside).  The start fractions of the sigma 1e-3 cases are printed.

Measured on an MI355X ("Robust loss", has the table).  The 54 step cases:
camera / point step error at most 7.4e-11 / 8.1e-13, cost 1.7e-13, weights 3.1e-12; Huber from
1e-4 off: 3.8e-12 / 3.4e-13, 1.5e-14, 1.8e-12.  Converged Cauchy: cost 1.1e-14 / 5.3e-15 / 6.8e-15
/ 5.1e-15 relative (4x30 s0, 6x40 s0, 7x70 s0, 7x70 s1); dR / dt / weights 2.7e-9 / 1.5e-9 /
9.9e-8, 5.6e-9 / 9.8e-9 / 1.5e-7, 3.0e-11 / 1.9e-11 / 1.6e-10, 7.9e-10 / 1.8e-9 / 3.0e-7 against
bars 2.7e-7 / 1.5e-7 / 2.0e-5, 6.5e-7 / 1.1e-6 / 1.7e-5, 1.9e-7 / 4.0e-7 / 1.8e-5, 7.9e-8 / 1.8e-7
/ 3.0e-5.  Clean 7x70: soft_l1 1.2e-13, huber 6.0e-14.  Downstream: the six masks equal, pose
errors those of the reference to four digits (worst 1.945e-2).  Permuted observations move the
cost by 7.1e-15 / 1.1e-14 and the 3-iteration weights by 8.9e-13 / 1.4e-12.
"""
import numpy as np
import pytest

import ba_fixture as bf
import ba_rigid_fixture as rf
import ba_robust_fixture as xf
import ba_robust_ref as br
import wash_fixture as wf
from oracle import tables_ref as tr
from tsbb15_amd import _ffi
from tsbb15_amd import tables as gt

pytestmark = pytest.mark.gpu

STEP_BAR = 1e-8
WEIGHT_BAR = 1e-8
COST_BAR = 1e-10
MOVE_FACTOR = 100.0
BRANCH_MIN = 0.10
ROBUST = ("soft_l1", "huber", "cauchy")
POSE_BAR, TABLES = xf.POSE_BAR, xf.TABLES
MODELS = {"free12": False, "rigid": True}
SHAPES = [("2x20", m) for m in MODELS] + [("4x30", m) for m in MODELS] + \
         [("7x70", m) for m in MODELS] + [("ring", "rigid")] + [("full", m) for m in MODELS]
SHAPE_IDS = [f"{s}-{m}" for s, m in SHAPES]
_cache = {}


def _problem(shape):
    if shape not in _cache:
        make = {"2x20": lambda: xf.dirty_problem(2, 20), "4x30": lambda: xf.dirty_problem(4, 30),
                "5x40": lambda: xf.dirty_problem(5, 40), "7x70": lambda: xf.dirty_problem(7, 70),
                "ring": xf.dirty_ring, "full": xf.dirty_full}[shape]
        _cache[shape] = make()
    return _cache[shape]


def _ref(key, c0, p0, P, **kw):
    """The reference's (cams, pts, info), computed once per key and never modified."""
    if key not in _cache:
        c, p, info = br.bundle_adjust_robust_lm(c0, p0, P["ov"], P["op"], P["uv"][:, 0],
                                                P["uv"][:, 1], **kw)
        for a in (c, p, info["weights"]):
            a.setflags(write=False)
        _cache[key] = (c, p, info)
    return _cache[key]


def _same_info(a, b):
    keys = set(a) | set(b)
    return all(np.array_equal(a[k], b[k]) if k == "weights" else a[k] == b[k] for k in keys)


def _raw(ctx, c0, p0, ov, op, uv, rigid, loss, f_scale, max_iter=200, ftol=1e-15):
    """rs_bundle_adjust_robust through ctypes: (cams, pts, info dict, weights)."""
    cams, pts = _ffi.f64c(c0).copy(), _ffi.f64c(p0).copy()
    ov, op = np.ascontiguousarray(ov, np.int32), np.ascontiguousarray(op, np.int32)
    uv = _ffi.f64c(uv)
    w = np.full(len(ov), np.nan)
    info = _ffi.BaInfo()
    d, i32 = _ffi.C.c_double, _ffi.C.c_int32
    _ffi.check(_ffi.lib().rs_bundle_adjust_robust(
        ctx.handle, _ffi.ptr(cams, d), len(cams), _ffi.ptr(pts, d), len(pts), _ffi.ptr(ov, i32),
        _ffi.ptr(op, i32), _ffi.ptr(uv, d), len(ov), max_iter, ftol, int(rigid), loss, f_scale,
        _ffi.ptr(w, d), _ffi.C.byref(info)))
    return cams, pts, {"cost_init": info.cost_init, "cost": info.cost,
                       "iterations": info.iterations, "status": info.status,
                       "rejected": info.rejected, "lambda": info.lam}, w


def _adjust(rigid):
    return gt.bundle_adjust_rigid if rigid else gt.bundle_adjust


def _step_error(new, old, ref_new):
    step, ref = new - old, ref_new - old
    return np.abs(step - ref).max() / np.abs(ref).max()


def _inside(P, cams, pts):
    """The share of the observations on Huber's quadratic branch, z <= 1."""
    r = tr.ba_residuals(cams, pts, P["ov"], P["op"], P["uv"][:, 0], P["uv"][:, 1])
    return float((br.z_of(r, xf.F_SCALE) <= 1.0).mean())


def _assert_steps(tag, got, start, ref, iterations, rigid):
    (c1, p1, info), (c0, p0), (cr, pr, iref) = got, start, ref
    ec, ep = _step_error(c1, c0, cr), _step_error(p1, p0, pr)
    rel = abs(info["cost"] - iref["cost"]) / iref["cost"]
    dw = np.abs(info["weights"] - iref["weights"]).max()
    print(f"{tag}: camera step error {ec:.3e}, point step error {ep:.3e} (of the largest step "
          f"component), cost rel {rel:.2e}, weights {dw:.2e} (range {info['weights'].min():.1e} .. "
          f"{info['weights'].max():.3f}), rejected {info['rejected']} (reference "
          f"{iref['rejected']})")
    assert info["iterations"] == iterations == iref["iterations"]
    assert info["status"] == 0 == iref["status"]
    assert set(info) == set(iref)
    assert ec < STEP_BAR and ep < STEP_BAR, (ec, ep)
    assert rel < 1e-9, rel
    assert dw < WEIGHT_BAR, dw
    assert info["cost_init"] == pytest.approx(iref["cost_init"], rel=1e-12)
    if rigid:
        assert rf.rotation_defect(c1) <= 1e-12


# ------------------------------------------------------------------------------------------
# 1. the linear loss is the old path, bit for bit
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", list(MODELS))
@pytest.mark.parametrize("size", [(5, 40), (7, 70)], ids=["5x40", "7x70"])
def test_linear_loss_is_bitwise_the_old_path(ctx, size, model):
    rigid = MODELS[model]
    P = bf.problem(*size)
    ov, op, uv = P["ov"], P["op"], P["uv"]
    c0, p0 = xf.start(P, 5e-2, rigid)
    old = _adjust(rigid)(c0, p0, ov, op, uv)
    cams, pts, info, w = _raw(ctx, c0, p0, ov, op, uv, rigid, 0, 0.37)
    assert cams.tobytes() == old[0].tobytes() and pts.tobytes() == old[1].tobytes()
    assert info == old[2] and "weights" not in old[2]
    assert np.all(w == 1.0)
    # and the keyword's default is that path
    kw = _adjust(rigid)(c0, p0, ov, op, uv, loss="linear", f_scale=2.0)
    assert kw[0].tobytes() == old[0].tobytes() and kw[1].tobytes() == old[1].tobytes()
    assert kw[2] == old[2]


# ------------------------------------------------------------------------------------------
# 2. step parity
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("iterations", [1, 3])
@pytest.mark.parametrize("loss", ROBUST)
@pytest.mark.parametrize("shape,model", SHAPES, ids=SHAPE_IDS)
def test_steps_match_reference(ctx, shape, model, loss, iterations):
    rigid = MODELS[model]
    P = _problem(shape)
    c0, p0 = xf.start(P, 1e-3, rigid)
    kw = dict(loss=loss, f_scale=xf.F_SCALE)
    refs = {k: _ref((shape, model, loss, k), c0, p0, P, rigid=rigid, max_iter=k, **kw)
            for k in ((1,) if iterations == 1 else (1, 2, 3))}
    if loss == "huber":
        # the kink: see the module docstring
        at = [_inside(P, c0, p0)] + [_inside(P, refs[k][0], refs[k][1]) for k in sorted(refs)][:-1]
        print(f"huber {shape} {model}: z <= 1 holds {', '.join(f'{100 * f:.1f} %' for f in at)} "
              f"of the observations at linearisation {', '.join(map(str, range(1, len(at) + 1)))}")
        for f in at[1:]:
            assert BRANCH_MIN <= f <= 1.0 - BRANCH_MIN, at
    got = _adjust(rigid)(c0, p0, P["ov"], P["op"], P["uv"], max_iter=iterations, **kw)
    _assert_steps(f"{loss} {shape} {model}, {iterations} iteration(s)", got, (c0, p0),
                  refs[iterations], iterations, rigid)


@pytest.mark.parametrize("shape,model", SHAPES, ids=SHAPE_IDS)
def test_huber_step_with_both_branches_at_the_start(ctx, shape, model):
    rigid = MODELS[model]
    P = _problem(shape)
    c0, p0 = xf.start(P, 1e-4, rigid)
    f = _inside(P, c0, p0)
    print(f"huber {shape} {model}, start 1e-4 off: z <= 1 holds {100 * f:.1f} % of the observations")
    assert BRANCH_MIN <= f <= 1.0 - BRANCH_MIN, f
    kw = dict(loss="huber", f_scale=xf.F_SCALE)
    ref = _ref((shape, model, "huber", "near"), c0, p0, P, rigid=rigid, max_iter=1, **kw)
    got = _adjust(rigid)(c0, p0, P["ov"], P["op"], P["uv"], max_iter=1, **kw)
    _assert_steps(f"huber {shape} {model} from 1e-4, one iteration", got, (c0, p0), ref, 1, rigid)


# ------------------------------------------------------------------------------------------
# 3. converged parity
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nC,nP,seed", [(4, 30, 0), (6, 40, 0), (7, 70, 0), (7, 70, 1)])
def test_cauchy_converges_to_the_reference(ctx, nC, nP, seed):
    W = wf.table(nC, nP, seed)
    ov, op, uv = W["ov"], W["op"], W["uv"]
    move = xf.own_move(W, 1e-3, "cauchy")
    cr, pr, iref = move["ref"]
    c0, p0 = rf.rigid_start(W, 1e-3)
    c1, p1, info = gt.bundle_adjust_rigid(c0, p0, ov, op, uv, loss="cauchy", f_scale=xf.F_SCALE)
    rel = abs(info["cost"] - iref["cost"]) / iref["cost"]
    a, b = rf.scale_fixed(c1, W["cams"]), rf.scale_fixed(cr, W["cams"])
    dR, dt = np.abs(a[:, :, :3] - b[:, :, :3]).max(), np.abs(a[:, :, 3] - b[:, :, 3]).max()
    dw = np.abs(info["weights"] - iref["weights"]).max()
    print(f"cauchy {nC}x{nP} s{seed}: cost {info['cost']:.13e} reference {iref['cost']:.13e} rel "
          f"{rel:.2e} (own move {move['cost']:.1e}); dR {dR:.2e} (bar "
          f"{MOVE_FACTOR * move['R']:.2e}), dt {dt:.2e} (bar {MOVE_FACTOR * move['t']:.2e}), "
          f"weights {dw:.2e} (bar {MOVE_FACTOR * move['weights']:.2e}); iterations "
          f"{info['iterations']} (reference {iref['iterations']}), rejected {info['rejected']} "
          f"({iref['rejected']}), status {info['status']} ({iref['status']})")
    assert rel < COST_BAR, rel
    assert dR <= MOVE_FACTOR * move["R"] and dt <= MOVE_FACTOR * move["t"], (dR, dt)
    assert dw <= MOVE_FACTOR * move["weights"], dw
    assert rf.rotation_defect(c1) <= 1e-12
    assert info["cost_init"] == pytest.approx(iref["cost_init"], rel=1e-12)
    assert info["status"] in (1, 2) and info["cost"] < info["cost_init"]
    # cost and weights are those of the returned state
    r = tr.ba_residuals(c1, p1, ov, op, uv[:, 0], uv[:, 1])
    cost, w = br.robust_cost(r, "cauchy", xf.F_SCALE)
    assert cost == pytest.approx(info["cost"], rel=1e-12)
    np.testing.assert_allclose(info["weights"], w, rtol=1e-9, atol=0)


@pytest.mark.parametrize("loss", ["soft_l1", "huber"])
def test_clean_table_converges_to_the_reference(ctx, loss):
    P = bf.problem(7, 70)
    move = xf.own_move(P, 1e-3, loss)
    iref = move["ref"][2]
    print(f"{loss} clean 7x70: the reference's own move in cost {move['cost']:.1e}")
    assert move["cost"] < 1e-12          # else COST_BAR would be a coin toss: see the docstring
    c0, p0 = rf.rigid_start(P, 1e-3)
    _, _, info = gt.bundle_adjust_rigid(c0, p0, P["ov"], P["op"], P["uv"], loss=loss,
                                        f_scale=xf.F_SCALE)
    rel = abs(info["cost"] - iref["cost"]) / iref["cost"]
    print(f"{loss} clean 7x70: cost {info['cost']:.13e} reference {iref['cost']:.13e} rel {rel:.2e}; "
          f"iterations {info['iterations']} (reference {iref['iterations']})")
    assert rel < COST_BAR, rel
    assert info["status"] in (1, 2)


# ------------------------------------------------------------------------------------------
# 4. downstream: Cauchy, then the wash
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nC,nP,seed", TABLES)
def test_cauchy_then_wash_gives_the_true_camera_mask(ctx, nC, nP, seed):
    W = wf.table(nC, nP, seed)
    ov, op, uv = W["ov"], W["op"], W["uv"]
    c0, p0 = rf.rigid_start(W, 1e-3)
    _, keep_true, *_ = gt.wash_points(W["cams"], p0, ov, op, uv, wf.THRESH)
    c1, p1, info = gt.bundle_adjust_rigid(c0, p0, ov, op, uv, loss="cauchy", f_scale=xf.F_SCALE)
    _, keep, *_ = gt.wash_points(c1, p1, ov, op, uv, wf.THRESH)
    eR, et = rf.pose_error(c1, W["cams"])
    print(f"{nC}x{nP} s{seed}: cauchy pose error R {eR:.3e} t {et:.3e}, {info['iterations']} "
          f"linearisations; the wash keeps {int(keep.sum())} of {len(keep)}, the wash at the true "
          f"cameras {int(keep_true.sum())}; {int((keep != keep_true).sum())} differ")
    assert np.array_equal(keep, keep_true)
    assert eR <= POSE_BAR and et <= POSE_BAR


def test_cauchy_then_wash_through_the_tables(ctx):
    W = wf.table(6, 40, 0)
    ov, op, uv = W["ov"], W["op"], W["uv"]
    _, keep_true, *_ = gt.wash_points(W["cams"], W["pts0"], ov, op, uv, wf.THRESH)
    T = wf.mini_tables(W)
    info = gt.BundleAdjustmentRigid(T, loss="cauchy", f_scale=xf.F_SCALE)
    assert info["weights"].shape == (len(ov),)
    cams = np.array([v.camera_pose.GetCameraMatrix() for v in T.T_views])
    eR, et = rf.pose_error(cams, W["cams"])
    out = gt.wash(T, wf.THRESH)
    wf.check_table(T)
    print(f"tables 6x40 s0: cauchy pose error R {eR:.3e} t {et:.3e}; the wash removes "
          f"{out['obs_removed']} observations, {int((~keep_true).sum())} at the true cameras")
    assert np.array_equal(out["obs_map"] >= 0, keep_true)
    assert len(T.T_obs) == int(keep_true.sum())
    assert eR <= POSE_BAR and et <= POSE_BAR
    # the displaced observations are the ones the loss switched off
    w = info["weights"]
    assert np.median(w[W["bad"]]) < 1e-2 and np.median(w[~W["bad"]]) > 0.5


# ------------------------------------------------------------------------------------------
# 5. determinism and structure
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", list(MODELS))
def test_bitwise_reproducible_and_order_independent(ctx, model):
    rigid = MODELS[model]
    P = _problem("7x70")
    ov, op, uv = P["ov"], P["op"], P["uv"]
    c0, p0 = xf.start(P, 1e-3, rigid)
    c0_in, p0_in, uv_in = c0.copy(), p0.copy(), uv.copy()
    kw = dict(loss="cauchy", f_scale=xf.F_SCALE)
    a = _adjust(rigid)(c0, p0, ov, op, uv, **kw)
    b = _adjust(rigid)(c0, p0, ov, op, uv, **kw)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    assert a[2]["weights"].tobytes() == b[2]["weights"].tobytes() and _same_info(a[2], b[2])
    for x, y in ((c0, c0_in), (p0, p0_in), (uv, uv_in)):       # the inputs are not modified
        np.testing.assert_array_equal(x, y)
    perm = np.random.RandomState(9).permutation(len(ov))
    c = _adjust(rigid)(c0, p0, ov[perm], op[perm], uv[perm], **kw)
    rel = abs(c[2]["cost"] - a[2]["cost"]) / a[2]["cost"]
    # the weights in the caller's order, where rounding has had 3 iterations to grow, not 30
    a3 = _adjust(rigid)(c0, p0, ov, op, uv, max_iter=3, **kw)
    c3 = _adjust(rigid)(c0, p0, ov[perm], op[perm], uv[perm], max_iter=3, **kw)
    dw = np.abs(c3[2]["weights"] - a3[2]["weights"][perm]).max()
    spread = np.abs(a3[2]["weights"] - a3[2]["weights"][perm]).max()
    print(f"permuted observations, {model}: cost moves by {rel:.2e} relative, weights after 3 "
          f"iterations by {dw:.2e} (against {spread:.2f} for the wrong order)")
    assert rel < COST_BAR, rel
    assert dw < WEIGHT_BAR < spread


@pytest.mark.parametrize("model", list(MODELS))
def test_unobserved_point_and_camera_stay_out(ctx, model):
    rigid = MODELS[model]
    P = _problem("5x40")
    ov, op, uv = P["ov"], P["op"], P["uv"]
    c0, p0 = xf.start(P, 1e-3, rigid)
    kw = dict(loss="cauchy", f_scale=xf.F_SCALE)
    base_c, base_p, base_info = _adjust(rigid)(c0, p0, ov, op, uv, **kw)
    cx = np.concatenate([c0, np.array([[[-0.0, 1.5, 2.5, 3.5], [0.1, -0.0, 7.0, 1e-300],
                                        [3.0, 2.0, -1.0, 0.25]]])])
    px = np.vstack([p0, [-0.0, 0.1234567, -9.5]])
    c1, p1, info = _adjust(rigid)(cx, px, ov, op, uv, **kw)
    assert c1[5].tobytes() == cx[5].tobytes() and p1[40].tobytes() == px[40].tobytes()
    assert c1[:5].tobytes() == base_c.tobytes() and p1[:40].tobytes() == base_p.tobytes()
    assert _same_info(info, base_info)


def test_single_camera_gives_the_same_bytes_for_both_models(ctx):
    P = _problem("5x40")
    rng = np.random.RandomState(41)
    cams = P["cams"][:1].copy()
    ov = np.zeros(80, dtype=np.int32)
    op = np.tile(np.arange(40, dtype=np.int32), 2)
    uv = bf.project(cams, P["pts"], ov, op) + 1e-4 * rng.standard_normal((80, 2))
    uv[::7] += 0.02
    p0 = P["pts"] + 1e-3 * rng.standard_normal(P["pts"].shape)
    for loss in ROBUST:
        a = gt.bundle_adjust(cams, p0, ov, op, uv, loss=loss, f_scale=xf.F_SCALE)
        b = gt.bundle_adjust_rigid(cams, p0, ov, op, uv, loss=loss, f_scale=xf.F_SCALE)
        assert b[0].tobytes() == cams.tobytes() == a[0].tobytes()
        assert b[1].tobytes() == a[1].tobytes() and not np.array_equal(b[1], p0)
        assert _same_info(a[2], b[2]) and a[2]["weights"].min() < 0.5


# ------------------------------------------------------------------------------------------
# 6. errors
# ------------------------------------------------------------------------------------------
def test_bad_input_raises_value_error(ctx):
    P = _problem("5x40")
    ov, op, uv = P["ov"], P["op"], P["uv"]
    c0, p0 = rf.rigid_start(P, 1e-3)
    for adjust in (gt.bundle_adjust, gt.bundle_adjust_rigid):
        with pytest.raises(ValueError, match="unknown loss"):
            adjust(c0, p0, ov, op, uv, loss="tukey")
        for bad in (0.0, -3e-4, np.nan, np.inf):
            with pytest.raises(ValueError, match="f_scale"):
                adjust(c0, p0, ov, op, uv, loss="cauchy", f_scale=bad)
    for rigid in (0, 1):
        with pytest.raises(ValueError, match="loss"):
            _raw(ctx, c0, p0, ov, op, uv, rigid, 4, xf.F_SCALE)
        with pytest.raises(ValueError, match="loss"):
            _raw(ctx, c0, p0, ov, op, uv, rigid, -1, xf.F_SCALE)
        for bad in (0.0, -3e-4, np.nan, np.inf):
            for loss in (0, 3):
                with pytest.raises(ValueError, match="f_scale"):
                    _raw(ctx, c0, p0, ov, op, uv, rigid, loss, bad)
    nan_uv = uv.copy()
    nan_uv[17, 1] = np.nan
    far_uv = uv.copy()
    far_uv[5, 0] = np.inf
    for loss in ROBUST:
        for bad_uv in (nan_uv, far_uv):           # a non-finite robust cost at the start
            with pytest.raises(ValueError, match="non-finite"):
                gt.bundle_adjust_rigid(c0, p0, ov, op, bad_uv, loss=loss, f_scale=xf.F_SCALE)
    scaled = c0.copy()
    scaled[2, :, :3] *= 1.001                     # the rigid model keeps its rotation check
    with pytest.raises(ValueError, match="camera 2"):
        gt.bundle_adjust_rigid(scaled, p0, ov, op, uv, loss="cauchy", f_scale=xf.F_SCALE)
    with pytest.raises(ValueError):
        gt.bundle_adjust_rigid(c0, p0, np.r_[ov[:-1], 5].astype(np.int32), op, uv, loss="huber")
    # and the context still works afterwards
    out = gt.bundle_adjust_rigid(c0, p0, ov, op, uv, max_iter=1, loss="cauchy", f_scale=xf.F_SCALE)
    assert out[2]["iterations"] == 1 and np.isfinite(out[2]["weights"]).all()
