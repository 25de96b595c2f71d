"""GPU bundle adjustment at the camera counts where k_ba_chol, k_ba_final and k_ba_step of ba.hip
take another path: rs_bundle_adjust / rs_bundle_adjust_rigid / rs_bundle_adjust_robust against
oracle/tables_ref.bundle_adjust_lm, tests/ba_rigid_ref.py and tests/ba_robust_ref.py on closed
rings of 22 .. 128 cameras (ba_rigid_fixture.large_ring).  tests/test_ba_shapes_cpu.py proves
from the kernel's constants which branch each count reaches: 22 / 23 (12 parameters) and 43 / 44
(rigid) are one and two passes over the 240-column LDS tile, 45 / 88 (rigid) the second panel row
per thread, 88 (12 parameters) the second iteration over `base`, 128 the cap.

Runs.  3 linearisations up to 45 cameras, 1 at 88 and 128 (the oracle takes 1.0 s and 3.4 s a
linearisation there, the rigid reference 0.7 s and 2.2 s).  Everything is compared as
test_gpu_ba_rigid._assert_steps does: iterations and status equal, the step of the cameras and
of the points relative to the largest step component, the cost to 1e-9 relative, and for rigid
cameras max |R^T R - I| <= 1e-12.

Bars.  Rigid: STEP_BAR = 1e-8; the reference's Schur route and its dense solve differ by at most
1.3e-12 (cameras) and 1.0e-12 (points) on these rings (2.6e-12 / 2.5e-12 on the chain of short
tracks), and under a 1e-13 relative perturbation of the start points the reference moves by at
most 1.3e-12 / 1.2e-12, the cost by 7.7e-14; the bar keeps the factor of 1000 and more.
12 parameters: with only camera 0 fixed a projective gauge remains and the ring is far worse
conditioned than the Dino fixtures.  Under the same perturbation the oracle's own one-step camera
step moves by 1.4e-10 (22), 2.4e-10 (23), 6.0e-10 (45), 2.4e-9 (88) and 8.4e-10 (128), its point
step by 2.1e-12 .. 1.8e-10, its cost by at most 2.3e-12.  So the bar is measured against the
oracle, never against the GPU: per shape max(STEP_BAR, MOVE_FACTOR x the oracle's own move of a
one-linearisation run), cameras and points each with their own move, MOVE_FACTOR = 100 as in
test_gpu_ba_rigid.py.  That gives camera bars of 1.4e-8 .. 2.4e-7 and point bars of 1e-8 (1.8e-8
at 88 cameras).  A skipped tile pass or a dropped panel row is an error of 5e-2 or more of the
step (shown once by cutting the tile loop to one pass and the rows per thread to one in scratch
builds: DESIGN.md section 10), five orders of magnitude above every bar.

Further cases.  A 128-camera chain of tracks of 2 .. 4 views, where 7624 of the 8128 pair lists
of k_ba_schur are empty (the rings have tracks of every length and no empty list).  Camera 20
and point 30 of a 46-camera problem unobserved: the rest bit for bit the 45-camera ring.  Two
calls at 128 cameras bit-equal.  129 cameras refused by all three entry points before a kernel
runs.  Cauchy on the dirty 44-camera ring (ba_run<6, true>), the bars of test_gpu_ba_robust.py.

Measured on an MI355X ("Limits", has the table), camera / point step error
and relative cost.  12 parameters: 22 4.1e-11 / 9.6e-12, 2.3e-14; 23 2.8e-11 / 5.5e-12, 1.1e-14;
45 5.4e-11 / 9.1e-12, 1.7e-14; 88 1.0e-9 / 7.0e-11, 1.5e-12; 128 5.4e-10 / 1.0e-11, 1.1e-12: at
least 150 times below their bars.  Rigid: 43 2.2e-13 / 4.0e-14, 5.4e-15; 44 3.7e-13 / 1.0e-13,
3.7e-14; 88 7.7e-13 / 7.9e-14, 1.8e-15; 128 1.3e-12 / 1.6e-13, 3.7e-14; short tracks 2.9e-12 /
2.4e-12, 3.8e-13.  Cauchy: 7.1e-13 / 1.2e-14, cost 2.1e-15, weights 1.1e-12.
"""
import numpy as np
import pytest

import ba_rigid_fixture as rf
import ba_robust_fixture as xf
import ba_robust_ref as br
import ba_rigid_ref as rr
from oracle import tables_ref as tr
from tsbb15_amd import _ffi
from tsbb15_amd import tables as gt

pytestmark = pytest.mark.gpu

STEP_BAR = 1e-8
WEIGHT_BAR = 1e-8
MOVE_FACTOR = 100.0
PERTURBATION = 1e-13
# cameras -> linearisations
FREE12 = {22: 3, 23: 3, 45: 3, 88: 1, 128: 1}
RIGID = {43: 3, 44: 3, 88: 1, 128: 1}
assert tuple(FREE12) == rf.LARGE_FREE12 and tuple(RIGID) == rf.LARGE_RIGID
CASES = [("free12", n) for n in FREE12] + [("rigid", n) for n in RIGID]
CASE_IDS = [f"{m}-{n}" for m, n in CASES]
_cache = {}


def _start(model, nC, perturbed=False):
    """(cams0, pts0), read-only; perturbed: the points moved by 1e-13 relative."""
    key = ("start", model, nC, perturbed)
    if key not in _cache:
        P = rf.large_ring(nC)
        c0, p0 = xf.start(P, 1e-3, model == "rigid")
        if perturbed:
            p0 = p0 * (1.0 + PERTURBATION * np.random.RandomState(5000).standard_normal(p0.shape))
        c0.setflags(write=False)
        p0.setflags(write=False)
        _cache[key] = (c0, p0)
    return _cache[key]


def _ref(model, nC, iterations, perturbed=False):
    """The reference's (cams, pts, info) for that start, computed once and never modified."""
    key = ("ref", model, nC, iterations, perturbed)
    if key not in _cache:
        P = rf.large_ring(nC)
        c0, p0 = _start(model, nC, perturbed)
        lm = rr.bundle_adjust_rigid_lm if model == "rigid" else tr.bundle_adjust_lm
        c, p, info = lm(c0, p0, P["ov"], P["op"], P["uv"][:, 0], P["uv"][:, 1], max_iter=iterations)
        c.setflags(write=False)
        p.setflags(write=False)
        _cache[key] = (c, p, info)
    return _cache[key]


def _gpu(model, nC, iterations):
    """The GPU's (cams, pts, info) for the unperturbed start, computed once."""
    key = ("gpu", model, nC, iterations)
    if key not in _cache:
        P = rf.large_ring(nC)
        c0, p0 = _start(model, nC)
        adjust = gt.bundle_adjust_rigid if model == "rigid" else gt.bundle_adjust
        _cache[key] = adjust(c0, p0, P["ov"], P["op"], P["uv"], max_iter=iterations)
    return _cache[key]


def _step_error(new, old, ref_new):
    step, ref = new - old, ref_new - old
    return np.abs(step - ref).max() / np.abs(ref).max()


def _own_move(model, nC):
    """How far the reference's own one-linearisation step moves (cameras, points, of the largest
    step component; cost, relative) under the perturbation of the start points."""
    (ca, pa, ia), (cb, pb, ib) = _ref(model, nC, 1), _ref(model, nC, 1, perturbed=True)
    c0, p0 = _start(model, nC)
    return (_step_error(cb, c0, ca), _step_error(pb, p0, pa),
            abs(ia["cost"] - ib["cost"]) / ia["cost"])


# ------------------------------------------------------------------------------------------
# 1. parity at every named shape
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model,nC", CASES, ids=CASE_IDS)
def test_steps_match_reference(ctx, model, nC):
    iterations = (RIGID if model == "rigid" else FREE12)[nC]
    c0, p0 = _start(model, nC)
    cr, pr, iref = _ref(model, nC, iterations)
    if model == "rigid":
        bar_c = bar_p = STEP_BAR
        moved = ""
    else:
        mc, mp, mcost = _own_move(model, nC)
        bar_c, bar_p = max(STEP_BAR, MOVE_FACTOR * mc), max(STEP_BAR, MOVE_FACTOR * mp)
        moved = f"; the oracle's own move {mc:.2e} / {mp:.2e}, cost {mcost:.2e}"
    c1, p1, info = _gpu(model, nC, iterations)
    ec, ep = _step_error(c1, c0, cr), _step_error(p1, p0, pr)
    rel = abs(info["cost"] - iref["cost"]) / iref["cost"]
    print(f"{model} {nC} cameras, {iterations} iteration(s): camera step error {ec:.3e} (bar "
          f"{bar_c:.2e}), point step error {ep:.3e} (bar {bar_p:.2e}), cost rel {rel:.2e}, "
          f"rejected {info['rejected']}{moved}")
    assert info["iterations"] == iterations == iref["iterations"]
    assert info["status"] == 0 == iref["status"]
    assert ec < bar_c and ep < bar_p, (ec, ep)
    assert info["cost"] == pytest.approx(iref["cost"], rel=1e-9)
    assert info["cost_init"] == pytest.approx(iref["cost_init"], rel=1e-12)
    assert c1[0].tobytes() == c0[0].tobytes()
    if model == "rigid":
        assert info["rejected"] == iref["rejected"]
        assert rf.rotation_defect(c1) <= 1e-12


# ------------------------------------------------------------------------------------------
# 2. most pair blocks empty
# ------------------------------------------------------------------------------------------
def test_short_tracks_leave_most_pair_blocks_empty(ctx):
    """128 rigid cameras in a chain of tracks of 2 .. 4 views: 7624 of the 8128 pair blocks of
    k_ba_schur have no observation pair and must come out as zeros; the long-track rings above
    have none of those."""
    P = rf.short_track_ring(128)
    ov, op, uv = P["ov"], P["op"], P["uv"]
    c0, p0 = rf.rigid_start(P, 1e-3)
    cr, pr, iref = rr.bundle_adjust_rigid_lm(c0, p0, ov, op, uv[:, 0], uv[:, 1], max_iter=1)
    c1, p1, info = gt.bundle_adjust_rigid(c0, p0, ov, op, uv, max_iter=1)
    ec, ep = _step_error(c1, c0, cr), _step_error(p1, p0, pr)
    rel = abs(info["cost"] - iref["cost"]) / iref["cost"]
    print(f"short tracks, 128 rigid cameras: camera step error {ec:.3e}, point step error "
          f"{ep:.3e}, cost rel {rel:.2e}, rejected {info['rejected']} ({iref['rejected']})")
    assert info["iterations"] == 1 == iref["iterations"] and info["status"] == 0 == iref["status"]
    assert info["rejected"] == iref["rejected"]
    assert ec < STEP_BAR and ep < STEP_BAR, (ec, ep)
    assert info["cost"] == pytest.approx(iref["cost"], rel=1e-9)
    assert rf.rotation_defect(c1) <= 1e-12


# ------------------------------------------------------------------------------------------
# 3. gaps in the slot map, read beyond lane 512
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", ["free12", "rigid"])
def test_unobserved_camera_and_point_in_the_middle_stay_out(ctx, model):
    """45 cameras plus camera 20 and point 30 without an observation: the rest must do bit for
    bit what it does without them (cam_of_slot skips 20; with 12 parameters the scatter of the
    528 camera steps reads it beyond lane 512), and the two come back as they went in."""
    P = rf.large_ring(45)
    ov, op, uv = P["ov"], P["op"], P["uv"]
    c0, p0 = _start(model, 45)
    base_c, base_p, base_info = _gpu(model, 45, 3)
    junk = np.array([[[-0.0, 1.5, 2.5, 3.5], [0.1, -0.0, 7.0, 1e-300], [3.0, 2.0, -1.0, 0.25]]])
    cx = np.concatenate([c0[:20], junk, c0[20:]])
    px = np.vstack([p0[:30], [-0.0, 0.1234567, -9.5], p0[30:]])
    ovx = (ov + (ov >= 20)).astype(np.int32)
    opx = (op + (op >= 30)).astype(np.int32)
    adjust = gt.bundle_adjust_rigid if model == "rigid" else gt.bundle_adjust
    c1, p1, info = adjust(cx, px, ovx, opx, uv, max_iter=3)
    assert c1[20].tobytes() == cx[20].tobytes() and p1[30].tobytes() == px[30].tobytes()
    assert np.delete(c1, 20, axis=0).tobytes() == base_c.tobytes()
    assert np.delete(p1, 30, axis=0).tobytes() == base_p.tobytes()
    assert info == base_info
    assert not np.array_equal(base_c[21], c0[21])


# ------------------------------------------------------------------------------------------
# 4. determinism at the cap
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", ["free12", "rigid"])
def test_bitwise_reproducible_at_128_cameras(ctx, model):
    P = rf.large_ring(128)
    c0, p0 = _start(model, 128)
    a = _gpu(model, 128, 1)
    adjust = gt.bundle_adjust_rigid if model == "rigid" else gt.bundle_adjust
    b = adjust(c0, p0, P["ov"], P["op"], P["uv"], max_iter=1)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    assert a[2] == b[2]
    assert not np.array_equal(a[0][127], c0[127]) and not np.array_equal(a[1], p0)


# ------------------------------------------------------------------------------------------
# 5. one camera above the cap
# ------------------------------------------------------------------------------------------
def test_129_cameras_raise_before_any_kernel():
    """A valid ring of 129 cameras: ValueError from all three entry points, and nothing was
    launched: a timed context still shows the sums of the call before (a call that gets as far
    as its first kernel has cleared them)."""
    P = rf.ring_problem(129, 131)
    ov, op, uv = P["ov"], P["op"], P["uv"]
    assert len(np.unique(ov)) == 129 == _ffi.BA_MAX_CAMERAS + 1
    Q = rf.large_ring(22)
    own = _ffi.Context()
    try:
        _ffi.ba_timing(own, 1)
        c0, p0 = _start("rigid", 22)
        gt.bundle_adjust_rigid(c0, p0, Q["ov"], Q["op"], Q["uv"], max_iter=1, ctx=own)
        before = _ffi.ba_timing(own, 1)
        assert before[1] >= 1 and before[0][_ffi.BA_KERNELS[-1]] > 0.0
        calls = [lambda c, p: gt.bundle_adjust(c, p, ov, op, uv, ctx=own),
                 lambda c, p: gt.bundle_adjust_rigid(c, p, ov, op, uv, ctx=own)]
        for rigid in (False, True):
            for loss in ("soft_l1", "huber", "cauchy"):
                adjust = gt.bundle_adjust_rigid if rigid else gt.bundle_adjust
                calls.append(lambda c, p, adjust=adjust, loss=loss: adjust(
                    c, p, ov, op, uv, ctx=own, loss=loss, f_scale=xf.F_SCALE))
        for rigid, call in zip([False, True] + 3 * [False] + 3 * [True], calls):
            c0, p0 = xf.start(P, 1e-3, rigid)
            with pytest.raises(ValueError, match="RS_BA_MAX_CAMERAS"):
                call(c0, p0)
            assert _ffi.ba_timing(own, 1) == before
        # and the context still works afterwards
        c0, p0 = _start("rigid", 22)
        again = gt.bundle_adjust_rigid(c0, p0, Q["ov"], Q["op"], Q["uv"], max_iter=1, ctx=own)
        assert again[2]["iterations"] == 1 and _ffi.ba_timing(own, 0)[1] == before[1]
    finally:
        own.close()


# ------------------------------------------------------------------------------------------
# 6. the robust instantiation past one tile
# ------------------------------------------------------------------------------------------
def test_cauchy_rigid_44_cameras(ctx):
    """ba_run<6, true> with two passes over the Cholesky tile, on the dirty 44-camera ring; the
    bars of test_gpu_ba_robust.py."""
    P = xf.dirty_ring(44, rf.LARGE_RINGS[44][0])
    ov, op, uv = P["ov"], P["op"], P["uv"]
    assert len(ov) == rf.LARGE_RINGS[44][1] and 0.02 < P["bad"].mean() < 0.1
    c0, p0 = rf.rigid_start(P, 1e-3)
    kw = dict(loss="cauchy", f_scale=xf.F_SCALE)
    cr, pr, iref = br.bundle_adjust_robust_lm(c0, p0, ov, op, uv[:, 0], uv[:, 1], rigid=True,
                                              max_iter=3, **kw)
    c1, p1, info = gt.bundle_adjust_rigid(c0, p0, ov, op, uv, max_iter=3, **kw)
    ec, ep = _step_error(c1, c0, cr), _step_error(p1, p0, pr)
    rel = abs(info["cost"] - iref["cost"]) / iref["cost"]
    dw = np.abs(info["weights"] - iref["weights"]).max()
    print(f"cauchy, 44 rigid cameras, 3 iterations: camera step error {ec:.3e}, point step error "
          f"{ep:.3e}, cost rel {rel:.2e}, weights {dw:.2e} (range {info['weights'].min():.1e} .. "
          f"{info['weights'].max():.3f}), rejected {info['rejected']} ({iref['rejected']})")
    assert info["iterations"] == 3 == iref["iterations"]
    assert info["status"] == 0 == iref["status"]
    assert set(info) == set(iref)
    assert ec < STEP_BAR and ep < STEP_BAR, (ec, ep)
    assert rel < 1e-9, rel
    assert dw < WEIGHT_BAR, dw
    assert info["cost_init"] == pytest.approx(iref["cost_init"], rel=1e-12)
    assert rf.rotation_defect(c1) <= 1e-12
