"""The rigid-camera GPU bundle adjustment (tsbb15_amd.tables.bundle_adjust_rigid /
BundleAdjustmentRigid, rs_bundle_adjust_rigid of ba.hip) against its numpy restatement
tests/ba_rigid_ref.py, which tests/test_ba_rigid_cpu.py checks against finite differences and a
dense solve.

Shapes.  2x20: one free camera, a 6 x 6 system inside one 12-wide block column.  4x30: three
free cameras (odd: half a block column of padding).  5x40, 7x70: the shapes of
tests/test_gpu_ba.py.  ring 42x60: 41 free cameras, an odd count, 246 columns padded to 252; the
last block column starts at 240, exactly the end of the 240-column LDS tile of the Cholesky
panel, so the tile is filled once and never passed (tests/test_gpu_ba_large.py has the rings that
pass it).  3x676 fully visible: camera rows longer than an LDS tile.

Bars.  One step (and the 3-step runs): the step of the returned 3 x 4 cameras and of the points
within STEP_BAR = 1e-8 of the largest step component (the reference's Schur route and a dense
solve differ by 1.7e-13 / 6.5e-14), the cost to 1e-9 relative.  Converged runs: the cost within
COST_BAR = 1e-10 relative of the reference's (which itself moves by 2e-14 .. 1.3e-13 under a
1e-13 perturbation of the start); R and the scale-fixed t within 100 times the reference's own
move for that fixture, the larger over its two starts (tests/test_ba_rigid_cpu.py test 5:
4x30 9.4e-10 / 3.1e-10, 7x70 5.2e-10 / 5.5e-10): the GPU differs from the reference by
rounding of the size of that perturbation, and the accept / reject decisions near the minimum
diverge the same way.

Measured on an MI355X ("Rigid cameras", has the table).  One step, camera /
point step error: 2x20 1.7e-12 / 3.4e-13, 4x30 5.4e-13 / 1.7e-13, 5x40 6.9e-13 / 1.9e-13, 7x70
7.2e-13 / 2.6e-13; ring, 3 iterations 2.2e-13 / 6.0e-14; 3x676, 3 iterations 2.3e-12 / 1.5e-13;
costs within 8.1e-13.  Converged: cost 9.0e-14 / 5.9e-14 (4x30, sigma 1e-3 / 5e-2) and 2.0e-14 /
9.3e-15 (7x70) relative; dR / dt 1.4e-9 / 5.4e-10 and 4.6e-10 / 2.0e-10 against bars 9.4e-8 /
3.1e-8 (4x30), 1.3e-10 / 1.3e-10 and 2.9e-11 / 3.0e-11 against 5.2e-8 / 5.5e-8 (7x70);
max|R^T R - I| 1.1e-15 .. 1.8e-15.  Permuted observations move the cost by 3.5e-15.  The
reference's own problem ends at 1.1104691497772e-06 (scipy, 12 parameters: 1.1166393833202e-06).
"""
import numpy as np
import pytest

import ba_fixture as bf
import ba_rigid_fixture as rf
import ba_rigid_ref as rr
from conftest import golden
from oracle import tables_ref as tr
from tables_fixture import MiniTables, Pose
from tsbb15_amd import tables as gt

pytestmark = pytest.mark.gpu

STEP_BAR = 1e-8
COST_BAR = 1e-10
MOVE_FACTOR = 100.0
SIZES = {"2x20": (2, 20), "4x30": (4, 30), "5x40": (5, 40), "7x70": (7, 70)}
SIGMAS = (1e-3, 5e-2)
_cache = {}


def _problem(size):
    if size not in _cache:
        _cache[size] = bf.problem(*SIZES[size])
    return _cache[size]


def _ref(key, c0, p0, ov, op, uv, **kw):
    """The reference's (cams, pts, info), computed once per key and never modified."""
    if key not in _cache:
        c, p, info = rr.bundle_adjust_rigid_lm(c0, p0, ov, op, uv[:, 0], uv[:, 1], **kw)
        c.setflags(write=False)
        p.setflags(write=False)
        _cache[key] = (c, p, info)
    return _cache[key]


def _own_move(size):
    """Per start the reference's own move and converged result; the fixture's move is the larger."""
    key = ("move", size)
    if key not in _cache:
        per = {s: rf.own_move(_problem(size), s) for s in SIGMAS}
        _cache[key] = (per, max(m["R"] for m in per.values()), max(m["t"] for m in per.values()))
    return _cache[key]


def _cost(cams, pts, ov, op, uv):
    r = tr.ba_residuals(cams, pts, ov, op, uv[:, 0], uv[:, 1])
    return 0.5 * float(r @ r)


def _step_error(new, old, ref_new):
    step, ref = new - old, ref_new - old
    return np.abs(step - ref).max() / np.abs(ref).max()


def _assert_steps(tag, got, start, ref, iterations):
    (c1, p1, info), (c0, p0), (cr, pr, iref) = got, start, ref
    ec, ep = _step_error(c1, c0, cr), _step_error(p1, p0, pr)
    rel = abs(info["cost"] - iref["cost"]) / iref["cost"]
    print(f"{tag}: camera step error {ec:.3e}, point step error {ep:.3e} (of the largest step "
          f"component), cost rel {rel:.2e}, rejected {info['rejected']} (reference "
          f"{iref['rejected']})")
    assert info["iterations"] == iterations == iref["iterations"]
    assert info["status"] == 0 == iref["status"]
    assert ec < STEP_BAR and ep < STEP_BAR, (ec, ep)
    assert info["cost"] == pytest.approx(iref["cost"], rel=1e-9)
    assert rf.rotation_defect(c1) <= 1e-12


# ------------------------------------------------------------------------------------------
# 1. one-step parity
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", list(SIZES))
def test_one_step_matches_reference(ctx, size):
    P = _problem(size)
    ov, op, uv = P["ov"], P["op"], P["uv"]
    c0, p0 = rf.rigid_start(P, 1e-3)
    ref = _ref((size, "step"), c0, p0, ov, op, uv, max_iter=1)
    got = gt.bundle_adjust_rigid(c0, p0, ov, op, uv, max_iter=1)
    _assert_steps(f"one step {size}", got, (c0, p0), ref, 1)


# ------------------------------------------------------------------------------------------
# 2. convergence
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sigma", SIGMAS)
@pytest.mark.parametrize("size", ["4x30", "7x70"])
def test_converges_to_the_reference(ctx, size, sigma):
    P = _problem(size)
    ov, op, uv = P["ov"], P["op"], P["uv"]
    per, move_R, move_t = _own_move(size)
    cr, pr, iref = per[sigma]["ref"]
    c0, p0 = rf.rigid_start(P, sigma)
    c0_in, p0_in = c0.copy(), p0.copy()
    c1, p1, info = gt.bundle_adjust_rigid(c0, p0, ov, op, uv)
    rel = abs(info["cost"] - iref["cost"]) / iref["cost"]
    a, b = rf.scale_fixed(c1, P["cams"]), rf.scale_fixed(cr, P["cams"])
    dR, dt = np.abs(a[:, :, :3] - b[:, :, :3]).max(), np.abs(a[:, :, 3] - b[:, :, 3]).max()
    defect = rf.rotation_defect(c1)
    print(f"convergence {size} sigma {sigma}: cost {info['cost']:.13e} reference "
          f"{iref['cost']:.13e} rel {rel:.2e}; dR {dR:.2e} (bar {MOVE_FACTOR * move_R:.2e}), "
          f"dt {dt:.2e} (bar {MOVE_FACTOR * move_t:.2e}); max|RtR - I| {defect:.1e}; iterations "
          f"{info['iterations']} (reference {iref['iterations']}), rejected {info['rejected']} "
          f"({iref['rejected']}), status {info['status']}")
    np.testing.assert_array_equal(c0, c0_in)          # the inputs are not modified
    np.testing.assert_array_equal(p0, p0_in)
    assert set(info) == set(iref)
    assert rel < COST_BAR, rel
    assert dR <= MOVE_FACTOR * move_R and dt <= MOVE_FACTOR * move_t, (dR, dt)
    assert defect <= 1e-12 and np.linalg.det(c1[:, :, :3]).min() > 0
    assert info["cost_init"] == pytest.approx(iref["cost_init"], rel=1e-12)
    assert c1[0].tobytes() == c0[0].tobytes()
    assert _cost(c1, p1, ov, op, uv) == pytest.approx(info["cost"], rel=1e-12)
    assert info["status"] in (1, 2)
    assert info["cost"] < info["cost_init"]


# ------------------------------------------------------------------------------------------
# 3. determinism and structure
# ------------------------------------------------------------------------------------------
def test_bitwise_reproducible_and_order_independent(ctx):
    P = _problem("7x70")
    ov, op, uv = P["ov"], P["op"], P["uv"]
    c0, p0 = rf.rigid_start(P, 5e-2)
    a = gt.bundle_adjust_rigid(c0, p0, ov, op, uv)
    b = gt.bundle_adjust_rigid(c0, p0, ov, op, uv)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    assert a[2] == b[2]
    perm = np.random.RandomState(9).permutation(len(ov))
    c = gt.bundle_adjust_rigid(c0, p0, ov[perm], op[perm], uv[perm])
    rel = abs(c[2]["cost"] - a[2]["cost"]) / a[2]["cost"]
    print(f"permuted observations: cost moves by {rel:.2e} relative")
    assert rel < COST_BAR, rel


def test_unobserved_point_and_camera_stay_out(ctx):
    P = _problem("5x40")
    ov, op, uv = P["ov"], P["op"], P["uv"]
    c0, p0 = rf.rigid_start(P, 1e-3)
    base_c, base_p, base_info = gt.bundle_adjust_rigid(c0, p0, ov, op, uv)
    # the unobserved camera is no rotation: it is neither checked nor touched
    cx = np.concatenate([c0, np.array([[[-0.0, 1.5, 2.5, 3.5], [0.1, -0.0, 7.0, 1e-300],
                                        [3.0, 2.0, -1.0, 0.25]]])])
    px = np.vstack([p0, [-0.0, 0.1234567, -9.5]])
    c1, p1, info = gt.bundle_adjust_rigid(cx, px, ov, op, uv)
    assert c1[5].tobytes() == cx[5].tobytes() and p1[40].tobytes() == px[40].tobytes()
    assert c1[:5].tobytes() == base_c.tobytes() and p1[:40].tobytes() == base_p.tobytes()
    assert info == base_info


# ------------------------------------------------------------------------------------------
# 4. nC == 1: no free camera, the point arithmetic of bundle_adjust
# ------------------------------------------------------------------------------------------
def test_single_camera_equals_bundle_adjust_bitwise(ctx):
    P = _problem("5x40")
    rng = np.random.RandomState(41)
    cams = P["cams"][:1].copy()
    ov = np.zeros(80, dtype=np.int32)
    op = np.tile(np.arange(40, dtype=np.int32), 2)
    uv = bf.project(cams, P["pts"], ov, op) + 1e-4 * rng.standard_normal((80, 2))
    p0 = P["pts"] + 1e-3 * rng.standard_normal(P["pts"].shape)
    a = gt.bundle_adjust(cams, p0, ov, op, uv)
    b = gt.bundle_adjust_rigid(cams, p0, ov, op, uv)
    assert b[0].tobytes() == cams.tobytes() == a[0].tobytes()
    assert b[1].tobytes() == a[1].tobytes() and not np.array_equal(b[1], p0)
    assert a[2] == b[2]


# ------------------------------------------------------------------------------------------
# 5. 41 free cameras: an odd count, 246 columns padded to 252, and the last block column
#    starting exactly at the end of the Cholesky panel's LDS tile (one full tile, one pass)
# ------------------------------------------------------------------------------------------
def test_ring_of_42_cameras(ctx):
    if "ring" not in _cache:
        _cache["ring"] = rf.ring_problem(42, 60)
    P = _cache["ring"]
    ov, op, uv = P["ov"], P["op"], P["uv"]
    assert len(ov) == 1111 and len(np.unique(ov)) == 42 and rf.depths(P).min() > 0.2
    c0, p0 = rf.rigid_start(P, 1e-3)
    ref = _ref("ring3", c0, p0, ov, op, uv, max_iter=3)
    got = gt.bundle_adjust_rigid(c0, p0, ov, op, uv, max_iter=3)
    _assert_steps("ring 42 x 60, 3 iterations", got, (c0, p0), ref, 3)


# ------------------------------------------------------------------------------------------
# 6. camera rows longer than an LDS tile
# ------------------------------------------------------------------------------------------
def test_fully_visible_long_rows(ctx):
    if "full" not in _cache:
        _cache["full"] = bf.problem(3, 676, full=True)
    P = _cache["full"]
    ov, op, uv = P["ov"], P["op"], P["uv"]
    c0, p0 = rf.rigid_start(P, 1e-3)
    ref = _ref("full3", c0, p0, ov, op, uv, max_iter=3)
    got = gt.bundle_adjust_rigid(c0, p0, ov, op, uv, max_iter=3)
    _assert_steps("3 x 676 fully visible, 3 iterations", got, (c0, p0), ref, 3)


# ------------------------------------------------------------------------------------------
# 7. errors
# ------------------------------------------------------------------------------------------
def test_bad_input_raises_value_error(ctx):
    P = _problem("5x40")
    ov, op, uv = P["ov"], P["op"], P["uv"]
    c0, p0 = rf.rigid_start(P, 1e-3)
    scaled = c0.copy()
    scaled[2, :, :3] *= 1.001
    with pytest.raises(ValueError, match="camera 2"):
        gt.bundle_adjust_rigid(scaled, p0, ov, op, uv)
    mirrored = c0.copy()
    mirrored[3, 1, :3] *= -1.0
    with pytest.raises(ValueError, match="camera 3"):
        gt.bundle_adjust_rigid(mirrored, p0, ov, op, uv)
    for bad_ov in (np.r_[ov[:-1], 5], np.r_[ov[:-1], -1]):
        with pytest.raises(ValueError):
            gt.bundle_adjust_rigid(c0, p0, bad_ov.astype(np.int32), op, uv)
    for bad_op in (np.r_[op[:-1], 40], np.r_[op[:-1], -1]):
        with pytest.raises(ValueError):
            gt.bundle_adjust_rigid(c0, p0, ov, bad_op.astype(np.int32), uv)
    nan_uv = uv.copy()
    nan_uv[17, 1] = np.nan
    with pytest.raises(ValueError):
        gt.bundle_adjust_rigid(c0, p0, ov, op, nan_uv)
    with pytest.raises(ValueError):
        gt.bundle_adjust_rigid(np.zeros((129, 3, 4)), p0, ov, op, uv)   # above the camera cap
    # a non-rotation in camera 0 is not looked at: camera 0 is not free
    free0 = c0.copy()
    free0[0, :, :3] *= 1.001
    assert gt.bundle_adjust_rigid(free0, p0, ov, op, uv, max_iter=1)[0][0].tobytes() == \
        free0[0].tobytes()
    # and the context still works afterwards
    assert gt.bundle_adjust_rigid(c0, p0, ov, op, uv, max_iter=1)[2]["iterations"] == 1


# ------------------------------------------------------------------------------------------
# 8. drop-in
# ------------------------------------------------------------------------------------------
def test_bundle_adjustment_rigid_on_a_table(ctx):
    z = golden("tables.npz")
    g = lambda k: z[f"noisy_{k}"]
    nC, nP = int(g("ba_n_views")), int(g("ba_n_points"))
    x0 = g("ba_x0")
    c0, p0 = x0[:12 * nC].reshape(nC, 3, 4).copy(), x0[12 * nC:].reshape(nP, 3).copy()
    ov, op = g("ba_obs_view").astype(np.int32), g("ba_obs_point").astype(np.int32)
    uv = np.ascontiguousarray(g("ba_obs_coords")[:, :2])
    cost_final = float(g("ba_cost_final"))
    T = MiniTables(g("K"))
    for v in range(len(c0)):
        T.addView(v, Pose(c0[v, :, :3].copy(), c0[v, :, 3].copy()))
    for p in p0:
        T.addPoint(p.copy())
    for c, v, p in zip(g("ba_obs_coords"), g("ba_obs_view"), g("ba_obs_point")):
        T.addObs(c.copy(), int(v), int(p))
    info = gt.BundleAdjustmentRigid(T)
    print(f"reference problem, rigid: cost {info['cost']:.13e} scipy (12 parameters) "
          f"{cost_final:.13e}")
    assert info["cost"] <= cost_final
    assert all(isinstance(v.camera_pose, Pose) for v in T.T_views)
    cams = np.array([v.camera_pose.GetCameraMatrix() for v in T.T_views])
    assert rf.rotation_defect(cams) <= 1e-12 and np.linalg.det(cams[:, :, :3]).min() > 0
    np.testing.assert_array_equal(cams[0], c0[0])
    assert not np.array_equal(cams[1], c0[1])
    pts = np.array([p.point for p in T.T_points])
    assert pts.shape == p0.shape and not np.array_equal(pts, p0)
    assert _cost(cams, pts, ov, op, uv) == pytest.approx(info["cost"], rel=1e-12)
    # the table is still a table: the next view registers on it
    n_views = T.T_views.size
    gt.add_new_view(T, g("K"), 2, g("match_queries"), g("match_y2_hom"), g("match_y1"),
                    g("match_y2"))
    assert T.T_views.size == n_views + 1
