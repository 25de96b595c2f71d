"""The rigid-camera bundle adjustment without a GPU: the numpy reference tests/ba_rigid_ref.py
checks itself (Jacobians, Schur route against a dense solve), pins the motive (the 12-parameter
adjustment leaves SO(3), the rigid one does not and lands nearer the true poses), measures how
far it moves under input-level rounding (the GPU parity bars of tests/test_gpu_ba_rigid.py are
derived from that), and the ABI / binding / host-helper surface is checked.

Measured here (tests/ba_fixture.py problems, uv noise 1e-4, rigid starts):

  problem        12-parameter oracle           rigid reference
                 max|R^T R - I|  R / t error   max|R^T R - I|  R / t error
  5x40 s 1e-3    0.131           0.079 / 0.135  1.3e-15        0.017 / 0.012
  5x40 s 5e-2    0.273           0.116 / 0.145  1.6e-15        0.017 / 0.012
  7x70 s 1e-3    0.367           0.239 / 0.396  1.6e-15        0.0031 / 0.016
  7x70 s 5e-2    0.327           0.236 / 0.396  1.6e-15        0.0031 / 0.016

Schur route against the dense solve, one step on 5x40: 1.7e-13 (cameras) / 6.5e-14 (points) of
the largest step component.  Noise-free 5x40: final cost 6e-31, poses to 6.4e-15.

The reference's own move under a 1e-13 relative perturbation of the start points (cost
relative; R; t with the scale fixed by |t_1|):

  4x30 s 1e-3   1.1e-13  9.4e-10  3.1e-10      4x30 s 5e-2   1.0e-13  3.3e-12  1.2e-12
  5x40 s 1e-3   5.1e-14  1.9e-09  2.0e-09      5x40 s 5e-2   1.3e-13  5.2e-14  5.8e-14
  7x70 s 1e-3   4.7e-14  7.8e-11  5.6e-11      7x70 s 5e-2   2.1e-14  5.2e-10  5.5e-10

The parameter move depends on which trials the last iterations accept, so it spreads over three
orders of magnitude between starts of one problem; a fixture's own move is the larger of its two.
"""
import ctypes
import inspect

import numpy as np
import pytest

import ba_fixture as bf
import ba_rigid_fixture as rf
import ba_rigid_ref as rr
from oracle import tables_ref as tr
from tsbb15_amd import _ffi
from tsbb15_amd import tables as gt

SIZES = {"4x30": (4, 30), "5x40": (5, 40), "7x70": (7, 70)}
_cache = {}


def _problem(size):
    if size not in _cache:
        _cache[size] = bf.problem(*SIZES[size])
    return _cache[size]


def _uv(P):
    return P["uv"][:, 0], P["uv"][:, 1]


# ------------------------------------------------------------------------------------------
# 1. Jacobians against central differences through the retraction
# ------------------------------------------------------------------------------------------
def test_jacobians_match_finite_differences():
    P = _problem("5x40")
    ov, op = P["ov"], P["op"]
    u, v = _uv(P)
    cams, pts = rf.rigid_start(P, 5e-2)
    Jc, Jp = rr.jacobian(cams, pts, ov, op)
    h = 1e-6
    worst_c = worst_p = 0.0
    for k in range(len(cams)):
        for q in range(6):
            d = np.zeros((len(cams), 6))
            d[k, q] = h
            rp = tr.ba_residuals(rr.retract(cams, d), pts, ov, op, u, v)
            rm = tr.ba_residuals(rr.retract(cams, -d), pts, ov, op, u, v)
            fd = ((rp - rm) / (2 * h)).reshape(-1, 2)
            sel = ov == k
            worst_c = max(worst_c, np.abs(fd[sel] - Jc[sel, :, q]).max())
            assert np.abs(fd[~sel]).max() == 0.0
    for q in range(3):
        d = np.zeros_like(pts)
        d[:, q] = h          # every observation sees exactly one point: all points at once
        rp = tr.ba_residuals(cams, pts + d, ov, op, u, v)
        rm = tr.ba_residuals(cams, pts - d, ov, op, u, v)
        fd = ((rp - rm) / (2 * h)).reshape(-1, 2)
        worst_p = max(worst_p, np.abs(fd - Jp[:, :, q]).max())
    scale = max(np.abs(Jc).max(), np.abs(Jp).max())
    print(f"Jc vs central differences {worst_c:.2e}, Jp {worst_p:.2e} (largest entry {scale:.2e})")
    # central differences: truncation h^2 |r'''| / 6 plus rounding eps |r| / h ~ 1e-10 each
    assert worst_c < 1e-7 * scale and worst_p < 1e-7 * scale


def test_exp_is_a_rotation_and_matches_its_series():
    for w in ([0.3, -0.2, 0.5], [1e-7, 2e-7, -1e-7], [0.0, 0.0, 0.0], [2.0, 1.0, -2.5]):
        E = rr.exp_so3(w)
        # an entry of E carries about 3 roundings (|E| <= 1), an entry of E^T E sums 3 products of
        # two such entries and rounds 3 more times: 2 * 3 + 3 = 9 eps = 2e-15
        assert np.abs(E.T @ E - np.eye(3)).max() < 2e-15 and np.linalg.det(E) > 0
        K, S, term = rr.hat(w), np.eye(3), np.eye(3)
        for n in range(1, 40):
            term = term @ K / n
            S = S + term
        assert np.abs(E - S).max() < 1e-14


# ------------------------------------------------------------------------------------------
# 2. the Schur route equals the dense solve
# ------------------------------------------------------------------------------------------
def test_schur_route_equals_dense_solve():
    P = _problem("5x40")
    u, v = _uv(P)
    c0, p0 = rf.rigid_start(P, 1e-3)
    a = rr.bundle_adjust_rigid_lm(c0, p0, P["ov"], P["op"], u, v, max_iter=1)
    b = rr.bundle_adjust_rigid_lm(c0, p0, P["ov"], P["op"], u, v, max_iter=1, solver="dense")
    ec = np.abs(a[0] - b[0]).max() / np.abs(a[0] - c0).max()
    ep = np.abs(a[1] - b[1]).max() / np.abs(a[1] - p0).max()
    print(f"Schur vs dense, one step 5x40: cameras {ec:.2e}, points {ep:.2e} of the largest "
          f"step component")
    assert a[2]["iterations"] == b[2]["iterations"] == 1
    # the GPU's one-step bar is 1e-8; the reference must define the step 100 times finer
    assert ec < 1e-10 and ep < 1e-10


# ------------------------------------------------------------------------------------------
# 3. the motive
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sigma", [1e-3, 5e-2])
@pytest.mark.parametrize("size", ["5x40", "7x70"])
def test_twelve_parameters_leave_so3_rigid_does_not(size, sigma):
    P = _problem(size)
    u, v = _uv(P)
    c0, p0 = rf.rigid_start(P, sigma)
    assert rf.rotation_defect(c0) < 1e-14
    co, _, io = tr.bundle_adjust_lm(c0, p0, P["ov"], P["op"], u, v)
    cr, _, ir = rr.bundle_adjust_rigid_lm(c0, p0, P["ov"], P["op"], u, v)
    do, dr = rf.rotation_defect(co), rf.rotation_defect(cr)
    eo, er = rf.pose_error(co, P["cams"]), rf.pose_error(cr, P["cams"])
    print(f"{size} sigma {sigma}: 12-parameter max|RtR - I| {do:.3f}, pose error {eo[0]:.3f} / "
          f"{eo[1]:.3f}, cost {io['cost']:.4e}; rigid {dr:.1e}, {er[0]:.4f} / {er[1]:.4f}, cost "
          f"{ir['cost']:.4e} ({ir['iterations']} linearisations, {ir['rejected']} rejected)")
    assert do > 1e-2
    assert dr <= 1e-12
    assert np.linalg.det(cr[:, :, :3]).min() > 0
    assert er[0] < eo[0] and er[1] < eo[1]
    assert ir["cost"] < ir["cost_init"] and ir["status"] in (1, 2)


# ------------------------------------------------------------------------------------------
# 4. noise-free data: the true poses come back
# ------------------------------------------------------------------------------------------
def test_noise_free_recovers_the_truth():
    P = bf.problem(5, 40, noise=0.0)
    u, v = _uv(P)
    c0, p0 = rf.rigid_start(P, 1e-3)
    c, p, info = rr.bundle_adjust_rigid_lm(c0, p0, P["ov"], P["op"], u, v)
    eR, et = rf.pose_error(c, P["cams"])
    print(f"noise-free 5x40: cost {info['cost']:.1e}, pose error {eR:.1e} / {et:.1e}")
    assert info["cost"] < 1e-20
    assert eR < 1e-10 and et < 1e-10


# ------------------------------------------------------------------------------------------
# 5. the reference's own move under input-level rounding
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sigma", [1e-3, 5e-2])
@pytest.mark.parametrize("size", list(SIZES))
def test_own_move_under_rounding_level_perturbation(size, sigma):
    m = rf.own_move(_problem(size), sigma)
    print(f"own move {size} sigma {sigma}: cost {m['cost']:.2e} relative, R {m['R']:.2e}, "
          f"t {m['t']:.2e}")
    # the GPU bars are COST_BAR = 1e-10 and 100 x the parameter move: they mean something only
    # while the reference itself stays well inside 1e-10 in cost and, times 100, well inside
    # the 1e-4 observation noise in the poses
    assert m["cost"] < 1e-11
    assert m["R"] < 1e-6 and m["t"] < 1e-6


# ------------------------------------------------------------------------------------------
# 6. ABI and bindings
# ------------------------------------------------------------------------------------------
def test_abi_and_binding():
    lib = ctypes.CDLL(_ffi.LIB_PATH)
    assert hasattr(lib, "rs_bundle_adjust_rigid") and "rs_bundle_adjust_rigid" in _ffi._SIGS
    assert _ffi._SIGS["rs_bundle_adjust_rigid"] == _ffi._SIGS["rs_bundle_adjust"]
    src = open(_ffi.HEADER_PATH).read()
    assert "int rs_bundle_adjust_rigid(rs_ctx *ctx, double *cams, int64_t nC" in src
    assert ctypes.sizeof(_ffi.BaInfo) == 40 and len(_ffi.BA_KERNELS) == 8


def test_python_signatures():
    p = inspect.signature(gt.bundle_adjust_rigid).parameters
    assert list(p) == ["cams", "pts", "obs_view", "obs_point", "uv", "max_iter", "ftol", "ctx"]
    assert (p["max_iter"].default, p["ftol"].default, p["ctx"].default) == (200, 1e-15, None)
    p = inspect.signature(gt.BundleAdjustmentRigid).parameters
    assert list(p) == ["T", "max_iter", "ftol", "ctx"]
    assert (p["max_iter"].default, p["ftol"].default, p["ctx"].default) == (200, 1e-15, None)
    for name in ("bundle_adjust_rigid", "nearest_rotations", "BundleAdjustmentRigid"):
        assert name in gt.__doc__


def test_length_checks_need_no_device():
    P = _problem("5x40")
    with pytest.raises(ValueError):
        gt.bundle_adjust_rigid(P["cams"], P["pts"], P["ov"][:-1], P["op"], P["uv"])
    with pytest.raises(ValueError):
        gt.bundle_adjust_rigid(P["cams"], P["pts"], P["ov"], P["op"], P["uv"][:-1])
    with pytest.raises(ValueError):
        gt.bundle_adjust_rigid(P["cams"], P["pts"], P["ov"][:0], P["op"][:0], P["uv"][:0])
    with pytest.raises(ValueError):
        gt.bundle_adjust_rigid(P["cams"][:0], P["pts"], P["ov"], P["op"], P["uv"])


# ------------------------------------------------------------------------------------------
# 7. nearest_rotations
# ------------------------------------------------------------------------------------------
def test_nearest_rotations():
    P = _problem("5x40")
    cams = P["cams"]
    out = gt.nearest_rotations(cams)
    assert out is not cams and np.abs(out - cams).max() <= 1e-15
    rng = np.random.RandomState(5)
    bad = cams.copy()
    bad[1, :, :3] *= 1.3                                           # scaled
    bad[2, :, :3] = bad[2, :, :3] @ (np.eye(3) + 0.2 * rng.standard_normal((3, 3)))  # sheared
    bad[3, :, :3] = np.diag([1.0, 1.0, -1.0]) @ bad[3, :, :3]      # reflected
    bad_in = bad.copy()
    out = gt.nearest_rotations(bad)
    np.testing.assert_array_equal(bad, bad_in)
    np.testing.assert_array_equal(out[:, :, 3], bad[:, :, 3])
    assert rf.rotation_defect(out) <= 1e-14
    assert np.allclose(np.linalg.det(out[:, :, :3]), 1.0, atol=1e-14)
    assert np.abs(out[1, :, :3] - cams[1, :, :3]).max() <= 1e-15   # a scaled rotation: itself
    # the polar factor is the nearest rotation: no random rotation nearby is nearer
    M = bad[2, :, :3]
    best = np.linalg.norm(out[2, :, :3] - M)
    for _ in range(50):
        Q = rr.exp_so3(0.05 * rng.standard_normal(3)) @ out[2, :, :3]
        assert np.linalg.norm(Q - M) >= best
    # the 12-parameter oracle's cameras are not rotations; after the helper they are
    u, v = _uv(P)
    c0, p0 = rf.rigid_start(P, 1e-3)
    co, _, _ = tr.bundle_adjust_lm(c0, p0, P["ov"], P["op"], u, v, max_iter=5)
    assert rf.rotation_defect(co) > 1e-6
    assert rf.rotation_defect(gt.nearest_rotations(co)) <= 1e-14
