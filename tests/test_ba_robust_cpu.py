"""Bundle adjustment under a robust loss without a GPU: the numpy reference
tests/ba_robust_ref.py checks itself (weights and gradient against central differences, Schur
route against a dense solve, the linear loss against the two existing references), and pins the
motive on the tables of tests/wash_fixture.py: the sum-of-squares adjustment bends the cameras
towards the outliers and the wash after it throws good observations away; under a Cauchy loss
the poses come out as if the outliers were gone and the wash returns the mask it returns at the
true cameras.

Measured here (wash_fixture.table(nC, nP, seed): noise 1e-4, 11-15 % of the observations displaced
by 0.02; start ba_rigid_fixture.rigid_start(., 1e-3); rigid cameras; wash thresh 1e-3; Cauchy
f_scale 3e-4; pose error R / t of ba_rigid_fixture.pose_error):

  table     linear BA              wash drops   Cauchy BA              wash mask      linearisations
            R / t error            good obs     R / t error            = true-camera  linear / Cauchy
  4x30 s0   1.31   / 0.488         34 of 80     1.92e-2 / 1.56e-2      yes            97  / 32
  4x30 s1   0.320  / 0.539         23 of 80     1.42e-2 / 1.25e-2      yes            160 / 29
  6x40 s0   0.522  / 0.662         62 of 136    7.32e-3 / 1.38e-2      yes            157 / 19
  6x40 s1   0.483  / 4.11          66 of 136    1.82e-2 / 8.13e-3      yes            181 / 26
  7x70 s0   0.453  / 0.575         136 of 265   6.07e-3 / 1.94e-2      yes            200 / 23
  7x70 s1   1.10   / 0.843         128 of 265   8.39e-3 / 7.19e-3      yes            154 / 25

ba_robust_fixture.POSE_BAR = 0.06 is 3 times the worst Cauchy figure (1.94e-2) and 5 times
below the best linear one (0.320).
"""
import inspect

import numpy as np
import pytest

import ba_fixture as bf
import ba_rigid_fixture as rf
import ba_rigid_ref as rr
import ba_robust_fixture as xf
import ba_robust_ref as br
import wash_fixture as wf
import wash_ref as wr
from oracle import tables_ref as tr
from tsbb15_amd import _ffi
from tsbb15_amd import tables as gt

ROBUST = ("soft_l1", "huber", "cauchy")
POSE_BAR, TABLES = xf.POSE_BAR, xf.TABLES
MIN_GOOD_DROPPED = 20
_cache = {}


def _dirty(nC, nP):
    if (nC, nP) not in _cache:
        _cache[(nC, nP)] = xf.dirty_problem(nC, nP)
    return _cache[(nC, nP)]


# ------------------------------------------------------------------------------------------
# 1. w = rho', and the gradient of the robust cost is J~^T r~
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("loss", br.LOSSES)
def test_weight_is_the_derivative_of_rho(loss):
    # both sides of Huber's kink at z = 1, none within h of it
    z = np.concatenate([np.linspace(0.0105, 0.9905, 50), np.linspace(1.0105, 30.0, 50),
                        [1e3, 4.4e3, 1e6]])
    h = 1e-3 * np.minimum(z, 1.0)
    fd = (br.rho(loss, z + h) - br.rho(loss, z - h)) / (2 * h)
    err = np.abs(fd - br.weight(loss, z)).max()
    print(f"{loss}: max |central difference - w| {err:.2e}")
    # truncation h^2 |rho'''| / 6 <= 1e-6 * 3/8 / 6 (soft_l1 at z = 0); rounding eps rho / h ~ 1e-12
    assert err < 1e-6
    assert br.rho(loss, 0.0) == 0.0 and br.weight(loss, 0.0) == 1.0
    # scipy's stated forms
    if loss == "soft_l1":
        np.testing.assert_allclose(br.rho(loss, z), 2 * (np.sqrt(1 + z) - 1), rtol=1e-13)
    if loss == "huber":
        assert br.rho(loss, 1.0) == 1.0 and br.weight(loss, 1.0) == 1.0


@pytest.mark.parametrize("rigid", [False, True], ids=["free12", "rigid"])
@pytest.mark.parametrize("loss", br.LOSSES)
def test_gradient_of_the_robust_cost(loss, rigid):
    P = _dirty(4, 30)
    ov, op = P["ov"].astype(np.int64), P["op"].astype(np.int64)
    u, v = P["uv"][:, 0], P["uv"][:, 1]
    cams, pts = xf.start(P, 1e-3, rigid)
    nC, nP, C, D = len(cams), len(pts), xf.F_SCALE, 6 if rigid else 12

    def terms(cm, pt):          # the cost, observation by observation
        return 0.5 * C ** 2 * br.rho(loss, br.z_of(tr.ba_residuals(cm, pt, ov, op, u, v), C))

    r = tr.ba_residuals(cams, pts, ov, op, u, v)
    cost, w = br.robust_cost(r, loss, C)
    assert cost == pytest.approx(terms(cams, pts).sum(), rel=1e-14)
    Jc, Jp, rt = br.scaled(*br.jacobian(cams, pts, ov, op, rigid), r, w)
    _, gc, _, gp, _ = br.normal_blocks(Jc, Jp, rt, ov, op, nC, nP)
    h = 1e-7
    fd_c, fd_p = np.zeros((nC, D)), np.zeros((nP, 3))
    for k in range(nC):
        for q in range(D):
            d = np.zeros((nC, D))
            d[k, q] = h
            fd_c[k, q] = (terms(br.retract(cams, d, rigid), pts).sum()
                          - terms(br.retract(cams, -d, rigid), pts).sum()) / (2 * h)
    for q in range(3):
        d = np.zeros_like(pts)
        d[:, q] = h             # every observation sees one point: all points at once
        np.add.at(fd_p[:, q], op, (terms(cams, pts + d) - terms(cams, pts - d)) / (2 * h))
    scale = max(np.abs(gc).max(), np.abs(gp).max())
    ec, ep = np.abs(fd_c - gc).max() / scale, np.abs(fd_p - gp).max() / scale
    print(f"{loss} {'rigid' if rigid else '12'}: gradient vs central differences, cameras "
          f"{ec:.2e}, points {ep:.2e} of the largest entry {scale:.2e}")
    # rounding eps cost / h = 2e-16 * 1e-4 / 1e-7 = 2e-13 against entries of 1e-3 .. 1e-2: 1e-9
    # relative; truncation is smaller.  Huber's rho'' jumps at z = 1: an observation within h of
    # the kink adds O(h) relative
    assert ec < 1e-6 and ep < 1e-6, (ec, ep)


# ------------------------------------------------------------------------------------------
# 2. the Schur route equals the dense solve
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rigid", [False, True], ids=["free12", "rigid"])
@pytest.mark.parametrize("loss", ROBUST)
def test_schur_route_equals_dense_solve(loss, rigid):
    P = _dirty(4, 30)
    u, v = P["uv"][:, 0], P["uv"][:, 1]
    c0, p0 = xf.start(P, 1e-3, rigid)
    kw = dict(loss=loss, f_scale=xf.F_SCALE, rigid=rigid, max_iter=1)
    a = br.bundle_adjust_robust_lm(c0, p0, P["ov"], P["op"], u, v, **kw)
    b = br.bundle_adjust_robust_lm(c0, p0, P["ov"], P["op"], u, v, solver="dense", **kw)
    ec = np.abs(a[0] - b[0]).max() / np.abs(a[0] - c0).max()
    ep = np.abs(a[1] - b[1]).max() / np.abs(a[1] - p0).max()
    dw = np.abs(a[2]["weights"] - b[2]["weights"]).max()
    print(f"Schur vs dense, one {loss} step, {'rigid' if rigid else '12'}: cameras {ec:.2e}, "
          f"points {ep:.2e} of the largest step component, weights {dw:.2e}")
    assert a[2]["iterations"] == b[2]["iterations"] == 1
    assert a[2]["rejected"] == b[2]["rejected"]
    # the GPU's one-step bar is 1e-8; the reference must define the step 100 times finer
    assert ec < 1e-10 and ep < 1e-10 and dw < 1e-10


# ------------------------------------------------------------------------------------------
# 3. the linear loss is the two existing references
# ------------------------------------------------------------------------------------------
def test_linear_loss_is_the_existing_references():
    P = bf.problem(4, 30)
    ov, op = P["ov"], P["op"]
    u, v = P["uv"][:, 0], P["uv"][:, 1]
    for rigid in (False, True):
        c0, p0 = xf.start(P, 1e-3, rigid)
        if rigid:
            ref = rr.bundle_adjust_rigid_lm(c0, p0, ov, op, u, v)
        else:
            ref = tr.bundle_adjust_lm(c0, p0, ov, op, u, v)
        got = br.bundle_adjust_robust_lm(c0, p0, ov, op, u, v, rigid=rigid, f_scale=0.37)
        rel = abs(got[2]["cost"] - ref[2]["cost"]) / ref[2]["cost"]
        print(f"linear loss, {'rigid' if rigid else '12'}: cost {got[2]['cost']:.16e} against "
              f"{ref[2]['cost']:.16e}, rel {rel:.1e}, iterations {got[2]['iterations']} / "
              f"{ref[2]['iterations']}")
        # the 12-parameter oracle sums its Schur complement in another order, so the last
        # accept / reject decisions (and the iteration count) may differ; the minimum does not
        assert rel <= 1e-13
        assert np.all(got[2]["weights"] == 1.0)


# ------------------------------------------------------------------------------------------
# 4. the motive: Cauchy before the wash
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nC,nP,seed", TABLES)
def test_cauchy_before_the_wash(nC, nP, seed):
    W = wf.table(nC, nP, seed)
    ov, op, uv = W["ov"], W["op"], W["uv"]
    u, v = uv[:, 0], uv[:, 1]
    c0, p0 = rf.rigid_start(W, 1e-3)
    good = ~W["bad"]
    _, keep_true, *_ = wr.wash_points(W["cams"], p0, ov, op, uv, wf.THRESH)
    cl, pl, il = br.bundle_adjust_robust_lm(c0, p0, ov, op, u, v, rigid=True)
    _, keep_lin, *_ = wr.wash_points(cl, pl, ov, op, uv, wf.THRESH)
    cc, pc, ic = br.bundle_adjust_robust_lm(c0, p0, ov, op, u, v, loss="cauchy",
                                            f_scale=xf.F_SCALE, rigid=True)
    _, keep_c, *_ = wr.wash_points(cc, pc, ov, op, uv, wf.THRESH)
    eR_l, et_l = rf.pose_error(cl, W["cams"])
    eR_c, et_c = rf.pose_error(cc, W["cams"])
    dropped = int((good & ~keep_lin).sum())
    print(f"{nC}x{nP} s{seed}: linear R {eR_l:.3e} t {et_l:.3e} ({il['iterations']} "
          f"linearisations), its wash drops {dropped} of {int(good.sum())} good observations; "
          f"cauchy R {eR_c:.3e} t {et_c:.3e} ({ic['iterations']} linearisations, status "
          f"{ic['status']}), its wash mask equals the true-camera mask: "
          f"{np.array_equal(keep_c, keep_true)}; bad-observation weights <= "
          f"{ic['weights'][W['bad']].max():.1e}")
    assert np.array_equal(keep_c, keep_true)
    assert dropped >= MIN_GOOD_DROPPED
    assert eR_c <= POSE_BAR and et_c <= POSE_BAR
    assert POSE_BAR < min(eR_l, et_l)          # the bar stays below the linear result
    assert ic["status"] in (1, 2) and ic["iterations"] < 200


# ------------------------------------------------------------------------------------------
# 5. the Python surface, as far as it goes without a device
# ------------------------------------------------------------------------------------------
def test_keywords_and_their_validation():
    for f in (gt.bundle_adjust, gt.bundle_adjust_rigid, gt.BundleAdjustment2,
              gt.BundleAdjustmentRigid):
        # keyword-only on top of the sum-of-squares signature, which the existing tests pin
        assert "loss" not in inspect.signature(f).parameters
        kw = inspect.signature(f, follow_wrapped=False).parameters
        assert kw["loss"].default == "linear" and kw["f_scale"].default == 1.0
        assert kw["loss"].kind is kw["f_scale"].kind is inspect.Parameter.KEYWORD_ONLY
    assert _ffi.BA_LOSSES == br.LOSSES
    assert "rs_bundle_adjust_robust" in _ffi._SIGS
    P = _dirty(4, 30)
    c0, p0 = xf.start(P, 1e-3, True)
    # raised before any device work: no GPU is needed to get here
    for f in (gt.bundle_adjust, gt.bundle_adjust_rigid):
        with pytest.raises(ValueError, match="unknown loss"):
            f(c0, p0, P["ov"], P["op"], P["uv"], loss="arctan")
        for bad in (0.0, -1e-3, np.nan, np.inf):
            with pytest.raises(ValueError, match="f_scale"):
                f(c0, p0, P["ov"], P["op"], P["uv"], loss="cauchy", f_scale=bad)
            with pytest.raises(ValueError, match="f_scale"):
                f(c0, p0, P["ov"], P["op"], P["uv"], f_scale=bad)
    T = wf.mini_tables(wf.table(4, 30, 0))
    before = [v.camera_pose for v in T.T_views]
    with pytest.raises(ValueError, match="unknown loss"):
        gt.BundleAdjustmentRigid(T, loss="Cauchy")
    assert all(a is b for a, b in zip(before, (v.camera_pose for v in T.T_views)))
