"""GPU drop-ins for the per-view SfM steps around PnP (tables.py).

Array-level functions (HIP kernels of tables.hip):

  * ``match_observations``  the 2D<->3D matching loop of Tables.addNewView (tables.py:116-135)
  * ``getEFromCameras``     fun.getEFromCameras (fun.py:12-21)
  * ``add_new_points``      the arithmetic of Tables.addNewPoints (tables.py:161-175): epipolar
                            gate |y1^T E y2| < 0.1 and optimal triangulation of the accepted
  * ``ba_residuals``        EpsilonBA of Tables.BundleAdjustment2 (tables.py:264-293)
  * ``ba_jacobian``         its Jacobian blocks (the nonzeros of tables.py:339-372)
  * ``bundle_adjust``       that objective minimised on the GPU (ba.hip): Levenberg-Marquardt,
                            points eliminated by a Schur complement, camera 0 fixed
  * ``bundle_adjust_rigid`` the same objective over rigid poses: 6 local coordinates per camera,
                            R+ = Exp(omega) R, t+ = Exp(omega) t + tau, so every R stays a
                            rotation (ba.hip, rs_bundle_adjust_rigid).  Both take scipy's
                            ``loss=`` ("soft_l1", "huber", "cauchy") and ``f_scale=``
                            (rs_bundle_adjust_robust); run them so before ``wash_points``
  * ``nearest_rotations``   host helper: the nearest rotation to every 3 x 3 block of (nC, 3, 4)
                            cameras, for tables that came through the 12-parameter adjustment
  * ``triangulate_nview``   every point from all its observations (wash.hip)
  * ``wash_points``         robust re-triangulation of every point from its own track and the
                            outlier verdict on its observations: the WASH1 / WASH2 steps that
                            main.py:101-107 and main.py:140-168 name and leave empty

Table-level replacements for the reference's methods (they take a reference ``Tables``
object -- anything with T_obs / T_views / T_points, addView / addPoint / addObs -- run the
arithmetic above on the GPU and do the same bookkeeping in the same order):

  * ``add_new_view(T, K, img_index, y1_hom, y2_hom, y1, y2)``      Tables.addNewView
  * ``add_new_points_table(T, A_y1_hom, A_y2_hom, v1, v2)``       Tables.addNewPoints
  * ``BundleAdjustment2(T)``                                       Tables.BundleAdjustment2
  * ``BundleAdjustmentRigid(T)``                                   the same write-back around
                                                                   ``bundle_adjust_rigid``
  * ``wash(T, thresh)``                                            the wash step (no reference code)
  * ``get3DPointsColorsAndNormals(T)``                             Tables.get3DPointsColorsAndNormals
"""
from __future__ import annotations

import functools
import inspect

import numpy as np

from . import _ffi

_d = _ffi.C.c_double
MATCH_TOL = 1e-4     # tables.py:125
EPIPOLAR_GATE = 0.1  # tables.py:168


def _ctx(ctx):
    return (ctx or _ffi.default_context()).handle


def _pose(C):
    """A CameraPose (R, t) or a (3, 4) matrix -> contiguous (3, 4) [R | t]."""
    if hasattr(C, "R"):
        M = np.zeros((3, 4))
        M[:, :3] = C.R
        M[:, 3] = np.asarray(C.t).ravel()
        return M
    M = _ffi.f64c(C)
    if M.shape != (3, 4):
        raise ValueError('camera must be (3, 4) or a CameraPose')
    return M


pose_matrix = _pose   # the public name (dense.table_views)


def match_observations(obs_coords, obs_point, queries, tol=MATCH_TOL, ctx=None):
    obs = _ffi.f64c(obs_coords).reshape(-1, 3)
    op = np.ascontiguousarray(obs_point, dtype=np.int64).ravel()
    if len(op) != len(obs):
        raise ValueError('one point index per observation')
    q = _ffi.f64c(queries).reshape(-1, 3)
    out = np.empty(len(q), dtype=np.int64)
    _ffi.check(_ffi.lib().rs_match_observations(
        _ctx(ctx), _ffi.ptr(obs, _d) if len(obs) else None,
        _ffi.ptr(op, _ffi.C.c_int64) if len(op) else None, len(obs),
        _ffi.ptr(q, _d) if len(q) else None, len(q), float(tol), _ffi.ptr(out, _ffi.C.c_int64)))
    return out


def getEFromCameras(C1, C2, ctx=None):
    a, b = _pose(C1), _pose(C2)
    E = np.empty((3, 3))
    _ffi.check(_ffi.lib().rs_e_from_cameras(_ctx(ctx), _ffi.ptr(a, _d), _ffi.ptr(b, _d), 1,
                                            _ffi.ptr(E, _d)))
    return E


def add_new_points(y1_hom, y2_hom, C1, C2, gate=EPIPOLAR_GATE, ctx=None):
    """Returns (accepted mask (n,) bool, X (n, 3) with NaN rows where rejected)."""
    a, b = _pose(C1), _pose(C2)
    y1 = _ffi.f64c(y1_hom).reshape(-1, 3)
    y2 = _ffi.f64c(y2_hom).reshape(-1, 3)
    if y1.shape != y2.shape:
        raise ValueError('y1_hom and y2_hom must have the same shape')
    n = len(y1)
    mask = np.empty(n, dtype=np.int32)
    X = np.empty((n, 3))
    if n:
        _ffi.check(_ffi.lib().rs_add_new_points(_ctx(ctx), _ffi.ptr(a, _d), _ffi.ptr(b, _d),
                                                _ffi.ptr(y1, _d), _ffi.ptr(y2, _d), n,
                                                float(gate), _ffi.ptr(mask, _ffi.C.c_int32),
                                                _ffi.ptr(X, _d)))
    return mask.astype(bool), X


def _ba_args(cams, pts, obs_view, obs_point):
    cams = _ffi.f64c(cams).reshape(-1, 3, 4)
    pts = _ffi.f64c(pts).reshape(-1, 3)
    ov = _ffi.i32c(obs_view, 'obs_view').ravel()
    op = _ffi.i32c(obs_point, 'obs_point').ravel()
    if len(ov) != len(op):
        raise ValueError('obs_view and obs_point differ in length')
    return cams, pts, ov, op


def ba_residuals(cams, pts, obs_view, obs_point, uv, ctx=None):
    """EpsilonBA: (2 nObs,) interleaved [u - c1.x/c3.x, v - c2.x/c3.x]."""
    cams, pts, ov, op = _ba_args(cams, pts, obs_view, obs_point)
    uv = _ffi.f64c(uv).reshape(-1, 2)
    if len(uv) != len(ov):
        raise ValueError('one (u, v) per observation')
    r = np.empty(2 * len(ov))
    if len(ov):
        _ffi.check(_ffi.lib().rs_ba_residuals(
            _ctx(ctx), _ffi.ptr(cams, _d), len(cams), _ffi.ptr(pts, _d), len(pts),
            _ffi.ptr(ov, _ffi.C.c_int32), _ffi.ptr(op, _ffi.C.c_int32), _ffi.ptr(uv, _d), len(ov),
            _ffi.ptr(r, _d)))
    return r


def ba_jacobian(cams, pts, obs_view, obs_point, ctx=None):
    """Per observation: Jc (n, 2, 12), Jp (n, 2, 3)."""
    cams, pts, ov, op = _ba_args(cams, pts, obs_view, obs_point)
    n = len(ov)
    Jc, Jp = np.empty((n, 2, 12)), np.empty((n, 2, 3))
    if n:
        _ffi.check(_ffi.lib().rs_ba_jacobian(
            _ctx(ctx), _ffi.ptr(cams, _d), len(cams), _ffi.ptr(pts, _d), len(pts),
            _ffi.ptr(ov, _ffi.C.c_int32), _ffi.ptr(op, _ffi.C.c_int32), n, _ffi.ptr(Jc, _d),
            _ffi.ptr(Jp, _d)))
    return Jc, Jp


def _loss_code(loss, f_scale):
    if loss not in _ffi.BA_LOSSES:
        raise ValueError(f"unknown loss {loss!r}: one of {', '.join(_ffi.BA_LOSSES)}")
    f_scale = float(f_scale)
    if not (np.isfinite(f_scale) and f_scale > 0.0):
        raise ValueError(f"f_scale must be finite and > 0, not {f_scale}")
    return _ffi.BA_LOSSES.index(loss), f_scale


def _robust_keywords(robust):
    """Decorator of the four adjustments.  The decorated function is the sum-of-squares call
    and keeps its parameters, positions and defaults (``inspect.signature`` reports them, through
    ``__wrapped__``); on top it accepts the keyword-only ``loss="linear"`` and ``f_scale=1.0``.
    Both are checked before anything else happens; "linear" calls the function itself, any other
    loss calls ``robust(*its_arguments, loss, f_scale)``."""
    def decorate(linear):
        sig = inspect.signature(linear)

        @functools.wraps(linear)
        def adjust(*args, loss="linear", f_scale=1.0, **kw):
            code, f_scale = _loss_code(loss, f_scale)
            if code == 0:
                return linear(*args, **kw)
            bound = sig.bind(*args, **kw)
            bound.apply_defaults()
            return robust(*bound.args, loss, f_scale)
        return adjust
    return decorate


@_robust_keywords(lambda *a: _bundle_adjust(False, *a))
def bundle_adjust(cams, pts, obs_view, obs_point, uv, max_iter=200, ftol=1e-15, ctx=None):
    """The objective of ``ba_residuals`` minimised over cameras 1.. (12 parameters each) and the
    points: Levenberg-Marquardt with Marquardt damping and Nielsen's update, the points
    eliminated by a Schur complement, all on the GPU in fp64 (rs_bundle_adjust).  Camera 0,
    and every camera or point without an observation, comes back bit for bit unchanged.  At
    most ``_ffi.BA_MAX_CAMERAS`` cameras.  The inputs are not modified.

    Returns (cams (nC, 3, 4), pts (nP, 3), info) with info = dict(cost_init, cost, iterations,
    status, rejected, lambda): costs are 0.5 |r|^2; status 1 = an accepted step gained
    <= ftol * cost, 2 = damping above 1e32, 0 = max_iter linearisations.

    ``loss`` = "soft_l1", "huber" or "cauchy" with the scale ``f_scale`` = C > 0 minimises the
    robust cost 0.5 C^2 sum_i rho(z_i), z_i = (ru_i^2 + rv_i^2) / C^2, instead
    (rs_bundle_adjust_robust): soft_l1 rho = 2 (sqrt(1 + z) - 1), huber rho = z for z <= 1 and
    2 sqrt(z) - 1 above, cauchy rho = log1p(z).  These are the names and forms of
    scipy.optimize.least_squares; unlike scipy, rho acts on the squared norm of an observation's
    residual, not on its u and v components separately.  The same LM runs on the re-weighted
    problem, the weights w_i = rho'(z_i) taken anew at every linearisation.  The costs in info
    are then robust costs, and info gains "weights": w_i (n,) at the returned state, in the
    order of the observations.  An outlier's weight is small: with "cauchy" and ``f_scale`` a
    few times the noise, the cameras come out as if the outliers had been removed, which is
    what ``wash_points`` needs to judge them.  ``loss`` = "linear" (the default) is the plain
    sum of squares, bit for bit what it was without these keywords.  ValueError for an unknown
    loss name or an ``f_scale`` that is not finite and > 0.  Both are keyword-only."""
    return _bundle_adjust(False, cams, pts, obs_view, obs_point, uv, max_iter, ftol, ctx)


def _bundle_adjust(rigid, cams, pts, obs_view, obs_point, uv, max_iter, ftol, ctx,
                   loss="linear", f_scale=1.0):
    code, f_scale = _loss_code(loss, f_scale)
    cams, pts, ov, op = _ba_args(cams, pts, obs_view, obs_point)
    cams, pts = cams.copy(), pts.copy()
    uv = _ffi.f64c(uv).reshape(-1, 2)
    if len(uv) != len(ov):
        raise ValueError('one (u, v) per observation')
    if len(ov) == 0:
        raise ValueError('bundle adjustment needs at least one observation')
    if len(cams) == 0:
        raise ValueError('bundle adjustment needs at least one camera')
    info = _ffi.BaInfo()
    i32 = _ffi.C.c_int32
    args = (_ctx(ctx), _ffi.ptr(cams, _d), len(cams), _ffi.ptr(pts, _d), len(pts),
            _ffi.ptr(ov, i32), _ffi.ptr(op, i32), _ffi.ptr(uv, _d), len(ov), int(max_iter),
            float(ftol))
    weights = None
    if code == 0:
        entry = _ffi.lib().rs_bundle_adjust_rigid if rigid else _ffi.lib().rs_bundle_adjust
        _ffi.check(entry(*args, _ffi.C.byref(info)))
    else:
        weights = np.empty(len(ov))
        _ffi.check(_ffi.lib().rs_bundle_adjust_robust(
            *args, int(bool(rigid)), code, f_scale, _ffi.ptr(weights, _d), _ffi.C.byref(info)))
    out = {"cost_init": info.cost_init, "cost": info.cost, "iterations": info.iterations,
           "status": info.status, "rejected": info.rejected, "lambda": info.lam}
    if weights is not None:
        out["weights"] = weights
    return cams, pts, out


@_robust_keywords(lambda *a: _bundle_adjust(True, *a))
def bundle_adjust_rigid(cams, pts, obs_view, obs_point, uv, max_iter=200, ftol=1e-15, ctx=None):
    """``bundle_adjust`` over rigid poses (rs_bundle_adjust_rigid): the same objective, LM rules
    and return value, but camera k = [R | t] moves by 6 local coordinates (omega, tau),
    R+ = Exp(omega) R, t+ = Exp(omega) t + tau, so every R comes back a rotation (to rounding;
    nothing is re-orthonormalised) and the reconstruction stays metric up to its global scale.

    Every free camera (1.. with an observation) must hold a rotation: max |R^T R - I| <= 1e-6
    and det R > 0, else ValueError names the camera -- ``nearest_rotations`` repairs cameras
    that came through the 12-parameter ``bundle_adjust``.  Camera 0, and every camera or point
    without an observation, comes back bit for bit unchanged.  The inputs are not modified.
    The keywords ``loss`` and ``f_scale`` as in ``bundle_adjust``."""
    return _bundle_adjust(True, cams, pts, obs_view, obs_point, uv, max_iter, ftol, ctx)


def nearest_rotations(cams):
    """(nC, 3, 4) cameras with every 3 x 3 block replaced by its nearest rotation in the
    Frobenius norm (the polar factor U diag(1, 1, det(U V^T)) V^T of its SVD, det +1); t is left
    alone.  Host numpy.  The input is not modified."""
    out = np.array(cams, dtype=np.float64).reshape(-1, 3, 4)
    for M in out:
        U, _, Vt = np.linalg.svd(M[:, :3])
        M[:, :3] = U @ np.diag([1.0, 1.0, np.linalg.det(U @ Vt)]) @ Vt
    return out


def _wash_args(cams, pts, obs_view, obs_point, uv):
    cams, pts, ov, op = _ba_args(cams, pts, obs_view, obs_point)
    uv = _ffi.f64c(uv).reshape(-1, 2)
    if len(uv) != len(ov):
        raise ValueError('one (u, v) per observation')
    if len(ov) == 0:
        raise ValueError('the wash needs at least one observation')
    if len(cams) == 0:
        raise ValueError('the wash needs at least one camera')
    return cams, pts.copy(), ov, op, uv


def triangulate_nview(cams, pts, obs_view, obs_point, uv, ctx=None):
    """Every point from all its observations (rs_triangulate_nview): the linear solution of its
    2m equations, then Levenberg-Marquardt on X, no robustness.  Returns (pts, ok (bool)); a
    point with fewer than 2 observations, a singular start or a non-finite result has ok False
    and keeps its input bits.  The inputs are not modified."""
    cams, pts, ov, op, uv = _wash_args(cams, pts, obs_view, obs_point, uv)
    ok = np.zeros(len(pts), dtype=np.int32)
    i32 = _ffi.C.c_int32
    _ffi.check(_ffi.lib().rs_triangulate_nview(
        _ctx(ctx), _ffi.ptr(cams, _d), len(cams), _ffi.ptr(pts, _d), len(pts), _ffi.ptr(ov, i32),
        _ffi.ptr(op, i32), _ffi.ptr(uv, _d), len(ov), _ffi.ptr(ok, i32)))
    return pts, ok.astype(bool)


def wash_points(cams, pts, obs_view, obs_point, uv, thresh, min_views=2, depth_sign=0, ctx=None):
    """Robust re-triangulation of every point from its own track and the verdict on its
    observations (rs_wash_points; the algorithm stands in include/rsamd.h): two-view hypotheses
    from every pair of the track scored by their inliers within ``thresh`` (and, with
    ``depth_sign`` = +-1, with that sign of the depth), two refits over the inliers.

    Returns (pts, obs_keep (bool), point_keep (bool), err2, info): a kept point has its new
    coordinates and at least ``min_views`` kept observations; every other point keeps its input
    bits and loses all its observations.  err2 is the final squared error per observation, NaN
    where the point failed.  info = dict(hypotheses, obs_removed, points_removed,
    points_failed).  At most ``_ffi.WASH_MAX_TRACK`` observations per point.  The inputs are not
    modified."""
    cams, pts, ov, op, uv = _wash_args(cams, pts, obs_view, obs_point, uv)
    obs_keep = np.zeros(len(ov), dtype=np.int32)
    point_keep = np.zeros(len(pts), dtype=np.int32)
    err2 = np.full(len(ov), np.nan)
    info = _ffi.WashInfo()
    i32 = _ffi.C.c_int32
    _ffi.check(_ffi.lib().rs_wash_points(
        _ctx(ctx), _ffi.ptr(cams, _d), len(cams), _ffi.ptr(pts, _d), len(pts), _ffi.ptr(ov, i32),
        _ffi.ptr(op, i32), _ffi.ptr(uv, _d), len(ov), float(thresh), int(min_views),
        int(depth_sign), _ffi.ptr(obs_keep, i32), _ffi.ptr(point_keep, i32), _ffi.ptr(err2, _d),
        _ffi.C.byref(info)))
    return pts, obs_keep.astype(bool), point_keep.astype(bool), err2, {
        "hypotheses": info.hypotheses, "obs_removed": info.obs_removed,
        "points_removed": info.points_removed, "points_failed": info.points_failed}


# ------------------------------------------------------------------------------------------
# table-level replacements
# ------------------------------------------------------------------------------------------
def add_new_view(T, K, img_index, y1_hom, y2_hom, y1, y2, solvePnPRansac=None, Rodrigues=None):
    """Tables.addNewView (tables.py:104-158) with the matching loop on the GPU and, by default,
    the GPU solvePnPRansac of tsbb15_amd.cv.  Returns (A_y1, A_y2) as the reference.

    The new view's pose is built with the class of the table's existing poses (the reference's
    help_classes.CameraPose in the pipeline), so no reference module is imported here.  When
    PnP-RANSAC fails -- fewer than 4 matched 2D<->3D correspondences (OpenCV asserts 4 too) or
    no consensus -- a ValueError names the number of matched points instead of the reference's
    crash inside Rodrigues / inliers[:, 0]."""
    from . import cv as gcv
    solvePnPRansac = solvePnPRansac or gcv.solvePnPRansac
    Rodrigues = Rodrigues or gcv.Rodrigues
    last = T.T_views[len(T.T_views) - 1]
    pose_cls = type(last.camera_pose)
    idx = np.asarray(last.observations_index, dtype=np.int64)
    obs = np.array([T.T_obs[v].image_coordinates for v in idx]).reshape(-1, 3)
    opt = np.array([T.T_obs[v].point_3D_index for v in idx], dtype=np.int64)
    m = match_observations(obs, opt, np.asarray(y1_hom)[:, :3])
    found = m >= 0
    x_i = m[found]
    D_3D = np.array([T.T_points[j].point for j in x_i]).reshape(-1, 3)
    D_img = np.asarray(y2)[found].reshape(-1, 2)
    D_img_hom = np.asarray(y2_hom)[found].reshape(-1, 3)
    A_y1 = np.asarray(y1)[~found].reshape(-1, 2).astype(np.float64)
    A_y2 = np.asarray(y2)[~found].reshape(-1, 2).astype(np.float64)
    if len(x_i) < 4:
        raise ValueError(f"solvePnPRansac found no pose for view {img_index}: {len(x_i)} "
                         f"putative correspondences matched known 3D points (PnP needs >= 4)")
    retval, R, t, inliers = solvePnPRansac(D_3D[:, :3], D_img[:, :2], K, np.zeros((4, 1)),
                                           useExtrinsicGuess=True)
    if not retval or R is None or inliers is None:
        raise ValueError(f"solvePnPRansac found no pose for view {img_index}: {len(x_i)} "
                         f"putative correspondences matched known 3D points, no consensus")
    R, _ = Rodrigues(R)
    view_index = T.addView(img_index, pose_cls(R, np.asarray(t)[:, 0]))
    for yy, x in zip(D_img_hom[inliers[:, 0]], x_i[inliers[:, 0]]):
        T.addObs(yy, view_index, x)
    return A_y1, A_y2


def add_new_points_table(T, A_y1_hom, A_y2_hom, view_index_1, view_index_2):
    """Tables.addNewPoints (tables.py:161-175): the gate and the triangulations in one GPU
    launch, then the reference's bookkeeping in the reference's order.  Returns the count."""
    C1 = T.T_views[view_index_1].camera_pose
    C2 = T.T_views[view_index_2].camera_pose
    mask, X = add_new_points(A_y1_hom, A_y2_hom, C1, C2)
    counter = 0
    for i in np.flatnonzero(mask):
        point_index = T.addPoint(X[i])
        T.addObs(A_y1_hom[i], view_index_1, point_index)
        T.addObs(A_y2_hom[i], view_index_2, point_index)
        counter += 1
    return counter


@_robust_keywords(lambda *a: _adjust_table(bundle_adjust, *a))
def BundleAdjustment2(T, max_iter=200, ftol=1e-15, ctx=None):
    """Tables.BundleAdjustment2 (tables.py:260-338) on the GPU: the cameras [R | t] of T_views,
    the points of T_points and image_coordinates[:2] of T_obs, in table order, through
    ``bundle_adjust`` instead of scipy's TRF, then the write-back of updateCameras3Dpoints2
    (tables.py:384-390): every view gets a new pose of its own pose class built from the 3 x 4
    result, every point its new coordinates.  Returns the info dict of ``bundle_adjust``.
    The keywords ``loss`` and ``f_scale`` are those of ``bundle_adjust`` (the reference's
    least_squares call leaves them at scipy's defaults, "linear" and 1.0); info["weights"] is in
    T_obs order."""
    return _adjust_table(bundle_adjust, T, max_iter, ftol, ctx)


@_robust_keywords(lambda *a: _adjust_table(bundle_adjust_rigid, *a))
def BundleAdjustmentRigid(T, max_iter=200, ftol=1e-15, ctx=None):
    """``BundleAdjustment2`` with ``bundle_adjust_rigid`` in place of ``bundle_adjust``: the same
    gathering and write-back, every view's R stays a rotation.  The poses of the table must be
    rotations already (ValueError otherwise; see ``nearest_rotations``).  The keywords ``loss``
    and ``f_scale`` as in ``BundleAdjustment2``."""
    return _adjust_table(bundle_adjust_rigid, T, max_iter, ftol, ctx)


def _adjust_table(adjust, T, max_iter, ftol, ctx, loss="linear", f_scale=1.0):
    cams = np.array([_pose(v.camera_pose) for v in T.T_views]).reshape(-1, 3, 4)
    pts = np.array([p.point for p in T.T_points], dtype=np.float64).reshape(-1, 3)
    uv = np.array([np.asarray(o.image_coordinates, dtype=np.float64).ravel()[:2]
                   for o in T.T_obs]).reshape(-1, 2)
    ov = np.array([o.view_index for o in T.T_obs], dtype=np.int32)
    op = np.array([o.point_3D_index for o in T.T_obs], dtype=np.int32)
    new_pose, new_points, info = adjust(cams, pts, ov, op, uv, max_iter=max_iter, ftol=ftol,
                                        ctx=ctx, loss=loss, f_scale=f_scale)
    for i, v in enumerate(T.T_views):
        v.camera_pose = type(v.camera_pose)(new_pose[i, :3, :3], new_pose[i, :, 3])
    for i, p in enumerate(T.T_points):
        p.point = new_points[i]
    return info


def wash(T, thresh, min_views=2, depth_sign=0, ctx=None):
    """The wash step main.py names and leaves empty (WASH1 main.py:101-107, WASH2
    main.py:140-168), for after BundleAdjustment2 and after addNewPoints: the arrays are
    gathered as in ``BundleAdjustment2``, ``wash_points`` decides, and the table is rewritten.
    Removed points and observations leave T_points / T_obs, the survivors keep their relative
    order; kept points get their new coordinates; every point_3D_index and every
    observations_index (views and points) is renumbered, removed entries dropped.  Element 0 of
    an observations_index, the reference's spurious 0 (help_classes.py:26,61), stays a literal
    0.  Views are never removed; one may be left without observations.

    Returns the info dict of ``wash_points`` plus point_map and obs_map: the new index of every
    old point / observation, -1 where removed."""
    cams = np.array([_pose(v.camera_pose) for v in T.T_views]).reshape(-1, 3, 4)
    pts = np.array([p.point for p in T.T_points], dtype=np.float64).reshape(-1, 3)
    uv = np.array([np.asarray(o.image_coordinates, dtype=np.float64).ravel()[:2]
                   for o in T.T_obs]).reshape(-1, 2)
    ov = np.array([o.view_index for o in T.T_obs], dtype=np.int32)
    op = np.array([o.point_3D_index for o in T.T_obs], dtype=np.int32)
    new_points, obs_keep, point_keep, _, info = wash_points(
        cams, pts, ov, op, uv, thresh, min_views=min_views, depth_sign=depth_sign, ctx=ctx)
    point_map = np.where(point_keep, np.cumsum(point_keep) - 1, -1)
    obs_map = np.where(obs_keep, np.cumsum(obs_keep) - 1, -1)
    for j in np.flatnonzero(point_keep):
        T.T_points[j].point = new_points[j]
    for i in np.flatnonzero(obs_keep):
        T.T_obs[i].point_3D_index = int(point_map[op[i]])
    for rec in list(T.T_views) + [T.T_points[j] for j in np.flatnonzero(point_keep)]:
        idx = np.asarray(rec.observations_index)
        tail = obs_map[idx[1:].astype(np.int64)]
        rec.observations_index = np.concatenate((idx[:1], tail[tail >= 0])).astype(idx.dtype)
    T.T_obs = T.T_obs[obs_keep]                      # object arrays (tables.py:16-18)
    T.T_points = T.T_points[point_keep]
    out = dict(info)
    out["point_map"], out["obs_map"] = point_map, obs_map
    return out


def get3DPointsColorsAndNormals(T, radius=None, ctx=None):
    """Tables.get3DPointsColorsAndNormals (tables.py:216-226) in two GPU calls instead of three
    quadratic np.concatenate loops.  Returns (points, colors, normals), each (nP, 3).

    The entry list of a point is its observations_index as it stands, including element 0, the
    reference's spurious 0 (help_classes.py:26): the reference averages over T_obs[0] for every
    point (tables.py:192, :204), so this does too.  colors are the mean colour / 255, normals the
    mean of view.getWorldPosition() - point, not normalised (``cloud.point_attributes``).

    With ``radius`` set, normals are instead the unit PCA normals of
    ``cloud.surface_normals(points, radius)``, each oriented to agree with its view normal; a row
    that is not ok (fewer than 3 points within ``radius``) falls back to its view normal,
    normalised.

    Deviation: for a point whose observations_index holds one entry the reference raises
    (``normal`` is never bound, tables.py:211-214) after dividing the colour without averaging
    (tables.py:196-198).  Here that point gets that single vector and that single colour / 255."""
    from . import cloud
    cams = np.array([_pose(v.camera_pose) for v in T.T_views]).reshape(-1, 3, 4)
    pts = np.array([p.point for p in T.T_points], dtype=np.float64).reshape(-1, 3)
    ov = np.array([o.view_index for o in T.T_obs], dtype=np.int32)
    col = np.array([np.asarray(o.color, dtype=np.float64).ravel()[:3]
                    for o in T.T_obs]).reshape(-1, 3)
    idx = [np.asarray(p.observations_index, dtype=np.int32).ravel() for p in T.T_points]
    entry_obs = np.concatenate(idx) if idx else np.zeros(0, np.int32)
    entry_point = np.repeat(np.arange(len(idx), dtype=np.int32), [len(i) for i in idx])
    colors, normals = cloud.point_attributes(cams, pts, entry_point, entry_obs, ov, col, ctx=ctx)
    if radius is not None:
        pca, ok, _, _, _ = cloud.surface_normals(pts, radius, orient=normals, ctx=ctx)
        with np.errstate(invalid='ignore', divide='ignore'):
            unit = normals / np.linalg.norm(normals, axis=1, keepdims=True)
        normals = np.where(ok[:, None], pca, unit)
    return pts, colors, normals
