"""The evaluation stage: how good a mesh is, and how good the cameras are.

The reference names this step (evaluation.py loads the true cameras of imgdata/dino_Ps.mat, prints
them and stops; main.py:180-181 saves R_eval_clean / t_eval_clean for it).  The measures are those
of the multi-view-stereo benchmark the Dino comes from (Seitz et al. 2006):

  * accuracy      the distance d such that a given fraction of the reconstruction lies within d
                  of the truth
  * completeness  the fraction of the truth that lies within a given distance of the
                  reconstruction

Both rest on ``mesh_distance``, the exact distance from many points to a triangle mesh (HIP kernels
of eval.hip; the contract stands in include/rsamd.h).  Everything about the cameras -- tens of
them -- is host numpy: ``decompose_projection``, ``align_similarity``, ``camera_errors``.

Both measures assume the two meshes stand in one frame.  ``register`` brings them there: trimmed
ICP of a point cloud to a mesh kept on the device (``MeshIndex``, the rs_eval_index_* entries),
one device step and one small host solve per iteration; ``compare_meshes(register=...)`` runs it
first.  ``register`` needs a start inside its basin; ``global_register`` finds one from any pose
and scale: FPFH descriptors (``cloud.fpfh``), nearest-descriptor matches, a RANSAC over
three-point similarities (``ransac_similarity``, global_reg.hip) and a verification of the best
hypotheses against the mesh.
"""
from __future__ import annotations

import numpy as np

from . import _ffi

_d = _ffi.C.c_double
_i32 = _ffi.C.c_int32

MAX_POINTS = 1 << 28    # RS_EVAL_MAX_POINTS
MAX_CELLS = 1 << 24     # RS_EVAL_MAX_CELLS
MAX_ENTRIES = 1 << 27   # RS_EVAL_MAX_ENTRIES
STAGES = _ffi.EVAL_STAGES


def _ctx(ctx):
    return (ctx or _ffi.default_context()).handle


def _points(a, name):
    a = _ffi.f64c(a)
    if a.ndim != 2 or a.shape[1] != 3:
        raise ValueError(f'{name} must be (n, 3)')
    return a


def _faces(faces, nv):
    f = np.asarray(faces)
    if f.size and not np.issubdtype(f.dtype, np.integer):
        raise ValueError('faces must hold integers')
    f = f.reshape(-1, 3) if f.size == 0 else f
    if f.ndim != 2 or f.shape[1] != 3:
        raise ValueError('faces must be (nf, 3)')
    if f.size and (f.min() < 0 or f.max() >= nv):
        raise ValueError('a face index is out of range')
    return _ffi.i32c(f, 'faces')


def default_cell(vertices, faces):
    """max(2 x the median diagonal of the faces' boxes, the mesh box's largest extent / 512), over
    the faces whose coordinates are finite; 1 for a mesh without one or without any extent.  Never
    below 2^-23 of the largest coordinate magnitude (rs_eval_mesh_distance refuses 2^-24)."""
    tri = vertices[faces]
    tri = tri[np.isfinite(tri).all(axis=(1, 2))]
    if len(tri) == 0:
        return 1.0
    lo, hi = tri.min(axis=1), tri.max(axis=1)
    diag = np.sqrt(((hi - lo) ** 2).sum(axis=1))
    cell = max(2.0 * float(np.median(diag)), float((hi.max(axis=0) - lo.min(axis=0)).max()) / 512.0,
               float(np.abs(tri).max()) / (1 << 23))
    return cell if np.isfinite(cell) and cell > 0.0 else 1.0


def mesh_distance(points, vertices, faces, max_dist=np.inf, cell=None, ctx=None):
    """The distance from every point to a triangle mesh (rs_eval_mesh_distance).

    points (n, 3), vertices (nv, 3), faces (nf, 3) integers.  Returns (dist, face, closest, info):
    dist (n) the distance to the closest point of the mesh, face (n) int32 the lowest-numbered
    face that attains it, closest (n, 3) that point.  A point farther than ``max_dist`` (+inf
    allowed) from every face, or a mesh without a valid face, gives dist = +inf, face = -1,
    closest = NaN; a point with a coordinate that is not finite gives dist = NaN, face = -1.  A
    face with a coordinate that is not finite or without area is skipped.

    ``cell`` is the side of the search grid, ``default_cell`` when None; the result does not
    depend on it, the time does.  info = dict(d2, cell, cells, entries, largest_cell, tests,
    faces_skipped, beyond), d2 (n) the squared distances as the kernel made them.  n == 0 returns
    empty arrays without a launch.  ValueError: bad shapes, an index out of range, max_dist not
    > 0, cell not finite or not > 0, or a cell so small that the grid passes MAX_CELLS cells or
    MAX_ENTRIES registrations."""
    points, vertices = _points(points, 'points'), _points(vertices, 'vertices')
    faces = _faces(faces, len(vertices))
    max_dist = float(max_dist)
    if not max_dist > 0.0:
        raise ValueError('max_dist must be positive (+inf is allowed)')
    cell = default_cell(vertices, faces) if cell is None else float(cell)
    if not np.isfinite(cell) or not cell > 0.0:
        raise ValueError('cell must be finite and positive')
    n = len(points)
    d2, face, closest = np.empty(n), np.full(n, -1, dtype=np.int32), np.empty((n, 3))
    info = _ffi.EvalInfo()
    if n > 0:
        _ffi.check(_ffi.lib().rs_eval_mesh_distance(
            _ctx(ctx), _ffi.ptr(points, _d), n, _ffi.ptr(vertices, _d), len(vertices),
            _ffi.ptr(faces, _i32), len(faces), max_dist, cell, _ffi.ptr(d2, _d),
            _ffi.ptr(face, _i32), _ffi.ptr(closest, _d), _ffi.C.byref(info)))
    return np.sqrt(d2), face, closest, {
        "d2": d2, "cell": cell, "cells": tuple(info.cells), "entries": info.entries,
        "largest_cell": info.largest_cell, "tests": info.tests,
        "faces_skipped": info.faces_skipped, "beyond": info.beyond}


def timing(enable, ctx=None):
    """Enable / disable HIP events between the stages of the next mesh_distance calls
    (rs_eval_timing); returns the last timed call's {stage: device ms}, -1 where none."""
    ctx = ctx or _ffi.default_context()
    ms = np.zeros(len(STAGES))
    _ffi.check(_ffi.lib().rs_eval_timing(ctx.handle, int(enable), _ffi.ptr(ms, _d)))
    return dict(zip(STAGES, ms.tolist()))


def sample_surface(vertices, faces, n, seed=0):
    """n points on the mesh, drawn uniformly by area with np.random.RandomState(seed) (host only).

    Returns (points (n, 3), face (n) int64).  One draw of n uniforms picks the faces by the
    running sum of the areas, a second and third give the place inside: with s = sqrt(r1) the
    point is (1 - s) a + s (1 - r2) b + s r2 c.  A face without area or with a coordinate that is
    not finite is never drawn.  ValueError for a mesh without area when n > 0."""
    vertices = _points(vertices, 'vertices')
    faces = _faces(faces, len(vertices))
    n = int(n)
    if n < 0:
        raise ValueError('n must not be negative')
    rs = np.random.RandomState(seed)
    tri = vertices[faces]
    with np.errstate(invalid='ignore', over='ignore'):
        cr = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
        area = 0.5 * np.sqrt((cr * cr).sum(axis=1))
    area[~np.isfinite(area)] = 0.0
    if n == 0:
        return np.empty((0, 3)), np.empty(0, dtype=np.int64)
    if not area.sum() > 0.0:
        raise ValueError('the mesh has no area to sample')
    cum = np.cumsum(area)
    u, r1, r2 = rs.uniform(size=n), rs.uniform(size=n), rs.uniform(size=n)
    # the first face whose running sum passes the draw: a face without area never is
    f = np.searchsorted(cum, u * cum[-1], side='right')
    f = np.minimum(f, int(np.flatnonzero(area > 0.0)[-1]))
    s = np.sqrt(r1)
    w = np.stack([1.0 - s, s * (1.0 - r2), s * r2], axis=1)
    return (w[:, :, None] * tri[f]).sum(axis=1), f.astype(np.int64)


def _distances(dist):
    dist = np.asarray(dist, dtype=np.float64).reshape(-1)
    if len(dist) == 0:
        raise ValueError('no distances')
    return dist


def accuracy(dist, fraction=0.9):
    """The distance within which ``fraction`` of the points lie: the ceil(fraction n)-th smallest
    value (fraction n is rounded to 9 decimals first, so that 0.7 x 10 counts as 7).  +inf counts
    as +inf.  ValueError for a NaN, an empty array or a fraction outside (0, 1]."""
    dist = _distances(dist)
    if np.isnan(dist).any():
        raise ValueError('a distance is NaN (a point with a coordinate that is not finite)')
    if not 0.0 < fraction <= 1.0:
        raise ValueError('fraction must be in (0, 1]')
    k = max(int(np.ceil(np.round(fraction * len(dist), 9))), 1)
    return float(np.partition(dist, k - 1)[k - 1])


def completeness(dist, threshold):
    """The share of the points within ``threshold``: mean(dist <= threshold)."""
    return float((_distances(dist) <= threshold).mean())


def compare_meshes(rec_v, rec_f, gt_v, gt_f, fraction=0.9, threshold=None, max_dist=np.inf,
                   samples=None, seed=0, ctx=None, register=None):
    """Accuracy and completeness of a reconstruction against the truth, both through
    mesh_distance: the reconstruction's points against the true mesh, and the truth's points
    against the reconstructed one.  The points are the meshes' vertices, or with ``samples`` that
    many surface samples of each (sample_surface, seeds ``seed`` and ``seed + 1``).  ``threshold``
    is completeness' distance, by default 1 % of the diagonal of the truth's box.

    ``register``, a dict of keywords for ``register`` (an empty one for its defaults), first
    registers the reconstruction's points to the true mesh and applies the similarity found to
    ``rec_v`` before both distance calls; the result gains s, R, t and ``registration``, what
    ``register`` returned.  With None nothing is aligned.  ``register="global"`` needs no start:
    ``global_register`` with its defaults on ``samples`` (2 000 when None) surface samples of the
    reconstruction and their faces' normals, so both meshes must be wound the same way.

    Returns dict(accuracy, completeness, fraction, threshold, dist_rec, dist_gt, info_rec,
    info_gt)."""
    rec_v, gt_v = _points(rec_v, 'rec_v'), _points(gt_v, 'gt_v')
    rec_f, gt_f = _faces(rec_f, len(rec_v)), _faces(gt_f, len(gt_v))
    if threshold is None:
        finite = gt_v[np.isfinite(gt_v).all(axis=1)]
        if len(finite) == 0:
            raise ValueError('the truth has no finite vertex to take a threshold from')
        threshold = 0.01 * float(np.sqrt(((finite.max(axis=0) - finite.min(axis=0)) ** 2).sum()))
    if isinstance(register, str):
        if register != "global":
            raise ValueError('register must be None, a dict of keywords or "global"')
        src, face = sample_surface(rec_v, rec_f, 2000 if samples is None else samples, seed)
        reg = global_register(src, face_normals(rec_v, rec_f)[face], gt_v, gt_f, seed=seed,
                              ctx=ctx)
    elif register is not None:
        src = rec_v if samples is None else sample_surface(rec_v, rec_f, samples, seed)[0]
        reg = _register(src, gt_v, gt_f, ctx=ctx, **dict(register))
    if register is not None:
        moved = apply_similarity(rec_v, reg["s"], reg["R"], reg["t"])
        out = compare_meshes(moved, rec_f, gt_v, gt_f, fraction=fraction, threshold=threshold,
                             max_dist=max_dist, samples=samples, seed=seed, ctx=ctx)
        out.update(s=reg["s"], R=reg["R"], t=reg["t"], registration=reg)
        return out
    if samples is None:
        rec_p, gt_p = rec_v, gt_v
    else:
        rec_p = sample_surface(rec_v, rec_f, samples, seed)[0]
        gt_p = sample_surface(gt_v, gt_f, samples, seed + 1)[0]
    dist_rec, _, _, info_rec = mesh_distance(rec_p, gt_v, gt_f, max_dist=max_dist, ctx=ctx)
    dist_gt, _, _, info_gt = mesh_distance(gt_p, rec_v, rec_f, max_dist=max_dist, ctx=ctx)
    return {"accuracy": accuracy(dist_rec, fraction),
            "completeness": completeness(dist_gt, threshold), "fraction": fraction,
            "threshold": threshold, "dist_rec": dist_rec, "dist_gt": dist_gt,
            "info_rec": info_rec, "info_gt": info_gt}


# ---- registration ------------------------------------------------------------------------------

REG_STAGES = _ffi.EVAL_REG_STAGES
REG_METRICS = _ffi.EVAL_REG_METRICS
REG_BLOCK = _ffi.EVAL_REG_BLOCK   # RS_EVAL_REG_BLOCK


def mesh_box(vertices, faces):
    """(centre, diagonal) of the box of the faces with finite coordinates, the box the grid is
    laid over; (0, 0) for a mesh without such a face."""
    tri = np.asarray(vertices)[np.asarray(faces).reshape(-1, 3)]
    tri = tri[np.isfinite(tri).all(axis=(1, 2))]
    if len(tri) == 0:
        return np.zeros(3), 0.0
    lo, hi = tri.min(axis=(0, 1)), tri.max(axis=(0, 1))
    return (lo + hi) / 2.0, float(np.sqrt(((hi - lo) ** 2).sum()))


class MeshIndex:
    """A target mesh and its search grid kept on the device (rs_eval_index): built once, queried
    many times.  ``cell`` is the grid's side, ``default_cell`` when None.  Use it as a context
    manager or call ``close``; the handle is also released when the object is collected.  The
    index uses the stream of ``ctx`` and keeps it alive."""

    def __init__(self, vertices, faces, cell=None, ctx=None):
        self._h = None
        vertices = _points(vertices, 'vertices')
        faces = _faces(faces, len(vertices))
        cell = default_cell(vertices, faces) if cell is None else float(cell)
        if not np.isfinite(cell) or not cell > 0.0:
            raise ValueError('cell must be finite and positive')
        self.ctx = ctx or _ffi.default_context()
        self.cell = cell
        self.origin, self.diagonal = mesh_box(vertices, faces)
        self.n_points = 0
        h, info = _ffi.C.c_void_p(), _ffi.EvalInfo()
        _ffi.check(_ffi.lib().rs_eval_index_create(
            self.ctx.handle, _ffi.ptr(vertices, _d), len(vertices), _ffi.ptr(faces, _i32),
            len(faces), cell, _ffi.C.byref(h), _ffi.C.byref(info)))
        self._h = h
        self.cells, self.entries = tuple(info.cells), info.entries
        self.largest_cell, self.faces_skipped = info.largest_cell, info.faces_skipped

    @property
    def handle(self):
        if self._h is None:
            raise RuntimeError('the mesh index is closed')
        return self._h

    def close(self):
        if getattr(self, '_h', None) is not None:
            _ffi.lib().rs_eval_index_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def distance(self, points, max_dist=np.inf):
        """What ``mesh_distance`` returns for these points against the index's mesh, bit for bit
        (rs_eval_index_query)."""
        h = self.handle
        points = _points(points, 'points')
        max_dist = float(max_dist)
        if not max_dist > 0.0:
            raise ValueError('max_dist must be positive (+inf is allowed)')
        n = len(points)
        d2, face, closest = np.empty(n), np.full(n, -1, dtype=np.int32), np.empty((n, 3))
        info = _ffi.EvalInfo()
        if n > 0:
            _ffi.check(_ffi.lib().rs_eval_index_query(
                h, _ffi.ptr(points, _d), n, max_dist, _ffi.ptr(d2, _d), _ffi.ptr(face, _i32),
                _ffi.ptr(closest, _d), _ffi.C.byref(info)))
        return np.sqrt(d2), face, closest, {
            "d2": d2, "cell": self.cell, "cells": tuple(info.cells), "entries": info.entries,
            "largest_cell": info.largest_cell, "tests": info.tests,
            "faces_skipped": info.faces_skipped, "beyond": info.beyond}

    def set_points(self, points):
        """Upload the source cloud of the steps that follow (rs_eval_index_set_points)."""
        h = self.handle
        points = _points(points, 'points')
        if len(points) == 0:
            raise ValueError('the source cloud needs at least one point')
        _ffi.check(_ffi.lib().rs_eval_index_set_points(h, _ffi.ptr(points, _d), len(points)))
        self.n_points = len(points)

    def step(self, s=1.0, R=None, t=None, keep=1.0, max_dist=np.inf, metric="plane",
             origin=None):
        """One registration step of the source cloud under p -> s R p + t (rs_eval_index_step,
        where the step is defined).  Returns dict(matched, kept, k, tests, tau, moments (40))."""
        h = self.handle
        if metric not in REG_METRICS:
            raise ValueError(f'metric must be one of {REG_METRICS}')
        T = np.empty(13)
        T[0] = s
        T[1:10] = np.eye(3).ravel() if R is None else np.asarray(R, dtype=np.float64).reshape(9)
        T[10:] = 0.0 if t is None else np.asarray(t, dtype=np.float64).reshape(3)
        o = _ffi.f64c(self.origin if origin is None else origin).reshape(3)
        rec = _ffi.EvalStep()
        _ffi.check(_ffi.lib().rs_eval_index_step(
            h, _ffi.ptr(T, _d), _ffi.ptr(o, _d), float(keep), float(max_dist),
            REG_METRICS.index(metric), _ffi.C.byref(rec)))
        return {"matched": rec.matched, "kept": rec.kept, "k": rec.k, "tests": rec.tests,
                "tau": rec.tau, "moments": np.array(rec.moments[:])}

    def read(self):
        """(d2, face, closest, kept) of the last step, kept a bool mask (rs_eval_index_read)."""
        h, n = self.handle, self.n_points
        d2, face, closest = np.empty(n), np.empty(n, dtype=np.int32), np.empty((n, 3))
        kept = np.empty(n, dtype=np.uint8)
        _ffi.check(_ffi.lib().rs_eval_index_read(
            h, _ffi.ptr(d2, _d), _ffi.ptr(face, _i32), _ffi.ptr(closest, _d),
            _ffi.ptr(kept, _ffi.C.c_uint8)))
        return d2, face, closest, kept.astype(bool)

    def timing(self, enable):
        """Enable / disable HIP events between the stages of this index's next steps
        (rs_eval_index_timing); returns the last timed step's {stage: device ms}, -1 where
        none."""
        ms = np.zeros(len(REG_STAGES))
        _ffi.check(_ffi.lib().rs_eval_index_timing(self.handle, int(enable), _ffi.ptr(ms, _d)))
        return dict(zip(REG_STAGES, ms.tolist()))


def rotation_exp(omega):
    """Rodrigues' formula: the rotation by |omega| about omega."""
    omega = np.asarray(omega, dtype=np.float64).reshape(3)
    th = float(np.sqrt((omega * omega).sum()))
    K = np.array([[0.0, -omega[2], omega[1]], [omega[2], 0.0, -omega[0]],
                  [-omega[1], omega[0], 0.0]])
    if th < 1e-8:
        a, b = 1.0 - th * th / 6.0, 0.5 - th * th / 24.0
    else:
        a, b = np.sin(th) / th, (1.0 - np.cos(th)) / (th * th)
    return np.eye(3) + a * K + b * (K @ K)


def step_rms(metric, rec):
    """The root mean square a step's record reports for its metric: of the distances (point) or
    of the distances along the matched faces' normals (plane), over the kept points."""
    total = rec["moments"][16 if metric == "point" else 35]
    return float(np.sqrt(total / rec["kept"]))


def step_update(metric, rec, origin, with_scale=True):
    """(ds, dR, dt) from a step's moments: the increment p' -> ds dR p' + dt.

    point: the moments centred (cov = sum y x^T / N - my mx^T, var = sum |x|^2 / N - |mx|^2),
    then the SVD of ``align_similarity``.  plane: J^T J z = -J^T r for z = (omega, u, sigma) by
    np.linalg.lstsq (the minimum-norm solution where the system is singular, as for a planar
    target), sigma dropped without ``with_scale``; dR = Exp(omega), ds = 1 + sigma.  Both are
    taken about ``origin``: dt = origin + u - ds dR origin."""
    mom, origin = rec["moments"], np.asarray(origin, dtype=np.float64)
    if metric == "point":
        N = float(rec["kept"])
        mx, my = mom[0:3] / N, mom[3:6] / N
        cov = mom[6:15].reshape(3, 3) / N - np.outer(my, mx)
        var = mom[15] / N - float((mx * mx).sum())
        U, D, Vt = np.linalg.svd(cov)
        S = np.array([1.0, 1.0, 1.0 if np.linalg.det(U) * np.linalg.det(Vt) >= 0.0 else -1.0])
        dR = (U * S) @ Vt
        ds = float((D * S).sum() / var) if with_scale and var > 0.0 else 1.0
        u = my - ds * dR @ mx
    else:
        A = np.zeros((7, 7))
        A[np.triu_indices(7)] = mom[0:28]
        A = A + np.triu(A, 1).T
        m = 7 if with_scale else 6
        z = np.linalg.lstsq(A[:m, :m], -mom[28:28 + m], rcond=None)[0]
        dR, u = rotation_exp(z[0:3]), z[3:6]
        ds = 1.0 + float(z[6]) if with_scale else 1.0
    return ds, dR, origin + u - ds * dR @ origin


def register(points, vertices, faces, metric="plane", keep=1.0, with_scale=True, init=None,
             max_dist=np.inf, max_iter=50, rtol=1e-6, atol=None, cell=None, index=None,
             ctx=None):
    """Trimmed ICP of a point cloud to a triangle mesh: the similarity (s, R, t) under which
    s R p + t lies on the mesh, from ``init`` = (s, R, t) (the identity when None; the tested
    basin is 20 degrees).

    Every iteration is one rs_eval_index_step on the device -- transform, closest points, the
    exact ``keep`` quantile tau of the matched squared distances (points farther than
    ``max_dist`` are unmatched; ties at tau are kept), the moments over the kept points about the
    centre of the mesh's box -- and ``step_update`` on the host.  ``metric`` "plane" minimises
    the distances along the matched faces' normals and converges quadratically; "point" is the
    closest-point / Umeyama update.  ``index`` reuses a MeshIndex of the mesh (vertices and faces
    are then not looked at); otherwise one is built with ``cell`` and closed again.

    Stops when rms_i <= atol (default 1e-12 of the mesh box's diagonal), when
    |rms_(i-1) - rms_i| <= rtol rms_(i-1), or after ``max_iter`` steps.  The transform returned is
    the one the last step was evaluated under: the last rms, dist and mask belong to it.

    Returns dict(s, R, t, iterations, converged, rms, kept, matched, tau, dist, mask): rms, kept,
    matched and tau hold one entry per step, dist (n) the distances (inf or NaN where unmatched)
    and mask (n) the kept points of the last step.  ValueError before any launch: bad shapes, no
    point, keep outside (0, 1], an unknown metric, an init that is not finite, max_dist not > 0,
    max_iter < 1; and when a step matches no point."""
    points = _points(points, 'points')
    if len(points) == 0:
        raise ValueError('points must hold at least one point')
    if metric not in REG_METRICS:
        raise ValueError(f'metric must be one of {REG_METRICS}')
    keep, max_dist, max_iter = float(keep), float(max_dist), int(max_iter)
    if not 0.0 < keep <= 1.0:
        raise ValueError('keep must be in (0, 1]')
    if not max_dist > 0.0:
        raise ValueError('max_dist must be positive (+inf is allowed)')
    if max_iter < 1:
        raise ValueError('max_iter must be at least 1')
    if init is None:
        s, R, t = 1.0, np.eye(3), np.zeros(3)
    else:
        s, R, t = init
        s, R, t = float(s), np.array(R, dtype=np.float64), np.array(t, dtype=np.float64)
        if R.shape != (3, 3) or t.shape != (3,):
            raise ValueError('init must be (s, R (3, 3), t (3))')
        if not (np.isfinite(s) and np.isfinite(R).all() and np.isfinite(t).all()):
            raise ValueError('init is not finite')
    own = index is None
    if own:
        index = MeshIndex(vertices, faces, cell=cell, ctx=ctx)
    try:
        origin = index.origin
        atol = 1e-12 * index.diagonal if atol is None else float(atol)
        index.set_points(points)
        hist = {"rms": [], "kept": [], "matched": [], "tau": []}
        converged = False
        for it in range(max_iter):
            rec = index.step(s, R, t, keep=keep, max_dist=max_dist, metric=metric, origin=origin)
            if rec["matched"] == 0:
                raise ValueError(f'step {it} matched no point: under the current transform no '
                                 'point lies within max_dist of the mesh')
            rms = step_rms(metric, rec)
            for key, val in (("rms", rms), ("kept", rec["kept"]), ("matched", rec["matched"]),
                             ("tau", rec["tau"])):
                hist[key].append(val)
            if rms <= atol or (it > 0 and abs(hist["rms"][-2] - rms) <= rtol * hist["rms"][-2]):
                converged = True
                break
            if it == max_iter - 1:
                break
            ds, dR, dt = step_update(metric, rec, origin, with_scale)
            s, R, t = ds * s, dR @ R, ds * dR @ t + dt
        d2, _, _, mask = index.read()
    finally:
        if own:
            index.close()
    return {"s": s, "R": R, "t": t, "iterations": len(hist["rms"]), "converged": converged,
            "rms": np.array(hist["rms"]), "kept": np.array(hist["kept"], dtype=np.int64),
            "matched": np.array(hist["matched"], dtype=np.int64), "tau": np.array(hist["tau"]),
            "dist": np.sqrt(d2), "mask": mask}


_register = register   # compare_meshes has a keyword of that name


# ---- global registration -----------------------------------------------------------------------

def ransac_similarity(src, dst, H, inlier_dist, seed=0, with_scale=True, scale=None,
                      edge_tol=0.15, min_edge=0.0, candidates=32, ctx=None):
    """RANSAC over the similarities of three correspondences src[i] <-> dst[i] (rs_sim3_ransac,
    where the sampler, the gates, the closed form and the score are written down).

    Hypothesis h < H draws three correspondences with the Philox / Floyd sampler, passes the
    gates (distinct targets, source edges > ``min_edge``, the three edge ratios within a factor
    1 + ``edge_tol`` of each other -- and of 1 without ``with_scale`` --, ``scale`` = (lo, hi)
    around the scale, (0, inf) when None), takes the similarity that maps one triangle's frame
    onto the other's, and counts the correspondences it brings within ``inlier_dist``.  The count
    alone does not pick the answer: ``global_register`` verifies the candidates against the mesh.

    Returns dict(h (c,) int64, count (c,) int64, s (c,), R (c, 3, 3), t (c, 3), info): the
    c <= ``candidates`` best survivors by (count descending, h ascending); info =
    dict(hypotheses, passed (5,) survivors per gate, tests, found)."""
    src, dst = _points(src, 'src'), _points(dst, 'dst')
    if src.shape != dst.shape:
        raise ValueError('src and dst must have the same shape')
    H, candidates = int(H), int(candidates)
    lo, hi = (0.0, np.inf) if scale is None else (float(scale[0]), float(scale[1]))
    cand = (_ffi.Sim3Candidate * max(candidates, 1))()
    info = _ffi.Sim3Info()
    _ffi.check(_ffi.lib().rs_sim3_ransac(
        _ctx(ctx), _ffi.ptr(src, _d), _ffi.ptr(dst, _d), len(src), H, float(inlier_dist),
        int(seed) & 0xFFFFFFFFFFFFFFFF, int(bool(with_scale)), lo, hi, float(edge_tol),
        float(min_edge), candidates, cand, _ffi.C.byref(info)))
    c = info.found
    model = np.array([cand[i].model[:] for i in range(c)], dtype=np.float64).reshape(c, 13)
    return {"h": np.array([cand[i].h for i in range(c)], dtype=np.int64),
            "count": np.array([cand[i].count for i in range(c)], dtype=np.int64),
            "s": model[:, 0].copy(), "R": model[:, 1:10].reshape(c, 3, 3).copy(),
            "t": model[:, 10:13].copy(),
            "info": {"hypotheses": info.hypotheses, "passed": np.array(info.passed[:]),
                     "tests": info.tests, "found": info.found}}


def face_normals(vertices, faces):
    """Unit normals of the faces, cross(b - a, c - a) normalised (NaN for a face without area)."""
    tri = np.asarray(vertices, dtype=np.float64)[np.asarray(faces).reshape(-1, 3)]
    cr = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    with np.errstate(invalid='ignore', divide='ignore'):
        return cr / np.sqrt((cr * cr).sum(axis=1))[:, None]


def rms_radius(points):
    """The root mean square distance of the finite points from their centroid."""
    p = np.asarray(points, dtype=np.float64)
    p = p[np.isfinite(p).all(axis=1)]
    if len(p) == 0:
        raise ValueError('no finite point')
    return float(np.sqrt(((p - p.mean(axis=0)) ** 2).sum(axis=1).mean()))


def global_correspondences(points, normals, vertices, faces, samples=None, k=32, seed=0,
                           ctx=None):
    """Steps 1 to 3 of ``global_register``: (src (M, 3), dst (M, 3), target (samples, 3)), the
    matched pairs of the cloud and of ``samples`` surface samples of the mesh (as many as the
    cloud has points when None) by nearest FPFH descriptor."""
    from . import cloud
    points = _points(points, 'points')
    samples = len(points) if samples is None else int(samples)
    target, face = sample_surface(vertices, faces, samples, seed)
    fa, _, _ = cloud.fpfh(points, normals, k=k, ctx=ctx)
    fb, _, _ = cloud.fpfh(target, face_normals(vertices, faces)[face], k=k, ctx=ctx)
    idx, _ = cloud.match_features(fa, fb, ctx=ctx)
    ok = idx >= 0
    return points[ok], target[idx[ok]], target


def global_register(points, normals, vertices, faces, samples=None, k=32, H=100000,
                    inlier_dist=None, scale=None, with_scale=True, edge_tol=0.15, min_edge=0.0,
                    candidates=32, keep=0.75, seed=0, refine=True, metric="plane", max_iter=50,
                    index=None, ctx=None):
    """The similarity (s, R, t) that brings an oriented cloud onto a mesh from any pose and
    scale: a coarse, correspondence-based alignment that lands inside the basin of ``register``,
    and with ``refine`` that refinement.

    1. ``samples`` surface samples of the mesh (as many as the cloud has points when None, so
       that both samplings are comparable) with their faces' normals;
    2. ``cloud.fpfh`` on both (``normals`` must point to the side the faces' normals do);
    3. ``cloud.match_features``, the cloud's descriptors against the samples';
    4. ``ransac_similarity`` with ``H`` hypotheses; by default ``scale`` is (0.5, 2) x the ratio
       of the two clouds' rms radii about their centroids (without an interval, collapsed
       hypotheses win) and ``inlier_dist`` 0.03 x the diagonal of the mesh's box;
    5. every candidate is verified by one ``MeshIndex.step(keep=keep, metric="point")`` of the
       whole cloud against the mesh, and the one with the lowest trimmed rms is kept (the first
       among equals): the correspondence count alone picks poses a half turn off;
    6. with ``refine``, ``register(init=...)`` with the same ``keep``, ``metric``, ``with_scale``.

    Returns dict(s, R, t, coarse (s, R, t), coarse_rms (c,), chosen, candidates (what
    ``ransac_similarity`` returned), correspondences, scale, inlier_dist, registration (what
    ``register`` returned, None without ``refine``)).  ValueError when no hypothesis survives the
    gates."""
    points = _points(points, 'points')
    if len(points) < 3:
        raise ValueError('points must hold at least three points')
    own = index is None
    if own:
        index = MeshIndex(vertices, faces, ctx=ctx)
    try:
        src, dst, target = global_correspondences(points, normals, vertices, faces, samples, k,
                                                  seed, ctx)
        if len(src) < 3:
            raise ValueError('fewer than three descriptors found a match')
        if scale is None:
            ratio = rms_radius(target) / rms_radius(points)
            scale = (0.5 * ratio, 2.0 * ratio)
        if inlier_dist is None:
            inlier_dist = 0.03 * index.diagonal
        cand = ransac_similarity(src, dst, H, inlier_dist, seed=seed, with_scale=with_scale,
                                 scale=scale, edge_tol=edge_tol, min_edge=min_edge,
                                 candidates=candidates, ctx=ctx)
        if len(cand["h"]) == 0:
            raise ValueError('no hypothesis survived the gates')
        index.set_points(points)
        rms = np.full(len(cand["h"]), np.inf)
        for c in range(len(rms)):
            rec = index.step(cand["s"][c], cand["R"][c], cand["t"][c], keep=keep, metric="point")
            if rec["kept"] > 0:
                rms[c] = step_rms("point", rec)
        best = int(np.argmin(rms))
        coarse = (float(cand["s"][best]), cand["R"][best].copy(), cand["t"][best].copy())
        reg = None
        if refine:
            reg = _register(points, vertices, faces, metric=metric, keep=keep,
                            with_scale=with_scale, init=coarse, max_iter=max_iter, index=index,
                            ctx=ctx)
    finally:
        if own:
            index.close()
    s, R, t = (reg["s"], reg["R"], reg["t"]) if refine else coarse
    return {"s": s, "R": R, "t": t, "coarse": coarse, "coarse_rms": rms, "chosen": best,
            "candidates": cand, "correspondences": len(src), "scale": tuple(scale),
            "inlier_dist": float(inlier_dist), "registration": reg}


# ---- cameras (host only) ---------------------------------------------------------------------

def nearest_rotation(M):
    """The rotation closest to M (..., 3, 3) in the Frobenius norm: U diag(1, 1, det(U V^T)) V^T."""
    U, _, Vt = np.linalg.svd(np.asarray(M, dtype=np.float64))
    D = np.ones(U.shape[:-2] + (3,))
    D[..., 2] = np.sign(np.linalg.det(U @ Vt))
    return (U * D[..., None, :]) @ Vt


def decompose_projection(P):
    """K, R, t of P ~ K [R | t] by an RQ decomposition of P[:, :3]: K upper triangular with a
    positive diagonal and K[2, 2] = 1, det R = +1.  P is (3, 4) or (n, 3, 4); the overall scale
    and sign of P do not matter.  ValueError for another shape or a singular P[:, :3]."""
    P = np.asarray(P, dtype=np.float64)
    if P.shape[-2:] != (3, 4) or P.ndim not in (2, 3):
        raise ValueError('P must be (3, 4) or (n, 3, 4)')
    if P.ndim == 3:
        parts = [decompose_projection(p) for p in P]
        return tuple(np.array([q[k] for q in parts]).reshape((len(P),) + s)
                     for k, s in enumerate(((3, 3), (3, 3), (3,))))
    det = np.linalg.det(P[:, :3])
    if not np.isfinite(det) or det == 0.0:
        raise ValueError('P[:, :3] is singular or not finite')
    P = P if det > 0.0 else -P
    # M = K R from the QR of the reversed matrix: (J M)^T = Q U  =>  M = (J U^T J)(J Q^T)
    Q, U = np.linalg.qr(P[::-1, :3].T)
    K, R = U.T[::-1, ::-1], Q.T[::-1]
    sign = np.where(np.diag(K) < 0.0, -1.0, 1.0)
    K, R = K * sign, sign[:, None] * R     # det R = +1: det K > 0 and det M > 0
    t = np.linalg.solve(K, P[:, 3])
    return K / K[2, 2], R, t


def align_similarity(src, dst, with_scale=True):
    """Umeyama's alignment: (s, R, t) minimising sum |dst_i - (s R src_i + t)|^2 with R a rotation
    (det +1 also where the best orthogonal map is a reflection) and s = 1 without ``with_scale``.
    src and dst are (n, 3)."""
    src, dst = _points(src, 'src'), _points(dst, 'dst')
    if src.shape != dst.shape or len(src) == 0:
        raise ValueError('src and dst must be (n, 3) with the same n > 0')
    ms, md = src.mean(axis=0), dst.mean(axis=0)
    xs, xd = src - ms, dst - md
    U, D, Vt = np.linalg.svd(xd.T @ xs / len(src))
    S = np.array([1.0, 1.0, 1.0 if np.linalg.det(U) * np.linalg.det(Vt) >= 0.0 else -1.0])
    R = (U * S) @ Vt
    var = (xs * xs).sum() / len(src)
    s = float((D * S).sum() / var) if with_scale and var > 0.0 else 1.0
    return s, R, md - s * R @ ms


def apply_similarity(points, s, R, t):
    """s R p + t for every row p of points."""
    return s * np.asarray(points, dtype=np.float64) @ np.asarray(R).T + np.asarray(t)


def camera_errors(R_est, t_est, R_gt, t_gt, frame=True):
    """Estimated cameras against true ones, x_cam = R X + t each, in the arrays of
    tables.getCamerasForEvaluation: R (n, 3, 3), t (n, 3) or (n, 3, 1).

      1. every estimated R is replaced by its nearest rotation; the largest |R R^T - I| before
         that is ``orthogonality_defect`` (a 12-parameter adjustment leaves R not orthogonal).
         The centres are -R^T t with R as given: the centre the pipeline itself works with
         (tables.py:189-214, rs_cloud_attributes), which is what it is to be charged for.
      2. the estimated centres are aligned to the true ones by align_similarity: (s, R, t).
      3. with ``frame``, one constant rotation of the camera frame F is estimated, the nearest
         rotation to sum_i R_gt,i (R_est,i R^T)^T, and divided out: a resectioning that fixes the
         cameras only up to such a gauge is not charged for it.  Without it F is the identity.

    Returns dict(s, R, t, frame, centre_error (n), rotation_error_deg (n), orthogonality_defect):
    centre_error_i = |s R c_est,i + t - c_gt,i|, rotation_error_deg_i the angle of
    R_gt,i (F R_est,i R^T)^T."""
    R_est, R_gt = (np.asarray(a, dtype=np.float64).reshape(-1, 3, 3) for a in (R_est, R_gt))
    t_est, t_gt = (np.asarray(a, dtype=np.float64).reshape(-1, 3) for a in (t_est, t_gt))
    n = len(R_est)
    if n == 0 or not (len(t_est) == len(R_gt) == len(t_gt) == n):
        raise ValueError('one R and one t per camera, the same number estimated and true, n > 0')
    eye = np.eye(3)
    defect = float(np.abs(R_est @ R_est.transpose(0, 2, 1) - eye).max())
    c_est = -np.einsum('nji,nj->ni', R_est, t_est)
    R_est = nearest_rotation(R_est)
    c_gt = -np.einsum('nji,nj->ni', R_gt, t_gt)
    s, Ra, ta = align_similarity(c_est, c_gt)
    moved = R_est @ Ra.T
    F = nearest_rotation((R_gt @ moved.transpose(0, 2, 1)).sum(axis=0)) if frame else eye
    E = R_gt @ (F @ moved).transpose(0, 2, 1)
    cos = np.clip((np.trace(E, axis1=1, axis2=2) - 1.0) / 2.0, -1.0, 1.0)
    return {"s": s, "R": Ra, "t": ta, "frame": F,
            "centre_error": np.linalg.norm(apply_similarity(c_est, s, Ra, ta) - c_gt, axis=1),
            "rotation_error_deg": np.degrees(np.arccos(cos)),
            "orthogonality_defect": defect}
