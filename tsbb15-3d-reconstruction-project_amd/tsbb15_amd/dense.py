"""The dense stage (HIP kernels of dense.hip): plane-sweep depth maps and their fusion into a
dense cloud.  The reference project stops at the sparse cloud of its Harris corners and hands
it to an outside tool; nothing here restates code of it.

  * ``plane_sweep``    winner-takes-all ZNCC plane sweep of one reference view against up to
                       eight source views (rs_dense_plane_sweep)
  * ``aggregate``      semi-global aggregation of a sweep's cost volume and the winner of the
                       summed cost (rs_dense_aggregate)
  * ``plane_sweep_sgm`` the sweep and the aggregation in one call, the volume staying on the
                       device (rs_dense_plane_sweep_sgm)
  * ``refine_depth``   index + sub-index offset -> depth, linear in 1 / depth (host)
  * ``consistency``    per pixel, the number of other views whose depth map agrees
                       (rs_dense_consistency)
  * ``depth_points``   a depth map back-projected to 3D points (host)
  * ``fuse``           the host loop over all views: sweep, refine, count, keep

Conventions: images are 2-D uint8, pixel (x, y) is column x, row y with centres at integers
(``features.corners``, ``Tables.addObs``); cameras are the project's normalised (3, 4) ``C``
and need not hold a rotation; ``K`` is (3, 3) with last row (0, 0, 1); ``P = K @ C = [M | m]``.
The depth of X in a view is ``C[2] @ [X; 1]``; the project's Dino cameras give negative
depths (``depth_sign`` of the wash).  The contract of both kernels stands in include/rsamd.h.
"""
from __future__ import annotations

import numpy as np

from . import _ffi

_d = _ffi.C.c_double
_f = _ffi.C.c_float
_i32 = _ffi.C.c_int32
_u8 = _ffi.C.c_uint8

MAX_SOURCES = 8
MAX_PATCH = 11
MAX_DEPTHS = 4096
MAX_SIDE = 16384
MAX_PIXELS = 1 << 26
MAX_VOLUME = 1 << 28
MAX_VIEWS = 128
STAGES = ("plane_sweep", "consistency")
SGM_MAX_DEPTHS = 256
SGM_MAX_VOLUME = 1 << 27
SGM_STAGES = ("sweep", "aggregate", "select")


def _ctx(ctx):
    return (ctx or _ffi.default_context()).handle


def _image(a, name):
    a = np.asarray(a)
    if a.dtype != np.uint8 or a.ndim != 2:
        raise ValueError(f'{name} must be a 2-D uint8 image')
    return np.ascontiguousarray(a)


def _calibration(K):
    K = _ffi.f64c(K)
    if K.shape != (3, 3) or not np.all(np.isfinite(K)):
        raise ValueError('K must be a finite (3, 3) matrix')
    if not np.array_equal(K[2], (0.0, 0.0, 1.0)):
        raise ValueError('the last row of K must be (0, 0, 1)')
    return K


def _cameras(cams, name):
    cams = _ffi.f64c(cams)
    if cams.ndim == 2:
        cams = cams[None]
    if cams.ndim != 3 or cams.shape[1:] != (3, 4):
        raise ValueError(f'{name} must be (3, 4) cameras')
    if not np.all(np.isfinite(cams)):
        raise ValueError(f'{name} must be finite')
    return cams


def _inverse(M, what):
    """M^-1 of a (3, 3) matrix; ValueError when M is singular to working precision."""
    if not np.linalg.cond(M) < 1e12:
        raise ValueError(f'{what}: K @ C[:, :3] is singular')
    return np.linalg.inv(M)


def _depths(depths):
    depths = _ffi.f64c(depths).reshape(-1)
    if not 1 <= len(depths) <= MAX_DEPTHS:
        raise ValueError('1 to 4096 depth hypotheses')
    if not np.all(np.isfinite(depths)) or np.any(depths == 0.0):
        raise ValueError('depths must be finite and nonzero')
    if np.any((depths > 0.0) != (depths[0] > 0.0)):
        raise ValueError('depths must all have one sign')
    return depths


def plane_warps(ref_cam, src_cams, K):
    """(A, b): per source s the map of a reference pixel p on the plane of depth d to the
    source, q = d A_s p + b_s, with A_s = M_s M_ref^-1 and b_s = m_s - A_s m_ref (fp64)."""
    K = _calibration(K)
    ref = _cameras(ref_cam, 'ref_cam')
    if len(ref) != 1:
        raise ValueError('ref_cam must be one (3, 4) camera')
    src = _cameras(src_cams, 'src_cams')
    Pr = K @ ref[0]
    Minv = _inverse(Pr[:, :3], 'ref_cam')
    A, b = np.empty((len(src), 3, 3)), np.empty((len(src), 3))
    for s, C in enumerate(src):
        Ps = K @ C
        A[s] = Ps[:, :3] @ Minv
        b[s] = Ps[:, 3] - A[s] @ Pr[:, 3]
    return A, b


def plane_sweep(ref_image, ref_cam, src_images, src_cams, K, depths, patch=7, min_var=4.0,
                return_volume=False, ctx=None):
    """Plane-sweep depth of one reference view (rs_dense_plane_sweep).

    ``src_images`` is a sequence (or a (S, h, w) array) of S images of the reference's shape,
    ``src_cams`` their (S, 3, 4) cameras, ``depths`` the (D,) plane depths in the reference
    view (finite, nonzero, of one sign).  Plane k is ``ref_cam[2] @ [X; 1] = depths[k]``.  The
    cost of (pixel, k) is the mean over the valid sources of the ZNCC between the patch x patch
    reference window and the same pixels warped through the plane into the source (bilinear);
    a source counts when the window and all its samples are inside and both windows have
    variance >= min_var (grey levels squared).

    Returns (index, delta, score, nvalid[, volume]): index (h, w) int32 the winning plane (the
    smallest k on ties), -1 where no hypothesis is valid; delta (h, w) float32 the parabola
    vertex through the winner and its two neighbours in [-0.5, 0.5], 0 where a neighbour is
    missing or invalid; score (h, w) float32 the winning cost (NaN at -1); nvalid (h, w) uint8
    the winner's number of sources; volume (D, h, w) float32 with NaN for invalid entries, only
    with ``return_volume`` -- the other outputs do not depend on it.

    ValueError before any launch: patch not odd or outside 3..11, S outside 1..8, D outside
    1..4096, a side not above patch or above 16384, h w > 2^26, D h w > 2^28 with a volume, an
    image not 2-D uint8, mixed shapes, cameras not finite, K's last row not (0, 0, 1), a
    singular reference camera, min_var not finite or <= 0, depths zero, non-finite or of mixed
    sign."""
    ref, src, A, b, depths, patch, min_var = _sweep_args(
        ref_image, ref_cam, src_images, src_cams, K, depths, patch, min_var)
    (h, w), D = ref.shape, len(depths)
    if return_volume and D * h * w > MAX_VOLUME:
        raise ValueError('a cost volume of more than 2^28 entries')
    index = np.empty((h, w), np.int32)
    delta, score = np.empty((h, w), np.float32), np.empty((h, w), np.float32)
    nvalid = np.empty((h, w), np.uint8)
    volume = np.empty((D, h, w), np.float32) if return_volume else None
    _ffi.check(_ffi.lib().rs_dense_plane_sweep(
        _ctx(ctx), _ffi.ptr(ref, _u8), h, w, _ffi.ptr(src, _u8), len(src), _ffi.ptr(A, _d),
        _ffi.ptr(b, _d), _ffi.ptr(depths, _d), D, patch, min_var, _ffi.ptr(index, _i32),
        _ffi.ptr(delta, _f), _ffi.ptr(score, _f), _ffi.ptr(nvalid, _u8),
        _ffi.ptr(volume, _f) if return_volume else None))
    if return_volume:
        return index, delta, score, nvalid, volume
    return index, delta, score, nvalid


def _sweep_args(ref_image, ref_cam, src_images, src_cams, K, depths, patch, min_var):
    """The checked arguments of a sweep: (ref, src (S, h, w), A, b, depths, patch, min_var);
    ValueError as ``plane_sweep`` lists them, but for the volume's size."""
    ref = _image(ref_image, 'ref_image')
    srcs = [_image(s, 'a source image') for s in src_images]
    if not 1 <= len(srcs) <= MAX_SOURCES:
        raise ValueError('1 to 8 source views')
    if any(s.shape != ref.shape for s in srcs):
        raise ValueError('all images must have one shape')
    patch = int(patch)
    if patch % 2 == 0 or not 3 <= patch <= MAX_PATCH:
        raise ValueError('patch must be odd, in 3..11')
    h, w = ref.shape
    if min(h, w) <= patch or max(h, w) > MAX_SIDE:
        raise ValueError('each image side must be above patch and at most 16384')
    if h * w > MAX_PIXELS:
        raise ValueError('more than 2^26 pixels')
    min_var = float(min_var)
    if not np.isfinite(min_var) or not min_var > 0.0:
        raise ValueError('min_var must be finite and positive')
    depths = _depths(depths)
    A, b = plane_warps(ref_cam, src_cams, K)
    if len(A) != len(srcs):
        raise ValueError('one camera per source image')
    if not (np.all(np.isfinite(A)) and np.all(np.isfinite(b))):
        raise ValueError('the plane warps are not finite')
    return ref, np.ascontiguousarray(np.stack(srcs)), A, b, depths, patch, min_var


def _sgm_args(D, h, w, p1, p2, paths):
    """(p1, p2, paths) checked against the aggregation's limits for a (D, h, w) volume."""
    if not 1 <= D <= SGM_MAX_DEPTHS:
        raise ValueError('1 to 256 depth hypotheses for the aggregation')
    if min(h, w) < 1 or max(h, w) > MAX_SIDE:
        raise ValueError('each image side must be in 1..16384')
    if D * h * w > SGM_MAX_VOLUME:
        raise ValueError('a volume of more than 2^27 entries for the aggregation')
    if paths not in (4, 8):
        raise ValueError('paths must be 4 or 8')
    p1, p2 = np.float32(p1), np.float32(p2)
    if not (np.isfinite(p1) and np.isfinite(p2) and 0.0 <= p1 <= p2):
        raise ValueError('p1 and p2 must be finite with 0 <= p1 <= p2')
    return float(p1), float(p2), int(paths)


def aggregate(volume, p1=0.1, p2=1.0, paths=8, return_aggregated=False, ctx=None):
    """Semi-global aggregation of a sweep's cost volume and the winner of the summed cost
    (rs_dense_aggregate; the definition stands in include/rsamd.h).

    ``volume`` is (D, h, w) float32 with NaN for invalid hypotheses, as ``plane_sweep`` returns
    it.  The cost 1 - volume (1 where NaN) is passed along ``paths`` = 4 or 8 directions with
    the penalties ``p1`` for a step of one plane and ``p2`` for a larger jump (float32), and the
    direction sums are added in a fixed order into S.

    Returns (index, delta, score[, S]): index (h, w) int32 the valid hypothesis of smallest S
    (the smallest k on ties), -1 where the pixel has none -- the same -1 set as the sweep's;
    delta (h, w) float32 the parabola vertex of S through the winner and its neighbours in
    [-0.5, 0.5], 0 where a neighbour is missing or invalid, with ``plane_sweep``'s sign, so
    ``refine_depth`` applies unchanged; score (h, w) float32 the winner's own entry of
    ``volume`` (NaN at -1); S (D, h, w) float32 only with ``return_aggregated``.

    ValueError before any launch: a volume not 3-D float32, D outside 1..256, a side above
    16384, D h w > 2^27, paths not 4 or 8, p1 or p2 not finite or not 0 <= p1 <= p2."""
    volume = np.asarray(volume)
    if volume.dtype != np.float32 or volume.ndim != 3:
        raise ValueError('volume must be a (D, h, w) float32 array')
    D, h, w = volume.shape
    p1, p2, paths = _sgm_args(D, h, w, p1, p2, paths)
    volume = np.ascontiguousarray(volume)
    index = np.empty((h, w), np.int32)
    delta, score = np.empty((h, w), np.float32), np.empty((h, w), np.float32)
    agg = np.empty((D, h, w), np.float32) if return_aggregated else None
    _ffi.check(_ffi.lib().rs_dense_aggregate(
        _ctx(ctx), _ffi.ptr(volume, _f), D, h, w, p1, p2, paths, _ffi.ptr(index, _i32),
        _ffi.ptr(delta, _f), _ffi.ptr(score, _f),
        _ffi.ptr(agg, _f) if return_aggregated else None))
    return (index, delta, score, agg) if return_aggregated else (index, delta, score)


def plane_sweep_sgm(ref_image, ref_cam, src_images, src_cams, K, depths, patch=7, min_var=4.0,
                    p1=0.1, p2=1.0, paths=8, return_volume=False, return_aggregated=False,
                    ctx=None):
    """``plane_sweep`` followed by ``aggregate`` in one call (rs_dense_plane_sweep_sgm): the
    volume goes from the sweep kernel to the aggregation in device memory and comes down only
    when asked for.

    Returns (index, delta, score, nvalid[, volume][, S]).  index, delta and score are those of
    ``aggregate`` on the sweep's volume; nvalid is the winner-takes-all winner's number of
    sources, exactly ``plane_sweep``'s; volume is bitwise ``plane_sweep``'s.

    ValueError before any launch: everything ``plane_sweep`` and ``aggregate`` list; D <= 256
    and D h w <= 2^27 hold whether or not a volume is returned."""
    ref, src, A, b, depths, patch, min_var = _sweep_args(
        ref_image, ref_cam, src_images, src_cams, K, depths, patch, min_var)
    (h, w), D = ref.shape, len(depths)
    p1, p2, paths = _sgm_args(D, h, w, p1, p2, paths)
    index = np.empty((h, w), np.int32)
    delta, score = np.empty((h, w), np.float32), np.empty((h, w), np.float32)
    nvalid = np.empty((h, w), np.uint8)
    volume = np.empty((D, h, w), np.float32) if return_volume else None
    agg = np.empty((D, h, w), np.float32) if return_aggregated else None
    _ffi.check(_ffi.lib().rs_dense_plane_sweep_sgm(
        _ctx(ctx), _ffi.ptr(ref, _u8), h, w, _ffi.ptr(src, _u8), len(src), _ffi.ptr(A, _d),
        _ffi.ptr(b, _d), _ffi.ptr(depths, _d), D, patch, min_var, p1, p2, paths,
        _ffi.ptr(index, _i32), _ffi.ptr(delta, _f), _ffi.ptr(score, _f), _ffi.ptr(nvalid, _u8),
        _ffi.ptr(volume, _f) if return_volume else None,
        _ffi.ptr(agg, _f) if return_aggregated else None))
    out = (index, delta, score, nvalid)
    if return_volume:
        out += (volume,)
    if return_aggregated:
        out += (agg,)
    return out


def refine_depth(index, delta, depths):
    """Depth per pixel from the winner and its sub-index offset: 1 / depth is interpolated
    linearly between depths[index] and the neighbour on the side of delta.  NaN at index -1.
    Host numpy, float64."""
    index = np.asarray(index)
    delta = np.asarray(delta, dtype=np.float64)
    inv = 1.0 / np.asarray(depths, dtype=np.float64).reshape(-1)
    ok = index >= 0
    i0 = np.where(ok, index, 0)
    i1 = np.clip(i0 + np.sign(delta).astype(np.int64), 0, len(inv) - 1)
    out = np.full(index.shape, np.nan)
    w = inv[i0] + np.abs(delta) * (inv[i1] - inv[i0])
    out[ok] = 1.0 / w[ok]
    return out


def consistency(depth_maps, cams, K, rel_tol=0.01, ctx=None):
    """Per view and pixel, the number of other views whose depth map agrees
    (rs_dense_consistency).  depth_maps is (V, h, w) float64 with NaN for "no depth", cams
    (V, 3, 4).  Pixel p of view i with depth d is X = M_i^-1 (d p - m_i); in view j it has
    depth d' = cams[j, 2] @ [X; 1] and lands, rounded to nearest, on a pixel whose depth d_j
    agrees when it is finite and |d_j - d'| <= rel_tol |d'|.  Returns count (V, h, w) uint8,
    0 where the depth is NaN.  ValueError: V outside 1..128, shapes that do not match, a
    singular or non-finite camera, rel_tol not finite or negative."""
    K = _calibration(K)
    depth = _ffi.f64c(depth_maps)
    cams = _cameras(cams, 'cams')
    if depth.ndim != 3 or len(depth) != len(cams):
        raise ValueError('depth_maps must be (V, h, w), one per camera')
    V, h, w = depth.shape
    if not 1 <= V <= MAX_VIEWS:
        raise ValueError('1 to 128 views')
    if min(h, w) < 1 or max(h, w) > MAX_SIDE or h * w > MAX_PIXELS or V * h * w > MAX_VOLUME:
        raise ValueError('depth maps of more than 2^26 pixels each or 2^28 in all')
    rel_tol = float(rel_tol)
    if not np.isfinite(rel_tol) or rel_tol < 0.0:
        raise ValueError('rel_tol must be finite and not negative')
    P = np.ascontiguousarray(K @ cams)
    Minv = np.ascontiguousarray([_inverse(p[:, :3], f'camera {i}') for i, p in enumerate(P)])
    count = np.empty((V, h, w), np.uint8)
    _ffi.check(_ffi.lib().rs_dense_consistency(
        _ctx(ctx), _ffi.ptr(depth, _d), V, h, w, _ffi.ptr(P, _d), _ffi.ptr(Minv, _d), rel_tol,
        _ffi.ptr(count, _u8)))
    return count


def depth_points(depth, cam, K):
    """The (h, w, 3) points X = M^-1 (d p - m) of a depth map, NaN where the depth is NaN.
    Host numpy."""
    K = _calibration(K)
    depth = np.asarray(depth, dtype=np.float64)
    P = K @ _cameras(cam, 'cam')[0]
    Minv = _inverse(P[:, :3], 'cam')
    h, w = depth.shape
    y, x = np.mgrid[0:h, 0:w]
    rhs = np.stack((depth * x, depth * y, depth), axis=-1) - P[:, 3]
    return rhs @ Minv.T


def fuse(images, cams, K, depths, neighbours=2, patch=7, min_var=4.0, min_views=2,
         rel_tol=0.01, return_maps=False, smooth=None, outliers=None, ctx=None):
    """Dense cloud of V posed views: every view is swept against its ``neighbours`` nearest
    views by index on either side, the depths are refined, ``consistency`` counts the agreeing
    views over all V maps, and the pixels with count >= min_views are kept.  ``smooth`` =
    (p1, p2) or (p1, p2, paths) sweeps every view with ``plane_sweep_sgm`` instead of
    ``plane_sweep``; None is the winner-takes-all sweep.

    Returns (points (N, 3), grey (N,) in [0, 1], view (N,) int32), view by view in row-major
    pixel order -- ready for ``cloud.surface_normals`` and, with the grey repeated into three
    columns, ``cloud.save_txt``.  With ``return_maps`` a dict follows: index, delta, depth
    (V, h, w), count and keep (V, h, w).  With ``outliers`` = dict(k=..., std_ratio=...) (the
    keywords of ``cloud.remove_outliers``) the three arrays are filtered by its mask; the maps
    are not."""
    cams = _cameras(cams, 'cams')
    V = len(cams)
    if len(images) != V:
        raise ValueError('one image per camera')
    sweep, sweep_kw = plane_sweep, {}
    if smooth is not None:
        if len(smooth) not in (2, 3):
            raise ValueError('smooth must be (p1, p2) or (p1, p2, paths)')
        sweep, sweep_kw = plane_sweep_sgm, dict(zip(("p1", "p2", "paths"), smooth))
    maps = {"index": [], "delta": [], "depth": []}
    for i in range(V):
        nb = [j for j in range(i - neighbours, i + neighbours + 1) if j != i and 0 <= j < V]
        index, delta, _, _ = sweep(images[i], cams[i], [images[j] for j in nb], cams[nb],
                                   K, depths, patch=patch, min_var=min_var, ctx=ctx, **sweep_kw)
        maps["index"].append(index)
        maps["delta"].append(delta)
        maps["depth"].append(refine_depth(index, delta, depths))
    maps = {k: np.stack(v) for k, v in maps.items()}
    maps["count"] = consistency(maps["depth"], cams, K, rel_tol=rel_tol, ctx=ctx)
    maps["keep"] = keep = maps["count"] >= min_views
    pts = [depth_points(maps["depth"][i], cams[i], K)[keep[i]] for i in range(V)]
    grey = [np.asarray(images[i], dtype=np.float64)[keep[i]] / 255.0 for i in range(V)]
    view = np.repeat(np.arange(V, dtype=np.int32), keep.reshape(V, -1).sum(axis=1))
    out = (np.concatenate(pts), np.concatenate(grey), view)
    if outliers is not None:
        from .cloud import remove_outliers
        mask = remove_outliers(out[0], ctx=ctx, **outliers)[0]
        out = tuple(a[mask] for a in out)
    return out + (maps,) if return_maps else out


def table_views(T):
    """(image indices, cameras (V, 3, 4)) of a Tables' views in T_views order: what ``fuse``
    needs of a finished reconstruction (``View.image`` is the index ``addView`` was given)."""
    from .tables import pose_matrix
    index = [int(v.image) for v in T.T_views]
    return index, np.array([pose_matrix(v.camera_pose) for v in T.T_views]).reshape(-1, 3, 4)


def timing(enable, ctx=None):
    """Enable / disable HIP events around the kernel of the next dense calls (rs_dense_timing);
    returns the last timed calls' {plane_sweep, consistency: device ms}, -1 where none."""
    ctx = ctx or _ffi.default_context()
    ms = np.zeros(len(STAGES))
    _ffi.check(_ffi.lib().rs_dense_timing(ctx.handle, int(enable), _ffi.ptr(ms, _d)))
    return dict(zip(STAGES, ms.tolist()))


def sgm_timing(enable, ctx=None):
    """Enable / disable HIP events between the stages of the next ``aggregate`` and
    ``plane_sweep_sgm`` calls (rs_dense_sgm_timing); returns the last timed calls' {sweep,
    aggregate, select: device ms}, -1 where none.  ``aggregate`` has no sweep and leaves that
    slot alone."""
    ctx = ctx or _ffi.default_context()
    ms = np.zeros(len(SGM_STAGES))
    _ffi.check(_ffi.lib().rs_dense_sgm_timing(ctx.handle, int(enable), _ffi.ptr(ms, _d)))
    return dict(zip(SGM_STAGES, ms.tolist()))
