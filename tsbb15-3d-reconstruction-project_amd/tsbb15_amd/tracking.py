"""The tracking stage on the GPU: from a sequence of grey images to the track array the
reference pipeline reads.

``correspondences.py`` serves ``getCorrByIndices(i, i + 1)`` from an array of tracks in the
layout of ``imgdata/README images.txt`` -- one row per scene point, ``x1 y1 ... xF yF``, ``-1``
where the point was not seen, sub-pixel coordinates -- and ``tables.addNewView`` relies on one
physical point keeping one coordinate per frame.  This module produces that array from images:

  * :func:`pyr_down`, :func:`pyramid`   the integer image pyramid        -> rs_pyr_down
  * :func:`track`                       pyramidal Lucas-Kanade, with the forward-backward test
                                                                         -> rs_klt_track
  * :func:`track_sequence`              Harris corners followed through all frames
  * :class:`Correspondences`            the reference's accessor on such an array

The definition (integer window sums, fp64 steps in one order) is in include/rsamd.h; the
kernels are in csrc/tracking.hip.  There is no CPU fallback: without the library or a GPU the
calls raise.
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np

from . import _ffi

C = _ffi.C
OK, LOST, FLAT, FB = 0, 1, 2, 3   # RS_KLT_*
MAX_WINDOW = 31                   # RS_KLT_MAX_WINDOW
MAX_LEVELS = 8                    # RS_KLT_MAX_LEVELS
MAX_ITER = 1024                   # RS_KLT_MAX_ITER
MAX_FEATURES = 1 << 22            # RS_KLT_MAX_N
MAX_SIDE = 32768                  # RS_IMAGE_MAX_SIDE
MIN_EIG = 1.0   # the smaller eigenvalue of the window's mean structure tensor, in grey levels^2

TrackResult = namedtuple("TrackResult", "pos status residual iters fb")


def _ctx(ctx):
    return ctx or _ffi.default_context()


def timing(enable, ctx=None):
    """Enable / disable HIP events between the stages of the next :func:`track` calls
    (rs_tracking_timing); returns the last timed call's {stage: device ms}, -1 where none."""
    ms = np.zeros(len(_ffi.TRACKING_STAGES))
    _ffi.check(_ffi.lib().rs_tracking_timing(_ctx(ctx).handle, int(enable),
                                             _ffi.ptr(ms, C.c_double)))
    return dict(zip(_ffi.TRACKING_STAGES, ms.tolist()))


def _grey(image, what='image'):
    image = np.asarray(image)
    if image.dtype != np.uint8:
        raise ValueError(f'{what} type must be 8-bit unsigned (np.uint8)')
    if image.ndim != 2:
        raise ValueError(f'{what} must be a 2D array')
    if min(image.shape) < 1 or max(image.shape) > MAX_SIDE:
        raise ValueError(f'{what} sides must be between 1 and {MAX_SIDE}')
    return np.ascontiguousarray(image)


def pyr_down(image, ctx=None):
    """The next pyramid level of a 2-D uint8 image: ((h + 1) // 2, (w + 1) // 2) uint8."""
    img = _grey(image)
    h, w = img.shape
    if h < 3 or w < 3:
        raise ValueError('both sides of a level that is reduced must be at least 3')
    out = np.empty(((h + 1) // 2, (w + 1) // 2), np.uint8)
    _ffi.check(_ffi.lib().rs_pyr_down(_ctx(ctx).handle, _ffi.ptr(img, C.c_uint8), h, w,
                                      _ffi.ptr(out, C.c_uint8)))
    return out


def pyramid(image, levels, ctx=None):
    """[level 0, ..., level levels - 1]; level 0 is the image itself."""
    levels = int(levels)
    if not 1 <= levels <= MAX_LEVELS:
        raise ValueError(f'levels must be between 1 and {MAX_LEVELS}')
    out = [_grey(image)]
    for _ in range(levels - 1):
        out.append(pyr_down(out[-1], ctx=ctx))
    return out


def default_levels(shape, window):
    """The largest level count, at most 4, whose coarsest level still has its shorter side at
    least 2 * window (1 when even the image has not)."""
    side, levels = min(shape), 1
    while levels < 4 and (side + 1) // 2 >= 2 * window:
        side = (side + 1) // 2
        levels += 1
    return levels


def _check_levels(shape, levels):
    h, w = shape
    for _ in range(levels - 1):
        if h < 3 or w < 3:
            raise ValueError('both sides of a level that is reduced must be at least 3')
        h, w = (h + 1) // 2, (w + 1) // 2


def track(img0, img1, pts, window=21, levels=None, max_iter=30, eps=0.01, min_eig=MIN_EIG,
          guess=None, fb_tol=None, ctx=None):
    """Follow the (2, n) positions ``pts`` (x row, y row; float64, sub-pixel) from ``img0`` into
    ``img1``, two 2-D uint8 images of one size.

    Returns ``TrackResult(pos (2, n) f8, status (n) i4, residual (n) f8, iters (n) i4,
    fb (n) f8)``: status OK / LOST / FLAT / FB, the mean absolute grey difference of the window
    at the result, the level-0 iterations, and the forward-backward distance (``fb_tol=None``
    switches that test off).  A status other than OK gives the position (-1, -1) and the
    residual -1.  ``guess`` is an optional (2, n) displacement at level 0."""
    img0, img1 = _grey(img0, 'img0'), _grey(img1, 'img1')
    if img0.shape != img1.shape:
        raise ValueError('the two images must have the same size')
    pts = np.asarray(pts)
    if pts.ndim != 2 or pts.shape[0] != 2:
        raise ValueError('pts must be (2, N): x row, y row')
    n = pts.shape[1]
    if n > MAX_FEATURES:
        raise ValueError(f'more than {MAX_FEATURES} features')
    pts = np.ascontiguousarray(pts, dtype=np.float64)
    window = int(window)
    if window % 2 != 1 or not 3 <= window <= MAX_WINDOW:
        raise ValueError(f'window must be odd, between 3 and {MAX_WINDOW}')
    levels = default_levels(img0.shape, window) if levels is None else int(levels)
    if not 1 <= levels <= MAX_LEVELS:
        raise ValueError(f'levels must be between 1 and {MAX_LEVELS}')
    _check_levels(img0.shape, levels)
    max_iter = int(max_iter)
    if not 1 <= max_iter <= MAX_ITER:
        raise ValueError(f'max_iter must be between 1 and {MAX_ITER}')
    eps, min_eig = float(eps), float(min_eig)
    if not eps >= 0.0:
        raise ValueError('eps must not be negative')
    if not (np.isfinite(min_eig) and min_eig >= 0.0):
        raise ValueError('min_eig must be finite and not negative')
    if fb_tol is None:
        fb_tol = -1.0
    else:
        fb_tol = float(fb_tol)
        if not fb_tol >= 0.0:
            raise ValueError('fb_tol must not be negative (None switches the test off)')
    gp = None
    if guess is not None:
        guess = np.asarray(guess)
        if guess.shape != (2, n):
            raise ValueError('guess must have the shape of pts')
        guess = np.ascontiguousarray(guess, dtype=np.float64)
        gp = _ffi.ptr(guess, C.c_double)
    pos = np.empty((2, n), np.float64)
    status, iters = np.empty(n, np.int32), np.empty(n, np.int32)
    residual, fb = np.empty(n, np.float64), np.empty(n, np.float64)
    h, w = img0.shape
    _ffi.check(_ffi.lib().rs_klt_track(
        _ctx(ctx).handle, _ffi.ptr(img0, C.c_uint8), _ffi.ptr(img1, C.c_uint8), h, w,
        _ffi.ptr(pts, C.c_double), gp, n, window, levels, max_iter, eps, min_eig, fb_tol,
        _ffi.ptr(pos, C.c_double), _ffi.ptr(status, C.c_int32), _ffi.ptr(residual, C.c_double),
        _ffi.ptr(iters, C.c_int32), _ffi.ptr(fb, C.c_double)))
    return TrackResult(pos, status, residual, iters, fb)


def detect(image, block_size=7, kernel_size=3, nms_window=9, rel=0.001, ctx=None):
    """The corners of the front end's chain (Harris, non-maximum suppression, the relative
    threshold) as (2, K) float64, strongest first; equal responses keep their scan order."""
    from . import features
    N = features.non_max_suppression(features.harris(image, block_size, kernel_size, ctx=ctx),
                                     nms_window, ctx=ctx)
    xy = features.corners(N, rel, ctx=ctx)
    order = np.argsort(-N[xy[1], xy[0]].astype(np.float64), kind='stable')
    return xy[:, order].astype(np.float64)


def select_new(candidates, live, min_distance, room):
    """Indices of the candidates ((2, K), strongest first) that start tracks: a candidate is taken
    when its Chebyshev distance to every live position ((2, M)) and to every candidate taken
    before it is larger than ``min_distance``, until ``room`` are taken."""
    taken = []
    pos = [np.asarray(live, np.float64).reshape(2, -1)]
    cand = np.asarray(candidates, np.float64).reshape(2, -1)
    for k in range(cand.shape[1]):
        if len(taken) >= room:
            break
        p = cand[:, k:k + 1]
        if all(np.all(np.abs(q - p).max(axis=0) > min_distance) for q in pos if q.size):
            taken.append(k)
            pos.append(p)
            if len(pos) > 64:   # keep the list of arrays short
                pos = [np.hstack(pos)]
    return np.asarray(taken, np.int64)


def track_sequence(images, max_features=5000, min_distance=8.0, window=21, levels=None,
                   max_iter=30, eps=0.01, min_eig=MIN_EIG, fb_tol=1.0, max_residual=20.0,
                   detector=None, tracker=None, ctx=None):
    """The track array of a sequence of equally sized 2-D uint8 images: (tracks, 2 * frames)
    float64 in the layout ``x1 y1 ... xF yF`` of imgdata/points.txt, -1 where a track was not
    seen.

    Frame 0 starts a track at each of its corners (:func:`detect`, strongest first, thinned by
    :func:`select_new`).  Every later frame is tracked from the one before it by :func:`track`
    with the forward-backward test; a track continues while its status is OK and its residual is
    at most ``max_residual`` (None: no gate), and a track that has ended stays ended.  Then the
    new frame's corners farther than ``min_distance`` (Chebyshev) from every live track start
    new rows, while fewer than ``max_features`` tracks are live.  ``detector(image)`` and
    ``tracker(img0, img1, pts, window=, levels=, max_iter=, eps=, min_eig=, fb_tol=)`` replace
    :func:`detect` and :func:`track`."""
    images = [_grey(im) for im in images]
    if not images:
        raise ValueError('no images')
    if any(im.shape != images[0].shape for im in images):
        raise ValueError('the images must all have the same size')
    max_features = int(max_features)
    if max_features < 1:
        raise ValueError('max_features must be positive')
    if not min_distance >= 0:
        raise ValueError('min_distance must not be negative')
    detector = detector or (lambda im: detect(im, ctx=ctx))
    if tracker is None:
        def tracker(a, b, p, **kw):
            return track(a, b, p, ctx=ctx, **kw)
    F = len(images)
    rows = []                                    # one (2 F) array per track
    live = np.zeros(0, np.int64)                 # rows alive in the current frame

    def start(t, live):
        cand = np.asarray(detector(images[t]), np.float64).reshape(2, -1)
        at = np.array([rows[i][2 * t:2 * t + 2] for i in live]).reshape(-1, 2).T
        new = select_new(cand, at, min_distance, max_features - len(live))
        first = len(rows)
        for k in new:
            row = np.full(2 * F, -1.0)
            row[2 * t:2 * t + 2] = cand[:, k]
            rows.append(row)
        return np.concatenate([live, np.arange(first, first + len(new), dtype=np.int64)])

    live = start(0, live)
    for t in range(1, F):
        if len(live):
            pts = np.array([rows[i][2 * t - 2:2 * t] for i in live]).T
            res = tracker(images[t - 1], images[t], pts, window=window, levels=levels,
                          max_iter=max_iter, eps=eps, min_eig=min_eig, fb_tol=fb_tol)
            pos, status, residual = np.asarray(res[0]), np.asarray(res[1]), np.asarray(res[2])
            keep = status == OK
            if max_residual is not None:
                keep &= residual <= max_residual
            for k in np.nonzero(keep)[0]:
                rows[live[k]][2 * t:2 * t + 2] = pos[:, k]
            live = live[keep]
        live = start(t, live)
    return np.array(rows).reshape(len(rows), 2 * F)


class Correspondences:
    """The reference's ``Correspondences`` on a track array in the points.txt layout: what
    main.py asks for its input, served from :func:`track_sequence`'s result."""

    def __init__(self, tracks):
        tracks = np.asarray(tracks, dtype=np.float64)
        if tracks.ndim != 2 or tracks.shape[1] % 2:
            raise ValueError('tracks must be (N, 2 * frames)')
        self.points = tracks

    @property
    def frames(self):
        return self.points.shape[1] // 2

    def getCorrByIndices(self, i1, i2):
        """(y1, y2), two (K, 2) arrays: the rows seen in both frames, a row counting as seen in
        a frame when any of its two coordinates there differs from -1."""
        for i in (i1, i2):
            if not 0 <= i < self.frames:
                raise ValueError('frame index out of range')
        y1 = self.points[:, i1 * 2:i1 * 2 + 2]
        y2 = self.points[:, i2 * 2:i2 * 2 + 2]
        both = np.any(y1 != -1, axis=1) & np.any(y2 != -1, axis=1)
        return np.array(y1[both, :]), np.array(y2[both, :])
