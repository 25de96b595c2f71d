"""The image front end on the GPU: from two grey images to putative correspondences.

The reference's recipe (fun.py:130-151) is

    lab3.harris -> lab3.non_max_suppression -> H > 0.001 * max(H) -> lab3.cut_out_rois
    -> fun.matchingMatrix -> lab3.joint_min

and every step with arithmetic runs in csrc/features.hip:

  * :func:`harris`                  lab3.py:131-157 -> rs_harris
  * :func:`non_max_suppression`     lab3.py:160-185 -> rs_non_max_suppression
  * :func:`corners`                 fun.py:135-138  -> rs_corners
  * :func:`matching_matrix`, :func:`match`
                                    lab3.py:565-602 + fun.py:113-120 + the argmins of
                                    lab3.py:551-552 -> rs_match_rois_u8 / rs_match_rois_f64
  * :func:`joint_min`, :func:`cut_out_rois`   host helpers without arithmetic
  * :func:`putative_correspondences`          the whole chain

There is no CPU fallback: without the library or a GPU the calls raise.
"""
from __future__ import annotations

import numpy as np

from . import _ffi

C = _ffi.C
HARRIS_K = 0.04              # lab3.py:154
MAX_BLOCK_SIZE = 31          # RS_HARRIS_MAX_BLOCK
MAX_ROI_SIZE = 15            # RS_MATCH_MAX_ROI
MAX_PATCHES = 32768          # RS_MATCH_MAX_N
MAX_PAIRS = 1 << 28          # RS_MATCH_MAX_PAIRS


def _ctx(ctx):
    return ctx or _ffi.default_context()


def timing(enable, ctx=None):
    """Enable / disable HIP events around the kernels of the next calls of this module
    (rs_features_timing); returns the last timed call's device ms, -1 when none."""
    ms = C.c_double(0.0)
    _ffi.check(_ffi.lib().rs_features_timing(_ctx(ctx).handle, int(enable), C.byref(ms)))
    return ms.value


def harris(image, block_size, kernel_size, k=HARRIS_K, raw=False, ctx=None):
    """Harris response of a 2-D uint8 image as float32 (h, w), negatives set to zero
    (``raw=True``: the unclamped response).  The definition is in include/rsamd.h."""
    image = np.asarray(image)
    if kernel_size not in (1, 3, 5, 7):
        raise ValueError('kernel_size must be 1, 3, 5, or 7')
    if not image.dtype == np.uint8:
        raise ValueError('Image type must be 8-bit unsigned (np.uint8)')
    if image.ndim == 3:
        raise ValueError('colour images are not converted here (OpenCV\'s fixed-point grey '
                         'conversion is not reproduced): convert to a 2-D uint8 image first')
    if image.ndim != 2:
        raise ValueError('image must be a 2D array')
    img = np.ascontiguousarray(image)
    h, w = img.shape
    out = np.empty((h, w), dtype=np.float32)
    _ffi.check(_ffi.lib().rs_harris(_ctx(ctx).handle, _ffi.ptr(img, C.c_uint8), h, w,
                                    int(block_size), int(kernel_size), float(k),
                                    1 if raw else 0, _ffi.ptr(out, C.c_float)))
    return out


def non_max_suppression(image, window_size, ctx=None):
    """``image`` (2-D float32) with every pixel that is not the maximum of its window, or lies
    nearer than (window_size - 1) / 2 to a border, set to zero."""
    image = np.asarray(image)
    if not window_size % 2 == 1:
        raise ValueError('window_size must be odd')
    if not image.ndim == 2:
        raise ValueError('image must be single channel (i.e. a 2D array)')
    if image.dtype != np.float32:
        raise ValueError('image must be float32 (the dtype lab3.harris returns)')
    img = np.ascontiguousarray(image)
    h, w = img.shape
    out = np.empty((h, w), dtype=np.float32)
    if h * w == 0:
        return out
    _ffi.check(_ffi.lib().rs_non_max_suppression(_ctx(ctx).handle, _ffi.ptr(img, C.c_float), h, w,
                                                 int(window_size), _ffi.ptr(out, C.c_float)))
    return out


def corners(H, rel=0.001, ctx=None):
    """(2, K) int64 positions -- row 0 x (column), row 1 y (row) -- where
    ``float64(H) > rel * float64(H.max())``, in row-major scan order: what
    ``np.flipud(np.vstack(np.nonzero(H > rel * H.max())))`` lists (fun.py:135-138)."""
    H = np.asarray(H)
    if H.ndim != 2 or H.dtype != np.float32:
        raise ValueError('H must be a 2D float32 array')
    H = np.ascontiguousarray(H)
    h, w = H.shape
    if h * w == 0:
        return np.zeros((2, 0), dtype=np.int64)
    buf = np.empty((2, h * w), dtype=np.int32)
    n = C.c_int64(0)
    _ffi.check(_ffi.lib().rs_corners(_ctx(ctx).handle, _ffi.ptr(H, C.c_float), h, w, float(rel),
                                     _ffi.ptr(buf, C.c_int32), h * w, C.byref(n)))
    return buf[:, :n.value].astype(np.int64)


def _check_centres(image, col_indices, row_indices, roi_size):
    """The checks of lab3.py:585-599, in the reference's precedence."""
    if not roi_size % 2 == 1:
        raise ValueError('ROI size must be odd')
    m = (roi_size - 1) // 2
    R, Cn = image.shape
    row_indices, col_indices = np.array(row_indices), np.array(col_indices)
    if np.any(R - m <= row_indices):
        raise ValueError('Row index to high, could not construct ROI')
    elif np.any(m > row_indices):
        raise ValueError('Row index to low, could not construct ROI')
    elif np.any(Cn - m <= col_indices):
        raise ValueError('Col index to high, could not construct ROI')
    elif np.any(m > col_indices):
        raise ValueError('Col index to low, could not construct ROI')
    return row_indices, col_indices, m


def cut_out_rois(image, col_indices, row_indices, roi_size):
    """lab3.py:565-602: the list of roi_size x roi_size views around (col, row) centres.  A host
    helper; :func:`match` gathers the patches on the GPU and never calls it."""
    image = np.asarray(image)
    row_indices, col_indices, m = _check_centres(image, col_indices, row_indices, roi_size)
    return [image[r - m:r + m + 1, c - m:c + m + 1] for r, c in zip(row_indices, col_indices)]


def joint_min(A):
    """lab3.py:529-563 on a given matrix: (vals, ri, ci) of the elements that are the minimum
    of both their row and their column, in ascending column order."""
    A = np.asarray(A)
    return _joint(np.argmin(A, axis=1), np.argmin(A, axis=0),
                  lambda ri, ci: np.array([A[i, j] for i, j in zip(ri, ci)]))


def _joint(row_mins, col_mins, values):
    cols = np.arange(len(col_mins))
    keep = row_mins[col_mins] == cols if len(row_mins) else np.zeros(len(cols), bool)
    ci = cols[keep]
    ri = np.asarray(col_mins)[keep]
    return values(ri, ci), ri.astype(np.int64), ci.astype(np.int64)


def _image_pair(img1, img2):
    img1, img2 = np.asarray(img1), np.asarray(img2)
    if img1.ndim != 2 or img2.ndim != 2:
        raise ValueError('images must be 2D arrays')
    if img1.dtype == np.uint8 and img2.dtype == np.uint8:
        return np.ascontiguousarray(img1), np.ascontiguousarray(img2), True
    if img1.dtype == np.float64 and img2.dtype == np.float64:
        if not (np.isfinite(img1).all() and np.isfinite(img2).all()):
            raise ValueError('images must be finite')
        return np.ascontiguousarray(img1), np.ascontiguousarray(img2), False
    raise ValueError('images must both be uint8 or both be float64')


def _centres(image, xy, roi_size):
    xy = np.asarray(xy)
    if xy.ndim != 2 or xy.shape[0] != 2:
        raise ValueError('patch centres must be (2, N): x row, y row')
    if xy.size and not np.issubdtype(xy.dtype, np.integer):
        if not np.array_equal(xy, np.floor(xy)):
            raise ValueError('patch centres must be integers')
    _check_centres(image, xy[0], xy[1], roi_size)
    return np.ascontiguousarray(xy, dtype=np.int32)


def _match(img1, xy1, img2, xy2, roi_size, wrap, want_matrix, ctx):
    """(row_min, col_min, row_val, M or None) of the patch-distance matrix."""
    img1, img2, is_u8 = _image_pair(img1, img2)
    roi_size = int(roi_size)
    c1, c2 = _centres(img1, xy1, roi_size), _centres(img2, xy2, roi_size)
    if roi_size > MAX_ROI_SIZE:
        raise ValueError(f'ROI size above {MAX_ROI_SIZE}')
    if wrap and not is_u8:
        raise ValueError('wrap applies to uint8 images only')
    n1, n2 = c1.shape[1], c2.shape[1]
    row_min, col_min = np.empty(n1, np.int32), np.empty(n2, np.int32)
    row_val = np.empty(n1, np.float64)
    M = np.empty((n1, n2), np.float64) if want_matrix else None
    if n1 == 0 or n2 == 0:
        # np.argmin of an empty axis raises in the reference; here: no row or column has a
        # partner, so there is no match
        return row_min[:0], col_min[:0], row_val[:0], M
    mp = _ffi.ptr(M, C.c_double) if want_matrix else None
    L, h = _ffi.lib(), _ctx(ctx).handle
    if is_u8:
        _ffi.check(L.rs_match_rois_u8(
            h, _ffi.ptr(img1, C.c_uint8), img1.shape[0], img1.shape[1], _ffi.ptr(c1, C.c_int32),
            n1, _ffi.ptr(img2, C.c_uint8), img2.shape[0], img2.shape[1], _ffi.ptr(c2, C.c_int32),
            n2, roi_size, 1 if wrap else 0, _ffi.ptr(row_min, C.c_int32),
            _ffi.ptr(col_min, C.c_int32), _ffi.ptr(row_val, C.c_double), mp))
    else:
        _ffi.check(L.rs_match_rois_f64(
            h, _ffi.ptr(img1, C.c_double), img1.shape[0], img1.shape[1], _ffi.ptr(c1, C.c_int32),
            n1, _ffi.ptr(img2, C.c_double), img2.shape[0], img2.shape[1], _ffi.ptr(c2, C.c_int32),
            n2, roi_size, _ffi.ptr(row_min, C.c_int32), _ffi.ptr(col_min, C.c_int32),
            _ffi.ptr(row_val, C.c_double), mp))
    return row_min, col_min, row_val, M


def matching_matrix(img1, xy1, img2, xy2, roi_size, wrap=False, ctx=None):
    """M[i, j] = ||roi1_i - roi2_j||_F as (n1, n2) float64, the ROIs being the roi_size x
    roi_size patches around the (2, n) centres ``xy`` (x row, y row).  ``wrap=True`` (uint8
    only) takes the differences modulo 256, as the reference's uint8 subtraction does."""
    return _match(img1, xy1, img2, xy2, roi_size, wrap, True, ctx)[3]


def match_argmins(img1, xy1, img2, xy2, roi_size, wrap=False, ctx=None):
    """(row_min (n1), col_min (n2)): np.argmin of the matching matrix along its rows and its
    columns, without the matrix."""
    r, c, _, _ = _match(img1, xy1, img2, xy2, roi_size, wrap, False, ctx)
    return r.astype(np.int64), c.astype(np.int64)


def match(img1, xy1, img2, xy2, roi_size, return_matrix=False, ctx=None):
    """Joint minima of the matching matrix (true differences): (vals, ri, ci) as
    ``lab3.joint_min(matchingMatrix(...))`` returns them, and the matrix when asked."""
    row_min, col_min, row_val, M = _match(img1, xy1, img2, xy2, roi_size, False, return_matrix,
                                          ctx)
    out = _joint(row_min, col_min, lambda ri, ci: row_val[ri])
    return out + (M,) if return_matrix else out


def putative_correspondences(img1, img2, block_size=7, kernel_size=3, nms_window=9, rel=0.001,
                             roi_size=7, ctx=None):
    """The recipe of fun.py:130-151 on two 2-D uint8 images: (coords1[:, ri], coords2[:, ci]),
    two (2, K) int64 arrays of matched corner positions (x row, y row), ready for
    ``fun.getFFromLabCode``."""
    coords = []
    for img in (img1, img2):
        H = non_max_suppression(harris(img, block_size, kernel_size, ctx=ctx), nms_window, ctx=ctx)
        coords.append(corners(H, rel, ctx=ctx))
    _, ri, ci = match(img1, coords[0], img2, coords[1], roi_size, ctx=ctx)
    return coords[0][:, ri], coords[1][:, ci]


def matching_matrix_rois(roi1, roi2, ctx=None):
    """fun.matchingMatrix (fun.py:113-120) on two lists of equally sized square ROIs: the ROIs
    of a list are stacked into one tall image and matched by the same kernels.  uint8 ROIs
    wrap modulo 256 as the reference's subtraction does; every other dtype is taken as float64."""
    stacks, centres, side = [], [], None
    n1, n2 = len(roi1), len(roi2)
    if n1 == 0 or n2 == 0:
        return np.empty((n1, n2))
    u8 = all(np.asarray(r).dtype == np.uint8 for r in list(roi1) + list(roi2))
    for rois in (roi1, roi2):
        a = np.stack([np.asarray(r) for r in rois])
        if a.ndim != 3 or a.shape[1] != a.shape[2] or a.shape[1] % 2 != 1:
            raise ValueError('ROIs must be square with an odd side')
        if side not in (None, a.shape[1]):
            raise ValueError('ROIs must all have the same size')
        side = a.shape[1]
        stacks.append(a.reshape(-1, side) if u8 else a.reshape(-1, side).astype(np.float64))
        k = np.arange(a.shape[0])
        centres.append(np.vstack([np.full_like(k, side // 2), k * side + side // 2]))
    return matching_matrix(stacks[0], centres[0], stacks[1], centres[1], side, wrap=u8, ctx=ctx)
