"""numpy restatement of the image front end (tsbb15_amd.features), written from the definitions
in include/rsamd.h: integer structure tensor in int64, response in float64 then cast.  The GPU
tests compare against this, never against the code under test."""
import numpy as np

_SMOOTH = {1: [1], 3: [1, 2, 1], 5: [1, 4, 6, 4, 1], 7: [1, 6, 15, 20, 15, 6, 1]}
_DERIV = {1: [-1, 0, 1], 3: [-1, 0, 1], 5: [-1, -2, 0, 2, 1], 7: [-1, -4, -5, 0, 5, 4, 1]}


def _correlate_rows(a, taps):
    """out[y, x] = sum_t taps[t] * a[y, x + t - r] over the reflect-101 continuation of a."""
    r = len(taps) // 2
    p = np.pad(a, ((0, 0), (r, r)), mode="reflect")
    w = a.shape[1]
    return sum(int(t) * p[:, i:i + w] for i, t in enumerate(taps))


def sobel(image, kernel_size):
    """(Ix, Iy) as exact int64 images."""
    a = np.asarray(image).astype(np.int64)
    sm, de = _SMOOTH[kernel_size], _DERIV[kernel_size]
    ix = _correlate_rows(_correlate_rows(a, de).T, sm).T
    iy = _correlate_rows(_correlate_rows(a, sm).T, de).T
    return ix, iy


def box_sum(a, block_size):
    """Unnormalised block_size^2 window sum, anchor at block_size // 2, reflect-101."""
    lo = block_size // 2
    hi = block_size - 1 - lo
    p = np.pad(a, ((lo, hi), (lo, hi)), mode="reflect")
    h, w = a.shape
    out = np.zeros_like(a)
    for i in range(block_size):
        for j in range(block_size):
            out += p[i:i + h, j:j + w]
    return out


def harris_scale(block_size, kernel_size):
    return 1.0 / (2.0 ** (kernel_size - 1) * block_size * 255.0)


def harris_tensor(image, block_size, kernel_size):
    """The three exact integer box sums (Sxx, Sxy, Syy)."""
    ix, iy = sobel(image, kernel_size)
    return box_sum(ix * ix, block_size), box_sum(ix * iy, block_size), box_sum(iy * iy, block_size)


def harris64(image, block_size, kernel_size, k=0.04):
    """The response in float64 and the magnitude s^4 (|ac| + b^2 + |k| (a + c)^2) its rounding
    error scales with (a, b, c the integer sums)."""
    sxx, sxy, syy = (t.astype(np.float64) for t in harris_tensor(image, block_size, kernel_size))
    s2 = harris_scale(block_size, kernel_size) ** 2
    a, b, c = sxx * s2, sxy * s2, syy * s2
    return (a * c - b * b - k * (a + c) * (a + c),
            np.abs(a * c) + b * b + abs(k) * (a + c) * (a + c))


def harris(image, block_size, kernel_size, k=0.04, raw=False):
    r = harris64(image, block_size, kernel_size, k)[0].astype(np.float32)
    if not raw:
        r[r < 0] = 0
    return r


def non_max_suppression(image, window_size):
    image = np.asarray(image)
    h, w = image.shape
    m = (window_size - 1) // 2
    out = np.zeros_like(image) * image          # 0 * v: the sign the reference's product leaves
    if h > 2 * m and w > 2 * m:
        win = np.lib.stride_tricks.sliding_window_view(image, (window_size, window_size))
        keep = win.max(axis=(2, 3)) == image[m:h - m, m:w - m]
        out[m:h - m, m:w - m] = np.where(keep, image[m:h - m, m:w - m], out[m:h - m, m:w - m])
    return out


def corners(H, rel=0.001):
    H = np.asarray(H)
    if H.size == 0:
        return np.zeros((2, 0), np.int64)
    hit = H.astype(np.float64) > rel * float(H.max())
    return np.flipud(np.vstack(np.nonzero(hit))).astype(np.int64)


def cut_out_rois(image, cols, rows, roi_size):
    m = (roi_size - 1) // 2
    return np.stack([image[r - m:r + m + 1, c - m:c + m + 1] for r, c in zip(rows, cols)]) \
        if len(cols) else np.zeros((0, roi_size, roi_size), image.dtype)


def matching_matrix_rois(r1, r2, wrap=False):
    """|r1[i] - r2[j]|_F.  uint8: exact integer squared distance (differences modulo 256 with
    wrap), then one correctly rounded root.  float64: plain numpy sums."""
    r1, r2 = np.asarray(r1), np.asarray(r2)
    n1, n2 = len(r1), len(r2)
    if r1.dtype == np.uint8:
        a = r1.reshape(n1, 1, -1).astype(np.int64)
        b = r2.reshape(1, n2, -1).astype(np.int64)
        d = a - b
        if wrap:
            d &= 255
        return np.sqrt((d * d).sum(axis=2).astype(np.float64))
    d = r1.reshape(n1, 1, -1) - r2.reshape(1, n2, -1)
    return np.sqrt((d * d).sum(axis=2))


def matching_matrix(img1, xy1, img2, xy2, roi_size, wrap=False):
    return matching_matrix_rois(cut_out_rois(img1, xy1[0], xy1[1], roi_size),
                                cut_out_rois(img2, xy2[0], xy2[1], roi_size), wrap)


def joint_min(A):
    A = np.asarray(A)
    if A.shape[0] == 0 or A.shape[1] == 0:
        return np.zeros(0), np.zeros(0, np.int64), np.zeros(0, np.int64)
    col_mins, row_mins = A.argmin(axis=0), A.argmin(axis=1)
    ci = np.array([c for c, r in enumerate(col_mins) if row_mins[r] == c], np.int64)
    ri = col_mins[ci].astype(np.int64)
    return A[ri, ci], ri, ci


def putative_correspondences(img1, img2, block_size=7, kernel_size=3, nms_window=9, rel=0.001,
                             roi_size=7):
    c = [corners(non_max_suppression(harris(i, block_size, kernel_size), nms_window), rel)
         for i in (img1, img2)]
    _, ri, ci = joint_min(matching_matrix(img1, c[0], img2, c[1], roi_size))
    return c[0][:, ri], c[1][:, ci]
