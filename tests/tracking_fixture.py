"""Inputs of the tracking tests: an analytic texture (a fixed sum of plane waves) that can be
resampled at any sub-pixel offset before it is quantised to uint8, so that the true displacement
between two images is known exactly."""
import functools

import numpy as np

SHIFTS = ((0.37, -0.81), (3.3, 2.6), (-7.25, 5.5))   # (dx, dy): p in image 0 is p + shift in image 1


@functools.lru_cache(maxsize=None)
def _waves(seed):
    rs = np.random.RandomState(seed)
    k = 48
    lam = rs.uniform(4.0, 40.0, k)
    ang = rs.uniform(0.0, 2.0 * np.pi, k)
    return 2.0 * np.pi / lam * np.cos(ang), 2.0 * np.pi / lam * np.sin(ang), \
        rs.uniform(0.0, 2.0 * np.pi, k), np.sqrt(lam)


@functools.lru_cache(maxsize=None)
def texture(h, w, shift=(0.0, 0.0), seed=7):
    """Read-only (h, w) uint8: the texture moved by ``shift`` = (dx, dy)."""
    kx, ky, ph, amp = _waves(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    x, y = x - shift[0], y - shift[1]
    f = np.zeros((h, w))
    for a, b, c, d in zip(kx, ky, ph, amp):
        f += d * np.cos(a * x + b * y + c)
    f *= 45.0 / np.sqrt(0.5 * np.sum(amp * amp))     # standard deviation 45 grey levels
    img = np.clip(np.floor(127.5 + f + 0.5), 0, 255).astype(np.uint8)
    img.setflags(write=False)
    return img


def shifted_pair(h, w, shift, seed=7):
    return texture(h, w, (0.0, 0.0), seed), texture(h, w, tuple(shift), seed)


def grid_points(h, w, margin, count, seed=3):
    """(2, count) fractional positions at least ``margin`` from every border."""
    rs = np.random.RandomState(seed)
    return np.vstack([rs.uniform(margin, w - 1 - margin, count),
                      rs.uniform(margin, h - 1 - margin, count)])
