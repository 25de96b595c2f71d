"""Synthetic image pairs for the front-end tests: smooth random texture, the second image the
first shifted by a known (dx, dy) plus a little integer noise."""
import functools

import numpy as np
from scipy.ndimage import gaussian_filter

SHIFT = (5, 3)   # (dx, dy): the pixel (x, y) of image 1 is the pixel (x - dx, y - dy) of image 2


@functools.lru_cache(maxsize=None)
def image_pair(h, w, seed=1):
    """Two read-only (h, w) uint8 images."""
    rs = np.random.RandomState(seed)
    base = gaussian_filter(rs.rand(h + 20, w + 20), 1.5)
    base = np.round((base - base.min()) / (base.max() - base.min()) * 255.0).astype(np.uint8)
    dx, dy = SHIFT
    img1 = base[10:10 + h, 10:10 + w].copy()
    noise = rs.randint(-2, 3, size=(h, w))
    img2 = np.clip(base[10 + dy:10 + dy + h, 10 + dx:10 + dx + w].astype(np.int64) + noise,
                   0, 255).astype(np.uint8)
    img1.setflags(write=False)
    img2.setflags(write=False)
    return img1, img2


def true_shift_share(c1, c2):
    """(matches that carry the true shift, matches) of two (2, K) coordinate arrays."""
    d = np.asarray(c1) - np.asarray(c2)
    good = (d[0] == SHIFT[0]) & (d[1] == SHIFT[1])
    return int(good.sum()), int(d.shape[1])
