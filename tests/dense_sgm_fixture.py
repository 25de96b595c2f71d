"""Inputs the tests of the semi-global aggregation share: seeded random volumes with NaNs, and
the noisy slanted scene.  Deterministic; nothing is read from disk."""
import functools

import numpy as np

import dense_fixture as df


def random_volume(shape, seed, nan_share=0.2):
    """A seeded (D, h, w) float32 volume in [-1, 1] with about nan_share NaN entries and one
    pixel column (all k of one pixel) that is NaN throughout."""
    rs = np.random.RandomState(seed)
    v = rs.uniform(-1.0, 1.0, shape).astype(np.float32)
    v[rs.uniform(size=shape) < nan_share] = np.nan
    D, h, w = shape
    v[:, rs.randint(h), rs.randint(w)] = np.nan
    return v


@functools.lru_cache(maxsize=None)
def noisy_slanted():
    """The slanted scene with every image perturbed by N(0, 35) grey levels: (images, cams,
    true depth)."""
    imgs, cams, depth = df.scene("slanted")
    noise = np.random.RandomState(7).normal(0, 35, imgs.shape)
    noisy = np.clip(np.rint(imgs.astype(np.float64) + noise), 0, 255).astype(np.uint8)
    noisy.setflags(write=False)
    return noisy, cams, depth
