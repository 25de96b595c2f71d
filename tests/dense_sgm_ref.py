"""Numpy restatement of the semi-global aggregation (include/rsamd.h: rs_dense_aggregate), the
checker of tests/test_gpu_dense_sgm.py.  fp32 throughout, every line one rounded operation, in
the order the header states them, so the GPU result must equal this one exactly.

It is written whole-line: for one direction the image is walked row by row (or column by column
for the two horizontal directions), and a step updates every line's (D,) vector at once; the
predecessor row is shifted by dx, and the pixels whose predecessor falls outside restart with
L = c.  The kernel's structure (lane groups, wrapped lines, prefetch) appears nowhere.
"""
import numpy as np

DIRECTIONS = ((1, 0), (-1, 0), (0, 1), (0, -1), (1, 1), (-1, -1), (1, -1), (-1, 1))
F = np.float32


def cost(volume):
    """c (D, h, w) float32: 1 - v, and 1 where v is NaN."""
    v = np.asarray(volume)
    assert v.dtype == np.float32 and v.ndim == 3
    with np.errstate(invalid="ignore"):
        return np.where(np.isnan(v), F(1), F(1) - v).astype(np.float32)


def _step(prev, c, p1, p2):
    """L of a set of pixels from their predecessors' L: prev, c are (D, n)."""
    inf = np.full((1,) + prev.shape[1:], np.inf, np.float32)
    m = prev.min(axis=0, keepdims=True)
    below = np.concatenate((inf, prev[:-1])) + p1        # L(q, k-1) + p1
    above = np.concatenate((prev[1:], inf)) + p1         # L(q, k+1) + p1
    t = np.minimum(np.minimum(prev, m + p2), np.minimum(below, above))
    return ((c + t) - m).astype(np.float32)


def path(c, dx, dy, p1, p2):
    """L_r (D, h, w) of one direction r = (dx, dy)."""
    p1, p2 = F(p1), F(p2)
    D, h, w = c.shape
    L = np.empty_like(c)
    if dy == 0:
        xs = range(w) if dx > 0 else range(w - 1, -1, -1)
        for i, x in enumerate(xs):
            L[:, :, x] = c[:, :, x] if i == 0 else _step(L[:, :, x - dx], c[:, :, x], p1, p2)
        return L
    ys = range(h) if dy > 0 else range(h - 1, -1, -1)
    for i, y in enumerate(ys):
        L[:, y] = c[:, y]                                  # no predecessor: the path starts here
        if i == 0:
            continue
        # the pixels x of this row whose predecessor x - dx lies inside the previous row
        x = np.arange(w)
        x = x[(x - dx >= 0) & (x - dx < w)]
        if len(x):
            L[:, y, x] = _step(L[:, y - dy, x - dx], c[:, y, x], p1, p2)
    return L


def aggregate(volume, p1=0.1, p2=1.0, paths=8):
    """S (D, h, w) float32: the direction sums added in direction order."""
    assert paths in (4, 8)
    c = cost(volume)
    S = None
    for dx, dy in DIRECTIONS[:paths]:
        L = path(c, dx, dy, p1, p2)
        S = L if S is None else (S + L).astype(np.float32)
    return S


def select(volume, S):
    """(index int32, delta float32, score float32) of the summed cost S over the valid
    hypotheses of `volume`."""
    volume = np.asarray(volume)
    D, h, w = volume.shape
    valid = ~np.isnan(volume)
    any_ok = valid.any(axis=0)
    masked = np.where(valid, S, np.inf)
    index = np.argmin(masked, axis=0)                      # the first on ties
    yy, xx = np.mgrid[0:h, 0:w]
    s0 = S[index, yy, xx]
    lo, hi = np.maximum(index - 1, 0), np.minimum(index + 1, D - 1)
    three = any_ok & (index > 0) & (index < D - 1) & valid[lo, yy, xx] & valid[hi, yy, xx]
    b, a = S[lo, yy, xx], S[hi, yy, xx]
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        den = ((b - F(2) * s0) + a).astype(np.float32)
        dl = np.clip((F(0.5) * (b - a)) / den, F(-0.5), F(0.5)).astype(np.float32)
    delta = np.where(three & (den > 0), dl, F(0)).astype(np.float32)
    score = np.where(any_ok, volume[index, yy, xx], np.nan).astype(np.float32)
    return np.where(any_ok, index, -1).astype(np.int32), delta, score


def solve(volume, p1=0.1, p2=1.0, paths=8):
    """(index, delta, score, S) of a volume."""
    S = aggregate(volume, p1, p2, paths)
    return select(volume, S) + (S,)
