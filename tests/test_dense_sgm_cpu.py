"""The numpy restatement of the semi-global aggregation (tests/dense_sgm_ref.py) against a second,
independent scalar restatement written straight from include/rsamd.h, and what the aggregation
is for: more right winners on a noisy scene.  No GPU.
"""
import numpy as np
import pytest

import dense_fixture as df
import dense_ref as dr
import dense_sgm_ref as sr
from dense_sgm_fixture import noisy_slanted, random_volume

F = np.float32
SHAPES = [(1, 5, 7), (2, 9, 4), (5, 1, 9), (5, 9, 1), (3, 1, 1), (12, 6, 8)]


def scalar_solve(v, p1, p2, paths):
    """(index, delta, score, S) by plain loops over direction, pixel and k; every operation a
    numpy float32 scalar operation."""
    D, h, w = v.shape
    p1, p2 = F(p1), F(p2)
    c = np.empty(v.shape, np.float32)
    for idx, x in np.ndenumerate(v):
        c[idx] = F(1) if np.isnan(x) else F(1) - x
    S = np.zeros(v.shape, np.float32)
    for r, (dx, dy) in enumerate(sr.DIRECTIONS[:paths]):
        L = np.empty(v.shape, np.float32)
        ys = range(h) if dy >= 0 else range(h - 1, -1, -1)
        xs = range(w) if dx >= 0 else range(w - 1, -1, -1)
        for y in ys:
            for x in xs:
                qx, qy = x - dx, y - dy
                if not (0 <= qx < w and 0 <= qy < h):
                    L[:, y, x] = c[:, y, x]
                    continue
                m = min(L[k, qy, qx] for k in range(D))
                for k in range(D):
                    t = min(L[k, qy, qx], m + p2)
                    if k > 0:
                        t = min(t, L[k - 1, qy, qx] + p1)
                    if k < D - 1:
                        t = min(t, L[k + 1, qy, qx] + p1)
                    L[k, y, x] = (c[k, y, x] + t) - m
        S = L if r == 0 else S + L
        assert S.dtype == np.float32
    index = np.full((h, w), -1, np.int32)
    delta = np.zeros((h, w), np.float32)
    score = np.full((h, w), np.nan, np.float32)
    for y in range(h):
        for x in range(w):
            best = -1
            for k in range(D):
                if not np.isnan(v[k, y, x]) and (best < 0 or S[k, y, x] < S[best, y, x]):
                    best = k
            if best < 0:
                continue
            index[y, x], score[y, x] = best, v[best, y, x]
            if 0 < best < D - 1 and not np.isnan(v[best - 1, y, x]) \
                    and not np.isnan(v[best + 1, y, x]):
                b, a = S[best - 1, y, x], S[best + 1, y, x]
                den = (b - F(2) * S[best, y, x]) + a
                if den > 0:
                    delta[y, x] = min(F(0.5), max(F(-0.5), (F(0.5) * (b - a)) / den))
    return index, delta, score, S


@pytest.mark.parametrize("paths", [4, 8])
@pytest.mark.parametrize("shape", SHAPES)
def test_scalar_restatement_equals_vectorised(shape, paths):
    v = random_volume(shape, seed=100 + sum(shape))
    assert np.isnan(v).all(axis=0).any()
    got = sr.solve(v, 0.1, 1.0, paths)
    want = scalar_solve(v, 0.1, 1.0, paths)
    for g, w_, name in zip(got, want, ("index", "delta", "score", "S")):
        assert g.dtype == w_.dtype and g.shape == w_.shape, name
        assert np.array_equal(g, w_, equal_nan=True), name
    assert np.array_equal(got[0] == -1, np.isnan(v).all(axis=0))


@pytest.mark.parametrize("paths", [4, 8])
def test_one_plane_is_a_running_sum(paths):
    """With D = 1: t = L(q), m = L(q), so L(p) = (c(p) + L(q)) - L(q): the restatement's S is
    that running expression summed over the directions, and the index is 0 or -1."""
    v = random_volume((1, 6, 7), seed=5)
    index, delta, score, S = sr.solve(v, 0.1, 1.0, paths)
    c = sr.cost(v)[0]
    h, w = c.shape
    want = None
    for dx, dy in sr.DIRECTIONS[:paths]:
        L = np.empty((h, w), np.float32)
        for y in (range(h) if dy >= 0 else range(h - 1, -1, -1)):
            for x in (range(w) if dx >= 0 else range(w - 1, -1, -1)):
                inside = 0 <= x - dx < w and 0 <= y - dy < h
                L[y, x] = (c[y, x] + L[y - dy, x - dx]) - L[y - dy, x - dx] if inside else c[y, x]
        want = L if want is None else want + L
    assert np.array_equal(S[0], want)
    assert np.array_equal(index, np.where(np.isnan(v[0]), -1, 0))
    assert np.all(delta == 0.0) and np.array_equal(score, v[0], equal_nan=True)


def test_noisy_scene_gains_ten_points():
    imgs, cams, depth = noisy_slanted()
    wta = dr.plane_sweep(imgs[0], cams[0], imgs[1:], cams[1:], df.K, df.DEPTHS, 3, df.MIN_VAR)
    vol = wta[4].astype(np.float32)
    index, _, _, _ = sr.solve(vol, 0.1, 1.0, 8)
    assert np.array_equal(index == -1, wta[0] == -1)
    valid = wta[0] >= 0
    truth = df.true_index(depth[0])
    share = lambda idx: float((np.abs(idx - truth)[valid] <= 1.0).mean())
    s_wta, s_sgm = share(wta[0]), share(index)
    print(f"within one plane of the truth: winner-takes-all {s_wta:.3f}, aggregated {s_sgm:.3f} "
          f"on {int(valid.sum())} valid pixels")
    assert s_sgm >= s_wta + 0.10
