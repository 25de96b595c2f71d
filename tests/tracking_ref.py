"""numpy restatement of the tracking stage (tsbb15_amd.tracking), written from the definition in
include/rsamd.h: integer pyramids, integer Sobel gradients, 14-bit bilinear weights, exact int64
window sums, and the few fp64 steps in the order the header states them.  Per-feature Python
loops over integer patches.  The GPU tests compare against this, never against the code under
test."""
import numpy as np

import features_ref

OK, LOST, FLAT, FB = 0, 1, 2, 3
_TAPS = (1, 4, 6, 4, 1)


def pyr_down(img):
    """Level l + 1 of a uint8 level l: ((h + 1) / 2, (w + 1) / 2), (S + 128) >> 8."""
    a = np.asarray(img)
    assert a.dtype == np.uint8 and a.ndim == 2 and min(a.shape) >= 3
    h, w = a.shape
    p = np.pad(a.astype(np.int64), 2, mode="reflect")
    rows = sum(t * p[i:i + h, :] for i, t in enumerate(_TAPS))          # (h, w + 4)
    S = sum(t * rows[:, j:j + w] for j, t in enumerate(_TAPS))          # (h, w)
    return ((S[::2, ::2] + 128) >> 8).astype(np.uint8)


def pyramid(img, levels):
    out = [np.ascontiguousarray(img)]
    for _ in range(levels - 1):
        out.append(pyr_down(out[-1]))
    return out


class _Level:
    def __init__(self, img):
        self.v = np.asarray(img).astype(np.int64)
        self.h, self.w = self.v.shape
        self.gx, self.gy = features_ref.sobel(img, 3)


def _inside(qx, qy, w, h, r):
    # NaN and infinity compare false
    return bool(qx >= r and qx < w - 1 - r and qy >= r and qy < h - 1 - r)


def _weights(qx, qy):
    ix, iy = np.floor(qx), np.floor(qy)
    a, b = np.float64(qx) - ix, np.float64(qy) - iy
    w00 = int(np.floor(((1.0 - a) * (1.0 - b)) * 16384.0 + 0.5))
    w01 = int(np.floor((a * (1.0 - b)) * 16384.0 + 0.5))
    w10 = int(np.floor(((1.0 - a) * b) * 16384.0 + 0.5))
    return int(ix), int(iy), (w00, w01, w10, 16384 - w00 - w01 - w10)


def _sample(v, ix, iy, wts, r):
    """The (2r + 1)^2 window of samples around (ix, iy) + fraction, as int64."""
    y0, x0, n = iy - r, ix - r, 2 * r + 1
    w00, w01, w10, w11 = wts
    return (w00 * v[y0:y0 + n, x0:x0 + n] + w01 * v[y0:y0 + n, x0 + 1:x0 + n + 1] +
            w10 * v[y0 + 1:y0 + n + 1, x0:x0 + n] +
            w11 * v[y0 + 1:y0 + n + 1, x0 + 1:x0 + n + 1] + 256) >> 9


def _track_one(P0, P1, px, py, gx, gy, r, max_iter, eps, min_eig):
    """(status, x, y, residual, iters) of one feature from pyramid P0 to pyramid P1."""
    f8 = np.float64
    n = (2 * r + 1) ** 2
    tau = f8(min_eig) * f8(n) * f8(65536.0)
    g = [f8(gx), f8(gy)]
    iters = 0
    d = g
    with np.errstate(all="ignore"):
        eps2 = f8(eps) * f8(eps)
        for l in range(len(P0) - 1, -1, -1):
            a0, a1 = P0[l], P1[l]
            s = f8(0.5) ** l
            plx, ply = f8(px) * s, f8(py) * s
            if not _inside(plx, ply, a0.w, a0.h, r):
                if l == 0:
                    return LOST, -1.0, -1.0, -1.0, iters
                g = [f8(2.0) * g[0], f8(2.0) * g[1]]
                continue
            ix, iy, wts = _weights(plx, ply)
            T = _sample(a0.v, ix, iy, wts, r)
            Gx = _sample(a0.gx, ix, iy, wts, r)
            Gy = _sample(a0.gy, ix, iy, wts, r)
            A, B, C = int((Gx * Gx).sum()), int((Gx * Gy).sum()), int((Gy * Gy).sum())
            Af, Bf, Cf = f8(A), f8(B), f8(C)
            det = Af * Cf - Bf * Bf
            textured = bool(Af + Cf >= f8(2.0) * tau and
                            (Af - tau) * (Cf - tau) - Bf * Bf >= 0.0 and det > 0.0)
            if not textured:
                if l == 0:
                    return FLAT, -1.0, -1.0, -1.0, iters
                g = [f8(2.0) * g[0], f8(2.0) * g[1]]
                continue
            d = [g[0], g[1]]
            for _ in range(max_iter):
                qx, qy = plx + d[0], ply + d[1]
                if not _inside(qx, qy, a1.w, a1.h, r):
                    if l == 0:
                        return LOST, -1.0, -1.0, -1.0, iters
                    break
                jx, jy, jw = _weights(qx, qy)
                E = T - _sample(a1.v, jx, jy, jw, r)
                bx, by = f8(int((E * Gx).sum())), f8(int((E * Gy).sum()))
                dx = (f8(8.0) * (Cf * bx - Bf * by)) / det
                dy = (f8(8.0) * (Af * by - Bf * bx)) / det
                d = [d[0] + dx, d[1] + dy]
                if l == 0:
                    iters += 1
                if dx * dx + dy * dy <= eps2:
                    break
            g = [f8(2.0) * d[0], f8(2.0) * d[1]] if l > 0 else d
            if l == 0:
                qx, qy = plx + d[0], ply + d[1]
                if not _inside(qx, qy, a1.w, a1.h, r):
                    return LOST, -1.0, -1.0, -1.0, iters
                jx, jy, jw = _weights(qx, qy)
                resid = f8(int(np.abs(T - _sample(a1.v, jx, jy, jw, r)).sum())) / f8(32 * n)
                return OK, float(qx), float(qy), float(resid), iters
    raise AssertionError("unreachable")


def track(img0, img1, pts, window=21, levels=3, max_iter=30, eps=0.01, min_eig=1.0, guess=None,
          fb_tol=None):
    """(pos (2, n) f8, status (n) i4, residual (n) f8, iters (n) i4, fb (n) f8).  ``levels`` is a
    count, never None here."""
    pts = np.asarray(pts, np.float64).reshape(2, -1)
    n = pts.shape[1]
    r = window // 2
    P0 = [_Level(a) for a in pyramid(img0, levels)]
    P1 = [_Level(a) for a in pyramid(img1, levels)]
    pos = np.full((2, n), -1.0)
    status = np.zeros(n, np.int32)
    resid = np.full(n, -1.0)
    iters = np.zeros(n, np.int32)
    fb = np.full(n, -1.0)
    gs = np.zeros((2, n)) if guess is None else np.asarray(guess, np.float64).reshape(2, n)
    for i in range(n):
        st, x, y, res, it = _track_one(P0, P1, pts[0, i], pts[1, i], gs[0, i], gs[1, i], r,
                                       max_iter, eps, min_eig)
        iters[i] = it
        if st == OK and fb_tol is not None and fb_tol >= 0:
            bst, bx, by, _, _ = _track_one(P1, P0, x, y, 0.0, 0.0, r, max_iter, eps, min_eig)
            if bst == OK:
                fb[i] = max(abs(np.float64(bx) - pts[0, i]), abs(np.float64(by) - pts[1, i]))
                if fb[i] > fb_tol:
                    st = FB
            else:
                st = FB
        status[i] = st
        if st == OK:
            pos[:, i] = x, y
            resid[i] = res
    return pos, status, resid, iters, fb


def detect(image, block_size=7, kernel_size=3, nms_window=9, rel=0.001):
    """The front end's corners as (2, K) float64, strongest first, ties in scan order."""
    N = features_ref.non_max_suppression(features_ref.harris(image, block_size, kernel_size),
                                         nms_window)
    xy = features_ref.corners(N, rel)
    order = np.argsort(-N[xy[1], xy[0]].astype(np.float64), kind="stable")
    return xy[:, order].astype(np.float64)


def check_sequence(tracks, images, candidates, max_features, min_distance, max_residual, **kw):
    """The properties of a track array (tracks, 2 * frames) over ``images``: every track alive
    in a frame continues exactly where this module's track() puts it (OK and within the residual
    gate) and is -1 otherwise; a track that has ended stays ended; a row starts only at one of
    the frame's ``candidates[t]`` ((2, K)), farther than min_distance (Chebyshev) from every
    track live in that frame before it; never more than max_features are live.  Returns the
    number of (continued, ended, started-after-frame-0) tracks."""
    tracks = np.asarray(tracks)
    F = len(images)
    assert tracks.dtype == np.float64 and tracks.shape[1] == 2 * F
    seen = np.stack([np.any(tracks[:, 2 * t:2 * t + 2] != -1, axis=1) for t in range(F)], axis=1)
    first = seen.argmax(axis=1)
    assert seen.any(axis=1).all()
    assert np.all(np.diff(first) >= 0), "rows are in the order they started"
    continued = ended = 0
    for t in range(1, F):
        alive = np.nonzero(seen[:, t - 1])[0]
        if len(alive):
            pts = tracks[alive, 2 * t - 2:2 * t].T
            pos, st, res, _, _ = track(images[t - 1], images[t], pts, **kw)
            keep = (st == OK) & (res <= max_residual)
            want = np.where(keep, pos, -1.0).T
            assert tracks[alive, 2 * t:2 * t + 2].tobytes() == want.tobytes()
            continued += int(keep.sum())
            ended += int((~keep).sum())
        dead = np.nonzero(~seen[:, t - 1] & (first < t))[0]
        assert not seen[dead, t].any(), "an ended track stays ended"
    for t in range(F):
        assert seen[:, t].sum() <= max_features
        new = np.nonzero(first == t)[0]
        cand = {tuple(c) for c in np.asarray(candidates[t]).T.tolist()}
        for k, i in enumerate(new):
            p = tracks[i, 2 * t:2 * t + 2]
            assert tuple(p.tolist()) in cand
            before = np.concatenate([np.nonzero(seen[:, t] & (first < t))[0], new[:k]])
            if len(before):
                dist = np.abs(tracks[before, 2 * t:2 * t + 2] - p).max(axis=1)
                assert dist.min() > min_distance
    return continued, ended, int((first > 0).sum())


def correspondences(points, i1, i2):
    """The reference's getCorrByIndices on the points.txt layout (x1 y1 ... xF yF per row): a
    row counts as seen in a frame when any of its two coordinates differs from -1."""
    points = np.asarray(points)
    y1 = points[:, i1 * 2:i1 * 2 + 2]
    y2 = points[:, i2 * 2:i2 * 2 + 2]
    seen1 = np.array([np.any(y1 != -1, axis=1)], dtype='bool')
    seen2 = np.array([np.any(y2 != -1, axis=1)], dtype='bool')
    both = np.logical_and(seen1, seen2)
    return np.array(y1[both[0], :]), np.array(y2[both[0], :])
