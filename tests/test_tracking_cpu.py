"""The tracking stage without a GPU: the numpy restatement tests/tracking_ref.py against
independent evaluations and known displacements, and the host-side parts of
tsbb15_amd.tracking (the sequence bookkeeping with the restatement injected as the tracker,
Correspondences, the argument checks)."""
import numpy as np
import pytest
from scipy import ndimage

import tracking_fixture as fx
import tracking_ref as ref
from tsbb15_amd import tracking

PYR_SHAPES = [(3, 3), (3, 8), (8, 3), (5, 6), (33, 47), (64, 64), (65, 129)]
H, W = 160, 200


@pytest.mark.parametrize("shape", PYR_SHAPES)
def test_pyr_down_against_float_correlation(shape):
    """The integer pyramid step equals the 5 x 5 binomial correlation evaluated in float64 over
    scipy's "mirror" (reflect-101) continuation, divided by 256 and rounded half up; both are
    exact (the sums are integers below 2^16)."""
    img = np.random.RandomState(shape[0] * 131 + shape[1]).randint(0, 256, shape).astype(np.uint8)
    k = np.array([1.0, 4.0, 6.0, 4.0, 1.0])
    S = ndimage.correlate(img.astype(np.float64), np.outer(k, k), mode="mirror")
    want = np.floor(S[::2, ::2] / 256.0 + 0.5).astype(np.uint8)
    got = ref.pyr_down(img)
    assert got.dtype == np.uint8 and got.shape == ((shape[0] + 1) // 2, (shape[1] + 1) // 2)
    assert np.array_equal(got, want)


def test_pyramid_shapes_and_extremes():
    levels = ref.pyramid(np.full((37, 50), 255, np.uint8), 4)
    assert [a.shape for a in levels] == [(37, 50), (19, 25), (10, 13), (5, 7)]
    assert all((a == 255).all() for a in levels)
    assert (ref.pyr_down(np.zeros((9, 9), np.uint8)) == 0).all()


def _errors(shift, window, levels):
    img0, img1 = fx.shifted_pair(H, W, shift)
    pts = fx.grid_points(H, W, 30, 20)
    pos, status, resid, iters, fb = ref.track(img0, img1, pts, window=window, levels=levels)
    err = np.abs(pos - pts - np.array(shift)[:, None]).max(axis=0)
    return np.where(status == ref.OK, err, np.inf), status


# the worst Chebyshev error the restatement measures over the 120 features of
# test_known_shifts, in pixels
WORST_MEASURED = 0.0311


def test_known_shifts():
    """Three levels recover (0.37, -0.81), (3.3, 2.6) and (-7.25, 5.5) on the analytic texture
    resampled at that offset and quantised to uint8: 20 points at least 30 px from the border,
    windows 15 and 21, 120 features in all.  None may be lost, and the worst Chebyshev error
    stays within 1.5 times the 0.0311 px this restatement measures on these inputs (medians
    0.006 - 0.010 px); the run is deterministic, the margin only absorbs another numpy build."""
    worst = 0.0
    for shift in fx.SHIFTS:
        for window in (15, 21):
            err, status = _errors(shift, window, 3)
            assert (status == ref.OK).all(), (shift, window, status)
            print(f"shift {shift} window {window}: worst {err.max():.4f} median "
                  f"{np.median(err):.4f}")
            worst = max(worst, float(err.max()))
    print(f"worst of all: {worst:.4f}")
    assert worst <= 1.5 * WORST_MEASURED


def test_one_level_does_worse_on_the_large_shift():
    """(-7.25, 5.5) is beyond what one level's window can follow for some points: its worst
    error (a lost feature counts as infinite) exceeds that of three levels, at both windows."""
    for window in (15, 21):
        one, _ = _errors(fx.SHIFTS[2], window, 1)
        three, _ = _errors(fx.SHIFTS[2], window, 3)
        print(f"window {window}: one level {one.max():.3f}, three levels {three.max():.3f}")
        assert one.max() > three.max()


def test_border_rule_and_flat_patches():
    """On a displacement-free pair, at 97 x 130 with window 15 (r = 7): x = r is inside, x just
    below r is not, x = w - 2 - r + 0.5 is inside and x = w - 1 - r is not.  A constant region is
    FLAT, and nothing is NaN."""
    h, w, r = 97, 130, 7
    img = fx.texture(h, w)
    xs = [r, r - 2.0 ** -20, w - 2 - r + 0.5, w - 1 - r]
    pts = np.array([xs, [40.25] * 4])
    pos, status, resid, iters, fb = ref.track(img, img, pts, window=15, levels=2)
    assert status.tolist() == [ref.OK, ref.LOST, ref.OK, ref.LOST]
    assert np.array_equal(pos[:, status == ref.OK], pts[:, status == ref.OK])
    flat = np.array(img)
    flat[20:60, 30:80] = 117
    out = ref.track(flat, flat, np.array([[55.5], [40.5]]), window=15, levels=2)
    assert out[1].tolist() == [ref.FLAT] and out[0].tolist() == [[-1.0], [-1.0]]
    assert not any(np.isnan(a).any() for a in out)


def test_forward_backward_restated():
    """Noise in the right half of image 1: the left half stays OK, FB appears on the right."""
    img0, img1 = fx.shifted_pair(97, 130, (0.6, -0.4))
    img1 = np.array(img1)
    img1[:, 65:] = np.random.RandomState(0).randint(0, 256, (97, 65))
    pts = np.vstack([np.linspace(14.3, 115.7, 24), np.full(24, 48.6)])
    pos, status, resid, iters, fb = ref.track(img0, img1, pts, window=15, levels=2, fb_tol=0.5)
    left = pts[0] < 65 - 12
    assert (status[left] == ref.OK).all() and (fb[left] >= 0).all() and (fb[left] <= 0.5).all()
    assert (status[~left] == ref.FB).any()
    assert np.all(pos[:, status != ref.OK] == -1) and np.all(resid[status != ref.OK] == -1)


def test_correspondences_against_the_reference_rule():
    rs = np.random.RandomState(4)
    pts = rs.uniform(0, 100, (12, 8))
    pts[1, 0:2] = -1          # unseen in frame 0
    pts[2, 2:4] = -1          # unseen in frame 1
    pts[3, 2] = -1            # one -1 only: the row still counts as seen in frame 1
    pts[4, 1] = -1            # likewise in frame 0
    pts[5, 0:4] = -1
    c = tracking.Correspondences(pts)
    for i1, i2 in ((0, 1), (1, 0), (1, 2), (0, 3)):
        y1, y2 = c.getCorrByIndices(i1, i2)
        w1, w2 = ref.correspondences(pts, i1, i2)
        assert y1.shape == w1.shape and np.array_equal(y1, w1) and np.array_equal(y2, w2)
    y1, y2 = c.getCorrByIndices(0, 1)
    assert y1.shape == (9, 2) and -1 in y2 and -1 in y1
    with pytest.raises(ValueError):
        tracking.Correspondences(np.zeros((3, 5)))
    with pytest.raises(ValueError):
        c.getCorrByIndices(0, 4)


def _sequence(frames=4, h=96, w=128):
    return [fx.texture(h, w, (1.3 * t, -0.7 * t)) for t in range(frames)]


def test_track_sequence_bookkeeping():
    """tsbb15_amd.tracking.track_sequence with the restatement injected as detector and
    tracker: the array has the properties tracking_ref.check_sequence states."""
    images = _sequence()
    kw = dict(window=15, levels=2, max_iter=20, eps=0.01, min_eig=1.0, fb_tol=0.5)
    tracks = tracking.track_sequence(images, max_features=150, min_distance=6.0, max_residual=4.0,
                                     detector=ref.detect, tracker=ref.track, **kw)
    cands = [ref.detect(im) for im in images]
    continued, ended, later = ref.check_sequence(tracks, images, cands, 150, 6.0, 4.0, **kw)
    print(f"{len(tracks)} tracks: {continued} continuations, {ended} ended, {later} started late")
    assert continued > 100 and ended > 0 and later > 0
    full = np.all(tracks != -1, axis=1)
    assert full.sum() > 20
    step = tracks[full, 2:4] - tracks[full, 0:2]
    assert np.abs(step - [1.3, -0.7]).max() < 0.1
    # the cap: with room for 10, frame 0 starts exactly the 10 strongest admissible corners
    few = tracking.track_sequence(images[:2], max_features=10, min_distance=6.0,
                                  detector=ref.detect, tracker=ref.track, **kw)
    assert (few[:, 0] != -1).sum() == 10 and (few[:, 2] != -1).sum() <= 10


def test_select_new():
    cand = np.array([[10.0, 12.0, 30.0, 30.0, 50.0], [10.0, 10.0, 10.0, 15.1, 10.0]])
    live = np.array([[50.0], [15.0]])
    assert tracking.select_new(cand, live, 5.0, 10).tolist() == [0, 2, 3]
    assert tracking.select_new(cand, live, 5.0, 2).tolist() == [0, 2]
    assert tracking.select_new(cand, np.zeros((2, 0)), 1.0, 10).tolist() == [0, 1, 2, 3, 4]


def test_default_levels():
    assert tracking.default_levels((576, 720), 21) == 4     # 576 -> 288 -> 144 -> 72 >= 42
    assert tracking.default_levels((160, 200), 21) == 2     # 160 -> 80 -> 40 < 42
    assert tracking.default_levels((40, 56), 21) == 1
    assert tracking.default_levels((4000, 4000), 3) == 4


def test_value_errors_before_the_library():
    img = np.zeros((40, 56), np.uint8)
    pts = np.array([[20.5], [20.5]])
    bad = [
        dict(img0=img.astype(np.float64)), dict(img1=img[:, :50]), dict(img0=img[None]),
        dict(pts=np.zeros((3, 1))), dict(pts=np.zeros(2)),
        dict(window=4), dict(window=1), dict(window=33),
        dict(levels=0), dict(levels=9), dict(levels=7),     # level 5 of 40 x 56 is 2 x 2
        dict(max_iter=0), dict(max_iter=10 ** 6),
        dict(eps=-1.0), dict(eps=float("nan")),
        dict(min_eig=-1.0), dict(min_eig=float("inf")),
        dict(fb_tol=-0.5), dict(fb_tol=float("nan")),
        dict(guess=np.zeros((2, 2))),
    ]
    for kw in bad:
        args = dict(img0=img, img1=img, pts=pts)
        args.update(kw)
        with pytest.raises(ValueError):
            tracking.track(**args)
    with pytest.raises(ValueError):
        tracking.pyr_down(np.zeros((2, 9), np.uint8))
    with pytest.raises(ValueError):
        tracking.pyr_down(np.zeros((9, 9), np.float32))
    with pytest.raises(ValueError):
        tracking.pyramid(img, 0)
    with pytest.raises(ValueError):
        tracking.track_sequence([])
    with pytest.raises(ValueError):
        tracking.track_sequence([img, img[:20]])
    with pytest.raises(ValueError):
        tracking.track_sequence([img], max_features=0)
