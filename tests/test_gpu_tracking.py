"""The tracking stage on the GPU (tsbb15_amd.tracking, csrc/tracking.hip) against the numpy
restatement tests/tracking_ref.py -- never against the code under test.  Every comparison is
exact: the bytes of positions, residual and forward-backward distance, equality of status and
iteration count."""
import functools

import numpy as np
import pytest

import tracking_fixture as fx
import tracking_ref as ref
from tsbb15_amd import fun, tracking

pytestmark = pytest.mark.gpu

SMALL, LARGE = (40, 56), (97, 130)
NAMES = ("pos", "status", "residual", "iters", "fb")


def _assert_same(got, want):
    for name, g, w in zip(NAMES, got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, name
        if g.tobytes() != w.tobytes():
            bad = np.nonzero(np.atleast_2d(g != w).any(axis=0))[0]
            raise AssertionError(f"{name} differs at {bad[:8]}: {np.atleast_2d(g)[:, bad[:4]]} "
                                 f"vs {np.atleast_2d(w)[:, bad[:4]]}")


@functools.lru_cache(maxsize=None)
def _pair(shape, shift=(1.7, -1.2), noise=2):
    """A shifted pair with a little integer noise in image 1."""
    img0, img1 = fx.shifted_pair(shape[0], shape[1], shift)
    rs = np.random.RandomState(shape[0])
    img1 = np.clip(img1.astype(np.int64) + rs.randint(-noise, noise + 1, shape), 0, 255)
    img1 = img1.astype(np.uint8)
    img1.setflags(write=False)
    return img0, img1


def _points(shape, n, seed):
    """Fractional positions over the whole image, the border strip included."""
    rs = np.random.RandomState(seed)
    return np.vstack([rs.uniform(0.0, shape[1] - 1.0, n), rs.uniform(0.0, shape[0] - 1.0, n)])


# ------------------------------------------------------------------------------------------
# pyramid
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(3, 3), (3, 8), (8, 3), (5, 6), (33, 47), (64, 64), (65, 129)])
def test_pyr_down(shape):
    img = np.random.RandomState(shape[0] * 131 + shape[1]).randint(0, 256, shape).astype(np.uint8)
    got = tracking.pyr_down(img)
    want = ref.pyr_down(img)
    assert got.dtype == np.uint8 and got.shape == want.shape and np.array_equal(got, want)


def test_pyramid_levels():
    img = _pair(LARGE)[0]
    got, want = tracking.pyramid(img, 4), ref.pyramid(img, 4)
    assert [a.shape for a in got] == [(97, 130), (49, 65), (25, 33), (13, 17)]
    assert all(np.array_equal(a, b) for a, b in zip(got, want))
    with pytest.raises(ValueError):
        tracking.pyr_down(np.zeros((2, 2), np.uint8))


# ------------------------------------------------------------------------------------------
# track against the restatement
# ------------------------------------------------------------------------------------------
# windows 3, 7, 9, 15, 21, 31 have 9, 49, 81, 225, 441, 961 pixels: fewer than the 64 lanes, a
# partial second round, up to 15 full rounds plus one lane.  At 97 x 130 level 3 is 13 x 17,
# where window 31 does not fit: the level is skipped.  Feature counts around the four waves of a
# workgroup and beyond one workgroup.
TRACK_CASES = [
    (3, 1, SMALL, 5), (3, 4, LARGE, 257), (7, 2, SMALL, 64), (7, 1, LARGE, 65),
    (9, 4, SMALL, 65), (9, 2, LARGE, 4), (15, 2, LARGE, 257), (15, 1, SMALL, 1),
    (21, 4, LARGE, 65), (21, 2, SMALL, 3), (31, 4, LARGE, 64), (31, 1, SMALL, 4),
    (31, 2, LARGE, 5),
]


@pytest.mark.parametrize("window,levels,shape,n", TRACK_CASES)
def test_track_matches_restatement(window, levels, shape, n):
    img0, img1 = _pair(shape)
    pts = _points(shape, n, seed=window * 1000 + n)
    pts[:, 0] = shape[1] / 2 + 0.37, shape[0] / 2 - 0.21   # one well inside, whatever the draw
    kw = dict(window=window, levels=levels, max_iter=20, eps=0.01, min_eig=1.0, fb_tol=0.75)
    got = tracking.track(img0, img1, pts, **kw)
    want = ref.track(img0, img1, pts, **kw)
    print(f"status counts {np.bincount(want[1], minlength=4).tolist()}, "
          f"iters up to {want[3].max()}")
    _assert_same(got, want)
    assert want[1][0] == ref.OK
    if n >= 64:
        assert (want[1] == ref.LOST).any()


def test_border_rule():
    """97 x 130, window 15 (r = 7): x = r, x = r - 2^-20, x = w - 2 - r + 0.5, x = w - 1 - r.  On
    a displacement-free pair: OK, LOST, OK, LOST.  On a pair shifted by (+2.4, -1.7) the third
    point walks out of the image while it iterates and ends LOST."""
    h, w, r = LARGE[0], LARGE[1], 7
    xs = [r, r - 2.0 ** -20, w - 2 - r + 0.5, w - 1 - r]
    pts = np.array([xs, [40.25] * 4])
    img = fx.texture(h, w)
    kw = dict(window=15, levels=1, max_iter=20, eps=0.01)
    got, want = tracking.track(img, img, pts, **kw), ref.track(img, img, pts, **kw)
    _assert_same(got, want)
    assert got.status.tolist() == [tracking.OK, tracking.LOST, tracking.OK, tracking.LOST]
    # the same rule along y
    ys = [r, r - 2.0 ** -20, h - 2 - r + 0.5, h - 1 - r]
    pty = np.array([[60.75] * 4, ys])
    got, want = tracking.track(img, img, pty, **kw), ref.track(img, img, pty, **kw)
    _assert_same(got, want)
    assert got.status.tolist() == [tracking.OK, tracking.LOST, tracking.OK, tracking.LOST]
    img0, img1 = fx.shifted_pair(h, w, (2.4, -1.7))
    got, want = tracking.track(img0, img1, pts, **kw), ref.track(img0, img1, pts, **kw)
    _assert_same(got, want)
    assert got.status[2] == tracking.LOST and got.iters[2] >= 1
    assert got.status[0] == tracking.OK


def test_flat_patches_and_bad_points():
    img0, img1 = (np.array(a) for a in _pair(LARGE))
    img0[20:70, 30:90] = 117
    img1[20:70, 30:90] = 117
    pts = np.array([[55.5, 60.25, 100.5, np.nan, np.inf, 50.0, -1e300, 1e300],
                    [40.5, 45.75, 80.5, 40.0, 40.0, np.nan, 40.0, 1e300]])
    for levels in (1, 3):
        got = tracking.track(img0, img1, pts, window=15, levels=levels, fb_tol=1.0)
        want = ref.track(img0, img1, pts, window=15, levels=levels, fb_tol=1.0)
        _assert_same(got, want)
        assert got.status[:2].tolist() == [tracking.FLAT, tracking.FLAT]
        assert (got.status[3:] == tracking.LOST).all()
        assert not any(np.isnan(a).any() for a in got)
        assert np.all(got.pos[:, got.status != tracking.OK] == -1)
        assert np.all(got.residual[got.status != tracking.OK] == -1)


def test_iteration_limits():
    img0, img1 = _pair(LARGE)
    pts = fx.grid_points(LARGE[0], LARGE[1], 12, 40)
    for kw in (dict(max_iter=1, eps=0.0), dict(max_iter=30, eps=1e300), dict(max_iter=30, eps=0.0),
               dict(max_iter=3, eps=1e-4)):
        got = tracking.track(img0, img1, pts, window=9, levels=2, **kw)
        want = ref.track(img0, img1, pts, window=9, levels=2, **kw)
        _assert_same(got, want)
        assert (got.status == tracking.OK).all()
        if kw["max_iter"] == 1 or kw["eps"] > 1:
            assert (got.iters == 1).all()
        else:
            assert 1 < got.iters.max() <= kw["max_iter"]


def test_given_guess():
    """One level cannot follow (-7.25, 5.5) with window 9; with the displacement as the guess
    it can."""
    shift = fx.SHIFTS[2]
    img0, img1 = fx.shifted_pair(LARGE[0], LARGE[1], shift)
    pts = fx.grid_points(LARGE[0], LARGE[1], 20, 33)
    rs = np.random.RandomState(1)
    guess = np.array(shift)[:, None] + rs.uniform(-0.4, 0.4, pts.shape)
    kw = dict(window=9, levels=1, max_iter=20)
    got = tracking.track(img0, img1, pts, guess=guess, **kw)
    _assert_same(got, ref.track(img0, img1, pts, guess=guess, **kw))
    assert (got.status == tracking.OK).all()
    assert np.abs(got.pos - pts - np.array(shift)[:, None]).max() < 0.1
    blind = tracking.track(img0, img1, pts, **kw)
    _assert_same(blind, ref.track(img0, img1, pts, **kw))
    ok = blind.status == tracking.OK
    assert (~ok).any() or np.abs(blind.pos - pts - np.array(shift)[:, None])[:, ok].max() > 1.0
    # with two levels the guess is applied at the top: half of it there
    got = tracking.track(img0, img1, pts, guess=guess, window=9, levels=2)
    _assert_same(got, ref.track(img0, img1, pts, guess=guess, window=9, levels=2))


def test_forward_backward():
    """The right half of image 1 is noise: the left half stays OK, FB appears on the right, every
    status is the restatement's."""
    img0, img1 = fx.shifted_pair(LARGE[0], LARGE[1], (0.6, -0.4))
    img1 = np.array(img1)
    img1[:, 65:] = np.random.RandomState(0).randint(0, 256, (LARGE[0], LARGE[1] - 65))
    pts = np.vstack([np.tile(np.linspace(14.3, 115.7, 24), 3),
                     np.repeat([30.4, 48.6, 66.1], 24)])
    kw = dict(window=15, levels=2, fb_tol=0.5)
    got, want = tracking.track(img0, img1, pts, **kw), ref.track(img0, img1, pts, **kw)
    _assert_same(got, want)
    left = pts[0] < 65 - 12
    assert (got.status[left] == tracking.OK).all()
    assert (got.fb[left] >= 0).all() and (got.fb[left] <= 0.5).all()
    assert (got.status[~left] == tracking.FB).any()
    off = tracking.track(img0, img1, pts, window=15, levels=2)
    _assert_same(off, ref.track(img0, img1, pts, window=15, levels=2))
    assert (off.fb == -1).all() and not (off.status == tracking.FB).any()


def test_no_features():
    img0, img1 = _pair(SMALL)
    got = tracking.track(img0, img1, np.zeros((2, 0)), window=7, fb_tol=1.0)
    assert got.pos.shape == (2, 0) and got.status.shape == (0,) and got.status.dtype == np.int32
    assert got.residual.shape == got.fb.shape == got.iters.shape == (0,)


def test_state_hygiene():
    """The same call twice gives the same bytes; a permutation of the points permutes the
    outputs; a large call followed by a small one on the same context still equals the
    restatement."""
    img0, img1 = _pair(LARGE)
    pts = _points(LARGE, 300, seed=9)
    kw = dict(window=15, levels=3, fb_tol=0.75)
    a = tracking.track(img0, img1, pts, **kw)
    b = tracking.track(img0, img1, pts, **kw)
    _assert_same(b, a)
    perm = np.random.RandomState(2).permutation(pts.shape[1])
    p = tracking.track(img0, img1, pts[:, perm], **kw)
    _assert_same(p, tracking.TrackResult(a.pos[:, perm], a.status[perm], a.residual[perm],
                                         a.iters[perm], a.fb[perm]))
    s0, s1 = _pair(SMALL)
    few = _points(SMALL, 6, seed=4)
    few[:, 0] = 28.4, 19.7
    got = tracking.track(s0, s1, few, window=7, levels=2, fb_tol=0.75)
    _assert_same(got, ref.track(s0, s1, few, window=7, levels=2, fb_tol=0.75))
    assert got.status[0] == tracking.OK


def test_timing_slots():
    img0, img1 = _pair(SMALL)
    tracking.timing(1)
    tracking.track(img0, img1, _points(SMALL, 8, seed=1), window=7, levels=2, fb_tol=1.0)
    ms = tracking.timing(1)
    assert set(ms) == {"pyramid", "forward", "backward"} and all(v >= 0 for v in ms.values())
    tracking.track(img0, img1, _points(SMALL, 8, seed=1), window=7, levels=2)
    ms = tracking.timing(0)
    assert ms["pyramid"] >= 0 and ms["forward"] >= 0 and ms["backward"] == -1


def test_errors_from_the_library(ctx):
    """The C entry point's own RS_EINVAL list, reached past the shim's checks."""
    from tsbb15_amd import _ffi
    C = _ffi.C
    img = np.ascontiguousarray(_pair(SMALL)[0])
    pts, pos = np.zeros((2, 1)), np.zeros((2, 1))
    st, it = np.zeros(1, np.int32), np.zeros(1, np.int32)
    res, fb = np.zeros(1), np.zeros(1)

    def call(h=40, w=56, window=7, levels=2, max_iter=5, eps=0.01, min_eig=1.0, fb_tol=-1.0):
        return _ffi.lib().rs_klt_track(
            ctx.handle, _ffi.ptr(img, C.c_uint8), _ffi.ptr(img, C.c_uint8), h, w,
            _ffi.ptr(pts, C.c_double), None, 1, window, levels, max_iter, eps, min_eig, fb_tol,
            _ffi.ptr(pos, C.c_double), _ffi.ptr(st, C.c_int32), _ffi.ptr(res, C.c_double),
            _ffi.ptr(it, C.c_int32), _ffi.ptr(fb, C.c_double))

    assert call() == _ffi.RS_OK
    for kw in (dict(window=8), dict(window=33), dict(levels=0), dict(levels=9), dict(levels=7),
               dict(max_iter=0), dict(eps=-1.0), dict(eps=float("nan")), dict(min_eig=-1.0),
               dict(fb_tol=float("nan")), dict(h=0)):
        assert call(**kw) == _ffi.RS_EINVAL, kw


# ------------------------------------------------------------------------------------------
# sequences
# ------------------------------------------------------------------------------------------
def test_track_sequence():
    """Four 96 x 128 frames of a texture translating by (1.3, -0.7) per frame, at most 150
    features: the array has the properties tracking_ref.check_sequence states (every
    continuation is the restatement's result for that pair, -1 where it is not OK; ended tracks
    stay ended; rows start only at corners farther than min_distance from the live tracks), and
    its first pair feeds fun.getFFromLabCode."""
    images = [fx.texture(96, 128, (1.3 * t, -0.7 * t)) for t in range(4)]
    kw = dict(window=15, levels=2, max_iter=20, eps=0.01, min_eig=1.0, fb_tol=0.5)
    tracks = tracking.track_sequence(images, max_features=150, min_distance=6.0, max_residual=4.0,
                                     **kw)
    cands = [ref.detect(im) for im in images]
    for im, c in zip(images, cands):     # the same corners in the same order, strongest first
        got = tracking.detect(im)
        assert got.dtype == np.float64 and np.array_equal(got, c)
    continued, ended, later = ref.check_sequence(tracks, images, cands, 150, 6.0, 4.0, **kw)
    print(f"{len(tracks)} tracks: {continued} continuations, {ended} ended, {later} started late")
    assert continued > 100 and ended > 0 and later > 0
    corr = tracking.Correspondences(tracks)
    y1, y2 = corr.getCorrByIndices(0, 1)
    assert y1.shape == y2.shape and y1.shape[1] == 2 and y1.shape[0] >= 20
    assert np.abs(y2 - y1 - [1.3, -0.7]).max() < 0.1
    F = fun.getFFromLabCode(y1.T, y2.T)
    assert np.asarray(F).shape == (3, 3) and np.isfinite(F).all()
