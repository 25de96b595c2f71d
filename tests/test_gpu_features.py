"""The image front end on the GPU (tsbb15_amd.features, csrc/features.hip) against the numpy
restatement tests/features_ref.py -- never against the code under test."""
import re

import numpy as np
import pytest

import features_fixture as fx
import features_ref as ref
from tsbb15_amd import features, fun, lab3

pytestmark = pytest.mark.gpu

EPS64 = np.finfo(np.float64).eps
HARRIS_SHAPES = [(37, 53), (130, 70)]
HARRIS_PARAMS = [(2, 3), (7, 3), (3, 5), (5, 7), (2, 1)]


def _texture(h, w, seed):
    return fx.image_pair(h, w, seed)[0]


def _bytes_equal(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


# ------------------------------------------------------------------------------------------
# Harris
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", HARRIS_SHAPES)
@pytest.mark.parametrize("bs,ks", HARRIS_PARAMS)
@pytest.mark.parametrize("raw", [False, True])
def test_harris(shape, bs, ks, raw):
    """|H_gpu - float32(H_ref)| <= 2^-23 |H_ref| + 16 eps64 s^4 (|ac| + b^2 + k (a + c)^2): one
    float32 rounding, plus the fp64 evaluation -- three scalings a, b, c by s^2, two products,
    one sum, one square, one product by k and two subtractions, each within eps64 of a term no
    larger than the bracket (at most 7 roundings on any one path, doubled for the restatement's
    own evaluation: 14 <= 16).  Border pixels are included."""
    img = _texture(*shape, seed=3)
    got = features.harris(img, bs, ks, raw=raw)
    assert got.dtype == np.float32 and got.shape == shape
    R, mag = ref.harris64(img, bs, ks)
    want = R.astype(np.float32).astype(np.float64)
    if not raw:
        want = np.maximum(want, 0.0)
        assert got.min() >= 0.0
    tol = 2.0 ** -23 * np.abs(R) + 16 * EPS64 * mag
    err = np.abs(got.astype(np.float64) - want)
    print(f"max err / tol = {(err / np.maximum(tol, 1e-300)).max():.3g}")
    assert np.all(err <= tol)
    assert (R > 0).any() and (bs != 2 or (R < 0).any())


def test_harris_drop_in_and_errors():
    img = _texture(37, 53, seed=3)
    assert _bytes_equal(lab3.harris(img, 7, 3), features.harris(img, 7, 3))
    with pytest.raises(ValueError, match="block_size"):
        features.harris(img, 32, 3)
    with pytest.raises(ValueError, match="larger"):
        features.harris(img[:8], 7, 3)


# ------------------------------------------------------------------------------------------
# NMS and corners
# ------------------------------------------------------------------------------------------
def _plateau_image():
    rs = np.random.RandomState(5)
    img = np.round(rs.rand(41, 67) * 5).astype(np.float32)
    img[10:14, 20:26] = 8.0
    img[0, 0] = img[40, 66] = 9.0           # border maxima are suppressed
    return img


@pytest.mark.parametrize("win", [1, 3, 9])
@pytest.mark.parametrize("kind", ["harris", "harris_raw", "plateau"])
def test_nms_bitwise(win, kind):
    if kind == "plateau":
        img = _plateau_image()
    else:
        img = ref.harris(_texture(130, 70, seed=3), 7, 3, raw=kind == "harris_raw")
    got = features.non_max_suppression(img, win)
    want = ref.non_max_suppression(img, win)
    assert _bytes_equal(got, want)
    if kind == "plateau" and win == 3:
        assert (got[10:14, 20:26] == 8.0).all() and got[0, 0] == 0.0
    assert _bytes_equal(lab3.non_max_suppression(img, win), want)


def test_corners_bitwise():
    H = ref.harris(_texture(130, 70, seed=3), 7, 3)
    dense = features.corners(H, 0.0)
    assert dense.shape[1] > 2048 * 2                      # many scan chunks
    assert np.array_equal(dense, ref.corners(H, 0.0))
    N = ref.non_max_suppression(H, 9)
    sparse = features.corners(N, 0.001)
    assert 0 < sparse.shape[1] < 200 and np.array_equal(sparse, ref.corners(N, 0.001))
    assert np.array_equal(features.corners(N), ref.corners(N))
    empty = features.corners(np.zeros((37, 53), np.float32))
    assert empty.shape == (2, 0)
    one = np.zeros((37, 53), np.float32)
    one[36, 52] = 2.0                                      # the very last pixel
    assert np.array_equal(features.corners(one), [[52], [36]])


# ------------------------------------------------------------------------------------------
# matching, uint8
# ------------------------------------------------------------------------------------------
def _centres(h, w, n, roi, rs):
    """n centres, the first four at the minimum legal distance from each border, some later
    ones duplicates of earlier ones (tied rows and columns)."""
    m = roi // 2
    xy = np.vstack([rs.randint(m, w - m, n), rs.randint(m, h - m, n)])
    edge = np.array([[m, w - m - 1, m, w - m - 1], [m, m, h - m - 1, h - m - 1]])
    xy[:, :min(4, n)] = edge[:, :min(4, n)]
    for k in range(8, n, 9):
        xy[:, k] = xy[:, k - 5]
    return xy


@pytest.fixture(scope="module")
def u8_pair():
    return fx.image_pair(60, 80, 2)


@pytest.mark.parametrize("n1,n2", [(70, 130), (1, 5), (5, 1)])
@pytest.mark.parametrize("roi", [3, 7, 15])
@pytest.mark.parametrize("wrap", [False, True])
def test_match_u8(u8_pair, n1, n2, roi, wrap):
    img1, _ = u8_pair
    rs = np.random.RandomState(100 * n1 + roi)
    xy1, xy2 = _centres(60, 80, n1, roi, rs), _centres(60, 80, n2, roi, rs)
    if n1 > 8 and n2 > 8:
        xy2[:, 5:8] = xy1[:, 5:8]
    # image 1 on both sides: duplicated centres give zero distances and exact ties
    want = ref.matching_matrix(img1, xy1, img1, xy2, roi, wrap)
    M = features.matching_matrix(img1, xy1, img1, xy2, roi, wrap=wrap)
    assert _bytes_equal(M, want)
    r, c = features.match_argmins(img1, xy1, img1, xy2, roi, wrap=wrap)
    assert np.array_equal(r, want.argmin(axis=1)) and np.array_equal(c, want.argmin(axis=0))
    if n1 > 8 and n2 > 8:
        assert ((want == want.min(axis=1, keepdims=True)).sum(axis=1) > 1).any()
        assert ((want == want.min(axis=0, keepdims=True)).sum(axis=0) > 1).any()
    if not wrap:
        for got, exp in zip(features.match(img1, xy1, img1, xy2, roi), ref.joint_min(want)):
            assert _bytes_equal(np.asarray(got), np.asarray(exp))
        out = features.match(img1, xy1, img1, xy2, roi, return_matrix=True)
        assert len(out) == 4 and _bytes_equal(out[3], want)


def test_match_two_images_and_empty(u8_pair):
    img1, img2 = u8_pair
    rs = np.random.RandomState(9)
    xy1, xy2 = _centres(60, 80, 70, 7, rs), _centres(60, 80, 130, 7, rs)
    want = ref.matching_matrix(img1, xy1, img2, xy2, 7)
    assert _bytes_equal(features.matching_matrix(img1, xy1, img2, xy2, 7), want)
    none = np.zeros((2, 0), np.int64)
    vals, ri, ci = features.match(img1, none, img2, xy2[:, :4], 7)
    assert vals.shape == ri.shape == ci.shape == (0,)
    assert features.matching_matrix(img1, none, img2, xy2[:, :4], 7).shape == (0, 4)


def test_match_errors(u8_pair):
    img1, img2 = u8_pair          # 60 x 80, roi 7: m = 3
    ok = np.array([[10], [10]])
    cases = [(np.array([[10], [57]]), 7, "Row index to high, could not construct ROI"),
             (np.array([[10], [2]]), 7, "Row index to low, could not construct ROI"),
             (np.array([[77], [10]]), 7, "Col index to high, could not construct ROI"),
             (np.array([[2], [10]]), 7, "Col index to low, could not construct ROI"),
             (ok, 6, "ROI size must be odd")]
    for xy, roi, text in cases:
        with pytest.raises(ValueError, match=re.escape(text)):
            features.match(img1, xy, img2, ok, roi)
        with pytest.raises(ValueError, match=re.escape(text)):
            features.matching_matrix(img1, ok, img2, xy, roi)
    # precedence: a high row is reported before a low column
    with pytest.raises(ValueError, match="Row index to high"):
        features.match(img1, np.array([[2, 10], [10, 57]]), img2, ok, 7)
    with pytest.raises(ValueError, match="ROI size above 15"):
        features.match(img1, np.array([[30], [30]]), img2, np.array([[30], [30]]), 17)


def test_matching_matrix_drop_in(u8_pair):
    """fun.matchingMatrix on lists of ROIs: uint8 wraps as the reference does, float64 is plain."""
    img1, img2 = u8_pair
    rs = np.random.RandomState(4)
    xy1, xy2 = _centres(60, 80, 9, 5, rs), _centres(60, 80, 70, 5, rs)
    r1, r2 = ref.cut_out_rois(img1, xy1[0], xy1[1], 5), ref.cut_out_rois(img2, xy2[0], xy2[1], 5)
    assert _bytes_equal(fun.matchingMatrix(list(r1), list(r2)),
                        ref.matching_matrix_rois(r1, r2, wrap=True))
    f1, f2 = r1.astype(np.float64), r2.astype(np.float64)
    assert _bytes_equal(fun.matchingMatrix(list(f1), list(f2)),
                        ref.matching_matrix_rois(r1, r2, wrap=False))


# ------------------------------------------------------------------------------------------
# matching, float64
# ------------------------------------------------------------------------------------------
def test_match_f64():
    rs = np.random.RandomState(12)
    img1, img2 = rs.randn(60, 80) * 40.0, rs.randn(60, 80) * 40.0
    xy1, xy2 = _centres(60, 80, 70, 7, rs), _centres(60, 80, 130, 7, rs)
    img2[:30] = img1[:30]
    xy2[:, 5:8] = xy1[:, 5:8]
    want = ref.matching_matrix(img1, xy1, img2, xy2, 7)
    vals, ri, ci, M = features.match(img1, xy1, img2, xy2, 7, return_matrix=True)
    tol = 2 * 7 * 7 * EPS64
    assert M.shape == (70, 130) and np.all(np.abs(M - want) <= tol * np.abs(want))
    r, c = features.match_argmins(img1, xy1, img2, xy2, 7)
    assert np.array_equal(r, M.argmin(axis=1)) and np.array_equal(c, M.argmin(axis=0))
    for got, exp in zip((vals, ri, ci), ref.joint_min(M)):
        assert _bytes_equal(np.asarray(got), np.asarray(exp))
    assert len(ri) > 3


# ------------------------------------------------------------------------------------------
# the chain, determinism
# ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def chain_ref():
    return {s: ref.putative_correspondences(*fx.image_pair(*s, 1))
            for s in ((96, 128), (200, 260))}


@pytest.mark.parametrize("shape", [(96, 128), (200, 260)])
def test_chain(chain_ref, shape):
    img1, img2 = fx.image_pair(*shape, 1)
    c1, c2 = features.putative_correspondences(img1, img2)
    w1, w2 = chain_ref[shape]
    assert np.array_equal(c1, w1) and np.array_equal(c2, w2)
    assert c1.shape == c2.shape and c1.shape[0] == 2 and c1.shape[1] >= 20
    p1, p2 = np.asarray(c1, np.float64), np.asarray(c2, np.float64)   # getFFromLabCode's input
    assert np.isfinite(p1).all() and np.isfinite(p2).all()


def test_determinism():
    img1, img2 = fx.image_pair(200, 260, 1)
    H = [features.harris(img1, 7, 3) for _ in range(2)]
    assert _bytes_equal(H[0], H[1])
    xy1 = ref.corners(ref.non_max_suppression(ref.harris(img1, 7, 3), 9))
    xy2 = ref.corners(ref.non_max_suppression(ref.harris(img2, 7, 3), 9))
    runs = [features.match(img1, xy1, img2, xy2, 7, return_matrix=True) for _ in range(2)]
    for a, b in zip(*runs):
        assert _bytes_equal(np.asarray(a), np.asarray(b))


def test_timing_events():
    img = _texture(130, 70, seed=3)
    features.timing(1)
    try:
        features.harris(img, 7, 3)
        assert 0.0 < features.timing(1) < 1e3
    finally:
        features.timing(0)
