"""The image front end without a GPU: the numpy restatement (tests/features_ref.py) against the
reference's recorded outputs (tests/golden/features.npz) and against closed forms, the host
helpers of tsbb15_amd.features, the C ABI surface, and the pipeline condition of the chain."""
import re

import numpy as np
import pytest

import features_fixture as fx
import features_ref as ref
from conftest import golden
from tsbb15_amd import _ffi, features, fun, lab3

ENTRIES = ("rs_harris", "rs_non_max_suppression", "rs_corners", "rs_match_rois_u8",
           "rs_match_rois_f64")


@pytest.fixture(scope="module")
def G():
    return golden("features.npz")


@pytest.mark.parametrize("name", ["rnd", "plat"])
@pytest.mark.parametrize("win", [1, 3, 5])
def test_nms_restatement_bitwise(G, name, win):
    want = G[f"nms_{name}_w{win}"]
    got = ref.non_max_suppression(G[f"nms_in_{name}"], win)
    assert got.dtype == want.dtype == np.float32
    assert got.tobytes() == want.tobytes()


def test_nms_plateau_keeps_equal_neighbours(G):
    assert (G["nms_plat_w3"][3:6, 4:8] == 9.0).all()


@pytest.mark.parametrize("cut", [ref.cut_out_rois, lambda *a: np.stack(features.cut_out_rois(*a)),
                                 lambda *a: np.stack(lab3.cut_out_rois(*a))])
def test_cut_out_rois_bitwise(G, cut):
    got = cut(G["roi_img"], G["roi_cols"], G["roi_rows"], 5)
    assert np.array_equal(got, G["roi_out"]) and got.dtype == np.uint8


def test_cut_out_rois_messages(G):
    names = [str(n) for n in G["roi_bad_names"]]
    assert len(names) == 8
    texts = set()
    for n in names:
        c, r, size = G[f"roi_bad_{n}_args"]
        msg = str(G[f"roi_bad_{n}_msg"])
        assert msg
        texts.add(msg)
        with pytest.raises(ValueError, match=re.escape(msg)):
            lab3.cut_out_rois(G["roi_img"], c, r, int(size[0]))
    assert len(texts) == 5


def test_matching_matrix_f64(G):
    want = G["mm_f64"]
    got = ref.matching_matrix_rois(G["mm_f64_r1"], G["mm_f64_r2"])
    tol = 2 * 7 * 7 * np.finfo(np.float64).eps
    assert np.all(np.abs(got - want) <= tol * np.abs(want))
    assert got[3, 2] == 0.0 == want[3, 2]


def test_matching_matrix_u8_wraps_bitwise(G):
    want = G["mm_u8"]
    got = ref.matching_matrix_rois(G["mm_u8_r1"], G["mm_u8_r2"], wrap=True)
    assert got.tobytes() == want.tobytes()
    true = ref.matching_matrix_rois(G["mm_u8_r1"], G["mm_u8_r2"], wrap=False)
    assert not np.array_equal(true, want) and true[4, 1] == 0.0 == want[4, 1]


@pytest.mark.parametrize("name", ["rnd", "tie", "mm"])
@pytest.mark.parametrize("jm", [ref.joint_min, features.joint_min, lab3.joint_min])
def test_joint_min_bitwise(G, name, jm):
    vals, ri, ci = jm(G[f"jm_{name}_in"])
    assert np.asarray(vals).tobytes() == G[f"jm_{name}_vals"].tobytes()
    assert np.array_equal(ri, G[f"jm_{name}_ri"]) and np.array_equal(ci, G[f"jm_{name}_ci"])


def test_joint_min_golden_has_ties(G):
    T = G["jm_tie_in"]
    assert ((T == T.min(axis=1, keepdims=True)).sum(axis=1) > 1).any()
    assert ((T == T.min(axis=0, keepdims=True)).sum(axis=0) > 1).any()


# d/dx and d/dy of the ramp I = gx x + gy y under the Sobel pair: gain * g
SOBEL_GAIN = {3: 8.0, 5: 128.0}


@pytest.mark.parametrize("bs,ks", [(3, 3), (2, 5)])
def test_harris_closed_forms(bs, ks):
    k = 0.04
    assert not ref.harris(np.full((20, 24), 77, np.uint8), bs, ks, raw=True).any()
    y, x = np.mgrid[0:30, 0:40]
    ramp = (3 * x + 2 * y).astype(np.uint8)
    assert ramp.max() == 3 * 39 + 2 * 29
    R = ref.harris64(ramp, bs, ks, k)[0]
    s = 1.0 / (2.0 ** (ks - 1) * bs * 255.0)
    g = SOBEL_GAIN[ks]
    want = -k * (bs * bs * ((g * 3) ** 2 + (g * 2) ** 2)) ** 2 * s ** 4
    halo = ks // 2 + bs
    inner = R[halo:-halo, halo:-halo]
    assert np.all(np.abs(inner - want) <= 1e-12 * abs(want))
    assert np.all(ref.harris(ramp, bs, ks)[halo:-halo, halo:-halo] == 0.0)
    assert np.abs(R - want).max() > 1e-3 * abs(want)     # the borders differ: reflection


def test_harris_tensor_bound():
    """The integer sums stay below 2^53 at the largest block and aperture."""
    img = np.zeros((80, 80), np.uint8)
    img[:, 40:] = 255
    sxx, _, _ = ref.harris_tensor(img, 31, 7)
    assert 0 < sxx.max() < 2 ** 53 and sxx.dtype == np.int64


def test_corners_order_and_empty():
    H = np.zeros((4, 5), np.float32)
    assert ref.corners(H).shape == (2, 0)
    H[3, 1], H[0, 4], H[0, 2], H[2, 0] = 5.0, 1.0, 2.0, 0.004
    assert np.array_equal(ref.corners(H), [[2, 4, 1], [0, 0, 3]])
    assert np.array_equal(ref.corners(H, 0.0), [[2, 4, 0, 1], [0, 0, 2, 3]])


def test_header_and_bindings_have_the_entries():
    src = open(_ffi.HEADER_PATH).read()
    for name in ENTRIES:
        assert re.search(r"^int %s\(" % name, src, flags=re.M), name
        assert name in _ffi._SIGS
    for const, val in (("RS_HARRIS_MAX_BLOCK", features.MAX_BLOCK_SIZE),
                       ("RS_MATCH_MAX_ROI", features.MAX_ROI_SIZE),
                       ("RS_MATCH_MAX_N", features.MAX_PATCHES)):
        assert re.search(r"#define %s %d\b" % (const, val), src), const


def test_drop_in_names_exist():
    for name in ("harris", "non_max_suppression", "cut_out_rois", "joint_min"):
        assert callable(getattr(lab3, name))
    assert callable(fun.matchingMatrix)


def test_argument_errors_need_no_gpu():
    u8 = np.zeros((20, 20), np.uint8)
    with pytest.raises(ValueError, match=re.escape("kernel_size must be 1, 3, 5, or 7")):
        features.harris(u8, 3, 2)
    with pytest.raises(ValueError, match=re.escape("Image type must be 8-bit unsigned (np.uint8)")):
        features.harris(u8.astype(np.float32), 3, 3)
    with pytest.raises(ValueError, match="convert"):
        features.harris(np.zeros((20, 20, 3), np.uint8), 3, 3)
    with pytest.raises(ValueError, match="window_size must be odd"):
        features.non_max_suppression(u8.astype(np.float32), 4)
    with pytest.raises(ValueError, match=re.escape("image must be single channel (i.e. a 2D array)")):
        features.non_max_suppression(np.zeros((4, 4, 3), np.float32), 3)
    f = np.full((20, 20), np.nan)
    with pytest.raises(ValueError, match="finite"):
        features.match(f, np.array([[5], [5]]), f, np.array([[5], [5]]), 3)


@pytest.mark.parametrize("h,w", [(96, 128), (200, 260)])
def test_pipeline_condition(h, w):
    """At least 0.9 of the joint-min matches of the restatement's chain carry the true shift
    (5, 3).  With the committed generator, seed 1: 42 of 44 (0.95) on the 96 x 128 pair and
    183 of 188 (0.97) on the 200 x 260 pair (a numpy prototype of the recipe that differed in
    the generator's details gave 43 of 43 and 182 of 195)."""
    img1, img2 = fx.image_pair(h, w, 1)
    c1, c2 = ref.putative_correspondences(img1, img2)
    good, total = fx.true_shift_share(c1, c2)
    print(f"{h} x {w}: {good} of {total}")
    assert total >= 20 and good >= 0.9 * total
