"""tests/features_edges_fixture.py without a GPU: every case has the property it is named for,
shown on the numpy restatement (tests/features_ref.py) alone, so that
tests/test_gpu_features_edges.py may simply demand the restatement's output:

  * corner list: the chunk counts 256, 257, 1024, 1025, 1025; the only maximum at pixel n - 1; a
    full chunk, an empty chunk between two with hits, hits at the first and last pixel of chunks
    255, 256, 1023 and 1024; the threshold rule of the header on either side of the threshold,
    and where numpy's own evaluation of the recipe's line leaves it;
  * matching: each tie class is in the restatement's matrix and resolves to the smallest index;
    the binary pair reaches 225 * 65025; the 32768-wide case has zeros in several tiles;
    the fp64 element counts leave the partial chunks claimed;
  * Harris: the step image reaches |Ix| = 163200, the noise tensor needs 41 bits, the responses
    have the stated signs, every shape is legal and the smallest is one pixel above the halo;
  * NMS: the kept pixel on the single legal row, the plateaus at the legal region's edge.
"""
import numpy as np
import pytest

import features_edges_fixture as fx
import features_fixture as base
import features_ref as ref

EPS64 = np.finfo(np.float64).eps


# ------------------------------------------------------------------------------------------
# 1. corner list
# ------------------------------------------------------------------------------------------
def test_chunk_counts_cross_the_scan_round_and_the_partial_cap():
    assert tuple(fx.corner_chunks(s) for s in fx.CORNER_SHAPES) == fx.CORNER_CHUNKS
    assert fx.CORNER_CHUNKS == (fx.SCAN_ROUND, fx.SCAN_ROUND + 1, fx.MAX_PARTIALS,
                                fx.MAX_PARTIALS + 1, fx.MAX_PARTIALS + 1)
    h, w = fx.CORNER_SHAPES[-1]
    assert h * w % fx.CHUNK != 0 and w & (w - 1) != 0       # a partial last chunk, w no power of 2


@pytest.mark.parametrize("shape", fx.CORNER_SHAPES)
def test_corner_case_has_its_structures(shape):
    H = fx.corner_case(shape)
    h, w = shape
    n, nb = h * w, fx.corner_chunks(shape)
    assert H.dtype == np.float32 and H.shape == shape
    flat = H.reshape(-1)
    assert flat[n - 1] == fx.CORNER_MAX and np.count_nonzero(flat == flat.max()) == 1
    xy = ref.corners(H, fx.CORNER_REL)
    assert xy.dtype == np.int64 and xy.shape[0] == 2
    at = xy[1] * w + xy[0]
    assert np.all(np.diff(at) > 0)                          # row-major scan order
    assert np.array_equal(at, np.flatnonzero(flat >= fx.CORNER_HIT))
    assert at[-1] == n - 1
    counts = fx.chunk_counts(xy, shape)
    assert len(counts) == nb and counts.sum() == xy.shape[1]
    assert counts[fx.FULL_CHUNK] == fx.CHUNK
    assert counts[fx.EMPTY_CHUNK] == 0 and counts[fx.EMPTY_CHUNK - 1] == 3 \
        and counts[fx.EMPTY_CHUNK + 1] == 5
    for c in fx.EDGE_CHUNKS:
        if c < nb:
            first, last = fx.chunk_span(c, n)
            assert first in at and last in at and counts[c] == 2, c
    assert sum(c < nb for c in fx.EDGE_CHUNKS) == (1, 2, 3, 4, 4)[fx.CORNER_SHAPES.index(shape)]
    # hits on both sides of every round of the scan, so that a lost carry moves them
    for lo in range(0, nb, fx.SCAN_ROUND):
        assert counts[lo:lo + fx.SCAN_ROUND].sum() > 0
    # the list depends on the maximum at n - 1: without it the decoys are hits
    rest = flat.copy()
    rest[n - 1] = 0.0
    assert rest.max() == fx.CORNER_HIT
    assert ref.corners(rest.reshape(shape), fx.CORNER_REL).shape[1] > xy.shape[1] + 300
    assert (flat < 0).sum() >= 290


@pytest.mark.parametrize("name", list(fx.BOUNDARY))
def test_threshold_boundary_and_the_two_rules(name):
    H, rel, px = fx.boundary_case(name)
    mx = fx.BOUNDARY[name][0]
    thr = rel * float(mx)
    assert H.max() == mx and px[0] < px[1] < px[2]
    assert np.float32(thr) == px[1]
    want = fx.header_rule(H, rel)
    at = lambda mask: [bool(mask[p]) for p in fx.BOUNDARY_AT]     # maximum, below, at, above
    assert at(want) == [True] + [float(p) > thr for p in px]
    assert np.array_equal(ref.corners(H, rel), fx.hits(want))
    f32, narrowed = fx.float32_rule(H, rel), fx.narrowed_rule(H, rel)
    # the installed numpy forms the product in float32 (numpy >= 2): its rule is float32_rule
    assert np.asarray(rel * np.max(H)).dtype == np.float32
    assert np.array_equal(fx.numpy_rule(H, rel), f32)
    if name == "representable":
        assert float(px[1]) == thr == 512.0
        assert at(want) == at(f32) == at(narrowed) == [True, False, False, True]
    elif name == "not representable":
        # the documented divergence: float32(thr) lies below the threshold, so narrowing changes
        # nothing, but the float32 product rounds up onto the pixel above, which then is no hit
        assert float(px[1]) < thr < float(px[2])
        assert mx == np.float32(5.4891353) and px[2] == np.float32(0.0054891356)
        assert at(want) == at(narrowed) == [True, False, False, True]
        assert np.float32(rel) * mx == px[2] and at(f32) == [True, False, False, False]
        assert not np.array_equal(fx.numpy_rule(H, rel), want)
    else:
        # float32(thr) lies above the threshold: that pixel is a hit, and a comparison against
        # the narrowed threshold (here also the float32 product) loses it
        assert float(px[0]) < thr < float(px[1])
        assert at(want) == [True, False, True, True]
        assert at(narrowed) == [True, False, False, True]
        assert np.float32(rel) * mx == px[1] and at(f32) == at(narrowed)


def test_each_float32_rule_differs_from_the_header_somewhere():
    cases = [fx.boundary_case(name)[:2] for name in fx.BOUNDARY]
    for rule in (fx.float32_rule, fx.narrowed_rule):
        assert any(not np.array_equal(rule(H, rel), fx.header_rule(H, rel)) for H, rel in cases)
    # and they are two rules: they part on the case where the product is formed in float32
    H, rel, _ = fx.boundary_case("not representable")
    assert not np.array_equal(fx.float32_rule(H, rel), fx.narrowed_rule(H, rel))


def test_sign_cases():
    imgs = fx.sign_images()
    assert imgs["mixed"].max() > 0 > imgs["mixed"].min() and (imgs["mixed"] == 0).any()
    assert imgs["zeros and negatives"].max() == 0 > imgs["zeros and negatives"].min()
    assert imgs["negatives"].max() < 0
    n = {(k, rel): ref.corners(H, rel).shape[1] for k, H in imgs.items() for rel in fx.SIGN_RELS}
    size = 37 * 53
    assert n["mixed", 1.0] == 0 and 0 < n["mixed", 0.0] < n["mixed", -0.5] < size
    assert n["mixed", 0.0] == (imgs["mixed"] > 0).sum()
    assert all(n["zeros and negatives", rel] == 0 for rel in fx.SIGN_RELS)
    assert all(n["negatives", rel] == 0 for rel in (0.0, 1.0, -0.5))
    assert 0 < n["negatives", 2.0] < size            # a maximum below zero: rel > 1 lowers the bar


def test_the_two_rules_agree_on_the_chain_fixtures():
    """The committed chain fixtures are far from the divergence: after NMS every positive value
    is more than 30 times the threshold."""
    counts = []
    for shape in ((96, 128), (200, 260)):
        for img in base.image_pair(*shape, 1):
            N = ref.non_max_suppression(ref.harris(img, 7, 3), 9)
            a, b, c = fx.header_rule(N, 0.001), fx.numpy_rule(N, 0.001), fx.float32_rule(N, 0.001)
            assert np.array_equal(a, b) and np.array_equal(a, c)
            assert np.array_equal(a, fx.narrowed_rule(N, 0.001))
            pos = N[N > 0].astype(np.float64)
            assert pos.min() > 30 * 0.001 * float(N.max())
            counts.append(int(a.sum()))
    assert counts == [51, 53, 223, 222]


def test_one_hot():
    assert np.array_equal(ref.corners(fx.one_hot()), [[31], [20]])


# ------------------------------------------------------------------------------------------
# 2. matching
# ------------------------------------------------------------------------------------------
def test_tie_sets_are_the_classes():
    for n in (63, 64, 65, 128, 129, 130):
        across, thread, tile, across_only = fx.tie_sets(n)
        assert across[:2] == [3, 9] and 3 // 4 != 9 // 4 and 3 // fx.TILE == 9 // fx.TILE
        assert thread == [4, 5] and 4 // 4 == 5 // 4
        assert tile == [19, 25] and 19 // 4 != 25 // 4 and 19 // fx.TILE == 25 // fx.TILE
        tiles = [i // fx.TILE for i in across_only]
        assert len(set(tiles)) == len(tiles) == {63: 1, 64: 1, 65: 2, 128: 2, 129: 2, 130: 3}[n]
        assert len({i // fx.TILE for i in across}) == (1 if n < 68 else (n - 1) // fx.TILE + 1)
        flat = across + thread + tile + across_only
        assert len(set(flat)) == len(flat) and max(flat) < n
        assert not set(flat) & (set(fx.HOLDERS) | set(fx.EXTREME_AT))
    assert fx.tie_sets(130)[0] == [3, 9, 67, 129] and fx.tie_sets(129)[0] == [3, 9, 67, 128]
    assert fx.tie_sets(65)[3] == [6, 64] and fx.tie_sets(130)[3] == [6, 70, 128]
    assert fx.tie_sets(1) == [[], [], [], []]


@pytest.mark.parametrize("roi", fx.MATCH_ROIS)
@pytest.mark.parametrize("n1,n2", fx.MATCH_SIZES)
def test_match_case_has_its_ties(n1, n2, roi):
    img = fx.u8_image()
    xy1, xy2 = fx.match_case(n1, n2, roi)
    assert xy1.shape == (2, n1) and xy2.shape == (2, n2)
    h, w = fx.MATCH_IMAGE
    m = roi // 2
    for xy in (xy1, xy2):
        assert xy[0].min() >= m and xy[0].max() <= w - m - 1
        assert xy[1].min() >= m and xy[1].max() <= h - m - 1
        k = [i for i in fx.EXTREME_AT if i < xy.shape[1]]
        assert np.array_equal(xy[:, k], fx.extremes(roi)[:, :len(k)])
    for wrap in (False, True):
        M = ref.matching_matrix(img, xy1, img, xy2, roi, wrap)
        assert M.shape == (n1, n2)
        for A, n_other in ((M, n2), (M.T, n1)):
            if A.shape[0] < fx.MIN_TIED:
                continue
            for holder, want in zip(fx.HOLDERS, fx.tie_sets(n_other)):
                assert list(np.flatnonzero(A[holder] == 0.0)) == want, (holder, want)
                if want:
                    assert A[holder].argmin() == want[0] == min(want)
    if n1 == n2 == 1:
        assert np.array_equal(xy1, fx.extremes(roi)[:, :1])


def test_sizes_sit_on_the_tile_edges():
    sides = {n for s in fx.MATCH_SIZES for n in s}
    assert {1, 63, 64, 65, 128, 129} <= sides
    assert fx.MATCH_SIZES[:6] == ((63, 65), (64, 64), (65, 63), (64, 129), (129, 128), (1, 1))


def test_binary_pair_reaches_the_largest_distance():
    a, b = fx.binary_pair()
    assert set(np.unique(a)) == {0, 255} and np.array_equal(a.astype(int) + b, np.full(a.shape, 255))
    xy1, xy2 = fx.binary_centres()
    M = ref.matching_matrix(a, xy1, b, xy2, 15)
    d2 = np.rint(M * M).astype(np.int64)
    assert d2.max() == 225 * 65025 and d2[5, 0] == d2[64, 64] == d2[0, 128] == 225 * 65025
    assert 225 * 65025 < 2 ** 31                       # the uint32 sum holds it
    assert len(np.unique(d2)) > 50
    # with wrap a difference of -255 counts as 1
    W = ref.matching_matrix(a, xy1, b, xy2, 15, True)
    assert not np.array_equal(W, M) and W.max() ** 2 < 225 * 65025


def test_many_case_has_zeros_in_several_tiles():
    img = fx.u8_image()
    one, many = fx.many_case()
    assert one.shape == (2, 1) and many.shape == (2, fx.MANY) and fx.MANY // fx.TILE == 512
    M = ref.matching_matrix(img, one, img, many, 3)
    zeros = np.flatnonzero(M[0] == 0.0)
    tiles = np.unique(zeros // fx.TILE)
    print(f"{len(zeros)} zeros in tiles {list(tiles)}")
    assert len(tiles) >= 5 and 20000 in zeros and zeros[0] < 20000
    assert M[0].argmin() == zeros[0] and zeros[0] // fx.TILE > 0 and tiles[-1] > 256


@pytest.mark.parametrize("roi", fx.F64_ROIS)
def test_f64_cases(roi):
    ne = roi * roi
    assert (ne // fx.F64_CHUNK, ne % fx.F64_CHUNK) == {1: (0, 1), 3: (0, 9), 9: (2, 17),
                                                       15: (7, 1)}[roi]
    img1, img2 = fx.f64_pair()
    assert np.array_equal(img1[:30], img2[:30]) and not (img1[30:] == img2[30:]).any()
    for n1, n2 in fx.F64_SIZES:
        xy1, xy2 = fx.f64_case(n1, n2, roi)
        assert xy1.shape == (2, n1) and xy2.shape == (2, n2)
        M = ref.matching_matrix(img1, xy1, img2, xy2, roi)
        zeros = np.argwhere(M == 0.0)
        if n1 >= 8:
            assert {(5, 6), (6, 70), (7, 128)} <= {tuple(z) for z in zeros}
        else:
            assert [tuple(z) for z in zeros] == [(0, 2), (0, 4)]
        assert (M > 0).mean() > 0.5            # zeros are the exception (roi 1: equal pixels meet)


# ------------------------------------------------------------------------------------------
# 3. Harris
# ------------------------------------------------------------------------------------------
def test_harris_shapes_are_legal_and_minimal():
    assert len(fx.HARRIS_PAIRS) == 9 and max(bs for bs, _ in fx.HARRIS_PAIRS) == 31
    for bs, ks in fx.HARRIS_PAIRS:
        R = fx.harris_halo(bs, ks)
        shapes = fx.harris_shapes(bs, ks)
        assert shapes[:3] == [(R + 1, R + 1), (R + 1, 100), (100, R + 1)]
        assert all(min(s) > R for s in shapes)
        if (bs, ks) in fx.HARRIS_TILE_PAIRS:
            assert shapes[3:] == list(fx.HARRIS_TILE_SHAPES)
    assert fx.harris_halo(31, 7) == 34 and fx.harris_halo(1, 1) == 2


def test_harris64_magnitude_uses_abs_k():
    img = fx.harris_image("noise", (37, 53))
    R, mag = ref.harris64(img, 4, 5, -0.1)
    Rp, magp = ref.harris64(img, 4, 5, 0.1)
    assert np.array_equal(mag, magp) and np.all(mag >= np.abs(R)) and np.all(mag > 0)
    assert np.all(R >= Rp) and (R > Rp).any()
    assert np.array_equal(ref.harris64(img, 4, 5)[1], ref.harris64(img, 4, 5, 0.04)[1])


def test_step_reaches_the_largest_derivative():
    for shape in fx.harris_shapes(31, 7) + fx.harris_shapes(1, 7):
        ix, iy = ref.sobel(fx.harris_image("step", shape), 7)
        assert np.abs(ix).max() == 255 * 640 == 163200 and not iy.any()


@pytest.mark.parametrize("bs,ks", fx.HARRIS_PAIRS)
def test_harris_signs(bs, ks):
    for shape in fx.harris_shapes(bs, ks):
        R = ref.harris64(fx.harris_image("step", shape), bs, ks)[0]
        assert (R <= 0).all() and (R < 0).any(), shape       # Iy = 0: R = -k a^2
        w = shape[1]
        assert (R[:, w // 2 - 1:w // 2 + 1] < 0).any(axis=1).all()     # along the edge
        assert not ref.harris64(fx.harris_image("constant", shape), bs, ks)[0].any()
        R = ref.harris64(fx.harris_image("texture", shape), bs, ks)[0]
        assert np.isfinite(R).all() and R.any()


def test_noise_tensor_needs_41_bits():
    img = fx.harris_image("noise", (35, 100))
    assert (35, 100) in fx.harris_shapes(31, 7)
    sxx, sxy, syy = ref.harris_tensor(img, 31, 7)
    assert 2 ** 40 <= max(sxx.max(), syy.max()) < 2 ** 41
    assert (ref.harris64(img, 31, 7)[0] > 0).all()


# ------------------------------------------------------------------------------------------
# 4. NMS
# ------------------------------------------------------------------------------------------
def test_nms_windows():
    assert fx.nms_windows((1, 1)) == [1, 3, 7, 31, 2147483647]
    assert fx.nms_windows((9, 33)) == [1, 3, 7, 9, 17, 31, 67, 2147483647]
    assert fx.nms_windows((41, 67)) == [1, 3, 7, 31, 41, 81, 135, 2147483647]
    for shape in fx.NMS_SHAPES:
        wins = fx.nms_windows(shape)
        assert all(x % 2 == 1 for x in wins)
        assert {1, 3, 7, 31, 2 * min(shape) - 1, 2 * max(shape) + 1, 2147483647} <= set(wins)


@pytest.mark.parametrize("shape", fx.NMS_SHAPES)
def test_nms_cases(shape):
    img = fx.nms_image(shape)
    h, w = shape
    assert img.dtype == np.float32 and np.isfinite(img).all()
    assert img[h // 2, w // 2] == fx.F32_MAX == img.max()
    if h * w >= 3:
        assert (img < 0).any() and np.signbit(img[img == 0]).any()
    for win in fx.nms_windows(shape):
        out = ref.non_max_suppression(img, win)
        m = (win - 1) // 2
        legal = h > 2 * m and w > 2 * m
        assert out.dtype == np.float32 and out.shape == shape
        if not legal:
            assert not out.any()
            assert np.array_equal(np.signbit(out), np.signbit(img))      # 0 * v keeps the sign
        else:
            assert out[h // 2, w // 2] == fx.F32_MAX
        if win == 1:
            assert out.tobytes() == img.tobytes()
        if win == min(shape) and win > 1 and max(shape) > 2 * m:
            # one row (column) of legal centres, and the kept pixel lies on it
            kept = np.argwhere(out != 0)
            assert len(kept) >= 1 and [h // 2, w // 2] in kept.tolist()
            assert set(kept[:, 0 if h < w else 1]) == {m}
    if h >= 8:
        out = ref.non_max_suppression(img, 3)
        assert (out[fx.PLATEAUS[3]] == fx.PLATEAU).all()
    if shape == (41, 67):
        for win, block in fx.PLATEAUS.items():
            out = ref.non_max_suppression(img, win)
            m = (win - 1) // 2
            assert block[0].start == m or block[1].start == m
            assert (out[block] == fx.PLATEAU).all() and (img[block] == fx.PLATEAU).all()
