"""The image front end (csrc/features.hip) at its tile, chunk and scan edges, at ties and on
either side of the corner threshold, against the numpy restatement tests/features_ref.py --
never against the code under test.  The cases come from tests/features_edges_fixture.py;
tests/test_features_edges_cpu.py shows on the restatement alone that each has the property it is
named for.

Every comparison is exact, except Harris (the bound test_gpu_features.py::test_harris derives:
2^-23 |R| + 16 eps64 mag) and the fp64 matrix (the bound test_match_f64 derives: 2 roi^2 eps64
relative).  The branch each test aims at, and what it would see if that branch were wrong:

  * test_corners_at_scan_and_partial_edges   257 and more chunks: without the carry of
    k_corner_scan the chunks from 256 on write over the first ones; 1025 chunks with the only
    maximum in the last pixel: a reduction that misses the tail lets 300 decoys in
  * test_corner_threshold_boundary           a float32 product loses the pixel one ulp above
    float32(0.001 * 5.4891353); a comparison against the fp64 product narrowed to float32
    loses the pixel float32(0.001 * 3), which lies above the fp64 threshold
  * test_match_u8_tile_edges_and_ties        a `<=` among a thread's four columns, among the 16
    threads of a tile row, or in k_match_argmin each moves a planted argmin (5 for 4, 25 for 19
    and 9 for 3, 64 / 70 / 128 for 6); the same for columns
  * test_match_f64_chunks                    225 = 7 x 32 + 1 and 81 = 2 x 32 + 17 elements: a
    chunk loop that drops or repeats an element is off by far more than 450 eps
  * test_harris_*                            a halo one pixel short changes the border pixels of
    the noise image at the smallest legal size
  * test_corners_leave_nothing_behind        a 1025th partial maximum, or any partial beyond
    those written, is a stale 1e30

Measured on the MI355X (figures, none of them the source of a bound): every exact comparison
held.  Harris: the output equalled float32 of the restatement's fp64 response in all cases but
two (block 1, aperture 7, noise, 5 x 100 and 15 x 31: 0.74 and 0.55 of the bound).  fp64
matrix: at most 0.081 of the bound (roi 3), 0 at roi 1.  No kernel needed a change.
"""
import numpy as np
import pytest

import features_edges_fixture as fx
import features_ref as ref
from tsbb15_amd import _ffi, features

pytestmark = pytest.mark.gpu

EPS64 = np.finfo(np.float64).eps
C = _ffi.C


def _bytes_equal(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _same_list(got, want):
    return got.dtype == np.int64 and got.shape == want.shape and np.array_equal(got, want)


# ------------------------------------------------------------------------------------------
# 1. corner list
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", fx.CORNER_SHAPES)
def test_corners_at_scan_and_partial_edges(ctx, shape):
    H = fx.corner_case(shape)
    want = ref.corners(H, fx.CORNER_REL)
    got = features.corners(H, fx.CORNER_REL, ctx=ctx)
    assert got.dtype == np.int64 and got.shape == want.shape and got.shape[0] == 2
    assert np.array_equal(got, want)
    assert got[0, -1] == shape[1] - 1 and got[1, -1] == shape[0] - 1
    assert np.array_equal(fx.chunk_counts(got, shape), fx.chunk_counts(want, shape))


@pytest.mark.parametrize("name", list(fx.BOUNDARY))
def test_corner_threshold_boundary(ctx, name):
    H, rel, px = fx.boundary_case(name)
    want = fx.hits(fx.header_rule(H, rel))
    # the maximum and the pixel above float32(thr); float32(thr) itself where it lies above thr
    expect = [fx.BOUNDARY_AT[0], fx.BOUNDARY_AT[3]] + ([fx.BOUNDARY_AT[2]] * (name == "rounds up"))
    got = features.corners(H, rel, ctx=ctx)
    assert _same_list(got, want) and np.array_equal(got, ref.corners(H, rel))
    assert got.T.tolist() == [[x, y] for y, x in sorted(expect)]


@pytest.mark.parametrize("rel", fx.SIGN_RELS)
@pytest.mark.parametrize("kind", list(fx.sign_images()))
def test_corner_threshold_signs(ctx, kind, rel):
    H = fx.sign_images()[kind]
    assert _same_list(features.corners(H, rel, ctx=ctx), ref.corners(H, rel))


def test_corners_leave_nothing_behind(ctx):
    """The context's scratch is grow-only and laid out from its start, so a call finds the
    previous call's image, partial maxima and counts where its own buffers lie.  A 1025 x 2048
    image of 1e30 first (rel = 1: no hit), then the 1025-chunk cases, then a small image: every
    list is the restatement's, so nothing stale was read -- a 1025th partial maximum least of
    all, which would be one of those 1e30."""
    dirty = np.full((1025, 2048), 1e30, np.float32)
    assert features.corners(dirty, 1.0, ctx=ctx).shape == (2, 0)
    for shape in ((1025, 2047), (1025, 2048)):
        big = fx.corner_case(shape)
        assert _same_list(features.corners(big, fx.CORNER_REL, ctx=ctx),
                          ref.corners(big, fx.CORNER_REL))
    small = fx.one_hot()
    got = features.corners(small, ctx=ctx)
    assert _same_list(got, ref.corners(small)) and got.tolist() == [[31], [20]]
    H, rel, _ = fx.boundary_case("not representable")
    assert _same_list(features.corners(H, rel, ctx=ctx), ref.corners(H, rel))


# ------------------------------------------------------------------------------------------
# 2. matching
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("roi", fx.MATCH_ROIS)
@pytest.mark.parametrize("n1,n2", fx.MATCH_SIZES)
def test_match_u8_tile_edges_and_ties(ctx, n1, n2, roi):
    img = fx.u8_image()
    xy1, xy2 = fx.match_case(n1, n2, roi)
    for wrap in (False, True):
        want = ref.matching_matrix(img, xy1, img, xy2, roi, wrap)
        M = features.matching_matrix(img, xy1, img, xy2, roi, wrap=wrap, ctx=ctx)
        assert _bytes_equal(M, want)
        r, c = features.match_argmins(img, xy1, img, xy2, roi, wrap=wrap, ctx=ctx)
        assert r.shape == (n1,) and c.shape == (n2,) and r.dtype == c.dtype == np.int64
        assert np.array_equal(r, want.argmin(axis=1)) and np.array_equal(c, want.argmin(axis=0))
        # the planted classes by name: the smallest index of each set
        for k, holder in enumerate(fx.HOLDERS):
            if n1 >= fx.MIN_TIED and fx.tie_sets(n2)[k]:
                assert r[holder] == fx.tie_sets(n2)[k][0]
            if n2 >= fx.MIN_TIED and fx.tie_sets(n1)[k]:
                assert c[holder] == fx.tie_sets(n1)[k][0]
    for got, exp in zip(features.match(img, xy1, img, xy2, roi, ctx=ctx),
                        ref.joint_min(ref.matching_matrix(img, xy1, img, xy2, roi))):
        assert _bytes_equal(np.asarray(got), np.asarray(exp))


@pytest.mark.parametrize("wrap", [False, True])
def test_match_u8_largest_distances(ctx, wrap):
    """Squared distances up to 225 * 65025: the uint32 sum and the correctly rounded root."""
    a, b = fx.binary_pair()
    xy1, xy2 = fx.binary_centres()
    want = ref.matching_matrix(a, xy1, b, xy2, 15, wrap)
    assert _bytes_equal(features.matching_matrix(a, xy1, b, xy2, 15, wrap=wrap, ctx=ctx), want)
    r, c = features.match_argmins(a, xy1, b, xy2, 15, wrap=wrap, ctx=ctx)
    assert np.array_equal(r, want.argmin(axis=1)) and np.array_equal(c, want.argmin(axis=0))
    if not wrap:
        assert want.max() == np.sqrt(225.0 * 65025.0)


@pytest.mark.parametrize("many_first", [False, True])
def test_match_512_partials(ctx, many_first):
    """RS_MATCH_MAX_N patches against one: 512 partial minima per row (column), no matrix."""
    img = fx.u8_image()
    one, many = fx.many_case()
    want = ref.matching_matrix(img, one, img, many, 3)
    if many_first:
        c, r = features.match_argmins(img, many, img, one, 3, ctx=ctx)
    else:
        r, c = features.match_argmins(img, one, img, many, 3, ctx=ctx)
    assert r.shape == (1,) and c.shape == (fx.MANY,)
    assert r[0] == want[0].argmin() and not c.any()


@pytest.mark.parametrize("n1,n2", fx.F64_SIZES)
@pytest.mark.parametrize("roi", fx.F64_ROIS)
def test_match_f64_chunks(ctx, roi, n1, n2):
    img1, img2 = fx.f64_pair()
    xy1, xy2 = fx.f64_case(n1, n2, roi)
    want = ref.matching_matrix(img1, xy1, img2, xy2, roi)
    vals, ri, ci, M = features.match(img1, xy1, img2, xy2, roi, return_matrix=True, ctx=ctx)
    assert M.dtype == np.float64 and M.shape == (n1, n2)
    tol = 2 * roi * roi * EPS64
    err = np.abs(M - want)
    print(f"roi {roi} ({n1}, {n2}): max err / tol = "
          f"{(err / np.maximum(tol * np.abs(want), 1e-300)).max():.3g}")
    assert np.all(err <= tol * np.abs(want))
    assert (want == 0.0).sum() >= 2 and np.all(M[want == 0.0] == 0.0)
    assert np.array_equal(M == 0.0, want == 0.0)
    r, c = features.match_argmins(img1, xy1, img2, xy2, roi, ctx=ctx)
    assert np.array_equal(r, M.argmin(axis=1)) and np.array_equal(c, M.argmin(axis=0))
    for got, exp in zip((vals, ri, ci), ref.joint_min(M)):
        assert _bytes_equal(np.asarray(got), np.asarray(exp))
    assert _bytes_equal(features.matching_matrix(img1, xy1, img2, xy2, roi, ctx=ctx), M)


# ------------------------------------------------------------------------------------------
# 3. Harris
# ------------------------------------------------------------------------------------------
def _harris_ratio(ctx, img, bs, ks, k=0.04):
    """Largest err / tol over both ``raw`` settings, after asserting the bound of test_harris."""
    R, mag = ref.harris64(img, bs, ks, k)
    tol = 2.0 ** -23 * np.abs(R) + 16 * EPS64 * mag
    worst = 0.0
    for raw in (False, True):
        got = features.harris(img, bs, ks, k=k, raw=raw, ctx=ctx)
        assert got.dtype == np.float32 and got.shape == img.shape
        want = R.astype(np.float32).astype(np.float64)
        if not raw:
            want = np.maximum(want, 0.0)
            assert got.min() >= 0.0
        err = np.abs(got.astype(np.float64) - want)
        assert np.all(err <= tol), (img.shape, raw, float((err - tol).max()))
        if tol.any():
            worst = max(worst, float((err / np.maximum(tol, 1e-300)).max()))
        if raw and not R.any():
            assert not got.any()
    return worst


@pytest.mark.parametrize("kind", fx.HARRIS_KINDS)
@pytest.mark.parametrize("bs,ks", fx.HARRIS_PAIRS)
def test_harris_smallest_shapes_and_tile_edges(ctx, bs, ks, kind):
    for shape in fx.harris_shapes(bs, ks):
        ratio = _harris_ratio(ctx, fx.harris_image(kind, shape), bs, ks)
        print(f"block {bs} aperture {ks} {kind} {shape}: max err / tol = {ratio:.3g}")


@pytest.mark.parametrize("kind", ["texture", "noise"])
@pytest.mark.parametrize("k", fx.HARRIS_KS)
def test_harris_k(ctx, k, kind):
    bs, ks, shape = fx.HARRIS_K_CASE
    ratio = _harris_ratio(ctx, fx.harris_image(kind, shape), bs, ks, k)
    print(f"k = {k} {kind}: max err / tol = {ratio:.3g}")


# ------------------------------------------------------------------------------------------
# 4. NMS
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", fx.NMS_SHAPES)
def test_nms_windows_and_sides(ctx, shape):
    img = fx.nms_image(shape)
    for win in fx.nms_windows(shape):
        got = features.non_max_suppression(img, win, ctx=ctx)
        assert _bytes_equal(got, ref.non_max_suppression(img, win)), win


# ------------------------------------------------------------------------------------------
# 5. the entry points' own error lists
# ------------------------------------------------------------------------------------------
def test_errors_from_the_library(ctx):
    """The C entry points' own RS_EINVAL lists, reached past the shim's checks."""
    L, OK, EINVAL = _ffi.lib(), _ffi.RS_OK, _ffi.RS_EINVAL
    u8 = np.ascontiguousarray(fx.u8_image())                       # 60 x 80
    f32 = np.zeros((60, 80), np.float32)
    out = np.zeros((60, 80), np.float32)

    def harris(h=60, w=80, bs=3, ks=3, k=0.04):
        return L.rs_harris(ctx.handle, _ffi.ptr(u8, C.c_uint8), h, w, bs, ks, k, 0,
                           _ffi.ptr(out, C.c_float))

    assert harris() == OK
    assert fx.harris_halo(3, 3) == 4
    for kw in (dict(h=4), dict(w=4), dict(h=4, w=4), dict(bs=0), dict(bs=32),
               dict(k=float("nan")), dict(k=float("inf")), dict(ks=2), dict(h=0)):
        assert harris(**kw) == EINVAL, kw
    for kw in (dict(h=5), dict(w=5), dict(h=5, w=5), dict(bs=31, ks=7, h=35, w=35), dict(bs=1)):
        assert harris(**kw) == OK, kw
    assert harris(bs=31, ks=7, h=34, w=35) == EINVAL

    def nms(window):
        return L.rs_non_max_suppression(ctx.handle, _ffi.ptr(f32, C.c_float), 60, 80, window,
                                        _ffi.ptr(out, C.c_float))

    assert nms(3) == OK
    for window in (0, 2, 8, -1):
        assert nms(window) == EINVAL, window

    H = np.zeros((37, 53), np.float32)
    H[[0, 5, 9, 20, 36], [0, 7, 52, 31, 52]] = 4.0
    xy = np.full((2, 5), -7, np.int32)
    n = C.c_int64(-1)

    def corners(cap, rel=0.001):
        n.value = -1
        return L.rs_corners(ctx.handle, _ffi.ptr(H, C.c_float), 37, 53, rel,
                            _ffi.ptr(xy, C.c_int32), cap, C.byref(n))

    assert corners(4) == EINVAL and n.value == 5        # *count is the true count
    assert np.all(xy == -7)                             # and nothing was written
    assert corners(0) == EINVAL and n.value == 5
    assert corners(5) == OK and n.value == 5
    assert np.array_equal(xy, ref.corners(H))
    for rel in (float("nan"), float("inf"), float("-inf")):
        assert corners(5, rel) == EINVAL, rel

    # matching: both entries.  The arrays are as long as the largest n named, so that a missing
    # check would read initialised memory.
    big = 32769
    centre = np.ascontiguousarray(np.tile(np.array([[10], [10]], np.int32), (1, big)))
    f64 = np.ascontiguousarray(u8, dtype=np.float64)
    rmin, cmin = np.zeros(big, np.int32), np.zeros(big, np.int32)
    rval = np.zeros(big)
    dummy = np.full(16, -7.0)

    def pair(n_, x=10, y=10):
        a = centre[:, :n_].copy() if n_ else centre[:, :1].copy()
        a[0, 0], a[1, 0] = x, y
        return a

    def match(kind, n1=1, n2=1, roi=7, M=False, xy1=None, xy2=None):
        a = pair(n1) if xy1 is None else xy1
        b = pair(n2) if xy2 is None else xy2
        outs = (_ffi.ptr(rmin, C.c_int32), _ffi.ptr(cmin, C.c_int32), _ffi.ptr(rval, C.c_double),
                _ffi.ptr(dummy, C.c_double) if M else None)
        if kind == "u8":
            return L.rs_match_rois_u8(ctx.handle, _ffi.ptr(u8, C.c_uint8), 60, 80,
                                      _ffi.ptr(a, C.c_int32), n1, _ffi.ptr(u8, C.c_uint8), 60, 80,
                                      _ffi.ptr(b, C.c_int32), n2, roi, 0, *outs)
        return L.rs_match_rois_f64(ctx.handle, _ffi.ptr(f64, C.c_double), 60, 80,
                                   _ffi.ptr(a, C.c_int32), n1, _ffi.ptr(f64, C.c_double), 60, 80,
                                   _ffi.ptr(b, C.c_int32), n2, roi, *outs)

    for kind in ("u8", "f64"):
        assert match(kind) == OK
        assert match(kind, n1=2, n2=3, M=True) == OK and np.all(dummy[:6] == 0.0)
        dummy[:] = -7.0
        for kw in (dict(n1=0), dict(n2=0), dict(n1=big), dict(n2=big), dict(roi=17), dict(roi=6),
                   dict(roi=0), dict(n1=16385, n2=16385, M=True)):
            assert match(kind, **kw) == EINVAL, (kind, kw)
        assert np.all(dummy == -7.0)                  # refused before anything was written
        # roi 7: a centre 2 from a border is refused on either side, 3 from it is accepted
        for x, y in ((2, 10), (77, 10), (10, 2), (10, 57)):
            assert match(kind, xy1=pair(1, x, y)) == EINVAL, (kind, x, y)
            assert match(kind, xy2=pair(1, x, y)) == EINVAL, (kind, x, y)
            assert match(kind, n2=3, xy2=pair(3, x, y)[:, ::-1].copy()) == EINVAL   # the last one
        for x, y in ((3, 3), (76, 3), (3, 56), (76, 56)):
            assert match(kind, xy1=pair(1, x, y), xy2=pair(1, x, y)) == OK, (kind, x, y)
