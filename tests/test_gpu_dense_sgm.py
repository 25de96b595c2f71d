"""The semi-global aggregation on the GPU (tsbb15_amd.dense.aggregate, plane_sweep_sgm,
csrc/dense_sgm.hip) against the numpy restatement tests/dense_sgm_ref.py.

Every operation of the definition is a single rounded fp32 add, subtract or min, stated in one
order, so there is no bar here: index, delta, score and S must equal the restatement's as
numbers, NaN for NaN.  The plane sweep under plane_sweep_sgm is compared bit for bit with
dense.plane_sweep, and the aggregation with the restatement applied to that GPU volume.
"""
import numpy as np
import pytest

import dense_fixture as df
import dense_sgm_ref as sr
from dense_sgm_fixture import noisy_slanted, random_volume
from tsbb15_amd import _ffi, dense

pytestmark = pytest.mark.gpu

# D = 1; D below, at and above 32 (lines packed into a wave) and 64 (one register per lane);
# D = 128, 255, 256 (two and four registers per lane, the last lanes dead at 255); images of one
# row, one column and one pixel; 40 x 56 gives several blocks of lines at D = 12.  The last three
# have lines longer than the kernel's ring of prefetched steps (16 steps, 8 past D = 128) at two,
# three and four registers per lane, so its unrolled main loop runs there and not only its tail.
SHAPES = [(1, 5, 7), (2, 9, 4), (5, 1, 9), (5, 9, 1), (3, 1, 1), (12, 40, 56), (31, 9, 33),
          (32, 9, 33), (33, 9, 33), (63, 7, 9), (64, 9, 7), (65, 6, 11), (128, 5, 6), (255, 3, 5),
          (256, 5, 3), (128, 18, 21), (160, 9, 10), (256, 9, 11)]
NAMES = ("index", "delta", "score", "S")


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a


def _same_bits(got, want):
    return len(got) == len(want) and all(
        x.shape == y.shape and x.dtype == y.dtype and np.array_equal(_bits(x), _bits(y))
        for x, y in zip(got, want))


def _equal(got, want, what):
    assert len(got) == len(want) == 4
    assert got[0].dtype == np.int32
    for g, w, name in zip(got, want, NAMES):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name)
        assert np.array_equal(g, w, equal_nan=True), (what, name)


def _seed(shape):
    return 1000 + 7 * shape[0] + 3 * shape[1] + shape[2]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_aggregate_equals_restatement(shape, ctx):
    v = random_volume(shape, _seed(shape))
    got = dense.aggregate(v, 0.1, 1.0, 8, return_aggregated=True, ctx=ctx)
    _equal(got, sr.solve(v, 0.1, 1.0, 8), shape)
    assert np.array_equal(got[0] == -1, np.isnan(v).all(axis=0)) and (got[0] == -1).any()
    three = dense.aggregate(v, 0.1, 1.0, 8, ctx=ctx)
    assert len(three) == 3 and _same_bits(three, got[:3])


@pytest.mark.parametrize("shape", [(12, 40, 56), (33, 9, 33), (128, 5, 6)],
                         ids=lambda s: "x".join(map(str, s)))
def test_four_paths(shape, ctx):
    v = random_volume(shape, _seed(shape))
    got = dense.aggregate(v, 0.1, 1.0, 4, return_aggregated=True, ctx=ctx)
    _equal(got, sr.solve(v, 0.1, 1.0, 4), shape)
    assert not np.array_equal(got[3], sr.aggregate(v, 0.1, 1.0, 8))


def test_all_nan_and_zero_penalties(ctx):
    v = np.full((7, 6, 9), np.nan, np.float32)
    got = dense.aggregate(v, return_aggregated=True, ctx=ctx)
    _equal(got, sr.solve(v), "all NaN")
    assert np.all(got[0] == -1) and np.all(got[1] == 0.0) and np.all(np.isnan(got[2]))
    v = random_volume((12, 40, 56), 3)
    got = dense.aggregate(v, 0.0, 0.0, 8, return_aggregated=True, ctx=ctx)
    _equal(got, sr.solve(v, 0.0, 0.0, 8), "p1 = p2 = 0")
    got = dense.aggregate(v, 0.25, 0.25, 8, return_aggregated=True, ctx=ctx)
    _equal(got, sr.solve(v, 0.25, 0.25, 8), "p1 = p2")


def _noisy_case():
    imgs, cams, _ = noisy_slanted()
    return imgs[0], cams[0], imgs[1:], cams[1:], df.K, df.DEPTHS, 3


def _cases():
    cases = {n: df.sweep_cases()[n] for n in ("odd_p5", "slanted_p7", "odd_D1", "odd_D2_S1",
                                               "tiny_p11")}
    cases["noisy_p3"] = _noisy_case()
    return cases


@pytest.mark.parametrize("name", ["odd_p5", "slanted_p7", "odd_D1", "odd_D2_S1", "tiny_p11",
                                  "noisy_p3"])
def test_plane_sweep_sgm(name, ctx):
    ref, rc, srcs, sc, K, depths, patch = _cases()[name]
    kw = dict(patch=patch, min_var=df.MIN_VAR, ctx=ctx)
    wta = dense.plane_sweep(ref, rc, srcs, sc, K, depths, return_volume=True, **kw)
    full = dense.plane_sweep_sgm(ref, rc, srcs, sc, K, depths, return_volume=True,
                                 return_aggregated=True, **kw)
    assert len(full) == 6
    index, delta, score, nvalid, volume, S = full
    assert _same_bits((volume, nvalid), (wta[4], wta[3]))
    _equal((index, delta, score, S), sr.solve(volume, 0.1, 1.0, 8), name)
    assert np.array_equal(index == -1, wta[0] == -1) and (index >= 0).any()
    plain = dense.plane_sweep_sgm(ref, rc, srcs, sc, K, depths, **kw)
    assert len(plain) == 4 and _same_bits(plain, full[:4])
    only_v = dense.plane_sweep_sgm(ref, rc, srcs, sc, K, depths, return_volume=True, **kw)
    only_s = dense.plane_sweep_sgm(ref, rc, srcs, sc, K, depths, return_aggregated=True, **kw)
    assert _same_bits(only_v, full[:5]) and _same_bits(only_s, full[:4] + full[5:])
    four = dense.plane_sweep_sgm(ref, rc, srcs, sc, K, depths, p1=0.05, p2=0.5, paths=4,
                                 return_aggregated=True, **kw)
    _equal(four[:3] + four[4:], sr.solve(volume, 0.05, 0.5, 4), name + " paths 4")
    if name == "noisy_p3":
        truth = df.true_index(noisy_slanted()[2][0])
        valid = wta[0] >= 0
        share = lambda idx: float((np.abs(idx - truth)[valid] <= 1.0).mean())
        print(f"within one plane of the truth: winner-takes-all {share(wta[0]):.3f}, "
              f"aggregated {share(index):.3f}")
        assert share(index) >= share(wta[0]) + 0.10


def test_fuse_smooth(ctx):
    imgs, cams, _ = noisy_slanted()
    kw = dict(neighbours=2, patch=3, min_var=df.MIN_VAR, min_views=2, rel_tol=0.01,
              return_maps=True, ctx=ctx)
    plain = dense.fuse(imgs, cams, df.K, df.DEPTHS, **kw)
    smooth = dense.fuse(imgs, cams, df.K, df.DEPTHS, smooth=(0.1, 1.0), **kw)
    maps = smooth[3]
    for i in range(3):
        nb = [j for j in range(3) if j != i]
        one = dense.plane_sweep_sgm(imgs[i], cams[i], imgs[nb], cams[nb], df.K, df.DEPTHS,
                                    patch=3, min_var=df.MIN_VAR, p1=0.1, p2=1.0, paths=8, ctx=ctx)
        assert _same_bits((maps["index"][i], maps["delta"][i]), one[:2])
    print(f"fuse keeps {len(plain[0])} pixels, with smooth=(0.1, 1.0) {len(smooth[0])}")
    assert len(smooth[0]) == maps["keep"].sum() and len(smooth[0]) >= len(plain[0])
    four = dense.fuse(imgs, cams, df.K, df.DEPTHS, smooth=(0.1, 1.0, 4), **kw)
    one = dense.plane_sweep_sgm(imgs[0], cams[0], imgs[1:], cams[1:], df.K, df.DEPTHS, patch=3,
                                min_var=df.MIN_VAR, paths=4, ctx=ctx)
    assert _same_bits((four[3]["index"][0], four[3]["delta"][0]), one[:2])
    again = dense.fuse(imgs, cams, df.K, df.DEPTHS, smooth=None, **kw)
    assert _same_bits([plain[3][k] for k in ("index", "delta", "count", "keep")],
                      [again[3][k] for k in ("index", "delta", "count", "keep")])
    with pytest.raises(ValueError):
        dense.fuse(imgs, cams, df.K, df.DEPTHS, smooth=(0.1,), **kw)


def test_reproducible_and_timing_slots():
    """Two runs are bit-equal, and timed and untimed runs are.  Slots start at -1; aggregate
    fills aggregate and select and leaves sweep alone; plane_sweep_sgm fills all three; a call
    after disabling changes nothing; dense.timing does not see these calls.  A context of its
    own, so that no earlier call has timed."""
    v = random_volume((33, 9, 33), 11)
    case = _noisy_case()
    sweep = lambda c: dense.plane_sweep_sgm(*case[:6], patch=case[6], min_var=df.MIN_VAR,
                                            return_volume=True, return_aggregated=True, ctx=c)
    timed = lambda ms, k: np.isfinite(ms[k]) and 0.0 < ms[k] < 1e3
    own = _ffi.Context()
    try:
        a1 = dense.aggregate(v, return_aggregated=True, ctx=own)
        a2 = dense.aggregate(v, return_aggregated=True, ctx=own)
        s1, s2 = sweep(own), sweep(own)
        assert _same_bits(a1, a2) and _same_bits(s1, s2)
        assert dense.sgm_timing(1, ctx=own) == {"sweep": -1.0, "aggregate": -1.0, "select": -1.0}
        a3 = dense.aggregate(v, return_aggregated=True, ctx=own)
        ms = dense.sgm_timing(1, ctx=own)
        print("after aggregate:", ms)
        assert ms["sweep"] == -1.0 and timed(ms, "aggregate") and timed(ms, "select")
        s3 = sweep(own)
        ms2 = dense.sgm_timing(0, ctx=own)
        print("after plane_sweep_sgm:", ms2)
        assert all(timed(ms2, k) for k in dense.SGM_STAGES)
        a4, s4 = dense.aggregate(v, return_aggregated=True, ctx=own), sweep(own)
        assert dense.sgm_timing(0, ctx=own) == ms2
        assert _same_bits(a1, a3) and _same_bits(a1, a4)
        assert _same_bits(s1, s3) and _same_bits(s1, s4)
        assert dense.timing(0, ctx=own) == {"plane_sweep": -1.0, "consistency": -1.0}
    finally:
        own.close()


def test_errors(ctx):
    v = random_volume((5, 6, 7), 1)

    def bad(volume=v, **kw):
        with pytest.raises(ValueError):
            dense.aggregate(volume, ctx=ctx, **kw)

    bad(paths=3)
    bad(paths=0)
    bad(p1=1.5)                                          # p1 > p2
    bad(p1=-0.1)
    for x in (np.nan, np.inf):
        bad(p1=x)
        bad(p2=x)
    bad(volume=v.astype(np.float64))
    bad(volume=v[0])
    bad(volume=np.zeros((0, 6, 7), np.float32))
    bad(volume=np.zeros((257, 2, 2), np.float32))
    bad(volume=np.zeros((5, 0, 7), np.float32))
    bad(volume=np.broadcast_to(np.float32(0), (2, 1, 16385)))
    bad(volume=np.broadcast_to(np.float32(0), (256, 1024, 513)))          # D h w > 2^27

    ref, rc, srcs, sc, K, depths, patch = df.sweep_cases()["fronto_p5"]

    def bad_sweep(**kw):
        a = dict(ref_image=ref, ref_cam=rc, src_images=srcs, src_cams=sc, K=K, depths=depths,
                 patch=5, min_var=4.0, ctx=ctx)
        a.update(kw)
        with pytest.raises(ValueError):
            dense.plane_sweep_sgm(**a)

    bad_sweep(paths=6)
    bad_sweep(p1=2.0, p2=1.0)
    bad_sweep(p1=-1.0)
    bad_sweep(p2=np.nan)
    bad_sweep(depths=np.linspace(2.0, 9.0, 257))                          # D > 256
    big = np.zeros((1024, 1024), np.uint8)
    bad_sweep(ref_image=big, src_images=[big, big], depths=np.linspace(2.0, 9.0, 129))
    for p in (1, 4, 13):                                                  # the sweep's own limits
        bad_sweep(patch=p)
    bad_sweep(src_images=[], src_cams=np.zeros((0, 3, 4)))
    bad_sweep(min_var=0.0)
    small = np.zeros((5, 20), np.uint8)
    bad_sweep(ref_image=small, src_images=[small, small])
    d = depths.copy()
    d[3] = -4.0
    bad_sweep(depths=d)


def test_c_abi_rejects_before_launch(ctx):
    """The limits hold at the C entries as well (RS_EINVAL), not only in the shims."""
    C = _ffi.C
    f = lambda a: _ffi.ptr(a, C.c_float)
    v = np.zeros((2, 4, 4), np.float32)
    idx = np.zeros((4, 4), np.int32)
    dl, sc = np.zeros((4, 4), np.float32), np.zeros((4, 4), np.float32)

    def agg(D=2, h=4, w=4, p1=0.1, p2=1.0, paths=8, volume=v, index=idx):
        return _ffi.lib().rs_dense_aggregate(
            ctx.handle, f(volume) if volume is not None else None, D, h, w, p1, p2, paths,
            _ffi.ptr(index, C.c_int32) if index is not None else None, f(dl), f(sc), None)

    for kw in (dict(D=0), dict(D=257), dict(paths=3), dict(p1=2.0), dict(p1=-0.5),
               dict(p1=np.nan), dict(p2=np.nan), dict(p2=np.inf), dict(h=0), dict(w=16385),
               dict(D=256, h=1024, w=513), dict(volume=None), dict(index=None)):
        assert agg(**kw) == _ffi.RS_EINVAL, kw
    assert agg() == _ffi.RS_OK

    img = np.zeros((16, 16), np.uint8)
    A, b = np.tile(np.eye(3), (1, 1, 1)), np.zeros((1, 3))
    nv = np.zeros((16, 16), np.uint8)
    i16, d16, s16 = np.zeros((16, 16), np.int32), np.zeros((16, 16), np.float32), \
        np.zeros((16, 16), np.float32)

    def sweep(D=2, patch=5, p1=0.1, p2=1.0, paths=8, h=16, w=16, S=1):
        depths = np.linspace(1.0, 2.0, max(D, 1))
        return _ffi.lib().rs_dense_plane_sweep_sgm(
            ctx.handle, _ffi.ptr(img, C.c_uint8), h, w, _ffi.ptr(img, C.c_uint8), S,
            _ffi.ptr(A, C.c_double), _ffi.ptr(b, C.c_double), _ffi.ptr(depths, C.c_double), D,
            patch, 4.0, p1, p2, paths, _ffi.ptr(i16, C.c_int32), f(d16), f(s16),
            _ffi.ptr(nv, C.c_uint8), None, None)

    for kw in (dict(D=0), dict(D=257), dict(paths=3), dict(p1=2.0), dict(p1=-0.5),
               dict(p1=np.nan), dict(p2=np.nan), dict(D=129, h=1024, w=1024), dict(patch=4),
               dict(S=0), dict(h=5)):
        assert sweep(**kw) == _ffi.RS_EINVAL, kw
    assert sweep() == _ffi.RS_OK
