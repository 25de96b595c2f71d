"""The dense stage on the GPU (tsbb15_amd.dense, csrc/dense.hip) against the numpy restatement
tests/dense_ref.py in fp64, on the procedural scenes of tests/dense_fixture.py.

SCORE_BAR.  The kernel forms the bilinear sample, the window sums, the score and the cost mean
in fp32, in its own summation order and with FMA contraction.  The bar is 8 x the largest
|cost(fp32, window sums reversed) - cost(fp64)| the restatement itself shows over every sweep
this file runs (dense_fixture.score_bar, computed from the restatement alone by the first test
that needs it and cached; tests/test_dense_cpu.py asserts it is below 1e-3).  Measured: largest deviation 5.07e-06
(fronto_p3), SCORE_BAR = 4.06e-05.

Validity flags (the NaN pattern, nvalid, index -1) are compared exactly: the CPU test asserts
that no warped coordinate of these sweeps lies within 1e-9 px of a validity boundary and no
warped-window variance within 2.0 of min_var n.

nvalid.  The stage's specification says "nvalid is equal".  Where the GPU's index equals the
restatement's, that is what is asserted.  On a near-tie the GPU may hold another index (one whose
reference cost is within 2 SCORE_BAR of the best), and its nvalid is then that hypothesis's
own source count, which may differ from the reference winner's; there the test asserts nvalid
against the restatement's count for the GPU's index.  This is a reading of the wording, not
the wording itself.
"""
import numpy as np
import pytest

import dense_fixture as df
import dense_ref as dr
from tsbb15_amd import _ffi, dense

pytestmark = pytest.mark.gpu



def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a


def _same_bits(got, want):
    return all(x.shape == y.shape and x.dtype == y.dtype and np.array_equal(_bits(x), _bits(y))
               for x, y in zip(got, want))


def _sweep(case, ctx, **kw):
    ref, rc, srcs, sc, K, depths, patch = case
    return dense.plane_sweep(ref, rc, srcs, sc, K, depths, patch=patch, min_var=df.MIN_VAR,
                             ctx=ctx, **kw)


def _check(got, want, name):
    """Test 1's comparison of (index, delta, score, nvalid, volume) with the fp64 restatement.
    Returns the number of pixels whose index differs (all of them near-ties)."""
    SCORE_BAR = df.score_bar()
    index, delta, score, nvalid, volume = got
    rindex, rdelta, rscore, rnvalid, rvolume, rcounts = want
    assert index.dtype == np.int32 and nvalid.dtype == np.uint8
    assert delta.dtype == score.dtype == volume.dtype == np.float32
    assert np.array_equal(np.isnan(volume), np.isnan(rvolume))
    ok = ~np.isnan(rvolume)
    dcost = float(np.abs(volume[ok] - rvolume[ok]).max()) if ok.any() else 0.0
    valid = rindex >= 0
    assert np.array_equal(index >= 0, valid)
    assert np.array_equal(index[~valid], rindex[~valid])
    assert np.array_equal(nvalid[~valid], rnvalid[~valid])
    assert np.all(np.isnan(score[~valid])) and np.all(delta[~valid] == 0.0)
    yy, xx = np.nonzero(valid)
    # the reference's costs at the GPU's index, and its best-to-second gap
    at_gpu = rvolume[index[valid], yy, xx]
    srt = np.sort(np.where(np.isnan(rvolume), -np.inf, rvolume), axis=0)
    with np.errstate(invalid="ignore"):
        gap = (srt[-1] - srt[-2])[valid] if len(rvolume) > 1 else np.full(valid.sum(), np.inf)
    clear = gap > 2 * SCORE_BAR
    differ = index[valid] != rindex[valid]
    dscore = float(np.abs(score[valid] - rscore[valid]).max()) if valid.any() else 0.0
    same = valid & (index == rindex)
    curv = dr.curvature(rvolume, rindex)
    three = same & np.isfinite(curv) & (curv < 0)
    ddelta = np.abs(delta[three] - rdelta[three]) * np.abs(curv[three])
    print(f"{name}: d cost {dcost:.2e}, d score {dscore:.2e}, bar {SCORE_BAR:.2e}; "
          f"{int(valid.sum())} valid pixels, {int((~clear).sum())} near-ties, "
          f"{int(differ.sum())} indices differ; d delta |curvature| "
          f"{float(ddelta.max()) if ddelta.size else 0.0:.2e} on {int(three.sum())} pixels")
    assert dcost <= SCORE_BAR
    assert not np.any(differ & clear)
    assert np.all(rscore[valid] - at_gpu <= 2 * SCORE_BAR)      # leaves out no pixel
    assert np.array_equal(nvalid[same], rnvalid[same])
    # where the indices differ the GPU reports the source count of its own hypothesis
    assert np.array_equal(nvalid[valid], rcounts[index[valid], yy, xx])
    assert dscore <= SCORE_BAR
    assert np.all(ddelta <= 8 * SCORE_BAR)
    away = same & ~three
    assert np.all(delta[away & ~np.isfinite(curv)] == 0.0)
    assert np.all(np.abs(delta) <= 0.5)
    return int(differ.sum())


@pytest.mark.parametrize("name", ["fronto_p3", "fronto_p5", "fronto_p7",
                                  "slanted_p3", "slanted_p5", "slanted_p7"])
def test_volume_and_winners(name, ctx):
    got = _sweep(df.sweep_cases()[name], ctx, return_volume=True)
    _check(got, df.reference_sweeps()[name], name)


@pytest.mark.parametrize("name", ["odd_p5", "odd_p9_D33", "odd_D1", "odd_D2_S1", "odd_S8",
                                  "tiny_p11", "slanted_p11"])
def test_size_boundaries(name, ctx):
    case = df.sweep_cases()[name]
    got = _sweep(case, ctx, return_volume=True)
    want = df.reference_sweeps()[name]
    _check(got, want, name)
    valid = want[0] >= 0
    assert valid.any()
    if name == "odd_D1":
        assert np.all(got[1] == 0.0) and set(np.unique(got[0])) == {-1, 0}
    if name == "odd_S8":
        assert len(np.unique(got[3][valid])) >= 4 and got[3].max() <= 5
    if name == "tiny_p11":
        assert valid.sum() == 4 and np.all(got[3][valid] == 1)


def test_negated_scene(ctx):
    ref, rc, srcs, sc, K, depths, patch = df.sweep_cases()["slanted_p7"]
    pos = dense.plane_sweep(ref, rc, srcs, sc, K, depths, patch=patch, ctx=ctx)
    neg = dense.plane_sweep(ref, -rc, srcs, -sc, K, -depths, patch=patch, ctx=ctx)
    assert (pos[0] >= 0).sum() > 1000
    assert _same_bits(neg, pos)
    assert np.array_equal(dense.refine_depth(neg[0], neg[1], -depths),
                          -dense.refine_depth(pos[0], pos[1], depths), equal_nan=True)


def test_invalid_regions(ctx):
    ref, rc, srcs, sc, K, depths, patch = df.sweep_cases()["fronto_p5"]
    r = patch // 2
    half = ref.copy()
    half[:, :df.W // 2] = 128
    got = dense.plane_sweep(half, rc, srcs, sc, K, depths, patch=patch, return_volume=True,
                            ctx=ctx)
    want = dr.plane_sweep(half, rc, srcs, sc, K, depths, patch, df.MIN_VAR)
    assert np.array_equal(got[0] == -1, want[0] == -1)
    assert np.array_equal(np.isnan(got[4]), np.isnan(want[4]))
    assert np.array_equal(got[3], want[3])
    assert np.all(got[0][:, :df.W // 2 - r] == -1)          # windows wholly in the flat half
    assert (got[0][:, df.W // 2:] >= 0).sum() > 500
    border = np.ones(ref.shape, bool)
    border[r:-r, r:-r] = False
    for res in (got, _sweep(df.sweep_cases()["fronto_p5"], ctx)):
        assert np.all(res[0][border] == -1) and np.all(res[3][border] == 0)
        assert np.all(np.isnan(res[2][border])) and np.all(res[1][border] == 0.0)
    flat = dense.plane_sweep(np.full_like(ref, 77), rc, srcs, sc, K, depths, patch=patch,
                             return_volume=True, ctx=ctx)
    assert np.all(flat[0] == -1) and np.all(flat[3] == 0) and np.all(flat[1] == 0.0)
    assert np.all(np.isnan(flat[2])) and np.all(np.isnan(flat[4]))


def test_reproducible(ctx):
    case = df.sweep_cases()["odd_S8"]
    a = _sweep(case, ctx, return_volume=True)
    b = _sweep(case, ctx, return_volume=True)
    c = _sweep(case, ctx)
    assert _same_bits(a, b)
    assert len(c) == 4 and _same_bits(c, a[:4])


def test_errors(ctx):
    ref, rc, srcs, sc, K, depths, patch = df.sweep_cases()["fronto_p5"]

    def bad(**kw):
        a = dict(ref_image=ref, ref_cam=rc, src_images=srcs, src_cams=sc, K=K, depths=depths,
                 patch=5, min_var=4.0, ctx=ctx)
        a.update(kw)
        with pytest.raises(ValueError):
            dense.plane_sweep(**a)

    for p in (1, 4, 13):
        bad(patch=p)
    bad(src_images=[], src_cams=np.zeros((0, 3, 4)))
    bad(src_images=[srcs[0]] * 9, src_cams=np.array([sc[0]] * 9))
    bad(depths=[])
    bad(depths=np.linspace(2.0, 9.0, 4097))
    small = np.zeros((5, 20), np.uint8)
    bad(ref_image=small, src_images=[small, small])                       # a side not above patch
    bad(ref_image=np.zeros((6, 16385), np.uint8), src_images=[np.zeros((6, 16385), np.uint8)] * 2)
    big = np.zeros((8193, 8193), np.uint8)                                # h w > 2^26, sides allowed
    bad(ref_image=big, src_images=[big, big])
    bad(depths=np.linspace(2.0, 9.0, 4096), return_volume=True, ref_image=np.zeros((300, 300), np.uint8),
        src_images=[np.zeros((300, 300), np.uint8)] * 2)                  # D h w > 2^28
    Kb = K.copy()
    Kb[2] = (0.0, 1e-3, 1.0)
    bad(K=Kb)
    sing = rc.copy()
    sing[2, :3] = sing[1, :3]
    bad(ref_cam=sing)
    for mv in (0.0, -1.0, np.inf, np.nan):
        bad(min_var=mv)
    bad(ref_image=ref.astype(np.float32))
    bad(ref_image=np.stack((ref, ref)))
    bad(src_images=[srcs[0], srcs[1][:-1]])
    nanc = sc.copy()
    nanc[1, 0, 0] = np.nan
    bad(src_cams=nanc)
    infc = rc.copy()
    infc[0, 3] = np.inf
    bad(ref_cam=infc)
    for k, v in ((3, 0.0), (3, np.nan), (3, np.inf), (3, -4.0)):
        d = depths.copy()
        d[k] = v
        bad(depths=d)
    bad(src_cams=sc[:1])                                                  # one camera per image
    depth, cams = df.consistency_case()
    with pytest.raises(ValueError):
        dense.consistency(depth[:2], cams, df.K, ctx=ctx)
    with pytest.raises(ValueError):
        dense.consistency(depth, cams, df.K, rel_tol=-0.1, ctx=ctx)
    with pytest.raises(ValueError):
        dense.consistency(np.zeros((129, 4, 4)), np.tile(cams[:1], (129, 1, 1)), df.K, ctx=ctx)


def test_c_abi_rejects_before_launch(ctx):
    """The limits hold at the C entry as well (RS_EINVAL -> ValueError), not only in the shim."""
    from tsbb15_amd import _ffi
    C = _ffi.C
    img = np.zeros((16, 16), np.uint8)
    A, b, d = np.tile(np.eye(3), (1, 1, 1)), np.zeros((1, 3)), np.array([1.0, -1.0])
    idx, nv = np.zeros((16, 16), np.int32), np.zeros((16, 16), np.uint8)
    dl, sc = np.zeros((16, 16), np.float32), np.zeros((16, 16), np.float32)

    def call(S=1, D=2, patch=5, min_var=4.0, h=16, w=16, depths=d):
        return _ffi.lib().rs_dense_plane_sweep(
            ctx.handle, _ffi.ptr(img, C.c_uint8), h, w, _ffi.ptr(img, C.c_uint8), S,
            _ffi.ptr(A, C.c_double), _ffi.ptr(b, C.c_double), _ffi.ptr(depths, C.c_double), D,
            patch, min_var, _ffi.ptr(idx, C.c_int32), _ffi.ptr(dl, C.c_float),
            _ffi.ptr(sc, C.c_float), _ffi.ptr(nv, C.c_uint8), None)

    assert call() == _ffi.RS_EINVAL                                       # mixed sign
    ok = np.array([1.0, 2.0])
    for kw in (dict(S=0), dict(S=9), dict(D=0), dict(D=4097), dict(patch=4), dict(patch=13),
               dict(min_var=0.0), dict(h=5), dict(w=16385), dict(h=8193, w=8193),
               dict(depths=np.array([1.0, 0.0]))):
        kw.setdefault("depths", ok)
        assert call(**kw) == _ffi.RS_EINVAL, kw
    assert call(depths=ok) == _ffi.RS_OK


def test_consistency(ctx):
    depth, cams = df.consistency_case()
    want = dr.consistency(depth, cams, df.K, 0.01)
    got = dense.consistency(depth, cams, df.K, rel_tol=0.01, ctx=ctx)
    print("consistency counts", np.bincount(want.ravel()))
    assert got.dtype == np.uint8 and np.array_equal(got, want)
    assert want.max() == 2 and (want == 2).sum() > 500
    assert np.all(got[0, 15:22, 20:31] == 0)            # the NaN hole
    assert np.all(got[3] == 0)                          # the view that sees nothing
    assert np.all(got[np.isnan(depth)] == 0)
    # the three maps alone, and a looser tolerance
    for tol in (0.01, 0.05):
        assert np.array_equal(dense.consistency(depth[:3], cams[:3], df.K, rel_tol=tol, ctx=ctx),
                              dr.consistency(depth[:3], cams[:3], df.K, tol))
    pts = dense.depth_points(depth[1], cams[1], df.K)
    assert np.allclose(pts, dr.depth_points(depth[1], cams[1], df.K), rtol=0, atol=1e-12,
                       equal_nan=True)


def test_fuse(ctx):
    imgs, cams, true_depth = df.scene("slanted")
    pts, grey, view, maps = dense.fuse(imgs, cams, df.K, df.DEPTHS, neighbours=2, patch=7,
                                       min_var=df.MIN_VAR, min_views=2, rel_tol=0.01,
                                       return_maps=True, ctx=ctx)
    ridx, rdelta, rdepth, rvol = df.reference_depth_maps("slanted")
    rkeep = dr.consistency(rdepth, cams, df.K, 0.01) >= 2
    keep = maps["keep"]
    assert len(pts) == len(grey) == len(view) == keep.sum() and pts.shape[1:] == (3,)
    # The reference pipeline with the GPU's winner wherever test 1 let it differ (a near-tie):
    # the GPU's mask must equal this one, up to its deltas.  Test 1 bounds a delta to within
    # 8 SCORE_BAR / |curvature| of the reference's, which moves 1 / depth by 0.025 of that: g is,
    # pixel by pixel, the relative depth change this allows (0 where both deltas are 0 by
    # definition, and where the GPU's own winner is used).  A pixel is excused when its own g
    # and that of the pixel it reads could change an agreement or a rounding
    # (dense_ref.consistency, `allowance`).
    SCORE_BAR = df.score_bar()
    differs = maps["index"] != ridx
    hidx = np.where(differs, maps["index"], ridx)
    hdelta = np.where(differs, maps["delta"].astype(np.float64), rdelta)
    hdepth = np.array([dr.refine_depth(hidx[i], hdelta[i], df.DEPTHS) for i in range(3)])
    curv = np.array([dr.curvature(rvol[i], ridx[i]) for i in range(3)])
    with np.errstate(invalid="ignore", divide="ignore"):
        g = 8 * SCORE_BAR / np.abs(curv) * 0.025 * np.abs(rdepth)
        g = np.where(np.isfinite(curv) & (curv < 0) & ~differs & np.isfinite(g), g, 0.0)
    hcount, _, _, excused = dr.consistency(hdepth, cams, df.K, 0.01, details=True, allowance=g)
    diff = keep != rkeep
    print(f"fuse: kept {int(keep.sum())} (reference {int(rkeep.sum())}), {int(diff.sum())} "
          f"differ from the reference mask, {int(differs.sum())} winners differ, g median "
          f"{float(np.median(g[g > 0])):.2e} max {float(g.max()):.2e}, {int(excused.sum())} "
          f"pixels excused, {int((keep != (hcount >= 2)).sum())} differ from the mask with the "
          f"GPU's near-tie winners")
    assert not np.any((keep != (hcount >= 2)) & ~excused)
    assert excused.sum() <= 0.05 * keep.size
    assert diff.sum() <= 0.02 * rkeep.sum()
    assert rkeep.sum() > 1000
    # every kept point within one depth step of the true plane
    off = np.abs(df.true_index(maps["depth"]) - df.true_index(true_depth))
    assert np.all(off[keep] <= 1.0)
    n, c = df.SLANTED
    assert np.abs(pts @ n - c).max() < 0.5
    assert np.all((grey >= 0) & (grey <= 1)) and np.array_equal(np.unique(view), [0, 1, 2])


def test_timing_slots():
    """Slots start at -1; rs_dense_plane_sweep fills plane_sweep alone and rs_dense_consistency
    fills consistency alone; a call after disabling changes nothing; timed and untimed results
    are bit-equal.  A context of its own, so that no earlier call has timed."""
    case = df.sweep_cases()["fronto_p5"]
    depth, cams = df.consistency_case()
    timed = lambda ms, k: np.isfinite(ms[k]) and 0.0 < ms[k] < 1e3
    own = _ffi.Context()
    try:
        plain_s = _sweep(case, own, return_volume=True)
        plain_c = dense.consistency(depth, cams, df.K, rel_tol=0.01, ctx=own)
        assert dense.timing(1, ctx=own) == {"plane_sweep": -1.0, "consistency": -1.0}
        timed_c = dense.consistency(depth, cams, df.K, rel_tol=0.01, ctx=own)
        ms = dense.timing(1, ctx=own)
        print("after consistency:", ms)
        assert timed(ms, "consistency") and ms["plane_sweep"] == -1.0
        timed_s = _sweep(case, own, return_volume=True)
        ms2 = dense.timing(0, ctx=own)
        print("after plane_sweep:", ms2)
        assert timed(ms2, "plane_sweep") and ms2["consistency"] == ms["consistency"]
        again_s = _sweep(case, own, return_volume=True)
        again_c = dense.consistency(depth, cams, df.K, rel_tol=0.01, ctx=own)
        assert dense.timing(0, ctx=own) == ms2
        assert _same_bits(plain_s, timed_s) and _same_bits(plain_s, again_s)
        assert np.array_equal(plain_c, timed_c) and np.array_equal(plain_c, again_c)
    finally:
        own.close()
