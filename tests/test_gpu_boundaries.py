"""The dense, surface and colour kernels exactly on their decision boundaries: the cases of
tests/boundary_fixture.py through the C entries, which take A, b, P and Minv as the fixture
states them, against tests/dense_ref.py, tests/surface_ref.py and tests/texture_ref.py and the
answers written out by hand in the fixture.  tests/test_boundaries_cpu.py proves that every case
sits on its boundary with margin exactly 0 and that fp32 and fp64 agree on every flag there, so
flags, counts, indices and NaN patterns are compared exactly and no pixel is excused.

BAR.  Plane-sweep costs and scores use the recipe of dense_fixture.score_bar on these cases
alone (boundary_fixture.score_bar): 8 x the largest deviation of the restatement in float32 with
reversed window sums from the restatement in fp64.  Measured: largest deviation 8.71e-08
(tie_pair), BAR = 6.97e-07.  The inputs make every window sum exact, so what is left is the
rounding of va vb, the square root and the quotient.

delta at a planted tie.  With c+ == c0 bit for bit the header's formula is 0.5 in real
arithmetic.  In float32, c- - 2 c0 is rounded before c+ is added, so the quotient is 1 or a few
floats off it, and delta is 0.5 or a few floats below (measured: 0.49999976 to 0.5); which one
depends on the last bits of c-.
tie_exact makes every step exact (costs -1, 1, 1) and there delta == 0.5 is asserted.  In
tie_pair and tie_triple the test asserts what the header fixes whatever the last bit: the first
copy wins, the copies' costs are equal bit for bit, and delta is bitwise the header's float32
formula of the three costs the kernel itself reports.  The mirror case, a clamp at -0.5, cannot
be planted: it needs c- >= c0, and then the strict comparison has already given the win to
index - 1.
"""
import numpy as np
import pytest

import boundary_fixture as bf
import dense_ref as dr
import surface_ref as sr
import texture_ref as tr
from tsbb15_amd import _ffi

pytestmark = pytest.mark.gpu

C = _ffi.C
_u8, _i32, _f32, _f64 = C.c_uint8, C.c_int32, C.c_float, C.c_double


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else \
        a.view(np.int64) if a.dtype == np.float64 else a


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(_bits(a), _bits(b))


# ------------------------------------------------------------------------------------------
# plane sweep
# ------------------------------------------------------------------------------------------
def _sweep(ctx, case, sgm=False):
    """(index, delta, score, nvalid, volume) of rs_dense_plane_sweep, or of
    rs_dense_plane_sweep_sgm (p1 = 1/8, p2 = 1, 8 paths)."""
    h, w = case["ref"].shape
    S, D = len(case["srcs"]), len(case["depths"])
    index, nvalid = np.full((h, w), -7, np.int32), np.full((h, w), 7, np.uint8)
    delta, score = np.full((h, w), -7, np.float32), np.full((h, w), -7, np.float32)
    volume = np.full((D, h, w), -7, np.float32)
    args = [ctx.handle, _ffi.ptr(case["ref"], _u8), h, w, _ffi.ptr(case["srcs"], _u8), S,
            _ffi.ptr(case["A"], _f64), _ffi.ptr(case["b"], _f64), _ffi.ptr(case["depths"], _f64),
            D, case["patch"], case["min_var"]]
    out = [_ffi.ptr(index, _i32), _ffi.ptr(delta, _f32), _ffi.ptr(score, _f32),
           _ffi.ptr(nvalid, _u8), _ffi.ptr(volume, _f32)]
    if sgm:
        _ffi.check(_ffi.lib().rs_dense_plane_sweep_sgm(*args, 0.125, 1.0, 8, *out, None))
    else:
        _ffi.check(_ffi.lib().rs_dense_plane_sweep(*args, *out))
    return index, delta, score, nvalid, volume


def _header_delta(cm, c0, cp):
    """clamp(0.5 (c- - c+) / (c- - 2 c0 + c+), -0.5, 0.5) in float32, one rounding a step."""
    f = np.float32
    den = (cm - f(2) * c0) + cp
    return np.clip(f(0.5) * (cm - cp) / den, f(-0.5), f(0.5))


def _check_sweep(name, got):
    """Flags, index and nvalid exactly, costs to BAR, delta by the header; returns the mask of the
    planted ties."""
    BAR = bf.score_bar()
    index, delta, score, nvalid, volume = got
    rindex, rdelta, rscore, rnvalid, rvolume, _ = bf.reference_sweeps()[name]
    assert index.dtype == np.int32 and nvalid.dtype == np.uint8
    assert np.array_equal(np.isnan(volume), np.isnan(rvolume))
    assert np.array_equal(index, rindex)                      # the -1 set included, none excused
    assert np.array_equal(nvalid, rnvalid)
    hand = bf.hand_valid(name)
    if hand is not None:
        assert np.array_equal(~np.isnan(volume), hand)
    valid = rindex >= 0
    assert np.all(np.isnan(score[~valid])) and np.all(delta[~valid] == 0.0)
    ok = ~np.isnan(rvolume)
    dcost = float(np.abs(volume[ok] - rvolume[ok]).max()) if ok.any() else 0.0
    dscore = float(np.abs(score[valid] - rscore[valid]).max()) if valid.any() else 0.0
    D, (h, w) = len(volume), index.shape
    yy, xx = np.mgrid[0:h, 0:w]
    i = np.maximum(index, 0)
    c0 = volume[i, yy, xx]
    assert np.array_equal(_bits(score[valid]), _bits(c0[valid]))
    cm = np.where(i > 0, volume[np.maximum(i - 1, 0), yy, xx], np.float32(np.nan))
    cp = np.where(i < D - 1, volume[np.minimum(i + 1, D - 1), yy, xx], np.float32(np.nan))
    three = valid & ~np.isnan(cm) & ~np.isnan(cp)
    assert np.all(delta[~three] == 0.0)
    tie = three & (_bits(cp) == _bits(c0))                    # a planted tie: the next copy
    curv = dr.curvature(rvolume, rindex)
    with np.errstate(invalid="ignore"):
        rtie = valid & (curv < 0) & (rvolume[np.minimum(i + 1, D - 1), yy, xx] == rvolume[i, yy, xx])
    assert np.array_equal(tie, rtie)
    with np.errstate(invalid="ignore", divide="ignore"):
        want = _header_delta(cm, c0, cp)
    assert np.array_equal(_bits(delta[tie]), _bits(want[tie]))
    assert np.all(delta[tie] <= 0.5) and np.all(delta[tie] >= np.float32(0.5) - np.float32(2e-6))
    away = three & ~tie
    assert np.all(np.isfinite(curv[away]) & (curv[away] < 0))
    ddelta = np.abs(delta[away] - rdelta[away]) * np.abs(curv[away])
    print(f"{name}: {int(valid.sum())} valid pixels, {int((~valid).sum())} without a hypothesis, "
          f"index, nvalid and the NaN pattern equal at all of them; d cost {dcost:.2e}, d score "
          f"{dscore:.2e}, bar {BAR:.2e}; {int(tie.sum())} planted ties; d delta |curvature| "
          f"{float(ddelta.max()) if ddelta.size else 0.0:.2e} on {int(away.sum())} pixels")
    assert dcost <= BAR and dscore <= BAR
    assert np.all(ddelta <= 8 * BAR)
    assert np.all(np.abs(delta) <= 0.5)
    return tie


@pytest.mark.parametrize("name", ["xpos_8x32_p3", "xneg_9x33_p3", "ypos_16x64_p3",
                                  "yneg_9x33_p3", "xpos_12x44_p11", "xboth_8x32_p3"])
def test_sweep_image_edges_and_tile_fit(name, ctx):
    """x' == 0, w - 1, y' == 0, h - 1 valid (the neighbour clamped), -1/2, w - 1/2, w invalid, on
    one tile exactly, with a row and a column of spill, on 2 x 2 tiles, and with patch 11."""
    tie = _check_sweep(name, _sweep(ctx, bf.sweep_cases()[name]))
    assert not tie.any()


def test_sweep_q2_zero(ctx):
    """q2 d == 0 on column 11: its windows are invalid, those one column on are valid, and the
    division by zero reaches no index."""
    got = _sweep(ctx, bf.sweep_cases()["q2_zero"])
    _check_sweep("q2_zero", got)
    assert np.all(got[0][1:7, 13:15] == 0) and (got[0] == 0).sum() == 12


@pytest.mark.parametrize("side", ["ref", "src"])
def test_sweep_variance_threshold(side, ctx):
    """n sum a^2 - (sum a)^2 == min_var n^2 == 162 is valid, on the reference side (integers) and
    on the warped side (float32); one float32 step of min_var above it nothing is."""
    on = _sweep(ctx, bf.sweep_cases()[f"var_{side}_on"])
    _check_sweep(f"var_{side}_on", on)
    assert (~np.isnan(on[4])).sum() == 6
    above = _sweep(ctx, bf.sweep_cases()[f"var_{side}_above"])
    _check_sweep(f"var_{side}_above", above)
    assert np.all(above[0] == -1) and np.all(np.isnan(above[4])) and np.all(above[3] == 0)


@pytest.mark.parametrize("name, k", [("tie_pair", 2), ("tie_triple", 1), ("tie_exact", 1)])
def test_sweep_ties(name, k, ctx):
    """A repeated depth: the first copy wins, the copies cost the same bit for bit, delta is the
    header's formula; 0.5 exactly where the costs are -1, 1, 1."""
    got = _sweep(ctx, bf.sweep_cases()[name])
    tie = _check_sweep(name, got)
    index, delta, _, _, volume = got
    assert tie.sum() >= 100 and np.all(index[tie] == k)
    depths = bf.sweep_cases()[name]["depths"]
    for j in range(len(depths)):
        if depths[j] == depths[k]:
            assert _same(volume[j], volume[k])
    if name == "tie_exact":
        assert np.array_equal(tie, index == 1)
        assert np.all(volume[0][tie] == -1.0) and np.all(volume[1][tie] == 1.0)
        assert np.all(delta[tie] == 0.5)
    print(f"{name}: delta at the ties: {np.unique(delta[tie])}")


def test_sweep_twin_sources(ctx):
    """Two identical sources: nvalid == 2 and the cost of one source, bit for bit."""
    one = _sweep(ctx, bf.sweep_cases()["xpos_8x32_p3"])
    two = _sweep(ctx, bf.sweep_cases()["twin_sources"])
    _check_sweep("twin_sources", two)
    assert (one[0] >= 0).sum() > 100
    assert _same(two[4], one[4]) and _same(two[2], one[2]) and _same(two[1], one[1])
    assert np.array_equal(two[0], one[0]) and np.array_equal(two[3], 2 * one[3])


@pytest.mark.parametrize("name, k", [("deep_last", 4095), ("deep_first", 0)])
def test_sweep_max_depths(name, k, ctx):
    """RS_DENSE_MAX_DEPTHS planes, the only valid one the last, and again the first."""
    got = _sweep(ctx, bf.sweep_cases()[name])
    _check_sweep(name, got)
    assert np.all(got[0][1:3, 1] == k) and (got[0] == -1).sum() == 14
    assert np.all(got[2][1:3, 1] == 1.0)


@pytest.mark.parametrize("name", bf.SGM_CASES)
def test_sweep_sgm_volume(name, ctx):
    """rs_dense_plane_sweep_sgm: volume and nvalid are bitwise those of the plain sweep."""
    case = bf.sweep_cases()[name]
    plain, sgm = _sweep(ctx, case), _sweep(ctx, case, sgm=True)
    _check_sweep(name, plain)
    assert _same(sgm[4], plain[4]) and _same(sgm[3], plain[3])
    assert np.array_equal(sgm[0] == -1, plain[0] == -1)
    print(f"{name}: sgm volume and nvalid bitwise equal, {int((sgm[0] != plain[0]).sum())} "
          f"aggregated winners differ from winner-takes-all")


# ------------------------------------------------------------------------------------------
# consistency
# ------------------------------------------------------------------------------------------
def _consistency(ctx, case):
    depth = case["depth"]
    V, h, w = depth.shape
    count = np.full((V, h, w), 77, np.uint8)
    _ffi.check(_ffi.lib().rs_dense_consistency(
        ctx.handle, _ffi.ptr(depth, _f64), V, h, w, _ffi.ptr(case["P"], _f64),
        _ffi.ptr(case["Minv"], _f64), case["rel_tol"], _ffi.ptr(count, _u8)))
    return count


@pytest.mark.parametrize("name", tuple(bf.consistency_cases()))
def test_consistency(name, ctx):
    """Projections on exact half-integers (2.5 to 3, -0.5 to 0, w - 0.5 to w), a depth difference
    of exactly rel_tol |d'| and the double past it, rel_tol 0, infinite depths, 128 views, and
    h w V on both sides of a workgroup's 256 lanes."""
    case = bf.consistency_cases()[name]
    got = _consistency(ctx, case)
    want = dr.consistency(case["depth"], case["P"], bf.I3, case["rel_tol"])
    values, lanes = np.unique(want, return_counts=True)
    print(f"{name}: counts {dict(zip(values.tolist(), lanes.tolist()))} over {want.size} lanes")
    assert np.array_equal(got, want)
    if name.startswith("half_pixel"):
        assert np.array_equal(got[0], bf.HALF_PIXEL_VIEW0[case["rel_tol"]])
        assert np.all(got[1][~np.isfinite(case["depth"][1])] == 0)
    if name == "views128":
        assert np.all(got == 127)


# ------------------------------------------------------------------------------------------
# TSDF fusion, extraction
# ------------------------------------------------------------------------------------------
def _integrate(ctx, case):
    V, h, w = case["depth"].shape
    nz, ny, nx = case["dims"]
    prior = case["tsdf"] is not None
    tsdf = case["tsdf"].copy() if prior else np.full(case["dims"], -7, np.float32)
    weight = case["weight"].copy() if prior else np.full(case["dims"], -7, np.float32)
    wts = case["weights"]
    _ffi.check(_ffi.lib().rs_surface_integrate(
        ctx.handle, _ffi.ptr(case["depth"], _f64), _ffi.ptr(wts, _f32) if wts is not None else None,
        V, h, w, _ffi.ptr(case["P"], _f64), _ffi.ptr(case["origin"], _f64), case["voxel"],
        nz, ny, nx, case["trunc"], int(prior), _ffi.ptr(tsdf, _f32), _ffi.ptr(weight, _f32)))
    return tsdf, weight


@pytest.mark.parametrize("name", tuple(bf.tsdf_cases()))
def test_tsdf(name, ctx):
    """Projections on half-integers and on u == w - 1, v == h - 1; s == -trunc (-1), the double
    behind it (nothing), s == trunc (1); a node on the camera plane; weights of 0, below 0, NaN
    and +inf; a prior whose weight is not > 0.  Every quotient is an fp64 number, so tsdf and
    weight are compared bit for bit."""
    case = bf.tsdf_cases()[name]
    got = _integrate(ctx, case)
    want = sr.integrate(case["depth"], case["P"], bf.I3, case["origin"], case["voxel"],
                        case["dims"], case["trunc"], case["weights"], case["tsdf"],
                        case["weight"])
    print(f"{name}: {int(np.isfinite(want[0]).sum())} of {want[0].size} nodes fused, tsdf values "
          f"{np.unique(want[0][np.isfinite(want[0])]).tolist()[:8]}")
    assert np.array_equal(np.isnan(got[0]), np.isnan(want[0]))
    assert _same(np.nan_to_num(got[0], nan=9.0), np.nan_to_num(want[0], nan=9.0))
    assert _same(got[1], want[1])
    if name == "plain":
        assert np.all(np.isnan(got[0][0])) and np.all(got[1][0] == 0)
        assert got[0][4, 0, 0] == -1.0 and np.isnan(got[0][4, 0, 2]) and got[0][2, 0, 1] == 1.0


@pytest.mark.parametrize("name", tuple(bf.extract_cases()))
def test_extract(name, ctx):
    """-0.0f is not negative; a node of weight exactly min_weight keeps its cell, the float
    below drops it."""
    from tsbb15_amd import surface
    tsdf, weight, origin, voxel, min_weight, nf = bf.extract_cases()[name]
    v, f = surface.extract(tsdf, weight, origin, voxel, min_weight=min_weight, ctx=ctx)
    rv, rf = sr.extract(tsdf, weight, origin, voxel, min_weight)
    print(f"{name}: {len(v)} vertices, {len(f)} faces")
    assert _same(v, rv) and np.array_equal(f, rf)
    assert (len(f) == 0) == (nf == 0)


# ------------------------------------------------------------------------------------------
# z-buffer, gather
# ------------------------------------------------------------------------------------------
def _render(ctx, v, f, shape):
    v, f = np.ascontiguousarray(v, dtype=np.float64), np.ascontiguousarray(f, dtype=np.int32)
    z = np.full((1,) + tuple(shape), -7, np.float32)
    _ffi.check(_ffi.lib().rs_surface_render_depth(
        ctx.handle, _ffi.ptr(v, _f64), len(v), _ffi.ptr(f, _i32), len(f),
        _ffi.ptr(bf.TEX_P, _f64), 1, shape[0], shape[1], _ffi.ptr(z, _f32)))
    return z


def _ulps(a, b):
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


@pytest.mark.parametrize("name", tuple(bf.raster_cases()))
def test_raster(name, ctx):
    """b == 0 exactly on a shared edge through pixel centres and on the box's own edges, boxes
    of 25 pixels (the lane kernel) and 81 (the wave kernel), a coordinate of -0.0, a vertex on
    the camera plane.  Coverage is compared exactly; the fronto plane's depth bit for bit."""
    v, f, shape, hand = bf.raster_cases()[name]
    z = _render(ctx, v, f, shape)
    want = tr.render_depth(v, f, bf.TEX_P, shape)
    print(f"{name}: {int(np.isfinite(want).sum())} of {want.size} pixels covered")
    assert np.array_equal(np.isnan(z), np.isnan(want))
    if hand is not None:
        assert _same(z, hand)
    both = ~np.isnan(want)
    assert not both.any() or _ulps(z[both], want[both]).max() <= 1
    if name.startswith("pair"):
        assert both.all() and np.all(z == 4.0)
        a = _render(ctx, v, f[:1], shape)
        b = _render(ctx, v, f[1:], shape)
        assert np.isfinite(a).sum() == np.isfinite(b).sum() == shape[0] * (shape[0] + 1) // 2
        assert (np.isfinite(a) & np.isfinite(b)).sum() == shape[0]     # the diagonal, in both


@pytest.mark.parametrize("channels", [1, 3])
@pytest.mark.parametrize("name", tuple(bf.gather_cases()))
def test_gather(name, channels, ctx):
    """u == 0, u == w - 1, v == h - 1; a footprint with one finite pixel and one with none;
    z == far (1 + rel_tol) at 0.25 and at 0 and the double behind it; g == min_cos (skipped)
    and min_cos one double lower (counted)."""
    case = bf.gather_cases()[name]
    v, f = case["vertices"], case["faces"]
    img = bf.gather_images(channels)
    h, w = case["shape"]
    nv = len(v)
    col, cnt = np.full((nv, channels), -7.0), np.full(nv, -7, np.int32)
    z = np.full((1, h, w), -7, np.float32)
    nrm = case["normals"]
    _ffi.check(_ffi.lib().rs_surface_colorize(
        ctx.handle, _ffi.ptr(v, _f64), nv, _ffi.ptr(f, _i32), len(f), _ffi.ptr(img, _u8),
        channels, _ffi.ptr(bf.TEX_P, _f64), 1, h, w,
        _ffi.ptr(nrm, _f64) if nrm is not None else None, case["rel_tol"], case["min_cos"],
        _ffi.ptr(col, _f64), _ffi.ptr(cnt, _i32), _ffi.ptr(z, _f32)))
    rcol, rcnt, rz = tr.vertex_colors(v, f, img, bf.TEX_P, nrm, case["rel_tol"], case["min_cos"])
    dcol = float(np.abs(col - rcol).max())
    print(f"{name}, {channels} channel(s): count {cnt.tolist()}, d colour {dcol:.2e}")
    assert _same(np.nan_to_num(z, nan=9.0), np.nan_to_num(rz, nan=9.0))
    assert np.array_equal(cnt, rcnt)
    if case["count"] is not None:
        assert cnt.tolist() == case["count"]
    else:
        assert cnt[12] == (name == "cos_below")
    assert dcol <= 1e-12
    assert np.all(col[cnt == 0] == 0.0)
