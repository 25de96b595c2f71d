"""The surface stage on the GPU (tsbb15_amd.surface, csrc/surface.hip) against the numpy
restatement tests/surface_ref.py, on the volumes of tests/surface_fixture.py.

Bars.  integrate: the NaN pattern and the weight are compared exactly -- tests/test_surface_cpu.py
(and _margins here, for the small scenes) assert that no projection lies within 1e-9 px of a
rounding boundary and no sample within 1e-9 of the truncation test -- and |dtsdf| <= 2^-23: the
value lies in [-1, 1] and the fp64 quotient may round to the neighbouring float32.  extract:
faces are equal exactly, vertices agree in number and order and to 1e-12 x the volume's largest
absolute coordinate (a handful of fp64 roundings and FMA contraction).

SCAN_CHUNK is the number of nodes one workgroup of the scans takes (RS_SURFACE_SCAN_CHUNK).  A
(2, 2, n) volume has 4 n nodes, so no such volume has 2047 or 2049 of them; the volumes used
are the nearest ones: 2044 (the last chunk is 4 short), 2048 (exactly one chunk), 2052 (4 nodes
spill into a second chunk) and 4100 (a third chunk is begun).
"""
import ctypes

import numpy as np
import pytest

import dense_fixture as df
import surface_fixture as fx
import surface_ref as ref
from tsbb15_amd import _ffi, dense, surface

pytestmark = pytest.mark.gpu

SCAN_CHUNK = 2048
TSDF_BAR = 2.0 ** -23


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a.view(np.int64) \
        if a.dtype == np.float64 else a


def _same_bits(got, want):
    return all(x.shape == y.shape and x.dtype == y.dtype and np.array_equal(_bits(x), _bits(y))
               for x, y in zip(got, want))


def _check_volume(got, want, what):
    tsdf, weight = got
    rtsdf, rweight = want
    assert tsdf.dtype == weight.dtype == np.float32 and tsdf.shape == rtsdf.shape
    assert np.array_equal(np.isnan(tsdf), np.isnan(rtsdf)), what
    assert np.array_equal(weight, rweight), what
    assert np.array_equal(np.isnan(tsdf), weight == 0), what
    ok = ~np.isnan(rtsdf)
    dev = float(np.abs(tsdf[ok].astype(np.float64) - rtsdf[ok]).max()) if ok.any() else 0.0
    print(f"{what}: |dtsdf| max {dev:.3e}, observed nodes {int(ok.sum())} of {ok.size}")
    assert dev <= TSDF_BAR, what
    if ok.any():
        assert np.abs(tsdf[ok]).max() <= 1.0


def _check_mesh(got, want, scale, what):
    v, f = got
    rv, rf = want
    assert v.dtype == np.float64 and f.dtype == np.int32
    assert v.ndim == 2 and v.shape[1] == 3 and f.ndim == 2 and f.shape[1] == 3
    assert np.array_equal(f, rf), what
    assert v.shape == rv.shape, what
    dev = float(np.abs(v - rv).max()) if len(v) else 0.0
    print(f"{what}: {len(v)} vertices, {len(f)} faces, |dX| max {dev:.3e}, bar {1e-12 * scale:.3e}")
    assert dev <= 1e-12 * scale, what


def _scale(origin, voxel, dims):
    far = np.asarray(origin) + voxel * (np.array(dims[::-1]) - 1)
    return float(max(np.abs(origin).max(), np.abs(far).max()))


# ------------------------------------------------------------------------------------------
# integrate
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", fx.SCENES)
def test_integrate_fixture(name, ctx):
    _, cams, depth = df.scene(name)
    got = surface.integrate(depth, cams, df.K, fx.ORIGIN, fx.VOXEL, fx.DIMS, fx.TRUNC, ctx=ctx)
    _check_volume(got, fx.reference_volume(name)[:2], name)


def test_integrate_weight_map(ctx):
    """dense.consistency's counts as the weight: pixels nobody agrees with drop out."""
    _, cams, depth = df.scene("slanted")
    depth = np.array(depth)
    depth[1, 10:20, 10:30] *= 1.05                    # view 1 disagrees there
    w = dense.consistency(depth, cams, df.K, rel_tol=0.01, ctx=ctx).astype(np.float32)
    assert 0.0 in w and 2.0 in w
    m = {}
    want = ref.integrate(depth, cams, df.K, fx.ORIGIN, fx.VOXEL, fx.DIMS, fx.TRUNC, weights=w,
                         margins=m)
    assert m["round"] >= 1e-9 and m["trunc"] >= 1e-9, m
    got = surface.integrate(depth, cams, df.K, fx.ORIGIN, fx.VOXEL, fx.DIMS, fx.TRUNC, weights=w,
                            ctx=ctx)
    _check_volume(got, want, "weight map")


SMALL_K = np.array([[9.0, 0.0, 3.5], [0.0, 9.0, 3.5], [0.0, 0.0, 1.0]])
SMALL_ORIGIN = np.array([-np.sqrt(0.1), -np.sqrt(0.002), np.sqrt(18.0)])   # the plane crosses it
SMALL_VOXEL = fx.VOXEL / 4.0
SMALL_TRUNC = 0.2


def _small_scene(V):
    """V views of 8 x 8 pixels of the slanted plane with exact depths; the views beyond the
    first stand on an irrational spiral around it."""
    cams = np.array([df.camera((0.4 * np.sin(1.0 + 0.7 * v) * (v > 0),
                                0.3 * np.cos(2.0 + 1.3 * v) * (v > 0), 0.0),
                               (0.3, 1, 0), 0.04 * np.sin(0.9 * v)) for v in range(V)])
    depth = np.array([df.render(C, df.SLANTED, 8, 8, SMALL_K)[1] for C in cams])
    return cams, depth


@pytest.mark.parametrize("V", (1, 128))
@pytest.mark.parametrize("dims", ((1, 1, 1), (2, 2, 2), (2, 3, 63), (2, 3, 64), (2, 3, 65),
                                  (3, 2, 257)))
def test_integrate_size_boundaries(dims, V, ctx):
    cams, depth = _small_scene(V)
    m = {}
    want = ref.integrate(depth, cams, SMALL_K, SMALL_ORIGIN, SMALL_VOXEL, dims, SMALL_TRUNC,
                         margins=m)
    assert m["round"] >= 1e-9 and m["trunc"] >= 1e-9, m
    assert want[1].max() > 0
    got = surface.integrate(depth, cams, SMALL_K, SMALL_ORIGIN, SMALL_VOXEL, dims, SMALL_TRUNC,
                            ctx=ctx)
    _check_volume(got, want, f"dims {dims} V {V}")


def test_integrate_negated_scene(ctx):
    _, cams, depth = df.scene("slanted")
    pos = surface.integrate(depth, cams, df.K, fx.ORIGIN, fx.VOXEL, fx.DIMS, fx.TRUNC, ctx=ctx)
    neg = surface.integrate(-depth, -cams, df.K, fx.ORIGIN, fx.VOXEL, fx.DIMS, fx.TRUNC, ctx=ctx)
    assert _same_bits(pos, neg)


def test_integrate_no_contribution(ctx):
    """A camera turned away, an all-NaN map and a view of zero weight add nothing; nodes nobody
    observes have weight 0 and tsdf NaN."""
    _, cams, depth = df.scene("slanted")
    base = surface.integrate(depth, cams, df.K, fx.ORIGIN, fx.VOXEL, fx.DIMS, fx.TRUNC, ctx=ctx)
    away = df.turned_away((0.11, 0.013, 0.0))
    cams5 = np.concatenate((cams, away[None], cams[:1]))
    depth5 = np.concatenate((depth, np.full_like(depth[:1], 4.0), np.full_like(depth[:1], np.nan)))
    more = surface.integrate(depth5, cams5, df.K, fx.ORIGIN, fx.VOXEL, fx.DIMS, fx.TRUNC, ctx=ctx)
    assert _same_bits(base, more)
    w = np.ones(depth5.shape, np.float32)
    w[4] = 0.0
    depth5[4] = depth[0]
    more = surface.integrate(depth5, cams5, df.K, fx.ORIGIN, fx.VOXEL, fx.DIMS, fx.TRUNC,
                             weights=w, ctx=ctx)
    assert _same_bits(base, more)

    none = surface.integrate(depth5[3:4], cams5[3:4], df.K, fx.ORIGIN, fx.VOXEL, fx.DIMS, fx.TRUNC,
                             ctx=ctx)
    assert np.all(none[1] == 0) and np.all(np.isnan(none[0]))
    tsdf, weight = base
    assert np.any(weight == 0) and np.array_equal(weight == 0, np.isnan(tsdf))


def test_integrate_split_calls(ctx):
    _, cams, depth = df.scene("slanted")
    args = (df.K, fx.ORIGIN, fx.VOXEL, fx.DIMS, fx.TRUNC)
    one = surface.integrate(depth, cams, *args, ctx=ctx)
    first = surface.integrate(depth[:2], cams[:2], *args, ctx=ctx)
    kept = (first[0].copy(), first[1].copy())
    two = surface.integrate(depth[2:], cams[2:], *args, tsdf=first[0], weight=first[1], ctx=ctx)
    assert _same_bits(first, kept)                      # the running volume is not modified
    assert np.array_equal(two[1], one[1])
    assert np.array_equal(np.isnan(two[0]), np.isnan(one[0]))
    # The definition stores the first call's T0 as float32, 0.5 ulp(T0) off, and that error
    # reaches T scaled by W0 / W <= 1; each result adds 0.5 ulp of its own.  Where the third
    # view cancels the first two, T is far smaller than T0 and the ulp of T itself says nothing
    # (the fp64 restatement alone differs by 7 such ulp on this scene).  The 2 ulp are
    # therefore those of the largest magnitude involved: the prior or the result.
    ok = ~np.isnan(one[0])
    prior = np.where(np.isnan(first[0]), 0.0, first[0])[ok]
    big = np.maximum(np.maximum(np.abs(one[0][ok]), np.abs(two[0][ok])), np.abs(prior))
    worst = float((np.abs(two[0][ok].astype(np.float64) - one[0][ok]) / np.spacing(big)).max())
    print("split calls: worst difference", worst, "ulp")
    assert worst <= 2.0
    # and against the restatement given the same prior
    want = ref.integrate(depth[2:], cams[2:], *args, tsdf=first[0], weight=first[1])
    _check_volume(two, want, "second call")


def test_integrate_reproducible(ctx):
    _, cams, depth = df.scene("fronto")
    a = surface.integrate(depth, cams, df.K, fx.ORIGIN, fx.VOXEL, fx.DIMS, fx.TRUNC, ctx=ctx)
    b = surface.integrate(depth, cams, df.K, fx.ORIGIN, fx.VOXEL, fx.DIMS, fx.TRUNC, ctx=ctx)
    assert _same_bits(a, b)


# ------------------------------------------------------------------------------------------
# extract
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", fx.SCENES)
def test_extract_fixture(name, ctx):
    """The volume as the GPU's own integrate made it."""
    _, cams, depth = df.scene(name)
    tsdf, weight = surface.integrate(depth, cams, df.K, fx.ORIGIN, fx.VOXEL, fx.DIMS, fx.TRUNC,
                                     ctx=ctx)
    got = surface.extract(tsdf, weight, fx.ORIGIN, fx.VOXEL, fx.MIN_WEIGHT, ctx=ctx)
    want = ref.extract(tsdf, weight, fx.ORIGIN, fx.VOXEL, fx.MIN_WEIGHT)
    _check_mesh(got, want, _scale(fx.ORIGIN, fx.VOXEL, fx.DIMS), name)
    assert len(got[0]) > 2000
    assert fx.plane_distance(got[0], name).max() <= 0.5 * fx.VOXEL
    again = surface.extract(tsdf, weight, fx.ORIGIN, fx.VOXEL, fx.MIN_WEIGHT, ctx=ctx)
    assert _same_bits(got, again)


@pytest.mark.parametrize("name", tuple(fx.SPHERES) + ("random",))
def test_extract_analytic(name, ctx):
    tsdf, weight, origin, voxel, mw = fx.extract_cases()[name]
    got = surface.extract(tsdf, weight, origin, voxel, mw, ctx=ctx)
    _check_mesh(got, fx.reference_extract(name), _scale(origin, voxel, tsdf.shape), name)


@pytest.mark.parametrize("name", tuple(fx.SPHERES))
def test_extract_sphere_mesh(name, ctx):
    """The properties of the mesh, on the GPU's own output."""
    tsdf, weight, origin, voxel, mw = fx.extract_cases()[name]
    v, f = surface.extract(tsdf, weight, origin, voxel, mw, ctx=ctx)
    assert ref.is_closed(f)
    assert ref.euler(v, f) == 2
    assert ref.signed_volume(v, f) > 0
    err, bound = fx.sphere_radial_error(v, name).max(), ref.sphere_bound(fx.SPHERES[name][2])
    print(name, err, bound)
    assert err <= bound


@pytest.mark.parametrize("n", (SCAN_CHUNK // 4 - 1, SCAN_CHUNK // 4, SCAN_CHUNK // 4 + 1,
                               2 * SCAN_CHUNK // 4 + 1))
def test_extract_scan_chunks(n, ctx):
    rs = np.random.RandomState(n)
    tsdf = rs.uniform(-1.0, 1.0, (2, 2, n)).astype(np.float32)
    weight = (rs.uniform(0.0, 1.0, (2, 2, n)) < 0.97).astype(np.float32)
    origin = np.array([0.3, -0.7, 1.1])
    got = surface.extract(tsdf, weight, origin, 0.01, 1.0, ctx=ctx)
    want = ref.extract(tsdf, weight, origin, 0.01, 1.0)
    assert len(want[1]) > n // 2
    _check_mesh(got, want, _scale(origin, 0.01, tsdf.shape), f"{4 * n} nodes")


def test_extract_empty_and_single_cell(ctx):
    one = np.ones((3, 4, 5), np.float32)

    def empty(m):
        v, f = m
        return v.shape == (0, 3) and v.dtype == np.float64 and f.shape == (0, 3) and \
            f.dtype == np.int32

    assert empty(surface.extract(one, one, np.zeros(3), 1.0, 1.0, ctx=ctx))        # all positive
    neg = one.copy()
    neg[1, 1, 1:3] = -1.0
    assert empty(surface.extract(neg, one, np.zeros(3), 1.0, 2.0, ctx=ctx))        # underweight
    assert empty(surface.extract(np.full((1, 1, 1), -1, np.float32), np.ones((1, 1, 1), np.float32),
                                 np.zeros(3), 1.0, 1.0, ctx=ctx))                  # no cell
    # one valid cell; its corner 000 is negative and lies in all six tets: six triangles on the
    # seven edges that leave it
    tsdf = np.ones((2, 2, 2), np.float32)
    tsdf[0, 0, 0] = -1.0
    v, f = surface.extract(tsdf, np.ones((2, 2, 2), np.float32), np.zeros(3), 1.0, 1.0, ctx=ctx)
    assert len(v) == 7 and len(f) == 6
    _check_mesh((v, f), ref.extract(tsdf, np.ones((2, 2, 2), np.float32), np.zeros(3), 1.0, 1.0),
                1.0, "corner 000")
    # corner 100 lies in two tets (x first): two triangles
    tsdf = np.ones((2, 2, 2), np.float32)
    tsdf[0, 0, 1] = -1.0
    w = np.ones((2, 2, 2), np.float32)
    got = surface.extract(tsdf, w, np.zeros(3), 1.0, 1.0, ctx=ctx)
    _check_mesh(got, ref.extract(tsdf, w, np.zeros(3), 1.0, 1.0), 1.0, "corner 100")
    assert len(got[1]) == 2
    # the same cell with one node underweight: no valid cell, no mesh
    w[1, 1, 1] = 0.0
    assert empty(surface.extract(tsdf, w, np.zeros(3), 1.0, 1.0, ctx=ctx))


def test_extract_capacity_too_small(ctx):
    """The ABI itself: RS_EINVAL, the right counts, and arrays nobody wrote to."""
    tsdf, weight, origin, voxel, mw = fx.extract_cases()["s12"]
    rv, rf = fx.reference_extract("s12")
    origin = np.ascontiguousarray(origin, dtype=np.float64)
    f32, f64, i32 = ctypes.c_float, ctypes.c_double, ctypes.c_int32
    for vcap, fcap in ((len(rv) - 1, len(rf)), (len(rv), len(rf) - 1), (0, 0)):
        v = np.full((max(vcap, 1), 3), -7.0)
        f = np.full((max(fcap, 1), 3), -7, np.int32)
        nv, nf = ctypes.c_int64(-1), ctypes.c_int64(-1)
        st = _ffi.lib().rs_surface_extract(
            ctx.handle, _ffi.ptr(tsdf, f32), _ffi.ptr(weight, f32), 12, 12, 12,
            _ffi.ptr(origin, f64), voxel, mw, _ffi.ptr(v, f64), vcap, _ffi.ptr(f, i32), fcap,
            ctypes.byref(nv), ctypes.byref(nf))
        assert st == _ffi.RS_EINVAL
        assert (nv.value, nf.value) == (len(rv), len(rf))
        assert np.all(v == -7.0) and np.all(f == -7)
    with pytest.raises(ValueError):
        _ffi.check(st)


def test_timing_slots():
    """Slots are -1 before a timed call and positive after it; a context destroyed with the
    timer on is clean.  A context of its own, so that no earlier call has timed."""
    _, cams, depth = df.scene("slanted")
    own = _ffi.Context()
    try:
        plain = surface.integrate(depth, cams, df.K, fx.ORIGIN, fx.VOXEL, fx.DIMS, fx.TRUNC, ctx=own)
        plain_m = surface.extract(*plain, fx.ORIGIN, fx.VOXEL, fx.MIN_WEIGHT, ctx=own)
        assert surface.timing(1, ctx=own) == dict.fromkeys(surface.STAGES, -1.0)
        timed = surface.integrate(depth, cams, df.K, fx.ORIGIN, fx.VOXEL, fx.DIMS, fx.TRUNC, ctx=own)
        ms = surface.timing(1, ctx=own)
        assert 0.0 < ms["integrate"] < 1e3
        assert ms["classify"] == ms["scan"] == ms["emit"] == -1.0
        timed_m = surface.extract(*timed, fx.ORIGIN, fx.VOXEL, fx.MIN_WEIGHT, ctx=own)
        ms2 = surface.timing(1, ctx=own)
        print(ms2)
        assert all(np.isfinite(ms2[k]) and 0.0 < ms2[k] < 1e3 for k in surface.STAGES)
        assert ms2["integrate"] == ms["integrate"]
        assert _same_bits(plain, timed) and _same_bits(plain_m, timed_m)
    finally:
        own.close()                                     # with the timer still on


# ------------------------------------------------------------------------------------------
# reconstruct
# ------------------------------------------------------------------------------------------
def test_reconstruct(ctx):
    imgs, cams, _ = df.scene("slanted")
    v, f, tsdf, weight = surface.reconstruct(imgs, cams, df.K, df.DEPTHS, fx.ORIGIN, fx.VOXEL,
                                             fx.DIMS, fx.TRUNC, min_weight=2, ctx=ctx)
    assert len(v) > 0 and len(f) > 0
    maps = dense.fuse(imgs, cams, df.K, df.DEPTHS, return_maps=True, ctx=ctx)[-1]
    depth = np.where(maps["keep"], maps["depth"], np.nan)
    t2, w2 = surface.integrate(depth, cams, df.K, fx.ORIGIN, fx.VOXEL, fx.DIMS, fx.TRUNC,
                               weights=maps["count"].astype(np.float32), ctx=ctx)
    v2, f2 = surface.extract(t2, w2, fx.ORIGIN, fx.VOXEL, min_weight=2, ctx=ctx)
    assert _same_bits((v, f, tsdf, weight), (v2, f2, t2, w2))
    dist = fx.plane_distance(v, "slanted") / fx.VOXEL
    print(f"reconstruct: {len(v)} vertices, {len(f)} faces, vertex distance to the plane: "
          f"median {np.median(dist):.3f}, max {dist.max():.3f} voxel")
