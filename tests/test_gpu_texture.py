"""Mesh colouring on the GPU (surface.render_depth, surface.vertex_colors,
csrc/surface_texture.hip) against the numpy restatement tests/texture_ref.py, on the cases of
tests/texture_fixture.py.

Bars.  render_depth: the NaN mask is compared exactly -- every case asserts that no evaluated
barycentric coordinate lies within 1e-9 of zero -- and the values to one float32 ulp: the depth
is an fp64 value rounded once, and the kernel's and numpy's fp64 may differ in the last bits
before that rounding.  vertex_colors: count exactly and colours to 1e-12 (a handful of fp64
roundings on values in [0, 1]).  The restatement's gather runs on the z-buffers the GPU returned,
so the 1e-9 asserted for its visibility margin holds for the very numbers the kernel compared; the
z-buffers themselves are held to the first bar in the same test.
"""
import ctypes

import numpy as np
import pytest

import dense_fixture as df
import surface_fixture as sf
import texture_fixture as fx
import texture_ref as ref
from tsbb15_amd import _ffi, dense, surface

pytestmark = pytest.mark.gpu

MARGIN = 1e-9
S = surface.RASTER_SMALL


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.int32, 8: np.int64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def _same_bits(got, want):
    return all(x.shape == y.shape and x.dtype == y.dtype and np.array_equal(_bits(x), _bits(y))
               for x, y in zip(got, want))


def _check_depth(got, want, what):
    assert got.dtype == np.float32 and got.shape == want.shape, what
    assert np.array_equal(np.isnan(got), np.isnan(want)), what
    ok = ~np.isnan(want)
    ulp = float((np.abs(got[ok] - want[ok]) / np.spacing(np.abs(want[ok]))).max()) if ok.any() \
        else 0.0
    print(f"{what}: {int(ok.sum())} covered pixels of {ok.size}, worst {ulp:.1f} float32 ulp")
    assert ulp <= 1.0, what


def _check_render(v, f, P_cams, K, shape, ctx, what):
    """render_depth against the restatement, its margin asserted; returns the GPU's z-buffers."""
    m = {}
    want = ref.render_depth(v, f, K @ P_cams, shape, margins=m)
    assert m.get("b", 1.0) >= MARGIN, (what, m)
    got = surface.render_depth(v, f, P_cams, K, shape, ctx=ctx)
    _check_depth(got, want, what)
    return got


def _check_colors(v, f, images, cams, K, normals, ctx, what, min_cos=0.0):
    col, cnt, z = surface.vertex_colors(v, f, images, cams, K, normals=normals,
                                        rel_tol=fx.REL_TOL, min_cos=min_cos, return_depth=True,
                                        ctx=ctx)
    m, d = {}, {}
    rcol, rcnt, _ = ref.vertex_colors(v, f, images, K @ cams, normals=normals, rel_tol=fx.REL_TOL,
                                      min_cos=min_cos, depth=z, margins=m, detail=d)
    assert all(x >= MARGIN for x in m.values()), (what, m)
    ch = 1 if images.ndim == 3 else 3
    assert col.dtype == np.float64 and col.shape == (len(v), ch) and cnt.dtype == np.int32
    assert np.array_equal(cnt, rcnt), what
    dev = float(np.abs(col - rcol).max()) if len(v) else 0.0
    print(f"{what}: {int((cnt > 0).sum())} of {len(v)} vertices coloured, |dcolour| max {dev:.2e}")
    assert dev <= 1e-12, what
    assert np.all(col[cnt == 0] == 0.0) and np.all((col >= 0.0) & (col <= 1.0))
    return col, cnt, z, d


# ------------------------------------------------------------------------------------------
# parity on the fixture meshes
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", fx.CASES)
def test_render_depth_fixture(name, ctx):
    v, f, imgs, cams, K = fx.case(name)
    want, m = fx.reference_depth(name)
    assert m["b"] >= MARGIN
    got = surface.render_depth(v, f, cams, K, imgs.shape[1:3], ctx=ctx)
    _check_depth(got, want, name)
    assert not np.isnan(got).all()


@pytest.mark.parametrize("name,channels,with_normals",
                         [("fronto", 1, False), ("fronto", 3, True), ("slanted", 3, False),
                          ("slanted", 1, True), ("s16", 1, False), ("s16", 1, True),
                          ("s16", 3, False), ("s16", 3, True), ("occlusion", 1, False)])
def test_vertex_colors_fixture(name, channels, with_normals, ctx):
    v, f, imgs, cams, K = fx.case(name)
    images = imgs if channels == 1 else fx.colour_images(name)
    normals = fx.normals_of(name) if with_normals else None
    what = f"{name} ch {channels} normals {with_normals}"
    col, cnt, z, _ = _check_colors(v, f, images, cams, K, normals, ctx, what)
    _check_depth(z, fx.reference_depth(name)[0], what)
    # and so the result on the restatement's own z-buffers, whose margins the CPU test asserts
    rcol, rcnt = fx.reference_colors(name, channels, with_normals)[:2]
    assert np.array_equal(cnt, rcnt) and np.abs(col - rcol).max() <= 1e-12
    assert (cnt > 0).sum() > len(v) // 3


def test_min_cos(ctx):
    v, f, imgs, cams, K = fx.case("s16")
    _, cnt, _, d = _check_colors(v, f, imgs, cams, K, fx.normals_of("s16"), ctx, "min_cos 0.5",
                                 min_cos=0.5)
    loose = fx.reference_colors("s16", 1, True)[1]
    assert np.nanmin(d["g"]) > 0.5 and 0 < (cnt > 0).sum() < (loose > 0).sum()


# ------------------------------------------------------------------------------------------
# shapes where the kernels can go wrong
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nf", (0, 1, 63, 64, 65, 257))
def test_face_counts(nf, ctx):
    v, f, imgs, cams, K = fx.case("s16")
    got = _check_render(v, f[:nf], cams, K, fx.SPHERE_SHAPE, ctx, f"nf {nf}")
    assert np.isnan(got).all() if nf == 0 else nf == 1 or not np.isnan(got).all()


@pytest.mark.parametrize("nv", (1, 63, 64, 65, 257))
def test_vertex_counts(nv, ctx):
    """The first nv vertices with the faces among them: a mesh with holes, coloured all the same."""
    v, f, imgs, cams, K = fx.case("s16")
    sub = f[np.all(f < nv, axis=1)]
    n = fx.normals_of("s16")[:nv]
    _check_colors(v[:nv], sub, imgs, cams, K, n, ctx, f"nv {nv} with {len(sub)} faces")
    col, cnt = surface.vertex_colors(v[:nv], sub[:0], imgs, cams, K, ctx=ctx)   # no occluder
    assert col.shape == (nv, 1) and np.all(cnt == 0) and np.all(col == 0.0)


SMALL_K = np.array([[9.0, 0.0, 3.5], [0.0, 9.0, 3.5], [0.0, 0.0, 1.0]])


def _small_scene(V, h=8, w=8):
    """V cameras on the irrational spiral of the surface test's _small_scene, a 7 x 7 grid mesh on
    the slanted plane, and images of noise."""
    cams = np.array([df.camera((0.4 * np.sin(1.0 + 0.7 * k) * (k > 0),
                                0.3 * np.cos(2.0 + 1.3 * k) * (k > 0), 0.0),
                               (0.3, 1, 0), 0.04 * np.sin(0.9 * k)) for k in range(V)])
    n, c = df.SLANTED
    g = (np.arange(7) - 3.0) * np.sqrt(0.19) + np.sqrt(0.0007)
    x, y = np.meshgrid(g, g - np.sqrt(0.0011))
    v = np.stack((x.ravel(), y.ravel(), (c - n[0] * x.ravel() - n[1] * y.ravel()) / n[2]), axis=1)
    i = (np.arange(6)[:, None] * 7 + np.arange(6)[None]).ravel()
    f = np.concatenate((np.stack((i, i + 7, i + 1), axis=1),          # normals towards -z
                        np.stack((i + 1, i + 7, i + 8), axis=1))).astype(np.int32)
    imgs = np.random.RandomState(V + h + w).randint(0, 256, (V, h, w)).astype(np.uint8)
    return v, f, imgs, cams


@pytest.mark.parametrize("V", (1, 128))
def test_view_counts(V, ctx):
    v, f, imgs, cams = _small_scene(V)
    _check_render(v, f, cams, SMALL_K, (8, 8), ctx, f"V {V}")
    _, cnt, _, _ = _check_colors(v, f, imgs, cams, SMALL_K, surface.vertex_normals(v, f), ctx,
                                 f"V {V}")
    assert cnt.max() > V // 2


@pytest.mark.parametrize("shape", ((1, 1), (1, 9)))
def test_tiny_images(shape, ctx):
    h, w = shape
    v, f, imgs, cams = _small_scene(3, h, w)
    K = np.array([[9.0, 0.0, (w - 1) / 2.0 + np.sqrt(0.01)], [0.0, 9.0, np.sqrt(0.02)],
                  [0.0, 0.0, 1.0]])
    got = _check_render(v, f, cams, K, shape, ctx, f"image {shape}")
    assert not np.isnan(got[:, 0, w // 2]).any()
    # a vertex is inside an image of one row only with v == 0 exactly: nothing is coloured
    _, cnt, _, _ = _check_colors(v, f, imgs, cams, K, None, ctx, f"image {shape}")
    assert np.all(cnt == 0)


def test_faces_not_drawn(ctx):
    """A face wholly outside the image and one with a vertex behind the camera change nothing."""
    v, f, imgs, cams, K = fx.case("s16")
    base = surface.render_depth(v, f, cams[:1], K, fx.SPHERE_SHAPE, ctx=ctx)
    Minv = np.linalg.inv(K @ cams[0][:, :3])
    centre = -Minv @ (K @ cams[0][:, 3])

    def at(px, py, depth):                              # the point that view 0 sees there
        return centre + depth * (Minv @ (px, py, 1.0))

    outside = [at(70.3, 5.2, 20.0), at(90.1, 9.7, 21.0), at(80.4, 30.6, 22.0)]
    behind = [at(10.2, 10.4, 5.0), at(50.3, 12.1, 5.0), at(30.7, 40.9, -1.0)]
    v2 = np.concatenate((v, outside, behind))
    f2 = np.concatenate((f, [[len(v), len(v) + 1, len(v) + 2],
                             [len(v) + 3, len(v) + 4, len(v) + 5]])).astype(np.int32)
    assert ref.box_pixels(v2, f2[-2], K @ cams[:1], fx.SPHERE_SHAPE) == 0
    assert ref.box_pixels(v2, f2[-1], K @ cams[:1], fx.SPHERE_SHAPE) == 0
    more = surface.render_depth(v2, f2, cams[:1], K, fx.SPHERE_SHAPE, ctx=ctx)
    assert _same_bits((base,), (more,))
    # in front, the same triangle hides the sphere
    v2[-1] = at(30.7, 40.9, 5.0)
    near = _check_render(v2, f2, cams[:1], K, fx.SPHERE_SHAPE, ctx, "triangle in front")
    assert np.nanmin(near) < 5.1 < np.nanmin(base)


def test_zero_area_faces(ctx):
    """s10_zero puts vertices on nodes: its degenerate triangles have A == 0 and are skipped."""
    v, f = sf.reference_extract("s10_zero")
    A = np.linalg.norm(np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]]), axis=1)
    assert (A == 0).sum() > 0
    c = np.array(sf.SPHERES["s10_zero"][1])
    cams = np.array([fx.look_at(c + 0.6 * e, c) for e in fx.EYES])
    _check_render(v, f, cams, fx.SPHERE_K, fx.SPHERE_SHAPE, ctx, "s10_zero")


@pytest.mark.parametrize("npix", (S - 1, S, S + 1))
def test_box_at_the_threshold(npix, ctx):
    """One triangle whose clipped box holds npix pixels: the lane's walk below and at
    RS_SURFACE_RASTER_SMALL, the wave's above."""
    v, f, P, shape = fx.box_triangle(npix)
    got = _check_render(v, f, P, np.eye(3), shape, ctx, f"box of {npix}")
    assert 0 < (~np.isnan(got)).sum() < npix


def test_whole_image_triangle(ctx):
    v, f, imgs, cams, K = fx.covered_case()
    got = _check_render(v, f, cams, K, (40, 56), ctx, "covered")
    assert not np.isnan(got[0]).any()
    _check_colors(v, f, imgs, cams, K, None, ctx, "covered")


def test_list_overflow(ctx):
    """More large faces than the list holds: the rest are walked by their own lanes, and the
    z-buffer is that of the one triangle they all repeat."""
    v, f, P, shape = fx.box_triangle(S + 1)
    one = surface.render_depth(v, f, P, np.eye(3), shape, ctx=ctx)
    many = np.repeat(f, surface.TEXTURE_LIST_CAP + 65, axis=0)
    got = surface.render_depth(v, many, P, np.eye(3), shape, ctx=ctx)
    assert _same_bits((one,), (got,)) and not np.isnan(one).all()


# ------------------------------------------------------------------------------------------
# properties
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("s16", "covered"))
def test_bit_equal_variants(name, ctx):
    v, f, imgs, cams, K = fx.covered_case() if name == "covered" else fx.case(name)
    n = surface.vertex_normals(v, f)
    args = dict(normals=n, rel_tol=fx.REL_TOL, return_depth=True, ctx=ctx)
    base = surface.vertex_colors(v, f, imgs, cams, K, **args)
    again = surface.vertex_colors(v, f, imgs, cams, K, **args)
    assert _same_bits(base, again)
    perm = np.random.RandomState(5).permutation(len(f))
    assert _same_bits(base, surface.vertex_colors(v, f[perm], imgs, cams, K, **args))
    turned = cams * np.array([-1.0, 1.0, -1.0])[:len(cams), None, None]
    assert _same_bits(base, surface.vertex_colors(v, f, imgs, turned, K, **args))
    z = surface.render_depth(v, f, cams, K, imgs.shape[1:3], ctx=ctx)
    assert _same_bits((z,), (base[2],))
    assert _same_bits((z,), (surface.render_depth(v, f[perm], -cams, K, imgs.shape[1:3], ctx=ctx),))


def test_convex_body_rule(ctx):
    def colorize(v, f, imgs, cams, K):
        return surface.vertex_colors(v, f, imgs, cams, K, rel_tol=fx.REL_TOL, ctx=ctx)

    back, front, judged = fx.convex_body(fx.visible_per_view(colorize))
    print("convex body: visible back", back, "hidden front", front, "judged", judged)
    assert back == 0 and front == 0 and judged >= 0.70


@pytest.mark.parametrize("name", sf.SCENES)
def test_affine_image_and_plane_depth(name, ctx):
    v, f, _, cams, K = fx.case(name)
    col, cnt, z, d = _check_colors(v, f, fx.affine_images(name), cams, K, fx.normals_of(name), ctx,
                                   f"affine {name}")
    ok = cnt > 0
    assert ok.sum() > len(v) // 2
    assert np.abs(col[ok, 0] - fx.affine_colour(d)[ok]).max() <= 1e-12
    err, covered = fx.plane_depth_error(z, name)
    print(name, "z-buffer against the exact depth:", err, "voxel on", covered, "pixels")
    assert covered > 600 and err <= 1.0


def test_occlusion_scene(ctx):
    v, f, imgs, cams, K = fx.case("occlusion")
    col, cnt = surface.vertex_colors(v, f, imgs, cams, K, rel_tol=fx.REL_TOL, ctx=ctx)
    seen, shadow = fx.views_named(col, cnt), fx.shadowed()
    assert shadow.sum() > 50 and not np.any(seen & shadow)
    assert seen[~shadow.any(axis=1)].sum() > 0


# ------------------------------------------------------------------------------------------
# arguments, timing, reconstruct
# ------------------------------------------------------------------------------------------
def test_argument_errors(ctx):
    v, f, imgs, cams, K = fx.case("s16")
    shape = fx.SPHERE_SHAPE
    bad_face = np.array(f)
    bad_face[7, 1] = len(v)
    neg_face = np.array(f)
    neg_face[0, 0] = -1
    flat = np.array(cams)
    flat[1][:, 0] = 0.0                                 # a zero column: det exactly 0
    f = np.ascontiguousarray(f, dtype=np.int32)
    nan = np.array(cams)
    nan[0, 0, 0] = np.nan
    many = np.repeat(cams[:1], 129, axis=0)
    for args in ((v, bad_face, cams, K, shape), (v, neg_face, cams, K, shape),
                 (v, f, flat, K, shape), (v, f, nan, K, shape), (v, f, many, K, shape),
                 (v, f, cams, K, (0, 8)), (v, f, cams, K, (8, 16385)), (v, f, cams, K, (8193, 8193)),
                 (v[:, :2], f, cams, K, shape), (v, f[:, :2], cams, K, shape),
                 (v, f.astype(np.float64), cams, K, shape)):
        with pytest.raises(ValueError):
            surface.render_depth(*args, ctx=ctx)
    for kw in (dict(faces=bad_face), dict(cams=flat), dict(images=imgs.astype(np.float32)),
               dict(images=imgs[:2]), dict(images=np.repeat(imgs[..., None], 2, axis=3)),
               dict(normals=np.zeros((len(v) - 1, 3))), dict(rel_tol=-0.1), dict(rel_tol=np.nan),
               dict(min_cos=np.inf)):
        a = dict(vertices=v, faces=f, images=imgs, cams=cams, K=K)
        a.update(kw)
        with pytest.raises(ValueError):
            surface.vertex_colors(ctx=ctx, **a)
    # the ABI itself: indices and cameras are checked there too, and nothing is written
    P = np.ascontiguousarray(K @ flat)
    out = np.full((3,) + shape, -7.0, np.float32)
    f64, i32, f32 = ctypes.c_double, ctypes.c_int32, ctypes.c_float
    lib = _ffi.lib()
    st = lib.rs_surface_render_depth(ctx.handle, _ffi.ptr(v, f64), len(v), _ffi.ptr(f, i32),
                                     len(f), _ffi.ptr(P, f64), 3, shape[0], shape[1],
                                     _ffi.ptr(out, f32))
    assert st == _ffi.RS_EINVAL
    P = np.ascontiguousarray(K @ cams)
    st2 = lib.rs_surface_render_depth(ctx.handle, _ffi.ptr(v, f64), len(v),
                                      _ffi.ptr(bad_face, i32), len(f), _ffi.ptr(P, f64), 3,
                                      shape[0], shape[1], _ffi.ptr(out, f32))
    st3 = lib.rs_surface_render_depth(ctx.handle, _ffi.ptr(v, f64), len(v), _ffi.ptr(f, i32),
                                      (2**31 - 1) // 3 + 1, _ffi.ptr(P, f64), 3, shape[0],
                                      shape[1], _ffi.ptr(out, f32))
    st4 = lib.rs_surface_render_depth(ctx.handle, _ffi.ptr(v, f64), 2**31, _ffi.ptr(f, i32),
                                      len(f), _ffi.ptr(P, f64), 3, shape[0], shape[1],
                                      _ffi.ptr(out, f32))
    assert st2 == st3 == st4 == _ffi.RS_EINVAL and np.all(out == -7.0)


def test_texture_timing_slots():
    """Slots are -1 before a timed call and positive after it; render_depth leaves the gather's
    slot alone, surface.timing sees nothing, and a context destroyed with the timer on is clean."""
    v, f, imgs, cams, K = fx.case("s16")
    own = _ffi.Context()
    try:
        plain = surface.vertex_colors(v, f, imgs, cams, K, return_depth=True, ctx=own)
        assert surface.texture_timing(1, ctx=own) == dict.fromkeys(surface.TEXTURE_STAGES, -1.0)
        z = surface.render_depth(v, f, cams, K, fx.SPHERE_SHAPE, ctx=own)
        ms = surface.texture_timing(1, ctx=own)
        assert 0.0 < ms["raster_small"] < 1e3 and 0.0 < ms["raster_large"] < 1e3
        assert ms["gather"] == -1.0
        timed = surface.vertex_colors(v, f, imgs, cams, K, return_depth=True, ctx=own)
        ms2 = surface.texture_timing(1, ctx=own)
        print(ms2)
        assert all(np.isfinite(ms2[k]) and 0.0 < ms2[k] < 1e3 for k in surface.TEXTURE_STAGES)
        assert surface.timing(0, ctx=own) == dict.fromkeys(surface.STAGES, -1.0)
        assert _same_bits(plain, timed) and _same_bits((z,), (timed[2],))
    finally:
        own.close()                                     # with the timer still on


def test_reconstruct_colors(ctx):
    imgs, cams, _ = df.scene("slanted")
    args = (imgs, cams, df.K, df.DEPTHS, sf.ORIGIN, sf.VOXEL, sf.DIMS, sf.TRUNC)
    plain = surface.reconstruct(*args, min_weight=2, ctx=ctx)
    out = surface.reconstruct(*args, min_weight=2, ctx=ctx, colors=True)
    assert len(plain) == 4 and len(out) == 5 and _same_bits(plain, out[:4])
    v, f = out[:2]
    col = surface.vertex_colors(v, f, imgs, cams, df.K, normals=surface.vertex_normals(v, f),
                                ctx=ctx)[0]
    assert _same_bits((out[4],), (col,))
    assert col.shape == (len(v), 1) and (col > 0).mean() > 0.5
    print(f"reconstruct: {len(v)} vertices, {int((col[:, 0] > 0).sum())} coloured")
