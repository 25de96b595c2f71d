"""tests/texture_ref.py, the numpy restatement of the mesh-colouring definitions, tested alone on
the cases of tests/texture_fixture.py: the margins that let tests/test_gpu_texture.py compare
masks and counts exactly, and the properties that make the definitions worth restating.  No GPU.
"""
import numpy as np
import pytest

import surface_fixture as sf
import texture_fixture as fx
import texture_ref as ref

MARGIN = 1e-9


@pytest.mark.parametrize("name", fx.CASES)
def test_margins(name):
    _, m = fx.reference_depth(name)
    print(name, "depth", m)
    assert m["b"] >= MARGIN, m
    for channels, with_normals in ((1, False), (1, True)):
        if with_normals and name == "occlusion":
            continue
        _, cnt, m, _ = fx.reference_colors(name, channels, with_normals)
        print(name, "normals" if with_normals else "plain", m, "coloured", int((cnt > 0).sum()),
              "of", len(cnt))
        assert m["inside"] >= MARGIN and m["visible"] >= MARGIN, m
        if with_normals:
            assert m["cos"] >= MARGIN, m
        assert (cnt > 0).sum() > len(cnt) // 3


def test_constants_match_the_header():
    import re
    from tsbb15_amd import _ffi, surface
    src = open(_ffi.HEADER_PATH).read()
    small = re.search(r"#define RS_SURFACE_RASTER_SMALL (\d+)", src)
    cap = re.search(r"#define RS_SURFACE_TEXTURE_LIST_CAP \(1 << (\d+)\)", src)
    slots = re.search(r"#define RS_SURFACE_TEXTURE_TIMING_SLOTS (\d+)", src)
    assert int(small.group(1)) == surface.RASTER_SMALL
    assert 1 << int(cap.group(1)) == surface.TEXTURE_LIST_CAP
    assert int(slots.group(1)) == len(surface.TEXTURE_STAGES)


def test_box_triangles_and_covered_case_margins():
    from tsbb15_amd import surface
    for npix in (surface.RASTER_SMALL - 1, surface.RASTER_SMALL, surface.RASTER_SMALL + 1):
        v, f, P, shape = fx.box_triangle(npix)
        m = {}
        z = ref.render_depth(v, f, P, shape, margins=m)
        assert m["b"] >= MARGIN and 0 < (~np.isnan(z)).sum() < npix
    v, f, _, cams, K = fx.covered_case()
    m = {}
    z = ref.render_depth(v, f, K @ cams, (40, 56), margins=m)
    assert m["b"] >= MARGIN
    assert not np.isnan(z[0]).any()                       # the big triangle covers view 0
    plain = fx.reference_depth("fronto")[0][0]
    mesh = ~np.isnan(plain)
    nearer = z[0][mesh] < plain[mesh]
    assert 0.2 < nearer.mean() < 0.8                      # in front of the mesh here, behind there


@pytest.mark.parametrize("name", ("fronto", "s16"))
def test_face_order_does_not_matter(name):
    v, f, imgs, cams, K = fx.case(name)
    perm = np.random.RandomState(3).permutation(len(f))
    z = ref.render_depth(v, f[perm], K @ cams, imgs.shape[1:3])
    assert np.array_equal(z.view(np.int32), fx.reference_depth(name)[0].view(np.int32))


def test_negated_cameras_change_nothing():
    v, f, imgs, cams, K = fx.case("slanted")
    z = ref.render_depth(v, f, K @ -cams, imgs.shape[1:3])
    assert np.array_equal(z.view(np.int32), fx.reference_depth("slanted")[0].view(np.int32))


@pytest.mark.parametrize("name", sf.SCENES)
def test_plane_depth(name):
    err, covered = fx.plane_depth_error(fx.reference_depth(name)[0], name)
    print(name, "z-buffer against the exact depth:", err, "voxel on", covered, "pixels")
    assert covered > 600 and err <= 1.0      # the fixture volume fills a part of each image


def test_convex_body_rule():
    def colorize(v, f, imgs, cams, K):
        return ref.vertex_colors(v, f, imgs, K @ cams, rel_tol=fx.REL_TOL)

    back, front, judged = fx.convex_body(fx.visible_per_view(colorize))
    print("convex body: visible back", back, "hidden front", front, "judged", judged)
    assert back == 0 and front == 0 and judged >= 0.70


@pytest.mark.parametrize("name", sf.SCENES)
def test_affine_image(name):
    v, f, _, cams, K = fx.case(name)
    d = {}
    col, cnt, _ = ref.vertex_colors(v, f, fx.affine_images(name), K @ cams,
                                    normals=fx.normals_of(name), rel_tol=fx.REL_TOL,
                                    depth=fx.reference_depth(name)[0], detail=d)
    assert np.array_equal(cnt, fx.reference_colors(name, 1, True)[1])
    want = fx.affine_colour(d)
    ok = cnt > 0
    assert ok.sum() > len(cnt) // 2
    assert np.abs(col[ok, 0] - want[ok]).max() <= 1e-12


def test_occlusion_scene():
    col, cnt, _, _ = fx.reference_colors("occlusion")
    seen = fx.views_named(col, cnt)
    shadow = fx.shadowed()
    print("occlusion: shadowed vertex-views", int(shadow.sum()))
    assert shadow.sum() > 50 and not np.any(seen & shadow)
    assert seen[~shadow.any(axis=1)].sum() > 0
