"""Meshes, cameras and images for the mesh-colouring tests.  A case is (vertices, faces, images,
cams, K); every reference result is computed once by tests/texture_ref.py, cached and read-only.

  fronto, slanted   surface_fixture.reference_mesh with dense_fixture.scene's cameras and images
  s16               the 16^3 sphere's mesh, three look-at cameras at 48 x 64, focal length 90
  occlusion         the same sphere and cameras with a plane mesh behind it; view v's image is the
                    constant 40 + 20 v, so colour x count names the views that saw a vertex
Camera positions have irrational components: no pixel centre lies on an edge and no vertex on a
decision's boundary (tests/test_texture_cpu.py asserts 1e-9 for every margin).
"""
import functools

import numpy as np

import dense_fixture as df
import surface_fixture as sf
import texture_ref as ref

CASES = ("fronto", "slanted", "s16", "occlusion")
SPHERE_SHAPE = (48, 64)
SPHERE_K = np.array([[90.0, 0.0, 31.5], [0.0, 90.0, 23.5], [0.0, 0.0, 1.0]])
SPHERE_CENTRE = np.array(sf.SPHERES["s16"][1])
SPHERE_R = sf.SPHERES["s16"][2]
# where the three cameras stand, seen from the sphere's centre; all in front of the plane below
EYES = np.array([[-np.sqrt(95.0), np.sqrt(61.0), -np.sqrt(402.0)],
                 [np.sqrt(249.0), np.sqrt(22.0), -np.sqrt(546.0)],
                 [np.sqrt(2.0), -np.sqrt(129.0), -np.sqrt(566.0)]])
PLANE_Z = SPHERE_CENTRE[2] + np.sqrt(75.0)
PLANE_N, PLANE_STEP = 30, np.sqrt(0.83)
REL_TOL = 0.01


def _freeze(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def look_at(eye, target):
    """[R | -R eye] with the optical axis through `target` and the image's y axis down."""
    fwd = (target - eye) / np.linalg.norm(target - eye)
    right = np.cross(fwd, (0.0, -1.0, 0.0))
    right /= np.linalg.norm(right)
    R = np.array([right, np.cross(fwd, right), fwd])
    return np.hstack((R, (-R @ eye)[:, None]))


def sphere_cameras():
    return np.array([look_at(SPHERE_CENTRE + e, SPHERE_CENTRE) for e in EYES])


def grid_plane():
    """A PLANE_N x PLANE_N grid of vertices at z = PLANE_Z, two triangles a square."""
    k = (np.arange(PLANE_N) - (PLANE_N - 1) / 2.0) * PLANE_STEP
    x, y = np.meshgrid(SPHERE_CENTRE[0] + k + np.sqrt(0.002), SPHERE_CENTRE[1] + k - np.sqrt(0.003))
    v = np.stack((x.ravel(), y.ravel(), np.full(x.size, PLANE_Z)), axis=1)
    i = (np.arange(PLANE_N - 1)[:, None] * PLANE_N + np.arange(PLANE_N - 1)[None]).ravel()
    f = np.concatenate((np.stack((i, i + 1, i + PLANE_N), axis=1),
                        np.stack((i + 1, i + PLANE_N + 1, i + PLANE_N), axis=1)))
    return v, f.astype(np.int32)


def sphere_images(cams, shape, channels):
    """Smooth synthetic images: sinusoids of the pixel coordinates, a phase per view and channel."""
    h, w = shape
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    out = np.empty((len(cams), h, w, channels), np.uint8)
    for v in range(len(cams)):
        for c in range(channels):
            out[v, :, :, c] = np.rint(128 + 60 * np.sin(0.31 * x + 0.7 * v + c) +
                                      50 * np.cos(0.23 * y - 0.4 * v + 2 * c))
    return out[..., 0] if channels == 1 else out


@functools.lru_cache(maxsize=None)
def case(name):
    """(vertices, faces, grey images, cams, K)."""
    if name in sf.SCENES:
        imgs, cams, _ = df.scene(name)
        v, f = sf.reference_mesh(name)
        return v, f, imgs, cams, df.K
    sv, sfaces = sf.reference_extract("s16")
    cams = sphere_cameras()
    if name == "s16":
        return _freeze(sv, sfaces, sphere_images(cams, SPHERE_SHAPE, 1), cams, SPHERE_K)
    pv, pf = grid_plane()
    v = np.concatenate((sv, pv))
    f = np.concatenate((sfaces, pf + len(sv))).astype(np.int32)
    imgs = np.empty((3,) + SPHERE_SHAPE, np.uint8)
    for k in range(3):
        imgs[k] = 40 + 20 * k
    return _freeze(v, f, imgs, cams, SPHERE_K)


def shape_of(name):
    return case(name)[2].shape[1:3]


def projections(name):
    v, f, imgs, cams, K = case(name)
    return K @ cams


@functools.lru_cache(maxsize=None)
def colour_images(name):
    """Three-channel images of a case's size."""
    _, _, imgs, cams, _ = case(name)
    return _freeze(sphere_images(cams, imgs.shape[1:3], 3))[0]


@functools.lru_cache(maxsize=None)
def affine_images(name):
    """I(x, y) = 2 x + 3 y + 10 in every view; the plane cases' 40 x 56 keeps it below 256."""
    _, _, imgs, _, _ = case(name)
    V, h, w = imgs.shape
    assert 2 * (w - 1) + 3 * (h - 1) + 10 <= 255
    y, x = np.mgrid[0:h, 0:w]
    return _freeze(np.repeat((2 * x + 3 * y + 10).astype(np.uint8)[None], V, axis=0))[0]


def normals_of(name):
    from tsbb15_amd import surface
    v, f = case(name)[:2]
    return surface.vertex_normals(v, f)


@functools.lru_cache(maxsize=None)
def reference_depth(name):
    """(z-buffers, margins) of a case."""
    v, f, imgs, _, _ = case(name)
    m = {}
    z = ref.render_depth(v, f, projections(name), imgs.shape[1:3], margins=m)
    z.setflags(write=False)
    return z, m


@functools.lru_cache(maxsize=None)
def reference_colors(name, channels=1, with_normals=False):
    """(colors, count, margins, detail) of a case on the restatement's own z-buffers."""
    v, f, imgs, _, _ = case(name)
    images = imgs if channels == 1 else colour_images(name)
    m, d = {}, {}
    col, cnt, _ = ref.vertex_colors(v, f, images, projections(name),
                                    normals=normals_of(name) if with_normals else None,
                                    rel_tol=REL_TOL, depth=reference_depth(name)[0], margins=m,
                                    detail=d)
    _freeze(col, cnt)
    return col, cnt, m, d


def convex_body(count_per_view_visible, name="s16"):
    """The convex-body rule's three figures for a (Nv, V) bool array "vertex i was visible in
    view v": (visible among c <= -0.25, hidden among c >= 0.25, the judged share)."""
    v, f, _, cams, K = case(name)
    n = normals_of(name)
    _, centres = ref.turn(K @ cams)
    wrong_back = wrong_front = judged = 0
    for k, c in enumerate(centres):
        d = c - v
        cos = np.sum(n * d, axis=1) / np.linalg.norm(d, axis=1)
        vis = count_per_view_visible[:, k]
        wrong_back += int(np.sum(vis & (cos <= -0.25)))
        wrong_front += int(np.sum(~vis & (cos >= 0.25)))
        judged += int(np.sum(np.abs(cos) >= 0.25))
    return wrong_back, wrong_front, judged / (len(v) * len(centres))


def visible_per_view(colorize, name="s16"):
    """(Nv, V) bool from V single-view calls of `colorize(vertices, faces, images, cams, K)`,
    which returns (colors, count, ...): count of a single view is its visibility."""
    v, f, imgs, cams, K = case(name)
    return np.stack([colorize(v, f, imgs[k:k + 1], cams[k:k + 1], K)[1] > 0
                     for k in range(len(cams))], axis=1)


def plane_depth_error(zbuf, name):
    """|z-buffer - exact plane depth| on covered pixels, in VOXEL."""
    _, cams, exact = df.scene(name)
    ok = ~np.isnan(zbuf)
    return float(np.abs(zbuf[ok].astype(np.float64) - exact[ok]).max() / sf.VOXEL), int(ok.sum())


def shadowed(name="occlusion"):
    """(Nv, V) bool: plane vertices whose ray to camera v passes within r - 1 voxel of the
    sphere's centre."""
    v, _, _, cams, K = case(name)
    _, centres = ref.turn(K @ cams)
    ns = len(sf.reference_extract("s16")[0])
    out = np.zeros((len(v), len(centres)), bool)
    for k, c in enumerate(centres):
        d = v - c
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        m = SPHERE_CENTRE - c
        dist = np.linalg.norm(m - (d @ m)[:, None] * d, axis=1)
        out[ns:, k] = dist[ns:] <= SPHERE_R - 1.0
    return out


def affine_colour(detail):
    """sum g (2 u + 3 v + 10) / (255 sum g) over the contributing views; NaN where there is none."""
    g = np.where(np.isnan(detail["g"]), 0.0, detail["g"])
    s = np.where(g != 0.0, 2.0 * detail["u"] + 3.0 * detail["v"] + 10.0, 0.0)
    with np.errstate(invalid="ignore"):
        return (g * s).sum(axis=1) / (255.0 * g.sum(axis=1))


def views_named(colors, count):
    """(Nv, V) bool from the occlusion scene's colours: with the constant images 40, 60 and 80
    and weight 1, colour x count x 255 is the sum over the views that saw the vertex, and the
    eight subsets have different sums."""
    total = np.rint(colors[:, 0] * count * 255.0).astype(int)
    table = {sum(40 + 20 * k for k in range(3) if s >> k & 1): s for s in range(8)}
    assert len(table) == 8 and all(t in table for t in total), set(total) - set(table)
    sets = np.array([table[t] for t in total])
    assert np.array_equal([bin(s).count("1") for s in sets], count)
    return np.stack([(sets >> k & 1).astype(bool) for k in range(3)], axis=1)


def box_triangle(npix):
    """(vertices, faces, P, shape): one triangle in front of the camera [I | 0] whose clipped
    bounding box holds exactly `npix` pixels, as bw x bh with the divisor pair nearest a square."""
    bh = max(d for d in range(1, int(np.sqrt(npix)) + 1) if npix % d == 0)
    bw = npix // bh
    h, w = bh + 7, bw + 7
    K = np.array([[50.0, 0.0, (w - 1) / 2.0], [0.0, 50.0, (h - 1) / 2.0], [0.0, 0.0, 1.0]])
    x0, y0 = 2.0 + np.sqrt(0.2), 2.0 + np.sqrt(0.3)          # the box starts at pixel (3, 3)
    px = np.array([[x0, y0, 1.0], [x0 + bw - np.sqrt(0.1), y0 + np.sqrt(0.01), 1.0],
                   [x0 + np.sqrt(0.02), y0 + bh - np.sqrt(0.15), 1.0]])
    depth = np.array([3.0, np.sqrt(11.0), np.sqrt(13.0)])
    vertices = (np.linalg.inv(K) @ px.T).T * depth[:, None]
    P = K @ np.hstack((np.eye(3), np.zeros((3, 1))))
    faces = np.array([[0, 1, 2]], np.int32)
    assert ref.box_pixels(vertices, faces[0], P, (h, w)) == npix
    return vertices, faces, P[None], (h, w)


@functools.lru_cache(maxsize=None)
def covered_case():
    """The fronto mesh with one triangle over the whole 40 x 56 image laid across it: nearer than
    the plane at one corner, farther at the other two."""
    v, f, imgs, cams, K = case("fronto")
    px = np.array([[-70.0 - np.sqrt(2.0), -5.0, 1.0], [60.0, 130.0 + np.sqrt(3.0), 1.0],
                   [120.0 + np.sqrt(5.0), -9.0, 1.0]])
    depth = np.array([np.sqrt(6.0), np.sqrt(50.0), np.sqrt(60.0)])
    big = (np.linalg.inv(K) @ px.T).T * depth[:, None]     # camera 0 is [I | 0]
    v2 = np.concatenate((v, big))
    f2 = np.concatenate((f, [[len(v), len(v) + 1, len(v) + 2]])).astype(np.int32)
    return _freeze(v2, f2, imgs, cams, K)
