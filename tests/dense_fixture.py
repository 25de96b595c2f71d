"""Procedural scenes for the dense stage: a textured plane n . X = c seen by a few cameras.

The texture is a sum of sinusoids over the plane's own 2-D coordinates, and every view is
rendered by exact ray-plane intersection per pixel (no resampling of another image), then
quantised to uint8.  Everything is deterministic; nothing is read from disk.
"""
import functools

import numpy as np

H, W = 40, 56
K = np.array([[60.0, 0.0, 27.5], [0.0, 60.0, 19.5], [0.0, 0.0, 1.0]])
INV_DEPTHS = 0.375 - 0.025 * np.arange(12)           # 0.375, 0.35, ..., 0.1
DEPTHS = 1.0 / INV_DEPTHS                             # depth 4.0 is index 5
TRUE_INDEX = 5
MIN_VAR = 4.0
FRONTO = (np.array([0.0, 0.0, 1.0]), 4.0)
SLANTED = (np.array([0.35, 0.1, 1.0]) / np.linalg.norm([0.35, 0.1, 1.0]), 4.0)
N_SINUSOIDS, MAX_FREQ, AMPLITUDE = 24, 22.0, 40.0


def rodrigues(axis, angle):
    a = np.asarray(axis, dtype=np.float64)
    a = a / np.linalg.norm(a)
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * Kx + (1 - np.cos(angle)) * (Kx @ Kx)


def camera(centre, axis=(0, 1, 0), angle=0.0):
    """[R | -R centre] with R the rotation by `angle` about `axis` (world to camera)."""
    R = rodrigues(axis, angle)
    return np.hstack((R, (-R @ np.asarray(centre, dtype=np.float64))[:, None]))


def cameras():
    """The base scene's reference view and its two sources."""
    return np.array([camera((0, 0, 0)),
                     camera((0.5, 0.03, 0.0), (0, 1, 0), -0.06),
                     camera((-0.45, -0.06, 0.05), (0.2, 1, 0), 0.05)])


def turned_away(centre=(0.1, 0.0, 0.0)):
    """A camera that looks along -z: every sample of the scene lies behind it."""
    return camera(centre, (0, 1, 0), np.pi)


def _texture(s, t, seed):
    rs = np.random.RandomState(seed)
    f = rs.uniform(-MAX_FREQ, MAX_FREQ, (N_SINUSOIDS, 2))
    ph = rs.uniform(0, 2 * np.pi, N_SINUSOIDS)
    acc = np.zeros_like(s)
    for (fs, ft), p in zip(f, ph):
        acc += np.sin(fs * s + ft * t + p)
    return 128.0 + AMPLITUDE * acc / np.sqrt(N_SINUSOIDS / 2.0)


def render(cam, plane, h=H, w=W, Kmat=K, seed=0):
    """The uint8 image of the textured plane in camera `cam`; (image, depth) with depth the
    exact cam[2] . [X; 1] of every pixel's plane point (NaN where the ray misses)."""
    n, c = plane
    P = Kmat @ cam
    Minv = np.linalg.inv(P[:, :3])
    centre = -Minv @ P[:, 3]
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    rays = np.stack((x, y, np.ones_like(x)), axis=-1) @ Minv.T          # X = centre + lam ray
    with np.errstate(divide="ignore", invalid="ignore"):
        lam = (c - n @ centre) / (rays @ n)
    X = centre + lam[..., None] * rays
    e1 = np.cross(n, (0.0, 1.0, 0.0))
    e1 /= np.linalg.norm(e1)
    e2 = np.cross(n, e1)
    img = _texture(X @ e1, X @ e2, seed)
    depth = X @ cam[2, :3] + cam[2, 3]
    hit = np.isfinite(lam) & (lam > 0)
    img = np.where(hit, np.clip(np.rint(img), 0, 255), 0).astype(np.uint8)
    return img, np.where(hit, depth, np.nan)


@functools.lru_cache(maxsize=None)
def scene(name="fronto", h=H, w=W, n_views=3):
    """(images (V, h, w) uint8, cams (V, 3, 4), true depth (V, h, w)) of a named plane; view 0
    is the reference camera [I | 0].  Cached: treat the arrays as read-only."""
    plane = {"fronto": FRONTO, "slanted": SLANTED}[name]
    cams = cameras()[:n_views]
    out = [render(C, plane, h, w) for C in cams]
    imgs, depth = np.array([o[0] for o in out]), np.array([o[1] for o in out])
    for a in (imgs, cams, depth):
        a.setflags(write=False)
    return imgs, cams, depth


def true_index(depth):
    """The (fractional) position of a true depth in DEPTHS' uniform 1 / depth ladder."""
    return (INV_DEPTHS[0] - 1.0 / depth) / 0.025


def interior(h, w, patch, inset=4):
    """Pixels at least `inset` px inside the border of valid windows."""
    m = np.zeros((h, w), bool)
    r = patch // 2 + inset
    m[r:h - r, r:w - r] = True
    return m


# ------------------------------------------------------------------------------------------
# The sweeps the GPU test runs.  A case is (ref image, ref cam, source images, source cams, K,
# depths, patch); tests/test_dense_cpu.py measures the fp32 bar and the margins on these very
# cases.
# ------------------------------------------------------------------------------------------
CASE_NAMES = ("fronto_p3", "fronto_p5", "fronto_p7", "slanted_p3", "slanted_p5", "slanted_p7",
              "slanted_p11", "odd_p5", "odd_p9_D33", "odd_D1", "odd_D2_S1", "odd_S8", "tiny_p11")


def _k_for(h, w):
    return np.array([[60.0, 0.0, (w - 1) / 2.0], [0.0, 60.0, (h - 1) / 2.0], [0.0, 0.0, 1.0]])


def _views(plane, cams, h, w, Kmat):
    return np.array([render(C, plane, h, w, Kmat)[0] for C in cams])


@functools.lru_cache(maxsize=None)
def sweep_cases():
    cases = {}
    for name in ("fronto", "slanted"):
        imgs, cams, _ = scene(name)
        for patch in (3, 5, 7):
            cases[f"{name}_p{patch}"] = (imgs[0], cams[0], imgs[1:], cams[1:], K, DEPTHS, patch)
    imgs, cams, _ = scene("slanted")
    cases["slanted_p11"] = (imgs[0], cams[0], imgs[1:], cams[1:], K, DEPTHS, 11)

    # 37 x 53: no multiple of the 32 x 8 tile; D = 1, 2, 33; S = 1; patch 9
    h, w = 37, 53
    Ko = _k_for(h, w)
    cams = cameras()
    io = _views(SLANTED, cams, h, w, Ko)
    d33 = 1.0 / np.linspace(0.4, 0.1, 33)
    cases["odd_p5"] = (io[0], cams[0], io[1:], cams[1:], Ko, DEPTHS, 5)
    cases["odd_p9_D33"] = (io[0], cams[0], io[1:], cams[1:], Ko, d33, 9)
    cases["odd_D1"] = (io[0], cams[0], io[1:], cams[1:], Ko, DEPTHS[5:6], 5)
    cases["odd_D2_S1"] = (io[0], cams[0], io[1:2], cams[1:2], Ko, DEPTHS[4:6], 7)

    # S = 8: three sources are turned away, every sample of theirs is invalid
    extra = [camera((0.3, -0.2, 0.0), (1, 0, 0), 0.04), camera((-0.25, 0.25, -0.05)),
             camera((0.0, -0.35, 0.02), (1, 0.3, 0), 0.07)]
    c8 = np.array([cams[1], turned_away(), cams[2], extra[0], turned_away((0.0, 0.2, 0.0)),
                   extra[1], turned_away((-0.3, 0.0, 0.1)), extra[2]])
    cases["odd_S8"] = (io[0], cams[0], _views(SLANTED, c8, h, w, Ko), c8, Ko, DEPTHS, 5)

    # 12 x 12 with patch 11: four window centres; each source shifts by under a pixel in one
    # diagonal direction, so each centre keeps exactly the sources whose shift suits it
    h = w = 12
    Ks = _k_for(h, w)
    c4 = np.array([camera((sx * 0.03, sy * 0.02, 0.0)) for sx in (1, -1) for sy in (1, -1)])
    ref = camera((0, 0, 0))
    cases["tiny_p11"] = (render(ref, FRONTO, h, w, Ks)[0], ref, _views(FRONTO, c4, h, w, Ks), c4,
                         Ks, DEPTHS, 11)
    assert tuple(cases) == CASE_NAMES
    return cases


@functools.lru_cache(maxsize=None)
def reference_sweeps():
    """name -> (index, delta, score, nvalid, volume, per-hypothesis source counts) of
    tests/dense_ref.py in fp64, computed once and shared; read-only."""
    import dense_ref
    out = {}
    for name, (ref, rc, srcs, sc, Kmat, depths, patch) in sweep_cases().items():
        res = dense_ref.plane_sweep(ref, rc, srcs, sc, Kmat, depths, patch, MIN_VAR, counts=True)
        for a in res:
            a.setflags(write=False)
        out[name] = res
    return out


@functools.lru_cache(maxsize=None)
def fp32_deviation():
    """name -> (largest |cost(fp32, window sums reversed) - cost(fp64)|, validity flags equal)
    over the case's whole volume, from the restatement alone."""
    import dense_ref
    out = {}
    for name, (ref, rc, srcs, sc, Kmat, depths, patch) in sweep_cases().items():
        v64 = reference_sweeps()[name][4]
        A, b = dense_ref.plane_warps(rc, sc, Kmat)
        v32, _ = dense_ref.cost_volume(ref, srcs, A, b, depths, patch, MIN_VAR, np.float32, True)
        same = np.array_equal(np.isnan(v32), np.isnan(v64))
        both = ~np.isnan(v64) & ~np.isnan(v32)
        dev = float(np.abs(v32[both].astype(np.float64) - v64[both]).max()) if both.any() else 0.0
        out[name] = (dev, same)
    return out


def score_bar():
    """SCORE_BAR: 8 x the largest fp32-reversed against fp64 cost deviation over every case the
    GPU test runs; the factor covers the kernel's own summation order and FMA contraction."""
    return 8.0 * max(dev for dev, _ in fp32_deviation().values())


@functools.lru_cache(maxsize=None)
def reference_depth_maps(name="slanted"):
    """Every view of a scene swept as the reference view against the other two by the
    restatement, refined: (index (V, h, w), delta, depth (V, h, w), volumes)."""
    import dense_ref
    imgs, cams, _ = scene(name)
    idx, dl, dep, vol = [], [], [], []
    for i in range(len(cams)):
        nb = [j for j in range(len(cams)) if j != i]
        r = dense_ref.plane_sweep(imgs[i], cams[i], imgs[nb], cams[nb], K, DEPTHS, 7, MIN_VAR)
        idx.append(r[0])
        dl.append(r[1])
        dep.append(dense_ref.refine_depth(r[0], r[1], DEPTHS))
        vol.append(r[4])
    out = tuple(np.array(a) for a in (idx, dl, dep, vol))
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def consistency_case():
    """(depth maps (4, h, w), cams (4, 3, 4)): the slanted scene's three refined maps, the first
    with a NaN hole, and a fourth view that is turned away and has no depth at all."""
    _, cams, _ = scene("slanted")
    depth = np.array(reference_depth_maps("slanted")[2])
    depth[0, 15:22, 20:31] = np.nan
    depth = np.concatenate((depth, np.full((1,) + depth.shape[1:], np.nan)))
    # (a centre of (0.1, 0, 0) would put view 0's pixels of depth 4 on exact half-integers)
    cams = np.concatenate((cams, turned_away((0.11, 0.013, 0.0))[None]))
    depth.setflags(write=False)
    cams.setflags(write=False)
    return depth, cams
