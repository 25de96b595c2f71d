"""Cases for the global registration: hand-placed clouds that put the descriptor's bins, the
pseudo-angle's branches, the matcher's tiles and the RANSAC's gates on their edges, and the
"egg", a closed mesh without a symmetry, whose samples are moved off it by poses of 60 to 180
degrees.  The restatement (tests/global_ref.py) runs once per case, cached and read-only.
"""
import functools

import numpy as np

import global_ref as ref
import register_fixture as rf

# ---- the egg ------------------------------------------------------------------------------------
# The blob of tests/register_fixture.py is nearly symmetric under a half turn about z: its radius
# holds cos(2 ph) and a weak cos(3 ph).  The egg adds a term that is odd under that turn, a bulge
# to one side, and a dent.
EGG_DIVISIONS = (20, 40)
SCALE = 1.3
TRANSLATION = np.array([2.0, -1.5, 1.0])
POSES = (((1.0, 0.0, 0.0), 60.0), ((0.0, 1.0, 0.0), 90.0), ((0.0, 0.0, 1.0), 120.0),
         ((1.0, 1.0, 0.0), 150.0), ((1.0, -2.0, 3.0), 180.0), ((-1.0, 1.0, 1.0), 100.0))
SAMPLES, OUTLIERS, NOISE_SIGMA = 2000, 400, 0.02     # 400 / 2 000: 20 % outliers
CLOUD_NAMES = ("clean", "outlier", "noisy")
KEEP = {"clean": 0.75, "outlier": 0.75, "noisy": 0.75}
K = 32
H = 100000
CANDIDATES = 8
BASIN_DEG = 20.0          # the basin register is tested for


def _egg_point(th, ph):
    r = (1.0 + 0.25 * np.sin(th) ** 2 * np.cos(2.0 * ph + 0.4)
         + 0.2 * np.cos(th) * np.sin(th) * np.sin(ph) + 0.15 * np.sin(th) ** 3 * np.cos(3.0 * ph)
         + 0.3 * np.sin(th) ** 2 * np.cos(ph - 0.7)
         - 0.25 * np.exp(-4.0 * ((th - 1.0) ** 2 + (np.sin(0.5 * (ph - 4.0))) ** 2)))
    x = r * np.sin(th) * np.cos(ph)
    y = 0.8 * r * np.sin(th) * np.sin(ph)
    z = 0.6 * r * np.cos(th) + 0.1 * r * np.sin(th) * np.cos(ph)
    return 5.0 * np.stack([x, y, z], axis=-1) + np.array([3.0, -2.0, 7.0])


@functools.lru_cache(maxsize=None)
def egg():
    """(vertices (762, 3), faces (1520, 3) int32), the blob's connectivity."""
    nt, nph = EGG_DIVISIONS
    th = np.pi * np.arange(1, nt) / nt
    ph = 2.0 * np.pi * np.arange(nph) / nph
    ring = _egg_point(th[:, None], ph[None, :]).reshape(-1, 3)
    v = np.concatenate((_egg_point(np.array(0.0), np.array(0.0))[None],
                        _egg_point(np.array(np.pi), np.array(0.0))[None], ring))
    assert rf.BLOB_DIVISIONS == EGG_DIVISIONS
    return rf._freeze(v, rf.blob()[1])


def truth(pose):
    axis, degrees = POSES[pose]
    return SCALE, rf.rotation(axis, degrees), TRANSLATION


def back(points, pose):
    s, R, t = truth(pose)
    return (np.asarray(points) - t) @ R / s


@functools.lru_cache(maxsize=None)
def _on_mesh():
    from tsbb15_amd import evaluation as ev
    v, f = egg()
    on, face = ev.sample_surface(v, f, SAMPLES, seed=7)
    nrm = ref.face_normals(v, f)[face]
    lo, hi = v.min(axis=0), v.max(axis=0)
    mid, half = (lo + hi) / 2.0, (hi - lo) / 2.0
    rs = np.random.RandomState(11)
    out = mid + 1.25 * half * rs.uniform(-1.0, 1.0, (OUTLIERS, 3))
    on_out = rs.standard_normal((OUTLIERS, 3))
    on_out /= np.sqrt((on_out * on_out).sum(axis=1))[:, None]
    noise = NOISE_SIGMA * np.random.RandomState(13).standard_normal(on.shape)
    return {"clean": (on, nrm), "outlier": (np.concatenate((on, out)), np.concatenate((nrm, on_out))),
            "noisy": (on + noise, nrm)}


@functools.lru_cache(maxsize=None)
def cloud(name, pose):
    """(points, normals) of a cloud in its own frame: the samples moved back through the pose."""
    p, nrm = _on_mesh()[name]
    _, R, _ = truth(pose)
    return rf._freeze(back(p, pose), nrm @ R)


@functools.lru_cache(maxsize=None)
def target_of(n, seed=0):
    """(samples, their descriptors): what global_register makes of the mesh for a cloud of n
    points (2 000, and 2 400 for the cloud with outliers)."""
    from tsbb15_amd import evaluation as ev
    v, f = egg()
    pts, face = ev.sample_surface(v, f, n, seed)
    return rf._freeze(pts, ref.fpfh(pts, ref.face_normals(v, f)[face], K)[0])


@functools.lru_cache(maxsize=None)
def coarse(name, pose, verify=True):
    """The restatement's coarse stage on a cloud."""
    v, f = egg()
    pts, nrm = cloud(name, pose)
    tgt, tf = target_of(len(pts))
    return ref.coarse(pts, nrm, v, f, tgt, tf, k=K, H=H, candidates=CANDIDATES, keep=KEEP[name],
                      verify=verify)


def rotation_angle_deg(A, B):
    """The angle of A B^T from its skew part and its trace, atan2(|w|, (tr - 1) / 2): the arc
    cosine of the trace alone cannot tell an angle below sqrt(2 eps) = 1.2e-6 degrees from 0."""
    M = np.asarray(A, dtype=np.float64) @ np.asarray(B, dtype=np.float64).T
    w = 0.5 * np.array([M[2, 1] - M[1, 2], M[0, 2] - M[2, 0], M[1, 0] - M[0, 1]])
    return float(np.degrees(np.arctan2(np.sqrt((w * w).sum()), 0.5 * (np.trace(M) - 1.0))))


def pose_errors(s, R, t, pose):
    """(rotation error in degrees, |s / s_true - 1|, |t - t_true| / the mesh's diagonal)."""
    ts, tR, tt = truth(pose)
    L = ref.register_ref.mesh_box(*egg())[1]
    return (rotation_angle_deg(R, tR), abs(s / ts - 1.0),
            float(np.linalg.norm(np.asarray(t) - tt)) / L)


# What the noise allows.  A point-to-plane fit of z = (omega, u, sigma), p -> p + omega x p + u +
# sigma p in the mesh's frame, to residuals of standard deviation sigma_n along the normals has
# the covariance sigma_n^2 (J^T J)^-1 with the rows J = [p x n, n, p . n].  The loop keeps the
# fraction ``keep`` of the smallest residuals; an estimator that rejects beyond c has the
# asymptotic variance E[r^2; |r| < c] / P(|r| < c and its boundary terms)^2, which for a normal
# residual and keep = 0.75 (c = 1.1503 sigma_n) is sigma_n^2 / (0.75 - 2 c phi(c)) =
# 3.62 sigma_n^2.  The pose (s, R, t) = (1 + sigma)(1 + [omega]x)(s, R, t)_true + (0, 0, u), so
# t - t_true = u + omega x t_true + sigma t_true.  The bars are NOISY_SIGMAS standard errors.
TRIM_VARIANCE = 1.0 / (0.75 - 2.0 * 1.1503 * np.exp(-0.5 * 1.1503 ** 2) / np.sqrt(2.0 * np.pi))
NOISY_SIGMAS = 5.0


@functools.lru_cache(maxsize=None)
def noisy_bars(pose):
    """(rotation in degrees, |s / s_true - 1|, |t - t_true| / L) that NOISY_SIGMAS standard
    errors of the trimmed point-to-plane fit allow on the noisy cloud."""
    p, n = _on_mesh()["clean"]
    J = np.concatenate((np.cross(p, n), n, (p * n).sum(axis=1)[:, None]), axis=1)
    C = TRIM_VARIANCE * NOISE_SIGMA ** 2 * np.linalg.inv(J.T @ J)
    t = truth(pose)[2]
    A = np.concatenate((-np.array([[0.0, -t[2], t[1]], [t[2], 0.0, -t[0]], [-t[1], t[0], 0.0]]),
                        np.eye(3), t[:, None]), axis=1)
    L = ref.register_ref.mesh_box(*egg())[1]
    return (NOISY_SIGMAS * float(np.degrees(np.sqrt(np.trace(C[:3, :3])))),
            NOISY_SIGMAS * float(np.sqrt(C[6, 6])),
            NOISY_SIGMAS * float(np.sqrt(np.trace(A @ C @ A.T))) / L)


# ---- descriptors: small clouds --------------------------------------------------------------
def _unit(rs, n):
    v = rs.standard_normal((n, 3))
    return v / np.sqrt((v * v).sum(axis=1))[:, None]


def _pairs(rows):
    """A cloud of isolated pairs for k = 1: pair m stands at x = 100 m, point 2 m at the origin of
    the pair with normal n_i, point 2 m + 1 at offset d with normal n_j."""
    pts, nrm = [], []
    for m, (d, ni, nj) in enumerate(rows):
        o = np.array([100.0 * m, 0.0, 0.0])
        pts += [o, o + np.asarray(d, dtype=np.float64)]
        nrm += [np.asarray(ni, dtype=np.float64), np.asarray(nj, dtype=np.float64)]
    return np.array(pts), np.array(nrm)


EDGES = tuple(k / 5.5 - 1.0 for k in range(0, 12))       # f with (f + 1) 5.5 on an integer
TINY = 2.0 ** -30                                         # 1 + TINY^2 rounds to 1
# (x, y) on the axes, on the diagonals of each branch, at the branches' joints and at zero
ANGLES = ((1.0, 0.0), (0.0, 1.0), (-1.0, 0.0), (0.0, -1.0), (0.0, 0.0), (-0.0, 1.0), (-0.0, -1.0),
          (-1.0, -0.0), (1.0, 1.0), (-1.0, 1.0), (-1.0, -1.0), (1.0, -1.0), (3.0, 1.0),
          (-3.0, 1.0), (-3.0, -1.0), (3.0, -1.0), (-1e-300, -1.0), (-1.0, -1e-300),
          (1e-300, 1e300), (-2.0 ** -60, -1.0)) + tuple(
              (4.0 - k, float(k)) for k in range(1, 4)) + tuple(
              (-float(k), 8.0 / 11.0 * k) for k in range(1, 4))


@functools.lru_cache(maxsize=None)
def fpfh_cases():
    """name -> (points, normals, k)."""
    c = {}
    for n, k in ((1, 4), (2, 4), (3, 4), (3, 1), (20, 32), (33, 32), (63, 8), (64, 8), (65, 8),
                 (300, 16), (300, 63)):
        rs = np.random.RandomState(1000 * n + k)
        c[f"random_{n}_k{k}"] = (rs.uniform(-1.0, 1.0, (n, 3)) * (3.0, 2.0, 1.0), _unit(rs, n), k)
    rs = np.random.RandomState(5)
    p, nr = rs.uniform(-1.0, 1.0, (40, 3)), _unit(rs, 40)
    p[7] = p[3]
    p[8] = p[3]
    p[21] = p[20]
    c["duplicates"] = (p.copy(), nr.copy(), 5)
    c["all_one_point"] = (np.tile(p[:1], (6, 1)), nr[:6].copy(), 3)
    # neighbours straight along the normal: c = d x n_i = 0, the pair is skipped on that side
    q = np.array([[0.0, 0.0, 0.0], [0.0, 0.0, 1.0], [0.0, 0.0, -2.0], [1.0, 0.0, 0.5],
                  [0.0, 3.0, 0.0]])
    c["along_the_normal"] = (q, np.tile([[0.0, 0.0, 1.0]], (5, 1)), 4)
    c["only_along_the_normal"] = (q[:3].copy(), np.tile([[0.0, 0.0, 2.0]], (3, 1)), 2)
    bad = nr.copy()
    bad[4] = np.nan
    bad[9, 1] = np.inf
    bad[30] = (np.nan, 0.0, 1.0)
    c["nan_normals"] = (p.copy(), bad, 6)
    holes = p.copy()
    holes[2] = np.nan
    holes[11, 0] = np.inf
    c["nan_points"] = (holes, nr.copy(), 6)
    c["nan_everything"] = (np.full((5, 3), np.nan), nr[:5].copy(), 2)
    z = (0.0, 0.0, 1.0)
    rows = [((1.0, 0.0, 0.0), z, (0.0, -1.0, 0.0)),          # f1 = 1, f2 = 0
            ((1.0, 0.0, 0.0), z, (0.0, 1.0, 0.0)),           # f1 = -1
            ((1.0, 0.0, 0.0), z, (1.0, 0.0, 0.0)),           # f1 = 0
            ((TINY, 0.0, 1.0), z, (0.0, -1.0, 0.0)),         # f2 = 1: sqrt(1 + 2^-60) = 1
            ((TINY, 0.0, -1.0), z, (0.0, -1.0, 0.0))]        # f2 = -1
    rows += [((1.0, 0.0, 0.0), z, (0.0, -f, 0.5)) for f in EDGES]           # f1 on an edge
    rows += [((1.0, 0.0, 0.0), z, (0.0, -np.nextafter(f, -2.0), 0.5)) for f in EDGES]
    rows += [((TINY, 0.0, 1.0), (0.0, 0.0, f), (0.0, -1.0, 0.0)) for f in EDGES]   # f2 = f
    rows += [((TINY, 0.0, 1.0), (0.0, 0.0, np.nextafter(f, 2.0)), (0.0, -1.0, 0.0)) for f in EDGES]
    c["bin_edges"] = _pairs(rows) + (1,)
    # u = z, d = x: v = (0, -1, 0), w = u x v = (1, 0, 0), so n_j = (y, 0, x)
    c["angles"] = _pairs([((1.0, 0.0, 0.0), z, (y, 0.0, x)) for x, y in ANGLES]) + (1,)
    for case in c.values():
        rf._freeze(case[0], case[1])
    return c


FPFH_NAMES = ("random_1_k4", "random_2_k4", "random_3_k4", "random_3_k1", "random_20_k32",
              "random_33_k32", "random_63_k8", "random_64_k8", "random_65_k8", "random_300_k16",
              "random_300_k63", "duplicates", "all_one_point", "along_the_normal",
              "only_along_the_normal", "nan_normals", "nan_points", "nan_everything", "bin_edges",
              "angles")


@functools.lru_cache(maxsize=None)
def fpfh_want(name):
    p, nr, k = fpfh_cases()[name]
    return rf._freeze(*ref.fpfh(p, nr, k))


@functools.lru_cache(maxsize=None)
def dyadic_cloud():
    """(points, normals, moved points, moved normals, k): coordinates on a grid of 1 / 64, a
    quarter turn about y with a mirror-free sign pattern, a scale of 4 and a dyadic shift: every
    product and sum of the descriptor is exact or scales by a power of two."""
    rs = np.random.RandomState(77)
    p = rs.randint(-512, 513, (150, 3)) / 64.0
    nr = rs.randint(-8, 9, (150, 3)) / 8.0
    nr[(nr == 0.0).all(axis=1)] = (0.0, 0.0, 1.0)
    R = np.array([[0.0, 0.0, 1.0], [0.0, 1.0, 0.0], [-1.0, 0.0, 0.0]])
    return rf._freeze(p, nr, 4.0 * p @ R.T + np.array([3.5, -20.0, 0.25]), nr @ R.T) + (12,)


# ---- matching ---------------------------------------------------------------------------------
MATCH_SIZES = ((1, 1), (1, ref.TILE + 1), (63, 65), (64, 64), (65, 63), (ref.TILE - 1, ref.TILE + 1),
               (ref.TILE, ref.TILE), (ref.TILE + 1, ref.TILE - 1), (300, 2 * ref.TILE + 5))
MATCH_DIMS = (1, 8, 9, 16, 17, 33, 36, 37, 64)       # 33 the descriptor; 8, 16, 36, 64 the kernels'


@functools.lru_cache(maxsize=None)
def match_case(n, m, D, kind="random"):
    """(fa, fb).  ``ties``: small integers, so that many d2 are exactly equal; ``nan``: NaN rows
    on both sides and an infinite entry."""
    rs = np.random.RandomState(n * 1000003 + m * 1009 + D)
    if kind == "ties":
        fa, fb = (rs.randint(0, 2, (n, D)).astype(np.float64),
                  rs.randint(0, 2, (m, D)).astype(np.float64))
        fb[(m + 1) // 2:] = fb[:m // 2]         # the rows of the first half once more
    else:
        fa, fb = rs.uniform(0.0, 2.0, (n, D)), rs.uniform(0.0, 2.0, (m, D))
    if kind == "nan":
        fa[::7, rs.randint(D)] = np.nan
        fb[::5, rs.randint(D)] = np.nan
        fb[1 % m, D - 1] = np.inf
    return rf._freeze(fa, fb)


# ---- RANSAC -----------------------------------------------------------------------------------
def _planted(M, inliers, seed, sigma=0.0):
    rs = np.random.RandomState(seed)
    src = rs.uniform(-2.0, 2.0, (M, 3))
    s, R, t = 1.3, rf.rotation((1.0, -2.0, 0.5), 140.0), np.array([0.5, 2.0, -1.0])
    dst = rs.uniform(-3.0, 3.0, (M, 3))
    good = rs.permutation(M)[:inliers]
    dst[good] = s * src[good] @ R.T + t + sigma * rs.standard_normal((inliers, 3))
    return src, dst


@functools.lru_cache(maxsize=None)
def ransac_cases():
    """name -> dict(src, dst, H, inlier_dist, and keywords of ransac_similarity)."""
    c = {}
    for M in (3, 4, 63, 64, 65):
        src, dst = _planted(M, max(3, M // 2), 100 + M, sigma=0.01)
        for H in (1, 64, 65, 4097):
            c[f"sizes_M{M}_H{H}"] = dict(src=src, dst=dst, H=H, inlier_dist=0.05, seed=M + H,
                                         edge_tol=0.5)
    src, dst = _planted(200, 20, 7)
    c["planted"] = dict(src=src, dst=dst, H=20000, inlier_dist=1e-9, seed=3, scale=(0.5, 2.0))
    c["planted_rigid_gate"] = dict(src=src, dst=dst, H=4097, inlier_dist=0.5, seed=3,
                                   with_scale=False, edge_tol=0.4)
    src1, dst1 = _planted(120, 60, 9)
    dst1 = (dst1 - np.array([0.5, 2.0, -1.0])) / 1.3          # the same rotation, no scale
    c["rigid"] = dict(src=src1, dst=dst1 + 0.25, H=4097, inlier_dist=1e-9, seed=5,
                      with_scale=False, edge_tol=0.01)
    c["all_gated_out"] = dict(src=src, dst=dst, H=4097, inlier_dist=0.1, seed=1, min_edge=100.0)
    c["scale_gate_empty"] = dict(src=src, dst=dst, H=4097, inlier_dist=0.1, seed=1,
                                 scale=(50.0, 60.0), edge_tol=10.0)
    rep = dst.copy()
    rep[::3] = rep[0]
    rep[1::3] = rep[1]
    c["repeated_dst"] = dict(src=src, dst=rep, H=4097, inlier_dist=0.3, seed=2, edge_tol=0.6)
    # an exact frame: R = 1, s = 1, t = 0 from the first three; the fourth lies (3, 4, 0) off
    sq = np.array([[0.0, 0.0, 0.0], [3.0, 0.0, 0.0], [0.0, 3.0, 0.0], [1.0, 1.0, 1.0]])
    dq = sq.copy()
    dq[3] += (3.0, 4.0, 0.0)
    c["at_the_distance"] = dict(src=sq, dst=dq, H=64, inlier_dist=5.0, seed=0, edge_tol=10.0)
    c["below_the_distance"] = dict(src=sq, dst=dq, H=64, inlier_dist=float(np.nextafter(5.0, 0.0)),
                                   seed=0, edge_tol=10.0)
    col = np.array([[0.0, 0.0, 0.0], [1.0, 1.0, 1.0], [2.0, 2.0, 2.0], [4.0, 4.0, 4.0]])
    c["collinear"] = dict(src=col, dst=2.0 * col, H=65, inlier_dist=0.1, seed=4)
    nan = src.copy()
    nan[::4] = np.nan
    c["nan_points"] = dict(src=nan, dst=dst, H=4097, inlier_dist=0.1, seed=6, edge_tol=1.0)
    r, d = _planted(65, 30, 31, sigma=0.02)
    c["two_chunks"] = dict(src=r, dst=d, H=ref.CHUNK + 65, inlier_dist=0.1, seed=8, edge_tol=0.05,
                           scale=(1.0, 1.6), candidates=40)
    for case in c.values():
        rf._freeze(case["src"], case["dst"])
    return c


RANSAC_NAMES = tuple(f"sizes_M{M}_H{H}" for M in (3, 4, 63, 64, 65) for H in (1, 64, 65, 4097)) + (
    "planted", "planted_rigid_gate", "rigid", "all_gated_out", "scale_gate_empty", "repeated_dst",
    "at_the_distance", "below_the_distance", "collinear", "nan_points", "two_chunks")


def ransac_args(name):
    case = dict(ransac_cases()[name])
    return (case.pop("src"), case.pop("dst"), case.pop("H"), case.pop("inlier_dist")), case


@functools.lru_cache(maxsize=None)
def ransac_want(name):
    args, kw = ransac_args(name)
    return ref.ransac(*args, **kw)
