"""Inputs that sit exactly on the decision boundaries of the dense, surface and colour stages
(include/rsamd.h), for tests/test_boundaries_cpu.py and tests/test_gpu_boundaries.py.

Everything is dyadic: cameras, warps, depths, voxels and tolerances are small integers times
powers of two, images hold grey levels within 16 of 128.  Every fp64 product and sum up to a
compared quantity is then exactly representable, so FMA contraction, summation order and fp32
against fp64 cannot move a decision, and a kernel must agree with the restatement on the
boundary itself.  The CPU test proves that for every case; this file only states the cases and,
where a case is small enough, the answer written out by hand.

Cameras are given as the matrices the C entries take (A, b; P, Minv; P).  The restatements that
want (cams, K) get (P, I3): K @ P is then P bit for bit.
"""
import functools

import numpy as np

I3 = np.eye(3)
MIN_VAR = 2.0                      # min_var n^2 = 162 at patch 3, 29282 at patch 11: exact in fp32
MIN_VAR_ABOVE = float(np.nextafter(np.float32(2.0), np.float32(3.0)))   # one float32 step above


def up(x):
    return float(np.nextafter(x, np.inf))


def down(x):
    return float(np.nextafter(x, -np.inf))


def texture(h, w, seed):
    """(h, w) uint8 within 16 of 128 from an integer recurrence of the pixel position."""
    y, x = np.mgrid[0:h, 0:w].astype(np.uint64)
    v = (x * np.uint64(73) + y * np.uint64(151) + np.uint64(seed) * np.uint64(29) + np.uint64(7))
    v = (v * np.uint64(2654435761)) % np.uint64(1 << 32)
    v = ((v >> np.uint64(7)) ^ (v >> np.uint64(19))) % np.uint64(33)
    return (v.astype(np.int64) + 112).astype(np.uint8)


# ------------------------------------------------------------------------------------------
# plane sweep
# ------------------------------------------------------------------------------------------
def _sweep(ref, srcs, A, b, depths, patch, min_var=MIN_VAR, **notes):
    case = dict(ref=np.ascontiguousarray(ref, dtype=np.uint8),
                srcs=np.ascontiguousarray(srcs, dtype=np.uint8),
                A=np.ascontiguousarray(A, dtype=np.float64).reshape(-1, 3, 3),
                b=np.ascontiguousarray(b, dtype=np.float64).reshape(-1, 3),
                depths=np.ascontiguousarray(depths, dtype=np.float64), patch=patch,
                min_var=min_var)
    case.update(notes)
    for v in case.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return case


def _shift_case(h, w, patch, t, axis, depths, match, seed, copies=1):
    """A = I and b = t e_axis: x' = x + t / d.  The source is the reference rolled by the shift of
    depths[match], so that plane matches exactly wherever its window is valid."""
    ref = texture(h, w, seed)
    s = t / depths[match]
    assert s == int(s)
    src = np.roll(ref, int(s), axis=1 - axis)
    b = [0.0, 0.0, 0.0]
    b[axis] = float(t)
    return _sweep(ref, [src] * copies, [I3] * copies, [b] * copies, depths, patch,
                  shift=(axis, float(t)), match=match)


def shift_valid(case):
    """By hand, for a shift case: valid[k, y, x] of the single source.  The window of (x, y) must
    lie in the image, and so must its outermost sample after the shift s_k = t / d_k: on the
    last column or row it is still valid (x' == w - 1), one step further it is not."""
    h, w = case["ref"].shape
    r = case["patch"] // 2
    axis, t = case["shift"]
    y, x = np.mgrid[0:h, 0:w]
    window = (x >= r) & (x <= w - 1 - r) & (y >= r) & (y <= h - 1 - r)
    out = []
    for d in case["depths"]:
        s = t / d
        c, hi = (x, w - 1) if axis == 0 else (y, h - 1)
        out.append(window & (c - r + s >= 0) & (c + r + s <= hi))
    return np.array(out)


LADDER = (1.0, 2.0, 4.0, 8.0)      # shifts 4, 2, 1, 1/2 at t = 4


def _alternating(h, w):
    """a(x, y) - 128 = (-1)^x m(y), m in 3..10: a shift by one column negates the shifted image,
    a shift by two restores it.  ZNCC is then exactly -1 and exactly 1."""
    y, x = np.mgrid[0:h, 0:w]
    return (128 + (1 - 2 * (x % 2)) * (3 + (y * 5) % 8)).astype(np.uint8)


def _q2_case():
    """Third row of A = (1, 0, -11), b = 0: q2 = d (x - 11) vanishes on column 11, is negative left
    of it and d k on column 11 + k.  Rows 0 and 1 are chosen so that x' = 2 + 6 / k and y' = 3:
    8, 5, 4, 3.5 on columns 12..15, weights in {0, 1/2}.  The warp does not depend on d, so one
    plane only (more would tie).  Window centres 13 and 14 are valid, 12 (it holds column 11,
    where q0 / q2 = 6 d / 0 and q1 / q2 = 0 / 0) is not."""
    h, w = 8, 16
    A = [[2.0, 0.0, -16.0], [3.0, 0.0, -33.0], [1.0, 0.0, -11.0]]
    return _sweep(texture(h, w, 5), [texture(h, w, 6)], [A], [[0.0, 0.0, 0.0]], [2.0], 3,
                  zero_column=11)


def q2_valid(case):
    h, w = case["ref"].shape
    out = np.zeros((1, h, w), bool)
    out[0, 1:h - 1, 13:15] = True
    return out


PLANT = (10, 3)                    # column and first row of the three planted pixels


def _planted(h, w):
    """Flat 128 but for three pixels at 131 in one column: a 3 x 3 window that holds all three
    has n sum a^2 - (sum a)^2 = 9 * 27 - 81 = 162 = MIN_VAR * 81, one that holds two has 126."""
    img = np.full((h, w), 128, np.uint8)
    c, r0 = PLANT
    img[r0:r0 + 3, c] = 131
    return img


def planted_valid(case):
    """By hand: plane k of the variance cases is valid on exactly three windows."""
    h, w = case["ref"].shape
    c, r0 = PLANT
    out = np.zeros((len(case["depths"]), h, w), bool)
    for k, d in enumerate(case["depths"]):
        s = int(4 / d) if case["planted"] == "src" else 0
        out[k, r0 + 1, c - s - 1:c - s + 2] = True
    if case["min_var"] != MIN_VAR:
        out[:] = False
    return out


def _deep(first):
    """RS_DENSE_MAX_DEPTHS planes on 4 x 4, patch 3, shift 4 / d_k: d_k = (k + 1) / 4096 for the
    first 4095 planes, a shift above 4 that takes every sample out of the image, and d = 4
    (shift 1) for the last, the match.  It keeps the window of column 1 inside; the windows of
    column 2 have no valid plane."""
    d = (np.arange(4096) + 1.0) / 4096.0
    d[4095] = 4.0
    depths = d[::-1].copy() if first else d
    return _shift_case(4, 4, 3, 4.0, 0, depths, 0 if first else 4095, 11)


@functools.lru_cache(maxsize=None)
def sweep_cases():
    c = {}
    # shifts and tile fit: one tile exactly, one row and one column spill, two by two tiles, a
    # halo wider than the interior rows
    c["xpos_8x32_p3"] = _shift_case(8, 32, 3, 4.0, 0, LADDER, 2, 1)
    c["xneg_9x33_p3"] = _shift_case(9, 33, 3, -4.0, 0, LADDER, 2, 2)
    c["ypos_16x64_p3"] = _shift_case(16, 64, 3, 4.0, 1, LADDER, 2, 3)
    c["yneg_9x33_p3"] = _shift_case(9, 33, 3, -4.0, 1, LADDER, 2, 4)
    c["xpos_12x44_p11"] = _shift_case(12, 44, 11, 4.0, 0, LADDER, 2, 5)
    # both directions at once: nvalid 0, 1 and 2
    p, n = c["xpos_8x32_p3"], _shift_case(8, 32, 3, -4.0, 0, LADDER, 2, 1)
    c["xboth_8x32_p3"] = _sweep(p["ref"], [p["srcs"][0], n["srcs"][0]], [I3, I3],
                                [p["b"][0], n["b"][0]], LADDER, 3)
    # ties
    c["tie_pair"] = _shift_case(9, 33, 3, 4.0, 0, (1.0, 2.0, 4.0, 4.0, 8.0), 2, 7)
    c["tie_triple"] = _shift_case(9, 33, 3, 4.0, 0, (8.0, 4.0, 4.0, 4.0, 2.0), 1, 8)
    alt = _alternating(8, 32)
    c["tie_exact"] = _sweep(alt, [alt], [I3], [[2.0, 0.0, 0.0]], (2.0, 1.0, 1.0), 3,
                            shift=(0, 2.0), match=1)
    c["twin_sources"] = _shift_case(8, 32, 3, 4.0, 0, LADDER, 2, 1, copies=2)
    c["q2_zero"] = _q2_case()
    # the variance thresholds, reference side and warped side, on and one float32 step above
    tex = texture(9, 33, 9)
    for side in ("ref", "src"):
        ref, src = (_planted(9, 33), tex) if side == "ref" else (tex, _planted(9, 33))
        for name, mv in (("on", MIN_VAR), ("above", MIN_VAR_ABOVE)):
            c[f"var_{side}_{name}"] = _sweep(ref, [src], [I3], [[4.0, 0.0, 0.0]], (4.0, 2.0), 3,
                                             min_var=mv, planted=side)
    c["deep_last"] = _deep(False)
    c["deep_first"] = _deep(True)
    return c


SGM_CASES = ("xneg_9x33_p3", "tie_pair")
SHIFT_CASES = ("xpos_8x32_p3", "xneg_9x33_p3", "ypos_16x64_p3", "yneg_9x33_p3", "xpos_12x44_p11",
               "tie_pair", "tie_triple", "tie_exact", "deep_last", "deep_first")
PLANTED_CASES = ("var_ref_on", "var_ref_above", "var_src_on", "var_src_above")


def hand_valid(name):
    """valid[k, y, x] written out by hand, or None where the case has no such answer."""
    case = sweep_cases()[name]
    if name in SHIFT_CASES:
        return shift_valid(case)
    if name in PLANTED_CASES:
        return planted_valid(case)
    if name == "q2_zero":
        return q2_valid(case)
    return None


def first_of_ties(depths):
    """Plane indices with the later copies of a repeated depth left out."""
    d = list(depths)
    return [k for k in range(len(d)) if d[k] not in d[:k]]


@functools.lru_cache(maxsize=None)
def reference_sweeps():
    """name -> (index, delta, score, nvalid, volume, counts) of tests/dense_ref.py in fp64,
    computed once and shared; read-only."""
    import dense_ref
    out = {}
    for name, c in sweep_cases().items():
        vol, nv = dense_ref.cost_volume(c["ref"], c["srcs"], c["A"], c["b"], c["depths"],
                                        c["patch"], c["min_var"])
        res = dense_ref.winners(vol, nv) + (vol, nv)
        for a in res:
            a.setflags(write=False)
        out[name] = res
    return out


@functools.lru_cache(maxsize=None)
def fp32_sweeps():
    """name -> (volume, nvalid) of the restatement in float32 with reversed window sums."""
    import dense_ref
    return {name: dense_ref.cost_volume(c["ref"], c["srcs"], c["A"], c["b"], c["depths"],
                                        c["patch"], c["min_var"], np.float32, True)
            for name, c in sweep_cases().items()}


@functools.lru_cache(maxsize=None)
def fp32_deviation():
    out = {}
    for name, (v32, _) in fp32_sweeps().items():
        v64 = reference_sweeps()[name][4]
        both = ~np.isnan(v64) & ~np.isnan(v32)
        out[name] = float(np.abs(v32[both].astype(np.float64) - v64[both]).max()) \
            if both.any() else 0.0
    return out


def score_bar():
    """The recipe of dense_fixture.score_bar on these cases alone: 8 x the largest deviation of
    the restatement in float32 with reversed window sums from the restatement in fp64."""
    return 8.0 * max(fp32_deviation().values())


# ------------------------------------------------------------------------------------------
# consistency
# ------------------------------------------------------------------------------------------
def _views(offsets):
    P = np.zeros((len(offsets), 3, 4))
    P[:, :, :3] = I3
    P[:, :, 3] = offsets
    return P, np.tile(I3, (len(offsets), 1, 1))


def _cons(depth, offsets, rel_tol, **notes):
    P, Minv = _views(offsets)
    case = dict(depth=np.ascontiguousarray(depth, dtype=np.float64), P=P, Minv=Minv,
                rel_tol=rel_tol)
    case.update(notes)
    return case


def _half_pixel_maps():
    """Two views, M = I, m_0 = 0 and m_1 = (1, -1, 0), every depth of view 0 equal to 2: pixel
    (x, y) of view 0 lands on (x + 1/2, y - 1/2) in view 1, which rounds to (x + 1, y), and a
    pixel of view 1 with depth 2 lands on (x - 1/2, y + 1/2) in view 0, which rounds to
    (x, y + 1).  So u == 2.5 goes to pixel 3, u == -0.5 to pixel 0, u == w - 0.5 to w (outside),
    and likewise for v.  d' is the pixel's own depth (the third rows are equal), so view 0's
    pixels compare 2 with what is planted in view 1: at rel_tol 0.25 the bound is 2.5 and 1.5."""
    h, w = 3, 6
    d0 = np.full((h, w), 2.0)
    d1 = np.full((h, w), 2.0)
    d1[0, 1:6] = (2.5, up(2.5), 1.5, down(1.5), 2.0)
    d1[1, 1:6] = (np.inf, -np.inf, np.nan, up(2.0), down(2.0))
    d1[2, 1:6] = (2.0, 2.25, 1.75, 4.0, 1.0)
    return np.array((d0, d1))


# count[0, y, x] by hand (view 1 read at (x + 1, y); column 5 lands outside), per rel_tol
HALF_PIXEL_VIEW0 = {0.25: [[1, 0, 1, 0, 1, 0], [0, 0, 0, 1, 1, 0], [1, 1, 1, 0, 0, 0]],
                    0.0: [[0, 0, 0, 0, 1, 0], [0, 0, 0, 0, 0, 0], [1, 0, 0, 0, 0, 0]]}


def _lane_maps(V, h, w, seed):
    """Depths from {2, 2.5, up(2.5), NaN}; view v is offset by (v, 0, 0), half a pixel a view."""
    pick = np.array((2.0, 2.0, 2.5, up(2.5), np.nan))
    t = np.stack([texture(h, w, seed + v) for v in range(V)]).astype(np.int64)
    return pick[t % 5]


@functools.lru_cache(maxsize=None)
def consistency_cases():
    c = {}
    m = [(0.0, 0.0, 0.0), (1.0, -1.0, 0.0)]
    c["half_pixel_tol25"] = _cons(_half_pixel_maps(), m, 0.25)
    c["half_pixel_tol0"] = _cons(_half_pixel_maps(), m, 0.0)
    c["views128"] = _cons(np.full((128, 2, 2), 4.0), np.zeros((128, 3)), 0.25)
    # h w V around the 256 lanes of a workgroup.  V = 2 cannot give an odd product, and a prime
    # 127 or 257 does not fit 64 x 16: 255 = 3 x 5 x 17, 256 = 2 x 8 x 16, 258 = 2 x 3 x 43
    for V, h, w in ((3, 5, 17), (2, 8, 16), (2, 3, 43)):
        off = [(float(v), 0.0, 0.0) for v in range(V)]
        c[f"lanes{V * h * w}"] = _cons(_lane_maps(V, h, w, 20), off, 0.25)
    return c


# ------------------------------------------------------------------------------------------
# TSDF fusion and extraction
# ------------------------------------------------------------------------------------------
def _tsdf(depth, P, origin, voxel, dims, trunc, weights=None, tsdf=None, weight=None):
    f32 = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.float32)
    return dict(depth=np.ascontiguousarray(depth, dtype=np.float64),
                P=np.ascontiguousarray(P, dtype=np.float64).reshape(-1, 3, 4),
                origin=np.array(origin, dtype=np.float64), voxel=float(voxel), dims=tuple(dims),
                trunc=float(trunc), weights=f32(weights), tsdf=f32(tsdf), weight=f32(weight))


# u = X0 / z + 1, v = X1 / z + 1/2, z = X2
TSDF_P = np.array([[1.0, 0.0, 1.0, 0.0], [0.0, 1.0, 0.5, 0.0], [0.0, 0.0, 1.0, 0.0]])


@functools.lru_cache(maxsize=None)
def tsdf_cases():
    """5 x 1 x 9 nodes (nz, ny, nx): X0 = -2 + ix / 2, X1 = 0, z = iz / 2, an image of 2 x 3.
    v = 1/2 at every node in front, which rounds up to row 1 = h - 1; row 0 holds NaN, so a
    kernel that rounded half down would fuse nothing.  On z = 1 the columns are u = X0 + 1 =
    -1, -1/2, ..., 3: -1/2 goes to pixel 0, 3/2 to pixel 2 = w - 1, 2 stays there, 5/2 goes to 3
    (outside).  z = 0 is the camera plane.  trunc = 1/2 and row 1 holds depths 3/2, the double
    below 3/2, and 2: at z = 2 the first gives s == -trunc (included, -1), the second is one
    step behind (excluded); at z = 1 both 3/2 and 2 give s >= trunc (exactly 1)."""
    nan = np.nan
    depth = np.array([[[nan, nan, nan], [1.5, down(1.5), 2.0]]])
    grid = dict(origin=(-2.0, 0.0, 0.0), voxel=0.5, dims=(5, 1, 9), trunc=0.5)
    c = {"plain": _tsdf(depth, TSDF_P, **grid)}
    # a second, identical view whose weights are 1, 0 and negative, then +inf, NaN and 1: it
    # counts only at the 1
    two = np.concatenate((depth, depth))
    wts = np.ones((2, 2, 3), np.float32)
    wts[1, 1] = (1.0, 0.0, -1.0)
    c["weights"] = _tsdf(two, (TSDF_P, TSDF_P), weights=wts, **grid)
    wts2 = wts.copy()
    wts2[1, 1] = (np.inf, np.nan, 1.0)
    c["weights_nan"] = _tsdf(two, (TSDF_P, TSDF_P), weights=wts2, **grid)
    # a prior of weight 1, 0, negative and NaN in turn along x, with a tsdf that must not be
    # read where the weight is not > 0
    W0 = np.tile(np.array((1.0, 0.0, -1.0, np.nan, 1.0, -0.0, 1.0, np.nan, -np.inf), np.float32),
                 (5, 1, 1))
    T0 = np.tile(np.array((0.5, 7.0, -3.0, np.nan, -1.0, np.inf, 0.25, 1e30, 0.5), np.float32),
                 (5, 1, 1))
    c["prior"] = _tsdf(depth, TSDF_P, tsdf=T0, weight=W0, **grid)
    # 1 x 1 x 257: one node past a workgroup; z = 2, u = X0 / 2 in steps of 1/4 from -1 to 63, an
    # image of 1 x 64, v = 0 = h - 1.  (The double below 3/2 minus 2 is exact in fp64; with z = 1
    # the double below 1/2 would round back onto -trunc.)
    P = np.array([[1.0, 0.0, 0.0, 0.0], [0.0, 1.0, 0.0, 0.0], [0.0, 0.0, 1.0, 0.0]])
    pick = np.array((2.5, down(2.5), 1.5, down(1.5), 2.0, 2.25, 1.75, np.nan))
    row = pick[texture(1, 64, 30).astype(np.int64)[0] % 8]
    c["row257"] = _tsdf(row[None, None, :], P, (-2.0, 0.0, 2.0), 0.5, (1, 1, 257), 0.5)
    return c


@functools.lru_cache(maxsize=None)
def extract_cases():
    """name -> (tsdf, weight, origin, voxel, min_weight, expected number of faces or None)."""
    one = np.ones((2, 2, 2), np.float32)
    c = {}
    t = one.copy()
    t[0, 0, 0] = -0.0
    c["minus_zero"] = (t, one * 2, (0.0, 0.0, 0.0), 1.0, 2.0, 0)
    t = one.copy()
    t[0, 0, 0] = -1.0
    c["minus_one"] = (t, one * 2, (0.0, 0.0, 0.0), 1.0, 2.0, None)
    w = one * 3
    w[1, 0, 1] = 2.0
    c["weight_on"] = (t, w, (0.0, 0.0, 0.0), 1.0, 2.0, None)
    w = w.copy()
    w[1, 0, 1] = np.nextafter(np.float32(2.0), np.float32(0.0))
    c["weight_below"] = (t, w, (0.0, 0.0, 0.0), 1.0, 2.0, 0)
    return c


# ------------------------------------------------------------------------------------------
# z-buffer and gather
# ------------------------------------------------------------------------------------------
TEX_P = np.array([[[1.0, 0.0, 0.0, 0.0], [0.0, 1.0, 0.0, 0.0], [0.0, 0.0, 1.0, 0.0]]])


def _square(n, z=4.0):
    """Two triangles over pixels [0, n - 1]^2 on the plane of depth z, sharing the diagonal
    (0, 0)-(n - 1, n - 1), which runs through pixel centres.  The first covers px >= py."""
    m = (n - 1) * z
    v = np.array([[-0.0, -0.0, z], [m, 0.0, z], [m, m, z], [0.0, m, z]])
    return v, np.array([[0, 1, 2], [0, 2, 3]], np.int32)


@functools.lru_cache(maxsize=None)
def raster_cases():
    """name -> (vertices, faces, (h, w), expected z-buffer written out by hand or None)."""
    c = {}
    for n, tag in ((5, "small"), (9, "large")):       # boxes of 25 and 81 pixels around the 32
        v, f = _square(n)
        c[f"pair_{tag}"] = (v, f, (n, n), np.full((1, n, n), 4.0, np.float32))
        py, px = np.mgrid[0:n, 0:n]
        one = np.where(px >= py, np.float32(4.0), np.float32(np.nan))[None]
        c[f"one_{tag}"] = (v, f[:1], (n, n), one)
        c[f"other_{tag}"] = (v, f[1:], (n, n),
                             np.where(px <= py, np.float32(4.0), np.float32(np.nan))[None])
    # a face with one vertex on the camera plane is skipped; the slanted face behind it is drawn
    v = np.array([[0.0, 0.0, 0.0], [32.0, 0.0, 4.0], [0.0, 32.0, 4.0],
                  [0.0, 0.0, 2.0], [32.0, 0.0, 4.0], [0.0, 32.0, 4.0]])
    c["camera_plane"] = (v, np.array([[0, 1, 2]], np.int32), (9, 9),
                         np.full((1, 9, 9), np.nan, np.float32))
    c["slanted"] = (v, np.array([[0, 1, 2], [3, 4, 5]], np.int32), (9, 9), None)
    return c


@functools.lru_cache(maxsize=None)
def gather_cases():
    """name -> dict(vertices, faces, normals, rel_tol, min_cos, count by hand).  The mesh is the
    first triangle of the 9 x 9 square (pixels px >= py hold 4.0, the rest NaN); the vertices
    below the three of the face belong to no face."""
    v, f = _square(9)
    f = f[:1]
    probes = np.array([
        [0.0, 0.0, 4.0],        # 3  u == 0, v == 0
        [32.0, 32.0, 4.0],      # 4  u == w - 1, v == h - 1: the footprint is clamped
        [32.0, 0.0, 4.0],       # 5  u == w - 1
        [10.0, 14.0, 4.0],      # 6  (2.5, 3.5): of the footprint only (3, 3) is covered
        [6.0, 18.0, 4.0],       # 7  (1.5, 4.5): no pixel of the footprint is covered
        [20.0, 10.0, 5.0],      # 8  z == far (1 + 1/4)
        [20.0, 10.0, up(5.0)],  # 9  one double behind it (u, v within 1e-15 of (4, 2))
        [16.0, 8.0, 4.0],       # 10 z == far
        [16.0, 8.0, up(4.0)],   # 11 one double behind
        [3.0, 0.0, 4.0],        # 12 the 3-4-5 vertex: g == 4 / 5 with the normal (0, 0, -1)
    ])
    vertices = np.concatenate((v[:3], probes))
    normals = np.tile((0.0, 0.0, -1.0), (len(vertices), 1))
    cases = {}
    base = dict(vertices=vertices, faces=f, shape=(9, 9))
    #                                   0  1  2  3  4  5  6  7  8  9 10 11 12
    cases["tol25"] = dict(base, normals=None, rel_tol=0.25, min_cos=0.0,
                          count=[1, 1, 1, 1, 1, 1, 1, 0, 1, 0, 1, 1, 1])
    cases["tol0"] = dict(base, normals=None, rel_tol=0.0, min_cos=0.0,
                         count=[1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 1, 0, 1])
    cases["cos_on"] = dict(base, normals=normals, rel_tol=0.25, min_cos=0.8, count=None)
    cases["cos_below"] = dict(base, normals=normals, rel_tol=0.25, min_cos=down(0.8), count=None)
    return cases


def gather_images(channels):
    img = np.stack([texture(9, 9, 40 + k).astype(np.int64) * 7 % 256 for k in range(channels)],
                   axis=-1).astype(np.uint8)
    return np.ascontiguousarray(img[None] if channels == 3 else img[None, :, :, 0])
