"""Inputs for tests/test_features_edges_cpu.py and tests/test_gpu_features_edges.py: the image
front end (csrc/features.hip: corner list, patch matching, Harris, non-maximum suppression) at
its tile, chunk and scan edges, at ties and on either side of the corner threshold.  Test
infrastructure; needs no GPU.

Every expected value is computed by tests/features_ref.py from these inputs; nothing here is
taken from the code under test.  No tolerance is defined here: the comparisons are exact, or use
the two bounds tests/test_gpu_features.py derives (test_harris, test_match_f64).

Constants of the kernels the cases aim at (features.hip):
  * corner list: chunks of 2048 pixels; the scan of the chunk counts runs in rounds of 256 with
    a carry; at most 1024 partial maxima
  * matching: 64 x 64 tiles; a thread owns 4 consecutive columns (rows) of a tile row (column),
    16 threads share it; fp64 patches are staged in chunks of 32 elements
  * Harris: 32 x 16 output tiles, halo max(1, ks / 2) + block_size
  * NMS: 32 x 8 tiles
"""
import functools

import numpy as np

import features_fixture as base
import features_ref as ref

F32_MAX = np.finfo(np.float32).max


def _frozen(a):
    a.setflags(write=False)
    return a


# ------------------------------------------------------------------------------------------
# 1. corner list
# ------------------------------------------------------------------------------------------
CHUNK = 2048            # pixels per workgroup (kCornerThreads * kCornerItems)
SCAN_ROUND = 256        # chunk counts per round of k_corner_scan
MAX_PARTIALS = 1024     # kCornerMaxBlocks
CORNER_SHAPES = ((512, 1024), (513, 1024), (1024, 2048), (1025, 2048), (1025, 2047))
CORNER_CHUNKS = (256, 257, 1024, 1025, 1025)
CORNER_REL = 0.001
CORNER_MAX = 1000.0     # at pixel n - 1 only: the threshold is 1
CORNER_HIT = 8.0
CORNER_DECOY = 0.5      # above 0.001 * 8: a hit as soon as the maximum at n - 1 is missed
FULL_CHUNK = 3
EMPTY_CHUNK = 6         # decoys only, between chunks 5 and 7 with hits
EDGE_CHUNKS = (255, 256, 1023, 1024)


def corner_chunks(shape):
    return -(-shape[0] * shape[1] // CHUNK)


def chunk_span(c, n):
    """(first, last) pixel of chunk c of an image of n pixels."""
    return c * CHUNK, min((c + 1) * CHUNK, n) - 1


@functools.lru_cache(maxsize=None)
def corner_case(shape):
    """Read-only float32 H of ``shape``, zero but for
      * CORNER_MAX at the last pixel n - 1 and nowhere else;
      * chunk FULL_CHUNK: CORNER_HIT at all 2048 pixels;
      * chunks 5 and 7: hits at 3 and at 5 pixels; chunk EMPTY_CHUNK between them: decoys only;
      * CORNER_HIT at the first and the last pixel of the chunks EDGE_CHUNKS that exist;
      * 300 more hits, 300 decoys and 300 negatives at random pixels of the other chunks."""
    h, w = shape
    n = h * w
    nb = corner_chunks(shape)
    rs = np.random.RandomState(n % 65521)
    H = np.zeros(n, np.float32)
    fixed = {FULL_CHUNK, 5, EMPTY_CHUNK, 7} | {c for c in EDGE_CHUNKS if c < nb}
    free = np.array([c for c in range(nb) if c not in fixed and c != nb - 1])
    at = rs.choice(free, 900) * CHUNK + rs.randint(0, CHUNK, 900)
    H[at[:300]] = CORNER_HIT
    H[at[300:600]] = CORNER_DECOY
    H[at[600:]] = -CORNER_HIT
    H[FULL_CHUNK * CHUNK:(FULL_CHUNK + 1) * CHUNK] = CORNER_HIT
    H[5 * CHUNK + np.array([1, 700, 2046])] = CORNER_HIT
    H[EMPTY_CHUNK * CHUNK + np.array([0, 9, 1024, 2047])] = CORNER_DECOY
    H[7 * CHUNK + np.array([0, 8, 63, 64, 2047])] = CORNER_HIT
    for c in EDGE_CHUNKS:
        if c < nb:
            H[list(chunk_span(c, n))] = CORNER_HIT
    H[n - 1] = CORNER_MAX
    return _frozen(H.reshape(h, w))


def chunk_counts(xy, shape):
    """Hits per 2048-pixel chunk of a (2, K) corner list."""
    return np.bincount((xy[1] * shape[1] + xy[0]) // CHUNK, minlength=corner_chunks(shape))


def one_hot():
    H = np.zeros((37, 53), np.float32)
    H[20, 31] = 2.0
    return H


# float32(rel * max) is the threshold, lies below it, lies above it
BOUNDARY = {"representable": (np.float32(1024.0), 0.5),
            "not representable": (np.float32(5.4891353), 0.001),
            "rounds up": (np.float32(3.0), 0.001)}
BOUNDARY_AT = ((0, 0), (17, 5), (36, 52), (9, 30))      # the maximum, below, at, above


def boundary_case(name):
    """(H, rel, pixels): a 37 x 53 image with the maximum and float32(rel * max) with its two
    float32 neighbours at BOUNDARY_AT; ``pixels`` are those three values, ascending."""
    mx, rel = BOUNDARY[name]
    t = np.float32(rel * float(mx))
    px = np.array([np.nextafter(t, np.float32(0)), t, np.nextafter(t, np.float32(np.inf))],
                  np.float32)
    H = np.zeros((37, 53), np.float32)
    H[BOUNDARY_AT[0]] = mx
    for at, v in zip(BOUNDARY_AT[1:], px):
        H[at] = v
    return H, rel, px


def header_rule(H, rel):
    """include/rsamd.h: (double)H > rel * (double)max(H)."""
    return H.astype(np.float64) > rel * float(H.max())


def numpy_rule(H, rel):
    """The recipe's own line as the installed numpy evaluates it."""
    return H > rel * np.max(H)


def float32_rule(H, rel):
    """What numpy >= 2 makes of that line, spelled out: a float32 product, a float32 comparison."""
    return H > np.float32(rel) * H.max()


def narrowed_rule(H, rel):
    """The other float32 comparison: the fp64 product, narrowed to float32 before comparing."""
    return H > np.float32(rel * float(H.max()))


def hits(mask):
    return np.flipud(np.vstack(np.nonzero(mask))).astype(np.int64)


def sign_images():
    """name -> 37 x 53 float32 image for rel = 0, 1 and a negative rel: positives, zeros (both
    signs) and negatives; zeros and negatives (maximum 0); negatives only."""
    rs = np.random.RandomState(77)
    mixed = np.round(rs.randn(37, 53) * 2).astype(np.float32)
    mixed[3, 4] = -0.0
    mixed[36, 52] = 9.0
    nonpos = -np.abs(mixed)
    nonpos[36, 52] = 0.0
    neg = nonpos - 1.0
    return {"mixed": mixed, "zeros and negatives": nonpos, "negatives": neg}


SIGN_RELS = (0.0, 1.0, -0.5, 2.0)


# ------------------------------------------------------------------------------------------
# 2. matching
# ------------------------------------------------------------------------------------------
TILE = 64
MATCH_IMAGE = (60, 80)
# the issue's six, and (130, 130): the only size at which index 129 exists
MATCH_SIZES = ((63, 65), (64, 64), (65, 63), (64, 129), (129, 128), (1, 1), (130, 130))
MATCH_ROIS = (1, 3, 15)
EXTREME_AT = (0, 1, 2, 7)       # indices of the four extreme legal centres
HOLDERS = (10, 11, 12, 13)      # rows (columns) whose zeros are the planted sets
MIN_TIED = 32                   # sides shorter than this carry no planted ties


def u8_image():
    return base.image_pair(*MATCH_IMAGE, 2)[0]


def tie_sets(n):
    """The planted index sets along a side of n entries, one per tie class; every set is held by
    one centre.  Indices that do not exist are left out.
      0  {3, 9, 67, 129 (128 when n = 129)}: across tiles, and 3 | 9 in one tile, two threads
      1  {4, 5}: one thread
      2  {19, 25}: one tile, two threads, nothing else
      3  {6, 70 (64 when n < 71), 128 when n >= 130}: across tiles, nothing else"""
    if n < MIN_TIED:
        return [[], [], [], []]
    sets = [[3, 9, 67, 129 if n >= 130 else 128], [4, 5], [19, 25],
            [6, 70 if n >= 71 else 64] + ([128] if n >= 130 else [])]
    return [[i for i in s if i < n] for s in sets]


def extremes(roi):
    h, w = MATCH_IMAGE
    m = roi // 2
    return np.array([[m, w - m - 1, m, w - m - 1], [m, m, h - m - 1, h - m - 1]])


@functools.lru_cache(maxsize=None)
def match_case(n1, n2, roi):
    """(xy1, xy2) for the image u8_image() on both sides.  Entries EXTREME_AT are the extreme
    legal centres.  Eight planted centres with eight different centre pixels, which no other
    centre shares (so their patches differ from every other patch at every roi): xy2 holds the
    first four at tie_sets(n2) and xy1[:, HOLDERS] are those four, so that row HOLDERS[k] has
    its zeros exactly at tie_sets(n2)[k]; the other four likewise with the sides swapped."""
    img = u8_image()
    h, w = MATCH_IMAGE
    m = roi // 2
    rs = np.random.RandomState(1000 * n1 + 10 * n2 + roi)
    ext = extremes(roi)
    taken = {int(img[y, x]) for x, y in ext.T}
    planted = []
    while len(planted) < 8:
        x, y = rs.randint(m, w - m), rs.randint(m, h - m)
        if int(img[y, x]) not in taken:
            taken.add(int(img[y, x]))
            planted.append((x, y))
    planted_values = {int(img[y, x]) for x, y in planted}
    out = []
    for n, mine, theirs in ((n1, planted[4:], planted[:4]), (n2, planted[:4], planted[4:])):
        xy = np.zeros((2, n), np.int64)
        for i in range(n):
            while True:
                x, y = rs.randint(m, w - m), rs.randint(m, h - m)
                if int(img[y, x]) not in planted_values:
                    break
            xy[:, i] = x, y
        for k, i in enumerate(EXTREME_AT):
            if i < n:
                xy[:, i] = ext[:, k]
        for centre, idx in zip(mine, tie_sets(n)):
            xy[:, idx] = np.array(centre)[:, None]
        if n >= MIN_TIED:
            xy[:, HOLDERS] = np.array(theirs).T
        out.append(_frozen(xy))
    return tuple(out)


def binary_pair():
    """A 0 / 255 noise image and its complement: equal centres are 225 * 65025 apart at roi 15."""
    rs = np.random.RandomState(31)
    a = (rs.randint(0, 2, MATCH_IMAGE) * 255).astype(np.uint8)
    return a, (255 - a).astype(np.uint8)


def binary_centres():
    rs = np.random.RandomState(32)
    xy1 = np.vstack([rs.randint(7, 73, 65), rs.randint(7, 53, 65)])
    xy2 = np.vstack([rs.randint(7, 73, 129), rs.randint(7, 53, 129)])
    xy2[:, [0, 64, 128]] = xy1[:, [5, 64, 0]]
    return xy1, xy2


MANY = 32768


@functools.lru_cache(maxsize=None)
def many_case():
    """(one (2, 1), many (2, 32768)) at roi 3: random legal centres of the 60 x 80 image, of
    which there are 4524, so that the one -- a copy of entry 20000 -- meets several exact zeros
    in different tiles."""
    rs = np.random.RandomState(33)
    many = np.vstack([rs.randint(1, 79, MANY), rs.randint(1, 59, MANY)])
    return _frozen(many[:, 20000:20001].copy()), _frozen(many)


F64_ROIS = (1, 3, 9, 15)
F64_SIZES = ((65, 129), (1, 5))
F64_CHUNK = 32


def f64_pair():
    """Two 60 x 80 float64 images that share their upper 30 rows."""
    rs = np.random.RandomState(12)
    img1, img2 = rs.randn(*MATCH_IMAGE) * 40.0, rs.randn(*MATCH_IMAGE) * 40.0
    img2[:30] = img1[:30]
    return img1, img2


def f64_case(n1, n2, roi):
    """(xy1, xy2): random centres, the extremes first, and shared centres whose patches lie in
    the rows the two images share: exact zeros."""
    h, w = MATCH_IMAGE
    m = roi // 2
    rs = np.random.RandomState(500 + 100 * n1 + roi)
    out = []
    for n in (n1, n2):
        xy = np.vstack([rs.randint(m, w - m, n), rs.randint(m, h - m, n)])
        k = min(4, n)
        xy[:, :k] = extremes(roi)[:, :k]
        out.append(xy)
    xy1, xy2 = out
    shared = np.vstack([rs.randint(m, w - m, 3), rs.randint(m, 30 - m, 3)])
    if n1 >= 8:
        xy1[:, 5:8] = shared
        xy2[:, [6, 70, 128]] = shared
    else:
        xy1[:, 0] = shared[:, 0]
        xy2[:, [2, 4]] = shared[:, :1]
    return xy1, xy2


# ------------------------------------------------------------------------------------------
# 3. Harris
# ------------------------------------------------------------------------------------------
HARRIS_PAIRS = ((1, 1), (1, 7), (2, 3), (4, 5), (8, 3), (16, 7), (30, 5), (31, 7), (31, 1))
HARRIS_TILE_PAIRS = ((1, 7), (2, 3), (4, 5), (8, 3))     # also at one 32 x 16 tile and around it
HARRIS_TILE_SHAPES = ((16, 32), (17, 33), (15, 31))
HARRIS_KINDS = ("texture", "noise", "step", "constant")
HARRIS_KS = (0.0, 0.04, 0.25, -0.1)
HARRIS_K_CASE = (4, 5, (37, 53))


def harris_halo(bs, ks):
    return max(1, ks // 2) + bs


def harris_shapes(bs, ks):
    R = harris_halo(bs, ks)
    shapes = [(R + 1, R + 1), (R + 1, 100), (100, R + 1)]
    if (bs, ks) in HARRIS_TILE_PAIRS:
        shapes += [s for s in HARRIS_TILE_SHAPES if min(s) > R]
    return shapes


def harris_image(kind, shape):
    h, w = shape
    if kind == "texture":
        return base.image_pair(h, w, 3)[0]
    if kind == "noise":
        return (np.random.RandomState(h * 1000 + w).randint(0, 2, shape) * 255).astype(np.uint8)
    if kind == "step":
        img = np.zeros(shape, np.uint8)
        img[:, w // 2:] = 255
        return img
    return np.full(shape, 77, np.uint8)


# ------------------------------------------------------------------------------------------
# 4. NMS
# ------------------------------------------------------------------------------------------
NMS_SHAPES = ((1, 1), (1, 9), (9, 1), (8, 32), (9, 33), (7, 31), (41, 67))
PLATEAU = 8.0
# (41, 67): window -> a block of PLATEAU whose first row and column lie at distance
# (window - 1) / 2 from the border, the edge of the legal region
PLATEAUS = {3: (slice(1, 3), slice(1, 5)), 7: (slice(3, 5), slice(40, 44)),
            31: (slice(15, 17), slice(50, 52))}


def nms_windows(shape):
    """1, 3, 7, 31, 2 min - 1, 2 max + 1, 2^31 - 1, and the smaller side itself where it is odd
    (one row or column of legal centres)."""
    lo, hi = min(shape), max(shape)
    wins = {1, 3, 7, 31, 2 * lo - 1, 2 * hi + 1, 2147483647}
    if lo % 2 == 1:
        wins.add(lo)
    return sorted(wins)


def nms_image(shape):
    """Finite float32: small integers of both signs (many equal neighbours), a few -0.0 (the last
    pixel is one, the first is -2), float32 max at the centre pixel (h // 2, w // 2), and on shapes that have room the plateaus."""
    h, w = shape
    rs = np.random.RandomState(7 * h + w)
    img = np.round(rs.rand(h, w) * 8 - 3).astype(np.float32)
    img[rs.rand(h, w) < 0.1] = -0.0
    if h * w >= 3:
        img[0, 0], img[-1, -1] = -2.0, -0.0
    if h >= 8:
        img[PLATEAUS[3]] = PLATEAU
    if shape == (41, 67):
        img[PLATEAUS[7]] = PLATEAU
        img[PLATEAUS[31]] = PLATEAU
    img[h // 2, w // 2] = F32_MAX
    return img
