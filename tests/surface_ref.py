"""The surface stage restated in numpy from the definitions in include/rsamd.h: TSDF fusion of
depth maps (``integrate``), marching tetrahedra on the Kuhn decomposition (``extract``) and the
derivation of its case table (``tet_table``).  All arithmetic is fp64; nothing here is read by
the package.
"""
import functools
import itertools

import numpy as np

EDGE_TYPES = ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1), (1, 1, 1))
PERMS = tuple(itertools.permutations(range(3)))     # (x, y, z) in lexicographic order
TET_EDGES = ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3))


def tet_corners(k):
    """The four corners (dx, dy, dz) of tet k along its path 000 -> +e_a -> +e_b -> 111."""
    a, b, _ = PERMS[k]
    p = np.zeros((4, 3), dtype=np.int64)
    p[1, a] = 1
    p[2, a] = p[2, b] = 1
    p[3] = 1
    return p


def corner_code(p):
    return int(p[0]) | int(p[1]) << 1 | int(p[2]) << 2


def edge_code(corners, i, j):
    """(owner corner code << 3) | edge type of the tet edge between path corners i and j."""
    i, j = min(i, j), max(i, j)
    e = tuple(int(v) for v in corners[j] - corners[i])
    return corner_code(corners[i]) << 3 | EDGE_TYPES.index(e)


@functools.lru_cache(maxsize=None)
def tet_table():
    """table[k][code] = (n, v0 .. v5): the n <= 2 triangles of tet k when the corners whose bit
    is set in `code` (bit i = path corner i) are negative; a vertex is an edge_code.  Every
    vertex is placed at its edge midpoint once and the triangle is oriented against the vector
    from the negative corners' centroid to the positive corners' centroid."""
    table = np.zeros((6, 16, 7), dtype=np.uint8)
    for k in range(6):
        P = tet_corners(k).astype(np.float64)

        def mid(e):
            return 0.5 * (P[e[0]] + P[e[1]])

        for code in range(1, 15):
            neg = [i for i in range(4) if code >> i & 1]
            pos = [i for i in range(4) if not code >> i & 1]
            out = P[pos].mean(axis=0) - P[neg].mean(axis=0)
            if len(neg) == 1 or len(pos) == 1:
                a = neg[0] if len(neg) == 1 else pos[0]
                tris = [[(a, b) for b in range(4) if b != a]]
            else:
                (n0, n1), (p0, p1) = neg, pos
                q = [(n0, p0), (n0, p1), (n1, p1), (n1, p0)]
                tris = [[q[0], q[1], q[2]], [q[0], q[2], q[3]]]
            row = [len(tris)]
            for t in tris:
                v = [mid(e) for e in t]
                if np.dot(np.cross(v[1] - v[0], v[2] - v[0]), out) < 0:
                    t = [t[0], t[2], t[1]]
                row += [edge_code(tet_corners(k), *e) for e in t]
            table[k, code, :len(row)] = row
    table.setflags(write=False)
    return table


def tet_corner_codes():
    return np.array([[corner_code(p) for p in tet_corners(k)] for k in range(6)], dtype=np.uint8)


def format_table():
    """The text the compiled header's check program prints."""
    lines = [" ".join(str(v) for v in row) for row in tet_corner_codes()]
    for k in range(6):
        for code in range(16):
            lines.append(" ".join(str(v) for v in tet_table()[k, code]))
    return "\n".join(lines) + "\n"


# ------------------------------------------------------------------------------------------
# 1. integrate
# ------------------------------------------------------------------------------------------
def node_positions(origin, voxel, dims):
    nz, ny, nx = dims
    iz, iy, ix = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    o = np.asarray(origin, dtype=np.float64)
    return np.stack((o[0] + voxel * ix, o[1] + voxel * iy, o[2] + voxel * iz), axis=-1)


def integrate(depth_maps, cams, K, origin, voxel, dims, trunc, weights=None, tsdf=None,
              weight=None, margins=None):
    """(tsdf, weight) float32 (nz, ny, nx).  With a dict `margins`, the smallest distance of a
    projection from a rounding boundary (px) and the smallest |s + trunc| over the samples
    that reach those tests are recorded in it."""
    depth = np.asarray(depth_maps, dtype=np.float64)
    V, h, w = depth.shape
    X = node_positions(origin, float(voxel), dims)
    acc, wsum = np.zeros(dims), np.zeros(dims)
    if margins is not None:
        margins.setdefault("round", np.inf)
        margins.setdefault("trunc", np.inf)
    with np.errstate(all="ignore"):
        for v in range(V):
            P = np.asarray(K, dtype=np.float64) @ np.asarray(cams[v], dtype=np.float64)
            q = X @ P[:, :3].T + P[:, 3]
            z = q[..., 2]
            fu, fv = q[..., 0] / z + 0.5, q[..., 1] / z + 0.5
            u, vv = np.floor(fu), np.floor(fv)
            inside = (u >= 0) & (u <= w - 1) & (vv >= 0) & (vv <= h - 1)
            ui = np.where(inside, u, 0).astype(np.int64)
            vi = np.where(inside, vv, 0).astype(np.int64)
            d = np.where(inside, depth[v, vi, ui], np.nan)
            wv = np.ones(dims) if weights is None else \
                np.where(inside, np.asarray(weights[v], dtype=np.float64)[vi, ui], np.nan)
            s = np.abs(d) - np.abs(z)
            front = inside & np.isfinite(d) & (d * z > 0) & np.isfinite(wv) & (wv > 0)
            use = front & (s >= -trunc)
            if margins is not None:
                near = np.isfinite(fu) & np.isfinite(fv) & (fu > -1) & (fu < w + 1) & \
                    (fv > -1) & (fv < h + 1)
                if near.any():
                    r = np.minimum(np.abs(fu - np.rint(fu)), np.abs(fv - np.rint(fv)))[near]
                    margins["round"] = min(margins["round"], float(r.min()))
                if front.any():
                    margins["trunc"] = min(margins["trunc"], float(np.abs(s + trunc)[front].min()))
            acc += np.where(use, wv * np.minimum(1.0, s / trunc), 0.0)
            wsum += np.where(use, wv, 0.0)
        W0 = np.zeros(dims) if weight is None else np.asarray(weight, dtype=np.float64)
        W0 = np.where(W0 > 0, W0, 0.0)
        T0 = np.zeros(dims) if tsdf is None else np.asarray(tsdf, dtype=np.float64)
        prior = np.where(W0 > 0, W0 * T0, 0.0)
        W = W0 + wsum
        T = np.where(W > 0, (prior + acc) / W, np.nan)
    return T.astype(np.float32), W.astype(np.float32)


# ------------------------------------------------------------------------------------------
# 2. extract
# ------------------------------------------------------------------------------------------
def _at(a, dx, dy, dz):
    """a[iz + dz, iy + dy, ix + dx] on a's own grid, False / 0 where that leaves the array
    (offsets in -1..1)."""
    p = np.pad(a, 1)
    nz, ny, nx = a.shape
    return p[1 + dz:1 + dz + nz, 1 + dy:1 + dy + ny, 1 + dx:1 + dx + nx]


def classify(tsdf, weight, min_weight):
    """(neg, cell, has): negative nodes, valid cells on the node grid (a cell is named by its
    lowest node), and has[..., t] = node owns a vertex on its edge of type t."""
    tsdf = np.asarray(tsdf, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        neg = tsdf < 0
    ok = (np.asarray(weight, dtype=np.float64) >= min_weight) & np.isfinite(tsdf)
    cell = np.ones(tsdf.shape, bool)
    for dz, dy, dx in itertools.product((0, 1), repeat=3):
        cell &= _at(ok, dx, dy, dz)
    has = np.zeros(tsdf.shape + (7,), bool)
    for t, (dx, dy, dz) in enumerate(EDGE_TYPES):
        inb = _at(np.ones(tsdf.shape, bool), dx, dy, dz)
        differ = inb & (neg != _at(neg, dx, dy, dz))
        anycell = np.zeros(tsdf.shape, bool)
        for sz, sy, sx in itertools.product((0, 1), repeat=3):
            if sx * dx or sy * dy or sz * dz:
                continue
            anycell |= _at(cell, -sx, -sy, -sz)
        has[..., t] = differ & anycell
    return neg, cell, has


def extract(tsdf, weight, origin, voxel, min_weight):
    """(vertices (Nv, 3) float64, faces (Nf, 3) int32) by the definition's numbering."""
    tsdf = np.asarray(tsdf, dtype=np.float32)
    nz, ny, nx = tsdf.shape
    neg, cell, has = classify(tsdf, weight, min_weight)
    vid = (np.cumsum(has.reshape(-1)) - 1).reshape(has.shape)
    origin = np.asarray(origin, dtype=np.float64)

    oz, oy, ox, ot = np.nonzero(has)
    e = np.array(EDGE_TYPES)[ot]
    fa = tsdf[oz, oy, ox].astype(np.float64)
    fb = tsdf[oz + e[:, 2], oy + e[:, 1], ox + e[:, 0]].astype(np.float64)
    t = fa / (fa - fb)
    o = np.stack((ox, oy, oz), axis=1).astype(np.float64)
    vertices = origin + voxel * (o + t[:, None] * e)

    cz, cy, cx = np.nonzero(cell)
    tris = np.full((len(cz), 6, 2, 3), -1, dtype=np.int64)
    table, corners = tet_table(), tet_corner_codes()
    for k in range(6):
        code = np.zeros(len(cz), dtype=np.int64)
        for i in range(4):
            c = int(corners[k, i])
            code |= neg[cz + (c >> 2 & 1), cy + (c >> 1 & 1), cx + (c & 1)].astype(np.int64) << i
        for m in range(1, 15):
            sel = np.nonzero(code == m)[0]
            if not len(sel):
                continue
            row = table[k, m]
            for j in range(int(row[0])):
                for q in range(3):
                    ec = int(row[1 + 3 * j + q])
                    c, ty = ec >> 3, ec & 7
                    tris[sel, k, j, q] = vid[cz[sel] + (c >> 2 & 1), cy[sel] + (c >> 1 & 1),
                                             cx[sel] + (c & 1), ty]
    tris = tris.reshape(-1, 3)
    faces = tris[tris[:, 0] >= 0].astype(np.int32)
    return vertices.reshape(-1, 3), faces.reshape(-1, 3)


# ------------------------------------------------------------------------------------------
# mesh properties the tests assert
# ------------------------------------------------------------------------------------------
def directed_edges(faces):
    f = np.asarray(faces, dtype=np.int64)
    return np.concatenate((f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]))


def repeated_directed_edges(faces):
    """How many directed edges occur more than once."""
    e = directed_edges(faces)
    _, n = np.unique(e, axis=0, return_counts=True)
    return int((n > 1).sum())


def is_closed(faces):
    """Every directed edge occurs once and its reverse once."""
    e = directed_edges(faces)
    if repeated_directed_edges(faces):
        return False
    a = np.unique(e, axis=0)
    b = np.unique(e[:, ::-1], axis=0)
    return a.shape == b.shape and bool(np.array_equal(a, b))


def euler(vertices, faces):
    e = np.sort(directed_edges(faces), axis=1)
    return len(vertices) - len(np.unique(e, axis=0)) + len(faces)


def signed_volume(vertices, faces):
    a, b, c = (vertices[faces[:, i]] for i in range(3))
    return float(np.einsum("ij,ij->i", a, np.cross(b, c)).sum() / 6.0)


def sphere_volume(n, centre, r):
    """(tsdf, weight) of |X - c| - r on an n^3 grid of unit voxels at the origin, float32."""
    X = node_positions((0.0, 0.0, 0.0), 1.0, (n, n, n))
    f = np.linalg.norm(X - np.asarray(centre, dtype=np.float64), axis=-1) - r
    return f.astype(np.float32), np.ones((n, n, n), np.float32)


def sphere_bound(r):
    """L^2 / (8 (r - L)), L = sqrt(3) voxels: linear interpolation of |X - c| - r along the
    longest tet edge."""
    L = np.sqrt(3.0)
    return L * L / (8.0 * (r - L))
