"""numpy restatement of the mesh simplification (include/rsamd.h, rs_mesh_simplify;
csrc/simplify.hip): vertex clustering on a uniform grid, quadric placement.  The reference project
has no such code; this is the definition written a second time, independent of the HIP source.

Every number is an IEEE double and every operation below is one rounded +, -, *, / or sqrt on
doubles -- numpy's element-wise operations are exactly that -- in the order the definition
states, so the device, which fuses no product with a sum in this stage, gives the same bits.  Sums
that have an order (the mean, the ten numbers of a quadric) are taken term by term, never with
numpy's own reductions, whose order is its own.  The operation order of the position (step 5) is
written once, here: ``jacobi3`` and ``positions``.
"""
import numpy as np

import mesh_ref

MAX_CELLS = 1 << 27
MEAN, QUADRIC = 0, 1
PLACEMENTS = {"mean": MEAN, "quadric": QUADRIC}
INFO_KEYS = ("clusters", "fallbacks", "degenerate_faces", "duplicate_faces", "longest_row")


def grid(vertices, cell, origin=None):
    """(origin, dims) as ``surface.simplify_grid``: the per-axis minimum unless given, and
    dims = floor((max - origin) / cell) + 1 along x, y, z."""
    v = np.asarray(vertices, dtype=np.float64).reshape(-1, 3)
    if origin is None:
        origin = v.min(axis=0) if len(v) else np.zeros(3)
    origin = np.asarray(origin, dtype=np.float64)
    if not len(v):
        return origin, (1, 1, 1)
    top = np.floor((v.max(axis=0) - origin) / float(cell))
    return origin, tuple(int(t) + 1 for t in top)


def cells(x, origin, cell):
    """floor((x - origin) / cell) per axis, as doubles."""
    return np.floor((x - origin) / cell)


def _ordered_sums(group, order, terms, ngroups):
    """Per group, the sum of the rows of ``terms`` in ascending ``order``, from the first term,
    left to right: (sums (ngroups, k), 0 for a group without a term; counts (ngroups,))."""
    o = np.lexsort((order, group))
    g, t = group[o], terms[o]
    count = np.bincount(g, minlength=ngroups)
    start = np.searchsorted(g, np.arange(ngroups))
    acc = np.zeros((ngroups, terms.shape[1]))
    has = count > 0
    acc[has] = t[start[has]]
    for r in range(1, int(count.max()) if len(count) else 0):
        sel = np.flatnonzero(count > r)
        acc[sel] = acc[sel] + t[start[sel] + r]
    return acc, count


def jacobi3(A):
    """Cyclic Jacobi on n symmetric 3 x 3 matrices (n, 3, 3), the loop of device_math.h's
    jacobi3_exact operation by operation: the sweeps stop, per matrix, when the off-diagonal
    mass is not above 1e-30 of the diagonal's, after 30 sweeps at the latest; the rotations
    are (0, 1), (0, 2), (1, 2), each skipped where its element is 0.  Returns (A with the
    eigenvalues on its diagonal, V with the eigenvectors in its columns)."""
    A = np.array(A, dtype=np.float64)
    n = len(A)
    V = np.zeros((n, 3, 3))
    V[:, 0, 0] = V[:, 1, 1] = V[:, 2, 2] = 1.0
    active = np.ones(n, dtype=bool)
    for _ in range(30):
        off = A[:, 0, 1] * A[:, 0, 1] + A[:, 0, 2] * A[:, 0, 2] + A[:, 1, 2] * A[:, 1, 2]
        dia = A[:, 0, 0] * A[:, 0, 0] + A[:, 1, 1] * A[:, 1, 1] + A[:, 2, 2] * A[:, 2, 2]
        active &= off > 1e-30 * dia
        if not active.any():
            break
        for p, q in ((0, 1), (0, 2), (1, 2)):
            idx = np.flatnonzero(active & (A[:, p, q] != 0.0))
            if not len(idx):
                continue
            a, v = A[idx], V[idx]
            apq = a[:, p, q]
            th = (a[:, q, q] - a[:, p, p]) / (2.0 * apq)
            t = np.where(th >= 0.0, 1.0, -1.0) / (np.abs(th) + np.sqrt(th * th + 1.0))
            c = 1.0 / np.sqrt(t * t + 1.0)
            s = t * c
            for k in range(3):      # columns p, q
                akp, akq = a[:, k, p].copy(), a[:, k, q].copy()
                a[:, k, p] = c * akp - s * akq
                a[:, k, q] = s * akp + c * akq
            for k in range(3):      # rows p, q
                apk, aqk = a[:, p, k].copy(), a[:, q, k].copy()
                a[:, p, k] = c * apk - s * aqk
                a[:, q, k] = s * apk + c * aqk
            for k in range(3):
                vkp, vkq = v[:, k, p].copy(), v[:, k, q].copy()
                v[:, k, p] = c * vkp - s * vkq
                v[:, k, q] = s * vkp + c * vkq
            A[idx], V[idx] = a, v
    return A, V


def positions(mean, quad, want, origin, cell, placement, rank_tol):
    """Step 5.  mean (n, 3), quad (n, 10) = A00 A01 A02 A11 A12 A22 b0 b1 b2 c, want (n, 3) the
    clusters' cell indices as doubles.  Returns (x (n, 3), fallback (n,) bool)."""
    n = len(mean)
    x = mean.copy()
    fallback = np.zeros(n, dtype=bool)
    if placement != QUADRIC or n == 0:
        return x, fallback
    q = quad
    A = np.empty((n, 3, 3))
    A[:, 0, 0], A[:, 0, 1], A[:, 0, 2] = q[:, 0], q[:, 1], q[:, 2]
    A[:, 1, 0], A[:, 1, 1], A[:, 1, 2] = q[:, 1], q[:, 3], q[:, 4]
    A[:, 2, 0], A[:, 2, 1], A[:, 2, 2] = q[:, 2], q[:, 4], q[:, 5]
    D, V = jacobi3(A)
    lam = [D[:, 0, 0], D[:, 1, 1], D[:, 2, 2]]
    L = lam[0].copy()
    L = np.where(lam[1] > L, lam[1], L)
    L = np.where(lam[2] > L, lam[2], L)
    use = L > 0.0
    m0, m1, m2 = mean[:, 0], mean[:, 1], mean[:, 2]
    r = [(-q[:, 6 + a]) - ((A[:, a, 0] * m0 + A[:, a, 1] * m1) + A[:, a, 2] * m2)
         for a in range(3)]
    thr = rank_tol * L
    for i in range(3):
        sel = use & (lam[i] > thr)
        g = ((V[:, 0, i] * r[0] + V[:, 1, i] * r[1]) + V[:, 2, i] * r[2]) / lam[i]
        for a in range(3):
            x[sel, a] = x[sel, a] + g[sel] * V[sel, a, i]
    ok = np.all(np.isfinite(x), axis=1) & np.all(cells(x, origin, cell) == want, axis=1)
    fallback = use & ~ok
    x[fallback] = mean[fallback]
    return x, fallback


def simplify(vertices, faces, origin, cell, dims, placement=QUADRIC, rank_tol=1e-3):
    """The seven steps of include/rsamd.h.  Returns a dict: vertices (Nc, 3), faces (Nk, 3)
    int32, vmap (Nv,) int32, fmap (Nf,) int32, quadrics (Nc, 10), mean (Nc, 3), keys (Nc,) and
    info, a dict of INFO_KEYS.  The clusters no surviving face names are kept."""
    v = np.ascontiguousarray(vertices, dtype=np.float64).reshape(-1, 3)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    origin = np.asarray(origin, dtype=np.float64)
    cell, rank_tol = float(cell), float(rank_tol)
    placement = PLACEMENTS.get(placement, placement)
    d0, d1, d2 = (int(d) for d in dims)
    assert min(d0, d1, d2) >= 1 and d0 * d1 * d2 <= MAX_CELLS
    nv, nf = len(v), len(f)
    if nv == 0:
        return {"vertices": np.zeros((0, 3)), "faces": np.zeros((0, 3), np.int32),
                "vmap": np.zeros(0, np.int32), "fmap": np.zeros(0, np.int32),
                "quadrics": np.zeros((0, 10)), "mean": np.zeros((0, 3)),
                "keys": np.zeros(0, np.int64), "info": dict.fromkeys(INFO_KEYS, 0)}
    with np.errstate(all="ignore"):
        # 1, 2: cells and clusters
        idx = cells(v, origin, cell)
        assert np.all(idx >= 0.0) and np.all(idx <= np.array([d0, d1, d2]) - 1.0)
        i = idx.astype(np.int64)
        key = (i[:, 2] * d1 + i[:, 1]) * d0 + i[:, 0]
        keys, vmap = np.unique(key, return_inverse=True)
        vmap = vmap.reshape(-1)
        nc = len(keys)
        want = np.stack((keys % d0, keys // d0 % d1, keys // d0 // d1), axis=1).astype(np.float64)
        # 3: the mean, in ascending vertex index
        sums, count = _ordered_sums(vmap, np.arange(nv), v, nc)
        mean = sums / count[:, None].astype(np.float64)
        # 4: the quadric, over the distinct (cluster, face) pairs in ascending face index
        xa, xb, xc = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
        u, w = xb - xa, xc - xa
        n0 = u[:, 1] * w[:, 2] - u[:, 2] * w[:, 1]
        n1 = u[:, 2] * w[:, 0] - u[:, 0] * w[:, 2]
        n2 = u[:, 0] * w[:, 1] - u[:, 1] * w[:, 0]
        d = -((n0 * xa[:, 0] + n1 * xa[:, 1]) + n2 * xa[:, 2])
        terms = np.stack((n0 * n0, n0 * n1, n0 * n2, n1 * n1, n1 * n2, n2 * n2,
                          n0 * d, n1 * d, n2 * d, d * d), axis=1).reshape(nf, 10)
        cl = vmap[f].reshape(nf, 3)
        pairs = np.unique(np.stack((cl.reshape(-1), np.repeat(np.arange(nf), 3)), axis=1),
                          axis=0).reshape(-1, 2)
        quad, _ = _ordered_sums(pairs[:, 0], pairs[:, 1], terms[pairs[:, 1]], nc)
        # 5: the position
        x, fallback = positions(mean, quad, want, origin, cell, placement, rank_tol)
    # 6: the faces
    degenerate = (cl[:, 0] == cl[:, 1]) | (cl[:, 1] == cl[:, 2]) | (cl[:, 0] == cl[:, 2])
    fmap = np.full(nf, -1, dtype=np.int32)
    alive = np.flatnonzero(~degenerate)
    sets = np.sort(cl[alive], axis=1)
    sets = sets.reshape(-1, 3)
    first = np.unique(sets, axis=0, return_index=True)[1] if len(alive) else np.zeros(0, int)
    kept = np.sort(alive[first])                     # the lowest index of every set, in order
    fmap[alive] = -2
    fmap[kept] = np.arange(len(kept), dtype=np.int32)
    longest = max(int(np.bincount(b).max()) if len(b) else 0
                  for b in (vmap, cl.reshape(-1), sets[:, 0]))
    info = {"clusters": nc, "fallbacks": int(fallback.sum()),
            "degenerate_faces": int(degenerate.sum()),
            "duplicate_faces": int(len(alive) - len(kept)), "longest_row": longest}
    return {"vertices": x, "faces": cl[kept].astype(np.int32).reshape(-1, 3),
            "vmap": vmap.astype(np.int32), "fmap": fmap, "quadrics": quad, "mean": mean,
            "keys": keys, "info": info}


def unreferenced(res):
    """The mask (Nc,) of the clusters no surviving face names."""
    named = np.zeros(len(res["vertices"]), dtype=bool)
    named[res["faces"].reshape(-1)] = True
    return ~named


def drop_unreferenced(res):
    """(vertices, faces, vmap, quadrics) after the clusters no surviving face names are removed:
    ``mesh_ref.compact`` and vmap composed with its map, as ``surface.simplify`` does."""
    keep = ~unreferenced(res)
    if keep.all():
        return res["vertices"], res["faces"], res["vmap"], res["quadrics"]
    vo, fo, cmap = mesh_ref.compact(res["vertices"], res["faces"], keep)
    return vo, fo, cmap[res["vmap"]], res["quadrics"][keep]


def nonmanifold_edges(faces):
    """The number of undirected edges that are not in exactly two faces."""
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    e = np.sort(np.concatenate((f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]])), axis=1)
    if not len(e):
        return 0
    return int(np.sum(np.unique(e, axis=0, return_counts=True)[1] != 2))
