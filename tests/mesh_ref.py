"""The mesh clean-up calls (rs_mesh_components, rs_mesh_compact, rs_mesh_smooth; include/rsamd.h)
restated in numpy and scipy.  Every result is unique, so the GPU is compared with these bit for
bit.

The smoothing sum: ``np.add.at`` adds its operands one after the other in index order, so on
directed edges sorted by (v, u) it forms ((x_u1 + x_u2) + x_u3) + ..., the contract's order.  It
starts from 0.0 where the contract starts from the first term; 0.0 + x is x bit for bit except
for x = -0.0, and a sum that is -0.0 in one and +0.0 in the other gives the same
x_v + f (s / n - x_v) in every case: with x_v != 0 the difference is -x_v either way, and with
x_v = +-0 the last addition has a +0.0 operand or result in both.
"""
import numpy as np
import scipy.sparse
import scipy.sparse.csgraph


def _faces(faces):
    return np.asarray(faces, dtype=np.int64).reshape(-1, 3)


def components(faces, n_vertices):
    """(label, size, count): label[v] the smallest vertex index of v's component, size[v] the
    faces of that component, count the number of components, vertices in no face included."""
    f = _faces(faces)
    n = int(n_vertices)
    rows = np.concatenate((f[:, 0], f[:, 0]))
    cols = np.concatenate((f[:, 1], f[:, 2]))
    g = scipy.sparse.coo_matrix((np.ones(len(rows), np.int8), (rows, cols)), shape=(n, n))
    count, comp = scipy.sparse.csgraph.connected_components(g, directed=False)
    least = np.full(count, n, np.int64)
    np.minimum.at(least, comp, np.arange(n))
    label = least[comp] if n else np.zeros(0, np.int64)
    per = np.bincount(label[f[:, 0]], minlength=n) if n else np.zeros(0, np.int64)
    size = per[label] if n else per
    return label.astype(np.int32), size.astype(np.int32), int(count)


def compact(vertices, faces, keep):
    """(vertices, faces, vmap) with the vertices where keep is false dropped."""
    v = np.asarray(vertices, dtype=np.float64).reshape(-1, 3)
    f = _faces(faces)
    keep = np.asarray(keep).astype(bool)
    new = np.cumsum(keep) - 1
    vmap = np.where(keep, new, -1).astype(np.int32)
    fk = keep[f].all(axis=1) if len(f) else np.zeros(0, bool)
    return v[keep].copy(), vmap[f[fk]].astype(np.int32).reshape(-1, 3), vmap


def rows(faces):
    """The sorted distinct directed edges (v, u), u != v, and how often each occurs in the rows:
    per face corner that names v, the face's other two indices."""
    f = _faces(faces)
    e = np.concatenate([f[:, [i, j]] for i in range(3) for j in range(3) if i != j])
    e = e[e[:, 0] != e[:, 1]]
    if not len(e):
        return np.zeros((0, 2), np.int64), np.zeros(0, np.int64)
    return np.unique(e, axis=0, return_counts=True)


def boundary(faces, n_vertices):
    """v ends a boundary edge: some u occurs exactly once in its row."""
    e, n = rows(faces)
    out = np.zeros(int(n_vertices), bool)
    out[e[n == 1, 0]] = True
    return out


def smooth(vertices, faces, iterations=10, lam=0.5, mu=-0.53, fixed=None, pin_boundary=True):
    x = np.array(vertices, dtype=np.float64).reshape(-1, 3)
    nv = len(x)
    e, _ = rows(faces)
    deg = np.bincount(e[:, 0], minlength=nv)
    still = deg == 0
    if fixed is not None:
        still |= np.asarray(fixed).astype(bool)
    if pin_boundary:
        still |= boundary(faces, nv)
    move = ~still
    for it in range(2 * int(iterations)):
        f = mu if it % 2 else lam
        s = np.zeros_like(x)
        np.add.at(s, e[:, 0], x[e[:, 1]])
        new = x.copy()
        new[move] = x[move] + f * (s[move] / deg[move, None].astype(np.float64) - x[move])
        x = new
    return x


def keep_components(label, size, n_faces, min_faces=None, keep_largest=None, min_fraction=None):
    """The policy of surface.remove_small, restated with plain loops."""
    roots = [int(v) for v in range(len(label)) if label[v] == v and size[v] > 0]
    ok = set(roots)
    if min_faces is not None:
        ok &= {r for r in roots if size[r] >= min_faces}
    if min_fraction is not None:
        ok &= {r for r in roots if size[r] >= min_fraction * n_faces}
    if keep_largest is not None:
        ok &= set(sorted(roots, key=lambda r: (-int(size[r]), r))[:keep_largest])
    return np.array([int(l) in ok for l in label], dtype=bool)


def radial_rms(vertices, centre, r):
    d = np.linalg.norm(np.asarray(vertices) - np.asarray(centre, dtype=np.float64), axis=1) - r
    return float(np.sqrt(np.mean(d * d)))
