"""Meshes for the simplification tests, and the restatement's result for each, computed once.
Everything is seeded, cached and read-only.  A case is (vertices, faces, cell, origin or None);
the grid's dims follow from it as ``surface.simplify_grid`` defines them.
"""
import functools

import numpy as np

import mesh_fixture as mfx
import simplify_ref as ref
import surface_fixture as sfx

CUBE_SIDE, CUBE_QUADS, CUBE_CELL = 8.0, 16, 2.0
# no cube vertex (a multiple of 0.5) lies on a cell face (origin + 2 k)
CUBE_ORIGIN = (-0.7, -0.9, -1.1)
CLUSTER_COUNTS = (63, 64, 65, 2047, 2048, 2049, 4097)
CELL_COUNTS = (2047, 2048, 2049)
ROW_LENGTHS = (1, 24, 25, 63, 64, 65)
SPHERE_CELLS = (3.0, 1.5)
RANDOM_CELL = 2.0


def _freeze(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def cube():
    """The surface of the cube [0, side]^3, CUBE_QUADS x CUBE_QUADS quads per side, each cut
    into two triangles that face outwards; the vertices on edges and corners are shared."""
    n, h = CUBE_QUADS, CUBE_SIDE / CUBE_QUADS
    index, verts, faces = {}, [], []

    def vid(p):
        if p not in index:
            index[p] = len(verts)
            verts.append(p)
        return index[p]

    for axis in range(3):
        a1, a2 = (axis + 1) % 3, (axis + 2) % 3
        for side in (0, n):
            for i in range(n):
                for j in range(n):
                    def at(di, dj):
                        p = [0, 0, 0]
                        p[axis], p[a1], p[a2] = side, i + di, j + dj
                        return vid(tuple(p))
                    q = (at(0, 0), at(1, 0), at(1, 1), at(0, 1))   # normal +axis
                    if side == 0:
                        q = q[::-1]
                    faces += [(q[0], q[1], q[2]), (q[0], q[2], q[3])]
    return _freeze(np.array(verts, dtype=np.float64) * h, np.array(faces, dtype=np.int32))


def cube_corners():
    s = CUBE_SIDE
    return np.array([(x, y, z) for x in (0.0, s) for y in (0.0, s) for z in (0.0, s)])


def cube_plane_distance(x):
    """Per point, the distance to the nearest of the cube's six face planes."""
    x = np.asarray(x)
    return np.minimum(np.abs(x), np.abs(x - CUBE_SIDE)).min(axis=1)


@functools.lru_cache(maxsize=None)
def star(n, seed=0):
    """n vertices in one cell, each joined to the same two far vertices, vertices and faces in
    a seeded order: with cell 1 and origin 0 the vertex row, the corner rows and the face row of
    the clusters all have n items, and n - 1 faces are duplicates of the first."""
    rs = np.random.RandomState(1000 + n + seed)
    inner = 0.05 + 0.9 * rs.uniform(size=(n, 3))
    v = np.concatenate((inner, [[3.5, 0.5, 0.5], [0.5, 3.5, 0.5]]))
    i = np.arange(n)
    f = np.stack((i, np.full(n, n), np.full(n, n + 1)), axis=1)
    f[1::2] = f[1::2, ::-1]                          # every other face the other way round
    f = np.array([np.roll(row, k % 3) for k, row in enumerate(f)]).reshape(-1, 3)
    v, f = mfx.renumber(v, f, rs.permutation(n + 2))
    return _freeze(v, f[rs.permutation(n)].astype(np.int32))


def _f(*rows):
    return np.array(rows, dtype=np.int32).reshape(-1, 3)


def hand_made():
    """name -> case.  Cell 1 and origin 0 unless the case is about the default origin."""
    o = np.zeros(3)
    tri = np.array([[0.2, 0.3, 0.1], [2.6, 0.4, 0.2], [0.5, 2.7, 1.3]])
    return {
        "no_face": (np.array([[0.5, 0.5, 0.5], [1.5, 0.2, 0.1], [0.6, 0.4, 0.3]]), _f(), 1.0, o),
        "one_face": (tri, _f((0, 1, 2)), 1.0, o),
        "unreferenced_vertex": (np.concatenate((tri, [[4.5, 4.5, 4.5]])), _f((0, 1, 2)), 1.0, o),
        "repeated_indices": (tri, _f((0, 0, 1), (2, 2, 2), (0, 1, 2), (1, 2, 1)), 1.0, o),
        "zero_area": (np.concatenate((tri, [[1.4, 0.35, 0.15]])), _f((0, 3, 1), (0, 1, 2)),
                      1.0, o),
        # a vertex exactly on a cell face belongs to the upper cell
        "on_cell_faces": (np.array([[1.0, 0.5, 0.5], [0.5, 2.0, 0.5], [0.5, 0.5, 3.0],
                                    [0.0, 0.0, 0.0], [2.0, 2.0, 2.0]]),
                          _f((0, 1, 2), (3, 0, 1), (4, 2, 1)), 1.0, o),
        # two faces over the same three cells, opposite orientation: the first stays
        "opposite_pair": (np.array([[0.5, 0.5, 0.5], [1.5, 0.5, 0.5], [0.5, 1.5, 0.5],
                                    [0.6, 0.4, 0.5], [1.4, 0.6, 0.5], [0.4, 1.6, 0.5]]),
                          _f((0, 1, 2), (5, 4, 3)), 1.0, o),
        # hub and rim of a fan in one cell: no face survives
        "fan_in_one_cell": (np.asarray(mfx.fan(9)[0]), np.asarray(mfx.fan(9)[1]), 8.0, None),
        # the default origin: the largest coordinate lies on the last cell's lower face
        "default_origin_top": (np.array([[0.25, 0.5, 1.0], [2.25, 0.5, 1.5], [0.25, 3.5, 1.25],
                                         [4.25, 4.5, 3.0]]),
                               _f((0, 1, 2), (1, 3, 2)), 1.0, None),
    }


@functools.lru_cache(maxsize=None)
def sparse_grid(ncell):
    """A grid of ncell x 1 x 1 cells (cell 1, origin 0) with five of them occupied."""
    x = np.array([0.5, 0.25, 1.5, ncell // 2 + 0.5, ncell - 2 + 0.5, ncell - 0.5])
    v = np.stack((x, np.linspace(0.1, 0.9, 6), np.linspace(0.8, 0.2, 6)), axis=1)
    return _freeze(v, _f((0, 2, 3), (1, 2, 3), (3, 4, 5), (0, 1, 5)))


@functools.lru_cache(maxsize=None)
def permuted_two_spheres(seed=11):
    v, f = mfx.two_sphere_mesh()
    return _freeze(*mfx.renumber(np.asarray(v), np.asarray(f),
                                 np.random.RandomState(seed).permutation(len(v))))


@functools.lru_cache(maxsize=None)
def cases():
    """name -> (vertices, faces, cell, origin or None): every mesh the GPU is compared on."""
    out = dict(hand_made())
    out["cube"] = cube() + (CUBE_CELL, np.array(CUBE_ORIGIN))
    for name in sfx.SCENES:
        out[f"plane_{name}"] = tuple(mfx.plane_mesh(name)) + (3.0 * sfx.VOXEL, None)
    for cell in SPHERE_CELLS:
        out[f"two_spheres_{cell}"] = tuple(mfx.two_sphere_mesh()) + (cell, None)
    out["two_spheres_permuted"] = permuted_two_spheres() + (SPHERE_CELLS[0], None)
    out[f"random_{RANDOM_CELL}"] = tuple(mfx.random_mesh()) + (RANDOM_CELL, None)
    out["random_3.0"] = tuple(mfx.random_mesh()) + (3.0, None)      # rows of about 1 500
    for n in CLUSTER_COUNTS:      # a vertex per cell, every x on a cell face
        order = "permuted" if n % 2 else "ascending"
        out[f"chain_{n}"] = tuple(mfx.chain(n - 2, order, seed=n)) + (0.5, None)
    out["chain_clustered"] = tuple(mfx.chain(3000, "permuted", seed=3)) + (1.7, None)
    for n in CELL_COUNTS:
        out[f"sparse_{n}"] = sparse_grid(n) + (1.0, np.zeros(3))
    for n in ROW_LENGTHS:
        out[f"star_{n}"] = star(n) + (1.0, np.zeros(3))
    out["one_cell"] = tuple(sfx.reference_extract("s12")) + (64.0, None)
    return out


@functools.lru_cache(maxsize=None)
def reference(name, placement="quadric", rank_tol=1e-3):
    """The restatement's result for a case (clusters no face names kept), its arrays frozen."""
    v, f, cell, origin = cases()[name]
    origin, dims = ref.grid(v, cell, origin)
    res = ref.simplify(v, f, origin, cell, dims, placement, rank_tol)
    _freeze(*(a for a in res.values() if isinstance(a, np.ndarray)))
    return res
