"""Procedural meshes for the mesh clean-up tests.  Everything is seeded, computed once, cached and
read-only; the volumes go through the numpy marching tetrahedra of tests/surface_ref.py.
"""
import functools

import numpy as np

import surface_fixture as sfx
import surface_ref

ORDERS = ("ascending", "descending", "permuted")
TWO_SPHERES = ((9.5, 9.6, 9.45), 6.7), ((19.3, 19.4, 19.2), 1.7)
NOISE_SIGMA = 0.15


def _freeze(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def renumber(vertices, faces, new_of_old):
    """The same mesh with vertex v called new_of_old[v]."""
    new_of_old = np.asarray(new_of_old)
    out = np.empty_like(vertices)
    out[new_of_old] = vertices
    return out, new_of_old[faces].astype(np.int32)


@functools.lru_cache(maxsize=None)
def chain(n, order="ascending", seed=0):
    """A strip of n triangles (i, i + 1, i + 2) on n + 2 vertices, numbered along the strip,
    against it, or by a seeded permutation: one component of diameter n / 2."""
    i = np.arange(n)
    faces = np.stack((i, i + 1, i + 2), axis=1).astype(np.int32)
    k = np.arange(n + 2)
    vertices = np.stack((0.5 * k, (k % 2).astype(np.float64), 0.01 * (k % 7)), axis=1)
    if order == "descending":
        vertices, faces = renumber(vertices, faces, k[::-1].copy())
    elif order == "permuted":
        vertices, faces = renumber(vertices, faces, np.random.RandomState(seed).permutation(n + 2))
    elif order != "ascending":
        raise ValueError(order)
    return _freeze(vertices, faces)


@functools.lru_cache(maxsize=None)
def fan(degree):
    """An open fan: hub 0, rim 1..degree, faces (0, i, i + 1).  The hub has `degree` neighbours."""
    t = np.linspace(0.0, 1.7 * np.pi, degree)
    rim = np.stack((np.cos(t), np.sin(t), 0.1 * np.sin(5.0 * t)), axis=1)
    vertices = np.concatenate(([[0.013, -0.021, 0.6]], rim))
    i = np.arange(1, degree)
    faces = np.stack((np.zeros_like(i), i, i + 1), axis=1).astype(np.int32)
    return _freeze(vertices, faces)


@functools.lru_cache(maxsize=None)
def two_sphere_volume():
    """A 24^3 volume, the minimum of two sphere distances: a large shell and a small floater."""
    X = surface_ref.node_positions((0.0, 0.0, 0.0), 1.0, (24, 24, 24))
    d = [np.linalg.norm(X - np.asarray(c), axis=-1) - r for c, r in TWO_SPHERES]
    tsdf = np.minimum(d[0], d[1]).astype(np.float32)
    return _freeze(tsdf, np.full((24, 24, 24), 2.0, np.float32))


@functools.lru_cache(maxsize=None)
def two_sphere_mesh():
    tsdf, weight = two_sphere_volume()
    return _freeze(*surface_ref.extract(tsdf, weight, np.zeros(3), 1.0, 1.0))


@functools.lru_cache(maxsize=None)
def noisy_sphere():
    """The s16 sphere mesh with radial Gaussian noise of NOISE_SIGMA voxels: (noisy vertices,
    faces, clean vertices)."""
    v, f = sfx.reference_extract("s16")
    _, c, _ = sfx.SPHERES["s16"]
    d = v - np.asarray(c)
    unit = d / np.linalg.norm(d, axis=1, keepdims=True)
    noisy = v + NOISE_SIGMA * np.random.RandomState(3).standard_normal(len(v))[:, None] * unit
    return _freeze(noisy, f, v)


@functools.lru_cache(maxsize=None)
def interleaved_spheres(seed=5):
    """Two s12 sphere meshes, the second shifted, their vertices interleaved by a seeded
    permutation: two components whose indices alternate at random."""
    v, f = sfx.reference_extract("s12")
    vertices = np.concatenate((v, v + np.array([20.0, 0.0, 0.0])))
    faces = np.concatenate((f, f + len(v))).astype(np.int32)
    perm = np.random.RandomState(seed).permutation(len(vertices))
    return _freeze(*renumber(vertices, faces, perm))


def small_meshes():
    """name -> (faces, n_vertices): the corner cases of the components."""
    f = lambda *rows: np.array(rows, dtype=np.int32).reshape(-1, 3)  # noqa: E731
    return {
        "no_face": (f(), 5),
        "one_face": (f((0, 1, 2)), 3),
        "shared_vertex": (f((0, 1, 2), (2, 3, 4)), 5),
        "disjoint": (f((0, 1, 2), (3, 4, 5)), 6),
        "repeated_index": (f((3, 3, 1), (0, 2, 2), (4, 4, 4)), 5),
        "unreferenced_middle": (f((0, 1, 5), (5, 4, 6), (7, 8, 9)), 10),
    }


def plane_mesh(name):
    return sfx.reference_mesh(name)


def random_mesh():
    return sfx.reference_extract("random")
