"""Volumes for the surface stage: the dense fixture's two planes fused into a small TSDF volume,
analytic spheres and a seeded random volume.  Every reference result is computed once by
tests/surface_ref.py, cached and read-only.
"""
import functools

import numpy as np

import dense_fixture
import surface_ref

VOXEL = float(np.sqrt(0.00221))
DIMS = (26, 22, 30)
ORIGIN = np.array([-np.sqrt(0.5), -np.sqrt(0.245), np.sqrt(11.5)])
TRUNC = 0.2
MIN_WEIGHT = 2.0
SCENES = ("fronto", "slanted")
# (n, centre, r): two generic spheres and one with nodes exactly on the surface
SPHERES = {"s12": (12, (5.3, 5.6, 5.45), 4.3), "s16": (16, (7.5, 7.5, 7.5), 5.7),
           "s10_zero": (10, (4.0, 4.0, 4.0), 3.0)}
RANDOM_DIMS = (9, 10, 11)


def _freeze(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def plane_of(name):
    return {"fronto": dense_fixture.FRONTO, "slanted": dense_fixture.SLANTED}[name]


@functools.lru_cache(maxsize=None)
def reference_volume(name):
    """(tsdf, weight, margins) of a scene's three exact depth maps."""
    _, cams, depth = dense_fixture.scene(name)
    m = {}
    tsdf, weight = surface_ref.integrate(depth, cams, dense_fixture.K, ORIGIN, VOXEL, DIMS, TRUNC,
                                         margins=m)
    _freeze(tsdf, weight)
    return tsdf, weight, m


@functools.lru_cache(maxsize=None)
def reference_mesh(name):
    tsdf, weight, _ = reference_volume(name)
    return _freeze(*surface_ref.extract(tsdf, weight, ORIGIN, VOXEL, MIN_WEIGHT))


def plane_distance(vertices, name):
    n, c = plane_of(name)
    return np.abs(vertices @ n - c)


@functools.lru_cache(maxsize=None)
def sphere(name):
    n, c, r = SPHERES[name]
    return _freeze(*surface_ref.sphere_volume(n, c, r))


@functools.lru_cache(maxsize=None)
def random_volume():
    rs = np.random.RandomState(20)
    tsdf = rs.uniform(-1.0, 1.0, RANDOM_DIMS).astype(np.float32)
    weight = (rs.uniform(0.0, 1.0, RANDOM_DIMS) < 0.9).astype(np.float32)
    return _freeze(tsdf, weight)


@functools.lru_cache(maxsize=None)
def extract_cases():
    """name -> (tsdf, weight, origin, voxel, min_weight) of the analytic volumes."""
    cases = {k: sphere(k) + (np.zeros(3), 1.0, 1.0) for k in SPHERES}
    cases["random"] = random_volume() + (np.array([0.25, -1.5, 3.0]), 0.5, 1.0)
    return cases


@functools.lru_cache(maxsize=None)
def reference_extract(name):
    tsdf, weight, origin, voxel, mw = extract_cases()[name]
    return _freeze(*surface_ref.extract(tsdf, weight, origin, voxel, mw))


def sphere_radial_error(vertices, name):
    _, c, r = SPHERES[name]
    return np.abs(np.linalg.norm(vertices - np.asarray(c), axis=1) - r)
