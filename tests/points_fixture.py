"""Clouds with normals, volumes and reference results for tests/test_points_cpu.py and
tests/test_gpu_points.py.  Test infrastructure; every reference is computed once, shared and
read-only.

  * plane()    a 9 x 9 lattice of spacing 0.125 in z = 0, centred on the origin, normals
               (0, 0, 1), radius 0.3,
               k = 16, nodes from -0.25 in steps of 0.0625, dims (9, 9, 9): full of ties, all 729
               nodes defined, 355 saturated, max |f - z| = 8.3e-17
  * sphere()   cloud_fixture.sphere() with normals p / |p|, voxel 0.1, radius 0.25, k = 16,
               min_weight 3, bounds(..., margin=0.2): dims (25, 25, 25), 5 732 vertices and
               11 460 faces through surface_ref.extract, closed, Euler characteristic 2, one
               component, max radial error 0.0130 (the small outward bias of IMLS on a curved
               surface), 3 285 nodes saturated.
               Recorded negative: with radius 0.2 the same cloud does not close (Euler
               characteristic -29); radius 0.25 is the smallest tried that does.
  * dino()     the reference's saved cloud through surface.oriented_cloud, voxel 0.05,
               radius 0.2: a demo (6 344 faces in 13 open components), not a quality bar
  * lattice()  the 5 x 5 x 5 integer lattice with normals (0, 0, 1): every d2 exact, neighbours
               exactly on the rim for radius 1 or 2

check_no_ties asserts what a comparison under a permutation of the points needs: no row of the
reference lists (k + 1 wide) holds two equal d2, so the list order, and with it the order of the
sums, cannot depend on the indices.
"""
from __future__ import annotations

import numpy as np

import cloud_fixture as cf
import knn_fixture as kf
import knn_ref as kr
import points_ref as pr
import surface_ref as sr
from tsbb15_amd import surface

_cache = {}


def _frozen(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


def plane():
    if "plane" not in _cache:
        g = (np.arange(9) - 4) * 0.125
        pts = np.stack(np.meshgrid(g, g, [0.0], indexing="ij"), axis=-1).reshape(-1, 3)
        normals = np.tile([[0.0, 0.0, 1.0]], (len(pts), 1))
        _cache["plane"] = _frozen(dict(
            points=np.ascontiguousarray(pts), normals=normals, radius=0.3, k=16,
            origin=np.full(3, -0.25), voxel=0.0625, dims=(9, 9, 9)))
    return _cache["plane"]


def sphere():
    if "sphere" not in _cache:
        pts = np.array(kf.sphere())
        normals = surface.oriented_cloud(pts, pts)[1]          # p / |p| as from_points has it
        origin, dims = surface.bounds(pts, 0.1, margin=0.2)
        _cache["sphere"] = _frozen(dict(points=pts, normals=normals, radius=0.25, k=16,
                                        voxel=0.1, min_weight=3, origin=origin, dims=dims))
    return _cache["sphere"]


def dino():
    if "dino" not in _cache:
        d = cf.dino()
        pts, unit, col, keep = surface.oriented_cloud(d["points"], d["normals"], d["colors"])
        origin, dims = surface.bounds(pts, 0.05, margin=0.1)
        _cache["dino"] = _frozen(dict(points=pts, normals=unit, colors=col, radius=0.2, k=16,
                                      voxel=0.05, min_weight=3, origin=origin, dims=dims,
                                      raw=d, kept=int(keep.sum())))
    return _cache["dino"]


def lattice():
    if "lattice" not in _cache:
        pts = np.array(kf.lattice())
        _cache["lattice"] = _frozen(dict(points=pts,
                                         normals=np.tile([[0.0, 0.0, 1.0]], (len(pts), 1))))
    return _cache["lattice"]


def case(name):
    return {"plane": plane, "sphere": sphere, "dino": dino}[name]()


def volume(name):
    """points_ref.volume of the case: (tsdf, weight, (value, count, saturated))."""
    key = ("volume", name)
    if key not in _cache:
        c = case(name)
        tsdf, weight, (value, count, sat) = pr.volume(c["points"], c["normals"], c["origin"],
                                                      c["voxel"], c["dims"], c["radius"], c["k"])
        for a in (tsdf, weight, value, count, sat):
            a.setflags(write=False)
        _cache[key] = (tsdf, weight, (value, count, sat))
    return _cache[key]


def mesh(name):
    """surface_ref.extract of volume(name) with the case's min_weight: (vertices, faces)."""
    key = ("mesh", name)
    if key not in _cache:
        c = case(name)
        tsdf, weight, _ = volume(name)
        v, f = sr.extract(tsdf, weight, c["origin"], c["voxel"], float(c["min_weight"]))
        v.setflags(write=False)
        f.setflags(write=False)
        _cache[key] = (v, f)
    return _cache[key]


def check_no_ties(name):
    """The smallest gap between consecutive d2 within the k + 1 nearest of every node that has
    two; asserted positive."""
    c = case(name)
    X = sr.node_positions(c["origin"], c["voxel"], c["dims"]).reshape(-1, 3)
    _, d2, count = kr.knn(c["points"], c["k"] + 1, queries=X, max_dist=c["radius"])
    with np.errstate(invalid="ignore"):                       # inf - inf past a list's end
        gaps = np.diff(d2, axis=1)[np.arange(c["k"])[None, :] < (count[:, None] - 1)]
    assert len(gaps) and float(gaps.min()) > 0.0
    return float(gaps.min())


def components(n_vertices, faces):
    """The number of connected components among the vertices that a face names."""
    label = np.arange(n_vertices)
    f = np.asarray(faces, dtype=np.int64)
    e = np.concatenate((f[:, [0, 1]], f[:, [1, 2]]))
    while True:
        low = np.minimum(label[e[:, 0]], label[e[:, 1]])
        new = label.copy()
        np.minimum.at(new, e[:, 0], low)
        np.minimum.at(new, e[:, 1], low)
        new = new[new]
        if np.array_equal(new, label):
            break
        label = new
    return len(np.unique(label[np.unique(f)]))
