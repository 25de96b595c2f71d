"""The simplification's definition, checked on the numpy restatement alone (tests/simplify_ref.py
on the meshes of tests/simplify_fixture.py); tests/test_gpu_simplify.py then holds the device to
the restatement bit for bit.

Bars.
  * Cube and plane: the quadric's minimum is exact there (the corner; any point of the plane), and
    the solve divides by eigenvalues within 1 / rank_tol = 1e3 of the largest, so the error is
    rounding (1e-16 relative) times at most that condition number and the handful of operations:
    1e-9 of the mesh's size leaves four orders of margin.
  * Moved distance: a vertex and the cluster that replaces it lie in one cell, so they differ by
    at most ``cell`` per axis; 1e-12 relative covers the rounding of the cell's own bounds.
"""
import numpy as np
import pytest

import mesh_fixture as mfx
import simplify_fixture as sx
import simplify_ref as ref
import surface_fixture as sfx

BRANCH_CASES = ("two_spheres_3.0", "two_spheres_1.5", "random_2.0")


def _run(v, f, cell, origin=None, placement="quadric", rank_tol=1e-3):
    origin, dims = ref.grid(v, cell, origin)
    return ref.simplify(v, f, origin, cell, dims, placement, rank_tol)


def test_cube_corners_and_planes():
    v, f = sx.cube()
    res = sx.reference("cube")
    assert res["info"]["clusters"] == 98          # the surface cells of a 5 x 5 x 5 grid
    corner_vertex = [int(np.flatnonzero(np.all(v == c, axis=1))[0]) for c in sx.cube_corners()]
    at = res["vertices"][res["vmap"][corner_vertex]]
    err = np.abs(at - sx.cube_corners()).max()
    plane = sx.cube_plane_distance(res["vertices"]).max()
    print(f"cube, quadric: corner error {err:.3g}, plane distance {plane:.3g}, "
          f"info {res['info']}")
    assert err <= 1e-9 * sx.CUBE_SIDE
    assert plane <= 1e-9 * sx.CUBE_SIDE
    assert res["info"]["fallbacks"] == 0
    mean = sx.reference("cube", placement="mean")
    merr = np.linalg.norm(mean["vertices"][mean["vmap"][corner_vertex]] - sx.cube_corners(),
                          axis=1)
    print(f"cube, mean: corner error {merr.min():.3g} .. {merr.max():.3g}")
    assert merr.min() > 0.1 * sx.CUBE_CELL
    assert np.array_equal(mean["faces"], res["faces"]) and np.array_equal(mean["vmap"], res["vmap"])


@pytest.mark.parametrize("name", sfx.SCENES)
def test_plane_stays_a_plane(name):
    """The fixture's vertices come out of a truncated float32 volume and miss the plane by up to
    1e-2; projected onto it they are an exact plane mesh of the same connectivity."""
    v, f = mfx.plane_mesh(name)
    n, c = sfx.plane_of(name)
    n = np.asarray(n, dtype=np.float64)
    exact = v - np.outer(v @ n - c, n) / (n @ n)
    extent = np.linalg.norm(exact.max(axis=0) - exact.min(axis=0))
    res = _run(exact, f, 3.0 * sfx.VOXEL)
    d_in = np.abs(exact @ n - c).max() / np.linalg.norm(n)
    d_out = np.abs(res["vertices"] @ n - c).max() / np.linalg.norm(n)
    print(f"{name}: {len(v)} -> {len(res['vertices'])} vertices, extent {extent:.3g}, distance "
          f"to the plane in {d_in:.3g}, out {d_out:.3g}, info {res['info']}")
    assert len(res["vertices"]) < len(v) / 4
    assert d_out <= 1e-9 * extent


@pytest.mark.parametrize("placement", ["quadric", "mean"])
@pytest.mark.parametrize("name", sorted(sx.cases()))
def test_no_vertex_leaves_its_cell(name, placement):
    v, _, cell, _ = sx.cases()[name]
    res = sx.reference(name, placement)
    moved = np.abs(res["vertices"][res["vmap"]] - v)
    assert moved.shape == v.shape
    assert moved.max(initial=0.0) <= cell * (1.0 + 1e-12)


def test_every_branch_is_taken():
    """Fall-backs, duplicates, degenerate faces and unreferenced clusters each occur on the
    fixtures; the counts are the restatement's own (DESIGN.md section 20 records them)."""
    seen = dict.fromkeys(("fallbacks", "duplicate_faces", "degenerate_faces", "unreferenced"), 0)
    for name in BRANCH_CASES:
        res = sx.reference(name)
        info = dict(res["info"], unreferenced=int(ref.unreferenced(res).sum()))
        print(name, len(res["faces"]), "faces", info)
        for k in seen:
            seen[k] = max(seen[k], info[k])
    assert all(n > 0 for n in seen.values()), seen


@pytest.mark.parametrize("name", sorted(sx.cases()))
def test_numbering_and_maps(name):
    v, f, cell, origin = sx.cases()[name]
    res = sx.reference(name)
    origin, dims = ref.grid(v, cell, origin)
    vmap, fmap, out = res["vmap"], res["fmap"], res["faces"]
    # clusters ascend by key, and every vertex is in the cluster of its cell
    assert np.all(np.diff(res["keys"]) > 0)
    i = np.floor((v - origin) / cell).astype(np.int64)
    assert np.array_equal(res["keys"][vmap], (i[:, 2] * dims[1] + i[:, 1]) * dims[0] + i[:, 0])
    assert np.array_equal(np.unique(vmap), np.arange(len(res["vertices"])))
    # survivors keep their order and their corner order
    kept = np.flatnonzero(fmap >= 0)
    assert np.array_equal(fmap[kept], np.arange(len(out)))
    assert np.array_equal(out, vmap[f[kept]])
    cl = vmap[np.asarray(f, dtype=np.int64)].reshape(-1, 3)
    degenerate = (cl[:, 0] == cl[:, 1]) | (cl[:, 1] == cl[:, 2]) | (cl[:, 0] == cl[:, 2])
    assert np.array_equal(fmap == -1, degenerate)
    # a duplicate has the cluster set of an earlier survivor, and no two survivors share a set
    sets = {tuple(sorted(row)): k for k, row in zip(kept, cl[kept])}
    assert len(sets) == len(kept)
    for k in np.flatnonzero(fmap == -2):
        assert sets[tuple(sorted(cl[k]))] < k
    assert set(np.unique(fmap[fmap < 0])) <= {-1, -2}
    assert res["info"]["clusters"] == len(res["vertices"])
    assert res["info"]["degenerate_faces"] == int((fmap == -1).sum())
    assert res["info"]["duplicate_faces"] == int((fmap == -2).sum())


def test_cluster_and_cell_counts_are_the_edges_meant():
    for n in sx.CLUSTER_COUNTS:
        assert sx.reference(f"chain_{n}")["info"]["clusters"] == n
    for n in sx.CELL_COUNTS:
        v, _, cell, origin = sx.cases()[f"sparse_{n}"]
        assert ref.grid(v, cell, origin)[1] == (n, 1, 1)
        assert sx.reference(f"sparse_{n}")["info"]["clusters"] == 5
    for n in sx.ROW_LENGTHS:
        info = sx.reference(f"star_{n}")["info"]
        assert info["longest_row"] == n and info["duplicate_faces"] == n - 1
    assert 1000 < sx.reference("random_3.0")["info"]["longest_row"] < 2500
    one = sx.reference("one_cell")
    assert one["info"]["clusters"] == 1 and len(one["faces"]) == 0
    assert one["info"]["longest_row"] == 3 * len(sx.cases()["one_cell"][1]) <= 15000


def test_by_hand():
    # exactly on a cell face: the upper cell
    res = sx.reference("on_cell_faces")
    want = [(1, 0, 0), (0, 2, 0), (0, 0, 3), (0, 0, 0), (2, 2, 2)]
    dims = ref.grid(*[sx.cases()["on_cell_faces"][k] for k in (0, 2, 3)])[1]
    assert dims == (3, 3, 4)
    keys = [(z * dims[1] + y) * dims[0] + x for x, y, z in want]
    assert np.array_equal(res["keys"][res["vmap"]], keys)
    # the default origin puts the largest coordinate on the last cell's lower face
    v, f, cell, _ = sx.cases()["default_origin_top"]
    origin, dims = ref.grid(v, cell)
    assert dims == (5, 5, 3) and np.array_equal(origin, [0.25, 0.5, 1.0])
    res = sx.reference("default_origin_top")
    assert res["keys"][res["vmap"][3]] == dims[0] * dims[1] * dims[2] - 1
    # opposite orientation over the same three cells: the lower index survives, as it was
    res = sx.reference("opposite_pair")
    assert np.array_equal(res["fmap"], [0, -2]) and np.array_equal(res["faces"], [[0, 1, 2]])
    assert res["info"]["duplicate_faces"] == 1
    # hub and rim in one cell: no face
    res = sx.reference("fan_in_one_cell")
    assert len(res["faces"]) == 0 and np.all(res["fmap"] == -1) and len(res["vertices"]) == 1
    # a zero-area face and faces with repeated indices still enter the quadrics
    res = sx.reference("zero_area")
    assert res["info"]["degenerate_faces"] == 0 and len(res["faces"]) == 2
    rep = sx.reference("repeated_indices")
    assert np.array_equal(rep["fmap"], [-1, -1, 0, -1])
    assert np.array_equal(rep["quadrics"], sx.reference("one_face")["quadrics"])   # they add 0


def test_quadrics_against_plain_sums():
    """The ten numbers against float sums in another order: equal to rounding."""
    v, f, cell, origin = sx.cases()["two_spheres_3.0"]
    res = sx.reference("two_spheres_3.0")
    n = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
    d = -np.einsum("ij,ij->i", n, v[f[:, 0]])
    want = np.zeros_like(res["quadrics"])
    cl = res["vmap"][f]
    for k in range(len(f)):
        t = np.array([n[k, 0] * n[k, 0], n[k, 0] * n[k, 1], n[k, 0] * n[k, 2], n[k, 1] * n[k, 1],
                      n[k, 1] * n[k, 2], n[k, 2] * n[k, 2], n[k, 0] * d[k], n[k, 1] * d[k],
                      n[k, 2] * d[k], d[k] * d[k]])
        for c in set(cl[k]):
            want[c] += t
    assert np.allclose(res["quadrics"], want, rtol=1e-12, atol=1e-12 * np.abs(want).max())


def test_drop_unreferenced_composes_the_maps():
    res = sx.reference("two_spheres_3.0")
    gone = ref.unreferenced(res)
    assert gone.any()
    vo, fo, vmap, quad = ref.drop_unreferenced(res)
    assert len(vo) == len(res["vertices"]) - gone.sum() == len(quad)
    assert np.array_equal(vmap < 0, gone[res["vmap"]])
    live = vmap >= 0
    assert np.array_equal(vo[vmap[live]], res["vertices"][res["vmap"][live]])
    assert np.array_equal(vo[fo], res["vertices"][res["faces"]])
