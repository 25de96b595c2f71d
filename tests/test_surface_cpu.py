"""The surface stage without a GPU: the restatement's meshes have the properties the definition
promises, the fixture volume keeps clear of every rounding boundary (so that the GPU's flags
may be compared exactly), the compiled case table equals the derived one, the host pieces of
tsbb15_amd.surface work, and every ValueError is raised before a launch."""
import os
import subprocess

import numpy as np
import pytest

import dense_fixture
import surface_fixture as fx
import surface_ref as ref
from tsbb15_amd import surface

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tsbb15-3d-reconstruction-project_amd", "csrc")


@pytest.mark.parametrize("name", fx.SCENES)
def test_fixture_margins(name):
    _, _, m = fx.reference_volume(name)
    print(name, m)
    assert m["round"] >= 1e-9
    assert m["trunc"] >= 1e-9


@pytest.mark.parametrize("name", fx.SCENES)
def test_fixture_mesh(name):
    v, f = fx.reference_mesh(name)
    dist = fx.plane_distance(v, name).max() / fx.VOXEL
    print(name, len(v), len(f), dist)
    assert len(v) > 0 and len(f) > 0
    assert dist <= 0.5
    assert ref.repeated_directed_edges(f) == 0
    assert f.min() >= 0 and f.max() < len(v)


@pytest.mark.parametrize("name", ("s12", "s16"))
def test_sphere(name):
    v, f = fx.reference_extract(name)
    err = fx.sphere_radial_error(v, name).max()
    bound = ref.sphere_bound(fx.SPHERES[name][2])
    print(name, len(v), len(f), err, bound)
    assert ref.is_closed(f)
    assert ref.euler(v, f) == 2
    assert ref.signed_volume(v, f) > 0
    assert err <= bound


def test_sphere_with_nodes_on_the_surface():
    tsdf, _ = fx.sphere("s10_zero")
    assert np.count_nonzero(tsdf == 0.0) > 0
    v, f = fx.reference_extract("s10_zero")
    assert ref.is_closed(f)
    assert ref.euler(v, f) == 2


def test_random_volume():
    v, f = fx.reference_extract("random")
    print(len(v), len(f))
    assert len(v) > 0 and len(f) > 0
    assert ref.repeated_directed_edges(f) == 0
    assert np.array_equal(np.unique(f), np.arange(len(v)))


def test_normals_point_to_the_positive_side():
    """The winding comes from the table: on the sphere every face normal points outwards."""
    v, f = fx.reference_extract("s12")
    c = np.asarray(fx.SPHERES["s12"][1])
    a, b, d = (v[f[:, i]] for i in range(3))
    n = np.cross(b - a, d - a)
    out = (a + b + d) / 3.0 - c
    area = np.linalg.norm(n, axis=1)
    assert np.all(np.einsum("ij,ij->i", n, out)[area > 1e-12] > 0)


def test_compiled_table_equals_derived(tmp_path):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    exe = str(tmp_path / "surface_table_check")
    cmd = [hipcc, "-O1", "-std=c++17", "-I" + CSRC, "-Wall", "-Werror", "-x", "c++",
           os.path.join(ROOT, "tests", "surface_table_check.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True)
    assert b.returncode == 0, b.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout == ref.format_table()


def test_table_shape():
    t = ref.tet_table()
    assert t[:, 0, 0].max() == 0 and t[:, 15, 0].max() == 0
    assert np.all(t[:, 1:15, 0] >= 1)
    for k in range(6):
        for code in range(1, 15):
            # the complementary case is the same surface, wound the other way
            n = int(t[k, code, 0])
            mine = {tuple(t[k, code, 1 + 3 * j:4 + 3 * j]) for j in range(n)}
            other = {tuple(t[k, 15 - code, 1 + 3 * j:4 + 3 * j]) for j in range(n)}
            assert {frozenset(x) for x in mine} == {frozenset(x) for x in other}
            assert mine != other


def test_ply_round_trip(tmp_path):
    v, f = fx.reference_extract("s12")
    n = surface.vertex_normals(v, f)
    col = np.random.RandomState(0).randint(0, 256, (len(v), 3)).astype(np.uint8)
    p = str(tmp_path / "m.ply")
    surface.save_ply(p, v, f, normals=n, colors=col)
    m = surface.load_ply(p)
    assert np.array_equal(m["vertices"], v.astype(np.float32).astype(np.float64))
    assert np.array_equal(m["faces"], f) and m["faces"].dtype == np.int32
    assert np.array_equal(m["normals"], n.astype(np.float32).astype(np.float64))
    assert np.array_equal(m["colors"], col)
    head = open(p, "rb").read(400).split(b"end_header\n")[0].decode().split("\n")
    assert head[:6] == ["ply", "format binary_little_endian 1.0", f"element vertex {len(v)}",
                        "property float x", "property float y", "property float z"]
    assert f"element face {len(f)}" in head
    assert "property list uchar int vertex_indices" in head

    surface.save_ply(p, v, f)
    m = surface.load_ply(p)
    assert m["normals"] is None and m["colors"] is None
    assert np.array_equal(m["faces"], f)
    surface.save_ply(p, v, f, colors=np.full((len(v), 3), 0.5))
    assert np.all(surface.load_ply(p)["colors"] == 128)


def test_ply_zero_faces(tmp_path):
    v = np.array([[0.0, 1.0, 2.0], [3.0, 4.0, 5.0]])
    p = str(tmp_path / "cloud.ply")
    surface.save_ply(p, v)
    assert b"element face 0\n" in open(p, "rb").read()
    m = surface.load_ply(p)
    assert np.array_equal(m["vertices"], v)
    assert m["faces"].shape == (0, 3) and m["faces"].dtype == np.int32
    with pytest.raises(ValueError):
        surface.save_ply(p, v, [[0, 1, 2]])
    with pytest.raises(ValueError):
        surface.save_ply(p, v, normals=np.zeros((3, 3)))


def test_vertex_normals_tetrahedron():
    v = np.array([[0.0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]])
    f = np.array([[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]])      # outward
    n = surface.vertex_normals(v, f)
    assert np.allclose(np.linalg.norm(n, axis=1), 1.0)
    # vertex 0: three faces of area 1/2 with normals -z, -y, -x
    assert np.allclose(n[0], -np.ones(3) / np.sqrt(3.0))
    # vertex 1: -z and -y of area 1/2 and the slanted face (1, 1, 1) / sqrt 3 of area sqrt 3 / 2
    e = np.array([0.0, -0.5, -0.5]) + 0.5 * np.ones(3)
    assert np.allclose(n[1], e / np.linalg.norm(e))
    lone = surface.vertex_normals(np.vstack((v, [[9.0, 9, 9]])), f)
    assert np.array_equal(lone[4], np.zeros(3))


def test_bounds():
    rs = np.random.RandomState(3)
    pts = rs.uniform(-1, 2, (50, 3)) * (1.0, 2.0, 0.5)
    pts[7] = np.nan
    origin, dims = surface.bounds(pts, 0.1, margin=0.25)
    good = pts[np.isfinite(pts).all(axis=1)]
    hi = origin + 0.1 * (np.array(dims[::-1]) - 1)
    assert np.all(origin <= good.min(axis=0) - 0.25 + 1e-12)
    assert np.all(hi >= good.max(axis=0) + 0.25 - 1e-12)
    assert np.all(hi - 0.1 < good.max(axis=0) + 0.25)
    with pytest.raises(ValueError):
        surface.bounds(np.full((3, 3), np.nan), 0.1)
    with pytest.raises(ValueError):
        surface.bounds(pts, 0.0)


# ------------------------------------------------------------------------------------------
# every ValueError of integrate and extract, without a GPU
# ------------------------------------------------------------------------------------------
def _integrate_args():
    _, cams, depth = dense_fixture.scene("fronto")
    return dict(depth_maps=depth, cams=cams, K=dense_fixture.K, origin=fx.ORIGIN, voxel=fx.VOXEL,
                dims=fx.DIMS, trunc=fx.TRUNC)


BAD_CAMS = np.array(dense_fixture.cameras())
BAD_CAMS[1, 0, 0] = np.inf


@pytest.mark.parametrize("change", [
    dict(dims=(2049, 1, 1)), dict(dims=(1, 1, 0)), dict(dims=(512, 512, 513)), dict(dims=(4, 4)),
    dict(voxel=0.0), dict(voxel=-1.0), dict(voxel=np.nan), dict(voxel=np.inf),
    dict(origin=(0.0, np.nan, 0.0)), dict(origin=(0.0, 0.0)), dict(origin=(np.inf, 0.0, 0.0)),
    dict(trunc=0.0), dict(trunc=-0.1), dict(trunc=np.nan),
    dict(cams=BAD_CAMS), dict(cams=dense_fixture.cameras()[:2]),
    dict(depth_maps=np.zeros((3, 40))), dict(depth_maps=np.zeros((0, 4, 4)), cams=np.zeros((0, 3, 4))),
    dict(depth_maps=np.zeros((129, 2, 2)), cams=np.tile(dense_fixture.cameras()[:1], (129, 1, 1))),
    dict(weights=np.ones((3, 40, 56))), dict(weights=np.ones((3, 40, 55), np.float32)),
    dict(tsdf=np.zeros(fx.DIMS, np.float32)), dict(weight=np.zeros(fx.DIMS, np.float32)),
    dict(tsdf=np.zeros(fx.DIMS, np.float32), weight=np.zeros(fx.DIMS)),
    dict(tsdf=np.zeros(fx.DIMS), weight=np.zeros(fx.DIMS, np.float32)),
    dict(tsdf=np.zeros((26, 22, 31), np.float32), weight=np.zeros((26, 22, 31), np.float32)),
    dict(K=np.eye(3) * 2.0),
])
def test_integrate_value_errors(change):
    args = _integrate_args()
    args.update(change)
    with pytest.raises(ValueError):
        surface.integrate(**args)


def test_integrate_image_limits():
    cams = np.tile(dense_fixture.cameras()[:1], (2, 1, 1))
    for shape in ((2, 1, 16385), (2, 16385, 1)):
        depth = np.zeros(shape)
        with pytest.raises(ValueError):
            surface.integrate(depth, cams, dense_fixture.K, fx.ORIGIN, fx.VOXEL, (2, 2, 2), 0.1)


@pytest.mark.parametrize("change", [
    dict(tsdf=np.zeros((4, 4, 4))), dict(tsdf=np.zeros((4, 4), np.float32)),
    dict(weight=np.zeros((4, 4, 5), np.float32)), dict(weight=np.zeros((4, 4, 4))),
    dict(origin=(0.0, 0.0, np.nan)), dict(voxel=0.0), dict(voxel=np.inf),
    dict(min_weight=0.0), dict(min_weight=-1.0), dict(min_weight=np.nan),
    dict(tsdf=np.zeros((1, 1, 2049), np.float32), weight=np.zeros((1, 1, 2049), np.float32)),
])
def test_extract_value_errors(change):
    args = dict(tsdf=np.zeros((4, 4, 4), np.float32), weight=np.ones((4, 4, 4), np.float32),
                origin=np.zeros(3), voxel=1.0, min_weight=1.0)
    args.update(change)
    with pytest.raises(ValueError):
        surface.extract(**args)
