"""The evaluation stage's mesh distance on the GPU (eval.hip) against the numpy restatement
(tests/eval_ref.py) on the cases of tests/eval_fixture.py, its independence of the grid, and
compare_meshes.

The bar on |d2_gpu - d2_ref| / L^2 (L the case's box diagonal) is 4 x the worst figure the fp64
restatement shows against its own longdouble run (tests/test_eval_cpu.py measures and asserts
it), floored at 16 eps:
    case            fp64 vs longdouble   bar
    one_triangle    0                    3.6e-15
    s12             4.485e-17            3.6e-15
    random          1.587e-17            3.6e-15
    big_and_small   4.485e-17            3.6e-15
    edges           1.312e-12            5.6e-12   (queries 100 box widths away, d2 = 1e4 L^2)
    half            1.304e-17            3.6e-15
    degenerate      4.9e-22              3.6e-15
Measured on an MI355X: the GPU's d2, face and closest are bit-equal to numpy's on every case (the
test prints the largest difference and the number of rows that differ).
"""
import numpy as np
import pytest

import eval_fixture as ef
import eval_ref
import surface_fixture
from tsbb15_amd import _ffi, evaluation as ev, surface

pytestmark = pytest.mark.gpu


def _bits(*arrays):
    return b"".join(np.ascontiguousarray(a).tobytes() for a in arrays)


def _run(case, ctx, **kw):
    kw.setdefault("cell", case.cell)
    kw.setdefault("max_dist", case.max_dist)
    return ev.mesh_distance(case.queries, case.vertices, case.faces, ctx=ctx, **kw)


def _check_parity(name, case, got, want):
    dist, face, closest, info = got
    d2 = info["d2"]
    rd2, rface, rclosest, pairs = want
    L2 = ef.diagonal(case) ** 2
    bar = ef.bar(name)
    assert np.array_equal(np.isnan(d2), np.isnan(rd2))
    assert np.array_equal(np.isinf(d2), np.isinf(rd2))
    assert np.array_equal(face == -1, rface == -1)
    assert np.array_equal(np.isnan(closest), np.isnan(rclosest))
    assert info["beyond"] == int(np.isinf(rd2).sum())
    ok = face >= 0
    rows = np.flatnonzero(ok)
    diff = np.abs(d2[ok] - rd2[ok])
    print(f"{name}: largest |d2_gpu - d2_ref| / L^2 = {float(diff.max() / L2) if len(rows) else 0:.3e}"
          f" (bar {bar:.3e}); rows that differ in d2 {int((diff != 0).sum())}, in face "
          f"{int((face != rface).sum())}, in closest "
          f"{int((closest[ok] != rclosest[ok]).any(axis=1).sum())} of {len(rows)}")
    assert (diff <= bar * L2).all()
    assert (pairs[rows, face[rows]] - rd2[rows] <= bar * L2).all()
    tri = case.vertices[case.faces[face[ok]]]
    bary = eval_ref.barycentric(closest[ok], tri[:, 0], tri[:, 1], tri[:, 2])
    assert bary.min() >= -1e-12 and bary.max() <= 1.0 + 1e-12
    e = case.queries[ok] - closest[ok]
    again = e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1] + e[:, 2] * e[:, 2]
    assert (np.abs(again - d2[ok]) <= 4.0 * ef.EPS * d2[ok]).all()
    assert np.array_equal(dist[ok], np.sqrt(d2[ok]))


@pytest.mark.parametrize("name", ef.CASE_NAMES)
def test_parity(name, ctx):
    case = ef.cases()[name]
    _check_parity(name, case, _run(case, ctx), ef.reference(name))


def test_hand_written_answers(ctx):
    case = ef.cases()["one_triangle"]
    dist, face, closest, info = _run(case, ctx)
    assert np.array_equal(info["d2"], [h[2] for h in ef.HAND])
    assert np.array_equal(closest, [h[1] for h in ef.HAND])
    assert (face == 0).all() and info["faces_skipped"] == 0 and info["beyond"] == 0


@pytest.mark.parametrize("count", ef.QUERY_COUNTS)
def test_query_counts(count, ctx):
    case = ef.cases()["s12"]
    d2, face, closest, _ = ef.reference("s12")
    got = ev.mesh_distance(case.queries[:count], case.vertices, case.faces, ctx=ctx)
    sub = ef.Case(case.vertices, case.faces, case.queries[:count], None, np.inf)
    _check_parity("s12", sub, got, (d2[:count], face[:count], closest[:count],
                                    ef.reference("s12")[3][:count]))


def _cells(case):
    lo, hi = ef.box_of(case.vertices, case.faces)
    width = float((hi - lo).max())
    return {"default": None, "one cell": 4.0 * width, "box / 64": width / 64.0,
            "boundaries": ef.EDGE_CELL, "the case's": case.cell}


@pytest.mark.parametrize("name", ("s12", "random", "big_and_small", "edges", "half", "degenerate"))
def test_independent_of_the_grid(name, ctx):
    case = ef.cases()[name]
    want, dims = None, set()
    for what, cell in _cells(case).items():
        dist, face, closest, info = _run(case, ctx, cell=cell)
        dims.add(info["cells"])
        bits = _bits(info["d2"], face, closest)
        want = want or bits
        assert bits == want, what
        if what == "one cell":
            assert info["cells"] == (1, 1, 1)
            nvalid = int(eval_ref.face_valid(case.vertices, case.faces).sum())
            nfinite = int(np.isfinite(case.queries).all(axis=1).sum())
            if case.max_dist == np.inf:
                assert info["tests"] == nfinite * nvalid
    assert len(dims) >= 3
    dist, face, closest, info = _run(case, ctx, cell=None)
    assert _bits(info["d2"], face, closest) == want, "a second identical call"


@pytest.mark.parametrize("name", ("s12", "random", "degenerate"))
def test_independent_of_the_face_order(name, ctx):
    case = ef.cases()[name]
    perm = np.random.RandomState(17).permutation(len(case.faces))
    _, face, closest, info = _run(case, ctx)
    _, pface, pclosest, pinfo = _run(ef.Case(case.vertices, case.faces[perm], case.queries,
                                             case.cell, case.max_dist), ctx)
    assert _bits(info["d2"]) == _bits(pinfo["d2"])
    rd2, _, _, pairs = ef.reference(name)
    tied = pairs == rd2[:, None]
    unique = (face >= 0) & (tied.sum(axis=1) == 1)
    assert unique.any()
    assert np.array_equal(perm[pface[unique]], face[unique])
    assert _bits(closest[unique]) == _bits(pclosest[unique])
    assert np.array_equal(pface == -1, face == -1)
    # among tied faces the lowest index of the permuted mesh wins
    where = np.empty(len(perm), dtype=np.int64)
    where[perm] = np.arange(len(perm))
    for i in np.flatnonzero((face >= 0) & ~unique):
        assert pface[i] == where[np.flatnonzero(tied[i])].min()


def test_info(ctx):
    cs = ef.cases()
    case = cs["s12"]
    _, _, _, info = _run(case, ctx)
    n, nf = len(case.queries), len(case.faces)
    print(f"s12: {info['tests'] / n:.1f} tests per query of {nf} faces, cells {info['cells']}, "
          f"{info['entries'] / nf:.2f} entries per face, largest cell {info['largest_cell']}")
    assert 0 < info["tests"] < n * nf / 4
    for name in ("s12", "random", "big_and_small", "degenerate"):
        c = cs[name]
        _, _, _, info = _run(c, ctx)
        dims, entries, largest = eval_ref.grid_entries(c.vertices, c.faces, info["cell"])
        assert info["cells"] == dims and info["entries"] == entries
        assert info["largest_cell"] == largest
        assert info["faces_skipped"] == int((~eval_ref.face_valid(c.vertices, c.faces)).sum())
    assert np.prod(_run(cs["random"], ctx)[3]["cells"]) > ef.SCAN_CHUNK
    assert _run(cs["degenerate"], ctx)[3]["faces_skipped"] == ef.DEGENERATE_SKIPPED


def test_empty_inputs(ctx):
    case = ef.cases()["s12"]
    dist, face, closest, info = ev.mesh_distance(np.zeros((0, 3)), case.vertices, case.faces,
                                                 ctx=ctx)
    assert dist.shape == (0,) and face.shape == (0,) and closest.shape == (0, 3)
    assert info["tests"] == 0 and info["entries"] == 0
    q = ef.cases()["degenerate"].queries
    dist, face, closest, info = ev.mesh_distance(q, case.vertices, np.zeros((0, 3), np.int32),
                                                 ctx=ctx)
    finite = np.isfinite(q).all(axis=1)
    assert np.isinf(dist[finite]).all() and np.isnan(dist[~finite]).all()
    assert (face == -1).all() and np.isnan(closest).all()
    assert info["beyond"] == finite.sum() and info["tests"] == 0 and info["cells"] == (1, 1, 1)
    # every face invalid
    dist, face, _, info = ev.mesh_distance(q, case.vertices, np.array([[0, 0, 1], [2, 2, 2]]),
                                           ctx=ctx)
    assert np.isinf(dist[finite]).all() and (face == -1).all() and info["faces_skipped"] == 2


def test_timing(ctx):
    case = ef.cases()["s12"]
    ev.timing(1, ctx=ctx)
    _run(case, ctx)
    ms = ev.timing(0, ctx=ctx)
    assert tuple(ms) == _ffi.EVAL_STAGES and all(v >= 0.0 for v in ms.values())


def test_compare_meshes(ctx):
    v, f = surface_fixture.reference_extract("s12")
    same = ev.compare_meshes(v, f, v, f, ctx=ctx)
    assert same["accuracy"] == 0.0 and same["completeness"] == 1.0
    assert (same["dist_rec"] == 0.0).all() and (same["dist_gt"] == 0.0).all()
    delta = 0.5                                    # half a voxel
    # a shade shorter than delta, so that the rounding of v + shift cannot pass it
    shift = (1.0 - 1e-9) * delta * np.array([2.0, -1.0, 2.0]) / 3.0
    for samples in (None, 3000):
        r = ev.compare_meshes(v + shift, f, v, f, threshold=delta, samples=samples, ctx=ctx)
        assert r["dist_rec"].max() <= delta and r["dist_gt"].max() <= delta
        assert 0.0 < r["accuracy"] <= delta and r["completeness"] == 1.0
        assert r["accuracy"] == eval_ref.kth_smallest(r["dist_rec"], 0.9)
        tight = ev.compare_meshes(v + shift, f, v, f, threshold=r["accuracy"] / 2,
                                  samples=samples, ctx=ctx)
        assert 0.0 < tight["completeness"] < 1.0
    again = ev.compare_meshes(v + shift, f, v, f, threshold=delta, samples=3000, ctx=ctx)
    assert _bits(again["dist_rec"], again["dist_gt"]) == _bits(r["dist_rec"], r["dist_gt"])


def test_sphere_points_against_the_gpu_mesh(ctx):
    tsdf, weight, origin, voxel, mw = surface_fixture.extract_cases()["s16"]
    v, f = surface.extract(tsdf, weight, origin, voxel, mw, ctx=ctx)
    _, centre, r = surface_fixture.SPHERES["s16"]
    d = np.random.RandomState(6).standard_normal((2000, 3))
    pts = np.asarray(centre) + r * d / np.linalg.norm(d, axis=1, keepdims=True)
    dist, face, _, _ = ev.mesh_distance(pts, v, f, ctx=ctx)
    radial = surface_fixture.sphere_radial_error(v, "s16").max()
    tri = v[f]
    edge = max(np.linalg.norm(tri[:, i] - tri[:, (i + 1) % 3], axis=1).max() for i in range(3))
    sag = r - np.sqrt(r * r - edge * edge / 4.0)
    print(f"s16: largest distance {dist.max():.4f}, radial error {radial:.4f} + sag {sag:.4f} "
          f"(longest edge {edge:.4f})")
    assert (face >= 0).all()
    assert dist.max() < radial + sag


def test_argument_errors(ctx):
    case = ef.cases()["s12"]
    q, v, f = case.queries[:10], case.vertices, case.faces
    bad = f.copy()
    bad[7, 1] = len(v)
    with pytest.raises(ValueError, match="out of range"):
        ev.mesh_distance(q, v, bad, ctx=ctx)
    # the library's own check, past the Python layer's
    d2, face, closest = np.empty(10), np.empty(10, np.int32), np.empty((10, 3))
    info = _ffi.EvalInfo()
    d, i32 = _ffi.C.c_double, _ffi.C.c_int32
    for wrong in (bad, -1 - f):
        st = _ffi.lib().rs_eval_mesh_distance(
            ctx.handle, _ffi.ptr(q, d), 10, _ffi.ptr(v, d), len(v), _ffi.ptr(wrong, i32), len(f),
            np.inf, 1.0, _ffi.ptr(d2, d), _ffi.ptr(face, i32), _ffi.ptr(closest, d),
            _ffi.C.byref(info))
        with pytest.raises(ValueError, match="out of range"):
            _ffi.check(st)
    with pytest.raises(ValueError, match="RS_EVAL_MAX_CELLS.*choose a larger cell"):
        ev.mesh_distance(q, v, f, cell=1e-6, ctx=ctx)
    with pytest.raises(ValueError, match="choose a larger cell"):
        ev.mesh_distance(q, v, f, cell=1e-300, ctx=ctx)
    # nine faces across the whole box at 250^3 cells: the cells fit, the registrations do not
    lo, hi = ef.box_of(v, f)
    big = np.array([lo, [hi[0], hi[1], lo[2]], [lo[0], hi[1], hi[2]]])
    with pytest.raises(ValueError, match="RS_EVAL_MAX_ENTRIES.*choose a larger cell"):
        ev.mesh_distance(q, big, np.tile([[0, 1, 2]], (9, 1)),
                         cell=float((hi - lo).max()) / 249.5, ctx=ctx)
    for kw in ({"max_dist": 0.0}, {"max_dist": -1.0}, {"max_dist": np.nan}, {"cell": 0.0},
               {"cell": -2.0}, {"cell": np.inf}, {"cell": np.nan}):
        with pytest.raises(ValueError):
            ev.mesh_distance(q, v, f, ctx=ctx, **kw)
    for wrong in (q[:, :2], q.reshape(-1)):
        with pytest.raises(ValueError):
            ev.mesh_distance(wrong, v, f, ctx=ctx)
    with pytest.raises(ValueError):
        ev.mesh_distance(q, v, f.astype(np.float64), ctx=ctx)
    # and the context still works
    assert np.isfinite(ev.mesh_distance(q, v, f, ctx=ctx)[0]).all()
