"""The device mesh index and the registration step on the GPU (eval.hip) against mesh_distance,
against the numpy restatement (tests/register_ref.py) on the cases of tests/register_fixture.py,
and evaluation.register / compare_meshes on top.

matched, kept, k, the bits of tau and the mask must be exact.  The bar on a moment is per slot,
relative to the sum of its terms' magnitudes: 4 x the worst figure the fp64 restatement shows
against its own longdouble run (tests/test_register_cpu.py: point 1.808e-16, plane 2.432e-16),
floored at 16 eps, so 3.6e-15 for both metrics.  The rms of a loop's step is the root of such a
moment over an exact count, so its relative bar is half of that; a step also inherits the
rounding of the steps before it through the transform, a few eps of the coordinates' magnitude
M = |box centre| + L / 2, so the rms bar is  bar / 2 x rms + 16 eps M.
The tests print whether the GPU's moments and rms were bit-equal to numpy's.
"""
import ctypes

import numpy as np
import pytest

import eval_fixture as ef
import eval_ref
import register_fixture as rf
import register_ref as ref
from tsbb15_amd import _ffi, evaluation as ev

pytestmark = pytest.mark.gpu


def _bits(*arrays):
    return b"".join(np.ascontiguousarray(a).tobytes() for a in arrays)


def _same(got, want):
    """The two mesh_distance tuples agree in every bit and every info entry."""
    assert _bits(got[0], got[1], got[2], got[3]["d2"]) == \
        _bits(want[0], want[1], want[2], want[3]["d2"])
    assert {k: v for k, v in got[3].items() if k != "d2"} == \
        {k: v for k, v in want[3].items() if k != "d2"}


@pytest.mark.parametrize("name", ef.CASE_NAMES)
def test_index_distance_is_mesh_distance(name, ctx):
    case = ef.cases()[name]
    lo, hi = ef.box_of(case.vertices, case.faces)
    width = float((hi - lo).max())
    cells = {"the case's": case.cell, "one cell": 4.0 * width, "box / 64": width / 64.0}
    indices = {what: ev.MeshIndex(case.vertices, case.faces, cell=cell, ctx=ctx)
               for what, cell in cells.items()}           # all alive at once
    try:
        first = None
        for what, cell in cells.items():
            want = ev.mesh_distance(case.queries, case.vertices, case.faces,
                                    max_dist=case.max_dist, cell=cell, ctx=ctx)
            index = indices[what]
            half = index.distance(case.queries[::2], max_dist=case.max_dist)
            assert _bits(half[1], half[3]["d2"]) == _bits(want[1][::2], want[3]["d2"][::2])
            _same(index.distance(case.queries, max_dist=case.max_dist), want)   # the second query
            first = first or want
            assert _bits(want[1], want[2], want[3]["d2"]) == _bits(first[1], first[2], first[3]["d2"])
        assert indices["one cell"].cells == (1, 1, 1)
    finally:
        for index in indices.values():
            index.close()
    with ev.MeshIndex(case.vertices, case.faces, ctx=ctx) as index:
        empty = index.distance(np.zeros((0, 3)))
        assert empty[0].shape == (0,) and empty[2].shape == (0, 3) and empty[3]["tests"] == 0


def _check_step(metric, got, arrays, want, what):
    d2, face, closest, mask = arrays
    assert (got["matched"], got["kept"], got["k"]) == (want["matched"], want["kept"], want["k"])
    if np.isnan(want["tau"]):
        assert np.isnan(got["tau"])
    else:
        assert _bits(np.float64(got["tau"])) == _bits(np.float64(want["tau"]))
    assert np.array_equal(mask, want["mask"])
    assert np.array_equal(face, want["face"])
    matched = face >= 0
    if got["matched"]:
        assert got["tau"] == np.sort(d2[matched])[got["k"] - 1]
        assert np.array_equal(mask, matched & (d2 <= got["tau"]))
    else:
        assert np.isnan(got["tau"]) and got["k"] == 0 and not mask.any()
    assert got["kept"] == int(mask.sum()) >= got["k"]
    dev = rf.deviation(got["moments"], want["moments"], want["scale"])
    equal = _bits(got["moments"]) == _bits(want["moments"].astype(np.float64))
    print(f"{what} {metric}: matched {got['matched']}, k {got['k']}, kept {got['kept']}, tau "
          f"{got['tau']!r}; moments deviate by {dev:.3e} (bar {rf.bar(metric):.3e}), bit-equal "
          f"{equal}; d2 bit-equal {_bits(d2) == _bits(want['d2'])}, closest bit-equal "
          f"{_bits(closest) == _bits(want['closest'])}")
    assert dev <= rf.bar(metric)
    assert (got["moments"][ref.NS[metric]:] == 0.0).all()


@pytest.fixture(scope="module")
def triangle_index(ctx):
    with ev.MeshIndex(rf.TRIANGLE, rf.TRI_FACES, ctx=ctx) as index:
        yield index


@pytest.fixture(scope="module")
def blob_index(ctx):
    with ev.MeshIndex(*rf.blob(), ctx=ctx) as index:
        yield index


@pytest.mark.parametrize("metric", rf.METRICS)
@pytest.mark.parametrize("name", rf.SMALL_NAMES)
def test_step_small(name, metric, triangle_index):
    case = rf.small_cases()[name]
    s, R, t = case["T"]
    triangle_index.set_points(case["points"])
    got = triangle_index.step(s, R, t, keep=case["keep"], max_dist=case["max_dist"],
                              metric=metric)
    _check_step(metric, got, triangle_index.read(), rf.small_step(name, metric), name)
    if name in rf.EXPECTED:
        assert (got["matched"], got["k"], got["kept"]) == rf.EXPECTED[name]
    if name == "none":
        assert (got["moments"] == 0.0).all()


@pytest.mark.parametrize("metric", rf.METRICS)
@pytest.mark.parametrize("name", rf.CLOUD_NAMES)
def test_step_blob(name, metric, blob_index):
    pts, keep = rf.clouds()[name]
    blob_index.set_points(pts)
    got = blob_index.step(keep=keep, metric=metric)
    _check_step(metric, got, blob_index.read(), rf.blob_step(name, metric), name)
    assert got["tests"] > 0


@pytest.mark.parametrize("metric", rf.METRICS)
def test_step_is_independent_of_the_cell(metric, ctx):
    v, f = rf.blob()
    pts, keep = rf.clouds()["outlier"]
    width = float((v.max(axis=0) - v.min(axis=0)).max())
    want, dims = None, set()
    for what, cell in (("default", None), ("one cell", 4.0 * width), ("box / 64", width / 64.0)):
        with ev.MeshIndex(v, f, cell=cell, ctx=ctx) as index:
            dims.add(index.cells)
            index.set_points(pts)
            for again in range(2):
                rec = index.step(*rf.MOVE, keep=keep, max_dist=3.0, metric=metric)
                bits = _bits(np.array([rec["matched"], rec["kept"], rec["k"]]),
                             np.float64(rec["tau"]), rec["moments"], *index.read())
                want = want or bits
                assert bits == want, (what, again)
    assert len(dims) == 3


@pytest.mark.parametrize("metric", rf.METRICS)
@pytest.mark.parametrize("name", rf.CLOUD_NAMES)
def test_register_against_the_restatement(name, metric, blob_index):
    v, f = rf.blob()
    pts, keep = rf.clouds()[name]
    iterations = rf.trace_iterations(name, metric)
    want = rf.blob_trace(name, metric)
    got = ev.register(pts, None, None, metric=metric, keep=keep, max_iter=iterations,
                      index=blob_index)
    assert got["iterations"] == want["iterations"] and got["converged"] == want["converged"]
    assert np.array_equal(got["kept"], want["kept"])
    assert np.array_equal(got["matched"], want["matched"])
    origin, L = ref.mesh_box(v, f)
    M = float(np.linalg.norm(origin)) + L / 2.0
    diff = np.abs(got["rms"] - want["rms"])
    allowed = 0.5 * rf.bar(metric) * want["rms"] + 16.0 * rf.EPS * M
    print(f"{name} {metric}: {got['iterations']} steps, rms {got['rms']}; largest |rms - rms_ref| "
          f"{diff.max():.3e} (allowed there {allowed[diff.argmax()]:.3e}), rms bit-equal "
          f"{_bits(got['rms']) == _bits(want['rms'])}, tau bit-equal "
          f"{_bits(got['tau']) == _bits(want['tau'])}, transform bit-equal "
          f"{_bits(got['R'], got['t']) == _bits(want['R'], want['t'])}")
    assert (diff <= allowed).all()
    assert np.array_equal(got["mask"], want["mask"])
    assert got["mask"].sum() == got["kept"][-1] and got["dist"].shape == (len(pts),)
    if (name, metric) == ("clean", "plane"):
        ts, tR, tt = rf.TRUTH
        rot = eval_ref.rotation_angle_deg(got["R"], tR)
        dt, ds = float(np.linalg.norm(got["t"] - tt)) / L, abs(got["s"] / ts - 1.0)
        print(f"rotation error {rot:.3e} deg, |t - t_true| / L {dt:.3e}, |s / s_true - 1| {ds:.3e}")
        assert rot <= 1e-8 and dt <= 1e-10 and ds <= 1e-10
        assert got["converged"]


def test_register_builds_its_own_index(ctx):
    v, f = rf.blob()
    pts, keep = rf.clouds()["outlier"]
    got = ev.register(pts, v, f, keep=keep, ctx=ctx)
    s, R, t = rf.TRUTH
    assert got["converged"] and got["iterations"] <= 8
    assert eval_ref.rotation_angle_deg(got["R"], R) <= 1e-8
    rigid = ev.register(ev.apply_similarity(pts, s, np.eye(3), np.zeros(3)), v, f, keep=keep,
                        with_scale=False, ctx=ctx)
    assert rigid["s"] == 1.0 and rigid["converged"]
    assert eval_ref.rotation_angle_deg(rigid["R"], R) <= 1e-8
    # from 20 degrees, the basin the loop is tested for
    far = ev.register(rf.clouds()["clean"][0], v, f, ctx=ctx,
                      init=(1.0, rf.rotation((1.0, 2.0, 3.0), -12.0), np.zeros(3)))
    assert far["converged"] and eval_ref.rotation_angle_deg(far["R"], R) <= 1e-8


def test_compare_meshes_registers_first(ctx):
    v, f = rf.blob()
    L = rf.blob_diagonal()
    moved = rf.back(v)
    plain = ev.compare_meshes(moved, f, v, f, ctx=ctx)
    assert plain["accuracy"] > 1e-3 * L and "registration" not in plain
    r = ev.compare_meshes(moved, f, v, f, ctx=ctx, register={})
    print(f"accuracy {plain['accuracy']:.4f} without, {r['accuracy']:.3e} with registration "
          f"({r['registration']['iterations']} steps)")
    assert r["accuracy"] < 1e-9 * L and r["completeness"] == 1.0
    assert eval_ref.rotation_angle_deg(r["R"], rf.TRUTH[1]) <= 1e-8
    assert abs(r["s"] / rf.TRUTH[0] - 1.0) <= 1e-10
    s = ev.compare_meshes(moved, f, v, f, ctx=ctx, samples=1500, register={"keep": 0.9})
    assert s["accuracy"] < 1e-9 * L


def test_timing(blob_index):
    blob_index.set_points(rf.clouds()["clean"][0])
    blob_index.timing(1)
    blob_index.step()
    ms = blob_index.timing(0)
    assert tuple(ms) == _ffi.EVAL_REG_STAGES and all(v >= 0.0 for v in ms.values())


def test_errors(ctx):
    v, f = rf.blob()
    pts = rf.clouds()["clean"][0]
    with pytest.raises(ValueError, match="matched no point"):
        ev.register(pts + 100.0, v, f, max_dist=1.0, ctx=ctx)
    for kw in ({"keep": 0.0}, {"keep": 1.0001}, {"metric": "line"}, {"max_dist": -1.0},
               {"init": (1.0, np.full((3, 3), np.nan), np.zeros(3))}):
        with pytest.raises(ValueError):
            ev.register(pts, v, f, ctx=ctx, **kw)
    bad = f.copy()
    bad[3, 2] = len(v)
    with pytest.raises(ValueError, match="out of range"):
        ev.MeshIndex(v, bad, ctx=ctx)
    with pytest.raises(ValueError, match="RS_EVAL_MAX_CELLS.*choose a larger cell"):
        ev.MeshIndex(v, f, cell=1e-6, ctx=ctx)
    for cell in (0.0, -1.0, np.inf, np.nan):
        with pytest.raises(ValueError):
            ev.MeshIndex(v, f, cell=cell, ctx=ctx)

    # the library's own checks, past the Python layer's
    lib, d, i32 = _ffi.lib(), _ffi.C.c_double, _ffi.C.c_int32
    h, info = ctypes.c_void_p(), _ffi.EvalInfo()
    for wrong in (bad, -1 - f):
        st = lib.rs_eval_index_create(ctx.handle, _ffi.ptr(v, d), len(v), _ffi.ptr(wrong, i32),
                                      len(f), 1.0, ctypes.byref(h), ctypes.byref(info))
        with pytest.raises(ValueError, match="out of range"):
            _ffi.check(st)
        assert not h.value
    index = ev.MeshIndex(v, f, ctx=ctx)
    T, o, rec = np.concatenate(([1.0], np.eye(3).ravel(), np.zeros(3))), np.zeros(3), _ffi.EvalStep()

    def step(T=T, o=o, keep=1.0, max_dist=np.inf, metric=1):
        return lib.rs_eval_index_step(index.handle, _ffi.ptr(T, d), _ffi.ptr(o, d), keep,
                                      max_dist, metric, ctypes.byref(rec))
    with pytest.raises(ValueError, match="no source cloud"):
        _ffi.check(step())
    with pytest.raises(ValueError, match="no step has run"):
        index.read()
    with pytest.raises(ValueError):
        index.set_points(np.zeros((0, 3)))
    index.set_points(pts)
    nanT = T.copy()
    nanT[4] = np.nan
    for kw in ({"keep": 0.0}, {"keep": 2.0}, {"keep": np.nan}, {"max_dist": 0.0}, {"metric": 2},
               {"metric": -1}, {"T": nanT}, {"o": np.array([0.0, np.inf, 0.0])}):
        with pytest.raises(ValueError):
            _ffi.check(step(**kw))
    with pytest.raises(ValueError, match="no step has run"):
        index.read()
    d2 = np.empty(4)
    st = lib.rs_eval_index_query(index.handle, _ffi.ptr(pts, d), 4, -1.0, _ffi.ptr(d2, d), None,
                                 None, ctypes.byref(info))
    with pytest.raises(ValueError, match="max_dist"):
        _ffi.check(st)
    # a step that matches nothing is no error of the ABI
    _ffi.check(step(max_dist=1e-9, T=np.concatenate(([1.0], np.eye(3).ravel(), [50.0, 0.0, 0.0]))))
    assert rec.matched == 0 and rec.kept == 0 and rec.k == 0 and np.isnan(rec.tau)
    assert not index.read()[3].any()
    # and the index still works
    _ffi.check(step())
    assert rec.matched == len(pts)
    index.close()
    index.close()
    for call in (lambda: index.distance(pts), lambda: index.set_points(pts), index.step,
                 index.read, lambda: ev.register(pts, None, None, index=index)):
        with pytest.raises(RuntimeError, match="closed"):
            call()
