"""Global registration on the GPU (csrc/global_reg.hip; tsbb15_amd.cloud.fpfh, match_features,
evaluation.ransac_similarity, global_register) against the numpy restatement tests/global_ref.py
on the cases of tests/global_fixture.py.

Bars.  Descriptors, matches, candidates, counts, models and gate statistics: equal in every bit.
Every device expression is fp64 without contraction in the header's order, and sqrt and division
round correctly on both sides.  The end-to-end runs must list the restatement's candidates and,
after the refinement, meet what tests/test_gpu_register.py asks of ``register`` on the
corresponding cloud of its blob: 1e-8 degrees, 1e-10 of the diagonal and 1e-10 of the scale on the
clean cloud; convergence within 8 steps and 1e-8 degrees with the outliers.  For the noisy cloud
that file has no bar against the truth; the one here is five standard errors of the trimmed
point-to-plane fit under the fixture's noise, from the fit's own covariance
(global_fixture.noisy_bars, where the derivation stands): 0.476 degrees, 1.15e-3 of the scale,
3.15e-3 of the diagonal.  Measured on the MI355X: 0.138 to 0.140 degrees, 2.1e-4 to 2.3e-4,
8.3e-4 to 8.4e-4 (1.5, 0.9 and 1.3 standard errors).
Rotation errors are measured by global_fixture.rotation_angle_deg: the arc cosine of the trace
cannot resolve an angle below 1.2e-6 degrees.
"""
import numpy as np
import pytest

import global_fixture as gf
import global_ref as ref
from tsbb15_amd import _ffi, cloud, evaluation as ev

pytestmark = pytest.mark.gpu


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64) if a.dtype == np.float64 else a


def _same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(_bits(a), _bits(b))


# ---- descriptors ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", gf.FPFH_NAMES)
def test_fpfh_equals_the_restatement(name, ctx):
    p, nr, k = gf.fpfh_cases()[name]
    want, wc = gf.fpfh_want(name)
    got, count, info = cloud.fpfh(p, nr, k=k, ctx=ctx)
    assert got.shape == (len(p), 33) and count.dtype == np.int32
    assert np.array_equal(count, wc)
    assert _same_bits(got, want), np.argwhere(_bits(got) != _bits(want))[:5]
    assert np.array_equal(np.isnan(got).all(axis=1), np.isnan(got).any(axis=1))
    full = ~np.isnan(got[:, 0])
    # three histograms of weight 1 each, twice: the point's own and its neighbours' mean
    assert np.allclose(got[full].sum(axis=1), 6.0, rtol=0.0, atol=1e-12)


def test_fpfh_does_not_depend_on_the_cell(ctx):
    p, nr, k = gf.fpfh_cases()["random_300_k16"]
    a = cloud.fpfh(p, nr, k=k, cell=0.3, ctx=ctx)
    b = cloud.fpfh(p, nr, k=k, cell=50.0, ctx=ctx)
    assert _same_bits(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert a[2]["cells"] != b[2]["cells"] and b[2]["cells"] == 1
    assert _same_bits(a[0], gf.fpfh_want("random_300_k16")[0])


def test_fpfh_is_invariant_under_an_exact_similarity(ctx):
    p, nr, q, mr, k = gf.dyadic_cloud()
    a = cloud.fpfh(p, nr, k=k, ctx=ctx)
    b = cloud.fpfh(q, mr, k=k, ctx=ctx)
    assert np.array_equal(a[1], b[1]) and a[1].min() > 0
    assert _same_bits(a[0], b[0])
    assert _same_bits(a[0], ref.fpfh(p, nr, k)[0])


def test_fpfh_arguments(ctx):
    p, nr, _ = gf.fpfh_cases()["random_65_k8"]
    for bad in (0, 64, 2.0):
        with pytest.raises(ValueError):
            cloud.fpfh(p, nr, k=bad, ctx=ctx)
    with pytest.raises(ValueError):
        cloud.fpfh(p, nr[:-1], k=4, ctx=ctx)
    with pytest.raises(ValueError):
        cloud.fpfh(p, nr, k=4, cell=-1.0, ctx=ctx)
    out, count, _ = cloud.fpfh(np.zeros((0, 3)), np.zeros((0, 3)), k=4, ctx=ctx)
    assert out.shape == (0, 33) and count.shape == (0,)


# ---- matching ---------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ("random", "ties", "nan"))
@pytest.mark.parametrize("D", gf.MATCH_DIMS)
def test_match_equals_the_restatement(D, kind, ctx):
    for n, m in gf.MATCH_SIZES:
        fa, fb = gf.match_case(n, m, D, kind)
        want = ref.match(fa, fb)
        got = cloud.match_features(fa, fb, ctx=ctx)
        assert got[0].dtype == np.int32
        assert np.array_equal(got[0], want[0]), (n, m, D, kind)
        assert _same_bits(got[1], want[1]), (n, m, D, kind)
        if kind == "ties" and m > 1:
            assert (got[0] < (m + 1) // 2).all()        # the first of two equal rows
        if kind == "nan":
            assert (got[0][::7] == -1).all() and np.isinf(got[1][::7]).all()
            assert not np.isin(got[0], np.arange(0, m, 5)).any()


def test_match_without_candidates(ctx):
    fa, fb = gf.match_case(65, 63, 33)
    idx, d2 = cloud.match_features(fa, np.zeros((0, 33)), ctx=ctx)
    assert (idx == -1).all() and np.isinf(d2).all() and len(idx) == 65
    idx, d2 = cloud.match_features(fa, np.full((70, 33), np.nan), ctx=ctx)
    assert (idx == -1).all() and np.isinf(d2).all()
    idx, d2 = cloud.match_features(np.zeros((0, 33)), fb, ctx=ctx)
    assert idx.shape == (0,) and d2.shape == (0,)
    with pytest.raises(ValueError):
        cloud.match_features(np.zeros((3, 65)), np.zeros((3, 65)), ctx=ctx)
    with pytest.raises(ValueError):
        cloud.match_features(fa, fb[:, :5], ctx=ctx)


def test_match_mutual(ctx):
    fa, fb = gf.match_case(300, 2 * ref.TILE + 5, 33)
    want = ref.match_mutual(fa, fb)
    got = cloud.match_features(fa, fb, mutual=True, ctx=ctx)
    assert np.array_equal(got[0], want[0]) and _same_bits(got[1], want[1])
    assert 0 < (got[0] >= 0).sum() < 300


# ---- RANSAC -----------------------------------------------------------------------------------
def _check_ransac(got, want, what):
    assert got["info"]["hypotheses"] == want["info"]["hypotheses"], what
    assert np.array_equal(got["info"]["passed"], want["info"]["passed"]), what
    assert got["info"]["tests"] == want["info"]["tests"], what
    assert got["info"]["found"] == want["info"]["found"] == len(got["h"]), what
    assert np.array_equal(got["h"], want["h"]), what
    assert np.array_equal(got["count"], want["count"]), what
    for key in ("s", "R", "t"):
        assert _same_bits(got[key], want[key]), (what, key)
    order = np.lexsort((got["h"], -got["count"]))
    assert np.array_equal(order, np.arange(len(order))), what


@pytest.mark.parametrize("name", gf.RANSAC_NAMES)
def test_ransac_equals_the_restatement(name, ctx):
    args, kw = gf.ransac_args(name)
    want = gf.ransac_want(name)
    got = ev.ransac_similarity(*args, ctx=ctx, **kw)
    _check_ransac(got, want, name)
    if name in ("all_gated_out", "scale_gate_empty", "collinear"):
        assert len(got["h"]) == 0 and got["R"].shape == (0, 3, 3)
    if name == "planted":
        # the winner is the first all-inlier triple; its model is the closed form of that triple
        src, dst = args[0], args[1]
        assert got["count"][0] == 20
        tup = ref.philox_ref.floyd_tuples(kw["seed"], int(got["h"][0]), 1, len(src), 3)
        model = ref.triple_model(src[tup], dst[tup])[0][0]
        assert _same_bits(np.concatenate(([got["s"][0]], got["R"][0].ravel(), got["t"][0])), model)
        assert abs(got["s"][0] - 1.3) < 1e-9
    if name == "repeated_dst":
        assert got["info"]["passed"][0] < got["info"]["hypotheses"]
    if name == "rigid":
        assert (got["s"] == 1.0).all() and got["count"][0] == 60


def test_ransac_counts_a_point_at_the_distance(ctx):
    at = ev.ransac_similarity(*gf.ransac_args("at_the_distance")[0], ctx=ctx, candidates=64,
                              **gf.ransac_args("at_the_distance")[1])
    below = ev.ransac_similarity(*gf.ransac_args("below_the_distance")[0], ctx=ctx, candidates=64,
                                 **gf.ransac_args("below_the_distance")[1])
    tup = ref.philox_ref.floyd_tuples(0, 0, 64, 4, 3)
    # the triples of the exact frame that start at the right angle: e1 and e2 lie along axes
    first = np.flatnonzero((tup != 3).all(axis=1) & (tup[:, 0] == 0))
    assert len(first) > 0
    for h in first:
        i, j = int(np.flatnonzero(at["h"] == h)[0]), int(np.flatnonzero(below["h"] == h)[0])
        assert at["count"][i] == 4 and below["count"][j] == 3
        assert at["s"][i] == 1.0 and np.array_equal(at["R"][i], np.eye(3))
        assert np.array_equal(at["t"][i], np.zeros(3))


def test_ransac_candidates_and_arguments(ctx):
    args, kw = gf.ransac_args("planted")
    want = gf.ransac_want("planted")
    hs, count, _ = want["survivors"]
    order = np.lexsort((hs, -count))
    one = ev.ransac_similarity(*args, ctx=ctx, candidates=1, **kw)
    assert one["h"][0] == hs[order[0]] and len(one["h"]) == 1
    many = ev.ransac_similarity(*args, ctx=ctx, candidates=1024, **kw)
    assert np.array_equal(many["h"], hs[order][:1024])
    assert np.array_equal(many["count"], count[order][:1024])
    src, dst, H, dist = args
    for bad in (dict(H=0), dict(candidates=0), dict(candidates=1025), dict(inlier_dist=-1.0),
                dict(edge_tol=np.nan), dict(min_edge=-1.0), dict(scale=(np.nan, 1.0))):
        call = dict(H=H, inlier_dist=dist)
        call.update(bad)
        with pytest.raises(ValueError):
            ev.ransac_similarity(src, dst, ctx=ctx, **call)
    with pytest.raises(ValueError):
        ev.ransac_similarity(src[:2], dst[:2], 10, 0.1, ctx=ctx)
    with pytest.raises(ValueError):
        ev.ransac_similarity(src, dst[:-1], 10, 0.1, ctx=ctx)


def test_timing(ctx):
    p, nr, k = gf.fpfh_cases()["random_300_k16"]
    cloud.global_timing(1, ctx=ctx)
    try:
        f, _, _ = cloud.fpfh(p, nr, k=k, ctx=ctx)
        cloud.match_features(f, f, ctx=ctx)
        args, kw = gf.ransac_args("planted")
        ev.ransac_similarity(*args, ctx=ctx, **kw)
        ms = cloud.global_timing(0, ctx=ctx)
    finally:
        cloud.global_timing(0, ctx=ctx)
    assert tuple(ms) == _ffi.GLOBAL_STAGES and all(v > 0.0 for v in ms.values()), ms


# ---- end to end -------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def egg_index(ctx):
    with ev.MeshIndex(*gf.egg(), ctx=ctx) as index:
        yield index


def test_the_mesh_descriptors_equal_the_restatement(ctx):
    v, f = gf.egg()
    for n in (gf.SAMPLES, gf.SAMPLES + gf.OUTLIERS):
        pts, face = ev.sample_surface(v, f, n, 0)
        got = cloud.fpfh(pts, ev.face_normals(v, f)[face], k=gf.K, ctx=ctx)[0]
        assert _same_bits(got, gf.target_of(n)[1])


@pytest.mark.parametrize("pose", range(len(gf.POSES)))
@pytest.mark.parametrize("name", gf.CLOUD_NAMES)
def test_global_register(name, pose, egg_index, ctx):
    v, f = gf.egg()
    pts, nrm = gf.cloud(name, pose)
    want = gf.coarse(name, pose, verify=False)
    got = ev.global_register(pts, nrm, v, f, k=gf.K, H=gf.H, candidates=gf.CANDIDATES,
                             keep=gf.KEEP[name], index=egg_index, ctx=ctx)
    assert got["correspondences"] == len(want["src"])
    assert got["scale"] == want["scale"] and got["inlier_dist"] == want["inlier_dist"]
    _check_ransac(got["candidates"], want["candidates"], (name, pose))
    rot, ds, dt = gf.pose_errors(*got["coarse"], pose)
    reg = got["registration"]
    print(f"{name} pose {pose}: chosen {got['chosen']} of {len(got['coarse_rms'])}, coarse "
          f"{rot:.2f} deg, scale {ds:.2e}, translation {dt:.2e} of the diagonal, trimmed rms "
          f"{got['coarse_rms'][got['chosen']]:.4f}; refined in {reg['iterations']} steps to "
          f"{gf.pose_errors(got['s'], got['R'], got['t'], pose)}")
    assert rot <= gf.BASIN_DEG
    rot, ds, dt = gf.pose_errors(got["s"], got["R"], got["t"], pose)
    if name == "clean":
        assert reg["converged"] and rot <= 1e-8 and dt <= 1e-10 and ds <= 1e-10
    elif name == "outlier":
        assert reg["converged"] and reg["iterations"] <= 8 and rot <= 1e-8
    else:
        bar = gf.noisy_bars(pose)
        assert reg["converged"] and rot <= bar[0] and ds <= bar[1] and dt <= bar[2], bar


def test_global_register_picks_by_the_mesh_and_not_by_the_count(egg_index, ctx):
    want = gf.coarse("outlier", 4, verify=True)
    v, f = gf.egg()
    pts, nrm = gf.cloud("outlier", 4)
    got = ev.global_register(pts, nrm, v, f, k=gf.K, H=gf.H, candidates=gf.CANDIDATES,
                             keep=gf.KEEP["outlier"], refine=False, index=egg_index, ctx=ctx)
    assert got["chosen"] == want["chosen"] and got["registration"] is None
    assert np.allclose(got["coarse_rms"], want["rms"], rtol=1e-12, atol=0.0)
    assert _same_bits(got["R"], want["coarse"][1]) and got["s"] == want["coarse"][0]


def test_compare_meshes_global(ctx):
    v, f = gf.egg()
    moved = gf.back(v, 3)
    L = ref.register_ref.mesh_box(v, f)[1]
    plain = ev.compare_meshes(moved, f, v, f, ctx=ctx)
    r = ev.compare_meshes(moved, f, v, f, ctx=ctx, register="global")
    print(f"accuracy {plain['accuracy']:.4f} without, {r['accuracy']:.3e} with the global "
          f"registration")
    assert plain["accuracy"] > 1e-2 * L
    assert r["accuracy"] < 1e-9 * L and r["completeness"] == 1.0
    assert gf.pose_errors(r["s"], r["R"], r["t"], 3)[0] <= 1e-8
    assert r["registration"]["registration"]["converged"]
    with pytest.raises(ValueError):
        ev.compare_meshes(moved, f, v, f, ctx=ctx, register="local")
