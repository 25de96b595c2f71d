"""The numpy restatement of the global registration (tests/global_ref.py) against independent
formulations, and the end-to-end proof on the CPU that the verified coarse pose lands inside the
20 degree basin DESIGN.md section 17.1 pins for ``register``, for every pose and cloud of
tests/global_fixture.py.  No GPU.
"""
import numpy as np
import pytest
from scipy.spatial import cKDTree

import eval_ref
import global_fixture as gf
import global_ref as ref
import register_ref
from tsbb15_amd import _ffi, cloud, evaluation as ev


def test_pseudo_angle_orders_directions_as_atan2_does():
    rs = np.random.RandomState(3)
    xy = rs.standard_normal((2000, 2))
    a = ref.pseudo_angle(xy[:, 0], xy[:, 1])
    # measured from the negative y axis, counter-clockwise, as a runs from 0 to 4
    phi = np.mod(np.arctan2(xy[:, 1], xy[:, 0]) + 0.5 * np.pi, 2.0 * np.pi)
    assert np.array_equal(np.argsort(a), np.argsort(phi))
    assert (a >= 0.0).all() and (a <= 4.0).all()
    got = ref.pseudo_angle(*np.array([(0.0, -1.0), (1.0, 0.0), (0.0, 1.0), (-1.0, 0.0),
                                      (0.0, 0.0), (-0.0, -1.0), (-1.0, -0.0), (1.0, 1.0),
                                      (-1.0, 1.0), (-1.0, -1.0), (1.0, -1.0)]).T)
    assert got.tolist() == [0.0, 1.0, 2.0, 3.0, 0.0, 0.0, 3.0, 1.5, 2.5, 3.5, 0.5]
    assert ref.bin11(np.array([-0.5, 0.0, 0.99, 10.0, 10.99, 11.0, 12.0, np.nan])).tolist() == \
        [0, 0, 0, 10, 10, 10, 10, 0]


def test_descriptor_by_a_plain_loop():
    """The vectorised restatement against a loop written from the header, with math.atan-free
    scalar arithmetic, on a cloud with duplicates and a NaN normal."""
    p, nr, k = gf.fpfh_cases()["nan_normals"]
    idx, d2, use = ref.neighbour_lists(p, k)
    hist = np.zeros((len(p), 33), dtype=np.int64)
    for i in range(len(p)):
        for e in range(k + 1):
            if not use[i, e] or not d2[i, e] > 0.0:
                continue
            j = idx[i, e]
            u, nj, d = nr[i], nr[j], p[j] - p[i]
            if not (np.isfinite(u).all() and np.isfinite(nj).all()):
                continue
            c = np.array([d[1] * u[2] - d[2] * u[1], d[2] * u[0] - d[0] * u[2],
                          d[0] * u[1] - d[1] * u[0]])
            cc = (c[0] * c[0] + c[1] * c[1]) + c[2] * c[2]
            if not cc > 0.0:
                continue
            v = c / np.sqrt(cc)
            w = np.array([u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2],
                          u[0] * v[1] - u[1] * v[0]])
            dot = lambda a, b: (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]      # noqa: E731
            f = (dot(v, nj), dot(u, d) / np.sqrt(d2[i, e]),
                 float(ref.pseudo_angle(dot(u, nj), dot(w, nj))))
            for g, q in enumerate(((f[0] + 1.0) * 5.5, (f[1] + 1.0) * 5.5, f[2] * 2.75)):
                hist[i, 11 * g + int(ref.bin11(np.float64(q)))] += 1
    got, c, _ = ref.spfh(p, nr, k)
    assert np.array_equal(got, hist) and np.array_equal(c, hist[:, :11].sum(axis=1))
    out, c2 = ref.fpfh(p, nr, k)
    assert np.array_equal(c, c2) and np.isnan(out[4]).all() and c[4] == 0
    full = ~np.isnan(out[:, 0])
    assert np.allclose(out[full].sum(axis=1), 6.0, rtol=0.0, atol=1e-12)


def test_every_bin_edge_and_branch_is_met():
    """The hand-placed pairs put f1 and f2 on -1, 0, 1 and on every k / 5.5 - 1, and the
    pseudo-angle on every branch and joint."""
    p, nr, k = gf.fpfh_cases()["bin_edges"]
    idx, d2, use = ref.neighbour_lists(p, k)
    counted, f1, f2, _ = ref.pair_features(p, nr, idx, d2, use)
    first = np.arange(0, len(p), 2)             # the pair seen from its first point
    e = use[first].argmax(axis=1)
    assert counted[first, e].all()
    v1, v2 = f1[first, e], f2[first, e]
    for f in (-1.0, 0.0, 1.0) + gf.EDGES:
        assert (v1 == f).any() and (v2 == f).any(), f
    p, nr, k = gf.fpfh_cases()["angles"]
    idx, d2, use = ref.neighbour_lists(p, k)
    counted, _, _, a = ref.pair_features(p, nr, idx, d2, use)
    e = use[first[:len(p) // 2]].argmax(axis=1)
    a = a[np.arange(0, len(p), 2), e]
    want = ref.pseudo_angle(*np.array(gf.ANGLES).T)
    assert np.array_equal(a, want)
    assert {0.0, 1.0, 2.0, 3.0, 1.5, 2.5, 3.5, 0.5, 4.0} <= set(a.tolist())
    assert set(ref.bin11(a * 2.75).tolist()) >= {0, 1, 2, 4, 5, 6, 8, 9, 10}


def test_a_similarity_changes_no_count():
    p, nr, q, mr, k = gf.dyadic_cloud()
    a, b = ref.spfh(p, nr, k), ref.spfh(q, mr, k)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[1].min() > 0
    assert np.array_equal(ref.fpfh(p, nr, k)[0], ref.fpfh(q, mr, k)[0])


def test_match_against_a_kd_tree():
    fa, fb = gf.match_case(300, 2 * ref.TILE + 5, 33)
    idx, d2 = ref.match(fa, fb)
    dist, near = cKDTree(fb).query(fa)
    assert np.array_equal(idx, near) and np.allclose(d2, dist * dist, rtol=1e-12)
    fa, fb = gf.match_case(65, 63, 16, "ties")
    idx, d2 = ref.match(fa, fb)
    full = ((fa[:, None, :] - fb[None, :, :]) ** 2).sum(axis=2)
    assert np.array_equal(d2, full.min(axis=1))            # small integers: exact
    assert np.array_equal(idx, (full == full.min(axis=1)[:, None]).argmax(axis=1))
    fa, fb = gf.match_case(64, 64, 9, "nan")
    idx, d2 = ref.match(fa, fb)
    assert (idx[::7] == -1).all() and not np.isin(idx, np.arange(0, 64, 5)).any()
    assert (idx[np.isfinite(fa).all(axis=1)] >= 0).all()


def test_ransac_restatement():
    want = gf.ransac_want("planted")
    args, kw = gf.ransac_args("planted")
    src, dst = args[0], args[1]
    passed = want["info"]["passed"]
    assert (np.diff(np.concatenate(([args[2]], passed))) <= 0).all()
    assert want["count"][0] == 20 and abs(want["s"][0] - 1.3) < 1e-9
    # a model maps its own triple onto the target triple, and is a similarity
    hs, count, models = want["survivors"]
    for h, m in list(zip(hs, models))[:50]:
        tup, words = ref.philox_ref.floyd_tuple(kw["seed"], int(h), len(src), 3)
        s, R, t = m[0], m[1:10].reshape(3, 3), m[10:]
        assert np.allclose(R @ R.T, np.eye(3), atol=1e-12) and np.linalg.det(R) > 0.0
        # the centroids agree exactly up to rounding; the vertices within the edge tolerance
        ca, cb = src[tup].mean(axis=0), dst[tup].mean(axis=0)
        assert np.allclose(s * R @ ca + t, cb, atol=1e-12)
        assert np.abs(s * src[tup] @ R.T + t - dst[tup]).max() <= 0.15 * 6.0 * 1.8
    umey = eval_ref.umeyama(src[ref.philox_ref.floyd_tuples(3, int(want["h"][0]), 1, 200, 3)[0]],
                            dst[ref.philox_ref.floyd_tuples(3, int(want["h"][0]), 1, 200, 3)[0]])
    assert np.allclose(umey[1], want["R"][0], atol=1e-9) and abs(umey[0] - want["s"][0]) < 1e-9
    at, below = gf.ransac_want("at_the_distance"), gf.ransac_want("below_the_distance")
    assert at["count"][0] == 4 and at["h"][0] == 0 and 0 not in below["h"][below["count"] == 4]
    assert gf.ransac_want("rigid")["count"][0] == 60
    for name in ("all_gated_out", "scale_gate_empty", "collinear"):
        assert len(gf.ransac_want(name)["h"]) == 0


def test_pruned_mesh_distance_is_the_brute_force():
    v, f = gf.egg()
    pts, _ = gf.cloud("outlier", 2)
    T = (1.2, gf.rf.rotation((1.0, 2.0, 3.0), 100.0), np.array([3.0, -2.0, 7.0]))
    moved = register_ref.transform(pts[::6], *T)
    assert np.array_equal(ref.mesh_d2(moved, v, f), eval_ref.mesh_distance(moved, v, f)[0])
    rec = register_ref.step(pts[::6], v, f, *T, register_ref.mesh_box(v, f)[0], 0.75, np.inf,
                            "point")
    assert ref.trimmed_rms(pts[::6], v, f, *T, 0.75) == np.sqrt(rec["moments"][16] / rec["kept"])


@pytest.mark.parametrize("pose", range(len(gf.POSES)))
@pytest.mark.parametrize("name", gf.CLOUD_NAMES)
def test_the_coarse_pose_lands_in_the_basin(name, pose):
    got = gf.coarse(name, pose)
    cand = got["candidates"]
    rot, ds, dt = gf.pose_errors(*got["coarse"], pose)
    top = gf.pose_errors(cand["s"][0], cand["R"][0], cand["t"][0], pose)[0]
    print(f"{name} pose {pose}: {len(got['src'])} matches, survivors per gate "
          f"{cand['info']['passed'].tolist()}, counts {cand['count'].tolist()}; verified "
          f"candidate {got['chosen']} (trimmed rms {got['rms'][got['chosen']]:.4f}): rotation "
          f"{rot:.2f} deg, |s / s_true - 1| {ds:.2e}, |t - t_true| / L {dt:.2e}; the top count "
          f"is {top:.2f} deg off")
    assert len(gf.POSES) >= 6 and 60.0 <= gf.POSES[pose][1] <= 180.0
    assert rot <= gf.BASIN_DEG


def test_python_arguments_without_a_device():
    p, nr, _ = gf.fpfh_cases()["random_65_k8"]
    for call in (lambda: cloud.fpfh(p, nr, k=0), lambda: cloud.fpfh(p, nr, k=64),
                 lambda: cloud.fpfh(p, nr[:3], k=4), lambda: cloud.fpfh(p[:, :2], nr, k=4),
                 lambda: cloud.match_features(np.zeros((3, 65)), np.zeros((3, 65))),
                 lambda: cloud.match_features(np.zeros((3, 4)), np.zeros((3, 5))),
                 lambda: ev.ransac_similarity(p, p[:-1], 10, 0.1)):
        with pytest.raises(ValueError):
            call()
    assert _ffi.FEATURE_MATCH_TILE == ref.TILE and _ffi.SIM3_CHUNK == ref.CHUNK
    assert _ffi.C.sizeof(_ffi.Sim3Candidate) == 120 and _ffi.C.sizeof(_ffi.Sim3Info) == 64
    n = ev.face_normals(*gf.egg())
    assert np.allclose((n * n).sum(axis=1), 1.0) and np.array_equal(n, ref.face_normals(*gf.egg()))
    assert ev.rms_radius(p) == ref.rms_radius(p)
