"""The evaluation stage without a GPU: the numpy restatement of the mesh distance against hand-
written answers and against its own longdouble run, and the host functions of
tsbb15_amd.evaluation (sampling, the two measures, the camera algebra).

Measured here, fp64 against longdouble, worst |d2 - d2_ld| / L^2 per case (L the box diagonal):
one_triangle 0, s12 4.485e-17, random 1.587e-17, big_and_small 4.485e-17, edges 1.312e-12 (its
queries 100 box widths away have d2 = 1e4 L^2), half 1.304e-17, degenerate 4.9e-22.  All but
`edges` lie below eps, so the GPU's bar, 4 x the figure floored at 16 eps, is 16 eps = 3.6e-15
for them and 5.6e-12 for `edges` (eval_fixture.MEASURED holds the figures rounded up; the test
asserts that they still bound the run).
"""
import os
import re

import numpy as np
import pytest

import dense_fixture
import eval_fixture as ef
import eval_ref
from conftest import PKG_DIR, golden
from tsbb15_amd import _ffi, evaluation as ev


def test_constants_match_the_header():
    src = open(_ffi.HEADER_PATH).read()
    for name, value in (("POINTS", ev.MAX_POINTS), ("CELLS", ev.MAX_CELLS),
                        ("ENTRIES", ev.MAX_ENTRIES)):
        m = re.search(r"#define RS_EVAL_MAX_%s \(1LL << (\d+)\)" % name, src)
        assert 1 << int(m.group(1)) == value
    slots = re.search(r"#define RS_EVAL_TIMING_SLOTS (\d+)", src)
    assert int(slots.group(1)) == len(ev.STAGES) == len(_ffi.EVAL_STAGES)
    assert _ffi.C.sizeof(_ffi.EvalInfo) == 64
    assert "/* 64 bytes */" in src
    chunk = re.search(r"kEvalScanThreads = (\d+);\s*constexpr int kEvalScanItems = (\d+);",
                      open(os.path.join(PKG_DIR, "csrc", "eval.hip")).read())
    assert int(chunk.group(1)) * int(chunk.group(2)) == ef.SCAN_CHUNK


def test_hand_written_answers():
    d2, face, closest = ef.reference("one_triangle")[:3]
    for (q, c, d, what), got_d, got_f, got_c in zip(ef.HAND, d2, face, closest):
        assert got_d == d, what
        assert got_f == 0, what
        assert np.array_equal(got_c, c), what
    # the same in longdouble
    c = ef.cases()["one_triangle"]
    d2l = eval_ref.mesh_distance(c.queries, c.vertices, c.faces, dtype=np.longdouble)[0]
    assert np.array_equal(d2l, [h[2] for h in ef.HAND])


@pytest.mark.parametrize("name", ef.CASE_NAMES)
def test_restatement_against_longdouble(name):
    c = ef.cases()[name]
    d2, face, closest, pairs = ef.reference(name)
    d2l, facel, closestl = eval_ref.mesh_distance(c.queries, c.vertices, c.faces, c.max_dist,
                                                  dtype=np.longdouble)
    L2 = ef.diagonal(c) ** 2
    both = np.isfinite(d2) & np.isfinite(d2l)
    assert np.array_equal(np.isnan(d2), np.isnan(d2l))
    assert np.array_equal(np.isfinite(d2), np.isfinite(d2l))
    worst = float(np.abs(d2[both] - d2l[both]).max() / L2) if both.any() else 0.0
    print(f"{name}: worst |d2 - d2_ld| / L^2 = {worst:.3e} (L = {np.sqrt(L2):.4f}), "
          f"recorded {ef.MEASURED[name]:.3e}, bar {ef.bar(name):.3e}")
    assert worst <= ef.MEASURED[name]
    # another face only where the two are as close as that error
    differ = both & (face != facel)
    rows = np.flatnonzero(differ)
    gap = np.abs(pairs[rows, face[rows]] - pairs[rows, facel[rows]])
    print(f"{name}: {len(rows)} rows pick another face, largest gap / L^2 = "
          f"{float(gap.max() / L2) if len(rows) else 0.0:.3e}")
    assert (gap <= max(ef.MEASURED[name], ef.EPS) * L2).all()
    # the closest point lies on its face and at the stated distance
    ok = face >= 0
    tri = c.vertices[c.faces[face[ok]]]
    bary = eval_ref.barycentric(closest[ok], tri[:, 0], tri[:, 1], tri[:, 2])
    assert bary.min() >= -1e-9 and bary.max() <= 1.0 + 1e-9
    e = c.queries[ok] - closest[ok]
    assert np.array_equal(e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1] + e[:, 2] * e[:, 2], d2[ok])


def test_case_edges():
    cs = ef.cases()
    half = ef.reference("half")[0]
    share = float(np.isinf(half).mean())
    print(f"half: {share:.3f} of the queries lie beyond max_dist")
    assert 0.25 < share < 0.75
    d2, face, closest = ef.reference("degenerate")[:3]
    c = cs["degenerate"]
    assert (~eval_ref.face_valid(c.vertices, c.faces)).sum() == ef.DEGENERATE_SKIPPED
    assert np.isnan(d2[len(ef.HAND):len(ef.HAND) + 3]).all()
    assert (face[len(ef.HAND):len(ef.HAND) + 3] == -1).all()
    # face 1 and its mirror image 6 tie on every hand query: the lower index wins
    assert (face[:len(ef.HAND)] == 1).all()
    assert np.array_equal(d2[:len(ef.HAND)], [h[2] for h in ef.HAND])
    # no face at all
    d2, face, closest = eval_ref.mesh_distance(c.queries, c.vertices, np.zeros((0, 3), np.int32))
    assert np.isinf(d2[:len(ef.HAND)]).all() and (face == -1).all() and np.isnan(closest).all()
    # the cases that must cross a boundary do
    dims, entries, _ = eval_ref.grid_entries(cs["random"].vertices, cs["random"].faces,
                                             ef.RANDOM_CELL)
    assert np.prod(dims) > ef.SCAN_CHUNK
    big = cs["big_and_small"]
    dims, entries, largest = eval_ref.grid_entries(big.vertices, big.faces,
                                                   ev.default_cell(big.vertices, big.faces))
    _, small, _ = eval_ref.grid_entries(cs["s12"].vertices, cs["s12"].faces,
                                        ev.default_cell(big.vertices, big.faces))
    assert entries == small + int(np.prod(dims))
    # the grown box reaches outside the grid, and the far queries start at a late ring
    lo, hi = ef.box_of(cs["s12"].vertices, cs["s12"].faces)
    q = cs["s12"].queries[-500:]
    outside = ((q < lo) | (q > hi)).any(axis=1)
    assert 50 < outside.sum() < 450
    assert (np.abs(cs["edges"].queries[-3:] - lo).max(axis=1) > 90 * (hi - lo).max()).all()


def test_default_cell():
    c = ef.cases()["s12"]
    tri = c.vertices[c.faces]
    diag = np.sqrt(((tri.max(axis=1) - tri.min(axis=1)) ** 2).sum(axis=1))
    assert ev.default_cell(c.vertices, c.faces) == 2.0 * np.median(diag)
    # one huge and flat mesh: the extent / 512 wins
    v = np.array([[0.0, 0, 0], [1e-3, 0, 0], [0, 1e-3, 0], [1000.0, 0, 0]])
    f = np.array([[0, 1, 2], [0, 1, 2], [0, 1, 3]])
    assert ev.default_cell(v, f) == 1000.0 / 512.0
    assert ev.default_cell(v, np.zeros((0, 3), np.int32)) == 1.0


def test_accuracy_and_completeness():
    d = np.array([0.5, 0.1, 0.4, 0.2, 0.3, 0.6, 0.9, 0.8, 0.7, 1.0])
    assert ev.accuracy(d, 0.9) == 0.9          # ceil(9.0) = 9: lands on an element
    assert ev.accuracy(d, 0.7) == 0.7          # 0.7 * 10 = 7.000000000000001 in fp64
    assert ev.accuracy(d, 0.85) == 0.9         # ceil(8.5) = 9
    assert ev.accuracy(d, 0.01) == 0.1
    assert ev.accuracy(d, 1.0) == 1.0
    for fr in (0.05, 0.1, 0.33, 0.5, 0.75, 0.9, 0.99, 1.0):
        assert ev.accuracy(d, fr) == eval_ref.kth_smallest(d, fr)
    ties = np.array([2.0, 1.0, 2.0, 2.0, 3.0])
    assert ev.accuracy(ties, 0.4) == 2.0 and ev.accuracy(ties, 0.2) == 1.0
    assert ev.accuracy(ties, 0.8) == 2.0 and ev.accuracy(ties, 0.81) == 3.0
    inf = np.array([1.0, np.inf, 2.0, np.inf])
    assert ev.accuracy(inf, 0.5) == 2.0 and ev.accuracy(inf, 0.75) == np.inf
    with pytest.raises(ValueError):
        ev.accuracy(np.array([1.0, np.nan]), 0.9)
    with pytest.raises(ValueError):
        ev.accuracy(np.array([]), 0.9)
    with pytest.raises(ValueError):
        ev.accuracy(d, 0.0)
    assert ev.completeness(d, 0.3) == 0.3      # <=, so the tie at 0.3 counts
    assert ev.completeness(inf, 5.0) == 0.5
    assert ev.completeness(ties, 2.0) == 0.8
    assert ev.completeness(np.array([np.nan, 1.0]), 2.0) == 0.5
    assert ev.completeness(d, 0.0) == 0.0


def test_sample_surface():
    c = ef.cases()["degenerate"]
    v = np.where(np.isfinite(c.vertices), c.vertices, 0.0)
    p, f = ev.sample_surface(v, c.faces, 4000, seed=3)
    p2, f2 = ev.sample_surface(v, c.faces, 4000, seed=3)
    assert p.tobytes() == p2.tobytes() and np.array_equal(f, f2)
    assert not np.array_equal(p, ev.sample_surface(v, c.faces, 4000, seed=4)[0])
    assert not np.isin(f, (0, 2)).any()        # no area: never drawn
    tri = v[c.faces[f]]
    bary = eval_ref.barycentric(p, tri[:, 0], tri[:, 1], tri[:, 2])
    assert bary.min() >= -1e-12 and bary.max() <= 1.0 + 1e-12
    assert np.abs((bary[:, :, None] * tri).sum(axis=1) - p).max() < 1e-12
    # by area: two triangles, one three times the other
    v2 = np.array([[0.0, 0, 0], [1, 0, 0], [0, 1, 0], [3, 0, 0], [0, 0, 1]])
    f2 = np.array([[0, 1, 2], [0, 3, 4]])
    share = (ev.sample_surface(v2, f2, 20000, seed=1)[1] == 1).mean()
    assert abs(share - 0.75) < 4 * np.sqrt(0.75 * 0.25 / 20000)
    # a face with a vertex that is not finite is never drawn either
    p, f = ev.sample_surface(c.vertices, c.faces, 500, seed=0)
    assert np.isfinite(p).all() and np.isin(f, (1, 4, 6)).all()
    assert ev.sample_surface(v2, f2, 0)[0].shape == (0, 3)
    with pytest.raises(ValueError):
        ev.sample_surface(v2, np.array([[0, 0, 1]]), 5)


def _seeded_similarity(seed):
    rs = np.random.RandomState(seed)
    R = dense_fixture.rodrigues(rs.standard_normal(3), rs.uniform(0.5, 3.0))
    return rs.uniform(0.3, 3.0), R, rs.standard_normal(3)


def test_align_similarity():
    rs = np.random.RandomState(8)
    src = rs.standard_normal((40, 3))
    s, R, t = _seeded_similarity(9)
    dst = ev.apply_similarity(src, s, R, t)
    gs, gR, gt = ev.align_similarity(src, dst)
    assert abs(gs - s) < 1e-12 and np.abs(gR - R).max() < 1e-12 and np.abs(gt - t).max() < 1e-12
    rigid = ev.apply_similarity(src, 1.0, R, t)
    gs, gR, gt = ev.align_similarity(src, rigid, with_scale=False)
    assert gs == 1.0 and np.abs(gR - R).max() < 1e-12 and np.abs(gt - t).max() < 1e-12
    # against the paper's formulas on noisy data
    noisy = dst + 0.05 * rs.standard_normal(dst.shape)
    for scale in (True, False):
        a, b = ev.align_similarity(src, noisy, scale), eval_ref.umeyama(src, noisy, scale)
        assert abs(a[0] - b[0]) < 1e-12
        assert np.abs(a[1] - b[1]).max() < 1e-12 and np.abs(a[2] - b[2]).max() < 1e-12
    # a mirrored set: still a rotation, and the best one (no rotation does better)
    mirrored = dst * np.array([1.0, 1.0, -1.0])
    ms, mR, mt = ev.align_similarity(src, mirrored)
    assert abs(np.linalg.det(mR) - 1.0) < 1e-12 and np.abs(mR @ mR.T - np.eye(3)).max() < 1e-12
    ref = eval_ref.umeyama(src, mirrored)
    assert np.abs(mR - ref[1]).max() < 1e-12 and abs(ms - ref[0]) < 1e-12
    cost = ((ev.apply_similarity(src, ms, mR, mt) - mirrored) ** 2).sum()
    assert cost > 1.0
    for k in range(20):
        s2, R2, t2 = _seeded_similarity(100 + k)
        R2 = mR @ dense_fixture.rodrigues(R2[0], 0.05)
        moved = ev.apply_similarity(src, ms, R2, 0.0)
        t2 = mirrored.mean(axis=0) - moved.mean(axis=0)
        assert ((moved + t2 - mirrored) ** 2).sum() >= cost


def _reproduces(P, K, R, t):
    rec = K @ np.concatenate((R, t[..., None]), axis=-1)
    scale = (rec * P).sum(axis=(-2, -1), keepdims=True) / (rec * rec).sum(axis=(-2, -1),
                                                                          keepdims=True)
    unit = np.abs(P).max(axis=(-2, -1), keepdims=True)
    return float((np.abs(rec * scale - P) / unit).max())


def test_decompose_projection():
    cams = dense_fixture.cameras()
    for scale in (1.0, -2.5, 1e-3):
        P = scale * (dense_fixture.K @ cams)
        K, R, t = ev.decompose_projection(P)
        assert K.shape == (len(cams), 3, 3) and t.shape == (len(cams), 3)
        assert np.abs(K - dense_fixture.K).max() < 1e-9
        assert np.abs(R - cams[:, :, :3]).max() < 1e-12
        assert np.abs(t - cams[:, :, 3]).max() < 1e-12
    K1, R1, t1 = ev.decompose_projection(P[1])
    assert K1.shape == (3, 3) and np.array_equal(K1, K[1]) and np.array_equal(t1, t[1])
    P = golden("evaluation.npz")["P"]
    K, R, t = ev.decompose_projection(P)
    assert _reproduces(P, K, R, t) < 1e-9
    assert (np.diagonal(K, axis1=1, axis2=2) > 0).all() and (K[:, 2, 2] == 1.0).all()
    assert (K[:, 1, 0] == 0).all() and (K[:, 2, 0] == 0).all() and (K[:, 2, 1] == 0).all()
    assert np.abs(np.linalg.det(R) - 1.0).max() < 1e-12
    assert np.abs(R @ R.transpose(0, 2, 1) - np.eye(3)).max() < 1e-12
    with pytest.raises(ValueError):
        ev.decompose_projection(np.zeros((3, 4)))
    with pytest.raises(ValueError):
        ev.decompose_projection(np.zeros((4, 4)))


def _camera_ring(n=12, seed=4):
    rs = np.random.RandomState(seed)
    R, t = [], []
    for k in range(n):
        a = 2.0 * np.pi * k / n
        centre = np.array([2.0 * np.cos(a), 0.3 * rs.standard_normal(), 2.0 * np.sin(a)])
        Rk = dense_fixture.rodrigues(rs.standard_normal(3), rs.uniform(0.0, 3.0))
        R.append(Rk)
        t.append(-Rk @ centre)
    return np.array(R), np.array(t)


def test_camera_errors_on_a_gauged_copy():
    R_gt, t_gt = _camera_ring()
    s, Rw, tw = _seeded_similarity(21)
    G = np.diag([-1.0, 1.0, -1.0]) @ dense_fixture.rodrigues((1.0, 2.0, 0.5), 0.2)
    # the world moved by X' = (Rw X + tw) / s ... as an estimate would have it: X = s Rw' X' + t
    c_gt = -np.einsum('nji,nj->ni', R_gt, t_gt)
    c_est = ev.apply_similarity(c_gt, 1.0 / s, Rw.T, -Rw.T @ tw / s)
    R_est = G.T @ R_gt @ Rw          # camera frame turned by the gauge, world by Rw
    t_est = -np.einsum('nij,nj->ni', R_est, c_est)
    e = ev.camera_errors(R_est, t_est, R_gt, t_gt)
    assert e["centre_error"].max() < 1e-12 and e["rotation_error_deg"].max() < 1e-5
    assert abs(e["s"] - s) < 1e-12 and np.abs(e["R"] - Rw).max() < 1e-12
    assert np.abs(e["frame"] - G).max() < 1e-12
    assert e["orthogonality_defect"] < 1e-14
    for Re, Rg in zip(R_est, R_gt):
        assert eval_ref.rotation_angle_deg(Rg, e["frame"] @ Re @ e["R"].T) < 1e-5
    off = ev.camera_errors(R_est, t_est, R_gt, t_gt, frame=False)
    assert np.array_equal(off["frame"], np.eye(3))
    assert off["rotation_error_deg"].min() > 150.0 and off["centre_error"].max() < 1e-12
    # one camera turned by 3 degrees and moved by 0.1 shows up as that
    R_bad, t_bad = R_est.copy(), t_est.copy()
    R_bad[5] = dense_fixture.rodrigues((0.0, 0.0, 1.0), np.radians(3.0)) @ R_est[5]
    far = ev.camera_errors(R_bad, t_bad, R_gt, t_gt)
    assert 2.5 < far["rotation_error_deg"][5] < 3.0
    assert np.delete(far["rotation_error_deg"], 5).max() < 0.5
    # a sheared R is reported and replaced
    R_sh = R_est @ (np.eye(3) + 0.01 * np.triu(np.ones((3, 3)), 1))
    sh = ev.camera_errors(R_sh, t_est, R_gt, t_gt)
    assert 0.005 < sh["orthogonality_defect"] < 0.05 and sh["rotation_error_deg"].max() < 1.0
    with pytest.raises(ValueError):
        ev.camera_errors(R_est[:3], t_est, R_gt, t_gt)


def test_camera_errors_on_the_reference_files():
    g = golden("evaluation.npz")
    assert g["P"].shape == (36, 3, 4) and g["R_eval_clean"].shape == (35, 3, 3)
    _, R_gt, t_gt = ev.decompose_projection(g["P"][:35])
    e = ev.camera_errors(g["R_eval_clean"], g["t_eval_clean"], R_gt, t_gt)
    _, R_all, t_all = ev.decompose_projection(g["P"])
    c_all = -np.einsum('nji,nj->ni', R_all, t_all)     # the whole turntable
    radius = np.linalg.norm(c_all - c_all.mean(axis=0), axis=1)
    assert np.abs(radius - 1.0).max() < 0.01          # the errors below are in these units
    med, worst = float(np.median(e["centre_error"])), float(e["centre_error"].max())
    rot = float(np.median(e["rotation_error_deg"]))
    print(f"centres: median {med:.4f}, max {worst:.4f}; rotation: median {rot:.3f} deg, "
          f"max {e['rotation_error_deg'].max():.3f} deg; defect {e['orthogonality_defect']:.4f}")
    assert rot < 5.0
    assert abs(med - 0.028) <= 0.0028 and abs(worst - 0.098) <= 0.0098
    assert np.abs(e["frame"] - np.diag([-1.0, 1.0, -1.0])).max() < 0.15
    assert 0.01 < e["orthogonality_defect"] < 0.2
    off = ev.camera_errors(g["R_eval_clean"], g["t_eval_clean"], R_gt, t_gt, frame=False)
    assert np.median(off["rotation_error_deg"]) > 90.0
    assert np.array_equal(off["centre_error"], e["centre_error"])
