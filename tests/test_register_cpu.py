"""Registration without a GPU: the numpy restatement of the step and its loop
(tests/register_ref.py) on the cases of tests/register_fixture.py, and the host side of
tsbb15_amd.evaluation.register.

Measured here on the blob (1 200 samples, 8 degrees, 4 % and 0.66 units off on a diagonal of
15.69), plane metric, rms per step:
    clean, keep 1.0       5.7e-1 1.4e-1 4.1e-3 5.3e-6 2.0e-12: converged at step 5; rotation error
                          0, |t - t_true| / L 4.9e-13, |s / s_true - 1| 3.8e-13
    outliers, keep 0.75   4.4e-1 1.2e-1 1.2e-2 1.2e-4 1.7e-7 5.5e-14: step 6; 0, 8.7e-15, 1.5e-14
The point metric is still 4.4 degrees off after 8 steps (rms 5.7e-1 .. 2.0e-1).
fp64 moments against the restatement's own longdouble run, worst deviation per slot relative to
the sum of the terms' magnitudes: point 1.808e-16 (k_one), plane 2.432e-16 (count_2048); both
below eps, so the GPU's bar, 4 x the figure floored at 16 eps, is 16 eps = 3.6e-15.
"""
import ctypes

import numpy as np
import pytest

import eval_ref
import register_fixture as rf
import register_ref as ref
from tsbb15_amd import _ffi, evaluation as ev

ROTATION_BAR_DEG, TRANSLATION_BAR, SCALE_BAR = 1e-8, 1e-10, 1e-10


def truth_errors(s, R, t):
    ts, tR, tt = rf.TRUTH
    return (eval_ref.rotation_angle_deg(R, tR),
            float(np.linalg.norm(t - tt)) / rf.blob_diagonal(), abs(s / ts - 1.0))


def test_blob():
    v, f = rf.blob()
    assert v.shape == (762, 3) and f.shape == (1520, 3)
    assert eval_ref.face_valid(v, f).all()
    # closed and consistently wound: every directed edge once, its reverse once
    e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]).astype(np.int64)
    fwd = set(map(tuple, e))
    assert len(fwd) == len(e) and fwd == set(map(tuple, e[:, ::-1]))
    assert 15.0 < rf.blob_diagonal() < 16.5
    for name, n in (("clean", 1200), ("outlier", 1500), ("noisy", 1200)):
        assert rf.clouds()[name][0].shape == (n, 3)
    s, R, t = rf.TRUTH
    on = ev.apply_similarity(rf.clouds()["clean"][0], s, R, t)
    assert ref.step(on[:50], v, f, 1.0, np.eye(3), np.zeros(3), np.zeros(3))["d2"].max() < 1e-25


@pytest.mark.parametrize("name", ("clean", "outlier"))
def test_plane_metric_reaches_the_truth(name):
    tr = rf.blob_trace(name, "plane")
    rot, dt, dsc = truth_errors(tr["s"], tr["R"], tr["t"])
    print(f"{name}: {tr['iterations']} steps, rms {tr['rms']}, kept {tr['kept'][-1]}, rotation "
          f"error {rot:.3e} deg, |t - t_true| / L {dt:.3e}, |s / s_true - 1| {dsc:.3e}")
    assert tr["iterations"] <= rf.COMPARE_ITERATIONS and tr["converged"]
    assert rot <= ROTATION_BAR_DEG and dt <= TRANSLATION_BAR and dsc <= SCALE_BAR
    keep = rf.clouds()[name][1]
    assert (tr["kept"] == ref.trim_rank(keep, len(rf.clouds()[name][0]))).all()
    if name == "outlier":     # the samples are kept, the outliers are not
        assert tr["mask"][:rf.SAMPLES].sum() == tr["kept"][-1]


def test_point_metric_lowers_the_rms_at_every_step():
    tr = rf.blob_trace("clean", "point")
    print(f"point: rms {tr['rms']}, rotation error {truth_errors(tr['s'], tr['R'], tr['t'])[0]:.3f}")
    assert tr["iterations"] == rf.COMPARE_ITERATIONS
    assert (np.diff(tr["rms"]) < 0.0).all()


def test_trim_rank():
    for keep, m, k in ((0.7, 10, 7), (0.3, 10, 3), (0.1, 30, 3), (0.6, 5, 3), (0.29, 100, 29),
                       (0.57, 100, 57), (1.0, 7, 7), (1e-6, 40, 1), (0.75, 1500, 1125),
                       (0.5, 3, 2), (1.0, 1, 1), (0.3, 0, 0), (0.07, 100, 7), (0.55, 100, 55),
                       (0.14, 50, 7)):
        assert ref.trim_rank(keep, m) == k, (keep, m)
    # why the rule subtracts 1e-9: these products land above their integer
    assert np.ceil(0.07 * 100) == 8.0 and np.ceil(0.55 * 100) == 56.0


@pytest.mark.parametrize("name", sorted(rf.EXPECTED))
def test_hand_placed_cases(name):
    for metric in rf.METRICS:
        r = rf.small_step(name, metric)
        assert (r["matched"], r["k"], r["kept"]) == rf.EXPECTED[name]
    r = rf.small_step(name, "plane")
    if name == "none":
        assert np.isnan(r["tau"]) and not r["mask"].any() and (r["moments"] == 0.0).all()
        return
    d2 = r["d2"][r["face"] >= 0]
    assert r["tau"] == np.sort(d2)[r["k"] - 1]
    if name == "ties":
        assert r["tau"] == 1.0 and r["mask"].tolist() == [True, True, True, False, False]
    if name == "on_face":
        assert r["tau"] == 0.0 and r["mask"].sum() == 3
    if name == "unmatched":
        assert np.isinf(r["d2"][3]) and np.isnan(r["d2"][4:]).all() and not r["mask"][3:].any()
    if name == "neighbours":
        keys = d2.view(np.uint64)
        assert len(set(keys >> np.uint64(8))) == 1 and len(set(keys)) == 5
    if name == "binades":
        # every pass of the select has candidates in more than one bin
        keys, prefix = d2.view(np.uint64), np.float64(r["tau"]).view(np.uint64)
        for p in range(8):
            sh = np.uint64(56 - 8 * p)
            cand = keys if p == 0 else keys[(keys >> (sh + np.uint64(8)))
                                            == (prefix >> (sh + np.uint64(8)))]
            assert len(set((cand >> sh) & np.uint64(255))) > 1, p


def test_moments_against_longdouble():
    for metric in rf.METRICS:
        worst, where = 0.0, None
        steps = [(n, rf.small_step) for n in rf.SMALL_NAMES] + [(n, rf.blob_step)
                                                                 for n in rf.CLOUD_NAMES]
        for name, fn in steps:
            a, b = fn(name, metric), fn(name, metric, np.longdouble)
            assert (a["matched"], a["kept"], a["tau"]) == (b["matched"], b["kept"], b["tau"]) \
                or np.isnan(a["tau"])
            dev = rf.deviation(a["moments"], b["moments"], b["scale"])
            worst, where = (dev, name) if dev > worst else (worst, where)
            assert (a["moments"][ref.NS[metric]:] == 0.0).all()
        print(f"{metric}: worst deviation {worst:.3e} ({where}), recorded "
              f"{rf.MEASURED[metric]:.3e}, bar {rf.bar(metric):.3e}")
        assert worst <= rf.MEASURED[metric]


def test_ordered_sum():
    rs = np.random.RandomState(4)
    for n in (1, 255, 257, rf.BLOCK, 2 * rf.BLOCK + 1):
        w = rs.standard_normal((n, 3)) * 10.0 ** rs.uniform(-3, 3, (n, 1))
        got, exact = ref.ordered_sum(w), np.array([np.sum(w[:, j].astype(np.longdouble))
                                                   for j in range(3)])
        assert (np.abs(got - exact) <= 16 * rf.EPS * np.abs(w).sum(axis=0)).all()
    # the order: the first block's lane 0 adds rows 0 and 256, and folds with lane 128 first
    w = np.zeros((rf.BLOCK, 1))
    w[0], w[256], w[128] = 1.0, 2.0 ** -53, 2.0 ** -53
    assert ref.ordered_sum(w)[0] == 1.0
    w[0], w[256], w[128] = 2.0 ** -53, 2.0 ** -53, 1.0
    assert ref.ordered_sum(w)[0] == 1.0 + 2.0 ** -52


def test_host_update_agrees_with_the_restatement():
    origin = ref.mesh_box(*rf.blob())[0]
    for metric in rf.METRICS:
        r = rf.blob_step("outlier", metric)
        rec = {"moments": r["moments"], "kept": r["kept"]}
        for with_scale in (True, False):
            a = ev.step_update(metric, rec, origin, with_scale)
            b = ref.update(metric, r["moments"], r["kept"], origin, with_scale)
            for x, y in zip(a, b):
                assert np.array_equal(x, y)
            assert with_scale or a[0] == 1.0
            assert abs(np.linalg.det(a[1]) - 1.0) < 1e-14
            assert np.abs(a[1] @ a[1].T - np.eye(3)).max() < 1e-14
        assert ev.step_rms(metric, rec) == np.sqrt(r["moments"][ref.RMS_SLOT[metric]] / r["kept"])
    assert np.array_equal(ev.mesh_box(*rf.blob())[0], origin)
    # a planar target leaves the plane system singular: lstsq takes the minimum-norm step
    r = rf.small_step("k_all", "plane")
    ds, dR, dt = ev.step_update("plane", {"moments": r["moments"], "kept": r["kept"]},
                                ref.mesh_box(rf.TRIANGLE, rf.TRI_FACES)[0])
    assert np.isfinite(ds) and np.isfinite(dR).all() and np.isfinite(dt).all()


def test_argument_errors_before_any_launch():
    v, f = rf.blob()
    p = rf.clouds()["clean"][0]
    for kw in ({"keep": 0.0}, {"keep": 1.5}, {"keep": np.nan}, {"metric": "line"},
               {"init": (np.nan, np.eye(3), np.zeros(3))},
               {"init": (1.0, np.eye(3), np.array([0.0, np.inf, 0.0]))},
               {"init": (1.0, np.eye(4), np.zeros(3))}, {"max_dist": 0.0}, {"max_iter": 0}):
        with pytest.raises(ValueError):
            ev.register(p, v, f, **kw)
    for wrong in (p[:, :2], p.reshape(-1), p[:0]):
        with pytest.raises(ValueError):
            ev.register(wrong, v, f)


def test_step_record_layout():
    assert ctypes.sizeof(_ffi.EvalStep) == 360
    assert len(_ffi.EVAL_REG_STAGES) == 4 and _ffi.EVAL_REG_SLOTS == ref.SLOTS
    assert _ffi.EVAL_REG_BLOCK == ref.BLOCK == ev.REG_BLOCK
