"""The numpy restatement of the dense stage (tests/dense_ref.py) on its own, on the scenes of
tests/dense_fixture.py: that the definition finds the planes, that fp32 arithmetic in another
summation order stays close to it (the source of the GPU test's SCORE_BAR), and that the
fixtures keep every discrete decision away from its boundary, so the GPU test may compare
validity flags and agreement counts exactly.  No GPU.

Measured on the base scene (40 x 56, two sources, D = 12, depth 4 at index 5), pixels at least
4 px inside the border of valid windows:
  fronto-parallel plane, patch 3 / 5 / 7: the winner is index 5 on 100 % of them;
  slanted plane: the winner is within one index of the truth on 99.8 / 100 / 100 %;
  median best-to-second gap 0.19-0.21 (fronto-parallel) and 0.11-0.13 (slanted);
  fp32 with reversed window sums against fp64: at most 5.07e-06 in any cost over all thirteen
  sweeps of the GPU test, no validity flag changes; SCORE_BAR = 8 x that = 4.06e-05.
"""
import numpy as np
import pytest

import dense_fixture as df
import dense_ref as dr

BASE = ["fronto_p3", "fronto_p5", "fronto_p7", "slanted_p3", "slanted_p5", "slanted_p7"]


def _gap(volume):
    srt = np.sort(np.where(np.isnan(volume), -np.inf, volume), axis=0)
    with np.errstate(invalid="ignore"):
        return srt[-1] - srt[-2]


@pytest.mark.parametrize("name", BASE)
def test_accuracy_and_gap(name):
    index, delta, score, nvalid, volume, _ = df.reference_sweeps()[name]
    patch = df.sweep_cases()[name][6]
    _, _, depth = df.scene(name.split("_")[0])
    valid = index >= 0
    m = df.interior(df.H, df.W, patch) & valid
    assert m.sum() > 1000
    exact = float((index[m] == df.TRUE_INDEX).mean())
    within = float((np.abs(index - df.true_index(depth[0]))[m] <= 1.0).mean())
    gap = _gap(volume)[valid]
    bar = df.score_bar()
    clear = float((gap > 2 * bar).mean())
    print(f"{name}: exact {exact:.4f}, within one {within:.4f}, median gap "
          f"{float(np.median(gap)):.3f}, gap above 2 SCORE_BAR on {clear:.4f}")
    if name.startswith("fronto"):
        assert exact == 1.0
    else:
        assert within >= 0.98
    assert clear >= 0.90
    # the outputs' own invariants
    assert np.all(np.abs(delta) <= 0.5) and np.all(delta[~valid] == 0)
    assert np.all(np.isnan(score[~valid])) and np.all(nvalid[~valid] == 0)
    assert np.all(nvalid[valid] >= 1)
    r = patch // 2
    border = np.ones(index.shape, bool)
    border[r:-r, r:-r] = False
    assert np.all(index[border] == -1)


def test_refined_depth_is_close():
    """Sub-index refinement on the slanted plane: the refined depth is within a quarter of a
    depth step of the truth on 95 % of the interior."""
    index, delta, *_ = df.reference_sweeps()["slanted_p7"]
    depth = dr.refine_depth(index, delta, df.DEPTHS)
    truth = df.scene("slanted")[2][0]
    m = df.interior(df.H, df.W, 7) & (index >= 0)
    off = np.abs(df.true_index(depth) - df.true_index(truth))[m]
    print(f"refined depth: median {np.median(off):.3f} steps, 95 % {np.percentile(off, 95):.3f}")
    assert np.percentile(off, 95) <= 0.25
    assert np.isnan(depth[index < 0]).all() and np.isfinite(depth[index >= 0]).all()
    # index without delta is the ladder itself
    assert np.array_equal(dr.refine_depth(index, np.zeros_like(delta), df.DEPTHS)[m],
                          (1.0 / (1.0 / df.DEPTHS))[index[m]])


def test_fp32_reversed_against_fp64():
    devs = df.fp32_deviation()
    for name, (dev, same) in devs.items():
        print(f"{name}: largest |cost fp32 reversed - cost fp64| {dev:.2e}, flags equal {same}")
    assert set(devs) == set(df.sweep_cases())
    assert all(same for _, same in devs.values())
    bar = df.score_bar()
    print(f"SCORE_BAR = 8 x {bar / 8:.3e} = {bar:.3e}")
    assert 0.0 < bar <= 1e-3


@pytest.mark.parametrize("name", df.CASE_NAMES)
def test_sweep_margins(name):
    ref, rc, srcs, sc, K, depths, patch = df.sweep_cases()[name]
    A, b = dr.plane_warps(rc, sc, K)
    cm = dr.coord_margin(A, b, depths, *ref.shape)
    n = patch * patch
    _, _, vb = dr.cost_volume(ref, srcs, A, b, depths, patch, df.MIN_VAR, details=True)
    vm = float(np.nanmin(np.abs(vb - df.MIN_VAR * n))) if np.isfinite(vb).any() else np.inf
    print(f"{name}: coordinate margin {cm:.2e} px, warped-variance margin {vm:.3f}")
    assert cm > 1e-9
    assert vm > 2.0


def test_negation_is_exact():
    """Negating every camera and every depth leaves A, the coordinates and so every output
    unchanged bit for bit (the Dino cameras' negative depths)."""
    ref, rc, srcs, sc, K, depths, patch = df.sweep_cases()["slanted_p5"]
    pos = dr.plane_sweep(ref, rc, srcs, sc, K, depths, patch, df.MIN_VAR)
    neg = dr.plane_sweep(ref, -rc, srcs, -sc, K, -depths, patch, df.MIN_VAR)
    for a, b in zip(pos, neg):
        assert np.array_equal(a, b, equal_nan=True)


def test_consistency_margins_and_counts():
    depth, cams = df.consistency_case()
    count, half, tolm = dr.consistency(depth, cams, df.K, 0.01, details=True)
    print(f"consistency: counts {np.bincount(count.ravel())}, rounding margin "
          f"{half.min():.2e} px, tolerance margin {tolm.min():.2e}")
    assert half.min() > 1e-9
    assert tolm.min() > 1e-9
    assert np.all(count[np.isnan(depth)] == 0) and np.all(count[3] == 0)
    assert count.max() == 2 and (count == 2).sum() > 500
    # the view without depth adds nothing to the others
    assert np.array_equal(count[:3], dr.consistency(depth[:3], cams[:3], df.K, 0.01))
    # a map compared with itself through the same camera agrees everywhere it has depth
    twice = dr.consistency(np.array([depth[1], depth[1]]), cams[[1, 1]], df.K, 1e-12)
    assert np.array_equal(twice[0] == 1, np.isfinite(depth[1]))


def test_reference_fusion_lies_on_the_plane():
    imgs, cams, truth = df.scene("slanted")
    ridx, rdelta, rdepth, _ = df.reference_depth_maps("slanted")
    keep = dr.consistency(rdepth, cams, df.K, 0.01) >= 2
    off = np.abs(df.true_index(rdepth) - df.true_index(truth))
    print(f"reference fusion: {int(keep.sum())} kept, largest offset {off[keep].max():.3f} steps")
    assert keep.sum() > 1000
    assert np.all(off[keep] <= 1.0)
    n, c = df.SLANTED
    for i in range(3):
        pts = dr.depth_points(rdepth[i], cams[i], df.K)[keep[i]]
        assert np.abs(pts @ n - c).max() < 0.5
