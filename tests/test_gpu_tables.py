"""GPU parity of the per-view SfM steps (tables.hip) against the reference's own outputs
(tests/golden/tables.npz) and the pinned oracle (oracle/tables_ref.py).

Bars: matching -- the same D / A partition, exactly; epipolar gate -- the same mask; new
points -- 1e-6 relative (optimal triangulation); BA residuals -- 1e-12 (same expression; the
reference's np.dot may sum in another order); BA Jacobian -- equal to the oracle's analytic
blocks to 1e-12 and consistent with finite differences of the GPU residuals (against the same
differences of the longdouble restatement of tests/tables_edges_fixture.py; measured on the
MI355X: 0.012 of the derived bar).  Sizes at tile and block edges, ties and the gate:
tests/test_gpu_tables_edges.py."""
import numpy as np
import pytest

from conftest import golden
from oracle import tables_ref as tr
from tsbb15_amd import tables as gt

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("tag", ["clean", "noisy"])
def test_matching(ctx, tag):
    z = golden("tables.npz")
    g = lambda k: z[f"{tag}_{k}"]
    m = gt.match_observations(g("match_obs_coords"), g("match_obs_point"), g("match_queries"))
    np.testing.assert_array_equal(m, tr.match_observations(g("match_obs_coords"),
                                                           g("match_obs_point"),
                                                           g("match_queries")))
    found = m >= 0
    nC = int(g("ba_n_views"))
    pts = g("ba_x_final")[12 * nC:].reshape(-1, 3)
    np.testing.assert_array_equal(pts[m[found]], g("match_D3"))
    np.testing.assert_array_equal(g("match_y1")[~found], g("match_A_y1"))
    # larger than one LDS tile, with duplicates: the FIRST match wins
    rng = np.random.RandomState(0)
    obs = rng.randn(1500, 3)
    obs[1200] = obs[700]
    pid = np.arange(1500) * 3
    q = np.vstack([obs[[5, 700, 1499]], obs[[10]] + 1e-3, obs[[20]] + 1e-5])
    np.testing.assert_array_equal(gt.match_observations(obs, pid, q), [15, 2100, 4497, -1, 60])


@pytest.mark.parametrize("tag", ["clean", "noisy"])
def test_add_new_points(ctx, tag):
    z = golden("tables.npz")
    g = lambda k: z[f"{tag}_{k}"]
    C1, C2 = g("new_C1"), g("new_C2")
    np.testing.assert_allclose(gt.getEFromCameras(C1, C2), g("new_E"), rtol=0, atol=1e-14)
    mask, X = gt.add_new_points(g("new_y1_hom"), g("new_y2_hom"), C1, C2)
    np.testing.assert_array_equal(mask, g("new_gate"))
    ref = g("new_X")
    err = np.abs(X[mask] - ref).max(axis=1) / np.abs(ref).max(axis=1)
    assert err.max() < 1e-6, err.max()
    assert np.all(np.isnan(X[~mask]))


@pytest.mark.parametrize("tag", ["clean", "noisy"])
def test_ba_residuals_and_jacobian(ctx, tag):
    z = golden("tables.npz")
    g = lambda k: z[f"{tag}_{k}"]
    nC, nP = int(g("ba_n_views")), int(g("ba_n_points"))
    view, point, y = g("ba_obs_view"), g("ba_obs_point"), g("ba_obs_coords")
    for x, r in ((g("ba_x0"), g("ba_r0")), (g("ba_x1"), g("ba_r1"))):
        cams, pts = x[:12 * nC].reshape(nC, 3, 4), x[12 * nC:].reshape(nP, 3)
        np.testing.assert_allclose(gt.ba_residuals(cams, pts, view, point, y[:, :2]), r,
                                   rtol=1e-12, atol=1e-15)
    Jc, Jp = gt.ba_jacobian(cams, pts, view, point)
    Jc0, Jp0 = tr.ba_jacobian(cams, pts, view, point)
    np.testing.assert_allclose(Jc, Jc0, rtol=1e-12, atol=1e-15)
    np.testing.assert_allclose(Jp, Jp0, rtol=1e-12, atol=1e-15)
    with pytest.raises(ValueError):
        gt.ba_residuals(cams, pts, view, point + nP, y[:, :2])


def test_ba_finite_differences_of_the_gpu_residuals(ctx):
    """Central differences of gt.ba_residuals in the 12 entries of one camera and the 3
    coordinates of one point against the same differences of the longdouble restatement, at the
    same float64 arguments: only the rounding of the two residuals separates them, so the bar is
    (bar_r(+h) + bar_r(-h)) / (2 h) with the residual's derived bar.  Whether such differences
    agree with the analytic blocks is tests/test_oracle_tables.py's affair."""
    import tables_edges_fixture as fx
    if not fx.LD_OK:
        pytest.skip(fx.LD_REASON)
    case = fx.ba_case(fx.FD_N, "nC3")
    worst = 0.0
    for name, h, plus, minus in fx.fd_steps(case):
        fd, ref_fd, bar = 0, 0, 0
        for sgn, c in ((1, plus), (-1, minus)):
            args = (c["cams"], c["pts"], c["ov"], c["op"], c["uv"])
            ref, b, _ = fx.ba_ref(*args)
            fd = fd + sgn * np.asarray(gt.ba_residuals(*args, ctx=ctx), dtype=fx.LD)
            ref_fd = ref_fd + sgn * ref["r"]
            bar = bar + b["r"]
        touched = ref_fd != 0
        assert touched.any(), name
        ratio = float((np.abs(fd - ref_fd) / bar).max())      # both over 2 h
        assert np.all(fd[~touched] == 0), name
        worst = max(worst, ratio)
        assert ratio <= 1.0, (name, ratio)
    print(f"finite differences: worst error / bar {worst:.3f}")
