"""The oracle's EPnP restatement (oracle/epnp_ref.py) on the CPU: the exact pose from noise-free
correspondences, front-facing and mirrored, and the float64 run against the 50-digit results
recorded in tests/golden/pnp_minimal.npz (make_golden_pnp_minimal.py), which set the bars of
tests/test_gpu_pnp_edges.py."""
import numpy as np
import pytest

from conftest import golden
from oracle import epnp_ref

EPS = np.finfo(np.float64).eps


def _rot(w):
    th = np.linalg.norm(w)
    k = w / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K


def dist(R, t, Rr, tr):
    return max(np.abs(R - Rr).max(), np.abs(t - tr).max() / np.abs(tr).max())


@pytest.mark.parametrize("m", [5, 6, 7, 30, 257])
def test_epnp_recovers_the_pose(m):
    rs = np.random.RandomState(m)
    for trial in range(10):
        R = _rot(rs.normal(0, 0.5, 3))
        t = np.array([rs.uniform(-1, 1), rs.uniform(-1, 1), rs.uniform(4, 9)])
        X = rs.uniform(-1.5, 1.5, (m, 3))
        q = X @ R.T + t
        y = np.column_stack([q[:, :2] / q[:, 2:], np.ones(m)])
        Re, te, err = epnp_ref.epnp(X, y)
        assert dist(Re, te, R, t) < 1e-9 and err < 1e-10, (m, trial)
        assert abs(np.linalg.det(Re) - 1.0) < 1e-12
        assert ((X @ Re.T + te)[:, 2] > 0).all()
        # the scene behind the camera (a camera matrix with a negative scale, as BAdino2's):
        # only the mirrored candidate fits, and it is far below 1e-2 of the front-facing error
        tb = t * np.array([1.0, 1.0, -1.0])
        q = X @ R.T + tb
        assert (q[:, 2] < 0).all()
        y = np.column_stack([q[:, :2] / q[:, 2:], np.ones(m)])
        Re, te, err = epnp_ref.epnp(X, y)
        assert dist(Re, te, R, tb) < 1e-9 and err < 1e-10, (m, trial)


def test_principal_axes_are_an_eigenbasis():
    rs = np.random.RandomState(1)
    for _ in range(20):
        d = rs.normal(0, 1, (9, 3)) * rs.uniform(0.1, 3, 3)
        C = d.T @ d
        V, lam = epnp_ref.principal_axes(C)
        np.testing.assert_allclose(V.T @ V, np.eye(3), atol=1e-14)
        assert np.linalg.det(V) > 0
        np.testing.assert_allclose(C @ V, V * np.array(lam), atol=1e-12 * max(lam))


@pytest.mark.parametrize("m", [6, 7, 64, 65, 257])
def test_epnp_float64_run_reproduces_the_golden_floors(m):
    """The float64 restatement against the recorded 50-digit poses: no sample is left out above
    the 5 % cap, and the float64 run stays within the bar its recorded floor sets (on the
    generator's BLAS it is the floor itself)."""
    z = golden("pnp_minimal.npz")
    X, y = z["epnp_X"][:, :m], z["epnp_y"][:, :m]
    Rg, tg, floor = z[f"epnp{m}_R"], z[f"epnp{m}_t"], z[f"epnp{m}_floor"]
    keep = floor <= 1e-9
    assert 1.0 - keep.mean() <= 0.05
    bar = max(4.0 * floor[keep].max(), 16.0 * EPS)
    for i in np.flatnonzero(keep):
        R, t, _ = epnp_ref.epnp(X[i], y[i])
        assert dist(R, t, Rg[i], tg[i]) <= bar, (m, i)
