"""Generate tests/golden/pnp_minimal.npz: noisy samples for the minimal PnP solvers and what the
oracle restatements (oracle/pnp_ref.p3p_pose4, oracle/epnp_ref.epnp) give on them in 50-digit
arithmetic, with the restatements' own fp64 error per sample.

  p3p_front_*   200 four-point samples of positive-depth scenes, 0.8 px pixel noise
  p3p_dino_*    50 four-point samples of BAdino2 views (dino_pnp_kat.npz; negative-scale
                cameras, the true pose is the mirrored-depth one), 0.8 px pixel noise: under
                that much noise the front-facing twin is chosen in all 50 (mirror_wins says no)
  p3p_dino_fine_*  50 more with 0.01 px noise, where the mirrored pose wins
  epnp_X, epnp_y  40 noisy point sets of 257 points; epnp<m>_* takes the first m of each,
                m in {6, 7, 64, 65, 257}

  *_X (S, m, 3) world points, *_y (S, m, 3) C-normalised homogeneous image points, *_R, *_t the
  mpmath pose rounded to float64 (NaN where the restatement finds none), *_floor the distance
  max(max |dR|, max |dt| / max |t|) between the float64 run and the mpmath run (inf where
  either finds no pose).

Runs on the CPU (numpy, mpmath); written with fixed zip timestamps, so two runs give equal bytes.

Usage:  python tests/golden/make_golden_pnp_minimal.py
"""
from __future__ import annotations

import io
import os
import sys
import zipfile

import mpmath as mp
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from oracle import epnp_ref, pnp_ref  # noqa: E402

mp.mp.dps = 50
EPNP_M = (6, 7, 64, 65, 257)


# ---- the restatements' arithmetic in mpmath ----------------------------------------------
def _obj(a):
    """numpy array of mpf from a float array (or a nested list of mpf)."""
    a = np.asarray(a, dtype=object)
    out = np.empty(a.shape, dtype=object)
    for i in np.ndindex(a.shape):
        out[i] = mp.mpf(a[i])
    return out


def _mat(a):
    return mp.matrix(np.asarray(a, dtype=object).tolist())


def _arr(m):
    return _obj(np.array(m.tolist(), dtype=object).reshape(m.rows, m.cols))


def _zeros(shape):
    return _obj(np.zeros(shape))


class MpP3P:
    pi = mp.pi
    sqrt = staticmethod(mp.sqrt)
    arccos = staticmethod(mp.acos)
    cos = staticmethod(mp.cos)
    cbrt = staticmethod(mp.cbrt)
    zeros = staticmethod(_zeros)

    @staticmethod
    def copysign(x, s):
        return -abs(x) if s < 0 else abs(x)

    @staticmethod
    def eye(n):
        return _obj(np.eye(n))

    @staticmethod
    def det(A):
        return mp.det(_mat(A))

    @staticmethod
    def solve(A, b):
        return _arr(mp.lu_solve(_mat(A), _mat(b.reshape(-1, 1))))[:, 0]

    @staticmethod
    def inv(A):
        return _arr(mp.inverse(_mat(A)))


class MpEpnp:
    jacobi_tol = mp.mpf(10) ** -90
    sqrt = staticmethod(mp.sqrt)
    zeros = staticmethod(_zeros)

    @staticmethod
    def eigh(A):
        E, Q = mp.eigsy(_mat(A))
        order = sorted(range(len(E)), key=lambda i: E[i])
        Q = _arr(Q)
        return [E[i] for i in order], Q[:, order]

    @staticmethod
    def lstsq(A, b):
        try:
            x, _ = mp.qr_solve(_mat(A), _mat(b.reshape(-1, 1)))
        except (ValueError, ZeroDivisionError):
            return None
        return _arr(x)[:, 0]

    @staticmethod
    def polar(M):
        U, _, V = mp.svd_r(_mat(M))
        return _arr(U * V)


# ---- scenes ------------------------------------------------------------------------------
def _rodrigues(w):
    th = np.linalg.norm(w)
    k = w / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * (Kx @ Kx)


K_FRONT = np.array([[700.0, 0.0, 640.0], [0.0, 700.0, 480.0], [0.0, 0.0, 1.0]])


def _front_scene(rs, m, extent):
    """m correspondences of a positive-depth scene with 0.8 px noise: X, y = K^-1 (uv, 1)."""
    R = _rodrigues(rs.normal(0, 0.3, 3))
    t = np.array([rs.uniform(-0.5, 0.5), rs.uniform(-0.5, 0.5), rs.uniform(4, 8)])
    X = rs.uniform(-extent, extent, (m, 3))
    q = X @ R.T + t
    uv = (q[:, :2] / q[:, 2:]) * 700.0 + np.array([640.0, 480.0]) + rs.normal(0, 0.8, (m, 2))
    y = np.linalg.solve(K_FRONT, np.vstack([uv.T, np.ones((1, m))])).T
    return X, np.ascontiguousarray(y)


def _dino_sample(rs, z, sigma=0.8):
    v = int(rs.randint(0, len(z["K"])))
    vis = np.flatnonzero(z["points2d"][v, 0] != -1)
    s = rs.choice(vis, 4, replace=False)
    uv = z["points2d"][v][:, s].T + rs.normal(0, sigma, (4, 2))
    y = np.linalg.solve(z["K"][v], np.vstack([uv.T, np.ones((1, 4))])).T
    return np.ascontiguousarray(z["points3d"][s][:, :3]), np.ascontiguousarray(y)


# ---- float64 against mpmath --------------------------------------------------------------
def dist(R, t, Rr, tr):
    return max(np.abs(R - Rr).max(), np.abs(t - tr).max() / np.abs(tr).max())


def _both(solver, ops_mp, X, y):
    """(R_mp, t_mp, floor) of one sample."""
    lo = solver(X, y)
    hi = solver(_obj(X), _obj(y), ops_mp)
    nan = np.full((3, 3), np.nan), np.full(3, np.nan)
    if hi is None:
        return nan[0], nan[1], np.inf
    R = np.array(hi[0].tolist(), dtype=np.float64)
    t = np.array(hi[1].tolist(), dtype=np.float64)
    if lo is None:
        return R, t, np.inf
    return R, t, dist(lo[0], lo[1], R, t)


def _solve_all(solver, ops_mp, Xs, ys):
    out = [_both(solver, ops_mp, X, y) for X, y in zip(Xs, ys)]
    return (np.array([o[0] for o in out]), np.array([o[1] for o in out]),
            np.array([o[2] for o in out]))


def _write_npz(path, arrays):
    """np.savez with fixed zip timestamps (equal inputs, equal bytes)."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as zf:
        for name in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arrays[name]), allow_pickle=False)
            zf.writestr(zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0)),
                        buf.getvalue(), compress_type=zipfile.ZIP_DEFLATED)


def main():
    out = {}
    rs = np.random.RandomState(20)
    front = [_front_scene(rs, 4, 1.5) for _ in range(200)]
    z = np.load(os.path.join(HERE, "dino_pnp_kat.npz"), allow_pickle=False)
    dino = [_dino_sample(rs, z) for _ in range(50)]
    rs = np.random.RandomState(22)
    fine = [_dino_sample(rs, z, 0.01) for _ in range(50)]
    for key, samples in (("p3p_front", front), ("p3p_dino", dino), ("p3p_dino_fine", fine)):
        Xs, ys = np.array([s[0] for s in samples]), np.array([s[1] for s in samples])
        R, t, floor = _solve_all(pnp_ref.p3p_pose4, MpP3P, Xs, ys)
        out.update({f"{key}_X": Xs, f"{key}_y": ys, f"{key}_R": R, f"{key}_t": t,
                    f"{key}_floor": floor})
        _report(key, floor)
    rs = np.random.RandomState(21)
    sets = [_front_scene(rs, max(EPNP_M), 1.5) for _ in range(40)]
    Xs, ys = np.array([s[0] for s in sets]), np.array([s[1] for s in sets])
    out.update(epnp_X=Xs, epnp_y=ys)
    for m in EPNP_M:
        R, t, floor = _solve_all(epnp_ref.epnp, MpEpnp, Xs[:, :m], ys[:, :m])
        out.update({f"epnp{m}_R": R, f"epnp{m}_t": t, f"epnp{m}_floor": floor})
        _report(f"epnp{m}", floor)
    path = os.path.join(HERE, "pnp_minimal.npz")
    _write_npz(path, out)
    print(f"wrote {path} ({os.path.getsize(path) / 1024:.1f} KiB)")


def _report(key, floor):
    keep = floor <= 1e-9
    print(f"{key}: {len(floor)} samples, {int((~keep).sum())} left out "
          f"({100.0 * (1 - keep.mean()):.1f} %), largest remaining floor {floor[keep].max():.3g}, "
          f"median {np.median(floor[keep]):.3g}")


if __name__ == "__main__":
    main()
