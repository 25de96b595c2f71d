"""ORACLE -- test infrastructure only, never shipped, never measured as the product.

CPU restatement of EPnP (Lepetit, Moreno-Noguer & Fua, "EPnP: An Accurate O(n) Solution to the
PnP Problem", IJCV 2009) as pnp_minimal.h epnp_pose documents it: four control points (the
centroid and the principal axes scaled by sqrt(eigenvalue / n)), barycentric coordinates (a zero
scale gives 0, as a pseudo-inverse does), the 2n x 12 system M through M^T M and its four
eigenvectors of smallest eigenvalue, the 6 x 10 matrix L and the control-point distances rho,
betas by the three linearisations (N = 1: all four vectors, N = 2, N = 3), five Gauss-Newton
steps each, the camera-frame control points with the sign that puts point 0 in front (or, for
the mirrored candidate, behind), absolute orientation (Procrustes, last row flipped on a
reflection), the mean reprojection error, and the front / mirror choice of pnp_ref.mirror_wins.

The reference project has no EPnP of its own (its p3p is cv2.solvePnP), so this is written from
the paper and the header comment, with numpy's eigh / lstsq / svd where the kernel has its own
Jacobi and Householder code.  One convention is the kernel's and is restated as such: the
principal axes are the columns the cyclic one-sided Jacobi of the 3 x 3 scatter matrix leaves
(pairs (0,1) (0,2) (1,2), V starting at the identity) -- EPnP on noisy data is not invariant
under flipping an axis, so the order and signs of the axes are part of the definition.

With n = 4 or 5 the system has an exact null space of dimension 4 or 2 and the result depends on
the basis the eigen-solver returns: no restatement can pin it, and this one is used for n >= 6.

``ops`` is the arithmetic (numpy float64 here); tests/golden/make_golden_pnp_minimal.py passes
the same operations in mpmath to measure this restatement's own rounding error.
"""
from __future__ import annotations

import numpy as np

from .pnp_ref import mirror_wins


class NumpyOps:
    jacobi_tol = 1e-30   # rotate while g^2 > tol a b (the kernel's)

    sqrt = staticmethod(np.sqrt)
    zeros = staticmethod(np.zeros)

    @staticmethod
    def eigh(A):
        """(eigenvalues ascending, eigenvectors in columns) of a symmetric matrix."""
        return np.linalg.eigh(A)

    @staticmethod
    def lstsq(A, b):
        """argmin |A x - b|, or None if A is rank deficient."""
        x, _, rank, _ = np.linalg.lstsq(A, b, rcond=None)
        return x if rank == A.shape[1] else None

    @staticmethod
    def polar(M):
        """U V^T of the SVD M = U S V^T."""
        U, _, Vt = np.linalg.svd(M)
        return U @ Vt


def principal_axes(C, ops=NumpyOps):
    """(V, lam): the columns of V are the principal axes of the symmetric 3 x 3 C in the order
    and with the signs of the cyclic one-sided Jacobi (device_math.h svd3_jacobi), lam the
    eigenvalues (the column norms of C V)."""
    B = C.copy()
    V = ops.zeros((3, 3))
    for i in range(3):
        V[i, i] = V[i, i] + 1.0
    for _ in range(60):
        rotated = False
        for p, q in ((0, 1), (0, 2), (1, 2)):
            a, b, g = B[:, p] @ B[:, p], B[:, q] @ B[:, q], B[:, p] @ B[:, q]
            if not g * g > ops.jacobi_tol * (a * b):
                continue
            rotated = True
            zeta = (b - a) / (2.0 * g)
            t = (1.0 if zeta >= 0.0 else -1.0) / (abs(zeta) + ops.sqrt(zeta * zeta + 1.0))
            c = 1.0 / ops.sqrt(t * t + 1.0)
            s = c * t
            for A in (B, V):
                ap, aq = A[:, p].copy(), A[:, q].copy()
                A[:, p] = c * ap - s * aq
                A[:, q] = s * ap + c * aq
        if not rotated:
            break
    lam = [ops.sqrt(B[:, j] @ B[:, j]) for j in range(3)]
    return V, lam


_PA = (0, 0, 0, 1, 1, 2)
_PB = (1, 2, 3, 2, 3, 3)


def epnp(X, y, ops=NumpyOps):
    """EPnP over n >= 4 correspondences X (n,3) <-> y (n,3) C-normalised homogeneous.  Returns
    (R, t, err) -- err the mean reprojection error in normalised coordinates -- or None."""
    n = len(X)
    u, v = y[:, 0] / y[:, 2], y[:, 1] / y[:, 2]
    c0 = X.sum(axis=0) / n
    d = X - c0
    V, lam = principal_axes(d.T @ d, ops)
    sc = [ops.sqrt(lam[j] / n) for j in range(3)]
    cw = [c0] + [c0 + sc[j] * V[:, j] for j in range(3)]
    alpha = ops.zeros((n, 4))
    for j in range(3):
        if sc[j] > 0.0:
            alpha[:, 1 + j] = (d @ V[:, j]) / sc[j]
    alpha[:, 0] = 1.0 - (alpha[:, 1] + alpha[:, 2] + alpha[:, 3])
    M = ops.zeros((2 * n, 12))
    for j in range(4):
        M[0::2, 3 * j] = alpha[:, j]
        M[0::2, 3 * j + 2] = -alpha[:, j] * u
        M[1::2, 3 * j + 1] = alpha[:, j]
        M[1::2, 3 * j + 2] = -alpha[:, j] * v
    _, E = ops.eigh(M.T @ M)
    vv = [E[:, i] for i in range(4)]          # ascending eigenvalues
    # L (6 x 10) and rho over the control-point pairs (0,1) (0,2) (0,3) (1,2) (1,3) (2,3); the
    # columns are b11 b12 b22 b13 b23 b33 b14 b24 b34 b44
    L, rho = ops.zeros((6, 10)), ops.zeros(6)
    for j in range(6):
        dv = [vv[i][3 * _PA[j]:3 * _PA[j] + 3] - vv[i][3 * _PB[j]:3 * _PB[j] + 3] for i in range(4)]
        L[j] = [dv[0] @ dv[0], 2.0 * (dv[0] @ dv[1]), dv[1] @ dv[1], 2.0 * (dv[0] @ dv[2]),
                2.0 * (dv[1] @ dv[2]), dv[2] @ dv[2], 2.0 * (dv[0] @ dv[3]),
                2.0 * (dv[1] @ dv[3]), 2.0 * (dv[2] @ dv[3]), dv[3] @ dv[3]]
        dc = cw[_PA[j]] - cw[_PB[j]]
        rho[j] = dc @ dc

    def gauss_newton(b):
        for _ in range(5):
            A, r = ops.zeros((6, 4)), ops.zeros(6)
            for j in range(6):
                l = L[j]
                A[j] = [2 * l[0] * b[0] + l[1] * b[1] + l[3] * b[2] + l[6] * b[3],
                        l[1] * b[0] + 2 * l[2] * b[1] + l[4] * b[2] + l[7] * b[3],
                        l[3] * b[0] + l[4] * b[1] + 2 * l[5] * b[2] + l[8] * b[3],
                        l[6] * b[0] + l[7] * b[1] + l[8] * b[2] + 2 * l[9] * b[3]]
                r[j] = rho[j] - (l[0] * b[0] * b[0] + l[1] * b[0] * b[1] + l[2] * b[1] * b[1]
                                 + l[3] * b[0] * b[2] + l[4] * b[1] * b[2] + l[5] * b[2] * b[2]
                                 + l[6] * b[0] * b[3] + l[7] * b[1] * b[3] + l[8] * b[2] * b[3]
                                 + l[9] * b[3] * b[3])
            dx = ops.lstsq(A, r)
            if dx is None:
                return b
            b = b + dx
        return b

    def pose_of(b, mirror):
        cc = (b[0] * vv[0] + b[1] * vv[1] + b[2] * vv[2] + b[3] * vv[3]).reshape(4, 3)
        z0 = alpha[0] @ cc[:, 2]
        if (z0 < 0.0) != mirror:
            cc = -cc
        pc = alpha @ cc
        pc0 = pc.sum(axis=0) / n
        R = ops.polar((pc - pc0).T @ d)
        det = (R[0, 0] * (R[1, 1] * R[2, 2] - R[1, 2] * R[2, 1])
               - R[0, 1] * (R[1, 0] * R[2, 2] - R[1, 2] * R[2, 0])
               + R[0, 2] * (R[1, 0] * R[2, 1] - R[1, 1] * R[2, 0]))
        if det < 0.0:
            R[2] = -R[2]
        t = pc0 - R @ c0
        q = X @ R.T + t
        du, dv_ = u - q[:, 0] / q[:, 2], v - q[:, 1] / q[:, 2]
        err = sum(ops.sqrt(du[i] * du[i] + dv_[i] * dv_[i]) for i in range(n)) / n
        return R, t, (err if err == err else float("inf"))

    inf = float("inf")
    best = [inf, inf]           # front-facing, mirrored
    arg = [None, None]
    for N in (1, 2, 3):
        b = ops.zeros(4)
        if N == 1:              # all four null vectors: b11 b12 b13 b14
            x = ops.lstsq(L[:, [0, 1, 3, 6]], rho)
            if x is None:
                continue
            s = -1.0 if x[0] < 0.0 else 1.0
            b[0] = ops.sqrt(s * x[0])
            if not b[0] > 0.0:
                continue
            b[1], b[2], b[3] = s * x[1] / b[0], s * x[2] / b[0], s * x[3] / b[0]
        else:                   # N = 2: b11 b12 b22; N = 3: b11 b12 b22 b13 b23
            x = ops.lstsq(L[:, :3] if N == 2 else L[:, :5], rho)
            if x is None:
                continue
            if x[0] < 0.0:
                b[0] = ops.sqrt(-x[0])
                b[1] = ops.sqrt(-x[2]) if x[2] < 0.0 else b[1]
            else:
                b[0] = ops.sqrt(x[0])
                b[1] = ops.sqrt(x[2]) if x[2] > 0.0 else b[1]
            if x[1] < 0.0:
                b[0] = -b[0]
            if N == 3:
                if not b[0] != 0.0:
                    continue
                b[2] = x[3] / b[0]
        b = gauss_newton(b)
        for mirror in (0, 1):
            R, t, e = pose_of(b, bool(mirror))
            if e < best[mirror]:
                best[mirror], arg[mirror] = e, (R, t)
    k = 1 if mirror_wins(best[1], best[0]) else 0
    if arg[k] is None:
        return None
    return arg[k][0], arg[k][1], best[k]
