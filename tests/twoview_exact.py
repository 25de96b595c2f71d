"""oracle/twoview_ref.triangulate_optimal restated step by step in mpmath (test helper).

The numpy oracle evaluates lab3.triangulate_optimal (lab3.py:382-475) in float64: three SVD
null vectors, the dehomogenised epipoles, np.roots of the degree-6 polynomial and one more SVD.
For forward motion, nearly rectified cameras or a tiny baseline those steps lose many digits, so
the oracle is no truth there.  ``triangulate_optimal`` below is the same sequence of steps at
50 digits (mp.svd_r for the null vectors, mp.polyroots for the sextic, the same argmin over the
real parts of the roots plus t = inf): the exact value of the reference's formulas for float64
inputs, against which both the oracle and the GPU are measured
(tests/golden/make_golden_twoview_edges.py, tests/test_twoview_edges_cpu.py).

It also returns the relative gap between the smallest cost s and the runner-up's, (s2 - s1) / s2,
over the candidates that are a different t (see TIE_T below): where that gap is at rounding level
the argmin, and with it X, is not a property of the input.

Imported only where mpmath is present.
"""
import mpmath as mp
import numpy as np

DPS = 50
TIE_T = 5e-8


def _mat(a):
    a = np.asarray(a, dtype=np.float64)
    return mp.matrix([[mp.mpf(float(v)) for v in row] for row in a])


def _cross_matrix(v):
    return mp.matrix([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]])


def _svd_last(M, left):
    """The singular vector of M's smallest singular value: U[:, -1] (left) or V[-1] (right),
    as a list.  A right vector of a wide matrix is the left vector of its transpose."""
    if not left:
        M = M.T
    U, S, _ = mp.svd_r(M, full_matrices=True)
    k = U.cols - 1
    if len(S) == U.cols:          # square or tall enough: the smallest singular value's column
        k = min(range(len(S)), key=lambda i: S[i])
    return [U[i, k] for i in range(U.rows)]


def _fmatrix_from_cameras(C1, C2):
    n = mp.matrix(_svd_last(C2, left=False))
    e = C1 * n
    pinv = C2.T * mp.inverse(C2 * C2.T)     # full row rank
    return _cross_matrix(e) * (C1 * pinv)


def _triangulate_linear(C1, C2, y1, y2):
    M = mp.matrix(6, 4)
    for s, (y, C) in enumerate(((y1, C1), (y2, C2))):
        B = _cross_matrix(y) * C
        for r in range(3):
            for c in range(4):
                M[3 * s + r, c] = B[r, c]
    X = _svd_last(M, left=False)
    return [X[0] / X[3], X[1] / X[3], X[2] / X[3]]


def _poly6(a, b, c, d):
    k1 = b * c - a * d
    return [a * c * k1,
            (a ** 2 + c ** 2) ** 2 + k1 * (b * c + a * d),
            4 * (a ** 2 + c ** 2) * (a * b + c * d) + 2 * a * c * k1 + b * d * k1,
            2 * (4 * a * b * c * d + a ** 2 * (3 * b ** 2) + c ** 2 * (3 * d ** 2 + b ** 2 * 2)),
            -a ** 2 * c * d + a * b * (4 * b ** 2 + c ** 2 + 4 * d ** 2 - 2 * d ** 2)
            + 2 * c * d * (2 * d ** 2 + b ** 2 * 3),
            b ** 4 - a ** 2 * d ** 2 + d ** 4 + b ** 2 * (c ** 2 + 2 * d ** 2),
            b * d * k1]


def triangulate_optimal(C1, C2, x1, x2, ties=False):
    """(X as float64 (3,), relative gap of the argmin's cost to the runner-up's) for float64
    inputs.  ties=True: also the list of X obtained from every other candidate that counts as
    the winner under TIE_T (what the argmin could have returned instead)."""
    with mp.workdps(DPS):
        C1, C2 = _mat(C1), _mat(C2)
        x1 = [mp.mpf(float(v)) for v in np.asarray(x1).ravel()[:2]]
        x2 = [mp.mpf(float(v)) for v in np.asarray(x2).ravel()[:2]]
        T1 = mp.matrix([[1, 0, x1[0]], [0, 1, x1[1]], [0, 0, 1]])
        T2 = mp.matrix([[1, 0, x2[0]], [0, 1, x2[1]], [0, 0, 1]])
        F = T1.T * (_fmatrix_from_cameras(C1, C2) * T2)
        u = _svd_last(F, left=True)
        v = _svd_last(F, left=False)
        e1 = [u[0] / u[2], u[1] / u[2]]
        e2 = [v[0] / v[2], v[1] / v[2]]
        n1 = mp.sqrt(e1[0] ** 2 + e1[1] ** 2)
        n2 = mp.sqrt(e2[0] ** 2 + e2[1] ** 2)
        e1 = [e1[0] / n1, e1[1] / n1]
        e2 = [e2[0] / n2, e2[1] / n2]
        R1 = mp.matrix([[e1[0], e1[1], 0], [-e1[1], e1[0], 0], [0, 0, 1]])
        R2 = mp.matrix([[e2[0], e2[1], 0], [-e2[1], e2[0], 0], [0, 0, 1]])
        F = R1 * (F * R2.T)
        a, b, c, d = F[1, 1], F[1, 2], F[2, 1], F[2, 2]
        g = _poly6(a, b, c, d)
        while g and g[0] == 0:        # np.roots strips leading zeros
            g = g[1:]
        roots = mp.polyroots(g, maxsteps=2000, extraprec=4 * mp.mp.prec) if len(g) > 1 else []
        r = [mp.re(z) for z in roots]
        s = [t ** 2 / (1 + t ** 2) + (c * t + d) ** 2 / ((a * t + b) ** 2 + (c * t + d) ** 2)
             for t in r]
        s.append(1 + c ** 2 / (a ** 2 + c ** 2))
        i = min(range(len(s)), key=lambda k: s[k])
        # the runner-up among the candidates that are another t: the reference takes the real
        # part of every root, so a complex pair is one candidate, and for nearly rectified
        # cameras, where the cost is symmetric about the real minimum up to ~1e-7, the complex
        # roots' real parts fall within ~2e-8 of that minimum and tie with it to 1e-17.  Such a
        # tie moves X by less than the 1e-6 bar (tests/test_twoview_edges_cpu.py evaluates X at
        # the tied candidates), so candidates within TIE_T (1 + |t|) of the winner count as
        # the winner.
        ti = r[i] if i < len(r) else None
        tied = [k for k in range(len(r)) if k != i and ti is not None
                and abs(r[k] - ti) <= TIE_T * (1 + abs(ti))]
        rest = [s[k] for k in range(len(s)) if k != i and k not in tied]
        s2 = min(rest) if rest else None
        gap = (s2 - s[i]) / s2 if s2 is not None and s2 > 0 else mp.mpf(1 if s2 is None else 0)

        def closest(l):
            return mp.matrix([-l[0] * l[2], -l[1] * l[2], l[0] ** 2 + l[1] ** 2])

        def X_of(k):
            if k < len(r):
                tm = r[k]
                l1 = [-(c * tm + d), a * tm + b, c * tm + d]
                l2 = [tm, mp.mpf(1), -tm]
            else:
                l1 = [-c, a, c]
                l2 = [mp.mpf(1), mp.mpf(0), mp.mpf(-1)]
            y1 = T1 * (R1.T * closest(l1))
            y2 = T2 * (R2.T * closest(l2))
            return np.array([float(v) for v in _triangulate_linear(C1, C2, y1, y2)])

        if ties:
            return X_of(i), float(gap), [X_of(k) for k in tied]
        return X_of(i), float(gap)


def rel_err(X, ref):
    """Largest relative error per point: max |X - ref| / max |ref| over the coordinates."""
    X, ref = np.asarray(X, np.float64), np.asarray(ref, np.float64)
    return np.abs(X - ref).max(axis=-1) / np.abs(ref).max(axis=-1)
