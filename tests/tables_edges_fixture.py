"""Inputs, np.longdouble restatements and bars for tests/test_tables_edges_cpu.py and
tests/test_gpu_tables_edges.py: the five per-view kernels of tables.hip (k_match_obs,
k_e_from_cameras, k_new_points, k_ba_residuals, k_ba_jacobian) at tile and block edges, at ties
and on either side of the epipolar gate.  Test infrastructure.

Every expectation is computed here, in np.longdouble (64-bit mantissa, eps 1.08e-19), from the
formulas of oracle/tables_ref.py; the CPU file pins each restatement to the oracle's own function
and proves the margin conditions under which a float64 kernel must agree with it exactly.

Bars (eps = 2^-52), each derived from the roundings of the expression, none from a measurement:

  * E            32 eps mag, mag the expression of getEFromCameras on absolute values: a dot
                 product of three terms is 3 roundings, R, t and E are three of them in a chain and
                 t adds 2, so at most about 12 roundings lie on a path; doubled for contraction
  * residual     8 eps (|u| + A / |w| + |a| W / w^2), A = sum |c0k xk|, W likewise for row 2:
                 4 roundings in a and in w, one in the quotient, one in the difference
  * Jacobian     with kappa = W / |w| the conditioning of w:
                 Jc[0:4], Jc[16:20]   8 eps kappa |x / w|
                 Jc[8:12], Jc[20:24]  16 eps kappa |x| A / w^2 (B for the second)
                 Jp                   16 eps kappa (|c0k| W + A |c2k|) / w^2 (row 1: c1k, B)
"""
from __future__ import annotations

import numpy as np

LD = np.longdouble
LD_EPS = float(np.finfo(LD).eps)
LD_OK = LD_EPS < 1e-18
LD_REASON = f"np.longdouble has eps {LD_EPS:.3g} here: no better than float64, no reference"
EPS = 2.0 ** -52


def _ld(a):
    return np.asarray(a, dtype=LD)


def rotation(rng):
    Q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
    return Q * np.sign(np.linalg.det(Q))


def rigid(rng, centre_scale=1.0):
    """[R | t] with a random rotation and t ~ centre_scale N(0, 1)."""
    return np.hstack([rotation(rng), centre_scale * rng.standard_normal((3, 1))])


# ------------------------------------------------------------------------------------------
# 1. match_observations
# ------------------------------------------------------------------------------------------
# 514 and 1026 on top of the tile edges: in 513 and 1025 the last row, alone in its tile, is a
# duplicate of an earlier one and never the match itself; here row m - 1 is the last row of a
# partial second / third tile and matches in its own right
MATCH_M = (0, 1, 511, 512, 513, 514, 1024, 1025, 1026)
MATCH_N = (0, 1, 255, 256, 257, 513)
MATCH_TOL = 1e-4
MATCH_RATIOS = (0.0, 0.5, 0.99, 1.01, 2.0)
MATCH_ROWS = (0, 255, 256, 511, 512, 513, 1023, 1024)   # and m - 1
MATCH_MARGIN = 1e-9
TILE = 512


def match_rows(m):
    """The rows every launch aims at, wherever they exist, ordered so that consecutive queries
    (neighbouring lanes of one wave) aim at different tiles."""
    rows = sorted({r for r in MATCH_ROWS + (m - 1,) if 0 <= r < m})
    tiles = [[r for r in rows if r // TILE == t] for t in range(3)]
    out = []
    while any(tiles):
        for t in tiles:
            if t:
                out.append(t.pop(0))
    return out


def match_case(m, n):
    """dict(obs (m, 3), obs_point (m,) int64, q (n, 3), row (n,), ratio (n,), tol).

    obs rows are (randn, randn, 1) with obs[512] = obs[511] and obs[1024] = obs[0] (duplicates
    across tiles: the `found < 0` gate) and obs[300] = obs[255] (within a tile: the break) where
    those rows exist; obs_point[k] = 2^40 + 3k.  Query i with i % 4 != 3 is obs[row] + ratio tol u,
    u a random unit vector: the j-th such query aims at match_rows(m)[j % R] with
    MATCH_RATIOS[(j // R) % 5], so n >= 60 holds every row at every ratio (n = 1 aims at row 0
    at ratio 0).  Query i with i % 4 == 3 is (randn, randn, 1) and matches nothing (row -1).
    With m = 0 every query is of that kind."""
    rng = np.random.RandomState(7919 * m + n)
    obs = np.column_stack([rng.standard_normal(m), rng.standard_normal(m), np.ones(m)])
    if m > 300:
        obs[300] = obs[255]
    if m > 512:
        obs[512] = obs[511]
    if m > 1024:
        obs[1024] = obs[0]
    obs_point = 2 ** 40 + 3 * np.arange(m, dtype=np.int64)
    rows = match_rows(m)
    q = np.column_stack([rng.standard_normal(n), rng.standard_normal(n), np.ones(n)])
    row = np.full(n, -1)
    ratio = np.full(n, np.nan)
    u = rng.standard_normal((n, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    j = 0
    for i in range(n):
        if i % 4 == 3 or not rows:
            continue
        row[i] = rows[j % len(rows)]
        ratio[i] = MATCH_RATIOS[(j // len(rows)) % len(MATCH_RATIOS)]
        q[i] = obs[row[i]] + (ratio[i] * MATCH_TOL) * u[i]
        j += 1
    return dict(obs=obs, obs_point=obs_point, q=q, row=row, ratio=ratio, tol=MATCH_TOL)


def match_distances(obs, q):
    """(n, m) longdouble ||obs[k] - q[i]||."""
    d = _ld(obs)[None, :, :] - _ld(q)[:, None, :]
    return np.sqrt((d * d).sum(axis=2))


def match_ref(obs, obs_point, q, tol):
    """Per query the point of the first observation whose distance is < tol, else -1."""
    out = np.full(len(q), -1, dtype=np.int64)
    if len(obs) == 0 or len(q) == 0:
        return out
    with np.errstate(invalid="ignore"):
        hit = match_distances(obs, q) < LD(tol)
    some = hit.any(axis=1)
    out[some] = np.asarray(obs_point, dtype=np.int64)[hit.argmax(axis=1)[some]]
    return out


def match_margin(obs, q, tol):
    """min over the finite pairs of | ||obs - q|| - tol | / tol (inf without a pair, and for
    tol = inf, which no finite distance comes near)."""
    if len(obs) == 0 or len(q) == 0 or np.isinf(tol):
        return np.inf
    d = match_distances(obs, q)
    d = d[np.isfinite(d)]
    return float((np.abs(d - LD(tol)) / LD(tol)).min()) if d.size else np.inf


def strict_cases():
    """name -> dict(obs, obs_point, q, tol, expect, exact).  ``expect`` is written down from the
    definition, not computed; ``exact`` marks the cases decided in exact arithmetic (every
    operand and result a power of two, zero or a difference of equal numbers), the only ones to
    which the margin condition does not apply."""
    t = 2.0 ** -13
    rng = np.random.RandomState(5)
    obs = np.column_stack([rng.standard_normal((6, 2)), np.ones(6)])
    pid = 2 ** 40 + 3 * np.arange(6, dtype=np.int64)
    fin = np.column_stack([rng.standard_normal((9, 2)), np.ones(9)])
    nan0 = obs.copy()
    nan0[0] = np.nan
    qnan = np.vstack([fin[:3], [[np.nan, 0.0, 1.0]], obs[:1], [[0.0, np.nan, np.nan]]])
    one, p1 = np.array([[0.0, 0.0, 1.0]]), pid[:1]
    at = np.array([[t, 0.0, 1.0]])
    return {
        "distance equal to tol": dict(obs=one, obs_point=p1, q=at, tol=t, expect=[-1],
                                      exact=True),
        "tol one ulp above": dict(obs=one, obs_point=p1, q=at, tol=t * (1.0 + EPS),
                                  expect=[pid[0]], exact=True),
        "tol 0, exact duplicate": dict(obs=obs, obs_point=pid, q=obs[[2, 0]], tol=0.0,
                                       expect=[-1, -1], exact=True),
        "tol inf": dict(obs=obs, obs_point=pid, q=fin, tol=np.inf, expect=[pid[0]] * 9,
                        exact=False),
        "tol inf, obs[0] NaN": dict(obs=nan0, obs_point=pid, q=fin, tol=np.inf,
                                    expect=[pid[1]] * 9, exact=False),
        "NaN query, tol inf": dict(obs=obs, obs_point=pid, q=qnan, tol=np.inf,
                                   expect=[pid[0]] * 3 + [-1, pid[0], -1], exact=False),
        "NaN query": dict(obs=obs, obs_point=pid, q=qnan, tol=MATCH_TOL,
                          expect=[-1, -1, -1, -1, pid[0], -1], exact=False),
    }


# ------------------------------------------------------------------------------------------
# 2. getEFromCameras
# ------------------------------------------------------------------------------------------
E_N = (1, 127, 128, 129, 257)
E_FACTOR = 32.0
E_TRUTH_FACTOR = 64.0


def e_cameras(n):
    """(C1, C2, is_rigid): (n, 3, 4) pairs; the even ones rigid, the odd ones general 3 x 4."""
    rng = np.random.RandomState(4000 + n)
    C1, C2 = rng.standard_normal((n, 3, 4)), rng.standard_normal((n, 3, 4))
    is_rigid = np.arange(n) % 2 == 0
    for i in np.flatnonzero(is_rigid):
        C1[i], C2[i] = rigid(rng), rigid(rng)
    return C1, C2, is_rigid


def e_ref(C1, C2):
    """(E, mag), both (n, 3, 3) longdouble: R = R2 R1^T, t = t2 - R t1, E = R^T [t]_x, and the
    same expression on absolute values."""
    def run(C1, C2, sign):
        R1, t1, R2, t2 = C1[:, :, :3], C1[:, :, 3], C2[:, :, :3], C2[:, :, 3]
        R = np.einsum("nij,nkj->nik", R2, R1)
        t = t2 + sign * np.einsum("nij,nj->ni", R, t1)
        tx = np.zeros(R.shape, dtype=LD)
        tx[:, 0, 1], tx[:, 0, 2] = sign * t[:, 2], t[:, 1]
        tx[:, 1, 0], tx[:, 1, 2] = t[:, 2], sign * t[:, 0]
        tx[:, 2, 0], tx[:, 2, 1] = sign * t[:, 1], t[:, 0]
        return np.einsum("nji,njk->nik", R, tx)
    C1, C2 = _ld(C1).reshape(-1, 3, 4), _ld(C2).reshape(-1, 3, 4)
    return run(C1, C2, LD(-1)), run(np.abs(C1), np.abs(C2), LD(1))


def e_truth_points(C1, C2, k=10, seed=0):
    """(y1, y2), both (n, k, 3) longdouble: k random 3D points seen by each pair, homogeneous
    and not normalised.  For a rigid pair y1^T E y2 = 0 in exact arithmetic."""
    rng = np.random.RandomState(seed)
    Xh = np.concatenate([rng.standard_normal((len(C1), k, 3)), np.ones((len(C1), k, 1))], axis=2)
    return (np.einsum("nij,nkj->nki", _ld(C1), _ld(Xh)),
            np.einsum("nij,nkj->nki", _ld(C2), _ld(Xh)))


# ------------------------------------------------------------------------------------------
# 3. add_new_points
# ------------------------------------------------------------------------------------------
NEW_N = (0, 1, 127, 128, 129, 300)
NEW_GATES = (0.1, 1e-3)
# the issue's nine, then +-0.2: the only planted residuals whose row scaled by 2 (e times 4) is
# still accepted
NEW_S = (0.0, 0.5, -0.5, 0.999, -0.999, 1.001, -1.001, 2.0, -2.0, 0.2, -0.2)
NEW_MARGIN = 1e-9
NEW_NAN_ROW = 5
NEW_DIRECTION = np.array([0.6, 0.8, 0.0])


def new_points_case(n, gate):
    """dict(C1, C2, y1, y2 (n, 3), s (n,), scaled_from (n,), gate).

    Row k of a true correspondence (a, b) of rigid C1, C2 has b moved along NEW_DIRECTION by
    lambda = (s gate - a^T E b) / (a^T E d), s = NEW_S[k % 11], so that a^T E b = s gate: every s
    is present from n = 11 on and accepted and rejected rows alternate within every wave.  Rows
    k % 16 == 13 are instead 2 x row k - 11 (the same s; third component 2, e four times as
    large; the triangulation, which reads components 0 and 1, sees the image points doubled);
    scaled_from names that row, -1 elsewhere.  Row NEW_NAN_ROW has NaN in y1."""
    rng = np.random.RandomState(6000 + n)
    C1 = rigid(rng, 0.1)
    # the second camera a unit to the side of the first and turned by about 0.2 rad (Rodrigues)
    w = 0.2 * rng.standard_normal(3)
    th = np.linalg.norm(w)
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    dR = np.eye(3) + np.sin(th) / th * K + (1 - np.cos(th)) / th ** 2 * K @ K
    C2 = np.hstack([dR @ C1[:, :3], (dR @ C1[:, 3] + [1.0, 0.2, 0.1])[:, None]])
    # points 4 .. 8 in front of camera 1
    Xc = np.column_stack([rng.uniform(-1, 1, n), rng.uniform(-1, 1, n), rng.uniform(4, 8, n)])
    X = (Xc - C1[:, 3]) @ C1[:, :3]                     # R1^T (Xc - t1)
    Xh = np.column_stack([X, np.ones(n)])
    E, _ = e_ref(C1[None], C2[None])
    E = E[0]
    a = _ld(Xh) @ _ld(C1).T
    b = _ld(Xh) @ _ld(C2).T
    a, b = a / a[:, 2:3], b / b[:, 2:3]
    a = _ld(a.astype(np.float64))                       # y1 is a float64 input as it stands
    s = np.array([NEW_S[k % len(NEW_S)] for k in range(n)])
    d = _ld(NEW_DIRECTION)
    lam = (_ld(s) * LD(gate) - np.einsum("ni,ij,nj->n", a, E, b)) / np.einsum("ni,ij,j->n", a, E, d)
    y1 = a.astype(np.float64)
    y2 = (b + lam[:, None] * d).astype(np.float64)
    y2[:, 2] = 1.0
    scaled_from = np.full(n, -1)
    for k in range(13, n, 16):
        scaled_from[k] = k - len(NEW_S)
        y1[k], y2[k] = 2.0 * y1[k - len(NEW_S)], 2.0 * y2[k - len(NEW_S)]
    if n > NEW_NAN_ROW:
        y1[NEW_NAN_ROW, 0] = np.nan
    return dict(C1=C1, C2=C2, y1=y1, y2=y2, s=s, scaled_from=scaled_from, gate=gate)


def new_points_ref(y1, y2, C1, C2, gate):
    """(mask (n,) bool, e (n,) longdouble): e = y1^T E y2, mask = |e| < gate (NaN: False)."""
    E, _ = e_ref(np.asarray(C1)[None], np.asarray(C2)[None])
    e = np.einsum("ni,ij,nj->n", _ld(y1).reshape(-1, 3), E[0], _ld(y2).reshape(-1, 3))
    with np.errstate(invalid="ignore"):
        return np.abs(e) < LD(gate), e


def reprojection_error(C1, C2, y1, y2, X):
    """(n,) longdouble: the summed squared distance of X's two projections from components 0 and
    1 of y1 and y2 as they stand -- the image points the triangulation reads, whatever the third
    component says."""
    Xh = np.column_stack([_ld(X), np.ones(len(X), dtype=LD)])
    out = np.zeros(len(X), dtype=LD)
    for C, y in ((C1, y1), (C2, y2)):
        p = Xh @ _ld(C).T
        out += (((p[:, :2] / p[:, 2:3]) - _ld(y)[:, :2]) ** 2).sum(axis=1)
    return out


# ------------------------------------------------------------------------------------------
# 4. ba_residuals / ba_jacobian
# ------------------------------------------------------------------------------------------
BA_N = (1, 255, 256, 257, 513)
BA_LAYOUTS = ("nC1", "nC3", "nP1", "nP2n")
BA_KAPPA = (1e2, 1e4)
R_FACTOR = 8.0
J_FACTOR = 8.0      # doubled for the blocks with w^2


def ba_case(n, layout):
    """dict(cams (nC, 3, 4), pts (nP, 3), ov, op (n,) int32, uv (n, 2)).

    layout "nC1": one camera, max(1, n // 4) points; "nC3": three cameras, n // 3 + 1 points;
    "nP1": three cameras, every observation of one point; "nP2n": three cameras, 2n points,
    at least half of them without an observation.  Cameras are general 3 x 4 (randn).

    The pair (camera k, point j) has the kind (j + k) % 4: 0 and 3 plain (w in 0.5 .. 2),
    1 behind (w in -2 .. -0.5), 2 ill-conditioned (|w| = W / kappa with kappa log-uniform in
    3e2 .. 3e3 and either sign).  Point j is the solution of its cameras' three equations
    c2 . x + c23 = w (the minimum-norm shift of a random point for a single camera), which moves
    it along the rows' own directions until every w is the wanted one; W depends on the point, so
    the ill-conditioned targets are set three times over.  uv is the projection + 0.01 N(0, 1)."""
    rng = np.random.RandomState(8000 + 10 * n + BA_LAYOUTS.index(layout))
    nC = 1 if layout == "nC1" else 3
    nP = {"nC1": max(1, n // 4), "nC3": n // 3 + 1, "nP1": 1, "nP2n": 2 * n}[layout]
    cams = rng.standard_normal((nC, 3, 4))
    M, m3 = cams[:, 2, :3], cams[:, 2, 3]
    pts = rng.standard_normal((nP, 3))
    kind = (np.arange(nP)[:, None] + np.arange(nC)[None, :]) % 4
    sign = np.where(kind == 1, -1.0, np.where(kind == 2, rng.choice([-1.0, 1.0], (nP, nC)), 1.0))
    mag = rng.uniform(0.5, 2.0, (nP, nC))
    kappa = np.exp(rng.uniform(np.log(3e2), np.log(3e3), (nP, nC)))
    for _ in range(3):
        W = np.abs(pts) @ np.abs(M).T + np.abs(m3)                    # (nP, nC)
        target = sign * np.where(kind == 2, W / kappa, mag)
        if nC == 1:
            w = pts @ M.T + m3
            pts = pts + (target - w) * M[0] / (M[0] @ M[0])
        else:
            pts = np.linalg.solve(M, (target - m3).T).T
    ov = rng.randint(0, nC, n).astype(np.int32)
    op = rng.randint(0, nP, n).astype(np.int32)
    if layout == "nC3" and n >= nP:
        op[:nP] = np.arange(nP)                                       # every point referenced
    xh = np.column_stack([pts[op], np.ones(n)])
    y = np.einsum("nij,nj->ni", cams[ov], xh)
    uv = y[:, :2] / y[:, 2:3] + 0.01 * rng.standard_normal((n, 2))
    return dict(cams=cams, pts=pts, ov=ov, op=op, uv=uv)


def ba_ref(cams, pts, ov, op, uv):
    """The longdouble restatement of oracle.tables_ref.ba_residuals / ba_jacobian and the bars.

    Returns dict(r (2n,), Jc (n, 2, 12), Jp (n, 2, 3)) longdouble, dict(r, Jc, Jp) float64 bars
    of the same shapes (0 at the structural zeros of Jc), and dict(w, kappa) float64."""
    c = _ld(cams).reshape(-1, 3, 4)[ov]
    n = len(ov)
    xh = np.concatenate([_ld(pts).reshape(-1, 3)[op], np.ones((n, 1), dtype=LD)], axis=1)
    uv = _ld(uv).reshape(-1, 2)
    ab = np.einsum("nrk,nk->nr", c[:, :2], xh)                        # a, b
    w = np.einsum("nk,nk->n", c[:, 2], xh)
    AB = np.einsum("nrk,nk->nr", np.abs(c[:, :2]), np.abs(xh))        # A, B
    W = np.einsum("nk,nk->n", np.abs(c[:, 2]), np.abs(xh))
    kappa = W / np.abs(w)
    r = uv - ab / w[:, None]
    Jc = np.zeros((n, 2, 12), dtype=LD)
    Jp = np.zeros((n, 2, 3), dtype=LD)
    bJc = np.zeros((n, 2, 12), dtype=LD)
    for row in range(2):
        Jc[:, row, 4 * row:4 * row + 4] = -xh / w[:, None]
        Jc[:, row, 8:12] = xh * (ab[:, row] / w ** 2)[:, None]
        Jp[:, row] = -(c[:, row, :3] * w[:, None] - c[:, 2, :3] * ab[:, row, None]) \
            / (w ** 2)[:, None]
        bJc[:, row, 4 * row:4 * row + 4] = J_FACTOR * EPS * kappa[:, None] \
            * np.abs(xh / w[:, None])
        bJc[:, row, 8:12] = 2 * J_FACTOR * EPS * kappa[:, None] * np.abs(xh) \
            * (AB[:, row] / w ** 2)[:, None]
    bJp = 2 * J_FACTOR * EPS * kappa[:, None, None] \
        * (np.abs(c[:, :2, :3]) * W[:, None, None]
           + AB[:, :, None] * np.abs(c[:, 2, None, :3])) / (w ** 2)[:, None, None]
    br = R_FACTOR * EPS * (np.abs(uv) + AB / np.abs(w)[:, None]
                           + np.abs(ab) * (W / w ** 2)[:, None])
    f = lambda a: np.asarray(a, dtype=np.float64)
    return (dict(r=r.reshape(-1), Jc=Jc, Jp=Jp),
            dict(r=f(br).reshape(-1), Jc=f(bJc), Jp=f(bJp)),
            dict(w=f(w), kappa=f(kappa)))


def worst_ratio(got, ref, bar):
    """max |got - ref| / bar over the entries with a bar; entries without one (bar 0) must be
    handled by the caller.  0 for nothing to compare."""
    err = np.abs(_ld(got) - ref)
    k = bar > 0
    return float((err[k] / bar[k]).max()) if k.any() else 0.0


# ------------------------------------------------------------------------------------------
# 5. finite differences of the residuals
# ------------------------------------------------------------------------------------------
FD_N = 5


def fd_steps(case):
    """The 15 perturbations of ba_case(FD_N, "nC3"): (name, h, plus, minus), plus / minus being
    copies of the case with one of the 12 entries of camera ov[0] or of the 3 coordinates of point
    op[0] moved by +-h, h = 1e-6 max(1, |p|)."""
    out = []
    k, j = int(case["ov"][0]), int(case["op"][0])
    for what, idx, size in (("cams", k, 12), ("pts", j, 3)):
        for e in range(size):
            p = case[what][idx].reshape(-1)[e]
            h = 1e-6 * max(1.0, abs(p))
            moved = []
            for sgn in (1.0, -1.0):
                c = dict(case)
                c[what] = case[what].copy()
                c[what][idx].reshape(-1)[e] = p + sgn * h
                moved.append(c)
            out.append((f"{what}[{idx}][{e}]", h, moved[0], moved[1]))
    return out
