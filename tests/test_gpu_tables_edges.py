"""The per-view kernels of tables.hip (k_match_obs, k_e_from_cameras, k_new_points,
k_ba_residuals, k_ba_jacobian) against the np.longdouble restatements of
tests/tables_edges_fixture.py, at tile and block edges, at ties and on either side of the gate.
tests/test_tables_edges_cpu.py pins those restatements to oracle/tables_ref.py and proves the
margins that let this file demand equal integers and masks.

Bars are derived in the fixture's docstring; the figures below are what the MI355X gave against
them (worst error / bar), none of them the source of a bar.

Measured on the MI355X.  Matching (9 x 6 sizes, 7 strictness cases) and every gate mask: equal.
E, n = 1 .. 257: at most 0.027 of the bar against the restatement, 0.022 of the bar on true
correspondences.  New points: rows with |s| <= 0.5 within 1.1e-14 of the oracle (bar 1e-6);
rows at |s| = 0.999 and scaled rows: reprojection error at most 1 + 5.6e-15 of the oracle's (bar
1 + 1e-6).  BA, 20 cases with kappa up to 3.0e3: residuals at most 0.060 of the bar, Jc 0.139,
Jp 0.126; the zero quarters of Jc are zeros.  No kernel needed a change.

One claim about the scaled rows could not be tested as first worded ("X of a row scaled by 2
equals X of the unscaled row bit for bit"): the triangulation reads components 0 and 1, which the
scaling doubles, so it sees other image points -- in the oracle too.  What does follow from
"reads components 0 and 1 only" is tested instead: rows that differ in their third components
alone give X bit for bit (test_triangulation_ignores_the_third_component), and an accepted scaled
row is held to the oracle's reprojection error for the row as it stands.

Value mutations of k_match_obs, each run once against the matching tests on a scratch build:
`< tol` -> `<= tol` fails "distance equal to tol" and "tol 0, exact duplicate"; `found = base + k`
-> `found = k` fails every size with m >= 1024 and n >= 255 (since then m = 514 and 1026 were
added, which a numpy model of the walk shows failing too); without the `break` the three tol = inf
cases fail (since then obs[300] = obs[255] was added: the model fails every m >= 511, n >= 255).
"""
import numpy as np
import pytest

import tables_edges_fixture as fx
from oracle import twoview_ref as tv
from tables_fixture import Pose
from tsbb15_amd import _ffi, cloud, evaluation, twoview
from tsbb15_amd import tables as gt

pytestmark = pytest.mark.gpu

if not fx.LD_OK:
    pytest.skip(fx.LD_REASON, allow_module_level=True)

LD = fx.LD
_d = _ffi.C.c_double


def _e_batch(ctx, C1, C2):
    """rs_e_from_cameras on n pairs (the wrapper passes 1)."""
    C1, C2 = _ffi.f64c(C1).reshape(-1, 3, 4), _ffi.f64c(C2).reshape(-1, 3, 4)
    E = np.full((len(C1), 3, 3), np.nan)
    _ffi.check(_ffi.lib().rs_e_from_cameras(ctx.handle, _ffi.ptr(C1, _d), _ffi.ptr(C2, _d),
                                            len(C1), _ffi.ptr(E, _d)))
    return E


def _dirty(ctx):
    """Leave the context's scratch arena full of non-zero doubles (about 1 MiB of them)."""
    rng = np.random.RandomState(1)
    E = _e_batch(ctx, rng.standard_normal((4096, 3, 4)) + 3.0, rng.standard_normal((4096, 3, 4)))
    assert np.all(np.isfinite(E))


# ------------------------------------------------------------------------------------------
# 1. match_observations
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", fx.MATCH_N)
@pytest.mark.parametrize("m", fx.MATCH_M)
def test_match_at_tile_and_block_edges(ctx, m, n):
    c = fx.match_case(m, n)
    ref = fx.match_ref(c["obs"], c["obs_point"], c["q"], c["tol"])
    out = gt.match_observations(c["obs"], c["obs_point"], c["q"], c["tol"], ctx=ctx)
    assert out.dtype == np.int64 and out.shape == (n,)
    np.testing.assert_array_equal(out, ref)
    if m == 0:
        assert np.all(out == -1)
    # the first match wins across tiles: obs[512] = obs[511], obs[1024] = obs[0]
    inside = c["ratio"] < 1.0
    for dup, first in ((512, 511), (1024, 0)):
        if m > first:
            k = inside & ((c["row"] == dup) | (c["row"] == first))
            assert np.all(out[k] == c["obs_point"][first])
    # every edge row that exists was found at least once, with its 64-bit point
    if n >= 255:
        for row in fx.match_rows(m):
            first = {512: 511, 1024: 0}.get(row, row)
            assert (out[inside & (c["row"] == row)] == 2 ** 40 + 3 * first).sum() >= 3, row


@pytest.mark.parametrize("name", list(fx.strict_cases()))
def test_match_strictness(ctx, name):
    c = fx.strict_cases()[name]
    out = gt.match_observations(c["obs"], c["obs_point"], c["q"], c["tol"], ctx=ctx)
    np.testing.assert_array_equal(out, c["expect"])


# ------------------------------------------------------------------------------------------
# 2. rs_e_from_cameras, batched
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", fx.E_N)
def test_e_from_cameras_batched(ctx, n):
    C1, C2, is_rigid = fx.e_cameras(n)
    ref, mag = fx.e_ref(C1, C2)
    E = _e_batch(ctx, C1, C2)
    assert np.all(np.isfinite(E))
    ratio = float((np.abs(fx._ld(E) - ref) / (fx.E_FACTOR * fx.EPS * mag)).max())
    # ground truth without the restatement: true correspondences of the rigid pairs
    y1, y2 = fx.e_truth_points(C1, C2)
    e = np.einsum("nki,nij,nkj->nk", y1, fx._ld(E), y2)
    scale = np.einsum("nki,nij,nkj->nk", np.abs(y1), mag, np.abs(y2))
    truth = float((np.abs(e) / (fx.E_TRUTH_FACTOR * fx.EPS * scale))[is_rigid].max())
    print(f"E n = {n}: {ratio:.3f} of the bar against the restatement, {truth:.3f} of the bar "
          f"on true correspondences")
    assert ratio <= 1.0 and truth <= 1.0
    # the wrapper, with matrices and with pose objects, is entry i of the batch bit for bit
    for i in sorted({0, n - 1}):
        assert gt.getEFromCameras(C1[i], C2[i], ctx=ctx).tobytes() == E[i].tobytes()
        poses = [Pose(C[i, :, :3].copy(), C[i, :, 3].copy()) for C in (C1, C2)]
        assert gt.getEFromCameras(*poses, ctx=ctx).tobytes() == E[i].tobytes()


# ------------------------------------------------------------------------------------------
# 3. add_new_points
# ------------------------------------------------------------------------------------------
def _rel(X, ref):
    return np.abs(X - ref).max(axis=1) / np.abs(ref).max(axis=1)


@pytest.mark.parametrize("n,gate", [(n, fx.NEW_GATES[0]) for n in fx.NEW_N]
                         + [(300, fx.NEW_GATES[1])])
def test_add_new_points_around_the_gate(ctx, n, gate):
    c = fx.new_points_case(n, gate)
    C1, C2, y1, y2, s, src = c["C1"], c["C2"], c["y1"], c["y2"], c["s"], c["scaled_from"]
    rmask, _ = fx.new_points_ref(y1, y2, C1, C2, gate)
    _dirty(ctx)
    mask, X = gt.add_new_points(y1, y2, C1, C2, gate=gate, ctx=ctx)
    assert mask.dtype == bool and mask.shape == (n,) and X.shape == (n, 3)
    np.testing.assert_array_equal(mask, rmask)            # the scaled and the NaN rows included
    assert np.all(np.isnan(X[~mask])) and np.all(np.isfinite(X[mask]))
    if n > fx.NEW_NAN_ROW:
        assert not mask[fx.NEW_NAN_ROW]
    # a row scaled by 2 has image points (2x, 2y) as far as the triangulation goes, in the
    # oracle as well: no true correspondence, so it is judged like the rows far from the
    # constraint
    plain = src < 0
    near = np.flatnonzero(plain & mask & (np.abs(s) <= 0.5))
    far = np.flatnonzero(mask & (~plain | (np.abs(s) == 0.999)))
    assert len(near) + len(far) == mask.sum()
    oracle = {i: tv.triangulate_optimal(C1, C2, y1[i], y2[i]) for i in list(near) + list(far)}
    worst = 0.0
    if len(near):
        worst = float(_rel(X[near], np.array([oracle[i] for i in near])).max())
        assert worst < 1e-6, worst
    excess = 0.0
    if len(far):
        mine = fx.reprojection_error(C1, C2, y1[far], y2[far], X[far])
        theirs = fx.reprojection_error(C1, C2, y1[far], y2[far],
                                       np.array([oracle[i] for i in far]))
        excess = float((mine / theirs).max()) - 1.0
        assert np.all(mine <= theirs * (1 + LD(1e-6))), excess
    if n >= 300:
        assert (mask & ~plain).sum() >= 2
    print(f"new points n = {n} gate {gate}: {mask.sum()} accepted, {(mask & ~plain).sum()} of "
          f"them scaled; |s| <= 0.5 within {worst:.2e} of the oracle (bar 1e-6); |s| = 0.999 "
          f"and scaled: reprojection error at most 1 {excess:+.2e} of the oracle's")


def test_triangulation_ignores_the_third_component(ctx):
    """The gate reads the third component, the triangulation does not (tables.py:161-175 hands
    whole vectors to lab3.triangulate_optimal, which reads components 0 and 1): with the gate
    wide open, rows that differ in their third components only give X bit for bit."""
    c = fx.new_points_case(129, fx.NEW_GATES[0])
    y1, y2 = c["y1"].copy(), c["y2"].copy()
    y1[:, 2] = y2[:, 2] = 1.0
    z1, z2 = y1.copy(), y2.copy()
    z1[:, 2] = np.tile([2.0, -3.0, 0.5, 1e6], 33)[:129]
    z2[:, 2] = np.tile([2.0, 0.25, -7.0], 43)
    m1, X1 = gt.add_new_points(y1, y2, c["C1"], c["C2"], gate=1e300, ctx=ctx)
    m2, X2 = gt.add_new_points(z1, z2, c["C1"], c["C2"], gate=1e300, ctx=ctx)
    fin = np.isfinite(y1).all(axis=1)
    assert fin.sum() == 128 and np.array_equal(m1, fin) and np.array_equal(m2, fin)
    assert np.all(np.isfinite(X1[fin])) and X1[fin].tobytes() == X2[fin].tobytes()


# ------------------------------------------------------------------------------------------
# 4. ba_residuals / ba_jacobian
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", fx.BA_LAYOUTS)
@pytest.mark.parametrize("n", fx.BA_N)
def test_ba_residuals_and_jacobian_at_block_edges(ctx, n, layout):
    c = fx.ba_case(n, layout)
    args = (c["cams"], c["pts"], c["ov"], c["op"])
    ref, bar, cond = fx.ba_ref(*args, c["uv"])
    _dirty(ctx)
    r = gt.ba_residuals(*args, c["uv"], ctx=ctx)
    _dirty(ctx)
    Jc, Jp = gt.ba_jacobian(*args, ctx=ctx)
    assert r.shape == (2 * n,) and Jc.shape == (n, 2, 12) and Jp.shape == (n, 2, 3)
    assert np.all(np.isfinite(r)) and np.all(np.isfinite(Jc)) and np.all(np.isfinite(Jp))
    # the zero quarters are written, as +0.0 or -0.0 but nothing else
    assert np.all(Jc[:, 0, 4:8] == 0.0) and np.all(Jc[:, 1, 0:4] == 0.0)
    rr = fx.worst_ratio(r, ref["r"], bar["r"])
    rc = fx.worst_ratio(Jc, ref["Jc"], bar["Jc"])
    rp = fx.worst_ratio(Jp, ref["Jp"], bar["Jp"])
    print(f"BA n = {n} {layout}: worst error / bar: r {rr:.3f}, Jc {rc:.3f}, Jp {rp:.3f} "
          f"(largest kappa {cond['kappa'].max():.3g})")
    assert rr <= 1.0 and rc <= 1.0 and rp <= 1.0


def test_ba_empty_input(ctx):
    c = fx.ba_case(1, "nC3")
    e = np.zeros(0, dtype=np.int32)
    r = gt.ba_residuals(c["cams"], c["pts"], e, e, np.zeros((0, 2)), ctx=ctx)
    Jc, Jp = gt.ba_jacobian(c["cams"], c["pts"], e, e, ctx=ctx)
    assert r.shape == (0,) and Jc.shape == (0, 2, 12) and Jp.shape == (0, 2, 3)
    assert r.dtype == Jc.dtype == Jp.dtype == np.float64
    out = gt.match_observations(np.zeros((4, 3)), np.arange(4), np.zeros((0, 3)), ctx=ctx)
    assert out.shape == (0,) and out.dtype == np.int64


# ------------------------------------------------------------------------------------------
# 6. indices are refused, never wrapped
# ------------------------------------------------------------------------------------------
def test_wrapped_indices_raise(ctx):
    c = fx.ba_case(257, "nC3")
    cams, pts, ov, op, uv = c["cams"], c["pts"], c["ov"], c["op"], c["uv"]
    nC, nP = len(cams), len(pts)
    big = 2 ** 32
    ov64, op64 = ov.astype(np.int64), op.astype(np.int64)
    calls = {
        "ba_residuals point + 2^32": lambda: gt.ba_residuals(cams, pts, ov, op64 + big, uv,
                                                             ctx=ctx),
        "ba_residuals view + 2^32": lambda: gt.ba_residuals(cams, pts, ov64 + big, op, uv, ctx=ctx),
        "ba_jacobian point + 2^32": lambda: gt.ba_jacobian(cams, pts, ov, op64 + big, ctx=ctx),
        "ba_residuals point + 0.7": lambda: gt.ba_residuals(cams, pts, ov, op + 0.7, uv, ctx=ctx),
        "bundle_adjust point + 2^32": lambda: gt.bundle_adjust(cams, pts, ov, op64 + big, uv,
                                                               max_iter=1, ctx=ctx),
        "triangulate_nview view + 2^32": lambda: gt.triangulate_nview(cams, pts, ov64 + big, op,
                                                                      uv, ctx=ctx),
        "wash_points view + 2^32": lambda: gt.wash_points(cams, pts, ov64 + big, op, uv, 1e-3,
                                                          ctx=ctx),
        # unchanged: what was refused before still is
        "point -1": lambda: gt.ba_residuals(cams, pts, ov, np.where(np.arange(257) == 9, -1, op),
                                            uv, ctx=ctx),
        "view nC": lambda: gt.ba_residuals(cams, pts, np.where(np.arange(257) == 256, nC, ov), op,
                                           uv, ctx=ctx),
        "point nP": lambda: gt.ba_jacobian(cams, pts, ov, np.where(np.arange(257) == 0, nP, op),
                                           ctx=ctx),
        "nP = 0 with n > 0": lambda: gt.ba_residuals(cams, pts[:0], ov, op * 0, uv, ctx=ctx),
        "cloud entry_obs + 2^32": lambda: cloud.point_attributes(
            cams, pts, np.arange(nP), np.arange(nP, dtype=np.int64) + big, ov, np.zeros((257, 3)),
            ctx=ctx),
        "twoview cam + 2^32": lambda: twoview.triangulate_optimal_batch(
            cams[0], cams[1], uv[:4].T.copy(), uv[4:8].T.copy(), cam=np.full(4, big), ctx=ctx),
        "evaluation faces + 2^32": lambda: evaluation.mesh_distance(
            pts[:5], pts[:3], np.array([[0, 1, 2 + big]]), ctx=ctx),
    }
    for name, call in calls.items():
        with pytest.raises(ValueError):
            call()
            pytest.fail(f"{name}: no ValueError")
    # and the same calls with honest indices go through, integer-valued floats included
    r = gt.ba_residuals(cams, pts, ov.astype(np.float64), op64, uv, ctx=ctx)
    assert r.tobytes() == gt.ba_residuals(cams, pts, ov, op, uv, ctx=ctx).tobytes()
    cloud.point_attributes(cams, pts, np.arange(nP), np.arange(nP, dtype=np.int64), ov,
                           np.zeros((257, 3)), ctx=ctx)
    twoview.triangulate_optimal_batch(cams[0], cams[1], uv[:4].T.copy(), uv[4:8].T.copy(),
                                      cam=np.zeros(4, dtype=np.int64), ctx=ctx)
