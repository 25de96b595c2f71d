"""tests/boundary_fixture.py on the CPU: every case sits exactly on the boundary it names, and the
restatements (dense_ref, surface_ref, texture_ref) are unambiguous there.  This is what lets
tests/test_gpu_boundaries.py compare flags, counts and indices with no pixel excused.  Nothing
here touches the GPU.
"""
from fractions import Fraction

import numpy as np
import pytest

import boundary_fixture as bf
import dense_ref as dr
import surface_ref as sr
import texture_ref as tr

SWEEPS = tuple(bf.sweep_cases())


# ------------------------------------------------------------------------------------------
# plane sweep
# ------------------------------------------------------------------------------------------
def _coords(case):
    """(k, s) -> (x', y', valid) of every reference pixel, fp64."""
    h, w = case["ref"].shape
    return {(k, s): dr.warp_coords(case["A"][s], case["b"][s], d, h, w)
            for k, d in enumerate(case["depths"]) for s in range(len(case["srcs"]))}


@pytest.mark.parametrize("name", SWEEPS)
def test_sweep_inputs_are_dyadic(name):
    """Grey levels within 16 of 128; every valid sample has interpolation weights in {0, 1/2}
    and is either exactly on a boundary of the validity predicate or at least 1/2 px inside."""
    case = bf.sweep_cases()[name]
    h, w = case["ref"].shape
    for img in (case["ref"],) + tuple(case["srcs"]):
        assert img.dtype == np.uint8 and img.min() >= 112 and img.max() <= 144
    coords = _coords(case)
    for xs, ys, valid in coords.values():
        fx, fy = xs[valid] - np.floor(xs[valid]), ys[valid] - np.floor(ys[valid])
        assert np.all(np.isin(fx, (0.0, 0.5))) and np.all(np.isin(fy, (0.0, 0.5)))
        with np.errstate(invalid="ignore"):
            out = np.isfinite(xs) & ~valid
            miss = np.maximum.reduce([-xs, xs - (w - 1.0), -ys, ys - (h - 1.0)])
        # an invalid finite coordinate with q2 d > 0 misses the image by half a pixel or more
        assert np.all(miss[out & (miss > 0)] >= 0.5)


@pytest.mark.parametrize("name, k, y, x, want", [
    # x' == 0 and x' == -1/2; x' == w - 1 (the right neighbour is clamped, fx == 0), w - 1/2, w
    ("xneg_9x33_p3", 0, 4, 4, (0.0, 4.0, True)),
    ("xneg_9x33_p3", 3, 4, 0, (-0.5, 4.0, False)),
    ("xpos_8x32_p3", 0, 3, 27, (31.0, 3.0, True)),
    ("xpos_8x32_p3", 3, 3, 31, (31.5, 3.0, False)),
    ("xpos_8x32_p3", 2, 3, 31, (32.0, 3.0, False)),
    ("xpos_8x32_p3", 3, 3, 30, (30.5, 3.0, True)),
    # y' == h - 1, h - 1/2 and -1/2
    ("ypos_16x64_p3", 1, 13, 9, (9.0, 15.0, True)),
    ("ypos_16x64_p3", 3, 15, 9, (9.0, 15.5, False)),
    ("yneg_9x33_p3", 2, 1, 9, (9.0, 0.0, True)),
    ("yneg_9x33_p3", 3, 0, 9, (9.0, -0.5, False)),
    # q2 d == 0, and one dyadic step (q2 = d) beside it
    ("q2_zero", 0, 3, 12, (8.0, 3.0, True)),
    ("q2_zero", 0, 3, 15, (3.5, 3.0, True)),
])
def test_sweep_coordinates_on_the_boundary(name, k, y, x, want):
    case = bf.sweep_cases()[name]
    xs, ys, valid = _coords(case)[(k, 0)]
    assert (xs[y, x], ys[y, x], bool(valid[y, x])) == want


def test_sweep_q2_is_exactly_zero():
    case = bf.sweep_cases()["q2_zero"]
    A, d = case["A"][0], case["depths"][0]
    x = np.arange(16.0)
    q2 = d * (A[2, 0] * x + A[2, 2]) + case["b"][0][2]
    assert q2[11] == 0.0 and q2[12] == d and np.all(q2[:11] * d < 0)
    xs, ys, valid = _coords(case)[(0, 0)]
    assert np.all(np.isinf(xs[:, 11])) and np.isnan(ys[3, 11]) and not valid[:, :12].any()
    assert valid[:, 12:].all()


@pytest.mark.parametrize("name", SWEEPS)
def test_sweep_flags_do_not_depend_on_the_arithmetic(name):
    """Condition 2: float32 with reversed window sums and fp64 give the same NaN pattern and the
    same nvalid; and the hand-written validity, where there is one, is the restatement's."""
    v64, n64 = bf.reference_sweeps()[name][4:6]
    v32, n32 = bf.fp32_sweeps()[name]
    assert np.array_equal(np.isnan(v32), np.isnan(v64)) and np.array_equal(n32, n64)
    hand = bf.hand_valid(name)
    if hand is not None:
        assert np.array_equal(~np.isnan(v64), hand)
        assert np.array_equal(n64, hand.astype(np.uint8))


@pytest.mark.parametrize("name", SWEEPS)
def test_sweep_no_pixel_needs_excusing(name):
    """Condition 3: with the later copies of a repeated depth left out, the best-to-second gap
    of the restatement exceeds twice the cost bar at every valid pixel; the copies themselves
    tie bit for bit and the first wins."""
    case = bf.sweep_cases()[name]
    index, _, _, _, vol, _ = bf.reference_sweeps()[name]
    bar = bf.score_bar()
    keep = bf.first_of_ties(case["depths"])
    for k in range(len(case["depths"])):
        first = list(case["depths"]).index(case["depths"][k])
        assert np.array_equal(vol[k], vol[first], equal_nan=True)
        assert not np.any(index == k) or first == k
    if len(keep) > 1:
        srt = np.sort(np.where(np.isnan(vol[keep]), -np.inf, vol[keep]), axis=0)
        with np.errstate(invalid="ignore"):
            gap = (srt[-1] - srt[-2])[index >= 0]
        assert np.all(gap > 2 * bar), (name, float(gap.min()), bar)


def test_sweep_bar():
    dev = bf.fp32_deviation()
    worst = max(dev, key=dev.get)
    print(f"largest fp32-reversed against fp64 deviation {dev[worst]:.3e} ({worst}), "
          f"bar {bf.score_bar():.3e}")
    assert 0.0 < bf.score_bar() < 1e-3


def test_sweep_both_sides_of_every_window_boundary():
    """A window whose outermost sample lies exactly on the last column (or the first, or the
    last or first row) is valid, the next one is not: both occur in each shift case."""
    for name in ("xpos_8x32_p3", "xneg_9x33_p3", "ypos_16x64_p3", "yneg_9x33_p3",
                 "xpos_12x44_p11"):
        case = bf.sweep_cases()[name]
        h, w = case["ref"].shape
        r = case["patch"] // 2
        axis, t = case["shift"]
        vol = bf.reference_sweeps()[name][4]
        for k, d in enumerate(case["depths"]):
            s = t / d
            if s != int(s):
                continue
            n = (w, h)[axis]
            last = n - 1 - r - int(s) if s > 0 else r - int(s)     # outermost sample on the edge
            step = 1 if s > 0 else -1
            mid = (h // 2, last) if axis == 0 else (last, w // 2)
            nxt = (h // 2, last + step) if axis == 0 else (last + step, w // 2)
            assert not np.isnan(vol[k][mid]) and np.isnan(vol[k][nxt]), (name, k)
            assert r <= last + step <= n - 1 - r                   # its window is in the image


def test_sweep_variance_thresholds():
    """Condition 1 for va and vb: exactly min_var n^2 = 162, which float32 holds; the twin's
    threshold is above 162 in float32 as well as in fp64."""
    n = 9
    assert float(np.float32(bf.MIN_VAR * n * n)) == bf.MIN_VAR * n * n == 162.0
    assert np.float32(bf.MIN_VAR_ABOVE * n * n) > np.float32(162.0)
    assert bf.MIN_VAR_ABOVE * n * n > 162.0
    c, r0 = bf.PLANT
    for side in ("ref", "src"):
        on, above = bf.sweep_cases()[f"var_{side}_on"], bf.sweep_cases()[f"var_{side}_above"]
        img = (on["ref"] if side == "ref" else on["srcs"][0]).astype(np.int64) - 128
        win = img[r0:r0 + 3, c - 1:c + 2]
        assert n * (win * win).sum() - win.sum() ** 2 == 162
        _, nv, vb = dr.cost_volume(on["ref"], on["srcs"], on["A"], on["b"], on["depths"], 3,
                                   on["min_var"], details=True)
        if side == "src":       # the warped window of plane 0 (shift 1), vb / n as details gives it
            assert vb[0, 0, r0 + 1, c - 1] * n == 162.0
        assert nv.sum() == 3 * len(on["depths"])
        assert bf.reference_sweeps()[f"var_{side}_above"][3].sum() == 0
        assert np.all(bf.reference_sweeps()[f"var_{side}_above"][0] == -1)
        assert above["min_var"] > on["min_var"]


def test_sweep_ties():
    """The first of a repeated depth wins and delta is what the header's formula gives.  With
    c+ == c0 the formula is 0.5 in real arithmetic; in floating point (c- - 2 c0) is rounded
    before c+ is added, so it is 0.5 or the float just below unless the three costs make every
    step exact, which tie_exact arranges: its costs are -1, 1, 1 in float32 and in fp64."""
    for name, k in (("tie_pair", 2), ("tie_triple", 1)):
        index, delta, _, _, vol, _ = bf.reference_sweeps()[name]
        assert set(np.unique(index)) == {-1, k}
        won = (index == k) & ~np.isnan(vol[k - 1])          # c- exists as well
        assert won.sum() >= 100 and np.array_equal(vol[k + 1][won], vol[k][won])
        assert np.all(np.abs(delta[won] - 0.5) <= 1e-9) and np.all(delta[won] <= 0.5)
    index, delta, score, _, vol, _ = bf.reference_sweeps()["tie_exact"]
    won = index == 1
    assert won.sum() == 6 * 28 and np.all(index[1:7, 29] == 0) and (index >= 0).sum() == 6 * 29
    for v in (vol, bf.fp32_sweeps()["tie_exact"][0]):
        assert np.all(v[0][won] == -1.0) and np.all(v[1][won] == 1.0) and np.all(v[2][won] == 1.0)
    assert np.all(delta[won] == 0.5) and np.all(delta[~won] == 0.0)
    w32 = dr.winners(*bf.fp32_sweeps()["tie_exact"])
    assert w32[1].dtype == np.float32 and np.all(w32[1][won] == np.float32(0.5))


def test_sweep_twin_sources_and_deep_ladders():
    one, two = bf.reference_sweeps()["xpos_8x32_p3"], bf.reference_sweeps()["twin_sources"]
    assert np.array_equal(two[4], one[4], equal_nan=True)
    assert np.array_equal(two[3], 2 * one[3]) and np.array_equal(two[0], one[0])
    for name, k in (("deep_last", 4095), ("deep_first", 0)):
        index, _, score, nvalid, vol, _ = bf.reference_sweeps()[name]
        want = np.full((4, 4), -1)
        want[1:3, 1] = k
        assert np.array_equal(index, want)
        assert (~np.isnan(vol)).sum() == 2 and np.all(score[1:3, 1] == 1.0)


# ------------------------------------------------------------------------------------------
# consistency
# ------------------------------------------------------------------------------------------
def _consistency(case, **kw):
    return dr.consistency(case["depth"], case["P"], bf.I3, case["rel_tol"], **kw)


@pytest.mark.parametrize("name", tuple(bf.consistency_cases()))
def test_consistency_matrices_and_margins(name):
    """What the restatement computes from (P, I3) is the P and Minv the C entry is given, bit for
    bit; every rounding and every tolerance test is exactly on its boundary or well off it."""
    case = bf.consistency_cases()[name]
    for P, Minv in zip(case["P"], case["Minv"]):
        assert np.array_equal(bf.I3 @ P, P)
        assert np.array_equal(np.linalg.inv((bf.I3 @ P)[:, :3]), Minv)
    count, half, tol = _consistency(case, details=True)
    assert np.all((half == 0.0) | (half >= 0.05))
    assert np.all((tol == 0.0) | (tol >= 1e-3) | (tol <= 1e-15))   # on, well off, or one double
    if name.startswith("half_pixel"):
        assert (half == 0.0).sum() >= 20 and (tol == 0.0).any()
        assert np.array_equal(count[0], bf.HALF_PIXEL_VIEW0[case["rel_tol"]])
        assert np.all(count[1][~np.isfinite(case["depth"][1])] == 0)
        assert np.all(count[1, 2, :2] == 0)        # v == h - 1/2 goes to row h: outside
        assert count[1, 0, 0] == 1                 # u == -1/2 goes to pixel 0: inside
    if name == "views128":
        assert np.all(count == 127)
    if name.startswith("lanes"):
        assert int(name[5:]) == case["depth"].size and len(np.unique(count)) >= 2


def test_consistency_half_integers():
    """The projections themselves: (d x + m0) / d in fp64, exactly k + 1/2."""
    case = bf.consistency_cases()["half_pixel_tol25"]
    X = dr.depth_points(case["depth"][0], case["P"][0], bf.I3)
    q = X @ case["P"][1][:, :3].T + case["P"][1][:, 3]
    assert np.array_equal(q[..., 0] / q[..., 2], np.arange(6.0) + 0.5 + np.zeros((3, 1)))
    assert np.array_equal(q[..., 1] / q[..., 2], np.arange(3.0)[:, None] - 0.5 + np.zeros(6))
    assert np.floor(2.5 + 0.5) == 3 and np.floor(-0.5 + 0.5) == 0 and np.floor(5.5 + 0.5) == 6


# ------------------------------------------------------------------------------------------
# TSDF fusion, extraction
# ------------------------------------------------------------------------------------------
def _exact_tsdf(case):
    """rs_surface_integrate restated once more, node by node in rational arithmetic: (T, W) as
    Fractions (None for NaN) and the smallest non-zero distances to the two boundaries.  A
    projection or a depth that is not finite contributes nothing, as in the header."""
    F = Fraction
    nz, ny, nx = case["dims"]
    V, h, w = case["depth"].shape
    T, W = np.empty(case["dims"], object), np.empty(case["dims"], object)
    on = dict(round=0, trunc=0, plus=0)
    off = dict(round=F(1), trunc=F(1))
    for iz in range(nz):
        for iy in range(ny):
            for ix in range(nx):
                X = [F(o) + F(case["voxel"]) * i for o, i in zip(case["origin"], (ix, iy, iz))]
                acc, wsum = F(0), F(0)
                for v in range(V):
                    q = [sum(F(p) * c for p, c in zip(row[:3], X)) + F(row[3])
                         for row in case["P"][v]]
                    if q[2] == 0:
                        continue
                    fu, fv = q[0] / q[2] + F(1, 2), q[1] / q[2] + F(1, 2)
                    for f in (fu, fv):
                        m = abs(f - round(f))
                        on["round"] += m == 0
                        off["round"] = min(off["round"], m) if m else off["round"]
                    u, r = fu.__floor__(), fv.__floor__()
                    if not (0 <= u <= w - 1 and 0 <= r <= h - 1):
                        continue
                    d = case["depth"][v, r, u]
                    wv = 1.0 if case["weights"] is None else float(case["weights"][v, r, u])
                    if not (np.isfinite(d) and F(d) * q[2] > 0 and np.isfinite(wv) and wv > 0):
                        continue
                    s = abs(F(d)) - abs(q[2])
                    m = abs(s + F(case["trunc"]))
                    on["trunc"] += m == 0
                    on["plus"] += s == F(case["trunc"])
                    off["trunc"] = min(off["trunc"], m) if m else off["trunc"]
                    if s >= -F(case["trunc"]):
                        acc += F(wv) * min(F(1), s / F(case["trunc"]))
                        wsum += F(wv)
                W0 = 0.0 if case["weight"] is None else float(case["weight"][iz, iy, ix])
                W0 = F(W0) if W0 > 0 else F(0)
                prior = W0 * F(float(case["tsdf"][iz, iy, ix])) if W0 > 0 else F(0)
                W[iz, iy, ix] = W0 + wsum
                T[iz, iy, ix] = (prior + acc) / (W0 + wsum) if W0 + wsum > 0 else None
    return T, W, on, off


@pytest.mark.parametrize("name", tuple(bf.tsdf_cases()))
def test_tsdf_on_the_boundaries(name):
    case = bf.tsdf_cases()[name]
    assert np.array_equal(bf.I3 @ case["P"], case["P"])
    margins = {}
    T, W = sr.integrate(case["depth"], case["P"], bf.I3, case["origin"], case["voxel"],
                        case["dims"], case["trunc"], case["weights"], case["tsdf"],
                        case["weight"], margins)
    assert margins["round"] == 0.0 and margins["trunc"] == 0.0
    Tx, Wx, on, off = _exact_tsdf(case)
    print(f"{name}: {on['round']} projections on a half-integer, {on['trunc']} samples with "
          f"s == -trunc, {on['plus']} with s == trunc; the nearest other ones are "
          f"{float(off['round']):.3g} px and {float(off['trunc']):.3g} away")
    assert on["round"] >= 4 and on["trunc"] >= 1 and on["plus"] >= 1
    assert off["round"] >= Fraction(1, 8)
    # the exact quotient is an fp64 number (so fp64 arithmetic cannot round it two ways), and
    # rounded to float32 it is the restatement's; all but the quotients one double off 1 or 0
    # are float32 numbers themselves
    in32 = 0
    for i in np.ndindex(case["dims"]):
        assert float(np.float32(float(Wx[i]))) == Wx[i] and W[i] == float(Wx[i])
        if Tx[i] is None:
            assert np.isnan(T[i])
            continue
        assert Fraction(float(Tx[i])) == Tx[i]
        assert np.float32(float(Tx[i])) == T[i]
        in32 += Fraction(float(T[i])) == Tx[i]
    finite = int(np.isfinite(T).sum())
    print(f"{name}: {finite} finite nodes, {in32} of them exactly float32")
    assert finite - in32 <= finite // 4
    if name == "plain":
        assert np.all(np.isnan(T[0])) and np.all(W[0] == 0)            # the camera plane
        assert T[4, 0, 0] == -1.0 and W[4, 0, 0] == 1.0                # s == -trunc
        assert np.isnan(T[4, 0, 2]) and W[4, 0, 2] == 0.0              # one step behind
        assert T[2, 0, 1] == 1.0 and np.isnan(T[2, 0, 7])              # u == -1/2 in, 5/2 out
    if name == "weights":
        assert set(np.unique(W)) == {0.0, 1.0, 2.0}
    if name == "prior":
        assert np.all(np.isfinite(T[:, :, (0, 4, 6)])) and np.all(np.isfinite(W))


@pytest.mark.parametrize("name", tuple(bf.extract_cases()))
def test_extract_cases(name):
    tsdf, weight, origin, voxel, min_weight, nf = bf.extract_cases()[name]
    v, f = sr.extract(tsdf, weight, origin, voxel, min_weight)
    if nf is not None:
        assert len(f) == nf and len(v) == 0
    else:
        assert len(f) >= 1 and len(v) == 7 and np.all(np.isin(v, (0.0, 0.5)))
    if name == "minus_zero":
        assert np.signbit(tsdf[0, 0, 0]) and tsdf[0, 0, 0] == 0.0
    if name.startswith("weight"):
        assert (float(weight[1, 0, 1]) >= min_weight) == (name == "weight_on")
        assert np.all(np.delete(weight.ravel(), 5) > min_weight)


# ------------------------------------------------------------------------------------------
# z-buffer, gather
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", tuple(bf.raster_cases()))
def test_raster_cases(name):
    v, f, shape, hand = bf.raster_cases()[name]
    margins = {}
    z = tr.render_depth(v, f, bf.TEX_P, shape, margins)
    if name != "camera_plane":
        assert margins["b"] == 0.0
    if hand is not None:
        assert np.array_equal(z.view(np.int32), hand.view(np.int32))
    n = shape[0]
    covered = int(np.isfinite(z).sum())
    want = {"pair": n * n, "one_": n * (n + 1) // 2, "othe": n * (n + 1) // 2, "came": 0,
            "slan": 45}[name[:4]]
    assert covered == want
    if name[:4] in ("pair", "one_", "othe"):
        box = tr.box_pixels(v, f[0], bf.TEX_P, shape)
        assert box == n * n and (box > 32) == name.endswith("large")
        x = tr.project(bf.TEX_P[0], v)
        assert np.array_equal(x[:, :2] / x[:, 2:], np.round(x[:, :2] / x[:, 2:]))
        assert np.signbit(v[0, 0]) and v[0, 0] == 0.0


@pytest.mark.parametrize("name", tuple(bf.gather_cases()))
def test_gather_cases(name):
    case = bf.gather_cases()[name]
    P, centres = tr.turn(bf.TEX_P)
    assert np.array_equal(P, bf.TEX_P) and np.all(centres == 0.0)
    margins, detail = {}, {}
    col, count, z = tr.vertex_colors(case["vertices"], case["faces"], bf.gather_images(3),
                                     bf.TEX_P, case["normals"], case["rel_tol"],
                                     case["min_cos"], margins=margins, detail=detail)
    assert margins["inside"] == 0.0 and margins["visible"] == 0.0
    if case["count"] is not None:
        assert count.tolist() == case["count"]
    foot = lambda x0, y0: int(np.isfinite(z[0, y0:y0 + 2, x0:x0 + 2]).sum())
    assert foot(2, 3) == 1 and foot(1, 4) == 0
    if case["normals"] is not None:
        X = case["vertices"][12]
        assert X @ case["normals"][12] / -np.sqrt(X @ X) == 0.8 == 4.0 / 5.0
        assert count[12] == (name == "cos_below")
        assert margins["cos"] == (0.0 if name == "cos_on" else 0.8 - bf.down(0.8))
        assert detail["g"][3, 0] == 1.0 and count[3] == 1
    col1, count1, _ = tr.vertex_colors(case["vertices"], case["faces"], bf.gather_images(1),
                                       bf.TEX_P, case["normals"], case["rel_tol"],
                                       case["min_cos"])
    assert np.array_equal(count1, count) and np.array_equal(col1[:, 0], col[:, 0])
