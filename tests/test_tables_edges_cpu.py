"""tests/tables_edges_fixture.py without a GPU: every longdouble restatement pinned to the
oracle's own function (oracle/tables_ref.py), and the conditions of the inputs proved on the
reference alone, so that tests/test_gpu_tables_edges.py may demand equal integers and masks of a
float64 kernel:

  * matching: no (query, observation) distance within 1e-9 tol of tol, except in the cases
    decided in exact arithmetic; the rows 0, 255, 256, 511, 512, 513, 1023, 1024 and m - 1 are
    all hit, neighbouring queries in different tiles; the duplicates resolve to the first row;
  * the gate: |e| never within 1e-9 gate of gate; the planted s gate is what e is; |s| = 0.999
    accepted and |s| = 1.001 rejected; the scaled rows carry 4 e;
  * BA: w < 0 for a fifth of the observations at least, kappa in 1e2 .. 1e4 for a fifth at least,
    w never 0, no other kappa above 1e2;
  * ``_ffi.i32c`` raises instead of wrapping or truncating.
"""
import numpy as np
import pytest

import tables_edges_fixture as fx
from oracle import tables_ref as tr
from tsbb15_amd import _ffi

if not fx.LD_OK:
    pytest.skip(fx.LD_REASON, allow_module_level=True)

LD = fx.LD


def test_longdouble_is_extended():
    assert np.finfo(np.longdouble).eps < 1e-18


# ------------------------------------------------------------------------------------------
# 1. matching
# ------------------------------------------------------------------------------------------
def test_match_ref_is_the_oracle():
    for m, n in ((1, 1), (513, 60), (1025, 90)):
        c = fx.match_case(m, n)
        ref = fx.match_ref(c["obs"], c["obs_point"], c["q"], c["tol"])
        np.testing.assert_array_equal(
            ref, tr.match_observations(c["obs"], c["obs_point"], c["q"], c["tol"]))
    for name, c in fx.strict_cases().items():
        ref = fx.match_ref(c["obs"], c["obs_point"], c["q"], c["tol"])
        with np.errstate(invalid="ignore"):
            ora = tr.match_observations(c["obs"], c["obs_point"], c["q"], c["tol"])
        np.testing.assert_array_equal(ref, c["expect"], err_msg=name)
        np.testing.assert_array_equal(ora, c["expect"], err_msg=name)


@pytest.mark.parametrize("m", fx.MATCH_M)
def test_match_cases_keep_their_margin(m):
    worst = np.inf
    for n in fx.MATCH_N:
        c = fx.match_case(m, n)
        assert c["obs"].shape == (m, 3) and c["q"].shape == (n, 3)
        assert np.all(c["obs_point"] > 2 ** 31) and c["obs_point"].dtype == np.int64
        worst = min(worst, fx.match_margin(c["obs"], c["q"], c["tol"]))
        ref = fx.match_ref(c["obs"], c["obs_point"], c["q"], c["tol"])
        aimed = c["row"] >= 0
        # an aimed query is found exactly when its ratio is below 1, a random one never
        assert np.array_equal(ref >= 0, aimed & (c["ratio"] < 1.0))
        first = np.where(c["row"] == 512, 511, np.where(c["row"] == 1024, 0, c["row"]))
        found = ref >= 0
        assert np.array_equal(ref[found], c["obs_point"][first[found]])
        if m == 0:
            assert not aimed.any() and np.all(ref == -1)
    print(f"m = {m}: smallest | d - tol | / tol = {worst:.3e}")
    assert worst > fx.MATCH_MARGIN


@pytest.mark.parametrize("m", [m for m in fx.MATCH_M if m])
def test_match_cases_hit_the_edge_rows(m):
    rows = fx.match_rows(m)
    assert set(rows) == {r for r in fx.MATCH_ROWS + (m - 1,) if r < m}
    for n in (n for n in fx.MATCH_N if n >= 255):
        c = fx.match_case(m, n)
        for r in rows:
            assert set(c["ratio"][c["row"] == r]) == set(fx.MATCH_RATIOS), (m, n, r)
        if m > 512:
            # every wave finds its matches in every tile there is, and neighbouring aimed
            # queries change tile as often as the rows allow (m = 513 has one row in tile 1)
            for lo in range(0, n - 63, 64):
                wave = c["row"][lo:lo + 64]
                assert set(wave[wave >= 0] // fx.TILE) == set(range((m - 1) // fx.TILE + 1))
            tiles = c["row"][c["row"] >= 0] // fx.TILE
            assert np.mean(tiles[1:] != tiles[:-1]) > 1 / 3
            assert np.array_equal(c["obs"][512], c["obs"][511])
        if m > 1024:
            assert np.array_equal(c["obs"][1024], c["obs"][0])


def test_strict_cases_are_what_they_claim():
    cases = fx.strict_cases()
    for name, c in cases.items():
        if not c["exact"]:
            assert fx.match_margin(c["obs"], c["q"], c["tol"]) > fx.MATCH_MARGIN, name
    c = cases["distance equal to tol"]
    assert float(fx.match_distances(c["obs"], c["q"])[0, 0]) == c["tol"] == 2.0 ** -13
    c = cases["tol one ulp above"]
    assert c["tol"] == np.nextafter(2.0 ** -13, 1.0)


# ------------------------------------------------------------------------------------------
# 2. getEFromCameras
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", fx.E_N)
def test_e_ref_is_the_oracle_and_vanishes_on_true_pairs(n):
    C1, C2, is_rigid = fx.e_cameras(n)
    assert is_rigid.sum() == (n + 1) // 2
    E, mag = fx.e_ref(C1, C2)
    assert np.all(mag > 0)
    worst = 0.0
    for i in range(0, n, 16):
        ora = tr.getEFromCameras(C1[i, :, :3], C1[i, :, 3], C2[i, :, :3], C2[i, :, 3])
        worst = max(worst, float((np.abs(ora - E[i]) / (fx.E_FACTOR * fx.EPS * mag[i])).max()))
    assert worst <= 1.0, worst
    # ground truth: the restatement itself satisfies y1^T E y2 = 0 far below the GPU's bar
    y1, y2 = fx.e_truth_points(C1, C2)
    e = np.einsum("nki,nij,nkj->nk", y1, E, y2)
    scale = np.einsum("nki,nij,nkj->nk", np.abs(y1), mag, np.abs(y2))
    for i in np.flatnonzero(is_rigid):
        R1, R2 = C1[i, :, :3], C2[i, :, :3]
        assert np.abs(R1 @ R1.T - np.eye(3)).max() < 1e-14
        assert np.abs(R2 @ R2.T - np.eye(3)).max() < 1e-14
    ratio = float((np.abs(e) / (fx.E_TRUTH_FACTOR * fx.EPS * scale))[is_rigid].max())
    print(f"n = {n}: oracle at {worst:.3f} of the bar, restatement on true pairs at {ratio:.3f}")
    # the rotations are orthogonal to float64 rounding only, which is all the bar allows for
    assert ratio <= 1.0


# ------------------------------------------------------------------------------------------
# 3. add_new_points
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gate", fx.NEW_GATES)
@pytest.mark.parametrize("n", fx.NEW_N)
def test_new_points_cases(n, gate):
    c = fx.new_points_case(n, gate)
    y1, y2, s, src = c["y1"], c["y2"], c["s"], c["scaled_from"]
    assert y1.shape == y2.shape == (n, 3)
    mask, e = fx.new_points_ref(y1, y2, c["C1"], c["C2"], gate)
    if n == 0:
        return
    E, _ = fx.e_ref(c["C1"][None], c["C2"][None])
    fin = np.isfinite(e)
    assert (~fin).sum() == (1 if n > fx.NEW_NAN_ROW else 0) and not mask[~fin].any()
    # the margin: the kernel's e differs from this one by rounding, 1e-16 of its terms
    margin = float((np.abs(np.abs(e[fin]) - LD(gate)) / LD(gate)).min())
    assert margin > fx.NEW_MARGIN, margin
    plain = fin & (src < 0)
    # what was planted is what is there
    assert float(np.abs(e[plain] - LD(gate) * s[plain]).max()) < 1e-12 * gate
    assert np.array_equal(mask[plain], np.abs(s[plain]) < 1.0)
    for v in (0.999, -0.999):
        assert mask[plain & (s == v)].all()
    for v in (1.001, -1.001):
        assert not mask[plain & (s == v)].any()
    if n >= 11:
        assert set(s) == set(fx.NEW_S)
    if n >= 64:
        # both kinds in every wave
        for lo in range(0, n - 63, 64):
            assert 0 < mask[lo:lo + 64].sum() < 64
    sc = np.flatnonzero(src >= 0)
    assert len(sc) == len(range(13, n, 16))
    for k in sc:
        assert np.array_equal(y1[k], 2.0 * y1[src[k]]) and y1[k, 2] == 2.0 == y2[k, 2]
        if np.isfinite(e[src[k]]):
            assert float(abs(e[k] - 4 * e[src[k]])) <= 1e-17
    if n >= 300:
        assert mask[sc].any() and not mask[sc].all()
        assert (mask[sc] & (s[sc] != 0)).any()               # the +-0.2 rows
        assert (~mask[sc] & mask[src[sc]]).any()             # accepted unscaled, rejected scaled
    # the moves are well defined: a^T E d is far from 0
    aEd = np.einsum("ni,ij,j->n", fx._ld(y1[plain]), E[0], fx._ld(fx.NEW_DIRECTION))
    assert float(np.abs(aEd).min()) > 0.3
    # third components other than 1 occur only on the scaled rows
    assert np.all(y2[src < 0, 2] == 1.0)
    # pin to the oracle on the rows it can decide
    ok = np.flatnonzero(fin)[:40]
    E64 = tr.getEFromCameras(c["C1"][:, :3], c["C1"][:, 3], c["C2"][:, :3], c["C2"][:, 3])
    ora = np.array([abs(a @ E64 @ b) < gate for a, b in zip(y1[ok], y2[ok])])
    assert np.array_equal(ora, mask[ok])


# ------------------------------------------------------------------------------------------
# 4. BA
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", fx.BA_LAYOUTS)
@pytest.mark.parametrize("n", fx.BA_N)
def test_ba_cases(n, layout):
    c = fx.ba_case(n, layout)
    cams, pts, ov, op, uv = c["cams"], c["pts"], c["ov"], c["op"], c["uv"]
    nC, nP = len(cams), len(pts)
    assert nC == (1 if layout == "nC1" else 3)
    assert ov.dtype == op.dtype == np.int32 and len(ov) == len(op) == len(uv) == n
    assert ov.min() >= 0 and ov.max() < nC and op.min() >= 0 and op.max() < nP
    if layout == "nP1":
        assert nP == 1
    if layout == "nP2n":
        assert nP == 2 * n and len(np.unique(op)) <= nP // 2
    ref, bar, cond = fx.ba_ref(cams, pts, ov, op, uv)
    w, kappa = cond["w"], cond["kappa"]
    assert np.all(np.isfinite(w)) and np.all(w != 0.0)
    ill = (kappa >= fx.BA_KAPPA[0]) & (kappa <= fx.BA_KAPPA[1])
    assert np.all(kappa[~ill] < fx.BA_KAPPA[0])
    print(f"n = {n} {layout}: nC {nC} nP {nP}, w < 0 for {np.mean(w < 0):.2f}, kappa in "
          f"1e2 .. 1e4 for {np.mean(ill):.2f} (largest {kappa.max():.3g})")
    if n >= 255:
        assert np.mean(w < 0) >= 0.2 and np.mean(ill) >= 0.2
    # the restatement is the oracle's formula: float64 differs from it within the bars
    r = tr.ba_residuals(cams, pts, ov, op, uv[:, 0], uv[:, 1])
    Jc, Jp = tr.ba_jacobian(cams, pts, ov, op)
    assert fx.worst_ratio(r, ref["r"], bar["r"]) <= 1.0
    assert fx.worst_ratio(Jc, ref["Jc"], bar["Jc"]) <= 1.0
    assert fx.worst_ratio(Jp, ref["Jp"], bar["Jp"]) <= 1.0
    assert np.all(bar["r"] > 0) and np.all(bar["Jp"] > 0)
    zero = np.zeros((2, 12), bool)
    zero[0, 4:8] = zero[1, 0:4] = True
    assert np.all((bar["Jc"] == 0) == zero[None]) and np.all(ref["Jc"][:, zero] == 0)


def test_fd_steps():
    case = fx.ba_case(fx.FD_N, "nC3")
    steps = fx.fd_steps(case)
    assert len(steps) == 15
    for name, h, plus, minus in steps:
        what = "cams" if name.startswith("cams") else "pts"
        d = (plus[what] - minus[what]).reshape(-1)
        assert np.count_nonzero(d) == 1 and abs(d[d != 0][0] - 2 * h) <= 1e-15
        assert h >= 1e-6
        other = "pts" if what == "cams" else "cams"
        assert np.array_equal(plus[other], case[other])


# ------------------------------------------------------------------------------------------
# 6. index conversion
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad", [
    np.array([0, 2 ** 32 + 1]), np.array([-2 ** 31 - 1]), np.array([2 ** 31]), [1.7],
    np.array([0.0, np.nan]), [np.inf], np.array([2.0 ** 40]), np.array([2 ** 63], dtype=np.uint64),
    np.array(["1"]), np.array([1 + 0j]), np.array([None, 1]), [True, False], [2 ** 70]])
def test_i32c_raises(bad):
    with pytest.raises(ValueError, match="the index"):
        _ffi.i32c(bad, "the index")


def test_i32c_converts():
    out = _ffi.i32c(np.array([3.0, -1.0, 2.0 ** 31 - 1]), "x")
    assert out.dtype == np.int32 and list(out) == [3, -1, 2 ** 31 - 1]
    assert list(_ffi.i32c([-2 ** 31, 0], "x")) == [-2 ** 31, 0]
    assert _ffi.i32c(np.arange(4, dtype=np.uint8), "x").dtype == np.int32
    a = np.arange(6, dtype=np.int32)
    assert _ffi.i32c(a, "x") is a                              # no copy
    b = _ffi.i32c(a[::2], "x")
    assert b.flags.c_contiguous and list(b) == [0, 2, 4]
    for empty in ([], np.zeros((0, 3)), np.zeros(0, dtype=np.int64)):
        e = _ffi.i32c(empty, "x")
        assert e.dtype == np.int32 and e.shape == np.shape(empty)


def test_wrappers_refuse_a_wrapped_index_before_the_library():
    """The conversion stands in front of every call, so these need no GPU: an index 2^32 too
    large is refused, not wrapped onto a valid one."""
    from tsbb15_amd import cloud, evaluation, tables, twoview
    cams, pts = np.zeros((2, 3, 4)), np.zeros((3, 3))
    ov, op = np.array([0, 1]), np.array([1, 2])
    with pytest.raises(ValueError, match="obs_point"):
        tables._ba_args(cams, pts, ov, op + 2 ** 32)
    with pytest.raises(ValueError, match="obs_view"):
        tables._ba_args(cams, pts, ov + 2 ** 32, op)
    with pytest.raises(ValueError, match="obs_point"):
        tables._ba_args(cams, pts, ov, [1.7, 2])
    assert tables._ba_args(cams, pts, ov.astype(float), op)[2].dtype == np.int32
    with pytest.raises(ValueError, match="entry_obs"):
        cloud._index(np.array([2 ** 32]), "entry_obs")
    with pytest.raises(ValueError, match="cam"):
        twoview.triangulate_optimal_batch(np.zeros((3, 4)), np.zeros((3, 4)), np.zeros((2, 1)),
                                          np.zeros((2, 1)), cam=np.array([2 ** 32]))
    with pytest.raises(ValueError):
        evaluation._faces(np.array([[0, 1, 2 + 2 ** 32]]), 3)
