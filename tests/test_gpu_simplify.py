"""Mesh simplification on the GPU (tsbb15_amd.surface.simplify, csrc/simplify.hip) against the
numpy restatement tests/simplify_ref.py on the meshes of tests/simplify_fixture.py.

Bars.  Every result is unique -- integer atomics whose order a sort removes, fp64 sums in a stated
order, no product fused with a sum -- so positions, quadrics, faces, vmap, fmap and the info record
are compared bit for bit; there is no tolerance anywhere in this file.

The cases put the cluster count and the cell count one below, at and one above the scan's chunk of
2048 (and the clusters at 63, 64, 65 and 4097), the rows one below, at and one above the switch
from insertion to heap sort (24 | 25) and the wave (64), at about 1 500 (the random mesh at cell 3)
and at every corner of a mesh that lies in one cell; vertices stand exactly on cell faces in the
chains, in ``on_cell_faces`` and, for the default origin, in every case that uses it (the minimum
lies on the first cell's lower face).
"""
import ctypes

import numpy as np
import pytest

import dense_fixture as df
import mesh_fixture as mfx
import simplify_fixture as sx
import simplify_ref as ref
import surface_fixture as sfx
from tsbb15_amd import _ffi, surface

pytestmark = pytest.mark.gpu

_i32 = ctypes.c_int32
_i64 = ctypes.c_int64
_d = ctypes.c_double
FILL = 0x5A


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64) if a.dtype == np.float64 else a.view(np.int32) \
        if a.dtype == np.float32 else a


def _same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape)
    assert np.array_equal(_bits(got), _bits(want)), what


def _check(name, ctx, placement="quadric", rank_tol=1e-3):
    v, f, cell, origin = sx.cases()[name]
    res = sx.reference(name, placement, rank_tol)
    vo, fo, vmap, info = surface.simplify(v, f, cell, origin=origin, placement=placement,
                                          rank_tol=rank_tol, drop_unreferenced=False,
                                          return_info=True, ctx=ctx)
    what = f"{name} {placement} {rank_tol}"
    _same(vmap, res["vmap"], what + ": vmap")
    _same(info["fmap"], res["fmap"], what + ": fmap")
    _same(fo, res["faces"], what + ": faces")
    _same(info["quadrics"], res["quadrics"], what + ": quadrics")
    _same(vo, res["vertices"], what + ": vertices")
    assert {k: info[k] for k in ref.INFO_KEYS} == res["info"], what
    assert info["unreferenced"] == int(ref.unreferenced(res).sum())
    return res


# ------------------------------------------------------------------------------------------
# every case, both placements
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("placement", surface.SIMPLIFY_PLACEMENTS)
@pytest.mark.parametrize("name", sorted(sx.cases()))
def test_cases_match_the_restatement(name, placement, ctx):
    _check(name, ctx, placement)


@pytest.mark.parametrize("name", ["cube", "two_spheres_3.0", "two_spheres_1.5", "random_2.0",
                                  "two_spheres_permuted", "plane_slanted", "zero_area"])
def test_rank_tol_zero(name, ctx):
    _check(name, ctx, "quadric", 0.0)


def test_the_order_of_the_sums_is_part_of_the_result(ctx):
    """The permuted two-sphere mesh is the same surface, and gives the same clusters, but its sums
    run in another order: it is compared with the restatement of the permuted mesh (above), and
    here only what does not depend on the order is compared with the original."""
    a, b = sx.reference("two_spheres_3.0"), sx.reference("two_spheres_permuted")
    assert a["info"]["clusters"] == b["info"]["clusters"]
    assert np.array_equal(a["keys"], b["keys"])
    assert np.allclose(a["mean"], b["mean"], rtol=0, atol=1e-12)
    assert not np.array_equal(_bits(a["mean"]), _bits(b["mean"]))


def test_twice_the_same_bits(ctx):
    v, f, cell, origin = sx.cases()["random_3.0"]
    a = surface.simplify(v, f, cell, return_info=True, ctx=ctx)
    b = surface.simplify(v, f, cell, return_info=True, ctx=ctx)
    for x, y in zip(a[:3] + (a[3]["quadrics"],), b[:3] + (b[3]["quadrics"],)):
        _same(x, y, "second call")


def test_branch_counts(ctx):
    seen = dict.fromkeys(("fallbacks", "duplicate_faces", "degenerate_faces", "unreferenced"), 0)
    for name in ("two_spheres_3.0", "two_spheres_1.5", "random_2.0"):
        v, f, cell, origin = sx.cases()[name]
        info = surface.simplify(v, f, cell, return_info=True, ctx=ctx)[3]
        print(name, {k: info[k] for k in ref.INFO_KEYS + ("unreferenced",)})
        for k in seen:
            seen[k] = max(seen[k], info[k])
    assert all(n > 0 for n in seen.values()), seen


# ------------------------------------------------------------------------------------------
# the C call: capacities, empty meshes, argument errors
# ------------------------------------------------------------------------------------------
class _Raw:
    """One rs_mesh_simplify call on arrays pre-filled with FILL."""

    def __init__(self, ctx, v, f, origin, cell, dims, placement=1, rank_tol=1e-3, vcap=None,
                 fcap=None, nv=None, nf=None):
        self.v = np.ascontiguousarray(v, dtype=np.float64).reshape(-1, 3)
        self.f = np.ascontiguousarray(f, dtype=np.int32).reshape(-1, 3)
        n = len(self.v) if nv is None else nv
        m = len(self.f) if nf is None else nf
        vcap = len(self.v) if vcap is None else vcap
        fcap = len(self.f) if fcap is None else fcap
        self.vout = np.full((max(vcap, 0), 3), np.nan)
        self.fout = np.full((max(fcap, 0), 3), FILL, np.int32)
        self.vmap = np.full(len(self.v), FILL, np.int32)
        self.fmap = np.full(len(self.f), FILL, np.int32)
        self.quad = np.full((max(vcap, 0), 10), np.nan)
        self.info = _ffi.SimplifyInfo(*([FILL] * 5))
        self.nv, self.nf = _i64(-7), _i64(-7)
        origin = np.ascontiguousarray(origin, dtype=np.float64)
        dims = np.ascontiguousarray(dims, dtype=np.int64)

        def p(a, t):
            return _ffi.ptr(a, t) if a.size else None

        self.status = _ffi.lib().rs_mesh_simplify(
            ctx.handle, p(self.v, _d), n, p(self.f, _i32), m, _ffi.ptr(origin, _d), cell,
            _ffi.ptr(dims, _i64), placement, rank_tol, p(self.vout, _d), vcap,
            p(self.fout, _i32), fcap, p(self.vmap, _i32), p(self.fmap, _i32), p(self.quad, _d),
            ctypes.byref(self.nv), ctypes.byref(self.nf), ctypes.byref(self.info))

    def untouched(self):
        return (np.isnan(self.vout).all() and np.isnan(self.quad).all() and
                np.all(self.fout == FILL) and np.all(self.vmap == FILL) and
                np.all(self.fmap == FILL) and
                all(getattr(self.info, k) == FILL for k in ref.INFO_KEYS))


def test_capacity_protocol(ctx):
    v, f, cell, origin = sx.cases()["two_spheres_3.0"]
    origin, dims = ref.grid(v, cell, origin)
    res = sx.reference("two_spheres_3.0")
    nc, nk = len(res["vertices"]), len(res["faces"])
    for vcap, fcap in ((0, 0), (nc - 1, nk), (nc, nk - 1)):
        r = _Raw(ctx, v, f, origin, cell, dims, vcap=vcap, fcap=fcap)
        assert r.status == _ffi.RS_EINVAL, (vcap, fcap)
        assert (r.nv.value, r.nf.value) == (nc, nk)
        assert r.untouched(), (vcap, fcap)
    r = _Raw(ctx, v, f, origin, cell, dims, vcap=nc, fcap=nk)
    assert r.status == 0 and (r.nv.value, r.nf.value) == (nc, nk)
    _same(r.vout, res["vertices"], "exact capacity: vertices")
    _same(r.fout, res["faces"], "exact capacity: faces")
    _same(r.quad, res["quadrics"], "exact capacity: quadrics")
    _same(r.vmap, res["vmap"], "exact capacity: vmap")
    _same(r.fmap, res["fmap"], "exact capacity: fmap")
    assert {k: getattr(r.info, k) for k in ref.INFO_KEYS} == res["info"]


def test_empty_meshes(ctx):
    r = _Raw(ctx, np.zeros((0, 3)), np.zeros((0, 3), np.int32), np.zeros(3), 1.0, (1, 1, 1))
    assert r.status == 0 and (r.nv.value, r.nf.value) == (0, 0)
    assert all(getattr(r.info, k) == 0 for k in ref.INFO_KEYS)
    vo, fo, vmap, info = surface.simplify(np.zeros((0, 3)), np.zeros((0, 3), np.int32), 1.0,
                                          return_info=True, ctx=ctx)
    assert vo.shape == (0, 3) and fo.shape == (0, 3) and vmap.shape == (0,)
    assert fo.dtype == vmap.dtype == np.int32 and info["clusters"] == 0
    # vertices without a face: the clusters and their means, no face
    v = sx.cases()["no_face"][0]
    for drop in (False, True):
        vo, fo, vmap, info = surface.simplify(v, np.zeros((0, 3), np.int32), 1.0,
                                              origin=np.zeros(3), drop_unreferenced=drop,
                                              return_info=True, ctx=ctx)
        assert len(fo) == 0 and info["clusters"] == 2 and info["unreferenced"] == 2
        assert len(vo) == (0 if drop else 2) and np.all((vmap == -1) == drop)


def test_c_argument_errors(ctx):
    v, f, cell, origin = sx.cases()["one_face"]
    dims = (3, 3, 2)
    assert _Raw(ctx, v, f, origin, cell, dims).status == 0
    nan, inf = float("nan"), float("inf")
    bad = {
        "cell zero": dict(cell=0.0), "cell negative": dict(cell=-1.0),
        "cell nan": dict(cell=nan), "cell inf": dict(cell=inf),
        "dim zero": dict(dims=(3, 0, 2)), "dim negative": dict(dims=(3, 3, -1)),
        "too many cells": dict(dims=(1 << 9, 1 << 9, (1 << 9) + 1)),
        "cells overflow": dict(dims=(1 << 40, 1 << 40, 1 << 40)),
        "placement 2": dict(placement=2), "placement -1": dict(placement=-1),
        "rank_tol 1": dict(rank_tol=1.0), "rank_tol negative": dict(rank_tol=-1e-3),
        "rank_tol nan": dict(rank_tol=nan),
        "origin nan": dict(origin=(0.0, nan, 0.0)),
        "vertex above the grid": dict(dims=(2, 3, 2)),
        "vertex below the grid": dict(origin=(0.3, 0.0, 0.0)),
        "negative nv": dict(nv=-1), "negative nf": dict(nf=-1),
        "negative capacity": dict(vcap=-1),
    }
    for what, change in bad.items():
        kw = dict(origin=origin, cell=cell, dims=dims)
        kw.update(change)
        r = _Raw(ctx, v, f, **kw)
        assert r.status == _ffi.RS_EINVAL, what
        assert (r.nv.value, r.nf.value) == (0, 0) and r.untouched(), what
    for what, vv, ff in (("vertex nan", np.where(np.arange(9).reshape(3, 3) == 4, nan, v), f),
                         ("vertex inf", np.where(np.arange(9).reshape(3, 3) == 8, inf, v), f),
                         ("index out of range", v, [[0, 1, 3]]),
                         ("negative index", v, [[0, -1, 2]])):
        r = _Raw(ctx, vv, ff, origin, cell, dims)
        assert r.status == _ffi.RS_EINVAL and r.untouched(), what
    assert (1 << 9) * (1 << 9) * (1 << 9) == surface.SIMPLIFY_MAX_CELLS


def test_python_argument_errors(ctx):
    v, f, cell, origin = sx.cases()["one_face"]
    nan = float("nan")
    calls = {
        "cell zero": lambda: surface.simplify(v, f, 0.0, ctx=ctx),
        "cell negative": lambda: surface.simplify(v, f, -1.0, ctx=ctx),
        "cell nan": lambda: surface.simplify(v, f, nan, ctx=ctx),
        "cell inf": lambda: surface.simplify(v, f, float("inf"), ctx=ctx),
        "placement": lambda: surface.simplify(v, f, 1.0, placement="median", ctx=ctx),
        "rank_tol 1": lambda: surface.simplify(v, f, 1.0, rank_tol=1.0, ctx=ctx),
        "rank_tol negative": lambda: surface.simplify(v, f, 1.0, rank_tol=-0.1, ctx=ctx),
        "rank_tol nan": lambda: surface.simplify(v, f, 1.0, rank_tol=nan, ctx=ctx),
        "origin nan": lambda: surface.simplify(v, f, 1.0, origin=(0.0, nan, 0.0), ctx=ctx),
        "origin shape": lambda: surface.simplify(v, f, 1.0, origin=(0.0, 0.0), ctx=ctx),
        "vertex below the origin": lambda: surface.simplify(v, f, 1.0, origin=(0.3, 0, 0), ctx=ctx),
        "all below the origin": lambda: surface.simplify(v, f, 1.0, origin=(9.0, 9, 9), ctx=ctx),
        "too many cells": lambda: surface.simplify(v, f, 1e-3, ctx=ctx),
        "vertex nan": lambda: surface.simplify(np.full((3, 3), nan), f, 1.0, ctx=ctx),
        "vertices shape": lambda: surface.simplify(np.zeros((3, 2)), f, 1.0, ctx=ctx),
        "index out of range": lambda: surface.simplify(v, [[0, 1, 3]], 1.0, ctx=ctx),
        "faces shape": lambda: surface.simplify(v, [[0, 1]], 1.0, ctx=ctx),
        "faces dtype": lambda: surface.simplify(v, [[0.0, 1.0, 2.0]], 1.0, ctx=ctx),
    }
    for what, call in calls.items():
        with pytest.raises(ValueError):
            call()
            pytest.fail(what)


# ------------------------------------------------------------------------------------------
# the Python layer
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["two_spheres_3.0", "random_2.0", "unreferenced_vertex"])
def test_drop_unreferenced_is_compact_composed(name, ctx):
    v, f, cell, origin = sx.cases()[name]
    res = sx.reference(name)
    assert ref.unreferenced(res).any()
    kept = surface.simplify(v, f, cell, origin=origin, drop_unreferenced=False, ctx=ctx)
    vo, fo, vmap, info = surface.simplify(v, f, cell, origin=origin, return_info=True, ctx=ctx)
    keep = np.zeros(len(kept[0]), np.uint8)
    keep[kept[1].reshape(-1)] = 1
    cv, cf, cmap = surface.compact(kept[0], kept[1], keep, ctx=ctx)
    _same(vo, cv, "vertices")
    _same(fo, cf, "faces")
    _same(vmap, cmap[kept[2]], "vmap")
    want = ref.drop_unreferenced(res)
    for got, w, what in zip((vo, fo, vmap, info["quadrics"]), want,
                            ("vertices", "faces", "vmap", "quadrics")):
        _same(got, np.asarray(w, dtype=got.dtype), "restated " + what)
    _same(info["fmap"], res["fmap"], "fmap")
    assert info["unreferenced"] == int(ref.unreferenced(res).sum())


def test_reconstruct_simplify(ctx):
    imgs, cams, _ = df.scene("slanted")
    args = (imgs, cams, df.K, df.DEPTHS, sfx.ORIGIN, sfx.VOXEL, sfx.DIMS, sfx.TRUNC)
    kw = {"keep_largest": 1, "iterations": 2}
    plain = surface.reconstruct(*args, min_weight=2, ctx=ctx, clean=kw)
    none = surface.reconstruct(*args, min_weight=2, ctx=ctx, clean=kw, simplify=None)
    for x, y in zip(plain, none):
        _same(x, y, "simplify=None")
    v0, f0 = surface.extract(plain[2], plain[3], sfx.ORIGIN, sfx.VOXEL, min_weight=2, ctx=ctx)
    c = surface.clean(v0, f0, ctx=ctx, **kw)
    for x, y in zip(plain[:2], c[:2]):
        _same(x, y, "clean")
    skw = {"cell": 3.0 * sfx.VOXEL, "placement": "quadric"}
    got = surface.reconstruct(*args, min_weight=2, ctx=ctx, clean=kw, simplify=skw, colors=True)
    want = surface.simplify(c[0], c[1], ctx=ctx, **skw)
    _same(got[0], want[0], "vertices")
    _same(got[1], want[1], "faces")
    _same(got[2], plain[2], "tsdf")
    _same(got[3], plain[3], "weight")
    col = surface.vertex_colors(want[0], want[1], imgs, cams, df.K,
                                normals=surface.vertex_normals(want[0], want[1]), ctx=ctx)[0]
    _same(got[4], col, "colours")
    assert 0 < len(want[1]) < len(c[1]) / 4
    origin, dims = ref.grid(c[0], skw["cell"])
    res = ref.simplify(c[0], c[1], origin, skw["cell"], dims)
    for x, y, what in zip(want, ref.drop_unreferenced(res), ("vertices", "faces", "vmap")):
        _same(x, np.asarray(y, dtype=x.dtype), "restated " + what)
    print(f"reconstruct simplify: {len(c[0])} -> {len(want[0])} vertices, "
          f"{len(c[1])} -> {len(want[1])} faces")


def test_timing(ctx):
    own = _ffi.Context(0)
    try:
        v, f, cell, origin = sx.cases()["two_spheres_1.5"]
        assert all(x == -1.0 for x in surface.simplify_timing(1, ctx=own).values())
        mesh_before = surface.mesh_timing(0, ctx=own)
        plain = surface.simplify(v, f, cell, drop_unreferenced=False, ctx=ctx)
        timed = surface.simplify(v, f, cell, drop_unreferenced=False, ctx=own)
        ms = surface.simplify_timing(0, ctx=own)
        print(ms)
        assert tuple(ms) == surface.SIMPLIFY_STAGES == ("cluster", "rows", "quadric", "faces")
        assert all(np.isfinite(x) and 0.0 < x < 1e3 for x in ms.values())
        assert surface.mesh_timing(0, ctx=own) == mesh_before
        for x, y in zip(plain, timed):
            _same(x, y, "timed")
    finally:
        own.close()
