"""The bundle-adjustment surface that needs no GPU: the ABI record, the binding, the argument
checks made before any device call, and the test fixture's own bookkeeping."""
import ctypes
import inspect

import numpy as np
import pytest

import ba_fixture as bf
from oracle import tables_ref as tr
from tsbb15_amd import _ffi
from tsbb15_amd import tables as gt


def test_ba_info_layout_and_binding():
    assert ctypes.sizeof(_ffi.BaInfo) == 40
    assert [f[0] for f in _ffi.BaInfo._fields_][:3] == ["cost_init", "cost", "lam"]
    lib = ctypes.CDLL(_ffi.LIB_PATH)
    for name in ("rs_bundle_adjust", "rs_ba_timing"):
        assert hasattr(lib, name) and name in _ffi._SIGS
    src = open(_ffi.HEADER_PATH).read()
    assert "rs_bundle_adjust(" in src and "RS_BA_MAX_CAMERAS %d" % _ffi.BA_MAX_CAMERAS in src
    assert len(_ffi.BA_KERNELS) == 8 and "#define RS_BA_TIMING_SLOTS 8" in src


def test_python_signatures():
    p = inspect.signature(gt.bundle_adjust).parameters
    assert list(p) == ["cams", "pts", "obs_view", "obs_point", "uv", "max_iter", "ftol", "ctx"]
    assert (p["max_iter"].default, p["ftol"].default, p["ctx"].default) == (200, 1e-15, None)
    p = inspect.signature(gt.BundleAdjustment2).parameters
    assert list(p) == ["T", "max_iter", "ftol", "ctx"]
    assert (p["max_iter"].default, p["ftol"].default) == (200, 1e-15)


def test_length_checks_need_no_device():
    P = bf.problem(5, 40)
    with pytest.raises(ValueError):
        gt.bundle_adjust(P["cams"], P["pts"], P["ov"][:-1], P["op"], P["uv"])
    with pytest.raises(ValueError):
        gt.bundle_adjust(P["cams"], P["pts"], P["ov"], P["op"], P["uv"][:-1])
    with pytest.raises(ValueError):
        gt.bundle_adjust(P["cams"], P["pts"], P["ov"][:0], P["op"][:0], P["uv"][:0])


def test_fixture_sizes_and_scene():
    for (nC, nP), n in (((5, 40), 140), ((7, 70), 311)):
        P = bf.problem(nC, nP)
        assert len(P["ov"]) == len(P["op"]) == len(P["uv"]) == n
        assert np.array_equal(P["cams"][0], np.hstack([np.eye(3), np.zeros((3, 1))]))
        track = np.bincount(P["op"], minlength=nP)
        assert np.array_equal(track, 2 + np.arange(nP) % (nC - 1))
        # noise of 1e-4 per coordinate: cost at the truth ~ n * 1e-8
        r = tr.ba_residuals(P["cams"], P["pts"], P["ov"], P["op"], P["uv"][:, 0], P["uv"][:, 1])
        assert 0.2 * n * 1e-8 < 0.5 * r @ r < 3 * n * 1e-8
    assert len(bf.problem(3, 676, full=True)["ov"]) == 2028
