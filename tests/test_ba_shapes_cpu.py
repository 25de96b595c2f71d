"""Which branches of k_ba_chol, k_ba_final, k_ba_step and k_ba_schur (csrc/ba.hip) the large rings
of tests/test_gpu_ba_large.py execute.  No GPU: the loop schedule of k_ba_chol is restated below
from the constants read out of ba.hip and the header, and every named camera count must reach the
branch it is named for while its neighbour below must not.  Retuning kBaCholTile, kBaCholThreads,
kBaCholRows or kBaFinalThreads then fails here instead of moving the GPU tests off their edges.

With the shipped constants (tile 240, 512 threads, 2 rows per thread, block columns of 12):

  model     cameras  N     what it is the smallest for (below: the neighbour stays out)
  12-param  22       252   the last block column starts at c0 = 240: one pass, a full tile
  12-param  23       264   c0 = 252: a second pass over the LDS tile, 12 columns wide
  rigid     43       252   one pass, a full tile (42 free cameras, no pad)
  rigid     44       264   the second pass, and half a block column of identity pad
  12-param  45       528   a second panel row per thread (5 lanes hold one), a third tile pass,
                           rows, ys[] and cam_of_slot beyond lane 512 in the backward solve
  rigid     88       528   the same with 522 real columns and a pad
  12-param  88       1044  the second iteration of the loop over `base`; 12 nC = 1056 camera
                           entries in k_ba_final, more than its 1024 threads
  both      128      1524 / 768   the cap: ys[] used to 1524 of 1536 doubles, 8128 pair blocks

The same file pins the fixtures those tests run on (ba_rigid_fixture.large_ring).
"""
import os
import re

import numpy as np
import pytest

import ba_fixture as bf
import ba_rigid_fixture as rf
from conftest import REPO
from tsbb15_amd import _ffi

BA_HIP = os.path.join(REPO, "tsbb15-3d-reconstruction-project_amd", "csrc", "ba.hip")
NAMES = ("kBaCholTile", "kBaCholThreads", "kBaCholRows", "kBaFinalThreads")


def constants(ba_hip=BA_HIP, header=_ffi.HEADER_PATH):
    """The constants of the schedule, from the sources."""
    src, hdr = open(ba_hip).read(), open(header).read()
    K = {}
    for name in NAMES:
        found = re.findall(r"constexpr int %s = (\d+);" % name, src)
        assert len(found) == 1, name
        K[name] = int(found[0])
    found = re.findall(r"^#define RS_BA_RIGID_BW (\d+)$", src, re.M)
    assert len(found) == 1
    K["RS_BA_RIGID_BW"] = int(found[0])
    found = re.findall(r"^#define RS_BA_MAX_CAMERAS (\d+)\b", hdr, re.M)
    assert len(found) == 1
    K["RS_BA_MAX_CAMERAS"] = int(found[0])
    # ys[] of k_ba_chol is sized by the cap
    assert "constexpr int kBaMaxFree = RS_BA_MAX_CAMERAS;" in src
    assert "__shared__ double ys[12 * kBaMaxFree];" in src
    return K


def schedule(K, D, nC):
    """What k_ba_chol<D, BW> does for nC cameras, all observed (nC - 1 free): the loops over k,
    m0 and base of the kernel with their bounds, nothing else."""
    tile, threads, rows = K["kBaCholTile"], K["kBaCholThreads"], K["kBaCholRows"]
    BW = 12 if D == 12 else K["RS_BA_RIGID_BW"]
    nreal = D * (nC - 1)
    N = (nreal + BW - 1) // BW * BW
    R, nb = N + 1, N // BW
    out = dict(N=N, nreal=nreal, pad=N - nreal, passes=0, last_mc=0, nq=0, second_rows=0, bases=0)
    for k in range(nb):
        c0 = BW * k
        m0s = list(range(0, c0, tile))
        out["passes"] = max(out["passes"], len(m0s))
        if k == nb - 1 and m0s:
            out["last_mc"] = min(tile, c0 - m0s[-1])
        if not m0s:
            continue
        bases = list(range(c0, R, threads * rows))
        out["bases"] = max(out["bases"], len(bases))
        for base in bases:
            nq = min(rows, (R - base + threads - 1) // threads)
            out["nq"] = max(out["nq"], nq)
            if nq == 2:
                # lanes whose row base + threads + tid exists; the others clamp to R - 1
                out["second_rows"] = max(out["second_rows"], min(threads, R - base - threads))
    return out


K = constants()


def test_constants_are_the_shipped_ones_and_the_cap_fits():
    assert K["RS_BA_MAX_CAMERAS"] == _ffi.BA_MAX_CAMERAS == 128
    assert K["RS_BA_RIGID_BW"] == 12 and K["kBaCholRows"] == 2
    assert K["kBaCholTile"] % 12 == 0
    top = schedule(K, 12, K["RS_BA_MAX_CAMERAS"])
    assert top["N"] == 1524 <= 12 * K["RS_BA_MAX_CAMERAS"] == 1536
    # Ts[], D[], ys[] and the flag of k_ba_chol: 36.5 KB of the 64 KB a workgroup may declare
    lds = 8 * (K["kBaCholTile"] * 12 + 144 + 12 * K["RS_BA_MAX_CAMERAS"]) + 4
    assert lds == 36484 and lds <= 65536
    # the schedule never needs a third row per thread or a third `base` iteration
    assert top["nq"] == 2 == K["kBaCholRows"] and top["bases"] == 2
    assert max(rf.LARGE_FREE12) == max(rf.LARGE_RIGID) == K["RS_BA_MAX_CAMERAS"]


def test_tile_passes_22_against_23_and_43_against_44():
    tile = K["kBaCholTile"]
    for D, below, at in ((12, 22, 23), (6, 43, 44)):
        a, b = schedule(K, D, below), schedule(K, D, at)
        # the boundary from below: exactly one pass, over a full tile
        assert (a["N"], a["passes"], a["last_mc"]) == (tile + 12, 1, tile)
        # one block column more: a second pass, a partial tile
        assert (b["N"], b["passes"], b["last_mc"]) == (tile + 24, 2, 12)
        assert a["nq"] == b["nq"] == 1 and a["bases"] == b["bases"] == 1
    assert schedule(K, 6, 43)["pad"] == 0 and schedule(K, 6, 44)["pad"] == 6
    # the ring of test_gpu_ba_rigid.py: 246 columns padded to 252, the last block column starts
    # exactly at the tile's end, one pass
    ring = schedule(K, 6, 42)
    assert (ring["nreal"], ring["N"], ring["passes"], ring["last_mc"]) == (246, 252, 1, tile)


def test_second_row_per_thread_44_against_45_and_87_against_88():
    threads = K["kBaCholThreads"]
    for D, below, at in ((12, 44, 45), (6, 87, 88)):
        a, b = schedule(K, D, below), schedule(K, D, at)
        assert a["nq"] == 1 and a["second_rows"] == 0
        assert b["nq"] == 2 and b["N"] == 528
        # R - c0 - threads at c0 = 12: five lanes hold a second row, the others clamp to R - 1
        assert b["second_rows"] == 5 < threads
        assert a["bases"] == b["bases"] == 1
        # a third pass over the tile, and lanes >= 512 in the backward solve, ys[] and the scatter
        assert b["passes"] == 3 and b["last_mc"] == 516 - 2 * K["kBaCholTile"]
        assert b["nreal"] > threads
    assert schedule(K, 6, 88)["pad"] == 6 and schedule(K, 6, 87)["pad"] == 0
    # N > 512 alone is first reached two cameras earlier
    assert schedule(K, 12, 43)["N"] <= threads < schedule(K, 12, 44)["N"]


def test_second_base_iteration_87_against_88():
    a, b = schedule(K, 12, 87), schedule(K, 12, 88)
    assert a["bases"] == 1 and b["bases"] == 2 and b["N"] == 1044
    assert b["passes"] == 5 and b["nq"] == 2 and b["second_rows"] == K["kBaCholThreads"]
    # the rigid model never gets there
    assert schedule(K, 6, K["RS_BA_MAX_CAMERAS"])["bases"] == 1
    assert schedule(K, 6, K["RS_BA_MAX_CAMERAS"])["N"] == 768


def test_final_and_step_lanes():
    ft = K["kBaFinalThreads"]
    # k_ba_final<12>: the strided loop over 12 nC camera entries wraps from 86 cameras on
    assert 12 * 85 <= ft < 12 * 86 <= 12 * 88
    assert 6 * K["RS_BA_MAX_CAMERAS"] <= ft
    # k_ba_step<12> (256 lanes a workgroup): camera lanes in [nP, 12 nC) in a second workgroup
    for nC in rf.LARGE_FREE12:
        assert 12 * nC > 256 and 12 * nC > rf.LARGE_RINGS[nC][0]


@pytest.mark.parametrize("nC", sorted(rf.LARGE_RINGS))
def test_large_ring_fixture(nC):
    nP, n = rf.LARGE_RINGS[nC]
    P = rf.large_ring(nC)
    ov, op, uv = P["ov"], P["op"], P["uv"]
    assert len(ov) == len(op) == len(uv) == n and len(P["cams"]) == nC and len(P["pts"]) == nP
    assert np.array_equal(np.unique(ov), np.arange(nC))          # every camera observed
    assert rf.depths(P).min() > 0.2
    assert np.array_equal(P["cams"][0], np.hstack([np.eye(3), np.zeros((3, 1))]))
    assert rf.rotation_defect(P["cams"]) < 1e-14
    # point j has 2 + j % (nC - 1) observations, so every track length 2 .. nC occurs
    track = np.bincount(op, minlength=nP)
    assert np.array_equal(track, 2 + np.arange(nP) % (nC - 1))
    lengths, count = np.unique(track, return_counts=True)
    assert np.array_equal(lengths, np.arange(2, nC + 1))
    extra = nP - (nC - 1)                                        # lengths that occur twice
    assert np.array_equal(count, np.where(np.arange(nC - 1) < extra, 2, 1))
    # no observation twice
    assert len(np.unique(ov.astype(np.int64) * nP + op)) == n


def test_ring_of_42_is_unchanged():
    P = rf.ring_problem(42, 60)
    assert len(P["ov"]) == 1111 and len(np.unique(P["ov"])) == 42
    assert np.array_equal(np.sort(P["op"]), bf.sparse_tracks(42, 60)[1])


def _shared_points(P):
    """Per pair a <= b of free cameras, in k_ba_schur's block order, the points both see."""
    nC = len(P["cams"])
    seen = np.zeros((nC, len(P["pts"])), np.int64)
    seen[P["ov"], P["op"]] = 1
    return (seen[1:] @ seen[1:].T)[np.triu_indices(nC - 1)]


def test_pair_blocks():
    """k_ba_schur runs one workgroup per pair of free cameras a <= b: 8128 at 128 cameras.  The
    rings have tracks of every length up to nC, so no pair list is empty there and the longest
    needs more than one LDS tile of 32 pairs; the short-track ring is the opposite, 7624 of its
    8128 lists are empty (S_ab = 0)."""
    for nC, blocks in ((128, 8128), (88, 3828)):
        co = _shared_points(rf.large_ring(nC))
        assert len(co) == blocks and co.min() >= 1 and co.max() > 32
    P = rf.short_track_ring(128)
    assert len(P["ov"]) == 514 and np.array_equal(np.unique(P["ov"]), np.arange(128))
    assert np.bincount(P["op"]).min() == 2 and np.bincount(P["op"]).max() == 4
    co = _shared_points(P)
    empty = int((co == 0).sum())
    print(f"short-track ring, 128 cameras: {len(co)} pair blocks, {empty} empty")
    # pairs at most 3 apart along the chain share a point, and (126, 1), (127, 1) across camera 0
    assert len(co) == 8128 and empty == 8128 - (127 + 126 + 125 + 124) - 2 == 7624
