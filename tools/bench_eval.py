#!/usr/bin/env python
"""Time the evaluation stage's mesh distance (evaluation.mesh_distance, csrc/eval.hip) and the
numpy restatement of the same definitions on this host's CPU.

Inputs: the mesh of tools/bench_texture.py -- the slanted plane of tests/dense_fixture.py in 16
views of 576 x 720, fused into a 256^3 volume, as surface.extract makes it.  Two queries:
  vertices   the mesh's vertices displaced by a seeded noise of half a voxel, against the mesh
  samples    as many surface samples of the mesh (evaluation.sample_surface), against a copy of
             the mesh shifted by half a voxel
GPU figures, after `--warmup` calls: `kernel_ms` is the device time between HIP events around a
stage's kernels (rs_eval_timing: bin, scan, scatter, query; no upload, no download), `wall_ms` the
host clock around the whole synchronous Python call; median, min and max of the timed calls.
`queries_per_second` is over the query kernel alone, `tests_per_query` and `entries_per_face` come
from the call's info.  `bytes_per_test` is what a test reads, 76: the entry's index and the
packed triangle.  `fp64_flops_per_test` counts the routine's adds, multiplies and one division
chain by hand (about 110); the rate over the query kernel is set against the 78.6e12 fp64 flop/s
of the MI355X's vector units.

CPU baseline and check: on the mesh of a `--cpu-side`^3 volume the same query runs with one cell
for the whole mesh (brute force) on the GPU and in tests/eval_ref.py on the CPU, with the
differences.  Needs a GPU; there is no fallback.  Writes one JSON file (default
profiles/eval_bench.json) and prints it.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "tsbb15-3d-reconstruction-project_amd"),
          os.path.join(REPO, "tests"), os.path.join(REPO, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

FP64_RATE = 78.6e12     # flop / s, vector fp64 (FMA counted as two)
FLOPS_PER_TEST = 110
BYTES_PER_TEST = 76


def stats(x):
    return {"median": round(float(np.median(x)), 4), "min": round(float(min(x)), 4),
            "max": round(float(max(x)), 4)}


def make_mesh(df, surface, bs, h, w, V, side):
    """(vertices, faces, voxel) of bench_surface's scene at this size."""
    depth, cams, K = bs.make_scene(df, h, w, V)
    origin, voxel, dims, trunc = bs.make_volume(side)
    tsdf, weight = surface.integrate(depth, cams, K, origin, voxel, dims, trunc)
    v, f = surface.extract(tsdf, weight, origin, voxel, min_weight=2.0)
    return v, f, float(voxel)


def timed(ev, pts, v, f, repeats, warmup, **kw):
    for _ in range(warmup):
        out = ev.mesh_distance(pts, v, f, **kw)
    wall, kern = [], {k: [] for k in ev.STAGES}
    for _ in range(repeats):
        t0 = time.perf_counter()
        out = ev.mesh_distance(pts, v, f, **kw)
        wall.append((time.perf_counter() - t0) * 1e3)
        ms = ev.timing(1)
        for k in kern:
            kern[k].append(ms[k])
    dist, face, _, info = out
    query = float(np.median(kern["query"])) * 1e-3
    n = len(pts)
    return {"queries": n, "kernel_ms": {k: stats(x) for k, x in kern.items()},
            "wall_ms": stats(wall), "cell": float(f"{info['cell']:.6g}"),
            "cells": list(info["cells"]), "entries": info["entries"],
            "entries_per_face": round(info["entries"] / max(len(f), 1), 3),
            "largest_cell": info["largest_cell"], "tests": info["tests"],
            "tests_per_query": round(info["tests"] / n, 2),
            "queries_per_second": float(f"{n / query:.4e}"),
            "tests_per_second": float(f"{info['tests'] / query:.4e}"),
            "fp64_rate_fraction": round(info["tests"] * FLOPS_PER_TEST / query / FP64_RATE, 4),
            "gather_bytes_per_second": float(f"{info['tests'] * BYTES_PER_TEST / query:.4e}"),
            "beyond": info["beyond"], "median_distance": float(f"{np.median(dist):.6g}"),
            "max_distance": float(f"{dist.max():.6g}")}, out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--repeats", type=int, default=10, help="timed GPU calls")
    ap.add_argument("--warmup", type=int, default=2, help="untimed GPU calls before them")
    ap.add_argument("--size", type=int, nargs=2, default=[576, 720], metavar=("H", "W"))
    ap.add_argument("--views", type=int, default=16)
    ap.add_argument("--side", type=int, default=256, help="nodes per side of the volume")
    ap.add_argument("--cpu-side", type=int, default=32)
    ap.add_argument("--cpu-queries", type=int, default=2000)
    ap.add_argument("--cells", type=float, nargs="*", default=[],
                    help="further cell sides to time the vertex query with, in voxels")
    ap.add_argument("--no-reference", action="store_true", help="skip the CPU baseline")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "eval_bench.json"))
    a = ap.parse_args()

    import bench_surface as bs
    import dense_fixture as df
    import eval_ref
    from tsbb15_amd import _ffi, evaluation as ev, surface
    if _ffi.device_count() < 1:
        raise SystemExit("bench_eval: no GPU visible")
    h, w = a.size
    v, f, voxel = make_mesh(df, surface, bs, h, w, a.views, a.side)
    nv, nf = len(v), len(f)
    res = {"repeats": a.repeats, "warmup": a.warmup, "size": [h, w], "views": a.views,
           "side": a.side, "vertices": nv, "faces": nf, "voxel": voxel,
           "library": os.path.basename(os.path.dirname(_ffi.LIB_PATH)),
           "fp64_flops_per_second": FP64_RATE, "fp64_flops_per_test": FLOPS_PER_TEST,
           "bytes_per_test": BYTES_PER_TEST, "gpu": {}}
    print(f"bench_eval: {nv} vertices, {nf} faces, voxel {voxel:.5f}", flush=True)

    rs = np.random.RandomState(0)
    noisy = v + 0.5 * voxel * rs.standard_normal(v.shape)
    shifted = v + 0.5 * voxel * np.array([2.0, -1.0, 2.0]) / 3.0
    t0 = time.perf_counter()
    samples = ev.sample_surface(v, f, nv, seed=0)[0]
    res["sample_surface_seconds"] = round(time.perf_counter() - t0, 4)
    ev.timing(1)
    g = res["gpu"]
    g["vertices"], _ = timed(ev, noisy, v, f, a.repeats, a.warmup)
    g["samples"], _ = timed(ev, samples, shifted, f, a.repeats, a.warmup)
    # the same queries in a seeded random order: what the caller's coherent order is worth
    perm = rs.permutation(nv)
    g["vertices_shuffled"], _ = timed(ev, noisy[perm], v, f, a.repeats, a.warmup)
    for c in a.cells:
        g[f"vertices_cell_{c:g}"], _ = timed(ev, noisy, v, f, a.repeats, a.warmup,
                                             cell=c * voxel)
    for k, val in g.items():
        print(f"bench_eval: {k} {val}", flush=True)

    if not a.no_reference:
        cv, cf, cvox = make_mesh(df, surface, bs, 72, 90, 4, a.cpu_side)
        q = (cv + 0.5 * cvox * rs.standard_normal(cv.shape))[:a.cpu_queries]
        width = float((cv.max(axis=0) - cv.min(axis=0)).max())
        brute, (bd, bface, bclosest, binfo) = timed(ev, q, cv, cf, 3, 1, cell=4.0 * width)
        _, gface, gclosest, ginfo = ev.mesh_distance(q, cv, cf)
        t0 = time.perf_counter()
        rd2, rface, rclosest = eval_ref.mesh_distance(q, cv, cf)
        sec = time.perf_counter() - t0
        res["cpu"] = {"side": a.cpu_side, "vertices": len(cv), "faces": len(cf),
                      "queries": len(q), "tests": len(q) * len(cf), "seconds": round(sec, 4),
                      "cpu_tests_per_second": float(f"{len(q) * len(cf) / sec:.4e}"),
                      "gpu_one_cell": brute,
                      "d2_bit_equal": bool(np.array_equal(binfo["d2"], rd2)),
                      "d2_max_diff": float(f"{np.abs(binfo['d2'] - rd2).max():.3e}"),
                      "faces_differ": int((bface != rface).sum()),
                      "closest_bit_equal": bool(np.array_equal(bclosest, rclosest)),
                      "grid_equals_one_cell": bool(
                          np.array_equal(ginfo["d2"], binfo["d2"]) and
                          np.array_equal(gface, bface) and np.array_equal(gclosest, bclosest))}
        print(f"bench_eval: cpu {res['cpu']}", flush=True)

    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(json.dumps(res, sort_keys=True))


if __name__ == "__main__":
    main()
