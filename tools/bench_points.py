#!/usr/bin/env python
"""Time the surface from oriented points (tsbb15_amd.surface.points_volume; csrc/cloud_knn.hip)
stage by stage, and the route a caller had before it: cloud.knn with the nodes as queries.

Inputs: the noisy unit sphere of tests/cloud_fixture.py at n = 1e5 and 1e6 with normals p / |p|;
volumes of 128^3 and 256^3 nodes over [-1.05, 1.05]^3; radius = 3 voxels; k = 8, 16, 32.  A sweep
of the cell from 0.5 to 2 times the radius (the default is the radius times 1 + 2^-19) on the 1e6
sphere, 128^3, k = 16.

GPU figures, after `--warmup` calls: `kernel_ms` per stage is the device time between HIP events
(rs_surface_points_timing: box, grid, scan, scatter, field; no upload, no download), `wall_ms` the
host clock around the whole synchronous call (upload, kernels, download of the two volumes, the
Python shim); median, min and max of `--repeats` timed calls.  `tested_per_node` is info.tested /
nodes, `defined` and `saturated` are the info's counts, `nodes_per_second` and `tests_per_second`
are over the field stage.

The unfused route, on the 128^3 volumes: cloud.knn(pts, k, queries=nodes, max_dist=radius), the
same walk, which writes and downloads 12 k + 4 bytes per node where the fused call writes 8.  Timed
the same way (rs_cloud_knn_timing).  `fused_over_knn` is the ratio of the medians, for the wall
clocks and for the sums of the kernel stages; `knn_spread` is (max - min) / median of the knn
call's wall clock, the margin `not_slower` allows.  The numpy slot loop that the route still needs
after the lists is not timed: the comparison is with the knn call alone.

Needs a GPU; there is no fallback.  Writes one JSON file (default profiles/points_bench.json) and
prints it.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "tsbb15-3d-reconstruction-project_amd"),
          os.path.join(REPO, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

STAGES = ("box", "grid", "scan", "scatter", "field")
KNN_STAGES = ("box", "grid", "scan", "scatter", "query")
HALF = 1.05


def stats(x):
    return {"median": round(float(np.median(x)), 4), "min": round(float(min(x)), 4),
            "max": round(float(max(x)), 4)}


def timed(fn, timing, stages, warmup, repeats):
    """fn() -> (..., info) timed; returns (info, wall stats, kernel stats per stage)."""
    for _ in range(warmup):
        out = fn()
    wall, kern = [], {s: [] for s in stages}
    for _ in range(repeats):
        t0 = time.perf_counter()
        out = fn()
        wall.append((time.perf_counter() - t0) * 1e3)
        ms = timing(1)
        for s in stages:
            kern[s].append(ms[s])
    return out[-1], stats(wall), {s: stats(v) for s, v in kern.items()}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--warmup", type=int, default=2, help="untimed GPU calls before the timed")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--sizes", type=int, nargs="+", default=[100000, 1000000])
    ap.add_argument("--sides", type=int, nargs="+", default=[128, 256])
    ap.add_argument("--ks", type=int, nargs="+", default=[8, 16, 32])
    ap.add_argument("--no-knn", action="store_true", help="skip the unfused route")
    ap.add_argument("--no-sweep", action="store_true", help="skip the cell sweep")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "points_bench.json"))
    a = ap.parse_args()

    import cloud_fixture as cf
    import surface_ref as sr
    from tsbb15_amd import _ffi, cloud, surface
    if _ffi.device_count() < 1:
        raise SystemExit("bench_points: no GPU visible")
    surface.points_timing(1)
    cloud.knn_timing(1)
    res = {"warmup": a.warmup, "repeats": a.repeats,
           "library": os.path.relpath(_ffi.LIB_PATH, REPO), "volume": {}, "unfused": {}}
    origin = np.full(3, -HALF)

    def volume(pts, nrm, side, k, cell=None):
        voxel = 2.0 * HALF / (side - 1)
        info, wall, kern = timed(
            lambda: surface.points_volume(pts, nrm, origin, voxel, (side,) * 3, 3.0 * voxel, k=k,
                                          cell=cell, return_info=True),
            surface.points_timing, STAGES, a.warmup, a.repeats)
        nodes, sec = side ** 3, kern["field"]["median"] * 1e-3
        return {"n": len(pts), "side": side, "k": k, "voxel": voxel, "radius": 3.0 * voxel,
                "info": info, "wall_ms": wall, "kernel_ms": kern,
                "kernels_ms": round(sum(v["median"] for v in kern.values()), 4),
                "tested_per_node": round(info["tested"] / nodes, 1),
                "defined": info["defined"], "saturated": info["saturated"],
                "nodes_per_second": float(f"{nodes / sec:.3e}"),
                "tests_per_second": float(f"{info['tested'] / sec:.3e}")}

    clouds = {}
    for n in a.sizes:
        pts = cf.sphere(n)
        clouds[n] = (pts, pts / np.linalg.norm(pts, axis=1, keepdims=True))
    for n, (pts, nrm) in clouds.items():
        for side in a.sides:
            for k in a.ks:
                name = f"sphere_{n}_side{side}_k{k}"
                r = res["volume"][name] = volume(pts, nrm, side, k)
                print(f"bench_points: {name}: field {r['kernel_ms']['field']}, wall "
                      f"{r['wall_ms']}, tested/node {r['tested_per_node']}, defined "
                      f"{r['defined']}, saturated {r['saturated']}", flush=True)

    if not a.no_knn:
        side = min(a.sides)
        voxel = 2.0 * HALF / (side - 1)
        nodes = np.ascontiguousarray(sr.node_positions(origin, voxel, (side,) * 3).reshape(-1, 3))
        for n, (pts, nrm) in clouds.items():
            for k in a.ks:
                name = f"sphere_{n}_side{side}_k{k}"
                info, wall, kern = timed(
                    lambda: cloud.knn(pts, k, queries=nodes, max_dist=3.0 * voxel,
                                      cell=3.0 * voxel * (1.0 + 2.0 ** -19)),
                    cloud.knn_timing, KNN_STAGES, a.warmup, a.repeats)
                fused = res["volume"][name]
                kernels = round(sum(v["median"] for v in kern.values()), 4)
                spread = (wall["max"] - wall["min"]) / wall["median"]
                ratio = fused["wall_ms"]["median"] / wall["median"]
                res["unfused"][name] = {
                    "knn_wall_ms": wall, "knn_kernel_ms": kern, "knn_kernels_ms": kernels,
                    "knn_tested": info["tested"], "fused_tested": fused["info"]["tested"],
                    "fused_wall_ms": fused["wall_ms"], "fused_kernels_ms": fused["kernels_ms"],
                    "knn_spread": round(spread, 4),
                    "fused_over_knn": {"wall": round(ratio, 4),
                                       "kernels": round(fused["kernels_ms"] / kernels, 4)},
                    "not_slower": bool(ratio <= 1.0 + spread)}
                print(f"bench_points: unfused {name}: {res['unfused'][name]}", flush=True)

    if not a.no_sweep:
        n, side, k = max(a.sizes), min(a.sides), 16
        pts, nrm = clouds[n]
        radius = 3.0 * 2.0 * HALF / (side - 1)
        res["cell_sweep"] = {"n": n, "side": side, "k": k, "radius": radius, "rows": []}
        for f in (0.5, 0.7, 1.0, 1.0 + 2.0 ** -19, 1.2, 1.4, 2.0):
            r = volume(pts, nrm, side, k, cell=f * radius)
            row = {"factor": f, "cell": f * radius, "cells": r["info"]["cells"],
                   "largest_cell": r["info"]["largest_cell"],
                   "tested_per_node": r["tested_per_node"], "field_ms": r["kernel_ms"]["field"],
                   "build_ms": round(sum(r["kernel_ms"][s]["median"]
                                         for s in ("box", "grid", "scan", "scatter")), 4),
                   "wall_ms": r["wall_ms"]}
            res["cell_sweep"]["rows"].append(row)
            print(f"bench_points: sweep {row}", flush=True)

    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(res, sort_keys=True))


if __name__ == "__main__":
    main()
