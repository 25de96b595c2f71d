#!/usr/bin/env python
"""Time the mesh simplification (tsbb15_amd.surface.simplify; csrc/simplify.hip) on the benchmark
mesh of tools/bench_surface.py: the slanted plane fused from 16 views into a 256^3 volume and
extracted with min_weight 2 (378 355 vertices, 754 208 faces), at cells of 2 and 4 voxels.

GPU figures per cell size, after `--warmup` calls: `kernel_ms` is the device time between HIP
events around a slot's kernels (rs_simplify_timing: no upload, no download), `wall_ms` the host
clock around the whole synchronous Python call with ``drop_unreferenced=False`` (one ABI call:
upload, kernels, two waits, download); median, min and max of the timed calls.  `bytes` is what
the slot's passes must read and write at the least, counted from the shapes (pass_bytes below;
gathered re-reads, which the caches serve, the sorts' passes over their rows and atomics are not
counted), `bytes_per_second` that over the kernel time and `copy_rate_fraction` that against the
6.29e12 B/s a float4 copy kernel reaches on the MI355X.

Per cell size also: the output's sizes, the info record, the edges of the output that are not in
exactly two faces (clustering folds the surface; nothing repairs it, no bar), and
``evaluation.compare_meshes`` between output and input in voxels.  Two derived bars are checked
and the tool fails when one is missed: no output vertex is further than sqrt(3) cell from the
input mesh (a vertex and its cluster share a cell), and the result equals the numpy restatement
(tests/simplify_ref.py), run on the whole benchmark mesh, bit for bit; its time is reported for
scale.  Needs a GPU; there is no fallback.  Writes one JSON file (default
profiles/simplify_bench.json) and prints it.
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

import bench_surface  # noqa: E402

COPY_RATE = bench_surface.COPY_RATE
stats = bench_surface.stats


def pass_bytes(nv, nf, ncell, nc, alive, kept):
    """The least traffic of each slot: nv vertices, nf faces, ncell cells of which nc are
    occupied, `alive` faces that are not degenerate, `kept` that survive.  A row build over n
    items into nv buckets is: off and cursor cleared (8 nv), the buckets in (4 n), the scan's item
    in and out twice (16 nv), the buckets and offsets in and the items out (8 n)."""
    rows = lambda n: 8 * nv + 4 * n + 16 * nv + 8 * n  # noqa: E731
    return {
        # cells cleared; keys: vertices in, key and flag out; scan; vmap: key in, vmap and the
        # cluster's key out
        "cluster": 4 * ncell + (24 * nv + 8 * nv) + 16 * ncell + (4 * nv + 4 * nv + 4 * nc),
        # the vertex rows; mean: row in and sorted out, vertices in, mean out; faces: faces and
        # vertices in, plane, three corner buckets, face bucket and two keys out; the corner rows
        "rows": rows(nv) + (8 * nv + 24 * nv + 24 * nc) +
                (12 * nf + 24 * nv + 32 * nf + 12 * nf + 4 * nf + 8 * nf) + rows(3 * nf),
        # rows in and sorted out, planes, mean and key in, quadric and position out
        "quadric": 24 * nf + 32 * nf + 28 * nc + 104 * nc,
        # the face rows; flags cleared; rows in and sorted out, keys in, flags out; scan; emit:
        # faces and offsets in, the kept faces and fmap out
        "faces": rows(nf) + 4 * nf + (8 * alive + 8 * alive + 4 * alive) + 16 * nf +
                 (12 * nf + 4 * nf + 12 * kept + 4 * nf),
    }


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--repeats", type=int, default=10, help="timed GPU calls per cell size")
    ap.add_argument("--warmup", type=int, default=2, help="untimed GPU calls before them")
    ap.add_argument("--size", type=int, nargs=2, default=[576, 720], metavar=("H", "W"))
    ap.add_argument("--views", type=int, default=16)
    ap.add_argument("--side", type=int, default=256, help="nodes per side of the volume")
    ap.add_argument("--cells", type=float, nargs="+", default=[2.0, 4.0], help="in voxels")
    ap.add_argument("--no-reference", action="store_true", help="skip the numpy restatement")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "simplify_bench.json"))
    a = ap.parse_args()

    import dense_fixture as df
    import simplify_ref as ref
    from tsbb15_amd import _ffi, evaluation, surface
    if _ffi.device_count() < 1:
        raise SystemExit("bench_simplify: no GPU visible")
    h, w = a.size
    depth, cams, K = bench_surface.make_scene(df, h, w, a.views)
    origin, voxel, dims, trunc = bench_surface.make_volume(a.side)
    tsdf, weight = surface.integrate(depth, cams, K, origin, voxel, dims, trunc)
    v, f = surface.extract(tsdf, weight, origin, voxel, min_weight=2.0)
    nv, nf = len(v), len(f)
    print(f"bench_simplify: {nv} vertices, {nf} faces, voxel {voxel:.6g}", flush=True)
    res = {"repeats": a.repeats, "warmup": a.warmup, "dims": list(dims), "vertices": nv,
           "faces": nf, "voxel": voxel, "copy_bytes_per_second": COPY_RATE,
           "input_nonmanifold_edges": ref.nonmanifold_edges(f), "cells": {}}
    ok = True
    for cv in a.cells:
        cell = cv * voxel
        gorigin, gdims = surface.simplify_grid(v, cell)
        call = lambda: surface.simplify(v, f, cell, drop_unreferenced=False,  # noqa: E731
                                        return_info=True)
        surface.simplify_timing(1)
        for _ in range(a.warmup):
            out = call()
        wall, kern = [], {k: [] for k in surface.SIMPLIFY_STAGES}
        for _ in range(a.repeats):
            t0 = time.perf_counter()
            out = call()
            wall.append((time.perf_counter() - t0) * 1e3)
            ms = surface.simplify_timing(1)
            for k in kern:
                kern[k].append(ms[k])
        surface.simplify_timing(0)
        vo, fo, vmap, info = out
        counts = {k: info[k] for k in ref.INFO_KEYS + ("unreferenced",)}
        ncell = int(np.prod(gdims))
        need = pass_bytes(nv, nf, ncell, len(vo), nf - info["degenerate_faces"], len(fo))
        slots = {}
        for k in surface.SIMPLIFY_STAGES:
            sec = float(np.median(kern[k])) * 1e-3
            slots[k] = {"kernel_ms": stats(kern[k]), "bytes": need[k],
                        "bytes_per_second": float(f"{need[k] / sec:.4e}"),
                        "copy_rate_fraction": round(need[k] / sec / COPY_RATE, 4)}
        cmp_ = evaluation.compare_meshes(vo, fo, v, f)
        far = float(np.max(cmp_["dist_rec"])) if len(vo) else 0.0
        bound = float(np.sqrt(3.0) * cell)
        moved = float(np.abs(vo[vmap] - v).max())
        entry = {"cell_voxels": cv, "cell": cell, "grid": list(gdims), "grid_cells": ncell,
                 "slots": slots, "wall_ms": stats(wall),
                 "wall_covers": "one ABI call: upload, kernels, two waits, download",
                 "kernel_ms_sum": round(sum(float(np.median(kern[k])) for k in kern), 4),
                 "out_vertices": len(vo), "out_faces": len(fo), "info": counts,
                 "nonmanifold_edges": ref.nonmanifold_edges(fo),
                 "moved_per_axis_max_voxels": moved / voxel,
                 "output_to_input_max_voxels": far / voxel,
                 "bound_sqrt3_cell_voxels": bound / voxel, "within_bound": bool(far <= bound),
                 "accuracy_voxels": float(cmp_["accuracy"]) / voxel,
                 "completeness": float(cmp_["completeness"]),
                 "completeness_threshold_voxels": float(cmp_["threshold"]) / voxel}
        ok = ok and entry["within_bound"]
        if not a.no_reference:
            t0 = time.perf_counter()
            r = ref.simplify(v, f, gorigin, cell, gdims)
            entry["numpy_restatement_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
            entry["restatement_mesh"] = "the whole benchmark mesh"
            same = all(np.array_equal(np.ascontiguousarray(x).view(np.int64)
                                      if x.dtype == np.float64 else x, np.ascontiguousarray(
                                          y).view(np.int64) if y.dtype == np.float64 else y)
                       for x, y in ((vo, r["vertices"]), (fo, r["faces"]), (vmap, r["vmap"]),
                                    (info["fmap"], r["fmap"]), (info["quadrics"], r["quadrics"])))
            entry["bits_equal"] = bool(same and {k: info[k] for k in ref.INFO_KEYS} == r["info"])
            ok = ok and entry["bits_equal"]
        res["cells"][f"{cv:g}"] = entry
        print(f"bench_simplify: cell {cv:g} voxels {entry}", flush=True)

    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(json.dumps(res, sort_keys=True))
    if not ok:
        raise SystemExit("bench_simplify: a derived bar was missed (within_bound, bits_equal)")


if __name__ == "__main__":
    main()
