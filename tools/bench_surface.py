#!/usr/bin/env python
"""Time the surface stage (tsbb15_amd.surface, csrc/surface.hip): TSDF fusion and mesh extraction,
and the numpy restatement of the same definitions on this host's CPU.

Inputs: the slanted plane of tests/dense_fixture.py rendered with exact depths into 16 views of
576 x 720 (the Dino images' size), fused into a 256^3 volume that the plane crosses; the mesh is
extracted from that volume with min_weight 2.

GPU figures, after `--warmup` calls: `kernel_ms` is the device time between HIP events around a
stage's kernels (rs_surface_timing: no upload, no download), `wall_ms` the host clock around the
whole synchronous Python call -- for `extract` that is both ABI calls, so the volume's second
upload is in it; median, min and max of the timed calls.  `node_views_per_second` = nodes x views
over the integrate kernel time.  For classify, scan and emit `bytes` is what the pass must read
and write at the least, counted from the shapes (pass_bytes below; re-reads of neighbours, which the
caches serve, are not counted), `bytes_per_second` that over the kernel time and
`copy_rate_fraction` that against the 6.29e12 B/s a float4 copy kernel reaches on the MI355X
(8.0e12 B/s is the HBM3E specification).  These passes do a few integer operations per byte: the
bound that applies to them is memory bandwidth.  integrate does some thirty fp64 operations and
two fp64 divisions per node-view on 8 gathered bytes that neighbouring lanes share: its bound is
fp64 arithmetic, and only its rate is reported.

CPU baseline: tests/surface_ref.py (fp64) once at `--cpu-side`^3 with 4 views of 72 x 90, a size it
finishes in seconds, with the same rates.  Needs a GPU; there is no fallback.  Writes one JSON
file (default profiles/surface_bench.json) and prints it.
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

COPY_RATE = 6.29e12   # bytes / s, a float4 copy kernel over HBM3E


def stats(x):
    return {"median": round(float(np.median(x)), 4), "min": round(float(min(x)), 4),
            "max": round(float(max(x)), 4)}


def pass_bytes(n, nv, nf):
    """The least traffic of each extraction pass for n nodes, nv vertices and nf faces."""
    return {
        # cells: tsdf + weight in, flag out; nodes: tsdf + flag in, mask out
        "classify": n * (4 + 4 + 1) + n * (4 + 1 + 1),
        # per count array: bytes in and offsets out, then offsets in and out again for the add
        "scan": 2 * n * (1 + 4 + 4 + 4),
        # vertices: tsdf + mask + base in, 3 doubles a vertex out; faces: flag + base in,
        # 3 int32 a face out
        "emit": n * (4 + 1 + 4) + 24 * nv + n * (1 + 4) + 12 * nf,
    }


def make_scene(df, h, w, V):
    """V views of the slanted plane with exact depths: the fixture's three cameras and more on a
    ring around the first."""
    f = 60.0 * w / df.W
    K = np.array([[f, 0.0, (w - 1) / 2.0], [0.0, f, (h - 1) / 2.0], [0.0, 0.0, 1.0]])
    cams = list(df.cameras())
    for v in range(3, V):
        a = 2.0 * np.pi * (v - 3) / max(V - 3, 1)
        cams.append(df.camera((0.5 * np.cos(a), 0.35 * np.sin(a), 0.02 * np.sin(3 * a)),
                              (np.sin(a), np.cos(a), 0.0), 0.05))
    cams = np.array(cams[:V])
    depth = np.array([df.render(C, df.SLANTED, h, w, K)[1] for C in cams])
    return depth, cams, K


def make_volume(side, extent=3.0):
    """(origin, voxel, dims, trunc): a cube of `extent` world units around the plane's centre."""
    voxel = extent / (side - 1)
    origin = np.array([-extent / 2.0, -extent / 2.0, np.sqrt(18.0) - extent / 2.0])
    return origin, voxel, (side, side, side), 5.0 * voxel


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--repeats", type=int, default=10, help="timed GPU calls per stage")
    ap.add_argument("--warmup", type=int, default=2, help="untimed GPU calls before them")
    ap.add_argument("--size", type=int, nargs=2, default=[576, 720], metavar=("H", "W"))
    ap.add_argument("--views", type=int, default=16)
    ap.add_argument("--side", type=int, default=256, help="nodes per side of the volume")
    ap.add_argument("--cpu-side", type=int, default=128)
    ap.add_argument("--no-reference", action="store_true", help="skip the CPU baseline")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "surface_bench.json"))
    a = ap.parse_args()

    import dense_fixture as df
    import surface_ref as sr
    from tsbb15_amd import _ffi, surface
    if _ffi.device_count() < 1:
        raise SystemExit("bench_surface: no GPU visible")
    surface.timing(1)
    h, w = a.size
    depth, cams, K = make_scene(df, h, w, a.views)
    origin, voxel, dims, trunc = make_volume(a.side)
    n = dims[0] * dims[1] * dims[2]
    res = {"repeats": a.repeats, "warmup": a.warmup, "size": [h, w], "views": a.views,
           "dims": list(dims), "nodes": n, "copy_bytes_per_second": COPY_RATE, "gpu": {}}

    fuse = lambda: surface.integrate(depth, cams, K, origin, voxel, dims, trunc)
    for _ in range(a.warmup):
        tsdf, weight = fuse()
    wall, kern = [], []
    for _ in range(a.repeats):
        t0 = time.perf_counter()
        tsdf, weight = fuse()
        wall.append((time.perf_counter() - t0) * 1e3)
        kern.append(surface.timing(1)["integrate"])
    sec = float(np.median(kern)) * 1e-3
    res["gpu"]["integrate"] = {
        "kernel_ms": stats(kern), "wall_ms": stats(wall), "node_views": n * a.views,
        "node_views_per_second": float(f"{n * a.views / sec:.4e}"),
        "observed_nodes": int((weight > 0).sum()), "bound": "fp64 arithmetic"}
    print(f"bench_surface: integrate {res['gpu']['integrate']}", flush=True)

    mesh = lambda: surface.extract(tsdf, weight, origin, voxel, min_weight=2.0)
    for _ in range(a.warmup):
        v, f = mesh()
    wall, kern = [], {k: [] for k in surface.STAGES[1:]}
    for _ in range(a.repeats):
        t0 = time.perf_counter()
        v, f = mesh()
        wall.append((time.perf_counter() - t0) * 1e3)
        ms = surface.timing(1)
        for k in kern:
            kern[k].append(ms[k])
    need = pass_bytes(n, len(v), len(f))
    res["gpu"]["extract"] = {"wall_ms": stats(wall), "vertices": len(v), "faces": len(f),
                             "wall_covers": "both ABI calls: sizes, then the mesh"}
    for k in kern:
        sec = float(np.median(kern[k])) * 1e-3
        res["gpu"][k] = {"kernel_ms": stats(kern[k]), "bytes": need[k],
                         "bytes_per_second": float(f"{need[k] / sec:.4e}"),
                         "copy_rate_fraction": round(need[k] / sec / COPY_RATE, 4),
                         "bound": "memory bandwidth"}
        print(f"bench_surface: {k} {res['gpu'][k]}", flush=True)
    print(f"bench_surface: extract {res['gpu']['extract']}", flush=True)

    if not a.no_reference:
        cd, cc, cK = make_scene(df, 72, 90, 4)
        co, cv, cdims, ct = make_volume(a.cpu_side)
        cn = cdims[0] * cdims[1] * cdims[2]
        t0 = time.perf_counter()
        rt, rw = sr.integrate(cd, cc, cK, co, cv, cdims, ct)
        t1 = time.perf_counter()
        rv, rf = sr.extract(rt, rw, co, cv, 2.0)
        t2 = time.perf_counter()
        gt, gw = surface.integrate(cd, cc, cK, co, cv, cdims, ct)
        gv, gf = surface.extract(gt, gw, co, cv, min_weight=2.0)
        both = ~np.isnan(rt) & ~np.isnan(gt)
        res["cpu"] = {"dims": list(cdims), "views": 4, "size": [72, 90],
                      "integrate_seconds": round(t1 - t0, 4),
                      "cpu_node_views_per_second": float(f"{cn * 4 / (t1 - t0):.4e}"),
                      "extract_seconds": round(t2 - t1, 4),
                      "cpu_extract_nodes_per_second": float(f"{cn / (t2 - t1):.4e}"),
                      "vertices": len(rv), "faces": len(rf),
                      "weight_equal": bool(np.array_equal(rw, gw)),
                      "tsdf_max_diff": float(f"{np.abs(rt[both] - gt[both]).max():.3e}"),
                      "mesh_sizes_equal": bool(len(gv) == len(rv) and len(gf) == len(rf))}
        print(f"bench_surface: cpu {res['cpu']}", flush=True)

    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(json.dumps(res, sort_keys=True))


if __name__ == "__main__":
    main()
