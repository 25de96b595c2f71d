#!/usr/bin/env python
"""Time the k-NN calls of the point-cloud stage (tsbb15_amd.cloud.knn, knn_normals,
knn_mean_dist; csrc/cloud_knn.hip) stage by stage, and scipy's kd-tree on this host's CPU.

Inputs: the reference's own Dino cloud (tests/golden/cloud.npz, 688 points) at k = 15, its k0;
the noisy unit sphere of tests/cloud_fixture.py at n = 1e5 and 1e6 with k = 8, 16, 32, 64; the
1e6 sphere in a seeded random order; as many external queries (the sphere's points displaced by
a seeded noise of 0.01) in the caller's order and shuffled; a sweep of the cell at 1e6 points and
k = 16 (G = 0.5, 0.7, 1, 1.4 and 2 times the default's round(cbrt(n))).

GPU figures, after `--warmup` calls: `kernel_ms` per stage is the device time between HIP events
(rs_cloud_knn_timing: box, grid, scan, scatter, query, and normals or mean_dist for the
consumers; no upload, no download), `wall_ms` the host clock around the whole synchronous call
(upload, kernels, download of the lists, the Python shim); median, min and max of 20 (Dino), 10
(1e5) or 5 (1e6) timed calls.  `tested_per_query` is info.tested / m, `queries_per_second` and
`tests_per_second` are over the query stage, `gathered_bytes_per_second` counts the 24 bytes of
a packed point per test.

CPU baseline, one run each: scipy.spatial.cKDTree(pts).query(pts, k, workers=threads), tree
construction included; `lists_equal` compares its index lists with the GPU's.  Needs a GPU; there
is no fallback.  Writes one JSON file (default profiles/knn_bench.json) and prints it.
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

STAGES = ("box", "grid", "scan", "scatter", "query", "normals", "mean_dist")


def stats(x):
    return {"median": round(float(np.median(x)), 4), "min": round(float(min(x)), 4),
            "max": round(float(max(x)), 4)}


def timed(cloud, fn, m, warmup, repeats, used=STAGES[:5]):
    """fn() -> (..., info) timed; returns (last output, figures)."""
    for _ in range(warmup):
        out = fn()
    wall, kern = [], {s: [] for s in used}
    for _ in range(repeats):
        t0 = time.perf_counter()
        out = fn()
        wall.append((time.perf_counter() - t0) * 1e3)
        ms = cloud.knn_timing(1)
        for s in used:
            kern[s].append(ms[s])
    info = out[-1]
    res = {"m": m, "repeats": repeats, "info": info, "wall_ms": stats(wall),
           "kernel_ms": {s: stats(v) for s, v in kern.items()},
           "tested_per_query": round(info["tested"] / m, 1)}
    sec = res["kernel_ms"]["query"]["median"] * 1e-3
    res["queries_per_second"] = float(f"{m / sec:.3e}")
    res["tests_per_second"] = float(f"{info['tested'] / sec:.3e}")
    res["gathered_bytes_per_second"] = float(f"{24 * info['tested'] / sec:.3e}")
    return out, res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--warmup", type=int, default=2, help="untimed GPU calls before the timed")
    ap.add_argument("--sizes", type=int, nargs="+", default=[100000, 1000000])
    ap.add_argument("--ks", type=int, nargs="+", default=[8, 16, 32, 64])
    ap.add_argument("--threads", type=int, default=16, help="CPU baseline threads")
    ap.add_argument("--no-reference", action="store_true", help="skip the CPU baseline")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "knn_bench.json"))
    a = ap.parse_args()

    import cloud_fixture as cf
    from tsbb15_amd import _ffi, cloud
    if _ffi.device_count() < 1:
        raise SystemExit("bench_knn: no GPU visible")
    cloud.knn_timing(1)
    res = {"warmup": a.warmup, "cpu_threads": a.threads, "gpu": {}, "cpu": {}}
    g = res["gpu"]

    def reps(n):
        return 20 if n < 10000 else (10 if n <= 200000 else 5)

    def show(name):
        r = g[name]
        print(f"bench_knn: {name}: query {r['kernel_ms']['query']}, wall {r['wall_ms']}, "
              f"tested/query {r['tested_per_query']}, tests/s {r['tests_per_second']:.2e}",
              flush=True)

    clouds = {"dino_688": np.array(cf.dino()["points"])}
    for n in a.sizes:
        clouds[f"sphere_{n}"] = cf.sphere(n)
    lists = {}
    for cname, pts in clouds.items():
        for k in ([15] if cname.startswith("dino") else a.ks):
            name = f"{cname}_k{k}"
            out, g[name] = timed(cloud, lambda: cloud.knn(pts, k), len(pts), a.warmup,
                                 reps(len(pts)))
            lists[name] = out[0]
            show(name)

    big = max(a.sizes)
    pts = clouds[f"sphere_{big}"]
    rng = np.random.default_rng(3)
    shuffled = pts[rng.permutation(big)]
    name = f"sphere_{big}_k16_shuffled"
    _, g[name] = timed(cloud, lambda: cloud.knn(shuffled, 16), big, a.warmup, reps(big))
    show(name)
    Q = pts + 0.01 * rng.standard_normal(pts.shape)
    for tag, q in (("external", Q), ("external_shuffled", Q[rng.permutation(big)])):
        name = f"sphere_{big}_k16_{tag}"
        _, g[name] = timed(cloud, lambda: cloud.knn(pts, 16, queries=q), big, a.warmup, reps(big))
        show(name)
    name = f"sphere_{big}_k16_normals"
    _, g[name] = timed(cloud, lambda: cloud.knn_normals(pts, 16), big, a.warmup, reps(big),
                       STAGES[:6])
    show(name)
    name = f"sphere_{big}_k16_mean_dist"
    _, g[name] = timed(cloud, lambda: cloud.knn_mean_dist(pts, 16), big, a.warmup, reps(big),
                       STAGES[:5] + STAGES[6:])
    show(name)

    ext = float((pts.max(axis=0) - pts.min(axis=0)).max())
    G0 = min(max(round(big ** (1.0 / 3.0)), 1), 256)
    res["cell_sweep"] = {"n": big, "k": 16, "default_G": G0, "rows": []}
    for f in (0.5, 0.7, 1.0, 1.4, 2.0):
        G = f * G0
        _, r = timed(cloud, lambda: cloud.knn(pts, 16, cell=ext / G), big, a.warmup, reps(big))
        row = {"factor": f, "G": G, "cell": ext / G, "cells": r["info"]["cells"],
               "largest_cell": r["info"]["largest_cell"], "tested_per_query": r["tested_per_query"],
               "query_ms": r["kernel_ms"]["query"], "build_ms": round(sum(
                   r["kernel_ms"][s]["median"] for s in ("box", "grid", "scan", "scatter")), 4),
               "tests_per_second": r["tests_per_second"]}
        res["cell_sweep"]["rows"].append(row)
        print(f"bench_knn: sweep {row}", flush=True)

    if not a.no_reference:
        from scipy.spatial import cKDTree
        for cname, pts in clouds.items():
            for k in ([15] if cname.startswith("dino") else a.ks):
                name = f"{cname}_k{k}"
                t0 = time.perf_counter()
                _, ii = cKDTree(pts).query(pts, k, workers=a.threads)
                sec = time.perf_counter() - t0
                wall = g[name]["wall_ms"]["median"] * 1e-3
                kern = sum(v["median"] for v in g[name]["kernel_ms"].values()) * 1e-3
                res["cpu"][name] = {
                    "seconds": round(sec, 4),
                    "lists_equal": bool(np.array_equal(ii.reshape(len(pts), k), lists[name])),
                    "cpu_over_gpu_wall": round(sec / wall, 1),
                    "cpu_over_gpu_kernels": round(sec / kern, 1)}
                print(f"bench_knn: cpu {name}: {res['cpu'][name]}", flush=True)

    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(res, sort_keys=True))


if __name__ == "__main__":
    main()
