#!/usr/bin/env python
"""Time the point-cloud stage (tsbb15_amd.cloud, csrc/cloud.hip) stage by stage, and the same
work on this host's CPU.

Inputs: the reference's own Dino cloud (tests/golden/cloud.npz, 688 points, r = 0.1, oriented
by its view normals) and the noisy unit sphere of tests/cloud_fixture.py at n = 1e5 and 1e6 with
r = sqrt(120 / n), which gives a median of about 30 neighbours; for rs_cloud_attributes a
synthetic table of 36 cameras with 4 entries per point on the same clouds.

GPU figures, after `--warmup` calls: `kernel_ms` per stage is the device time between HIP events
(rs_cloud_timing: grid, scan, sort, normals; no upload, no download), `kernel_ms.total` their
sum, `wall_ms` the host clock around the whole synchronous call (staging copies, upload,
kernels, download, the Python shim); median, min and max of the timed calls.  `pairs_per_second`
is info.pairs_tested over the normals stage.  `fp64_peak_fraction` counts 8 flops per pair
tested (3 subtractions, 3 products, 2 additions), 15 more per neighbour found (3 + 12 for s and
S) and 600 per ok row for the eigen-solve, over the normals stage, against 78.6 TFLOP/s.

CPU baseline, one run each on `--threads` threads: scipy.spatial.cKDTree.query_ball_point
(workers = threads) for the neighbourhoods, the same M by np.add.reduceat over the flattened
lists, and one batched np.linalg.eigh; tree construction included.  Needs a GPU; there is no
fallback.  Writes one JSON file (default profiles/cloud_bench.json) and prints it.
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

FP64_PEAK = 78.6e12
STAGES = ("grid", "scan", "sort", "normals")


def stats(x):
    return {"median": round(float(np.median(x)), 4), "min": round(float(min(x)), 4),
            "max": round(float(max(x)), 4)}


def time_normals(cloud, pts, radius, orient, warmup, repeats):
    for _ in range(warmup):
        out = cloud.surface_normals(pts, radius, orient=orient)
    wall, kern = [], {k: [] for k in STAGES + ("total",)}
    for _ in range(repeats):
        t0 = time.perf_counter()
        out = cloud.surface_normals(pts, radius, orient=orient)
        wall.append((time.perf_counter() - t0) * 1e3)
        ms = cloud.timing(1)
        for k in STAGES:
            kern[k].append(ms[k])
        kern["total"].append(sum(ms[k] for k in STAGES))
    info = out[4]
    res = {"n": len(pts), "radius": radius, "repeats": repeats, "info": info,
           "median_count": float(np.median(out[2])),
           "kernel_ms": {k: stats(v) for k, v in kern.items()}, "wall_ms": stats(wall)}
    sec = res["kernel_ms"]["normals"]["median"] * 1e-3
    flops = 8 * info["pairs_tested"] + 15 * info["neighbours_found"] + \
        600 * (len(pts) - info["rows_not_ok"])
    res["pairs_per_second"] = round(info["pairs_tested"] / sec)
    res["normals_flops"] = flops
    res["fp64_peak_fraction"] = float(f"{flops / sec / FP64_PEAK:.3e}")
    return out, res


def time_attributes(cloud, pts, warmup, repeats):
    rs = np.random.RandomState(0)
    n, nC, per = len(pts), 36, 4
    cams = np.zeros((nC, 3, 4))
    for k in range(nC):
        q, _ = np.linalg.qr(rs.standard_normal((3, 3)))
        cams[k, :, :3], cams[k, :, 3] = q, rs.standard_normal(3) * 3.0
    nobs = n * per
    ov = rs.randint(0, nC, nobs)
    col = rs.randint(0, 256, (nobs, 3)).astype(np.float64)
    ep, eo = np.repeat(np.arange(n), per), np.arange(nobs)
    fn = lambda: cloud.point_attributes(cams, pts, ep, eo, ov, col)
    for _ in range(warmup):
        fn()
    wall, kern = [], []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        wall.append((time.perf_counter() - t0) * 1e3)
        kern.append(cloud.timing(1)["attributes"])
    return {"n": n, "entries": nobs, "kernel_ms": stats(kern), "wall_ms": stats(wall)}


def cpu_normals(pts, radius, threads, chunk=100000):
    """(normals, count, evals, seconds per step) with scipy and numpy on `threads` threads."""
    from scipy.spatial import cKDTree
    from threadpoolctl import threadpool_limits
    n = len(pts)
    t0 = time.perf_counter()
    tree = cKDTree(pts)
    t_tree = time.perf_counter() - t0
    t_query = t_cov = t_eig = 0.0
    normals, evals = np.full((n, 3), np.nan), np.full((n, 3), np.nan)
    count = np.zeros(n, np.int64)
    with threadpool_limits(limits=threads):
        for at in range(0, n, chunk):
            q = pts[at:at + chunk]
            t0 = time.perf_counter()
            nb = tree.query_ball_point(q, radius, workers=threads, return_sorted=True)
            t_query += time.perf_counter() - t0
            t0 = time.perf_counter()
            k = np.fromiter((len(x) for x in nb), np.int64, len(nb))
            flat = np.concatenate([np.asarray(x, dtype=np.int64) for x in nb])
            start = np.concatenate(([0], np.cumsum(k)[:-1]))
            d = pts[flat] - np.repeat(q, k, axis=0)
            s = np.add.reduceat(d, start, axis=0) / k[:, None]
            outer = d[:, [0, 0, 0, 1, 1, 2]] * d[:, [0, 1, 2, 1, 2, 2]]
            S = np.add.reduceat(outer, start, axis=0) / k[:, None]
            M = S[:, [0, 1, 2, 1, 3, 4, 2, 4, 5]].reshape(-1, 3, 3) - s[:, :, None] * s[:, None, :]
            t_cov += time.perf_counter() - t0
            t0 = time.perf_counter()
            w, V = np.linalg.eigh(M)
            t_eig += time.perf_counter() - t0
            ok = k >= 3
            count[at:at + chunk] = k
            evals[at:at + chunk][ok] = w[ok]
            normals[at:at + chunk][ok] = V[ok, :, 0]
    sec = {"tree": t_tree, "query_ball_point": t_query, "covariance": t_cov, "eigh": t_eig}
    sec["total"] = sum(sec.values())
    return normals, count, evals, {k: round(v, 4) for k, v in sec.items()}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--repeats", type=int, default=10, help="timed GPU calls per case")
    ap.add_argument("--warmup", type=int, default=2, help="untimed GPU calls before them")
    ap.add_argument("--sizes", type=int, nargs="+", default=[100000, 1000000])
    ap.add_argument("--threads", type=int, default=16, help="CPU baseline threads")
    ap.add_argument("--no-reference", action="store_true", help="skip the CPU baseline")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "cloud_bench.json"))
    a = ap.parse_args()

    import cloud_fixture as cf
    from tsbb15_amd import _ffi, cloud
    if _ffi.device_count() < 1:
        raise SystemExit("bench_cloud: no GPU visible")
    cloud.timing(1)
    res = {"repeats": a.repeats, "warmup": a.warmup, "fp64_peak_flops": FP64_PEAK,
           "cpu_threads": a.threads, "gpu": {}, "cpu_seconds": {}, "gpu_over_cpu": {}}
    g = res["gpu"]

    d = cf.dino()
    cases = [("dino_688", np.array(d["points"]), 0.1, np.array(d["normals"]), 2 * a.repeats)]
    for n in a.sizes:
        cases.append((f"sphere_{n}", cf.sphere(n), float(np.sqrt(120.0 / n)), None,
                      a.repeats if n <= 200000 else max(3, a.repeats // 2)))
    outs = {}
    for name, pts, radius, orient, reps in cases:
        outs[name], g[name] = time_normals(cloud, pts, radius, orient, a.warmup, reps)
        g[name + "_attributes"] = time_attributes(cloud, pts, a.warmup, reps)
        print(f"bench_cloud: {name}: {g[name]}", flush=True)

    if not a.no_reference:
        for name, pts, radius, orient, reps in cases:
            normals, count, evals, sec = cpu_normals(pts, radius, a.threads)
            res["cpu_seconds"][name] = sec
            got = outs[name]
            ok = got[1]
            same = np.array_equal(count, got[2])
            dev = float(np.abs(evals[ok] - got[3][ok]).max() / radius ** 2) if same else None
            wall = g[name]["wall_ms"]["median"] * 1e-3
            kern = g[name]["kernel_ms"]["total"]["median"] * 1e-3
            res["gpu_over_cpu"][name] = {
                "counts_equal": bool(same), "evals_max_diff_over_r2": dev,
                "cpu_over_gpu_wall": round(sec["total"] / wall, 1),
                "cpu_over_gpu_kernels": round(sec["total"] / kern, 1)}
            print(f"bench_cloud: cpu {name}: {sec} {res['gpu_over_cpu'][name]}", flush=True)

    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(res, sort_keys=True))


if __name__ == "__main__":
    main()
