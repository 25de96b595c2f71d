#!/usr/bin/env python
"""Time the global registration (tsbb15_amd.cloud.fpfh, match_features,
evaluation.ransac_similarity, global_register; csrc/global_reg.hip) stage by stage, and this
host's route for the same work.

Input: the egg of tests/global_fixture.py, sampled at n = 1e4 and 1e5 points a side (the cloud with
seed 7, moved off the mesh by the fixture's pose 3; the mesh's samples with seed 0), k = 32,
H = 1e5 and 1e6 hypotheses with global_register's default gates.

GPU figures, after `--warmup` calls: `kernel_ms` is the device time between HIP events
(rs_cloud_knn_timing for the lists, rs_global_timing for spfh, fpfh, match, solve, count,
gather; no upload, no download), `wall_ms` the host clock around the whole synchronous call;
median, min and max of `--repeats` timed calls.  The descriptor stands against `cloud.knn` alone
with the same k + 1.

Host route, one run each: the numpy restatement tests/global_ref.py for the RANSAC at the smaller
H, and scipy.spatial.cKDTree(fb).query(fa, workers=threads) for the match, on `--cpu-queries`
rows of fa (a 33-dimensional tree prunes little), scaled to n.  The restatement of the descriptor
builds its lists by brute force in n^2 memory and is not timed.  Needs a GPU; there is no
fallback.  Writes one JSON file (default profiles/global_bench.json) and prints it.
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


def stats(x):
    return {"median": round(float(np.median(x)), 4), "min": round(float(min(x)), 4),
            "max": round(float(max(x)), 4)}


def timed(fn, read, warmup, repeats):
    """fn() timed; read() -> {stage: ms} after every timed call."""
    for _ in range(warmup):
        out = fn()
    wall, kern = [], {}
    for _ in range(repeats):
        t0 = time.perf_counter()
        out = fn()
        wall.append((time.perf_counter() - t0) * 1e3)
        for s, v in read().items():
            kern.setdefault(s, []).append(v)
    return out, {"repeats": repeats, "wall_ms": stats(wall),
                 "kernel_ms": {s: stats(v) for s, v in kern.items()}}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--sizes", type=int, nargs="+", default=[10000, 100000])
    ap.add_argument("--hypotheses", type=int, nargs="+", default=[100000, 1000000])
    ap.add_argument("--threads", type=int, default=16, help="CPU baseline threads")
    ap.add_argument("--cpu-queries", type=int, default=2000)
    ap.add_argument("--no-reference", action="store_true", help="skip the host route")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "global_bench.json"))
    a = ap.parse_args()

    import global_fixture as gf
    import global_ref as ref
    from tsbb15_amd import _ffi, cloud, evaluation as ev
    if _ffi.device_count() < 1:
        raise SystemExit("bench_global: no GPU visible")
    cloud.knn_timing(1)
    cloud.global_timing(1)
    v, f = gf.egg()
    fn = ev.face_normals(v, f)
    _, R, _ = gf.truth(3)
    K = gf.K
    res = {"warmup": a.warmup, "cpu_threads": a.threads, "k": K, "gpu": {}, "cpu": {}}
    g, cpu = res["gpu"], res["cpu"]

    def glob(*stages):
        return lambda: {s: cloud.global_timing(1)[s] for s in stages}

    def show(name):
        print(f"bench_global: {name}: {g[name]['kernel_ms']}, wall {g[name]['wall_ms']}",
              flush=True)

    for n in a.sizes:
        on, face = ev.sample_surface(v, f, n, seed=7)
        pts, nrm = gf.back(on, 3), fn[face] @ R
        tgt, tface = ev.sample_surface(v, f, n, seed=0)
        tnrm = fn[tface]

        name = f"knn_{n}"
        _, g[name] = timed(lambda: cloud.knn(pts, K + 1), lambda: cloud.knn_timing(1),
                           a.warmup, a.repeats)
        for s in ("normals", "mean_dist"):
            g[name]["kernel_ms"].pop(s, None)
        show(name)
        name = f"fpfh_{n}"
        (fa, _, _), g[name] = timed(
            lambda: cloud.fpfh(pts, nrm, k=K),
            lambda: {**{s: t for s, t in cloud.knn_timing(1).items()
                        if s not in ("normals", "mean_dist")}, **glob("spfh", "fpfh")()},
            a.warmup, a.repeats)
        show(name)
        fb = cloud.fpfh(tgt, tnrm, k=K)[0]
        name = f"match_{n}"
        (idx, _), g[name] = timed(lambda: cloud.match_features(fa, fb), glob("match"), a.warmup,
                                  a.repeats)
        sec = g[name]["kernel_ms"]["match"]["median"] * 1e-3
        g[name]["pairs_per_second"] = float(f"{n * n / sec:.3e}")
        g[name]["flops_per_second"] = float(f"{3 * 33 * n * n / sec:.3e}")
        show(name)
        ok = idx >= 0
        src, dst = pts[ok], tgt[idx[ok]]
        ratio = ev.rms_radius(tgt) / ev.rms_radius(pts)
        scale = (0.5 * ratio, 2.0 * ratio)
        dist = 0.03 * ev.mesh_box(v, f)[1]
        s_true, R_true, t_true = gf.truth(3)
        inl = np.linalg.norm(s_true * src @ R_true.T + t_true - dst, axis=1) <= dist
        for H in a.hypotheses:
            name = f"ransac_{n}_H{H}"
            out, g[name] = timed(lambda: ev.ransac_similarity(src, dst, H, dist, scale=scale),
                                 glob("solve", "count", "gather"), a.warmup, a.repeats)
            info = out["info"]
            sec = g[name]["kernel_ms"]["count"]["median"] * 1e-3
            g[name].update(
                M=len(src), inlier_rate=round(float(inl.mean()), 4),
                passed=[int(x) for x in info["passed"]], tests=int(info["tests"]),
                tests_per_second=float(f"{info['tests'] / sec:.3e}"),
                best_count=int(out["count"][0]),
                best_rotation_error_deg=round(gf.pose_errors(out["s"][0], out["R"][0],
                                                             out["t"][0], 3)[0], 3))
            show(name)
        name = f"global_register_{n}"
        t0 = time.perf_counter()
        reg = ev.global_register(pts, nrm, v, f, k=K)
        g[name] = {"wall_ms": round((time.perf_counter() - t0) * 1e3, 1),
                   "chosen": reg["chosen"],
                   "coarse_rotation_error_deg": round(gf.pose_errors(*reg["coarse"], 3)[0], 3),
                   "rotation_error_deg": float(f"{gf.pose_errors(reg['s'], reg['R'], reg['t'], 3)[0]:.3e}"),
                   "iterations": reg["registration"]["iterations"]}
        print(f"bench_global: {name}: {g[name]}", flush=True)

        if a.no_reference:
            continue
        from scipy.spatial import cKDTree
        q = min(n, a.cpu_queries)
        t0 = time.perf_counter()
        far, near = cKDTree(fb).query(fa[:q], workers=a.threads)
        sec = (time.perf_counter() - t0) * n / q
        d2 = ((fa[:q] - fb[idx[:q]]) ** 2).sum(axis=1)
        # small-integer histograms tie exactly; the tree takes any of the nearest, the GPU the first
        cpu[f"match_{n}"] = {"queries": q, "seconds_scaled_to_n": round(sec, 3),
                             "indices_equal": float((near == idx[:q]).mean()),
                             "distances_equal": bool(np.allclose(far * far, d2, rtol=1e-9,
                                                                 atol=1e-300)),
                             "cpu_over_gpu_wall": round(
                                 sec / (g[f"match_{n}"]["wall_ms"]["median"] * 1e-3), 1)}
        H = min(a.hypotheses)
        t0 = time.perf_counter()
        want = ref.ransac(src, dst, H, dist, scale=scale)
        sec = time.perf_counter() - t0
        got = ev.ransac_similarity(src, dst, H, dist, scale=scale)
        cpu[f"ransac_{n}_H{H}"] = {
            "seconds": round(sec, 3),
            "equal": bool(np.array_equal(want["h"], got["h"])
                          and np.array_equal(want["R"], got["R"])),
            "cpu_over_gpu_wall": round(
                sec / (g[f"ransac_{n}_H{H}"]["wall_ms"]["median"] * 1e-3), 1)}
        for key in (f"match_{n}", f"ransac_{n}_H{H}"):
            if key in cpu:
                print(f"bench_global: cpu {key}: {cpu[key]}", flush=True)

    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(json.dumps(res, sort_keys=True))


if __name__ == "__main__":
    main()
