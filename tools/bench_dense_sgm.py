#!/usr/bin/env python
"""Time the semi-global aggregation of the dense stage (tsbb15_amd.dense.plane_sweep_sgm,
csrc/dense_sgm.hip) beside the plane sweep of the same call.

Inputs: the textured slanted plane of tests/dense_fixture.py rendered at 576 x 720 (the Dino
images' size) into one reference view and four sources, every image perturbed by N(0, 35) grey
levels (seed 7); D = 128 planes uniform in 1 / depth, patch 7, 8 paths, p1 = 0.1, p2 = 1.0.

After `--warmup` calls, `--repeats` timed calls of plane_sweep_sgm without optional outputs.
`sweep_ms`, `aggregate_ms`, `select_ms` are the device times between HIP events around the stages
of each call (rs_dense_sgm_timing: no upload, no download): the sweep kernel; the cost launch,
one launch per direction and S back to the volume's layout; the winner.  `wall_ms` is the host
clock around the whole synchronous call.  Median, min and max of the timed calls.

Bytes per entry (an entry is one (pixel, plane) of the volume, D h w of them):
  `floor_bytes_per_entry`    one read of c and one read-modify-write of S per direction, 12 B x
                             paths = 96 B at 8 paths;
  `counted_bytes_per_entry`  what the launches move as written: the cost launch reads v and
                             writes c (8), the first direction reads c and writes S (8), every
                             other direction reads c, reads and writes S (12 each), and S goes
                             back to the volume's layout (8);
  `achieved_bytes_per_second` counted bytes over the median aggregate time;
  `implied_bytes_per_entry`  the median aggregate time at the measured HBM copy rate of
                             6.29 TB/s, per entry: what the time would pay for if the stage ran
                             at that rate, to be read against the floor.
Needs a GPU; there is no fallback.  Writes one JSON file (default
profiles/dense_sgm_bench.json) and prints it.
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

# bytes / s of a float4 copy over the whole chip as measured (8.0e12 nominal)
HBM_COPY_RATE = 6.29e12


def stats(x):
    return {"median": round(float(np.median(x)), 4), "min": round(float(min(x)), 4),
            "max": round(float(max(x)), 4)}


def counted_bytes_per_entry(paths):
    return 8 + 8 + 12 * (paths - 1) + 8


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--repeats", type=int, default=20, help="timed GPU calls")
    ap.add_argument("--warmup", type=int, default=3, help="untimed GPU calls before them")
    ap.add_argument("--size", type=int, nargs=2, default=[576, 720], metavar=("H", "W"))
    ap.add_argument("--planes", type=int, default=128)
    ap.add_argument("--sources", type=int, default=4)
    ap.add_argument("--patch", type=int, default=7)
    ap.add_argument("--paths", type=int, default=8, choices=(4, 8))
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "dense_sgm_bench.json"))
    a = ap.parse_args()

    import dense_fixture as df
    from bench_dense import make_scene
    from tsbb15_amd import _ffi, dense
    if _ffi.device_count() < 1:
        raise SystemExit("bench_dense_sgm: no GPU visible")
    h, w = a.size
    D, S = a.planes, a.sources
    imgs, cams, K = make_scene(df, h, w, S)
    noise = np.random.RandomState(7).normal(0, 35, imgs.shape)
    imgs = np.clip(np.rint(imgs.astype(np.float64) + noise), 0, 255).astype(np.uint8)
    depths = 1.0 / np.linspace(0.375, 0.1, D)
    run = lambda: dense.plane_sweep_sgm(imgs[0], cams[0], imgs[1:], cams[1:], K, depths,
                                        patch=a.patch, p1=0.1, p2=1.0, paths=a.paths)
    dense.sgm_timing(1)
    for _ in range(a.warmup):
        out = run()
    wall = []
    ms = {k: [] for k in dense.SGM_STAGES}
    for _ in range(a.repeats):
        t0 = time.perf_counter()
        out = run()
        wall.append((time.perf_counter() - t0) * 1e3)
        for k, v in dense.sgm_timing(1).items():
            ms[k].append(v)
    dense.sgm_timing(0)
    wta = dense.plane_sweep(imgs[0], cams[0], imgs[1:], cams[1:], K, depths, patch=a.patch)

    entries = D * h * w
    sec = float(np.median(ms["aggregate"])) * 1e-3
    counted = counted_bytes_per_entry(a.paths)
    res = {"repeats": a.repeats, "warmup": a.warmup, "size": [h, w], "D": D, "S": S,
           "patch": a.patch, "paths": a.paths, "p1": 0.1, "p2": 1.0, "entries": entries,
           "sweep_ms": stats(ms["sweep"]), "aggregate_ms": stats(ms["aggregate"]),
           "select_ms": stats(ms["select"]), "wall_ms": stats(wall),
           "aggregate_over_sweep": round(float(np.median(ms["aggregate"]) /
                                               np.median(ms["sweep"])), 3),
           "floor_bytes_per_entry": 12 * a.paths,
           "counted_bytes_per_entry": counted,
           "achieved_bytes_per_second": float(f"{counted * entries / sec:.4e}"),
           "hbm_copy_bytes_per_second": HBM_COPY_RATE,
           "implied_bytes_per_entry": round(sec * HBM_COPY_RATE / entries, 1),
           "valid_pixels": int((out[0] >= 0).sum()),
           "winners_changed_fraction": round(float((out[0] != wta[0])[wta[0] >= 0].mean()), 4)}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(res, sort_keys=True))


if __name__ == "__main__":
    main()
