#!/usr/bin/env python
"""Time the plane sweep of the dense stage (tsbb15_amd.dense.plane_sweep, csrc/dense.hip), and
the numpy restatement of the same definition on this host's CPU.

Inputs: the textured slanted plane of tests/dense_fixture.py rendered at 576 x 720 (the Dino
images' size) into one reference view and four sources; D = 64 and 128 planes uniform in
1 / depth, S = 2 and 4 sources, patch 7.

GPU figures, after `--warmup` calls: `kernel_ms` is the device time between HIP events around
the one kernel (rs_dense_timing: no upload, no download), `wall_ms` the host clock around the
whole synchronous call (upload, kernel, download, the Python shim); median, min and max of the
timed calls.  `samples` = h w D S n patch samples per call, `samples_per_second` over the kernel
time.  `lds_read_bytes` = 2 n four-byte LDS reads per (pixel, plane, source), the kernel's
window loop as written; `lds_read_fraction` is that over the kernel time against the chip's
aggregate rate for four-byte LDS reads: 75 TB/s measured with every CU streaming ds_read_b32,
against 128 B per clock x 256 CUs x 2.4 GHz = 78.6 TB/s nominal.

CPU baseline: tests/dense_ref.py (fp64) once at `--cpu-size` with D = 16, S = 2, a size it
finishes in seconds; `cpu_samples_per_second` by the same count.  Needs a GPU; there is no
fallback.  Writes one JSON file (default profiles/dense_bench.json) and prints it.
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

# ds_read_b32 moves 128 B per clock per CU: 256 CUs at 2.4 GHz give 78.6e12 B/s nominal.  The
# rate measured with every CU streaming four-byte reads is about 75e12 B/s (0.95 of that, or the
# nominal rate at 2.29 GHz); the fraction is taken against the measured rate.
LDS_READ_B32_NOMINAL = 128 * 256 * 2.4e9
LDS_READ_B32_RATE = 75e12   # bytes / s, the whole chip


def stats(x):
    return {"median": round(float(np.median(x)), 4), "min": round(float(min(x)), 4),
            "max": round(float(max(x)), 4)}


def make_scene(df, h, w, n_src):
    """Reference view [I | 0] and n_src sources around it, all seeing the slanted plane."""
    f = 60.0 * w / df.W
    K = np.array([[f, 0.0, (w - 1) / 2.0], [0.0, f, (h - 1) / 2.0], [0.0, 0.0, 1.0]])
    base = df.cameras()
    cams = [base[0], base[1], base[2], df.camera((0.1, -0.4, 0.0), (1, 0, 0), 0.05),
            df.camera((-0.1, 0.45, 0.03), (1, 0, 0), -0.06)][:n_src + 1]
    imgs = [df.render(C, df.SLANTED, h, w, K)[0] for C in cams]
    return np.array(imgs), np.array(cams), K


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--repeats", type=int, default=10, help="timed GPU calls per case")
    ap.add_argument("--warmup", type=int, default=2, help="untimed GPU calls before them")
    ap.add_argument("--size", type=int, nargs=2, default=[576, 720], metavar=("H", "W"))
    ap.add_argument("--planes", type=int, nargs="+", default=[64, 128])
    ap.add_argument("--sources", type=int, nargs="+", default=[2, 4])
    ap.add_argument("--patch", type=int, default=7)
    ap.add_argument("--cpu-size", type=int, nargs=2, default=[72, 90], metavar=("H", "W"))
    ap.add_argument("--no-reference", action="store_true", help="skip the CPU baseline")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "dense_bench.json"))
    a = ap.parse_args()

    import dense_fixture as df
    import dense_ref as dr
    from tsbb15_amd import _ffi, dense
    if _ffi.device_count() < 1:
        raise SystemExit("bench_dense: no GPU visible")
    dense.timing(1)
    h, w = a.size
    n = a.patch * a.patch
    imgs, cams, K = make_scene(df, h, w, max(a.sources))
    res = {"repeats": a.repeats, "warmup": a.warmup, "size": [h, w], "patch": a.patch,
           "lds_read_b32_bytes_per_second": LDS_READ_B32_RATE,
           "lds_read_b32_nominal_bytes_per_second": LDS_READ_B32_NOMINAL, "gpu": {}}
    for D in a.planes:
        depths = 1.0 / np.linspace(0.375, 0.1, D)
        for S in a.sources:
            run = lambda: dense.plane_sweep(imgs[0], cams[0], imgs[1:S + 1], cams[1:S + 1], K,
                                            depths, patch=a.patch)
            for _ in range(a.warmup):
                out = run()
            wall, kern = [], []
            for _ in range(a.repeats):
                t0 = time.perf_counter()
                out = run()
                wall.append((time.perf_counter() - t0) * 1e3)
                kern.append(dense.timing(1)["plane_sweep"])
            samples = h * w * D * S * n
            sec = float(np.median(kern)) * 1e-3
            lds = 8 * samples
            r = {"D": D, "S": S, "kernel_ms": stats(kern), "wall_ms": stats(wall),
                 "samples": samples, "samples_per_second": float(f"{samples / sec:.4e}"),
                 "lds_read_bytes": lds,
                 "lds_read_bytes_per_second": float(f"{lds / sec:.4e}"),
                 "lds_read_fraction": round(lds / sec / LDS_READ_B32_RATE, 4),
                 "valid_pixels": int((out[0] >= 0).sum()),
                 "median_sources": float(np.median(out[3][out[0] >= 0]))}
            res["gpu"][f"D{D}_S{S}"] = r
            print(f"bench_dense: D={D} S={S}: {r}", flush=True)

    if not a.no_reference:
        ch, cw = a.cpu_size
        D, S = 16, 2
        ci, cc, cK = make_scene(df, ch, cw, S)
        depths = 1.0 / np.linspace(0.375, 0.1, D)
        t0 = time.perf_counter()
        ref = dr.plane_sweep(ci[0], cc[0], ci[1:], cc[1:], cK, depths, a.patch, 4.0)
        sec = time.perf_counter() - t0
        got = dense.plane_sweep(ci[0], cc[0], ci[1:], cc[1:], cK, depths, patch=a.patch)
        samples = ch * cw * D * S * n
        res["cpu"] = {"size": [ch, cw], "D": D, "S": S, "seconds": round(sec, 4),
                      "samples": samples,
                      "cpu_samples_per_second": float(f"{samples / sec:.4e}"),
                      "indices_equal_fraction": round(float((got[0] == ref[0]).mean()), 6),
                      "score_max_diff": float(f"{np.nanmax(np.abs(got[2] - ref[2])):.3e}")}
        print(f"bench_dense: cpu {res['cpu']}", flush=True)

    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(res, sort_keys=True))


if __name__ == "__main__":
    main()
