#!/usr/bin/env python
"""Time one GPU wash (tsbb15_amd.tables.wash_points, rs_wash_points) on a Dino-sized table and
the numpy reference (tests/wash_ref.py) on the same input.

The table: the 36 cameras and all points of tests/golden/dino_pnp_kat.npz in camera 0's frame
with the sparse tracks of tests/ba_fixture.py (point j is seen by 2 + j % 35 consecutive views
starting at view j % 36, observations shuffled), uv = exact projection + `--noise` N(0, 1), and
`--outliers` of the observations displaced by 0.02 in a random direction.  thresh = 1e-3.

GPU figures: the wall time of whole calls (host clock around the synchronous call: host CSR
build, one upload, one launch, one download), after warm-up calls; the median and the spread
of `--repeats` calls.  Needs a GPU; there is no fallback.  Writes one JSON file (default
profiles/wash_bench.json) and prints it.
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


def dino_table(nC=36, noise=1e-4, outliers=0.05, seed=0):
    import ba_fixture as bf
    nP = len(np.load(os.path.join(REPO, "tests", "golden", "dino_pnp_kat.npz"))["points3d"])
    P = bf.problem(nC, nP, seed, noise=noise)
    rng = np.random.RandomState(4000 + seed)
    uv = P["uv"].copy()
    n = len(uv)
    pick = rng.choice(n, int(round(outliers * n)), replace=False)
    ang = rng.uniform(0.0, 2.0 * np.pi, len(pick))
    uv[pick] += 0.02 * np.stack([np.cos(ang), np.sin(ang)], axis=1)
    bad = np.zeros(n, bool)
    bad[pick] = True
    pts0 = P["pts"] + 0.05 * rng.standard_normal(P["pts"].shape)
    return P["cams"], pts0, P["ov"], P["op"], uv, bad


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--repeats", type=int, default=20, help="timed GPU calls")
    ap.add_argument("--warmup", type=int, default=3, help="untimed GPU calls before them")
    ap.add_argument("--noise", type=float, default=1e-4)
    ap.add_argument("--outliers", type=float, default=0.05)
    ap.add_argument("--thresh", type=float, default=1e-3)
    ap.add_argument("--no-reference", action="store_true", help="skip the numpy reference run")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "wash_bench.json"))
    a = ap.parse_args()

    from tsbb15_amd import _ffi
    from tsbb15_amd import tables as gt
    if _ffi.device_count() < 1:
        raise SystemExit("bench_wash: no GPU visible")
    ctx = _ffi.default_context()
    cams, pts0, ov, op, uv, bad = dino_table(noise=a.noise, outliers=a.outliers)
    lens = np.bincount(op, minlength=len(pts0))
    res = {"table": {"cameras": len(cams), "points": len(pts0), "observations": len(ov),
                     "displaced": int(bad.sum()), "longest_track": int(lens.max()),
                     "pairs": int((lens * (lens - 1) // 2).sum()), "noise": a.noise,
                     "thresh": a.thresh}}
    print(f"bench_wash: {res['table']}", flush=True)

    for _ in range(a.warmup):
        gt.wash_points(cams, pts0, ov, op, uv, a.thresh, ctx=ctx)
    wall = []
    for _ in range(a.repeats):
        t0 = time.perf_counter()
        out = gt.wash_points(cams, pts0, ov, op, uv, a.thresh, ctx=ctx)
        wall.append((time.perf_counter() - t0) * 1e3)
    pts, obs_keep, point_keep, err2, info = out
    med = float(np.median(wall))
    long = (lens >= 4)[op]
    res["gpu"] = {"info": info, "wall_ms": [round(w, 4) for w in wall],
                  "wall_ms_median": round(med, 4), "wall_ms_min": round(min(wall), 4),
                  "wall_ms_max": round(max(wall), 4),
                  "hypotheses_per_second": round(info["hypotheses"] / (med * 1e-3)),
                  "misclassified_on_tracks_ge_4": int((obs_keep[long] == bad[long]).sum())}
    print(f"bench_wash: gpu {res['gpu']}", flush=True)

    if not a.no_reference:
        import wash_ref as wr
        t0 = time.perf_counter()
        ref = wr.wash_points(cams, pts0, ov, op, uv, a.thresh)
        sec = time.perf_counter() - t0
        both = ref[2] & point_keep
        res["reference_cpu"] = {
            "info": ref[4], "seconds": round(sec, 3),
            "masks_equal": bool(np.array_equal(ref[1], obs_keep)
                                and np.array_equal(ref[2], point_keep)),
            "kept_points_max_abs_diff": float(np.abs(ref[0][both] - pts[both]).max())}
        res["speedup_vs_reference"] = round(sec * 1e3 / med, 1)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(res, sort_keys=True))


if __name__ == "__main__":
    main()
