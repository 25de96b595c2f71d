#!/usr/bin/env python
"""Time mesh registration (evaluation.register, the rs_eval_index_* entries of csrc/eval.hip) and
the only way to iterate without them: a loop of evaluation.mesh_distance and numpy.

Inputs: the mesh of tools/bench_eval.py (the slanted plane of tests/dense_fixture.py in 16 views
of 576 x 720, fused into a 256^3 volume).  The source cloud is its vertices displaced by a seeded
noise of half a voxel and then moved, about the box centre, by 1 degree, 1 voxel and 1 % of scale;
keep is 0.9.  The target is planar up to its noise: the motion along the plane is not determined
(np.linalg.lstsq takes the minimum-norm step) and neither is a free scale, since a smaller cloud
lies closer to the plane.  The stage and iteration times are what this input is for; the loops do
not stop by their own rule on it, and `rigid` records the fit without
scale.

Per metric, after `--warmup` calls, median, min and max of `--repeats`:
  step_kernel_ms   device time between HIP events around a step's stages (rs_eval_index_timing:
                   transform, query, select, moments), at the start transform
  step_wall_ms     host clock around one MeshIndex.step at the start transform (the record's
                   download and the synchronisation included)
  iteration_wall_ms  host clock around a whole evaluation.register on a built index with the cloud
                   re-uploaded, over its iterations: step, numpy solve and the final read
  baseline_iteration_wall_ms  host clock around one iteration of the baseline loop with the same
                   cell: numpy transform, evaluation.mesh_distance (which rebuilds the grid and
                   downloads three arrays), np.partition for tau, the moments in numpy
                   (tests/register_ref.py's terms, np.sum), the same solve
  iterations, baseline_iterations   steps until the loop's own stop rule
  rigid            one more evaluation.register with with_scale=False: its iterations, rms and
                   host clock per iteration
`index_build_wall_ms` and `set_points_wall_ms` are paid once per mesh and per cloud.  The baseline
calls the same rs_eval_mesh_distance this commit ships; its source is that of the parent commit.
Needs a GPU; there is no fallback.  Writes one JSON file (default profiles/register_bench.json) and
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
          os.path.join(REPO, "tests"), os.path.join(REPO, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

KEEP = 0.9


def stats(x):
    return {"median": round(float(np.median(x)), 4), "min": round(float(min(x)), 4),
            "max": round(float(max(x)), 4)}


def clock(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def baseline_iteration(ev, ref, pts, v, f, cell, origin, T, metric):
    """One iteration made of what the parent commit has: returns (rms, matched, next T)."""
    s, R, t = T
    moved = ev.apply_similarity(pts, s, R, t)
    _, face, closest, info = ev.mesh_distance(moved, v, f, cell=cell)
    d2 = info["d2"]
    matched = face >= 0
    m = int(matched.sum())
    k = ref.trim_rank(KEEP, m)
    tau = np.partition(d2[matched], k - 1)[k - 1]
    mask = matched & (d2 <= tau)
    mom = np.zeros(ref.SLOTS)
    w = ref.terms(metric, moved, closest, d2, face, v, f, origin, mask)
    mom[:w.shape[1]] = w.sum(axis=0)
    kept = int(mask.sum())
    rms = float(np.sqrt(mom[ref.RMS_SLOT[metric]] / kept))
    ds, dR, dt = ref.update(metric, mom, kept, origin)
    return rms, m, (ds * s, dR @ R, ds * dR @ t + dt)


def baseline_loop(ev, ref, pts, v, f, cell, origin, diag, metric, max_iter=50, rtol=1e-6):
    T, rms, wall = (1.0, np.eye(3), np.zeros(3)), [], []
    for it in range(max_iter):
        ms, (r, _, nxt) = clock(lambda: baseline_iteration(ev, ref, pts, v, f, cell, origin, T,
                                                           metric))
        wall.append(ms)
        rms.append(r)
        if r <= 1e-12 * diag or (it > 0 and abs(rms[-2] - r) <= rtol * rms[-2]):
            break
        T = nxt
    return rms, wall


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--repeats", type=int, default=10, help="timed calls")
    ap.add_argument("--warmup", type=int, default=2, help="untimed calls before them")
    ap.add_argument("--size", type=int, nargs=2, default=[576, 720], metavar=("H", "W"))
    ap.add_argument("--views", type=int, default=16)
    ap.add_argument("--side", type=int, default=256, help="nodes per side of the volume")
    ap.add_argument("--no-baseline", action="store_true")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "register_bench.json"))
    a = ap.parse_args()

    import bench_eval
    import bench_surface as bs
    import dense_fixture as df
    import register_ref as ref
    from tsbb15_amd import _ffi, evaluation as ev, surface
    if _ffi.device_count() < 1:
        raise SystemExit("bench_register: no GPU visible")
    h, w = a.size
    v, f, voxel = bench_eval.make_mesh(df, surface, bs, h, w, a.views, a.side)
    nv, nf = len(v), len(f)
    print(f"bench_register: {nv} vertices, {nf} faces, voxel {voxel:.5f}", flush=True)
    origin, diag = ev.mesh_box(v, f)
    cell = ev.default_cell(v, f)
    rs = np.random.RandomState(0)
    noisy = v + 0.5 * voxel * rs.standard_normal(v.shape)
    axis = np.array([1.0, 2.0, 3.0]) / np.sqrt(14.0)
    s0, R0 = 1.01, ev.rotation_exp(np.radians(1.0) * axis)
    t0 = voxel * np.array([2.0, -1.0, 2.0]) / 3.0
    pts = origin + (noisy - origin - t0) @ R0 / s0      # s0 R0 (p - o) + o + t0 puts it back
    res = {"repeats": a.repeats, "warmup": a.warmup, "size": [h, w], "views": a.views,
           "side": a.side, "vertices": nv, "faces": nf, "points": len(pts), "voxel": voxel,
           "cell": float(f"{cell:.6g}"), "keep": KEEP, "diagonal": float(f"{diag:.6g}"),
           "start": {"degrees": 1.0, "translation_voxels": 1.0, "scale": s0},
           "library": os.path.basename(os.path.dirname(_ffi.LIB_PATH)), "metrics": {}}

    build = [clock(lambda: ev.MeshIndex(v, f, cell=cell).close())[0]
             for _ in range(a.warmup + a.repeats)][a.warmup:]
    res["index_build_wall_ms"] = stats(build)
    with ev.MeshIndex(v, f, cell=cell) as index:
        res["cells"], res["entries"] = list(index.cells), index.entries
        up = [clock(lambda: index.set_points(pts))[0] for _ in range(a.warmup + a.repeats)]
        res["set_points_wall_ms"] = stats(up[a.warmup:])
        for metric in ev.REG_METRICS:
            index.timing(1)
            wall, kern = [], {k: [] for k in ev.REG_STAGES}
            for i in range(a.warmup + a.repeats):
                ms, rec = clock(lambda: index.step(keep=KEEP, metric=metric))
                if i >= a.warmup:
                    wall.append(ms)
                    for k, val in index.timing(1).items():
                        kern[k].append(val)
            index.timing(0)
            loops, its = [], []
            for i in range(a.warmup + a.repeats):
                ms, out = clock(lambda: ev.register(pts, None, None, metric=metric, keep=KEEP,
                                                    index=index))
                if i >= a.warmup:
                    loops.append(ms / out["iterations"])
                    its.append(out["iterations"])
            ang = np.degrees(np.arccos(np.clip((np.trace(out["R"] @ R0.T) - 1.0) / 2.0, -1, 1)))
            m = {"step_kernel_ms": {k: stats(x) for k, x in kern.items()},
                 "step_wall_ms": stats(wall), "iteration_wall_ms": stats(loops),
                 "iterations": int(its[-1]), "converged": bool(out["converged"]),
                 "matched": int(rec["matched"]), "kept": int(rec["kept"]),
                 "tests_per_point": round(rec["tests"] / len(pts), 2),
                 "rms_voxels": [float(f"{r / voxel:.5g}") for r in out["rms"]],
                 "rotation_left_degrees": float(f"{ang:.4g}"),
                 "scale_left": float(f"{abs(out['s'] / s0 - 1.0):.4g}")}
            # the same loop for a rigid motion: on this planar, noisy target a free scale is not
            # determined (a smaller cloud lies closer to the plane)
            ms, rigid = clock(lambda: ev.register(pts, None, None, metric=metric, keep=KEEP,
                                                  with_scale=False, index=index))
            ang = np.degrees(np.arccos(np.clip((np.trace(rigid["R"] @ R0.T) - 1.0) / 2.0, -1, 1)))
            m["rigid"] = {"iterations": int(rigid["iterations"]),
                          "converged": bool(rigid["converged"]),
                          "iteration_wall_ms": round(ms / rigid["iterations"], 4),
                          "rms_voxels": [float(f"{r / voxel:.5g}") for r in rigid["rms"]],
                          "rotation_left_degrees": float(f"{ang:.4g}")}
            q = float(np.median(kern["query"]))
            m["other_stages_over_query"] = round(
                sum(float(np.median(kern[k])) for k in kern if k != "query") / q, 4)
            res["metrics"][metric] = m
            print(f"bench_register: {metric} {m}", flush=True)
            if not a.no_baseline:
                for _ in range(a.warmup):
                    baseline_iteration(ev, ref, pts, v, f, cell, origin,
                                       (1.0, np.eye(3), np.zeros(3)), metric)
                rms, bwall = baseline_loop(ev, ref, pts, v, f, cell, origin, diag, metric)
                m["baseline_iteration_wall_ms"] = stats(bwall)
                m["baseline_iterations"] = len(rms)
                m["baseline_rms_voxels"] = [float(f"{r / voxel:.5g}") for r in rms]
                m["baseline_over_iteration"] = round(
                    float(np.median(bwall)) / m["iteration_wall_ms"]["median"], 2)
                print(f"bench_register: {metric} baseline {stats(bwall)} x {len(rms)}",
                      flush=True)
    if not a.no_baseline:
        # what of a baseline iteration is the mesh_distance call alone
        md = [clock(lambda: ev.mesh_distance(pts, v, f, cell=cell))[0]
              for _ in range(a.warmup + a.repeats)][a.warmup:]
        res["mesh_distance_wall_ms"] = stats(md)

    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(json.dumps(res, sort_keys=True))


if __name__ == "__main__":
    main()
