#!/usr/bin/env python
"""Time one GPU bundle adjustment (tsbb15_amd.tables.bundle_adjust, rs_bundle_adjust) on a
Dino-sized problem and the CPU oracle (oracle.tables_ref.bundle_adjust_lm) on the same input.

The problem: the 36 cameras and 676 points of tests/golden/dino_pnp_kat.npz in camera 0's
frame; point j is seen by 2 + j % 35 consecutive views starting at view j % 36; observations
shuffled; uv = exact projection + `--noise` N(0, 1); the start perturbs cameras 1.. and the
points by `--sigma` N(0, 1).

`--rigid` times tsbb15_amd.tables.bundle_adjust_rigid (rs_bundle_adjust_rigid) on the same
table instead, the start turned into rotations by tests/ba_rigid_fixture.rigid_start
(Exp(sigma n) R, t + sigma n, X + sigma n), against tests/ba_rigid_ref.py, and writes
profiles/ba_rigid_bench.json.  The two problems take different LM paths: compare the time per
trial as well as per call.

`--loss NAME --f-scale X` (soft_l1, huber, cauchy) times the same table under a robust loss
(rs_bundle_adjust_robust) against tests/ba_robust_ref.py and writes
profiles/ba_robust_bench.json; with `--rigid` the rigid model.  The weights of each linearisation
are formed inside k_ba_linearize's slot, the final weights count in the last slot.

GPU figures: the wall time of whole calls (host clock around the synchronous call: upload, host
CSR build, LM loop, download), and, from a separate call with rs_ba_timing on, the device time
per kernel summed over the call (HIP events between the kernels).  Needs a GPU; there is no
fallback.  Writes one JSON file (default profiles/ba_bench.json) and prints it.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "tests"),
          os.path.join(REPO, "tsbb15-3d-reconstruction-project_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def dino_problem(nC=36, nP=676, noise=1e-4, sigma=1e-3, seed=0, rigid=False):
    z = np.load(os.path.join(REPO, "tests", "golden", "dino_pnp_kat.npz"))
    R, t, X = z["R"][:nC], z["t"][:nC], z["points3d"][:nP]
    cams = np.empty((nC, 3, 4))
    for k in range(nC):
        Rk = R[k] @ R[0].T
        cams[k, :, :3], cams[k, :, 3] = Rk, t[k] - Rk @ t[0]
    pts = X @ R[0].T + t[0]
    ov = np.array([(j % nC + s) % nC for j in range(nP) for s in range(2 + j % (nC - 1))],
                  dtype=np.int32)
    op = np.array([j for j in range(nP) for s in range(2 + j % (nC - 1))], dtype=np.int32)
    rng = np.random.RandomState(seed)
    perm = rng.permutation(len(ov))
    ov, op = ov[perm], op[perm]
    xh = np.hstack([pts[op], np.ones((len(op), 1))])
    y = np.einsum('nij,nj->ni', cams[ov], xh)
    uv = y[:, :2] / y[:, 2:3] + noise * rng.standard_normal((len(ov), 2))
    if rigid:
        import ba_rigid_fixture as rf
        cams0, pts0 = rf.rigid_start({"cams": cams, "pts": pts}, sigma, seed=seed)
        return cams0, pts0, ov, op, uv
    cams0, pts0 = cams.copy(), pts.copy()
    cams0[1:] += sigma * rng.standard_normal(cams0[1:].shape)
    pts0 += sigma * rng.standard_normal(pts0.shape)
    return cams0, pts0, ov, op, uv


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--repeats", type=int, default=5, help="timed GPU calls (after one warm-up)")
    ap.add_argument("--max-iter", type=int, default=200)
    ap.add_argument("--noise", type=float, default=1e-4)
    ap.add_argument("--sigma", type=float, default=1e-3)
    ap.add_argument("--no-oracle", action="store_true", help="skip the CPU oracle run")
    ap.add_argument("--rigid", action="store_true",
                    help="time bundle_adjust_rigid from a rigid start")
    ap.add_argument("--loss", default="linear", choices=("linear", "soft_l1", "huber", "cauchy"))
    ap.add_argument("--f-scale", type=float, default=3e-4, help="C of a robust --loss")
    ap.add_argument("--out", default=None,
                    help="default profiles/ba_bench.json, profiles/ba_rigid_bench.json with "
                         "--rigid, profiles/ba_robust_bench.json with a robust --loss")
    a = ap.parse_args()
    robust = a.loss != "linear"
    if a.out is None:
        a.out = os.path.join(REPO, "profiles", "ba_robust_bench.json" if robust else
                             "ba_rigid_bench.json" if a.rigid else "ba_bench.json")

    from tsbb15_amd import _ffi
    from tsbb15_amd import tables as gt
    if _ffi.device_count() < 1:
        raise SystemExit("bench_ba: no GPU visible")
    ctx = _ffi.default_context()
    cams0, pts0, ov, op, uv = dino_problem(noise=a.noise, sigma=a.sigma, rigid=a.rigid)
    entry = gt.bundle_adjust_rigid if a.rigid else gt.bundle_adjust
    if robust:
        def adjust(*args, **kw):
            c, p, info = entry(*args, loss=a.loss, f_scale=a.f_scale, **kw)
            info["weights_min"] = float(info.pop("weights").min())
            return c, p, info
    else:
        adjust = entry
    res = {"problem": {"cameras": len(cams0), "points": len(pts0), "observations": len(ov),
                       "reduced_system": (6 if a.rigid else 12) * (len(cams0) - 1),
                       "noise": a.noise, "sigma": a.sigma, "max_iter": a.max_iter,
                       "entry": entry.__name__}}
    if robust:
        res["problem"].update(loss=a.loss, f_scale=a.f_scale)
    print(f"bench_ba: {res['problem']}", flush=True)

    adjust(cams0, pts0, ov, op, uv, max_iter=a.max_iter, ctx=ctx)      # warm-up
    wall = []
    for _ in range(a.repeats):
        t0 = time.perf_counter()
        c1, p1, info = adjust(cams0, pts0, ov, op, uv, max_iter=a.max_iter, ctx=ctx)
        wall.append((time.perf_counter() - t0) * 1e3)
    _ffi.ba_timing(ctx, True)
    c2, p2, info2 = adjust(cams0, pts0, ov, op, uv, max_iter=a.max_iter, ctx=ctx)
    ms, trials = _ffi.ba_timing(ctx, False)
    assert c2.tobytes() == c1.tobytes() and p2.tobytes() == p1.tobytes() and info2 == info
    if a.rigid:
        R = c1[:, :, :3]
        res["max_RtR_minus_I"] = float(np.abs(np.einsum('kji,kjl->kil', R, R) - np.eye(3)).max())
    res["gpu"] = {"info": info, "trials": trials, "wall_ms": [round(w, 3) for w in wall],
                  "wall_ms_median": round(float(np.median(wall)), 3),
                  "wall_ms_per_trial": round(float(np.median(wall)) / max(trials, 1), 4),
                  "kernel_ms_sum": {k: round(v, 4) for k, v in ms.items()},
                  "kernel_ms_total": round(sum(ms.values()), 4),
                  "kernel_us_per_launch": {
                      k: round(1e3 * v / max(info["iterations"] if i < 3 else trials, 1), 2)
                      for i, (k, v) in enumerate(ms.items())}}
    print(f"bench_ba: gpu {res['gpu']}", flush=True)

    if not a.no_oracle:
        if robust:
            import ba_robust_ref as br

            def lm(*args, **kw):
                c, p, info = br.bundle_adjust_robust_lm(*args, loss=a.loss, f_scale=a.f_scale,
                                                        rigid=a.rigid, **kw)
                info["weights_min"] = float(info.pop("weights").min())
                return c, p, info
        elif a.rigid:
            import ba_rigid_ref as tr
            lm = tr.bundle_adjust_rigid_lm
        else:
            from oracle import tables_ref as tr
            lm = tr.bundle_adjust_lm
        t0 = time.perf_counter()
        _, _, iref = lm(cams0, pts0, ov, op, uv[:, 0], uv[:, 1], max_iter=a.max_iter)
        sec = time.perf_counter() - t0
        res["oracle_cpu"] = {"info": iref, "seconds": round(sec, 2),
                             "cost_rel_diff": abs(info["cost"] - iref["cost"]) / iref["cost"]}
        res["speedup_vs_oracle"] = round(sec * 1e3 / float(np.median(wall)), 1)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(res, sort_keys=True))


if __name__ == "__main__":
    main()
