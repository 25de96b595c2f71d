#!/usr/bin/env python
"""Time the tracking stage (tsbb15_amd.tracking, csrc/tracking.hip).

Input: the synthetic pair of tests/features_fixture.py at 576 x 720 (the Dino frame size, shift
(5, 3) plus a little noise) and 4838 features, the reference's track count, at random
fractional positions at least 40 px from the border; window 21, three levels, forward-backward
on, 30 iterations at most, eps 0.01.

GPU figures after `--warmup` calls, median / min / max of `--repeats` calls: `kernel_ms` per
slot of rs_tracking_timing (pyramid: both images' pyramids; forward; backward: device time
between HIP events, no upload, no download) and `wall_ms`, the host clock around the whole
synchronous call (upload, kernels, download, the Python shim).  `feature_iterations` counts the
level-0 iterations the call returned (forward pass), and `feature_iterations_per_second` divides
them by the forward slot: the levels above 0 iterate too and are not counted, so the rate
understates the work.  `scaling` repeats the call with 4 and 16 times the features (forward slot,
median of 5 calls after 2).  The restatement tests/tracking_ref.py is timed on the first
`--ref-features` features and compared bit for bit.  Needs a GPU; there is no fallback.  Writes
one JSON file (default profiles/tracking_bench.json) and prints it.
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


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--repeats", type=int, default=20, help="timed GPU calls")
    ap.add_argument("--warmup", type=int, default=3, help="untimed GPU calls before them")
    ap.add_argument("--features", type=int, default=4838)
    ap.add_argument("--window", type=int, default=21)
    ap.add_argument("--levels", type=int, default=3)
    ap.add_argument("--ref-features", type=int, default=200,
                    help="features the numpy restatement is run on (0: skip)")
    ap.add_argument("--scale-features", type=int, nargs="*", default=[19352, 77408],
                    help="larger feature counts whose forward launch is timed too")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "tracking_bench.json"))
    a = ap.parse_args()

    import features_fixture as fx
    from tsbb15_amd import _ffi, tracking
    if _ffi.device_count() < 1:
        raise SystemExit("bench_tracking: no GPU visible")
    h, w = 576, 720
    img0, img1 = fx.image_pair(h, w, 1)
    rs = np.random.RandomState(0)
    pts = np.vstack([rs.uniform(40, w - 41, a.features), rs.uniform(40, h - 41, a.features)])
    kw = dict(window=a.window, levels=a.levels, max_iter=30, eps=0.01, fb_tol=1.0)
    res = {"image": [h, w], "features": a.features, "window": a.window, "levels": a.levels,
           "max_iter": 30, "eps": 0.01, "fb_tol": 1.0, "repeats": a.repeats, "warmup": a.warmup}

    tracking.timing(1)
    for _ in range(a.warmup):
        out = tracking.track(img0, img1, pts, **kw)
    wall, slots = [], {k: [] for k in _ffi.TRACKING_STAGES}
    for _ in range(a.repeats):
        t0 = time.perf_counter()
        out = tracking.track(img0, img1, pts, **kw)
        wall.append((time.perf_counter() - t0) * 1e3)
        for k, v in tracking.timing(1).items():
            slots[k].append(v)
    tracking.timing(0)
    res["kernel_ms"] = {k: stats(v) for k, v in slots.items()}
    res["wall_ms"] = stats(wall)
    res["status_counts"] = dict(zip(("ok", "lost", "flat", "fb"),
                                    np.bincount(out.status, minlength=4).tolist()))
    ok = out.status == tracking.OK
    # the pixel (x, y) of image 0 is the pixel (x - dx, y - dy) of image 1
    err = np.abs(out.pos[:, ok] - pts[:, ok] + np.array(fx.SHIFT)[:, None]).max(axis=0)
    res["error_px"] = {"median": round(float(np.median(err)), 4),
                       "max": round(float(err.max()), 4)}
    res["feature_iterations"] = int(out.iters.sum())
    res["mean_iterations"] = round(float(out.iters.mean()), 3)
    fwd = res["kernel_ms"]["forward"]["median"]
    res["feature_iterations_per_second"] = round(res["feature_iterations"] / (fwd * 1e-3))
    res["window_pixel_iterations_per_second"] = round(
        res["feature_iterations"] * a.window * a.window / (fwd * 1e-3))

    # the same call with more features: how far one Dino-sized call is from filling the device
    res["scaling"] = []
    for n in a.scale_features:
        more = np.vstack([rs.uniform(40, w - 41, n), rs.uniform(40, h - 41, n)])
        tracking.timing(1)
        fwd_ms, its = [], 0
        for k in range(2 + 5):
            o = tracking.track(img0, img1, more, **kw)
            if k >= 2:
                fwd_ms.append(tracking.timing(1)["forward"])
                its = int(o.iters.sum())
        tracking.timing(0)
        m = float(np.median(fwd_ms))
        res["scaling"].append({"features": n, "forward_ms": round(m, 4),
                               "feature_iterations": its,
                               "feature_iterations_per_second": round(its / (m * 1e-3))})

    if a.ref_features > 0:
        import tracking_ref as ref
        k = min(a.ref_features, a.features)
        t0 = time.perf_counter()
        want = ref.track(img0, img1, pts[:, :k], **kw)
        res["numpy_cpu_seconds"] = round(time.perf_counter() - t0, 3)
        res["numpy_features"] = k
        res["equal_to_restatement"] = bool(all(
            np.ascontiguousarray(g[..., :k]).tobytes() == w_.tobytes()
            for g, w_ in zip(out, want)))

    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(res, sort_keys=True))


if __name__ == "__main__":
    main()
