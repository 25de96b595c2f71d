"""bench.py's timed loop (C2, Philox, runs back to back, the counting kernel timed on every
8th run) with what bench.py does not print: the plan's carry_stats() and recount_stats() over all
the runs, its lane_waits(), the prune_stats() of the last run and the count between the timing
events.  One JSON line (tools/carry_ab.sh and tools/nocheck_ab.sh collect them).

  python tools/carry_probe.py <label> [--steps 100 --warmup 200]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tsbb15-3d-reconstruction-project_amd")]

from tsbb15_amd import _ffi, synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("label")
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=200)
    args = ap.parse_args()
    n, H = 2000, 100_000
    ctx = _ffi.Context(0)
    p1, p2, _ = synth.two_view(n, 0.3, seed=1)
    plan = _ffi.F8Plan(ctx, n, H)
    plan.set_points(p1, p2)
    plan.set_timing(1, min(8, max(1, args.steps)))
    for i in range(args.warmup):
        plan.run(H, mode=_ffi.SAMPLER_PHILOX, seed=0xC2, hyp_offset=i * H)
    plan.result()
    ctx.synchronize()
    t0 = time.perf_counter()
    for i in range(args.steps):
        plan.run(H, mode=_ffi.SAMPLER_PHILOX, seed=0xC2, hyp_offset=(args.warmup + i) * H)
    r, _ = plan.result()
    ctx.synchronize()
    el = time.perf_counter() - t0
    rec = {"label": args.label, "probe": "carry", "steps": args.steps, "warmup": args.warmup,
           "value": H * args.steps / el, "ms_per_step": el / args.steps * 1e3,
           "count_ms": plan.kernel_ms(last_n=min(64, args.steps))["count_ms"],
           "best": [int(r.best_index), int(r.best_count)], "lane_waits": plan.lane_waits(),
           "prune_stats": plan.prune_stats()}
    try:
        rec["carry_stats"] = plan.carry_stats()
    except AttributeError:      # a library from before the carried bound (RSAMD_LIB)
        rec["carry_stats"] = None
    try:                        # [recounts at a flush, count launches of the last run]
        rec["recount_stats"] = list(plan.recount_stats())
    except AttributeError:      # a library from before the deferred recount
        rec["recount_stats"] = None
    try:                        # the point order: installed, points placed first, installs
        rec["order_stats"] = plan.order_stats()
    except AttributeError:      # a library from before the point order
        rec["order_stats"] = None
    plan.close()
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
