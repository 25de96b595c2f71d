"""Lane A/B probes that bench.py has no switch for; each prints one JSON line (tools/overlap_ab.sh
runs them against RSAMD_LIB / RSAMD_OVERLAP settings and collects the lines).

  python tools/lane_probe.py timing0 <label> [--steps 100 --warmup 200]
      bench.py's timed loop (C2, Philox, runs back to back) with timing level 0: no event
      packets and no exclusive timed runs (bench.py itself always sets level 1)
  python tools/lane_probe.py batch <label> [--batch 3 --steps 300]
      the same runs issued `--batch` at a time with a result() after each batch (an odd batch
      swaps lane and buffer-set parity at every result())
  python tools/lane_probe.py c5 <label>
      bench.py's extras.c5_stress leg alone: N = 10 000, 1e6 hypotheses, run + result(), best of 3
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
    ap.add_argument("mode", choices=("timing0", "batch", "c5"))
    ap.add_argument("label")
    ap.add_argument("--steps", type=int, default=None)
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--batch", type=int, default=3)
    args = ap.parse_args()
    ctx = _ffi.Context(0)
    rec = {"label": args.label, "probe": args.mode}
    if args.mode == "c5":
        n, H = 10_000, 1_000_000
        p1, p2, _ = synth.two_view(n, 0.60, seed=5)
    else:
        n, H = 2000, 100_000
        p1, p2, _ = synth.two_view(n, 0.3, seed=1)
    plan = _ffi.F8Plan(ctx, n, H)
    plan.set_points(p1, p2)

    def run(i, seed=0xC2):
        plan.run(H, mode=_ffi.SAMPLER_PHILOX, seed=seed, hyp_offset=i * H)

    if args.mode == "c5":
        plan.run(H, mode=_ffi.SAMPLER_PHILOX, seed=0xC5)
        plan.result()
        ts = []
        for _ in range(3):
            t = time.perf_counter()
            plan.run(H, mode=_ffi.SAMPLER_PHILOX, seed=0xC5)
            r, _ = plan.result()
            ts.append((time.perf_counter() - t) * 1e3)
        rec.update(ms_best_of_3=min(ts), ms_all=ts)
    else:
        steps = args.steps or (100 if args.mode == "timing0" else 300)
        batch = steps if args.mode == "timing0" else args.batch
        if args.mode == "timing0":
            plan.set_timing(0, 1)
        else:
            plan.set_timing(1, 8)
        for i in range(args.warmup):
            run(i)
        plan.result()
        ctx.synchronize()
        t0 = time.perf_counter()
        i = 0
        while i < steps:
            for _ in range(min(batch, steps - i)):
                run(args.warmup + i)
                i += 1
            r, _ = plan.result()
        ctx.synchronize()
        el = time.perf_counter() - t0
        rec.update(steps=steps, warmup=args.warmup, batch=batch, value=H * steps / el,
                   ms_per_step=el / steps * 1e3)
    rec["best"] = [int(r.best_index), int(r.best_count)]
    try:
        rec["lane_waits"] = plan.lane_waits()
    except AttributeError:      # a library from before the counter (RSAMD_LIB)
        rec["lane_waits"] = None
    plan.close()
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
