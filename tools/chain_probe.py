"""Per-run wall time of back-to-back Philox runs over the C2 points for several H, 100 runs after
200, best of 3: `issue` is the host's time to enqueue the runs, `total` includes the wait for the
last one.  With a small H the device work vanishes and what is left of `total` is the floor of the
lanes' launch chains, which is where a launch taken off the chain shows; at the bench's H the two
lanes' kernels compete for the machine and the chain is not the only bound.  One JSON line per H
(tools/nocheck_ab.sh collects them).

  python tools/chain_probe.py <label>
"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tsbb15-3d-reconstruction-project_amd")]
from tsbb15_amd import _ffi, synth  # noqa: E402

label = sys.argv[1]
n = 2000
ctx = _ffi.Context(0)
p1, p2, _ = synth.two_view(n, 0.3, seed=1)
for H in (100_000, 50_000, 25_000, 4096):
    plan = _ffi.F8Plan(ctx, n, H)
    plan.set_points(p1, p2)
    plan.set_timing(1, 8)
    for i in range(200):
        plan.run(H, mode=_ffi.SAMPLER_PHILOX, seed=0xC2, hyp_offset=i * H)
    plan.result()
    ctx.synchronize()
    best = None
    for rep in range(3):
        t0 = time.perf_counter()
        for i in range(100):
            plan.run(H, mode=_ffi.SAMPLER_PHILOX, seed=0xC2, hyp_offset=(200 + i) * H)
        t1 = time.perf_counter()
        plan.result()
        ctx.synchronize()
        t2 = time.perf_counter()
        r = ((t1 - t0) * 1e4, (t2 - t0) * 1e4)
        best = r if best is None or r[1] < best[1] else best
    print(json.dumps({"label": label, "probe": "chain", "H": H, "issue_us_per_run": round(best[0], 2),
                      "total_us_per_run": round(best[1], 2)}))
    plan.close()
