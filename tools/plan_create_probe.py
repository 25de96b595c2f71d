"""Median wall time of rs_f8_plan_create + rs_f8_plan_destroy (one JSON line).  The library under
test is the one RSAMD_LIB names, as for bench.py."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..",
                                "tsbb15-3d-reconstruction-project_amd"))
from tsbb15_amd import _ffi  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=3000)
ap.add_argument("--max-hyp", type=int, default=4000)
ap.add_argument("--repeats", type=int, default=20)
ap.add_argument("--label", default="")
a = ap.parse_args()
ctx = _ffi.default_context()
_ffi.F8Plan(ctx, a.n, a.max_hyp).close()  # the first call loads the code object
ms = []
for _ in range(a.repeats):
    t0 = time.perf_counter()
    _ffi.F8Plan(ctx, a.n, a.max_hyp).close()
    ms.append((time.perf_counter() - t0) * 1e3)
print(json.dumps({"label": a.label, "bench": "plan_create_destroy", "n": a.n, "max_hyp": a.max_hyp,
                  "repeats": a.repeats, "median_ms": statistics.median(ms), "min_ms": min(ms),
                  "max_ms": max(ms)}))
