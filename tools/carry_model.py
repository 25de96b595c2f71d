"""Float64 numpy model of the F plan's carried bound (f8_kernels.hip above k_f8_count32q,
"Carried bound"): a run screens every hypothesis against L = (c* of an earlier run over the same
points) - g instead of the best full count of a 2048-hypothesis sample, and is counted again in
full when its own c* turns out to be below L.  Built on tools/screen_model.py (models, cells,
window; the same one-sided certificate, no fp32 guard band).  No GPU.

Per configuration R independent runs of numpy-sampled hypotheses give the spread of c*; run r is
then screened against L = c*(run r - 1) - g for g = n/50, n/25, n/16, n/10 (and against its own
sample's L, today's rule), over its first `screened` hypotheses: K, survivors, the counting VALU as
a fraction of the whole plane, and whether the run would have fallen back (c* < L).  A run of the
model is `run_H` hypotheses; where that is below the bench's H it says so: the maximum of fewer
draws spreads more, so the fallback figures are then pessimistic.

  python tools/carry_model.py [C2|C5|pair ...]      (profiles/carry/model.txt is its output)
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tsbb15-3d-reconstruction-project_amd")]

from tools.screen_model import SCREEN_VALU, cells, models, window  # noqa: E402
from tsbb15_amd import synth  # noqa: E402

DIVS = (50, 25, 16, 10)
CONFIGS = {
    # name: n, outlier fraction, pair seed, bench H, model run H, runs, hypotheses screened
    "C2": (2000, 0.30, 1, 100_000, 100_000, 8, 8192),
    "C5": (10_000, 0.60, 5, 1_000_000, 100_000, 4, 4096),
    "pair": (257, 0.30, 3, 4096, 4096, 8, 4096),
}


def screen(inl, cert, n, L, m, min_skip):
    """K, npad and the survivors of the one-sided rule against L."""
    K, npad = window(n, L, m, min_skip)
    if K == npad:
        return K, npad, np.zeros(len(inl), dtype=bool)
    cup = K - cert[:, :K].sum(1)
    return K, npad, cup + (n - K) >= L - 1


def config(name):
    n, frac, seed, bench_H, run_H, runs, screened = CONFIGS[name]
    p1, p2, _ = synth.two_view(n, frac, seed=seed)
    rs = np.random.RandomState(3000 + seed)
    m, min_skip = max(16, n // 30), max(8, n // 8)
    cstar, planes = [], []
    for r in range(runs):
        F = models(p1, p2, run_H, rs)
        full = np.zeros(run_H, dtype=np.int64)
        for s in range(0, run_H, 4096):
            inl, cert = cells(F[s:s + 4096], p1, p2)
            full[s:s + 4096] = inl.sum(1)
            if s == 0:
                planes.append((inl[:screened].copy(), cert[:screened].copy()))
        cstar.append(int(full.max()))
    print(f"{name}: synth.two_view({n}, {frac}, seed={seed}), {runs} runs of {run_H} hypotheses "
          f"(bench H {bench_H}), {screened} screened per run, m {m}, least skip {min_skip}")
    print(f"  c* per run: {cstar}, spread {max(cstar) - min(cstar)}")
    share = 64.0 * 32 / bench_H   # the default sample's share of a bench run
    rows = [("sample", None)] + [(f"g = n/{d} = {max(1, n // d)}", max(1, n // d)) for d in DIVS]
    for label, g in rows:
        Ks, sv, valu, fb = [], [], [], 0
        for r in range(1, runs):
            inl, cert = planes[r]
            if g is None:
                L = int(inl[:2048].sum(1).max())
            else:
                L = cstar[r - 1] - g
                fb += cstar[r] < L
            K, npad, keep = screen(inl, cert, n, L, m, min_skip)
            f = keep.mean()
            w = SCREEN_VALU * K / npad + f if K < npad else 1.0
            Ks.append(K)
            sv.append(100 * f)
            valu.append(share + (1 - share) * w if g is None else w)
        print(f"  {label}: K {min(Ks)}-{max(Ks)} survivors {min(sv):.1f}-{max(sv):.1f} % counting "
              f"VALU / whole plane {min(valu):.3f}-{max(valu):.3f}"
              + ("" if g is None else f" fallbacks {fb} of {runs - 1}"))


if __name__ == "__main__":
    for name in sys.argv[1:] or list(CONFIGS):
        config(name)
