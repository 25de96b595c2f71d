"""Float64 numpy model of the F plan's pruned count: the exact prefix rule (a hypothesis is
dropped when its inlier count among the first K points plus the n - K points left cannot reach
L - 1) against the one-sided screening rule (a point of the prefix is a certified outlier when
e^2 > t^2 n1, n1 the squared length of the first epipolar line only; the hypothesis is dropped
when K - certified + (n - K) < L - 1).  No GPU: hypotheses are numpy 8-point samples through
oracle/ransac_ref.fmatrix_stls, so the figures are those of the rule, not of one Philox stream,
and the fp32 guard band is left out (it moves ~0.1 % of the cells).

  python tools/screen_model.py                  the tables for C2, C5 and the N = 257 pair
  python tools/screen_model.py inliers-first SEED...
      the pair of tests/test_gpu_f8_screen.py (N = 257, 60 % outliers, inliers first, a
      one-group sample, m = 0 and a least skip of 8 points, so that the weak L of 64
      hypotheses still prunes): per pair seed, 8 runs of 4096 hypotheses with L, K, c*, the
      largest upper bound c' = K - certified of a hypothesis past the sample, and whether
      K > c* and max c' > c* (the run in which a wrongly folded maximum would show)
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tsbb15-3d-reconstruction-project_amd")]

from oracle import ransac_ref  # noqa: E402
from tsbb15_amd import synth  # noqa: E402

T2 = ransac_ref.INLIER_THRESHOLD ** 2
SCREEN_VALU = 56.0 / 96.0   # SIMD cycles per point pair, screening loop / exact loop


def models(p1, p2, H, rs):
    n = p1.shape[1]
    F = np.empty((H, 3, 3))
    for h in range(H):
        idx = rs.choice(n, 8, replace=False)
        F[h] = ransac_ref.fmatrix_stls(p1[:, idx], p2[:, idx])
    return F


def cells(F, p1, p2, chunk=512):
    """(inlier, certified) boolean (H, n) planes: the exact test e^2 < t^2 min(n1, n2) and the
    one-sided outlier certificate e^2 > t^2 n1."""
    n = p1.shape[1]
    x1, x2 = np.vstack([p1, np.ones(n)]), np.vstack([p2, np.ones(n)])
    inl = np.empty((len(F), n), dtype=bool)
    cert = np.empty((len(F), n), dtype=bool)
    for s in range(0, len(F), chunk):
        Fc = F[s:s + chunk]
        l1 = Fc @ x2                              # (h, 3, n): a, b, l3
        l2 = np.transpose(Fc, (0, 2, 1)) @ x1     # c, d
        e2 = np.sum(l1 * x1, axis=1) ** 2
        n1 = l1[:, 0] ** 2 + l1[:, 1] ** 2
        n2 = l2[:, 0] ** 2 + l2[:, 1] ** 2
        with np.errstate(invalid="ignore"):
            inl[s:s + chunk] = e2 < T2 * np.minimum(n1, n2)
            cert[s:s + chunk] = e2 > T2 * n1
    return inl, cert


def window(n, L, m, min_skip):
    npad = (n + 7) // 8 * 8
    K = max(8, (n - L + m + 7) // 8 * 8)
    if L <= 1 or K > npad - min_skip:
        K = npad
    return K, npad


def rules(inl, cert, n, h0, m, min_skip):
    """L, K, and past the sample: survivors of either rule, the upper bounds c'."""
    full = inl.sum(1)
    L = int(full[:h0].max())
    K, npad = window(n, L, m, min_skip)
    pre = inl[h0:, :K].sum(1)
    cup = K - cert[h0:, :K].sum(1)
    need = L - 1 - (n - K)
    return L, K, npad, full, pre >= need, cup >= need, cup


def table(name, n, frac, seed, H, h0, bench_H, divs=(30, 20, 15, 12, 10)):
    p1, p2, _ = synth.two_view(n, frac, seed=seed)
    F = models(p1, p2, H, np.random.RandomState(1000 + seed))
    inl, cert = cells(F, p1, p2)
    print(f"{name}: synth.two_view({n}, {frac}, seed={seed}), {H} hypotheses, L from the "
          f"first {h0}")
    print(f"  certified outlier cells: exact rule {100 * (1 - inl.mean()):.1f} %, one-sided "
          f"{100 * cert.mean():.1f} %")
    s = 64.0 * 32 / bench_H   # the default sample's share of a bench run
    for d in divs:
        m = max(16, n // d)
        L, K, npad, full, ke, ko, _ = rules(inl, cert, n, h0, m, max(8, n // 8))
        fe, fo = ke.mean(), ko.mean()
        we = s + (1 - s) * (K / npad + fe * (npad - K) / npad)
        wo = s + (1 - s) * (SCREEN_VALU * K / npad + fo)
        print(f"  m = n/{d} = {m}: L {L} K {K} survivors exact {ke.sum()} ({100 * fe:.1f} %) "
              f"one-sided {ko.sum()} ({100 * fo:.1f} %) of {H - h0}; counting VALU / whole plane: "
              f"exact {we:.2f} one-sided {wo:.2f}")


def inliers_first(seeds, n=257, frac=0.60, H=4096, runs=8, m=0, min_skip=8):
    for seed in seeds:
        p1, p2, mask = synth.two_view(n, frac, seed=seed)
        order = np.argsort(~mask, kind="stable")
        q1, q2 = p1[:, order], p2[:, order]
        rs = np.random.RandomState(2000 + seed)
        hits = 0
        for r in range(runs):
            inl, cert = cells(models(q1, q2, H, rs), q1, q2)
            L, K, npad, full, _, ko, cup = rules(inl, cert, n, 64, m, min_skip)
            cstar = int(full.max())
            hit = K < npad and K > cstar and cup.max() > cstar
            hits += hit
            print(f"  seed {seed} run {r}: L {L} K {K} npad {npad} c* {cstar} max c' "
                  f"{int(cup.max())} survivors {int(ko.sum())} {'<-- K > c* and c_up > c*' if hit else ''}")
        print(f"seed {seed}: {hits} of {runs} runs with K > c* and max c' > c*")


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "inliers-first":
        inliers_first([int(a) for a in sys.argv[2:]] or [3])
    else:
        table("C2", 2000, 0.30, 1, 8192, 2048, 100_000)
        table("C5", 10_000, 0.60, 5, 4096, 2048, 1_000_000)
        table("pair", 257, 0.30, 3, 4096, 2048, 4096)
