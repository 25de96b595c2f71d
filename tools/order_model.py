"""Float64 numpy model of the F plan's point order: how many hypotheses survive the screening
prefix of a carried run when the points stand in the caller's order, and when the points that a
previous run's winner rejected stand first (csrc/f8_order.h, order_outliers_first).  Built on
tools/screen_model.py: numpy 8-point samples, the one-sided certificate e^2 > t^2 n1, no fp32
guard band.  The bound is the carried one, L = c* - max(16, n / 50), c* the best full count of the
hypotheses screened; the winner whose inlier set orders the points is the best of the first half
of the hypotheses, as a previous run would have delivered it.  A hypothesis survives when
K - (certified outliers among the first K points of the order) + (n - K) >= L - 1.

The work figure is the counting VALU in units of the whole exact plane (an unpruned single launch
is 1.0): the screening loop over K of npad points at 56 / 96 of the exact loop's cycles, plus the
survivors over the whole window.

  python tools/order_model.py        C2, C5, the N = 257 / 256 pairs of the tests and the
                                     inliers-first pair of tests/test_gpu_f8_screen.py
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import screen_model as sm  # noqa: E402
from tsbb15_amd import synth  # noqa: E402


def outliers_first(inl_winner):
    """The permutation of f8::order_outliers_first: indices outside the list ascending, then those
    inside ascending."""
    idx = np.arange(len(inl_winner))
    return np.concatenate([idx[~inl_winner], idx[inl_winner]])


def survivors(cert, order, n, K, L):
    cup = K - cert[:, order[:K]].sum(1)
    return cup + (n - K) >= L - 1


def row(inl, cert, n, m, min_skip, label):
    full = inl.sum(1)
    cstar = int(full.max())
    L = cstar - max(16, n // 50)
    K, npad = sm.window(n, L, m, min_skip)
    H = len(full)
    half = full[:H // 2]
    w = int(half.argmax())
    ident = np.arange(n)
    arms = {"given": ident, "outliers first": outliers_first(inl[w]),
            "inliers first": outliers_first(~inl[w])}
    out = []
    for name, order in arms.items():
        if K >= npad:
            keep = np.ones(H, bool)
        else:
            keep = survivors(cert, order, n, K, L)
            assert keep[full >= L - 1].all()      # the rule is sound in any order
        f = keep.mean()
        work = sm.SCREEN_VALU * K / npad + f if K < npad else 1.0
        out.append(f"{name} {int(keep.sum())} ({100 * f:.2f} %) work {work:.3f}")
    print(f"  {label}: winner {int(half.max())} of c* {cstar}, L {L} K {K} of npad {npad}, "
          f"{int((full >= 400).sum()) if n >= 2000 else int((full >= L - 1).sum())} "
          f"{'with count >= 400' if n >= 2000 else 'with count >= L - 1'}; survivors of {H}: "
          + "; ".join(out))


def config(name, n, frac, seed, H, divs, arrange=None):
    p1, p2, mask = synth.two_view(n, frac, seed=seed)
    if arrange is not None:
        o = arrange(mask)
        p1, p2 = p1[:, o], p2[:, o]
    F = sm.models(p1, p2, H, np.random.RandomState(1000 + seed))
    inl, cert = sm.cells(F, p1, p2)
    print(f"{name}: synth.two_view({n}, {frac}, seed={seed}), {H} hypotheses")
    for d in divs:
        row(inl, cert, n, max(16, n // d), max(8, n // 8), f"m = n/{d} = {max(16, n // d)}")


if __name__ == "__main__":
    config("C2", 2000, 0.30, 1, 6144, (60, 30, 20, 15))
    config("C5", 10_000, 0.60, 5, 1536, (30,))
    config("pair N = 257", 257, 0.30, 3, 4096, (30,))
    config("pair N = 256", 256, 0.30, 3, 4096, (30,))
    config("inliers-first pair N = 257 (60 % outliers, the true inliers first)", 257, 0.60, 3, 4096,
           (30,), arrange=lambda mask: np.argsort(~mask, kind="stable"))
