// The point order of the F plan's pruned count (f8_kernels.hip above k_f8_count32q, "Point
// order"), decided on the host with no HIP call: the permutation that puts the points a winner
// rejected first, when a plan installs it, and where the ordered copies of the points lie.
// f8_plan.hip does the HIP calls; tests/f8_order_check.cpp checks the functions without a device.
#pragma once

#include <cstdint>

#include "f8_sched.h"

namespace rs::f8 {

// A winner with this many inliers or fewer orders nothing (8 points fit any model they sampled)
constexpr int64_t kOrderMinCount = 8;

// perm[i] = the caller's index of the point at position i of the ordered copy: the indices outside
// the winner's inlier list first, ascending, then those inside, ascending.  inl: the n_inl indices
// of S_RANSAC, best_count: the winner's count.  Returns the number of points placed first, and 0
// with perm the identity when there is nothing to order by: best_count <= kOrderMinCount, an empty
// list, no point outside it, or a list that is not n_inl distinct indices of [0, n) (never
// trusted: it comes from memory the device wrote).  mark: n bytes of scratch.
inline int64_t order_outliers_first(const int *inl, int64_t n_inl, int64_t best_count, int64_t n,
                                    int32_t *perm, unsigned char *mark) {
  for (int64_t i = 0; i < n; ++i) {
    perm[i] = static_cast<int32_t>(i);
    mark[i] = 0;
  }
  if (best_count <= kOrderMinCount || n_inl <= 0 || n_inl >= n || !inl) return 0;
  for (int64_t k = 0; k < n_inl; ++k) {
    const int64_t j = inl[k];
    if (j < 0 || j >= n || mark[j]) return 0;
    mark[j] = 1;
  }
  int64_t o = 0, first = n - n_inl;
  for (int64_t i = 0, in = first; i < n; ++i) perm[mark[i] ? in++ : o++] = static_cast<int32_t>(i);
  return first;
}

// Whether a read flush installs the order (plan_wait; both lanes are drained there and the last
// run's header is final, recounted if it fell back).  enabled: RSAMD_ORDER and the pruned fp32
// count; installed: already done since set_points; runs_since_points: runs issued on the resident
// points.  One run per set_points (the drop-in's calls) never pays for an install.
inline bool order_installs(bool enabled, bool installed, int64_t runs_since_points) {
  return enabled && !installed && runs_since_points > 1;
}

// The margin m of K = roundup8(n - L + m) while an order is installed: max(16, n / 60) instead of
// prune_numbers' max(16, n / 30), unless the environment gave one.  With the winner's outliers
// first a third as many hypotheses survive a given K, so a shorter prefix pays: sweep at C2 with
// the order on (profiles/order/ab.txt, bench value in 1e9 hypotheses/s, two rounds): m = 16 /
// n/60 / n/30 / n/20 / n/15 gave 1.675-1.685 / 1.778-1.812 / 1.728-1.745 / 1.694-1.703 /
// 1.684-1.701.  In the caller's order n / 60 loses (kPruneMarginDiv's sweep), so it holds only
// for the runs that read the ordered copy.  Any m is sound.
constexpr int kOrderMarginDiv = 60;
inline int order_margin(int margin, bool margin_given, int n, bool installed) {
  return installed && !margin_given ? std::max(16, n / kOrderMarginDiv) : margin;
}

// The ordered copies, behind the point arena's buffers in the same allocation (plan_layout's
// buffers end at a multiple of 256 bytes): the permutation, the AoS float64 points the re-test
// reads and the point-pair layout, each laid out as plan_layout lays out its own.
struct OrderBufs {
  int32_t *d_perm = nullptr;
  rsd::Pt *d_pts = nullptr;
  float4 *d_pts32q = nullptr;
  size_t bytes = 0;
};
inline void order_layout(OrderBufs &o, char *base, int64_t cap_n) {
  const size_t n = static_cast<size_t>(cap_n);
  Layout L;
  L.bind(base, nullptr);
  arena_put(L, n, o.d_perm);
  arena_put(L, n, o.d_pts);
  arena_put(L, (n + 7) / 8 * 8, o.d_pts32q);
  o.bytes = L.total();
}

}  // namespace rs::f8
