// Plain records and sizes of the RANSAC-F path that the kernels, their launch interface and the
// host-only plan arithmetic (f8_sched.h) share: no function, nothing that needs a device compiler.
#pragma once

#include <stdint.h>

namespace rsd {

// One correspondence, AoS 32 B: left image (x1, y1) = p1 column, right image (x2, y2) = p2
// column (fun.getFFromLabCode(p1, p2), convention p1^T F p2 = 0, lab3.py:195-196).
struct Pt {
  double x1, y1, x2, y2;
};

// Similarity frame of the fp32 counting kernel: x~ = (x - c_i) / s per image i, one common
// scale s so both line-length terms scale by s^2 and the min() test is frame invariant.
struct Frame {
  double s, cx1, cy1, cx2, cy2;
};

// Per-hypothesis decision (k_f8_count32q): constants live with each model (G4,
// written by the solve); only the float64 re-test threshold is global.
struct GuardW {
  double thr2_px;
};

// Grid of the selection passes; the status buffer holds 4 words + kSelectBlocks counts.
constexpr int kSelectBlocks = 256;
constexpr int kStatusWords = 4 + kSelectBlocks;
// Per-run words of the pruned count (f8_kernels.h, PruneArgs)
constexpr int kPruneWords = 4;  // [0] cA (max count when K = npad), [1] survivors, [2] K, [3] L

// Result header of one F run, written by the tail into the run's pinned host slot (through the
// host mapping); S_RANSAC, n_inliers ints, goes to the slot's pinned list beside it.  The tail of a
// carried run that fell back selects nothing: it sets fell_back and leaves the other fields as they
// were (f8_plan.hip recounts such a run at the flush that reads it); every other tail clears it.
struct F8DevResult {
  double F[9];
  int64_t best_index;
  int64_t best_count;
  double best_std;
  double best_norm;
  int64_t max_count_fast;
  int64_t n_candidates;
  int64_t guard_mismatch;
  int64_t n_inliers;
  int64_t fell_back;
};

}  // namespace rsd
