// Launch interface of the RANSAC-F / PnP kernels (host side).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "device_math.h"

#define RSD_SAMPLER_PHILOX 0
#define RSD_SAMPLER_TUPLES 1

namespace rsd {

constexpr int kTailThreads = 512;  // workgroup of the fused tail + solve launch

// One run's solve (k_f8_solve / the solve half of k_f8_tail_solve).
struct SolveArgs {
  const Pt *pts;
  int n, H, mode;
  uint64_t seed, hyp_offset;
  const int *tuples;
  double *Fsoa;
  int64_t ld;
  int *counts;   // zeroed per hypothesis
  int *status;   // status words 0..3 zeroed
  float *F32soa; // unit-frame fp32 models (null: fp64 counting)
  Frame frame;
  int *gdone;    // per-group finish counters zeroed (fused c*)
  float4 *G4;    // per-hypothesis decision constants (k_f8_count32q), may be null
  double gT, gDe, gDn;  // their inputs: (t/s)^2 and the fp32 error bounds of e and m
  int *pw;       // pruned count: the run's kPruneWords words zeroed, may be null
  int *gdone_b;  // ... and the rest stage's per-group finish counters
};

// One run's selection tail (candidates, reference statistics, replay, S_RANSAC).
struct TailArgs {
  const Pt *pts;
  int n, H, slack, per_block;
  const double *Fsoa;
  int64_t ld;
  const int *counts;
  int *status;   // [c*, n_candidates, done counter, spare, per-block candidate counts]
  double thresh;
  int *cand, *ccount;
  int *cfast;          // fast count of each candidate (guard_mismatch without a gather)
  int *spec, *spec_j;  // per block: S_RANSAC of its first candidate (n ints), that index
  int nospec;          // RSAMD_NOSPEC=1: no speculative lists (the replay extracts S_RANSAC)
  double *cstd, *cnorm;
  F8DevResult *hres;  // pinned host header slot (device mapping)
  int *hinl;          // pinned host S_RANSAC (int32, device mapping)
  int *carry;         // the lane's carry word: the run's c* is left there, may be null
  // carried run: the prune words, the set's fallback storage (the whole count of every
  // hypothesis and its c* word, filled by the plan's recount) and the plan's fallback counter; all
  // null otherwise.  When the run fell back (carry_fell_back) the tail selects nothing: it marks
  // hres, counts the fallback and leaves the run's c_f in the carry word.  recount: the second
  // pass over such a run, after the recount: c* and the counts from the fallback storage
  const int *pw, *counts_fb, *fbw;
  int *n_fb;
  int recount;
};

hipError_t launch_pack_points(const double *p1, const double *p2, int n, Pt *pts,
                              hipStream_t s);
hipError_t launch_f8_solve(const Pt *pts, int n, int H, int mode, uint64_t seed,
                           uint64_t hyp_offset, const int *tuples, double *Fsoa, int64_t ld,
                           int *counts, int *status, hipStream_t s, float *F32soa = nullptr,
                           const Frame *frame = nullptr, int *gdone = nullptr);
// Point-pair packed fp32 counting (guard band + float64 re-test: counts bit-identical to
// launch_f8_count); ptsq in the k_pack_points32q layout.
hipError_t set_count_timeline(uint64_t *buf);  // RSAMD_TSTAMP diagnostics (null: off)
// words per wave of that timeline: real-time start / end, re-tests, HW_ID | XCC_ID,
// shader-clock start / end
constexpr int kCountTsWords = 6;
hipError_t launch_pack_points32q(const Pt *pts, int n, const Frame &fr, float4 *ptsq,
                                 hipStream_t s);
// Both of the count kernel's point arrays gathered through perm, a permutation of [0, n):
// pts_out[i] = pts[perm[i]] and ptsq the pair layout of pts_out (the plan's point order)
hipError_t launch_pack_points32q_perm(const Pt *pts, const int *perm, int n, const Frame &fr,
                                      Pt *pts_out, float4 *ptsq, hipStream_t s);
struct Count32qShape {
  int64_t per_wave;  // points of the (group, point) plane per wave (a multiple of 8)
  int64_t blocks;    // 256-thread workgroups launched
};
int count32q_resident_waves(int device);
// fp32 counting set-up (host): guard bounds of the unit frame, and the frame of the points
struct Bounds {
  double u, De, Dn, thr2;
};
Bounds fp32_bounds(const Frame &fr, double thresh);
bool unit_frame(const double *p1, const double *p2, int64_t n, Frame &fr);
Count32qShape count32q_shape(int n, int H, int waves, int slices_per_wave = 0);
hipError_t preload_f8();  // the F-RANSAC kernels' code object onto the current device
// pts (and with fr the point-pair layout ptsq) from the (2, n) arrays in one launch
hipError_t launch_pack_points_both(const double *p1, const double *p2, int n, Pt *pts,
                                   const Frame *fr, float4 *ptsq, hipStream_t s);
// Pruned count (derivation above k_f8_count32q): after a full count of the first g_first
// hypothesis groups has left L in status[0], the prefix stage screens the other groups over the
// points [0, K) only (certified outliers, no inlier count), K from L on the device, and lists
// the hypotheses that can still reach L - 1 (surv); the rest stage counts those over the whole
// window through the list.  The run's words: kPruneWords (f8_types.h).
struct PruneArgs {
  int *pw;       // the run's words
  int *surv;     // survivor hypothesis ids (ld ints)
  int *gdone_b;  // the rest stage's per-group finish counters
  int g_first;   // hypothesis groups counted in full by the sample stage
  int margin;    // m: K = roundup8(n - L + m)
  int min_skip;  // fewer points than this to skip: K = npad, nothing is pruned
  // carried run: L = *carry - gap instead of status[0] (null: the sample's L)
  const int *carry;
  int gap;
};
// What one launch of k_f8_count32q reads and writes.  counts / gdone / status are the stage's
// own: the recount of a carried run that fell back takes the set's fallback storage (counts_fb,
// gdone_fb and the word fbw) there.  gdone and status may be null (no fused c*), Hdev too (H
// hypotheses).
struct CountArgs {
  const float4 *ptsq;
  const Pt *pts;
  int n, H;
  const float *F32soa;
  const double *Fsoa;
  int64_t ld;
  GuardW g;
  int *counts, *gdone, *status;
  const float4 *G4;
  const int *Hdev;
};
// The stages (k_f8_count32q's MODE).  kCountWhole: H hypotheses over the whole window, pa unused.
// kCountPrefix: sh is the shape of the groups past pa.g_first over the whole window (the stage
// cuts its slices from K on the device), H the run's hypothesis count.  kCountRest: the survivors
// over the whole window; the grid is sized for `waves` resident waves (the survivor count is on
// the device), at most the grid of sh, the shape of the H hypotheses the prefix stage screened.
constexpr int kCountWhole = 0, kCountPrefix = 1, kCountRest = 2;
hipError_t launch_f8_count32q(int mode, const CountArgs &a, const Count32qShape &sh, int waves,
                              const PruneArgs &pa, hipStream_t s);
hipError_t launch_f8_count(const Pt *pts, int n, int H, const double *Fsoa, int64_t ld,
                           int chunk, double thr2, int *counts, hipStream_t s,
                           const int *Hdev = nullptr, const int *Hmap = nullptr);
// Selection tail: c* (k_f8_max, unless the counting kernel fused it), candidates + reference
// statistics + (last block) replay and S_RANSAC.  Candidates live in per-block segments of
// `cand`.
int select_per_block(int H);
int select_blocks(int H);
hipError_t launch_f8_max(const int *counts, int H, int *status, hipStream_t s);
// Tail of one run and/or solve of the next in one launch (either may be null).
hipError_t launch_f8_tail_solve(TailArgs *ta, SolveArgs *sa, hipStream_t s,
                                int tail_cus = 0);
hipError_t launch_residuals(const Pt *pts, int n, const double *F, double *out, hipStream_t s);

}  // namespace rsd
