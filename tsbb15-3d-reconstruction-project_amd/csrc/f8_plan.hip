// F plans (include/rsamd.h "RANSAC-F"): one correspondence set resident in HBM, runs of H
// hypotheses issued back to back.  Replaces the fun.getFFromLabCode hypothesis loop
// (fun.py:298-328).
//
// Per-run buffer sets (kBufs) used in rotation.  A run is a serial chain on one stream
// ("lane"): rs_f8_plan_run(k) enqueues on its lane
//
//   k_f8_tail_solve  [selection tail of the lane's previous run | solve of run k]  (one launch)
//   k_f8_count32x    counts of run k (+ fused c*): one launch, or with the pruned count
//                    (RSAMD_PRUNE=1, the fp32 path) three in a row on the same lane -- sample,
//                    prefix, rest (f8_kernels.hip above k_f8_count32q) -- with no host decision
//                    and no event between them; a run whose lane last ran the same H and
//                    threshold over the same points (RSAMD_CARRY=1) has prefix, rest, check
//                    instead, its bound from that run's c* in the lane's carry word
//
// and leaves run k's tail pending on that lane: it rides along with the lane's next solve, or
// is flushed alone by rs_f8_plan_result / set_points / destroy (plan_flush, the only place the
// host waits).  The tail (candidates, reference statistics, replay, S_RANSAC; latency bound, a
// few busy workgroups) and the solve (latency bound, ~1.5 waves per SIMD) thus share the
// machine instead of running back to back.
//
// One lane (RSAMD_OVERLAP=0): every run on the context's stream, the tail of run k-1 with the
// solve of run k.
//
// Two lanes (RSAMD_OVERLAP=1): lane 0 is the context's stream, lane 1 a non-blocking stream the
// plan creates the first time a run is placed on it.  A run goes to lane 0 when nothing is in
// flight, otherwise to the lane the previous run did not use, so consecutive runs execute
// concurrently: while one lane's count drains, the other lane's solve and count workgroups
// take the freed wave slots.  In a back-to-back sequence run k + 4 reuses buffer set and
// pinned slot k % 4 on the lane of run k, and run k's tail rides with the solve of run k + 2,
// so stream order alone protects them: there is no cross-stream event on the hot path (each
// event or wait is a packet the command processor retires between kernels; r01: ~3.5 us
// each).  Where the alternation is broken (the parity entry points run on lane 0 behind their
// parse and drain lane 1 first), a run about to use a set whose last run went to the other
// lane, with no host wait for that lane since, waits on the host for it (the set guard; never
// in a Philox or host-tuple sequence, whatever the number of runs between two plan_flush
// calls: rs_f8_plan_lane_waits counts these waits).  A run that records timing events runs its count
// alone: its lane waits for the other lane's end before the first event, the other lane waits
// for the last one.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "host.h"
#include "device_math.h"
#include "f8_kernels.h"

namespace {

// Per-run device buffers; kBufs sets in rotation.
struct RunBufs {
  int lane = 0;                // the lane of the last run that used this set (set guard)
  int64_t last_run = -1;       // ... and that run's index
  double *d_F = nullptr;       // 9 x ld SoA models (float64)
  float *d_F32 = nullptr;      // 9 x ld SoA models in the unit frame (fp32 counting)
  int *d_counts = nullptr;     // fast counts
  int *d_tuples = nullptr;     // host tuples (parity mode)
  int *d_cand = nullptr;       // candidate hypothesis ids, per-block segments
  int *d_status = nullptr;     // [c*, n_candidates, ., ., per-block candidate counts]
  int *d_ccount = nullptr;
  int *d_cfast = nullptr;      // fast counts of the candidates (guard_mismatch diagnostic)
  int *d_spec = nullptr;       // per select block: S_RANSAC of its first candidate
  int *d_spec_j = nullptr;     // per select block: that candidate's local index, or -1
  double *d_cstd = nullptr, *d_cnorm = nullptr;
  rsd::F8DevResult *d_res = nullptr;
  int *d_gdone = nullptr;      // per-group finish counters (fused c* in k_f8_count32x)
  float4 *d_G4 = nullptr;      // per-hypothesis decision constants (k_f8_count32q)
  // pruned count: the run's words (rsd::kPruneWords), the survivor list, the rest stage's
  // per-group finish counters; staged: the set's last run went through the three stages
  int *d_pw = nullptr;
  int *d_surv = nullptr;
  int *d_gdone_b = nullptr;
  bool staged = false;
  // carried run (no sample; L from the lane's carry word): the check stage's counts, per-group
  // finish counters and c* word; carried: the set's last run was such a run
  int *d_counts_fb = nullptr;
  int *d_gdone_fb = nullptr;
  int *d_fbw = nullptr;
  bool carried = false;
  double thresh = 0.0;         // the last run's threshold (rs_f8_plan_counts' recount)
  // host tuples (parity mode fed from the host) are staged in a pinned buffer owned by the
  // set, so the caller's array may go away as soon as rs_f8_plan_run returns; ev_copy marks
  // the end of the H2D copy that last read it (waited for before the buffer is refilled)
  int *h_tuples = nullptr;
  int64_t cap_h_tuples = 0;
  hipEvent_t ev_copy = nullptr;
  bool copy_pending = false;
};

// rs_f8_plan::overlap (two lanes) unless RSAMD_OVERLAP is set: two lanes measured 8-9 % ahead
// of one in every interleaved bench run (profiles/lanes/ab.txt)
constexpr int kOverlapDefault = 1;
// rs_f8_plan::prune and the sample size unless RSAMD_PRUNE / RSAMD_PRUNE_SAMPLE are set; the
// margin and the least number of skipped points worth pruning for come from n
// (profiles/prune/ab.txt; swept again for the screening prefix stage, profiles/screen/ab.txt)
constexpr int kPruneDefault = 1;
constexpr int kPruneSampleDefault = 32;
constexpr int kPruneMarginDiv = 30;   // m = max(16, n / 30)
constexpr int kPruneMinSkipDiv = 8;   // prune only when at least n / 8 points are skipped
// rs_f8_plan::carry and the gap unless RSAMD_CARRY / RSAMD_CARRY_GAP are set: a lane's run takes
// L = (c* of the lane's previous run) - g, g = max(kCarryGapMin, n / kCarryGapDiv), instead of a
// sample's (above k_f8_count32q, "Carried bound").  profiles/carry/ab.txt, C2, two rounds, bench
// value in 1e9 hypotheses/s: g = n/50 / n/25 / n/16 / n/10 gave 1.705-1.713 / 1.647-1.671 /
// 1.628-1.641 / 1.558-1.575, no fallback in 298 carried runs at any of them, hence n / 50.  The
// floor is for small n, where c* spreads like sqrt(n) and not like n: tools/carry_model.py
// (profiles/carry/model.txt) has c* 160-170 over 8 runs at N = 257, one fallback in 7 at g = 5
// and none at 16 (the floor of the margin m)
constexpr int kCarryDefault = 1;
constexpr int kCarryGapDiv = 50;
constexpr int kCarryGapMin = 16;

int env_int(const char *name, int dflt) {
  const char *v = std::getenv(name);
  return v ? std::atoi(v) : dflt;
}

}  // namespace

struct rs_f8_plan {
  rs_ctx *ctx = nullptr;
  int64_t n = 0, max_hyp = 0, ld = 0;
  int64_t cap_n = 0;           // points the per-point buffers hold (>= n; plan_retarget)
  double *d_p12 = nullptr;     // staging (2,n) p1 then (2,n) p2
  rsd::Pt *d_pts = nullptr;    // AoS float64 points
  float4 *d_pts32q = nullptr;  // the same, point-pair layout (k_f8_count32q)
  // kBufs: with two lanes the sets of runs k and k-1 (solve / count) and of runs k-2 and k-3
  // (their tails ride with those solves) are live at once
  static constexpr int kBufs = 4, kSlots = 4, kEvRing = 64, kLanes = 2;
  RunBufs buf[kBufs];
  // Each run's tail writes its result header into its own pinned slot (through the host
  // mapping) and S_RANSAC into its buffer set's HBM result; rs_f8_plan_result waits for the
  // last run and copies S_RANSAC on demand.
  rsd::F8DevResult *h_slot[kSlots] = {};
  rsd::F8DevResult *h_slot_dev[kSlots] = {};
  int *h_inl[kSlots] = {};      // pinned S_RANSAC per slot (cap_n ints), written by the tail
  int *h_inl_dev[kSlots] = {};
  hipEvent_t ring[kEvRing][4] = {};  // count start/end; tail+solve launch start/end
  bool timed[kEvRing] = {};          // whether run r % kEvRing recorded its events
  int64_t runs = 0, last_H = 0;
  bool pending = false;              // stream work not yet waited for
  // Two lanes (RSAMD_OVERLAP=1; kOverlapDefault otherwise): consecutive runs alternate between
  // the context's stream (lane 0) and lane1, each lane a serial chain tail+solve -> count, so
  // one lane's solve and count fill the wave slots the other lane's count leaves idle.
  bool overlap = kOverlapDefault != 0;
  hipStream_t lane1 = nullptr;       // created when the first run is placed on it
  int last_lane = 0;                 // the lane of the last issued run
  bool busy[kLanes] = {};            // the lane has work the host has not waited for
  bool tail_pending[kLanes] = {};    // the lane's last run's tail is not enqueued yet
  rsd::TailArgs tail[kLanes] = {};   // ... its arguments
  // set guard: runs issued when the host last waited for the lane (every run of the lane below
  // that index is complete), and how often a run had to wait on the host for the other lane
  int64_t synced[kLanes] = {};
  int64_t lane_waits = 0;
  // timed runs count alone: ev_end marks the other lane's end before the run's first timing
  // event; excl[l] is the timed run's last event, which lane l waits for before its next launch
  hipEvent_t ev_end[kEvRing] = {};
  hipEvent_t excl[kLanes] = {};
  // counting kernel: fp32 point-pair kernel with the float64 guard re-test (default), or the
  // plain float64 kernel (rs_f8_plan_set_count_precision; both give identical counts)
  rsd::Frame frame{1.0, 0.0, 0.0, 0.0, 0.0};
  bool fp32_ok = false;       // finite points and a non-degenerate frame
  bool use_fp32 = true;
  // HIP timing events per run (each is a marker packet between kernels): 0 none, 1 around the
  // counting kernel (default; the bench's roofline timing), 2 also the tail+solve launch
  int timing = 1;
  int timing_every = 1;       // RSAMD_TIMING_EVERY / rs_f8_plan_set_timing: time every k-th run
  int q_waves = 6144;         // resident waves of the fp32 kernel (RSAMD_WAVES)
  int q_slices = 0;           // slices per resident wave (RSAMD_QSLICES; 0: count32q_shape)
  int tail_cus = 256;         // CUs shared by the tail + solve launch
  // Pruned count (fp32 path; derivation above k_f8_count32q): a full count of the first
  // prune_sample groups, the others screened over the prefix [0, K), a full count of the survivors.
  // RSAMD_PRUNE=0: the single whole-window launch.  Margin / min-skip below 0: from n
  // (prune_params)
  int prune = kPruneDefault;                // RSAMD_PRUNE
  int prune_sample = kPruneSampleDefault;   // RSAMD_PRUNE_SAMPLE: hypothesis groups of the sample
  int prune_margin = -1;                    // RSAMD_PRUNE_MARGIN: m of K = roundup8(n - L + m)
  int prune_min_skip = -1;                  // RSAMD_PRUNE_MINSKIP: prune only if >= this many points go
  // Carried bound (fp32 path, pruning on; derivation above k_f8_count32q): a run on a lane whose
  // previous run had the same H and threshold over the same points takes L from that run's c*,
  // left in d_carry[lane] by its tail, less the gap; no sample stage, a check stage that counts
  // everything again only if the bound turned out to be above c*.  carry_ok[l]: lane l's word
  // holds the c* of a run with carry_H / carry_thresh over the resident points
  int carry = kCarryDefault;                // RSAMD_CARRY
  int carry_gap = 0;                        // RSAMD_CARRY_GAP (may be negative: every run falls back)
  bool carry_gap_set = false;
  int *d_carry = nullptr;                   // kLanes carry words, then the fallback counter
  bool carry_ok[kLanes] = {};
  int64_t carry_H = 0;
  double carry_thresh = 0.0;
  int64_t n_carried = 0;                    // runs carried since the plan was created
  int *d_full = nullptr;      // rs_f8_plan_counts after a pruned run: the full counts (ld ints)
  int nospec = 0;             // RSAMD_NOSPEC=1 (test hook): the replay extracts S_RANSAC itself
  uint64_t *d_ts = nullptr;   // RSAMD_TSTAMP=<file>: wave timeline of the counting kernel
  const char *ts_path = nullptr;

  const RunBufs &last() const { return buf[(runs - 1) % kBufs]; }
};

static void plan_free(rs_f8_plan *p) {
  (void)hipFree(p->d_p12);
  (void)hipFree(p->d_pts);
  (void)hipFree(p->d_pts32q);
  (void)hipFree(p->d_full);
  (void)hipFree(p->d_carry);
  if (p->d_ts) {
    (void)rsd::set_count_timeline(nullptr);
    (void)hipFree(p->d_ts);
  }
  for (RunBufs &b : p->buf) {
    (void)hipFree(b.d_F);
    (void)hipFree(b.d_F32);
    (void)hipFree(b.d_counts);
    (void)hipFree(b.d_tuples);
    (void)hipFree(b.d_cand);
    (void)hipFree(b.d_status);
    (void)hipFree(b.d_ccount);
    (void)hipFree(b.d_cfast);
    (void)hipFree(b.d_spec);
    (void)hipFree(b.d_spec_j);
    (void)hipFree(b.d_cstd);
    (void)hipFree(b.d_cnorm);
    (void)hipFree(b.d_res);
    (void)hipFree(b.d_gdone);
    (void)hipFree(b.d_G4);
    (void)hipFree(b.d_pw);
    (void)hipFree(b.d_surv);
    (void)hipFree(b.d_gdone_b);
    (void)hipFree(b.d_counts_fb);
    (void)hipFree(b.d_gdone_fb);
    (void)hipFree(b.d_fbw);
    if (b.h_tuples) (void)hipHostFree(b.h_tuples);
    if (b.ev_copy) (void)hipEventDestroy(b.ev_copy);
  }
  for (auto &e : p->ev_end)
    if (e) (void)hipEventDestroy(e);
  if (p->lane1) (void)hipStreamDestroy(p->lane1);
  for (auto &h : p->h_slot)
    if (h) (void)hipHostFree(h);
  for (auto &h : p->h_inl)
    if (h) (void)hipHostFree(h);
  for (auto &r : p->ring)
    for (auto &e : r)
      if (e) (void)hipEventDestroy(e);
}

// the pinned S_RANSAC buffers of the result slots, cap ints each (the tail writes the winner's
// list through the host mapping; rs_f8_plan_result reads it without a copy)
static hipError_t alloc_h_inl(rs_f8_plan *p, int64_t cap) {
  hipError_t e = hipSuccess;
  for (int k = 0; k < rs_f8_plan::kSlots; ++k) {
    if (p->h_inl[k]) (void)hipHostFree(p->h_inl[k]);
    p->h_inl[k] = nullptr;
    p->h_inl_dev[k] = nullptr;
    if (e == hipSuccess)
      e = hipHostMalloc(reinterpret_cast<void **>(&p->h_inl[k]), sizeof(int) * static_cast<size_t>(cap));
    if (e == hipSuccess)
      e = hipHostGetDevicePointer(reinterpret_cast<void **>(&p->h_inl_dev[k]), p->h_inl[k], 0);
  }
  return e;
}

extern "C" int rs_f8_plan_create(rs_ctx *c, int64_t n, int64_t max_hyp, rs_f8_plan **out) {
  if (!c || !out) return fail(RS_EINVAL, "null pointer");
  *out = nullptr;
  if (n < 8) return fail(RS_EINVAL, "Cannot take a larger sample than population when 'replace=False'");
  if (n > (1LL << 30) || max_hyp < 1 || max_hyp > (1LL << 30))
    return fail(RS_EINVAL, "plan dimensions out of range");
  HIP_TRY(hipSetDevice(c->device));
  auto *p = new rs_f8_plan();
  p->ctx = c;
  p->n = n;
  p->cap_n = n;
  p->max_hyp = max_hyp;
  p->ld = (max_hyp + 63) / 64 * 64;
  const size_t res_bytes = sizeof(rsd::F8DevResult) + sizeof(int64_t) * static_cast<size_t>(n);
  if (const char *cm = std::getenv("RSAMD_COUNT"))  // tools: RSAMD_COUNT=fp64
    p->use_fp32 = std::strcmp(cm, "fp64") != 0;
  p->timing = env_int("RSAMD_TIMING", 1);
  p->timing_every = std::max(1, env_int("RSAMD_TIMING_EVERY", 1));
  {
    int cus = 256;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, c->device) != hipSuccess)
      cus = 256;
    p->tail_cus = cus;
    p->q_waves = std::max(1, env_int("RSAMD_WAVES", rsd::count32q_resident_waves(c->device)));
    p->q_slices = env_int("RSAMD_QSLICES", 0);
  }
  hipError_t e = hipSuccess;
#define ALLOC(ptr, bytes) \
  if (e == hipSuccess) e = hipMalloc(&(ptr), (bytes));
  ALLOC(p->d_p12, sizeof(double) * 4 * n);
  ALLOC(p->d_pts, sizeof(rsd::Pt) * n);
  ALLOC(p->d_pts32q, sizeof(float4) * ((n + 7) & ~7LL));
  for (RunBufs &b : p->buf) {
    ALLOC(b.d_F, sizeof(double) * 9 * p->ld);
    ALLOC(b.d_F32, sizeof(float) * 9 * p->ld);
    ALLOC(b.d_counts, sizeof(int) * p->ld);
    ALLOC(b.d_tuples, sizeof(int) * 8 * p->ld);
    ALLOC(b.d_cand, sizeof(int) * p->ld);
    ALLOC(b.d_status, sizeof(int) * rsd::kStatusWords);
    ALLOC(b.d_ccount, sizeof(int) * p->ld);
    ALLOC(b.d_cfast, sizeof(int) * p->ld);
    ALLOC(b.d_spec, sizeof(int) * rsd::kSelectBlocks * static_cast<size_t>(n));
    ALLOC(b.d_spec_j, sizeof(int) * rsd::kSelectBlocks);
    ALLOC(b.d_cstd, sizeof(double) * p->ld);
    ALLOC(b.d_cnorm, sizeof(double) * p->ld);
    ALLOC(b.d_res, res_bytes);
    ALLOC(b.d_gdone, sizeof(int) * (p->ld / 64));
    ALLOC(b.d_G4, sizeof(float4) * p->ld);
    ALLOC(b.d_pw, sizeof(int) * rsd::kPruneWords);
    ALLOC(b.d_surv, sizeof(int) * p->ld);
    ALLOC(b.d_gdone_b, sizeof(int) * (p->ld / 64));
    ALLOC(b.d_counts_fb, sizeof(int) * p->ld);
    ALLOC(b.d_gdone_fb, sizeof(int) * (p->ld / 64));
    ALLOC(b.d_fbw, sizeof(int));
  }
  ALLOC(p->d_carry, sizeof(int) * (rs_f8_plan::kLanes + 1));
  if (e == hipSuccess) e = hipMemset(p->d_carry, 0, sizeof(int) * (rs_f8_plan::kLanes + 1));
#undef ALLOC
  for (int k = 0; k < rs_f8_plan::kSlots; ++k) {
    if (e == hipSuccess)
      e = hipHostMalloc(reinterpret_cast<void **>(&p->h_slot[k]), sizeof(rsd::F8DevResult));
    if (e == hipSuccess)
      e = hipHostGetDevicePointer(reinterpret_cast<void **>(&p->h_slot_dev[k]), p->h_slot[k], 0);
  }
  if (e == hipSuccess) e = alloc_h_inl(p, p->cap_n);
  for (auto &r : p->ring)
    for (auto &ev : r)
      if (e == hipSuccess) e = hipEventCreate(&ev);
  p->overlap = env_int("RSAMD_OVERLAP", kOverlapDefault) != 0;
  p->nospec = env_int("RSAMD_NOSPEC", 0) != 0;
  p->prune = env_int("RSAMD_PRUNE", kPruneDefault) != 0;
  p->prune_sample = std::max(1, env_int("RSAMD_PRUNE_SAMPLE", kPruneSampleDefault));
  p->prune_margin = env_int("RSAMD_PRUNE_MARGIN", -1);
  p->prune_min_skip = env_int("RSAMD_PRUNE_MINSKIP", -1);
  p->carry = env_int("RSAMD_CARRY", kCarryDefault) != 0;
  p->carry_gap_set = std::getenv("RSAMD_CARRY_GAP") != nullptr;
  p->carry_gap = std::max(-(1 << 24), std::min(1 << 24, env_int("RSAMD_CARRY_GAP", 0)));
  p->ts_path = std::getenv("RSAMD_TSTAMP");
  if (p->ts_path) {
    p->overlap = false;  // one device-global timeline buffer: one counting launch at a time
    p->prune = 0;        // ... and one launch per run
    const size_t tsb = sizeof(uint64_t) * rsd::kCountTsWords * (static_cast<size_t>(p->q_waves) * 64 + 1024);
    if (hipMalloc(&p->d_ts, tsb) == hipSuccess) {
      (void)hipMemset(p->d_ts, 0, tsb);
      (void)rsd::set_count_timeline(p->d_ts);
    }
  }
  if (e != hipSuccess) {
    plan_free(p);
    delete p;
    return hip_fail(e, "rs_f8_plan_create");
  }
  *out = p;
  return RS_OK;
}

static int plan_flush(rs_f8_plan *p);

// The carry words no longer describe what the next run counts (new points, another counting
// kernel, another H or threshold): both lanes start again from a sample run
static void carry_drop(rs_f8_plan *p) {
  for (bool &ok : p->carry_ok) ok = false;
}

// A new population for an existing plan (the drop-in's calls, one pair after another): the
// per-point buffers are reallocated only when n exceeds what they hold; the per-hypothesis
// buffers, events and pinned slots are kept (a fresh plan allocates ~20 buffers)
static int plan_retarget(rs_f8_plan *p, int64_t n) {
  if (n < 8) return fail(RS_EINVAL, "Cannot take a larger sample than population when 'replace=False'");
  if (n > (1LL << 30)) return fail(RS_EINVAL, "plan dimensions out of range");
  int st = plan_flush(p);  // runs in flight read the resident points and results
  if (st) return st;
  if (n > p->cap_n) {
    const int64_t cap = std::max<int64_t>(n, p->cap_n + p->cap_n / 4);
    (void)hipFree(p->d_p12);
    (void)hipFree(p->d_pts);
    (void)hipFree(p->d_pts32q);
    p->d_p12 = nullptr;
    p->d_pts = nullptr;
    p->d_pts32q = nullptr;
    hipError_t e = hipMalloc(&p->d_p12, sizeof(double) * 4 * cap);
    if (e == hipSuccess) e = hipMalloc(&p->d_pts, sizeof(rsd::Pt) * cap);
    if (e == hipSuccess) e = hipMalloc(&p->d_pts32q, sizeof(float4) * ((cap + 7) & ~7LL));
    for (RunBufs &b : p->buf) {
      (void)hipFree(b.d_spec);
      (void)hipFree(b.d_res);
      b.d_spec = nullptr;
      b.d_res = nullptr;
      if (e == hipSuccess) e = hipMalloc(&b.d_spec, sizeof(int) * rsd::kSelectBlocks * static_cast<size_t>(cap));
      if (e == hipSuccess)
        e = hipMalloc(&b.d_res, sizeof(rsd::F8DevResult) + sizeof(int64_t) * static_cast<size_t>(cap));
    }
    if (e == hipSuccess) e = alloc_h_inl(p, cap);
    if (e != hipSuccess) {
      // the old buffers are gone: mark the plan empty (a later retarget reallocates) and let
      // the caller drop it (rs_f8_ransac_np destroys its cached plan)
      p->cap_n = 0;
      p->n = 0;
      return hip_fail(e, "rs_f8_plan retarget");
    }
    p->cap_n = cap;
  }
  p->n = n;
  p->fp32_ok = false;  // set_points decides it for the new points
  carry_drop(p);
  return RS_OK;
}

static hipStream_t lane_stream(const rs_f8_plan *p, int lane) {
  return lane == 0 ? p->ctx->stream : p->lane1;
}

// Lane 1, and the events that mark a lane's end for the timed runs, at the first run placed on
// it: a stream costs 15-30 ms to create, which single-run callers (rs_f8_ransac_np) never pay
static hipError_t ensure_lane1(rs_f8_plan *p) {
  if (p->lane1) return hipSuccess;
  hipError_t e = hipStreamCreateWithFlags(&p->lane1, hipStreamNonBlocking);
  for (auto &ev : p->ev_end)
    if (e == hipSuccess) e = hipEventCreateWithFlags(&ev, hipEventDisableTiming);
  if (e != hipSuccess) {  // all or nothing: a later run tries again from scratch
    for (auto &ev : p->ev_end) {
      if (ev) (void)hipEventDestroy(ev);
      ev = nullptr;
    }
    if (p->lane1) (void)hipStreamDestroy(p->lane1);
    p->lane1 = nullptr;
  }
  return e;
}

// The last event of a timed run on the other lane, if this lane has not waited for it yet
static hipError_t lane_excl_wait(rs_f8_plan *p, int lane) {
  hipError_t e = hipSuccess;
  if (p->excl[lane] && lane_stream(p, lane))
    e = hipStreamWaitEvent(lane_stream(p, lane), p->excl[lane], 0);
  p->excl[lane] = nullptr;
  return e;
}

// The lane's pending tail in a launch of its own (no next solve to ride along with)
static hipError_t lane_tail_alone(rs_f8_plan *p, int lane) {
  if (!p->tail_pending[lane]) return hipSuccess;
  hipError_t e = lane_excl_wait(p, lane);
  if (e == hipSuccess)
    e = rsd::launch_f8_tail_solve(&p->tail[lane], nullptr, lane_stream(p, lane));
  p->tail_pending[lane] = false;
  return e;
}

// Host wait for one lane, its pending tail included (the set guard and the parity entry points)
static hipError_t lane_drain(rs_f8_plan *p, int lane) {
  if (!p->busy[lane]) return hipSuccess;
  hipError_t e = lane_tail_alone(p, lane);
  if (e == hipSuccess) e = hipStreamSynchronize(lane_stream(p, lane));
  p->busy[lane] = false;
  p->synced[lane] = p->runs;
  ++p->lane_waits;
  return e;
}

// Enqueue both lanes' pending tails alone, then wait for both streams.
static int plan_flush(rs_f8_plan *p) {
  HIP_TRY(hipSetDevice(p->ctx->device));
  for (int l = 0; l < rs_f8_plan::kLanes; ++l) HIP_TRY(lane_tail_alone(p, l));
  if (p->busy[1]) HIP_TRY(hipStreamSynchronize(p->lane1));
  HIP_TRY(hipStreamSynchronize(p->ctx->stream));
  for (int l = 0; l < rs_f8_plan::kLanes; ++l) {
    p->busy[l] = false;
    p->excl[l] = nullptr;
    p->synced[l] = p->runs;
  }
  p->pending = false;
  return RS_OK;
}

extern "C" int rs_f8_plan_destroy(rs_f8_plan *p) {
  if (!p) return RS_OK;
  (void)plan_flush(p);
  plan_free(p);
  delete p;
  return RS_OK;
}

extern "C" int rs_f8_plan_set_points(rs_f8_plan *p, const double *p1, const double *p2) {
  if (!p || !p1 || !p2) return fail(RS_EINVAL, "null pointer");
  int st = plan_flush(p);  // runs in flight read the resident points
  if (st) return st;
  carry_drop(p);
  rs_ctx *c = p->ctx;
  const int64_t n = p->n;
  const size_t b = sizeof(double) * 2 * n;
  HIP_TRY(hipMemcpyAsync(p->d_p12, p1, b, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemcpyAsync(p->d_p12 + 2 * n, p2, b, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(rsd::launch_pack_points(p->d_p12, p->d_p12 + 2 * n, static_cast<int>(n), p->d_pts,
                                  c->stream));
  rsd::Frame fr{};
  p->fp32_ok = rsd::unit_frame(p1, p2, n, fr);
  if (p->fp32_ok) {
    p->frame = fr;
    HIP_TRY(rsd::launch_pack_points32q(p->d_pts, static_cast<int>(n), fr, p->d_pts32q,
                                       c->stream));
  }
  HIP_TRY(hipStreamSynchronize(c->stream));
  return RS_OK;
}

static int choose_chunk(const rs_f8_plan *p, int64_t H) {
  const int64_t groups = (H + 63) / 64;
  // aim for >= 8 units of work per SIMD (1024 SIMDs) without chunks below 64 points
  int64_t nchunks = (8192 + groups - 1) / groups;
  nchunks = std::max<int64_t>(1, std::min<int64_t>(nchunks, (p->n + 63) / 64));
  return static_cast<int>((p->n + nchunks - 1) / nchunks);
}

// The pruned count's arguments for buffer set b: the margin m = max(16, n / 30) and the least
// skip n / 8 (at least one block of 8 points) unless the environment gave them
static rsd::PruneArgs prune_args(const rs_f8_plan *p, const RunBufs &b) {
  const int n = static_cast<int>(p->n);
  rsd::PruneArgs pa{};
  pa.pw = b.d_pw;
  pa.surv = b.d_surv;
  pa.gdone_b = b.d_gdone_b;
  pa.g_first = std::min(p->prune_sample, 1 << 24);
  pa.margin = p->prune_margin >= 0 ? std::min(p->prune_margin, n) : std::max(16, n / kPruneMarginDiv);
  pa.min_skip = std::max(8, p->prune_min_skip >= 0 ? p->prune_min_skip : n / kPruneMinSkipDiv);
  if (b.carried) {  // no sample: every group is screened against the lane's carried bound
    pa.g_first = 0;
    pa.carry = p->d_carry + b.lane;
    pa.gap = p->carry_gap_set ? p->carry_gap : std::max(kCarryGapMin, n / kCarryGapDiv);
    pa.cf = b.d_status;
  }
  return pa;
}

// One run.  dev_tuples: tuple mode with the tuples already written (in range, by the GPU
// parity stream) into the buffer set this run uses, so there is no host copy or check.
static int plan_run(rs_f8_plan *p, int64_t H, int32_t mode, uint64_t seed, uint64_t hyp_offset,
                    const int32_t *host_tuples, double thresh, bool dev_tuples) {
  if (!p) return fail(RS_EINVAL, "null plan");
  if (H < 1 || H > p->max_hyp) return fail(RS_EINVAL, "hypothesis count out of plan range");
  if (mode != RS_SAMPLER_PHILOX && mode != RS_SAMPLER_TUPLES)
    return fail(RS_EINVAL, "unknown sampler mode");
  if (mode == RS_SAMPLER_TUPLES && !host_tuples && !dev_tuples)
    return fail(RS_EINVAL, "tuples required");
  if (!(thresh == thresh)) return fail(RS_EINVAL, "threshold is NaN");
  if (mode == RS_SAMPLER_TUPLES && !dev_tuples)
    for (int64_t i = 0; i < 8 * H; ++i)
      if (host_tuples[i] < 0 || host_tuples[i] >= p->n)
        return fail(RS_EINVAL, "tuple index out of range");
  rs_ctx *c = p->ctx;
  HIP_TRY(hipSetDevice(c->device));
  const int n = static_cast<int>(p->n), h = static_cast<int>(H);
  RunBufs &b = p->buf[p->runs % rs_f8_plan::kBufs];
  hipEvent_t *ev = p->ring[p->runs % rs_f8_plan::kEvRing];
  const int tl = (p->runs % p->timing_every == 0) ? p->timing : 0;  // this run's timing level
  p->timed[p->runs % rs_f8_plan::kEvRing] = tl >= 1;
  const int slot = static_cast<int>(p->runs % rs_f8_plan::kSlots);
  const bool fp32 = p->use_fp32 && p->fp32_ok;
  // lane choice: lane 0 when nothing is in flight, else the lane the previous run did not use;
  // device tuples were written on the context stream, so their run follows them on lane 0
  // (its entry point has drained lane 1 before the parse)
  int lane = 0;
  if (dev_tuples)
    HIP_TRY(lane_drain(p, 1));
  else if (p->overlap && p->pending)
    lane = 1 - p->last_lane;
  const int other = 1 - lane;
  if (lane == 1) HIP_TRY(ensure_lane1(p));
  hipStream_t ms = lane_stream(p, lane);
  // set guard: the set's last run went to the other lane and the host has not waited for that
  // lane since, so it may still be in flight there.  Taken only after a parity entry point broke
  // the alternation: in a Philox or host-tuple sequence the set's last run either used this
  // lane (stream order covers it) or preceded a plan_flush, after which lane and set parity may
  // differ from the recorded ones without any work left to wait for
  if (b.lane != lane && b.last_run >= p->synced[b.lane]) HIP_TRY(lane_drain(p, b.lane));
  b.lane = lane;
  b.last_run = p->runs;
  HIP_TRY(lane_excl_wait(p, lane));
  // a timed run counts alone: its lane waits here for the other lane's current end, and the
  // other lane waits for the run's last event before its next launch
  const bool excl = tl >= 1 && p->busy[other];
  hipEvent_t ev_end = excl ? p->ev_end[p->runs % rs_f8_plan::kEvRing] : nullptr;

  if (mode == RS_SAMPLER_TUPLES && !dev_tuples) {
    // stage through the set's pinned buffer: the copy no longer reads caller memory after
    // this call returns (the caller may free or reuse its tuples at once)
    if (b.copy_pending) {
      HIP_TRY(hipEventSynchronize(b.ev_copy));
      b.copy_pending = false;
    }
    if (b.cap_h_tuples < 8 * H) {
      if (b.h_tuples) HIP_TRY(hipHostFree(b.h_tuples));
      b.h_tuples = nullptr;
      b.cap_h_tuples = 0;
      HIP_TRY(hipHostMalloc(reinterpret_cast<void **>(&b.h_tuples), sizeof(int) * 8 * p->ld));
      b.cap_h_tuples = 8 * p->ld;
    }
    if (!b.ev_copy) HIP_TRY(hipEventCreateWithFlags(&b.ev_copy, hipEventDisableTiming));
    std::memcpy(b.h_tuples, host_tuples, sizeof(int) * 8 * H);
    HIP_TRY(hipMemcpyAsync(b.d_tuples, b.h_tuples, sizeof(int) * 8 * H, hipMemcpyHostToDevice,
                           ms));
    HIP_TRY(hipEventRecord(b.ev_copy, ms));
    b.copy_pending = true;
  }
  // [tail of the lane's previous run | solve of this run]: buffer set b was last used kBufs
  // runs back, on this lane (or on one drained above), and that run's tail precedes this
  // launch in stream order
  rsd::SolveArgs sa{};
  sa.pts = p->d_pts;
  sa.n = n;
  sa.H = h;
  sa.mode = mode;
  sa.seed = seed;
  sa.hyp_offset = hyp_offset;
  sa.tuples = b.d_tuples;
  sa.Fsoa = b.d_F;
  sa.ld = p->ld;
  sa.counts = b.d_counts;
  sa.status = b.d_status;
  sa.F32soa = fp32 ? b.d_F32 : nullptr;
  sa.frame = fp32 ? p->frame : rsd::Frame{1.0, 0.0, 0.0, 0.0, 0.0};
  sa.gdone = b.d_gdone;
  if (fp32) {
    const rsd::Bounds gb = rsd::fp32_bounds(p->frame, thresh);
    sa.G4 = b.d_G4;
    sa.gT = gb.thr2;
    sa.gDe = gb.De;
    sa.gDn = gb.Dn;
  }
  // the pruned count's stages, when the run has hypotheses past the sample
  const int h0 = static_cast<int>(std::min<int64_t>(H, 64LL * std::min(p->prune_sample, 1 << 24)));
  const bool staged = fp32 && p->prune && h0 < h;
  // ... without the sample when the lane's carry word holds the c* of a run like this one (the
  // decision is the host's alone: H and the threshold of the run that left the word)
  if (!(fp32 && H == p->carry_H && thresh == p->carry_thresh)) carry_drop(p);
  const bool carried = staged && p->carry && p->carry_ok[lane];
  b.staged = staged;
  b.carried = carried;
  b.thresh = thresh;
  if (staged) {
    sa.pw = b.d_pw;
    sa.gdone_b = b.d_gdone_b;
  }
  if (carried) {
    sa.counts_fb = b.d_counts_fb;
    sa.gdone_fb = b.d_gdone_fb;
    sa.fbw = b.d_fbw;
  }
  if (excl && tl >= 2) {
    HIP_TRY(hipEventRecord(ev_end, lane_stream(p, other)));
    HIP_TRY(hipStreamWaitEvent(ms, ev_end, 0));
  }
  if (tl >= 2) HIP_TRY(hipEventRecord(ev[2], ms));
  HIP_TRY(rsd::launch_f8_tail_solve(p->tail_pending[lane] ? &p->tail[lane] : nullptr, &sa, ms,
                                    p->tail_cus));
  p->tail_pending[lane] = false;
  if (tl >= 2) HIP_TRY(hipEventRecord(ev[3], ms));

  // counts of this run
  if (excl && tl == 1) {
    HIP_TRY(hipEventRecord(ev_end, lane_stream(p, other)));
    HIP_TRY(hipStreamWaitEvent(ms, ev_end, 0));
  }
  if (tl >= 1) HIP_TRY(hipEventRecord(ev[0], ms));
  if (carried) {
    // prefix of every group against L = the lane's carry word - gap -> the survivors over the
    // whole window (c_f in status[0]) -> check: everything again into the set's fallback storage
    // if c_f < L, else an empty launch of one slice per resident wave; all on the device
    const rsd::GuardW gw{thresh * thresh};
    const rsd::PruneArgs pa = prune_args(p, b);
    const rsd::Count32qShape sh1 = rsd::count32q_shape(n, h, p->q_waves, p->q_slices);
    HIP_TRY(rsd::launch_f8_count32q_prefix(p->d_pts32q, p->d_pts, n, h, b.d_F32, b.d_F, p->ld, sh1,
                                           gw, b.d_counts, ms, b.d_gdone, b.d_status, b.d_G4, pa));
    HIP_TRY(rsd::launch_f8_count32q_rest(p->d_pts32q, p->d_pts, n, h, b.d_F32, b.d_F, p->ld,
                                         p->q_waves, sh1, gw, b.d_counts, ms, b.d_status, b.d_G4, pa));
    const rsd::Count32qShape shc = rsd::count32q_shape(n, h, p->q_waves, 1);
    HIP_TRY(rsd::launch_f8_count32q_check(p->d_pts32q, p->d_pts, n, h, b.d_F32, b.d_F, p->ld, shc,
                                          gw, b.d_counts_fb, ms, b.d_gdone_fb, b.d_fbw, b.d_G4, pa));
    ++p->n_carried;
  } else if (staged) {
    // sample (whole window, c* of its groups = L in status[0]) -> prefix [0, K) of the other
    // groups screened, K from L on the device, survivors listed -> the survivors over the whole
    // window; all three in stream order on this lane, no host decision
    const rsd::GuardW gw{thresh * thresh};
    const rsd::Count32qShape sh0 = rsd::count32q_shape(n, h0, p->q_waves, p->q_slices);
    HIP_TRY(rsd::launch_f8_count32q(p->d_pts32q, p->d_pts, n, h0, b.d_F32, b.d_F, p->ld, sh0, gw,
                                    b.d_counts, ms, b.d_gdone, b.d_status, b.d_G4));
    const rsd::PruneArgs pa = prune_args(p, b);
    const rsd::Count32qShape sh1 = rsd::count32q_shape(n, h - h0, p->q_waves, p->q_slices);
    HIP_TRY(rsd::launch_f8_count32q_prefix(p->d_pts32q, p->d_pts, n, h, b.d_F32, b.d_F, p->ld, sh1,
                                           gw, b.d_counts, ms, b.d_gdone, b.d_status, b.d_G4, pa));
    HIP_TRY(rsd::launch_f8_count32q_rest(p->d_pts32q, p->d_pts, n, h - h0, b.d_F32, b.d_F, p->ld,
                                         p->q_waves, sh1, gw, b.d_counts, ms, b.d_status, b.d_G4, pa));
  } else if (fp32) {
    // fused c*: the chunk that completes a hypothesis group folds its max into status[0]
    const rsd::Count32qShape sh = rsd::count32q_shape(n, h, p->q_waves, p->q_slices);
    HIP_TRY(rsd::launch_f8_count32q(p->d_pts32q, p->d_pts, n, h, b.d_F32, b.d_F, p->ld, sh,
                                    rsd::GuardW{thresh * thresh}, b.d_counts, ms, b.d_gdone,
                                    b.d_status, b.d_G4));
  } else {
    HIP_TRY(rsd::launch_f8_count(p->d_pts, n, h, b.d_F, p->ld, choose_chunk(p, H),
                                 thresh * thresh, b.d_counts, ms));
    HIP_TRY(rsd::launch_f8_max(b.d_counts, h, b.d_status, ms));
  }
  if (tl >= 1) HIP_TRY(hipEventRecord(ev[1], ms));
  if (tl >= 1 && p->overlap) p->excl[other] = ev[1];

  // this run's tail rides along with the lane's next solve (or plan_flush)
  rsd::TailArgs &ta = p->tail[lane];
  ta = rsd::TailArgs{};
  ta.pts = p->d_pts;
  ta.n = n;
  ta.H = h;
  ta.slack = 1;
  ta.Fsoa = b.d_F;
  ta.ld = p->ld;
  ta.counts = b.d_counts;
  ta.status = b.d_status;
  ta.thresh = thresh;
  ta.cand = b.d_cand;
  ta.ccount = b.d_ccount;
  ta.cfast = b.d_cfast;
  ta.spec = b.d_spec;
  ta.spec_j = b.d_spec_j;
  ta.nospec = p->nospec;
  ta.cstd = b.d_cstd;
  ta.cnorm = b.d_cnorm;
  ta.res = b.d_res;
  ta.hres = p->h_slot_dev[slot];
  ta.hinl = p->h_inl_dev[slot];
  if (fp32) {  // this run's c* for the lane's next run, should that be one like it
    ta.carry = p->d_carry + lane;
    p->carry_H = H;
    p->carry_thresh = thresh;
    p->carry_ok[lane] = true;
  }
  if (carried) {
    ta.pw = b.d_pw;
    ta.counts_fb = b.d_counts_fb;
    ta.fbw = b.d_fbw;
    ta.n_fb = p->d_carry + rs_f8_plan::kLanes;
  }
  p->tail_pending[lane] = true;
  p->busy[lane] = true;
  p->last_lane = lane;
  ++p->runs;
  p->last_H = H;
  p->pending = true;
  return RS_OK;
}

extern "C" int rs_f8_plan_run(rs_f8_plan *p, int64_t H, int32_t mode, uint64_t seed,
                              uint64_t hyp_offset, const int32_t *host_tuples, double thresh) {
  return plan_run(p, H, mode, seed, hyp_offset, host_tuples, thresh, false);
}

// Parity mode with the numpy stream sampled on the GPU (np_sampler.hip) straight into the
// tuple buffer of the run about to be issued; advances (key, pos).  The sampler is synchronous
// on the context stream, and that buffer set was last read by the solve of run k-kBufs, which
// precedes it in stream order on lane 0 or ran on lane 1, drained here.  Populations beyond the GPU parse's range (and RSAMD_NP_HOST, a test
// hook) go through the host replay.
extern "C" int rs_f8_plan_run_np_slice(rs_f8_plan *p, int64_t H, int64_t start, int64_t count,
                                       uint32_t *key, int32_t *pos, double thresh) {
  if (!p || !key || !pos) return fail(RS_EINVAL, "null pointer");
  if (H < 1 || start < 0 || count < 1 || start + count > H)
    return fail(RS_EINVAL, "hypothesis slice out of range");
  if (count > p->max_hyp) return fail(RS_EINVAL, "hypothesis count out of plan range");
  int st;
  if (rs::np_gpu_supported(p->n, 8) && std::getenv("RSAMD_NP_HOST") == nullptr) {
    // the parse writes the run's tuples on the context stream: lane 1 is drained first (its
    // last run may have used this set), the run follows the parse on lane 0
    HIP_TRY(hipSetDevice(p->ctx->device));
    HIP_TRY(lane_drain(p, 1));
    if (start == 0 && count == H && std::getenv("RSAMD_NP_SYNC") == nullptr) {
      // the whole draw in one segment: the run is queued behind the parse before the host
      // waits for the parse's outcome (no host gap between them); should the parse ask to be
      // drawn again (a wrap-log overflow), that run is superseded by the synchronous path below
      bool queued = false;
      RunBufs &b = p->buf[p->runs % rs_f8_plan::kBufs];
      if ((st = rs::np_choice_enqueue(p->ctx, key, *pos, p->n, 8, H, b.d_tuples, &queued)))
        return st;
      if (queued) {
        const int run_st = plan_run(p, count, RS_SAMPLER_TUPLES, 0, 0, nullptr, thresh, true);
        bool rerun = false;
        if ((st = rs::np_choice_finish(p->ctx, key, pos, &rerun))) return st;
        if (run_st || !rerun) return run_st;
      }
    }
    RunBufs &b = p->buf[p->runs % rs_f8_plan::kBufs];
    if ((st = rs::np_choice_device(p->ctx, key, pos, p->n, 8, H, b.d_tuples, false, start, count)))
      return st;
    return plan_run(p, count, RS_SAMPLER_TUPLES, 0, static_cast<uint64_t>(start), nullptr, thresh,
                    true);
  }
  std::vector<int32_t> tuples(static_cast<size_t>(8 * H));
  if ((st = rs_np_choice_tuples(key, pos, p->n, 8, H, tuples.data()))) return st;
  return plan_run(p, count, RS_SAMPLER_TUPLES, 0, static_cast<uint64_t>(start),
                  tuples.data() + 8 * start, thresh, false);
}

// This rank's hypotheses [base, hi) of a sharded parse (rs_np_shard_*, step 4) straight into
// the tuple buffer of the run about to be issued, then that run; a rank holding no
// hypothesis only reads the final state (final_idx >= 0).  Candidate indices are run-local.
extern "C" int rs_f8_plan_run_np_shard(rs_f8_plan *p, rs_np_shard *sh, int64_t base, int64_t hi,
                                       int64_t next_start, int64_t final_idx, uint32_t *key_out,
                                       int32_t *pos_out, double thresh) {
  if (!p || !sh) return fail(RS_EINVAL, "null pointer");
  const int64_t count = hi - base;
  if (count > p->max_hyp) return fail(RS_EINVAL, "hypothesis count out of plan range");
  RunBufs &b = p->buf[p->runs % rs_f8_plan::kBufs];
  HIP_TRY(hipSetDevice(p->ctx->device));
  HIP_TRY(lane_drain(p, 1));  // the tuples are written on the context stream (lane 0)
  int st;
  if ((st = rs::np_shard_tuples_device(sh, base, hi, next_start, final_idx,
                                       count > 0 ? b.d_tuples : nullptr, key_out, pos_out)))
    return st;
  if (count < 1) return RS_OK;
  return plan_run(p, count, RS_SAMPLER_TUPLES, 0, static_cast<uint64_t>(base), nullptr, thresh, true);
}

extern "C" int rs_f8_plan_run_np(rs_f8_plan *p, int64_t H, uint32_t *key, int32_t *pos,
                                 double thresh) {
  return rs_f8_plan_run_np_slice(p, H, 0, H, key, pos, thresh);
}

// Complete the last run (its pending tail) and wait.  Accessors below then read its buffer
// set synchronously.
static int plan_wait(rs_f8_plan *p) {
  if (p->runs == 0) return fail(RS_EINVAL, "no run has been issued on this plan");
  return p->pending ? plan_flush(p) : RS_OK;
}

extern "C" int rs_f8_plan_result(rs_f8_plan *p, rs_f8_result *out, int64_t *inliers, int64_t cap,
                                 int64_t *n_inliers) {
  if (!p || !out) return fail(RS_EINVAL, "null pointer");
  int st = plan_wait(p);
  if (st) return st;
  const rsd::F8DevResult *r = p->h_slot[(p->runs - 1) % rs_f8_plan::kSlots];
  std::memcpy(out->F, r->F, sizeof(out->F));
  out->best_index = r->best_index;
  out->best_count = r->best_count;
  out->best_std = r->best_std;
  out->best_norm = r->best_norm;
  out->max_count_fast = r->max_count_fast;
  out->n_candidates = r->n_candidates;
  out->guard_mismatch = r->guard_mismatch;
  if (p->d_ts && p->ts_path) {  // diagnostics: append this run's wave timeline
    std::vector<uint64_t> t(rsd::kCountTsWords * (static_cast<size_t>(p->q_waves) * 64 + 1024));
    if (hipMemcpy(t.data(), p->d_ts, sizeof(uint64_t) * t.size(), hipMemcpyDeviceToHost) ==
        hipSuccess) {
      if (FILE *f = std::fopen(p->ts_path, "ab")) {
        std::fwrite(t.data(), sizeof(uint64_t), t.size(), f);
        std::fclose(f);
      }
    }
  }
  if (n_inliers) *n_inliers = r->n_inliers;
  const int64_t k = std::min<int64_t>(cap, r->n_inliers);
  if (inliers && k > 0) {
    const int *h = p->h_inl[(p->runs - 1) % rs_f8_plan::kSlots];  // written by the tail
    if (!h) return fail(RS_EINVAL, "the plan's buffers are gone (a failed retarget)");
    for (int64_t i = 0; i < k; ++i) inliers[i] = h[i];
  }
  return RS_OK;
}

extern "C" int rs_f8_plan_candidates(rs_f8_plan *p, rs_f8_candidate *out, int64_t cap,
                                     int64_t *n_out) {
  if (!p || !n_out) return fail(RS_EINVAL, "null pointer");
  int st = plan_wait(p);
  if (st) return st;
  const RunBufs &b = p->last();
  const int H = static_cast<int>(p->last_H);
  int pb = 0;  // the select-block layout the tail used (status word 3)
  HIP_TRY(hipMemcpy(&pb, b.d_status + 3, sizeof(int), hipMemcpyDeviceToHost));
  if (pb < 1) return fail(RS_EINVAL, "no selection layout recorded for the last run");
  const int nb = (H + pb - 1) / pb;
  std::vector<int> bc(nb);
  HIP_TRY(hipMemcpy(bc.data(), b.d_status + 4, sizeof(int) * nb, hipMemcpyDeviceToHost));
  std::vector<int> cand, cc;
  std::vector<double> cs, cn;
  for (int k = 0; k < nb; ++k) {
    if (bc[k] == 0) continue;
    const size_t o = cand.size(), m = static_cast<size_t>(bc[k]);
    const int64_t seg = static_cast<int64_t>(k) * pb;
    cand.resize(o + m);
    cc.resize(o + m);
    cs.resize(o + m);
    cn.resize(o + m);
    HIP_TRY(hipMemcpy(&cand[o], b.d_cand + seg, sizeof(int) * m, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(&cc[o], b.d_ccount + seg, sizeof(int) * m, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(&cs[o], b.d_cstd + seg, sizeof(double) * m, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(&cn[o], b.d_cnorm + seg, sizeof(double) * m, hipMemcpyDeviceToHost));
  }
  int cmax = 0;
  for (int v : cc) cmax = std::max(cmax, v);
  int64_t k = 0;
  for (size_t i = 0; i < cand.size(); ++i) {
    if (cc[i] != cmax || cmax == 0) continue;
    if (out && k < cap) {
      rs_f8_candidate &o = out[k];
      o.index = cand[i];
      o.count = cc[i];
      o.std_d = cs[i];
      o.norm_d = cn[i];
      for (int q = 0; q < 9; ++q)
        HIP_TRY(hipMemcpy(&o.F[q], b.d_F + q * p->ld + cand[i], sizeof(double),
                          hipMemcpyDeviceToHost));
    }
    ++k;
  }
  *n_out = k;
  return RS_OK;
}

// Whether the last run (complete: after plan_wait) was carried and fell back, by the test the
// check stage and the tail made on the device (carry_fell_back in f8_kernels.hip)
static int last_fell_back(rs_f8_plan *p, bool *fb) {
  const RunBufs &b = p->last();
  *fb = false;
  if (!b.carried) return RS_OK;
  int pw[rsd::kPruneWords] = {}, cf = 0;
  HIP_TRY(hipMemcpy(pw, b.d_pw, sizeof(pw), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(&cf, b.d_status, sizeof(int), hipMemcpyDeviceToHost));
  *fb = pw[2] < (p->n + 7) / 8 * 8 && cf < pw[3];
  return RS_OK;
}

extern "C" int rs_f8_plan_counts(rs_f8_plan *p, int32_t *counts, int64_t H) {
  if (!p || !counts) return fail(RS_EINVAL, "null pointer");
  int st = plan_wait(p);
  if (st) return st;
  if (H > p->last_H) return fail(RS_EINVAL, "H exceeds the last run");
  const RunBufs &b = p->last();
  const int *src = b.d_counts;
  int pw[rsd::kPruneWords] = {};
  if (b.staged) HIP_TRY(hipMemcpy(pw, b.d_pw, sizeof(pw), hipMemcpyDeviceToHost));
  const int n = static_cast<int>(p->n);
  bool fb = false;
  if ((st = last_fell_back(p, &fb))) return st;
  if (fb) {
    src = b.d_counts_fb;  // the check stage counted every hypothesis in full
  } else if (b.staged && pw[2] < (n + 7) / 8 * 8) {
    // a pruned run leaves prefix upper bounds for the hypotheses it dropped: the full counts come
    // from the whole-window kernel over the run's models, still in the buffer set (a
    // diagnostic accessor; nothing else is in flight after plan_wait)
    HIP_TRY(hipSetDevice(p->ctx->device));
    if (!p->d_full) HIP_TRY(hipMalloc(&p->d_full, sizeof(int) * p->ld));
    hipStream_t s = p->ctx->stream;
    const int h = static_cast<int>(p->last_H);
    HIP_TRY(hipMemsetAsync(p->d_full, 0, sizeof(int) * p->ld, s));
    const rsd::Count32qShape sh = rsd::count32q_shape(n, h, p->q_waves, p->q_slices);
    HIP_TRY(rsd::launch_f8_count32q(p->d_pts32q, p->d_pts, n, h, b.d_F32, b.d_F, p->ld, sh,
                                    rsd::GuardW{b.thresh * b.thresh}, p->d_full, s, nullptr,
                                    nullptr, b.d_G4));
    HIP_TRY(hipStreamSynchronize(s));
    src = p->d_full;
  }
  HIP_TRY(hipMemcpy(counts, src, sizeof(int) * H, hipMemcpyDeviceToHost));
  return RS_OK;
}

extern "C" int rs_f8_plan_stage_counts(rs_f8_plan *p, int32_t *counts, int64_t H) {
  if (!p || !counts) return fail(RS_EINVAL, "null pointer");
  int st = plan_wait(p);
  if (st) return st;
  if (H > p->last_H) return fail(RS_EINVAL, "H exceeds the last run");
  bool fb = false;
  if ((st = last_fell_back(p, &fb))) return st;
  HIP_TRY(hipMemcpy(counts, fb ? p->last().d_counts_fb : p->last().d_counts, sizeof(int) * H,
                    hipMemcpyDeviceToHost));
  return RS_OK;
}

extern "C" int rs_f8_plan_carry_stats(rs_f8_plan *p, int64_t *out) {
  if (!p || !out) return fail(RS_EINVAL, "null pointer");
  int st = plan_wait(p);
  if (st) return st;
  bool fb = false;
  if ((st = last_fell_back(p, &fb))) return st;
  int nfb = 0;
  HIP_TRY(hipMemcpy(&nfb, p->d_carry + rs_f8_plan::kLanes, sizeof(int), hipMemcpyDeviceToHost));
  out[0] = p->n_carried;
  out[1] = nfb;
  out[2] = p->last().carried ? 1 : 0;
  out[3] = fb ? 1 : 0;
  return RS_OK;
}

extern "C" int rs_f8_plan_prune_stats(rs_f8_plan *p, int64_t *out) {
  if (!p || !out) return fail(RS_EINVAL, "null pointer");
  int st = plan_wait(p);
  if (st) return st;
  const RunBufs &b = p->last();
  const int64_t npad = (p->n + 7) / 8 * 8;
  if (b.staged) {
    int pw[rsd::kPruneWords] = {};
    HIP_TRY(hipMemcpy(pw, b.d_pw, sizeof(pw), hipMemcpyDeviceToHost));
    out[0] = pw[3];
    out[1] = pw[2];
    out[2] = pw[1];
  } else {  // one whole-window launch: its c*, nothing skipped, nobody past a sample
    int cmax = 0;
    HIP_TRY(hipMemcpy(&cmax, b.d_status, sizeof(int), hipMemcpyDeviceToHost));
    out[0] = cmax;
    out[1] = npad;
    out[2] = 0;
  }
  out[3] = npad;
  return RS_OK;
}

extern "C" int rs_f8_plan_models(rs_f8_plan *p, double *F_out, int64_t H) {
  if (!p || !F_out) return fail(RS_EINVAL, "null pointer");
  int st = plan_wait(p);
  if (st) return st;
  if (H > p->last_H) return fail(RS_EINVAL, "H exceeds the last run");
  std::vector<double> soa(static_cast<size_t>(9 * H));
  for (int k = 0; k < 9; ++k)
    HIP_TRY(hipMemcpy(soa.data() + k * H, p->last().d_F + k * p->ld, sizeof(double) * H,
                      hipMemcpyDeviceToHost));
  for (int64_t h = 0; h < H; ++h)
    for (int k = 0; k < 9; ++k) F_out[h * 9 + k] = soa[k * H + h];
  return RS_OK;
}

extern "C" int rs_f8_plan_kernel_avg(rs_f8_plan *p, int64_t last_n, double *score_ms,
                                     double *solve_ms, double *total_ms) {
  if (!p) return fail(RS_EINVAL, "null plan");
  int st = plan_wait(p);
  if (st) return st;
  if (p->timing < 1) return fail(RS_EINVAL, "timing events are disabled (RSAMD_TIMING=0)");
  const int64_t k = std::max<int64_t>(
      1, std::min<int64_t>({last_n, p->runs, static_cast<int64_t>(rs_f8_plan::kEvRing)}));
  double sa = 0, sb = 0, sc = 0;
  int64_t nt = 0;
  for (int64_t r = p->runs - k; r < p->runs; ++r) {
    if (!p->timed[r % rs_f8_plan::kEvRing]) continue;
    ++nt;
    hipEvent_t *ev = p->ring[r % rs_f8_plan::kEvRing];
    float a = 0, b = 0, t = 0;
    HIP_TRY(hipEventElapsedTime(&b, ev[0], ev[1]));  // counting kernel
    if (p->timing >= 2) {
      HIP_TRY(hipEventElapsedTime(&a, ev[2], ev[3]));  // previous tail + this solve
      HIP_TRY(hipEventElapsedTime(&t, ev[2], ev[1]));  // tail+solve start .. count end
    }
    sa += a;
    sb += b;
    sc += t;
  }
  if (nt == 0) return fail(RS_EINVAL, "no timed run among the requested ones");
  // the solve / whole-run times need timing level 2; reported as -1 otherwise
  if (solve_ms) *solve_ms = p->timing >= 2 ? sa / nt : -1.0;
  if (score_ms) *score_ms = sb / nt;
  if (total_ms) *total_ms = p->timing >= 2 ? sc / nt : -1.0;
  return RS_OK;
}

extern "C" int rs_f8_plan_set_count_precision(rs_f8_plan *p, int32_t fp64) {
  if (!p) return fail(RS_EINVAL, "null plan");
  int st = plan_flush(p);  // runs in flight use the current kernel's buffers
  if (st) return st;
  p->use_fp32 = fp64 == 0;
  carry_drop(p);
  return RS_OK;
}

extern "C" int rs_f8_plan_set_timing(rs_f8_plan *p, int32_t level, int32_t every) {
  if (!p) return fail(RS_EINVAL, "null plan");
  if (level < 0 || level > 2 || every < 1) return fail(RS_EINVAL, "bad timing level / period");
  p->timing = level;
  p->timing_every = every;
  return RS_OK;
}

extern "C" int rs_f8_plan_lane_waits(rs_f8_plan *p, int64_t *waits) {
  if (!p || !waits) return fail(RS_EINVAL, "null pointer");
  *waits = p->lane_waits;
  return RS_OK;
}

extern "C" int rs_f8_plan_kernel_ms(rs_f8_plan *p, double *score_ms, double *solve_ms,
                                    double *total_ms) {
  return rs_f8_plan_kernel_avg(p, 1, score_ms, solve_ms, total_ms);
}

// ------------------------------------------------------------------------------------------
// numpy-exact one call (fun.getFFromLabCode loop)
// ------------------------------------------------------------------------------------------
extern "C" int rs_f8_ransac_np(rs_ctx *c, const double *p1, const double *p2, int64_t n,
                               int64_t H, uint32_t *mt_key, int32_t *mt_pos, double thresh,
                               rs_f8_result *out, int64_t *inliers, int64_t cap,
                               int64_t *n_inliers) {
  if (!c || !p1 || !p2 || !mt_key || !mt_pos || !out) return fail(RS_EINVAL, "null pointer");
  if (n < 8)
    return fail(RS_EINVAL, "Cannot take a larger sample than population when 'replace=False'");
  if (H < 1) return fail(RS_EINVAL, "hypothesis count must be positive");
  if (c->np_plan && c->np_plan->max_hyp < H) {
    rs_f8_plan_destroy(c->np_plan);
    c->np_plan = nullptr;
  }
  int st;
  if (!c->np_plan && (st = rs_f8_plan_create(c, n, H, &c->np_plan))) return st;
  // another pair's population: the same plan, its per-point buffers grown if need be
  if (c->np_plan->n != n && (st = plan_retarget(c->np_plan, n))) {
    // a failed reallocation leaves the per-point buffers freed: drop the plan, so that the next
    // call builds a fresh one instead of running on null buffers
    rs_f8_plan_destroy(c->np_plan);
    c->np_plan = nullptr;
    return st;
  }
  if ((st = rs_f8_plan_set_points(c->np_plan, p1, p2))) return st;
  uint32_t key[RS_MT_N];
  int32_t pos = *mt_pos;
  std::memcpy(key, mt_key, sizeof(key));
  if ((st = rs_f8_plan_run_np(c->np_plan, H, key, &pos, thresh))) return st;
  if ((st = rs_f8_plan_result(c->np_plan, out, inliers, cap, n_inliers))) return st;
  std::memcpy(mt_key, key, sizeof(key));
  *mt_pos = pos;
  return RS_OK;
}
