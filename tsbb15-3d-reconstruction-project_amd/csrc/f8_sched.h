// What an F plan (f8_plan.hip) decides on the host, with no HIP call: where its buffers lie in
// its arenas, which lane a run takes and which host waits that costs, how the run is counted, and
// the numbers of the pruned count.  f8_plan.hip does the HIP calls these decisions ask for;
// tests/f8_sched_check.cpp checks them without a device.
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstdlib>

#include "f8_types.h"
#include "host.h"

namespace rs::f8 {

constexpr int kBufs = 4, kSlots = 4, kLanes = 2;

// Per-run device buffers; kBufs sets in rotation.
struct RunBufs {
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
  int *d_gdone = nullptr;      // per-group finish counters (fused c* in k_f8_count32x)
  float4 *d_G4 = nullptr;      // per-hypothesis decision constants (k_f8_count32q)
  // pruned count: the run's words (rsd::kPruneWords), the survivor list, the rest stage's
  // per-group finish counters; staged: the set's last run went through the three stages
  int *d_pw = nullptr;
  int *d_surv = nullptr;
  int *d_gdone_b = nullptr;
  bool staged = false;
  // carried run (no sample; L from the lane's carry word): the fallback storage, which the recount
  // of a run that fell back zeroes and fills (counts, per-group finish counters, c* word);
  // carried: the set's last run was such a run
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

// The plan's four allocations.  Device: `hyp`, everything sized by ld (fixed at create), and
// `pts`, everything sized by the point capacity (regrown by plan_retarget).  Pinned, each with
// its device mapping: `slot`, the kSlots result headers (fixed), and `inl`, the kSlots S_RANSAC
// lists (regrown).  bytes: what plan_layout last reported.
struct Arenas {
  char *hyp = nullptr, *pts = nullptr;
  char *slot = nullptr, *slot_dev = nullptr, *inl = nullptr, *inl_dev = nullptr;
  size_t hyp_bytes = 0, pts_bytes = 0, slot_bytes = 0, inl_bytes = 0;
};

struct PlanBufs {
  Arenas mem;
  // kBufs: with two lanes the sets of runs k and k-1 (solve / count) and of runs k-2 and k-3
  // (their tails ride with those solves) are live at once
  RunBufs buf[kBufs];
  int *d_carry = nullptr;      // kLanes carry words, then the fallback counter
  double *d_p12 = nullptr;     // staging (2,n) p1 then (2,n) p2
  rsd::Pt *d_pts = nullptr;    // AoS float64 points
  float4 *d_pts32q = nullptr;  // the same, point-pair layout (k_f8_count32q)
  // Each run's tail writes its result header and S_RANSAC (cap_n ints) into its own pinned slot
  // through the host mapping; rs_f8_plan_result waits for the last run and reads them there.
  rsd::F8DevResult *h_slot[kSlots] = {}, *h_slot_dev[kSlots] = {};
  int *h_inl[kSlots] = {}, *h_inl_dev[kSlots] = {};
};

// The next `count` elements of the arena L lays out: the pointer from L's device base and, for a
// pinned arena, the one from its host base (an unbound base gives null: sizes only)
template <class T>
inline void arena_put(Layout &L, size_t count, T *&dev, T **host = nullptr) {
  const Layout::Buf<T> b = L.add<T>(count);
  dev = L.dev() ? b.dev() : nullptr;
  if (host) *host = L.host() ? b.host() : nullptr;
}

// Every buffer of the plan: m's pointers from m.mem's bases and m.mem's byte counts.  Each buffer
// is padded to 256 bytes (Layout's default), so it starts as aligned as its arena.
inline void plan_layout(PlanBufs &m, int64_t max_hyp, int64_t cap_n) {
  const size_t ld = static_cast<size_t>((max_hyp + 63) / 64 * 64), n = static_cast<size_t>(cap_n);
  Arenas &a = m.mem;
  Layout hyp, pts, slot, inl;
  hyp.bind(a.hyp, nullptr);
  pts.bind(a.pts, nullptr);
  slot.bind(a.slot_dev, a.slot);
  inl.bind(a.inl_dev, a.inl);
  for (RunBufs &b : m.buf) {
    arena_put(hyp, 9 * ld, b.d_F);
    arena_put(hyp, 9 * ld, b.d_F32);
    arena_put(hyp, ld, b.d_counts);
    arena_put(hyp, 8 * ld, b.d_tuples);
    arena_put(hyp, ld, b.d_cand);
    arena_put(hyp, rsd::kStatusWords, b.d_status);
    arena_put(hyp, ld, b.d_ccount);
    arena_put(hyp, ld, b.d_cfast);
    arena_put(hyp, rsd::kSelectBlocks, b.d_spec_j);
    arena_put(hyp, ld, b.d_cstd);
    arena_put(hyp, ld, b.d_cnorm);
    arena_put(hyp, ld / 64, b.d_gdone);
    arena_put(hyp, ld, b.d_G4);
    arena_put(hyp, rsd::kPruneWords, b.d_pw);
    arena_put(hyp, ld, b.d_surv);
    arena_put(hyp, ld / 64, b.d_gdone_b);
    arena_put(hyp, ld, b.d_counts_fb);
    arena_put(hyp, ld / 64, b.d_gdone_fb);
    arena_put(hyp, 1, b.d_fbw);
  }
  arena_put(hyp, kLanes + 1, m.d_carry);
  arena_put(pts, 4 * n, m.d_p12);
  arena_put(pts, n, m.d_pts);
  arena_put(pts, (n + 7) / 8 * 8, m.d_pts32q);
  for (RunBufs &b : m.buf) arena_put(pts, rsd::kSelectBlocks * n, b.d_spec);
  for (int k = 0; k < kSlots; ++k) {
    arena_put(slot, 1, m.h_slot_dev[k], &m.h_slot[k]);
    arena_put(inl, n, m.h_inl_dev[k], &m.h_inl[k]);
  }
  a.hyp_bytes = hyp.total();
  a.pts_bytes = pts.total();
  a.slot_bytes = slot.total();
  a.inl_bytes = inl.total();
}

struct Sched {
  bool overlap = true;         // two lanes
  int64_t runs = 0;            // runs issued
  bool pending = false;        // stream work not yet waited for
  int last_lane = 0;           // the lane of the last issued run
  bool busy[kLanes] = {};      // the lane has work the host has not waited for
  // set guard: runs issued when the host last waited for the lane (every run of the lane below
  // that index is complete), and how often a run had to wait on the host for the other lane
  int64_t synced[kLanes] = {};
  int64_t lane_waits = 0;
  int set_lane[kBufs] = {};                      // the lane of the last run that used the set
  int64_t set_last_run[kBufs] = {-1, -1, -1, -1};  // ... and that run's index
  // Carried bound: carry_ok[l]: lane l's carry word holds the c* of a run with carry_H /
  // carry_thresh over the resident points
  bool carry_ok[kLanes] = {};
  int64_t carry_H = 0;
  double carry_thresh = 0.0;
};

// The host is about to wait for one lane (the set guard and the parity entry points): false when
// the lane is idle and there is nothing to wait for
inline bool lane_drained(Sched &s, int lane) {
  if (!s.busy[lane]) return false;
  s.busy[lane] = false;
  s.synced[lane] = s.runs;
  ++s.lane_waits;
  return true;
}

// The host has waited for both lanes (plan_flush)
inline void flushed(Sched &s) {
  for (int l = 0; l < kLanes; ++l) {
    s.busy[l] = false;
    s.synced[l] = s.runs;
  }
  s.pending = false;
}

// Where the next run goes, and the host waits it needs first, in this order: lane 1 (drain1),
// then the lane that last used the run's buffer set (guard >= 0).  The waits' bookkeeping is done
// and the set is claimed for the run.
struct Placement {
  int lane;
  bool drain1;
  int guard;
};
inline Placement place(Sched &s, bool dev_tuples) {
  Placement pl{0, false, -1};
  // lane 0 when nothing is in flight, else the lane the previous run did not use; device tuples
  // were written on the context stream, so their run follows them on lane 0 (its entry point
  // has drained lane 1 before the parse)
  if (dev_tuples)
    pl.drain1 = lane_drained(s, 1);
  else if (s.overlap && s.pending)
    pl.lane = 1 - s.last_lane;
  // set guard: the set's last run went to the other lane and the host has not waited for that
  // lane since, so it may still be in flight there.  Taken only after a parity entry point broke
  // the alternation: in a Philox or host-tuple sequence the set's last run either used this
  // lane (stream order covers it) or preceded a plan_flush, after which lane and set parity may
  // differ from the recorded ones without any work left to wait for
  const int k = static_cast<int>(s.runs % kBufs), was = s.set_lane[k];
  if (was != pl.lane && s.set_last_run[k] >= s.synced[was] && lane_drained(s, was)) pl.guard = was;
  s.set_lane[k] = pl.lane;
  s.set_last_run[k] = s.runs;
  return pl;
}

// The run is enqueued; its tail is pending on its lane
inline void committed(Sched &s, int lane) {
  s.busy[lane] = true;
  s.last_lane = lane;
  ++s.runs;
  s.pending = true;
}

// HIP timing events of run `run`: 0 none, 1 around the count, 2 also the tail+solve launch; a
// timed run counts alone (exclusive) when the other lane has work
inline int timing_level(int64_t run, int timing, int every) { return run % every == 0 ? timing : 0; }
inline bool exclusive(const Sched &s, int lane, int tl) { return tl >= 1 && s.busy[1 - lane]; }

// The carry words no longer describe what the next run counts (new points, another counting
// kernel, another H or threshold): both lanes start again from a sample run
inline void carry_drop(Sched &s) {
  for (bool &ok : s.carry_ok) ok = false;
}

inline int env_int(const char *name, int dflt) {
  const char *v = std::getenv(name);
  return v ? std::atoi(v) : dflt;
}

// Pruned count (fp32 path; derivation above k_f8_count32q): a full count of the first `sample`
// groups, the others screened over the prefix [0, K), a full count of the survivors.  prune = 0:
// the single whole-window launch.  The margin and the least number of skipped points worth pruning
// for come from n unless given (profiles/prune/ab.txt; swept again for the screening prefix stage,
// profiles/screen/ab.txt).  Carried bound (pruning on): a run on a lane whose previous run had the
// same H and threshold over the same points takes L = (that run's c*, left in d_carry[lane] by its
// tail) - g, g = max(kCarryGapMin, n / kCarryGapDiv), instead of a sample's; no sample stage; if
// the bound turned out to be above c* the run is counted again when it is read (flush_recounts; above
// k_f8_count32q, "Carried bound").  profiles/carry/ab.txt, C2, two rounds, bench value in 1e9
// hypotheses/s: g = n/50 / n/25 / n/16 / n/10 gave 1.705-1.713 / 1.647-1.671 / 1.628-1.641 /
// 1.558-1.575, no fallback in 298 carried runs at any of them, hence n / 50.  The floor is for small
// n, where c* spreads like sqrt(n) and not like n: tools/carry_model.py (profiles/carry/model.txt)
// has c* 160-170 over 8 runs at N = 257, one fallback in 7 at g = 5 and none at 16 (the floor of
// the margin m)
constexpr int kPruneMarginDiv = 30;   // m = max(16, n / 30)
constexpr int kPruneMinSkipDiv = 8;   // prune only when at least n / 8 points are skipped
constexpr int kCarryGapDiv = 50;
constexpr int kCarryGapMin = 16;
struct PruneKnobs {
  int prune = 1;        // RSAMD_PRUNE
  int sample = 32;      // RSAMD_PRUNE_SAMPLE: hypothesis groups of the sample
  int margin = -1;      // RSAMD_PRUNE_MARGIN: m of K = roundup8(n - L + m); below 0: from n
  int min_skip = -1;    // RSAMD_PRUNE_MINSKIP: prune only if >= this many points go; below 0: from n
  int carry = 1;        // RSAMD_CARRY
  int carry_gap = 0;    // RSAMD_CARRY_GAP (may be negative: every run falls back)
  bool carry_gap_set = false;
};
inline PruneKnobs prune_knobs_env() {
  PruneKnobs k;
  k.prune = env_int("RSAMD_PRUNE", k.prune) != 0;
  k.sample = std::max(1, env_int("RSAMD_PRUNE_SAMPLE", k.sample));
  k.margin = env_int("RSAMD_PRUNE_MARGIN", -1);
  k.min_skip = env_int("RSAMD_PRUNE_MINSKIP", -1);
  k.carry = env_int("RSAMD_CARRY", k.carry) != 0;
  k.carry_gap_set = std::getenv("RSAMD_CARRY_GAP") != nullptr;
  k.carry_gap = std::max(-(1 << 24), std::min(1 << 24, env_int("RSAMD_CARRY_GAP", 0)));
  return k;
}

// How a run of H hypotheses on `lane` is counted.  h0: the hypotheses of the sample; staged: the
// pruned count's stages (the fp32 kernel, and hypotheses past the sample); carried: ... without
// the sample, the lane's carry word holding the c* of a run like this one (the decision is the
// host's alone: H and the threshold of the run that left the word).  Drops the carry words when
// this run is not like the one that left them.
struct CountPath {
  int h0;
  bool staged, carried;
};
inline CountPath count_path(Sched &s, const PruneKnobs &k, int lane, int64_t H, double thresh,
                            bool fp32) {
  const int h0 = static_cast<int>(std::min<int64_t>(H, 64LL * std::min(k.sample, 1 << 24)));
  const bool staged = fp32 && k.prune && h0 < H;
  if (!(fp32 && H == s.carry_H && thresh == s.carry_thresh)) carry_drop(s);
  return CountPath{h0, staged, staged && k.carry && s.carry_ok[lane]};
}
// ... and what its tail leaves: this run's c* for the lane's next run, should that be one like it
inline void carry_left(Sched &s, int lane, int64_t H, double thresh, bool fp32) {
  if (!fp32) return;
  s.carry_H = H;
  s.carry_thresh = thresh;
  s.carry_ok[lane] = true;
}

// Deferred recount (f8_kernels.hip above k_f8_count32q, "Carried bound").  The tail of a carried run
// that fell back selects nothing and marks the run's pinned header; the run is counted again only
// if it is read.  Only the last run before a flush can be read, so the decision is taken in
// plan_flush, after both lanes are drained (the header is final then), from host state and that
// flag alone.  pending: a run has been issued since the last flush (nothing pending: nothing new to
// read, and a run recounted at an earlier flush is not recounted again); last_carried: the last
// issued run was a carried one (no other tail sets the flag: a stale word in a slot is not
// trusted); header_fell_back: the flag of that run's slot; why: what the flush serves.
enum class FlushFor {
  kRead,  // an accessor of the last run (plan_wait)
  kDrop,  // set_points, a retarget, set_count_precision, destroy: the results are dropped
};
inline bool flush_recounts(bool pending, bool last_carried, bool header_fell_back, FlushFor why) {
  return pending && last_carried && header_fell_back && why == FlushFor::kRead;
}
// ... and whether that flush leaves the last run without a result: it fell back and was dropped
// unread.  The accessors refuse such a run until the next one is issued.
inline bool flush_drops_unread(bool pending, bool last_carried, bool header_fell_back, FlushFor why) {
  return pending && last_carried && header_fell_back && why == FlushFor::kDrop;
}

// The pruned count's numbers: the margin m = max(16, n / 30) and the least skip n / 8 (at least
// one block of 8 points) unless the environment gave them; a carried run has no sample (every
// group is screened against the lane's carried bound less the gap)
struct PruneNumbers {
  int g_first, margin, min_skip, gap;
};
inline PruneNumbers prune_numbers(const PruneKnobs &k, int n, bool carried) {
  PruneNumbers pn{};
  pn.g_first = carried ? 0 : std::min(k.sample, 1 << 24);
  pn.margin = k.margin >= 0 ? std::min(k.margin, n) : std::max(16, n / kPruneMarginDiv);
  pn.min_skip = std::max(8, k.min_skip >= 0 ? k.min_skip : n / kPruneMinSkipDiv);
  pn.gap = !carried ? 0 : k.carry_gap_set ? k.carry_gap : std::max(kCarryGapMin, n / kCarryGapDiv);
  return pn;
}

// Points per chunk of the float64 counting kernel
inline int choose_chunk(int64_t n, int64_t H) {
  const int64_t groups = (H + 63) / 64;
  // aim for >= 8 units of work per SIMD (1024 SIMDs) without chunks below 64 points
  int64_t nchunks = (8192 + groups - 1) / groups;
  nchunks = std::max<int64_t>(1, std::min<int64_t>(nchunks, (n + 63) / 64));
  return static_cast<int>((n + nchunks - 1) / nchunks);
}

}  // namespace rs::f8
