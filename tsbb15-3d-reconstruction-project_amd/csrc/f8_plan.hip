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
//                    threshold over the same points (RSAMD_CARRY=1) has prefix and rest alone,
//                    its bound from that run's c* in the lane's carry word
//
// and leaves run k's tail pending on that lane: it rides along with the lane's next solve, or
// is flushed alone by rs_f8_plan_result / set_points / destroy (plan_flush, the only place the
// host waits).  A carried run whose bound turned out to be above c* ("fell back", f8_kernels.hip
// above k_f8_count32q) is not counted again on the lane: its tail selects nothing and marks the
// run's pinned header.  Only the last run before a flush can be read through the API, so
// plan_flush, when it serves an accessor and finds that mark on the last run, counts the run again
// in full and runs its tail a second time before it returns (plan_recount).  A fallen-back run
// that is never read is never recounted: its pinned slot is marked, not filled.  The tail
// (candidates, reference statistics, replay, S_RANSAC; latency bound, a few busy workgroups) and
// the solve (latency bound, ~1.5 waves per SIMD) share the machine in their one launch instead of
// running back to back.
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
#include "f8_order.h"
#include "f8_sched.h"

namespace f8 = rs::f8;
using f8::RunBufs;

// rs_f8_plan::overlap (two lanes) unless RSAMD_OVERLAP is set: two lanes measured 8-9 % ahead
// of one in every interleaved bench run (profiles/lanes/ab.txt)
constexpr int kOverlapDefault = 1;

// The buffers (f8::PlanBufs: four arenas, laid out by f8::plan_layout) and the state the run
// decisions read and write (f8::Sched, f8::PruneKnobs) are plain data in f8_sched.h; what is left
// here are the HIP objects and the knobs of the launches.
struct rs_f8_plan : f8::PlanBufs {
  rs_ctx *ctx = nullptr;
  int64_t n = 0, max_hyp = 0, ld = 0;
  int64_t cap_n = 0;           // points the per-point arenas hold (>= n; plan_retarget)
  static constexpr int kBufs = f8::kBufs, kSlots = f8::kSlots, kEvRing = 64, kLanes = f8::kLanes;
  hipEvent_t ring[kEvRing][4] = {};  // count start/end; tail+solve launch start/end
  bool timed[kEvRing] = {};          // whether run r % kEvRing recorded its events
  int64_t last_H = 0;
  // Two lanes (RSAMD_OVERLAP=1; kOverlapDefault otherwise): consecutive runs alternate between
  // the context's stream (lane 0) and lane1, each lane a serial chain tail+solve -> count, so
  // one lane's solve and count fill the wave slots the other lane's count leaves idle.
  f8::Sched s;
  hipStream_t lane1 = nullptr;       // created when the first run is placed on it
  bool tail_pending[kLanes] = {};    // the lane's last run's tail is not enqueued yet
  rsd::TailArgs tail[kLanes] = {};   // ... its arguments
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
  f8::PruneKnobs knobs;       // the pruned count and the carried bound (RSAMD_PRUNE*, RSAMD_CARRY*)
  int64_t n_carried = 0;      // runs carried since the plan was created
  int64_t n_recounts = 0;     // fallen-back runs counted again at a flush (plan_recount)
  // Point order of the pruned count (f8_order.h): the ordered copies of d_pts / d_pts32q, which
  // the fp32 count's stages read while ord_on; installed by plan_wait, dropped by set_points and
  // a retarget
  f8::OrderBufs ord;
  int order = 1;              // RSAMD_ORDER
  bool ord_on = false;
  int64_t ord_first = 0;      // points placed first (the winner's outliers)
  int64_t ord_installs = 0;   // installs since the plan was created
  int64_t runs_since_points = 0;
  std::vector<int32_t> ord_perm;        // host scratch of an install
  std::vector<unsigned char> ord_mark;
  int count_launches = 0;     // launches the last run enqueued between its timing events
  bool unread_dropped = false;  // the last run fell back and a dropping flush left it unread
  int *d_full = nullptr;      // rs_f8_plan_counts after a pruned run: the full counts (ld ints)
  int nospec = 0;             // RSAMD_NOSPEC=1 (test hook): the replay extracts S_RANSAC itself
  uint64_t *d_ts = nullptr;   // RSAMD_TSTAMP=<file>: wave timeline of the counting kernel
  const char *ts_path = nullptr;

  const RunBufs &last() const { return buf[(s.runs - 1) % kBufs]; }
};

// The arenas sized by the point capacity (device buffers, pinned S_RANSAC lists) released and
// allocated again for `cap` points; the plan's pointers follow.  On failure the plan holds none.
static hipError_t alloc_point_arenas(rs_f8_plan *p, int64_t cap) {
  f8::Arenas &a = p->mem;
  (void)hipFree(a.pts);
  if (a.inl) (void)hipHostFree(a.inl);
  a.pts = a.inl = a.inl_dev = nullptr;
  f8::plan_layout(*p, p->max_hyp, cap);  // sizes; the per-point pointers go null
  p->ord_on = false;
  f8::order_layout(p->ord, nullptr, cap);
  // the ordered copies of the points lie behind plan_layout's buffers in the same allocation
  hipError_t e = hipMalloc(reinterpret_cast<void **>(&a.pts), a.pts_bytes + p->ord.bytes);
  if (e == hipSuccess) e = hipHostMalloc(reinterpret_cast<void **>(&a.inl), a.inl_bytes);
  if (e == hipSuccess) e = hipHostGetDevicePointer(reinterpret_cast<void **>(&a.inl_dev), a.inl, 0);
  if (e == hipSuccess) {
    f8::plan_layout(*p, p->max_hyp, cap);
    f8::order_layout(p->ord, a.pts + a.pts_bytes, cap);
  }
  return e;
}

static void plan_free(rs_f8_plan *p) {
  f8::Arenas &a = p->mem;
  (void)hipFree(a.hyp);
  (void)hipFree(a.pts);
  if (a.slot) (void)hipHostFree(a.slot);
  if (a.inl) (void)hipHostFree(a.inl);
  (void)hipFree(p->d_full);
  if (p->d_ts) {
    (void)rsd::set_count_timeline(nullptr);
    (void)hipFree(p->d_ts);
  }
  for (RunBufs &b : p->buf) {
    if (b.h_tuples) (void)hipHostFree(b.h_tuples);
    if (b.ev_copy) (void)hipEventDestroy(b.ev_copy);
  }
  for (auto &e : p->ev_end)
    if (e) (void)hipEventDestroy(e);
  if (p->lane1) (void)hipStreamDestroy(p->lane1);
  for (auto &r : p->ring)
    for (auto &e : r)
      if (e) (void)hipEventDestroy(e);
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
  if (const char *cm = std::getenv("RSAMD_COUNT"))  // tools: RSAMD_COUNT=fp64
    p->use_fp32 = std::strcmp(cm, "fp64") != 0;
  p->timing = f8::env_int("RSAMD_TIMING", 1);
  p->timing_every = std::max(1, f8::env_int("RSAMD_TIMING_EVERY", 1));
  {
    int cus = 256;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, c->device) != hipSuccess)
      cus = 256;
    p->tail_cus = cus;
    p->q_waves = std::max(1, f8::env_int("RSAMD_WAVES", rsd::count32q_resident_waves(c->device)));
    p->q_slices = f8::env_int("RSAMD_QSLICES", 0);
  }
  // the arenas fixed at create (per-hypothesis buffers, pinned result headers), then the per-point
  // ones, whose call lays everything out
  f8::Arenas &a = p->mem;
  f8::plan_layout(*p, max_hyp, n);
  hipError_t e = hipMalloc(reinterpret_cast<void **>(&a.hyp), a.hyp_bytes);
  if (e == hipSuccess) e = hipHostMalloc(reinterpret_cast<void **>(&a.slot), a.slot_bytes);
  if (e == hipSuccess) e = hipHostGetDevicePointer(reinterpret_cast<void **>(&a.slot_dev), a.slot, 0);
  if (e == hipSuccess) e = alloc_point_arenas(p, n);
  if (e == hipSuccess) e = hipMemset(p->d_carry, 0, sizeof(int) * (rs_f8_plan::kLanes + 1));
  for (auto &r : p->ring)
    for (auto &ev : r)
      if (e == hipSuccess) e = hipEventCreate(&ev);
  p->s.overlap = f8::env_int("RSAMD_OVERLAP", kOverlapDefault) != 0;
  p->nospec = f8::env_int("RSAMD_NOSPEC", 0) != 0;
  p->knobs = f8::prune_knobs_env();
  p->order = f8::env_int("RSAMD_ORDER", 1) != 0;
  p->ts_path = std::getenv("RSAMD_TSTAMP");
  if (p->ts_path) {
    p->s.overlap = false;  // one device-global timeline buffer: one counting launch at a time
    p->knobs.prune = 0;    // ... and one launch per run
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

static int plan_flush(rs_f8_plan *p, f8::FlushFor why);
static int plan_recount(rs_f8_plan *p);

// A new population for an existing plan (the drop-in's calls, one pair after another): the
// per-point arenas are reallocated only when n exceeds what they hold; the per-hypothesis
// arena, the result headers and the events are kept
static int plan_retarget(rs_f8_plan *p, int64_t n) {
  if (n < 8) return fail(RS_EINVAL, "Cannot take a larger sample than population when 'replace=False'");
  if (n > (1LL << 30)) return fail(RS_EINVAL, "plan dimensions out of range");
  int st = plan_flush(p, f8::FlushFor::kDrop);  // runs in flight read the resident points and results
  if (st) return st;
  if (n > p->cap_n) {
    const int64_t cap = std::max<int64_t>(n, p->cap_n + p->cap_n / 4);
    const hipError_t e = alloc_point_arenas(p, cap);
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
  f8::carry_drop(p->s);
  p->ord_on = false;
  p->runs_since_points = 0;
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

// The host wait for one lane that f8::lane_drained has booked, its pending tail included
static hipError_t lane_wait(rs_f8_plan *p, int lane) {
  hipError_t e = lane_tail_alone(p, lane);
  if (e == hipSuccess) e = hipStreamSynchronize(lane_stream(p, lane));
  return e;
}

// Host wait for lane 1 if it has work (the parity entry points, before their parse)
static hipError_t lane1_drain(rs_f8_plan *p) {
  return f8::lane_drained(p->s, 1) ? lane_wait(p, 1) : hipSuccess;
}

// Enqueue both lanes' pending tails alone, then wait for both streams.  The last run's header is
// final then: if it says the run fell back, a flush that serves an accessor counts the run again
// (f8::flush_recounts); one that drops the results does not, and the run stays without a result.
static int plan_flush(rs_f8_plan *p, f8::FlushFor why) {
  HIP_TRY(hipSetDevice(p->ctx->device));
  for (int l = 0; l < rs_f8_plan::kLanes; ++l) HIP_TRY(lane_tail_alone(p, l));
  if (p->s.busy[1]) HIP_TRY(hipStreamSynchronize(p->lane1));
  HIP_TRY(hipStreamSynchronize(p->ctx->stream));
  for (auto &e : p->excl) e = nullptr;
  const bool pending = p->s.pending && p->s.runs > 0;
  const bool carried = pending && p->last().carried;
  const bool marked =
      carried && p->h_slot[(p->s.runs - 1) % rs_f8_plan::kSlots]->fell_back != 0;
  f8::flushed(p->s);
  if (f8::flush_drops_unread(pending, carried, marked, why)) p->unread_dropped = true;
  if (f8::flush_recounts(pending, carried, marked, why)) return plan_recount(p);
  return RS_OK;
}

extern "C" int rs_f8_plan_destroy(rs_f8_plan *p) {
  if (!p) return RS_OK;
  (void)plan_flush(p, f8::FlushFor::kDrop);
  plan_free(p);
  delete p;
  return RS_OK;
}

extern "C" int rs_f8_plan_set_points(rs_f8_plan *p, const double *p1, const double *p2) {
  if (!p || !p1 || !p2) return fail(RS_EINVAL, "null pointer");
  int st = plan_flush(p, f8::FlushFor::kDrop);  // runs in flight read the resident points
  if (st) return st;
  f8::carry_drop(p->s);
  p->ord_on = false;
  p->runs_since_points = 0;
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

// What the steps of one run (plan_run, below them in its order) share
struct Run {
  int h, mode;
  uint64_t seed, hyp_offset;
  double thresh;
  bool fp32;
  int lane, tl;        // f8::place, f8::timing_level
  bool excl;           // f8::exclusive
  f8::CountPath cp;
  hipStream_t ms;      // the lane's stream
  hipEvent_t *ev;      // the run's ring entry
  hipEvent_t ev_end;   // exclusive run: marks the other lane's end
};

static int run_check(const rs_f8_plan *p, int64_t H, int32_t mode, const int32_t *host_tuples,
                     double thresh, bool dev_tuples) {
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
  return RS_OK;
}

// The run's lane and timing level, after the host waits the placement asks for (f8::place)
static int run_place(rs_f8_plan *p, Run &r, bool dev_tuples) {
  const int64_t k = p->s.runs % rs_f8_plan::kEvRing;
  r.ev = p->ring[k];
  r.tl = f8::timing_level(p->s.runs, p->timing, p->timing_every);
  p->timed[k] = r.tl >= 1;
  const f8::Placement pl = f8::place(p->s, dev_tuples);
  r.lane = pl.lane;
  if (pl.drain1) HIP_TRY(lane_wait(p, 1));
  if (r.lane == 1) HIP_TRY(ensure_lane1(p));
  r.ms = lane_stream(p, r.lane);
  if (pl.guard >= 0) HIP_TRY(lane_wait(p, pl.guard));
  HIP_TRY(lane_excl_wait(p, r.lane));
  // a timed run counts alone: its lane waits for the other lane's current end before its first
  // event, and the other lane waits for the run's last event before its next launch
  r.excl = f8::exclusive(p->s, r.lane, r.tl);
  r.ev_end = r.excl ? p->ev_end[k] : nullptr;
  return RS_OK;
}

// Host tuples through the set's pinned buffer: the copy no longer reads caller memory after
// plan_run returns (the caller may free or reuse its tuples at once)
static int stage_tuples(rs_f8_plan *p, RunBufs &b, const Run &r, const int32_t *host_tuples) {
  const int64_t H = r.h;
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
  HIP_TRY(hipMemcpyAsync(b.d_tuples, b.h_tuples, sizeof(int) * 8 * H, hipMemcpyHostToDevice, r.ms));
  HIP_TRY(hipEventRecord(b.ev_copy, r.ms));
  b.copy_pending = true;
  return RS_OK;
}

static rsd::SolveArgs solve_args(const rs_f8_plan *p, const RunBufs &b, const Run &r) {
  rsd::SolveArgs sa{};
  sa.pts = p->d_pts;
  sa.n = static_cast<int>(p->n);
  sa.H = r.h;
  sa.mode = r.mode;
  sa.seed = r.seed;
  sa.hyp_offset = r.hyp_offset;
  sa.tuples = b.d_tuples;
  sa.Fsoa = b.d_F;
  sa.ld = p->ld;
  sa.counts = b.d_counts;
  sa.status = b.d_status;
  sa.frame = rsd::Frame{1.0, 0.0, 0.0, 0.0, 0.0};
  sa.gdone = b.d_gdone;
  if (r.fp32) {
    const rsd::Bounds gb = rsd::fp32_bounds(p->frame, r.thresh);
    sa.F32soa = b.d_F32;
    sa.frame = p->frame;
    sa.G4 = b.d_G4;
    sa.gT = gb.thr2;
    sa.gDe = gb.De;
    sa.gDn = gb.Dn;
  }
  if (r.cp.staged) {
    sa.pw = b.d_pw;
    sa.gdone_b = b.d_gdone_b;
  }
  return sa;
}

// An exclusive run's lane waits for the other lane's current end
static int wait_other_lane(rs_f8_plan *p, const Run &r) {
  HIP_TRY(hipEventRecord(r.ev_end, lane_stream(p, 1 - r.lane)));
  HIP_TRY(hipStreamWaitEvent(r.ms, r.ev_end, 0));
  return RS_OK;
}

// [tail of the lane's previous run | solve of this run]: the run's buffer set was last used
// kBufs runs back, on this lane (or on one drained in run_place), and that run's tail precedes
// this launch in stream order
static int launch_tail_solve(rs_f8_plan *p, const Run &r, rsd::SolveArgs sa) {
  int st;
  if (r.excl && r.tl >= 2 && (st = wait_other_lane(p, r))) return st;
  if (r.tl >= 2) HIP_TRY(hipEventRecord(r.ev[2], r.ms));
  HIP_TRY(rsd::launch_f8_tail_solve(p->tail_pending[r.lane] ? &p->tail[r.lane] : nullptr, &sa, r.ms,
                                    p->tail_cus));
  p->tail_pending[r.lane] = false;
  if (r.tl >= 2) HIP_TRY(hipEventRecord(r.ev[3], r.ms));
  return RS_OK;
}

// The pruned count's arguments for buffer set b, whose run is on `lane`
static rsd::PruneArgs prune_args(const rs_f8_plan *p, const RunBufs &b, int lane) {
  const f8::PruneNumbers pn = f8::prune_numbers(p->knobs, static_cast<int>(p->n), b.carried);
  rsd::PruneArgs pa{};
  pa.pw = b.d_pw;
  pa.surv = b.d_surv;
  pa.gdone_b = b.d_gdone_b;
  pa.g_first = pn.g_first;
  pa.margin = f8::order_margin(pn.margin, p->knobs.margin >= 0, static_cast<int>(p->n), p->ord_on);
  pa.min_skip = pn.min_skip;
  if (b.carried) {  // every group is screened against the lane's carried bound
    pa.carry = p->d_carry + lane;
    pa.gap = pn.gap;
  }
  return pa;
}

// What the fp32 counting kernel reads and writes for h hypotheses of set b's last run
// Both point arrays from one copy: the ordered one while an order is installed (a count is a sum
// over the points and the drop rule holds for any fixed order, so every stage of a run, its
// recount and rs_f8_plan_counts may read either; installs happen only with both lanes drained)
static rsd::CountArgs count_args(const rs_f8_plan *p, const RunBufs &b, int h) {
  const float4 *ptsq = p->ord_on ? p->ord.d_pts32q : p->d_pts32q;
  const rsd::Pt *pts = p->ord_on ? p->ord.d_pts : p->d_pts;
  return rsd::CountArgs{ptsq, pts, static_cast<int>(p->n), h, b.d_F32, b.d_F, p->ld,
                        rsd::GuardW{b.thresh * b.thresh}, b.d_counts, b.d_gdone, b.d_status, b.d_G4,
                        nullptr};
}

// The counts of the run, between its timing events
static int enqueue_count(rs_f8_plan *p, RunBufs &b, const Run &r) {
  const int n = static_cast<int>(p->n), h = r.h, h0 = r.cp.h0;
  hipStream_t ms = r.ms;
  int st;
  if (r.excl && r.tl == 1 && (st = wait_other_lane(p, r))) return st;
  if (r.tl >= 1) HIP_TRY(hipEventRecord(r.ev[0], ms));
  rsd::CountArgs ca = count_args(p, b, h);
  const auto shape = [&](int hh, int slices) { return rsd::count32q_shape(n, hh, p->q_waves, slices); };
  if (r.cp.staged) {
    // sample (whole window, c* of its groups = L in status[0]) -> prefix [0, K) of the other
    // groups screened, K from L on the device, survivors listed -> the survivors over the whole
    // window; all in stream order on this lane, no host decision.  A carried run has no sample:
    // prefix of every group against L = the lane's carry word - gap -> the survivors (c_f in
    // status[0]), and nothing else: whether c_f reached L is the tail's test, and a run that fell
    // back is counted again when it is read (plan_recount)
    const rsd::PruneArgs pa = prune_args(p, b, r.lane);
    const int hr = r.cp.carried ? h : h - h0;  // the hypotheses the prefix stage screens
    const rsd::Count32qShape sh1 = shape(hr, p->q_slices);
    if (!r.cp.carried) {
      ca.H = h0;
      HIP_TRY(rsd::launch_f8_count32q(rsd::kCountWhole, ca, shape(h0, p->q_slices), 0, pa, ms));
    }
    ca.H = h;
    HIP_TRY(rsd::launch_f8_count32q(rsd::kCountPrefix, ca, sh1, 0, pa, ms));
    ca.H = hr;
    HIP_TRY(rsd::launch_f8_count32q(rsd::kCountRest, ca, sh1, p->q_waves, pa, ms));
    p->count_launches = r.cp.carried ? 2 : 3;
    if (r.cp.carried) ++p->n_carried;
  } else if (r.fp32) {
    // fused c*: the chunk that completes a hypothesis group folds its max into status[0]
    HIP_TRY(rsd::launch_f8_count32q(rsd::kCountWhole, ca, shape(h, p->q_slices), 0, {}, ms));
    p->count_launches = 1;
  } else {
    HIP_TRY(rsd::launch_f8_count(p->d_pts, n, h, b.d_F, p->ld, f8::choose_chunk(p->n, h),
                                 r.thresh * r.thresh, b.d_counts, ms));
    HIP_TRY(rsd::launch_f8_max(b.d_counts, h, b.d_status, ms));
    p->count_launches = 2;  // the float64 count and its c*
  }
  if (r.tl >= 1) HIP_TRY(hipEventRecord(r.ev[1], ms));
  if (r.tl >= 1 && p->s.overlap) p->excl[1 - r.lane] = r.ev[1];
  return RS_OK;
}

// The run's tail, which rides along with the lane's next solve (or plan_flush)
static rsd::TailArgs tail_args(const rs_f8_plan *p, const RunBufs &b, const Run &r, int slot) {
  rsd::TailArgs ta{};
  ta.pts = p->d_pts;
  ta.n = static_cast<int>(p->n);
  ta.H = r.h;
  ta.slack = 1;
  ta.Fsoa = b.d_F;
  ta.ld = p->ld;
  ta.counts = b.d_counts;
  ta.status = b.d_status;
  ta.thresh = r.thresh;
  ta.cand = b.d_cand;
  ta.ccount = b.d_ccount;
  ta.cfast = b.d_cfast;
  ta.spec = b.d_spec;
  ta.spec_j = b.d_spec_j;
  ta.nospec = p->nospec;
  ta.cstd = b.d_cstd;
  ta.cnorm = b.d_cnorm;
  ta.hres = p->h_slot_dev[slot];
  ta.hinl = p->h_inl_dev[slot];
  if (r.fp32) ta.carry = p->d_carry + r.lane;  // this run's c* for the lane's next run
  if (r.cp.carried) {
    ta.pw = b.d_pw;
    ta.counts_fb = b.d_counts_fb;
    ta.fbw = b.d_fbw;
    ta.n_fb = p->d_carry + rs_f8_plan::kLanes;
  }
  return ta;
}

// The last run, complete on both lanes, fell back and is about to be read: every hypothesis over
// the whole window into the set's fallback storage, then the run's tail a second time, which takes
// c*, the counts and max_count_fast from there (TailArgs::recount), fills the pinned slot and
// leaves the true c* in the lane's carry word.  Nothing else is in flight (plan_flush); the
// storage is zeroed here and not per run, so a run that did not fall back never touches it.
static int plan_recount(rs_f8_plan *p) {
  const RunBufs &b = p->last();
  const int lane = p->s.last_lane, h = static_cast<int>(p->last_H);
  hipStream_t ms = lane_stream(p, lane);
  HIP_TRY(hipMemsetAsync(b.d_counts_fb, 0, sizeof(int) * p->ld, ms));
  HIP_TRY(hipMemsetAsync(b.d_gdone_fb, 0, sizeof(int) * (p->ld / 64), ms));
  HIP_TRY(hipMemsetAsync(b.d_fbw, 0, sizeof(int), ms));
  rsd::CountArgs ca = count_args(p, b, h);
  ca.counts = b.d_counts_fb;
  ca.gdone = b.d_gdone_fb;
  ca.status = b.d_fbw;
  const rsd::Count32qShape sh =
      rsd::count32q_shape(static_cast<int>(p->n), h, p->q_waves, p->q_slices);
  HIP_TRY(rsd::launch_f8_count32q(rsd::kCountWhole, ca, sh, 0, {}, ms));
  rsd::TailArgs ta = p->tail[lane];  // the last run's (its lane has had no run since)
  ta.recount = 1;
  HIP_TRY(rsd::launch_f8_tail_solve(&ta, nullptr, ms));
  HIP_TRY(hipStreamSynchronize(ms));
  ++p->n_recounts;
  return RS_OK;
}

// One run.  dev_tuples: tuple mode with the tuples already written (in range, by the GPU
// parity stream) into the buffer set this run uses, so there is no host copy or check.
static int plan_run(rs_f8_plan *p, int64_t H, int32_t mode, uint64_t seed, uint64_t hyp_offset,
                    const int32_t *host_tuples, double thresh, bool dev_tuples) {
  int st = run_check(p, H, mode, host_tuples, thresh, dev_tuples);
  if (st) return st;
  HIP_TRY(hipSetDevice(p->ctx->device));
  RunBufs &b = p->buf[p->s.runs % rs_f8_plan::kBufs];
  const int slot = static_cast<int>(p->s.runs % rs_f8_plan::kSlots);
  Run r{static_cast<int>(H), mode, seed, hyp_offset, thresh, p->use_fp32 && p->fp32_ok};
  if ((st = run_place(p, r, dev_tuples))) return st;
  if (mode == RS_SAMPLER_TUPLES && !dev_tuples && (st = stage_tuples(p, b, r, host_tuples))) return st;
  r.cp = f8::count_path(p->s, p->knobs, r.lane, H, thresh, r.fp32);
  b.staged = r.cp.staged;
  b.carried = r.cp.carried;
  b.thresh = thresh;
  if ((st = launch_tail_solve(p, r, solve_args(p, b, r)))) return st;
  if ((st = enqueue_count(p, b, r))) return st;
  p->tail[r.lane] = tail_args(p, b, r, slot);
  p->tail_pending[r.lane] = true;
  f8::carry_left(p->s, r.lane, H, thresh, r.fp32);
  f8::committed(p->s, r.lane);
  p->last_H = H;
  p->unread_dropped = false;
  ++p->runs_since_points;
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
    HIP_TRY(lane1_drain(p));
    if (start == 0 && count == H && std::getenv("RSAMD_NP_SYNC") == nullptr) {
      // the whole draw in one segment: the run is queued behind the parse before the host
      // waits for the parse's outcome (no host gap between them); should the parse ask to be
      // drawn again (a wrap-log overflow), that run is superseded by the synchronous path below
      bool queued = false;
      RunBufs &b = p->buf[p->s.runs % rs_f8_plan::kBufs];
      if ((st = rs::np_choice_enqueue(p->ctx, key, *pos, p->n, 8, H, b.d_tuples, &queued)))
        return st;
      if (queued) {
        const int run_st = plan_run(p, count, RS_SAMPLER_TUPLES, 0, 0, nullptr, thresh, true);
        bool rerun = false;
        if ((st = rs::np_choice_finish(p->ctx, key, pos, &rerun))) return st;
        if (run_st || !rerun) return run_st;
      }
    }
    RunBufs &b = p->buf[p->s.runs % rs_f8_plan::kBufs];
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
  RunBufs &b = p->buf[p->s.runs % rs_f8_plan::kBufs];
  HIP_TRY(hipSetDevice(p->ctx->device));
  HIP_TRY(lane1_drain(p));  // the tuples are written on the context stream (lane 0)
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

// The point order (f8_order.h; derivation above k_f8_count32q, "Point order"), installed from the
// winner a read flush just delivered: the run's pinned S_RANSAC list and best_count, final after
// plan_flush (a fallen-back run has been recounted there).  Both lanes are drained and nothing
// reads the ordered copies.  One small upload, one pack launch and one wait on the context
// stream, after which either lane's launches see the copies.  A winner that orders nothing
// (f8::order_outliers_first returns 0) installs nothing, and a later read may try again.
static int order_install(rs_f8_plan *p) {
  const int slot = static_cast<int>((p->s.runs - 1) % rs_f8_plan::kSlots);
  const rsd::F8DevResult *r = p->h_slot[slot];
  const int *inl = p->h_inl[slot];
  if (!inl || r->fell_back != 0 || r->best_count <= f8::kOrderMinCount) return RS_OK;
  const size_t n = static_cast<size_t>(p->n);
  p->ord_perm.resize(n);
  p->ord_mark.resize(n);
  const int64_t first = f8::order_outliers_first(inl, r->n_inliers, r->best_count, p->n,
                                                 p->ord_perm.data(), p->ord_mark.data());
  if (first <= 0) return RS_OK;
  hipStream_t s = p->ctx->stream;
  HIP_TRY(hipMemcpyAsync(p->ord.d_perm, p->ord_perm.data(), sizeof(int32_t) * n,
                         hipMemcpyHostToDevice, s));
  HIP_TRY(rsd::launch_pack_points32q_perm(p->d_pts, p->ord.d_perm, static_cast<int>(p->n), p->frame,
                                          p->ord.d_pts, p->ord.d_pts32q, s));
  HIP_TRY(hipStreamSynchronize(s));
  p->ord_on = true;
  p->ord_first = first;
  ++p->ord_installs;
  return RS_OK;
}

// Complete the last run (its pending tail) and wait.  Accessors below then read its buffer
// set synchronously.  The one place an order is installed: a read flush of a plan that has
// issued more than one run on the resident points (f8::order_installs).
static int plan_wait(rs_f8_plan *p) {
  if (p->s.runs == 0) return fail(RS_EINVAL, "no run has been issued on this plan");
  if (p->s.pending) {
    int st = plan_flush(p, f8::FlushFor::kRead);
    if (st) return st;
    const bool enabled = p->order && p->knobs.prune && p->use_fp32 && p->fp32_ok;
    if (f8::order_installs(enabled, p->ord_on, p->runs_since_points)) return order_install(p);
    return RS_OK;
  }
  if (p->unread_dropped)
    return fail(RS_EINVAL, "the last run fell back and its results were dropped before they were read");
  return RS_OK;
}

extern "C" int rs_f8_plan_result(rs_f8_plan *p, rs_f8_result *out, int64_t *inliers, int64_t cap,
                                 int64_t *n_inliers) {
  if (!p || !out) return fail(RS_EINVAL, "null pointer");
  int st = plan_wait(p);
  if (st) return st;
  const rsd::F8DevResult *r = p->h_slot[(p->s.runs - 1) % rs_f8_plan::kSlots];
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
    const int *h = p->h_inl[(p->s.runs - 1) % rs_f8_plan::kSlots];  // written by the tail
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

// Whether the last run (complete and, if so, recounted: after plan_wait) was carried and fell
// back, by the test the tail made on the device (carry_fell_back in f8_kernels.hip)
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
    src = b.d_counts_fb;  // the recount counted every hypothesis in full
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
    rsd::CountArgs ca = count_args(p, b, h);
    ca.counts = p->d_full;
    ca.gdone = ca.status = nullptr;  // no fused c*
    HIP_TRY(rsd::launch_f8_count32q(rsd::kCountWhole, ca, sh, 0, {}, s));
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

extern "C" int rs_f8_plan_recount_stats(rs_f8_plan *p, int64_t *out) {
  if (!p || !out) return fail(RS_EINVAL, "null pointer");
  out[0] = p->n_recounts;
  out[1] = p->count_launches;
  return RS_OK;
}

extern "C" int rs_f8_plan_order_stats(rs_f8_plan *p, int64_t *out) {
  if (!p || !out) return fail(RS_EINVAL, "null pointer");
  out[0] = p->ord_on ? 1 : 0;
  out[1] = p->ord_on ? p->ord_first : 0;
  out[2] = p->ord_installs;
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
      1, std::min<int64_t>({last_n, p->s.runs, static_cast<int64_t>(rs_f8_plan::kEvRing)}));
  double sa = 0, sb = 0, sc = 0;
  int64_t nt = 0;
  for (int64_t r = p->s.runs - k; r < p->s.runs; ++r) {
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
  int st = plan_flush(p, f8::FlushFor::kDrop);  // runs in flight use the current kernel's buffers
  if (st) return st;
  p->use_fp32 = fp64 == 0;
  f8::carry_drop(p->s);
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
  *waits = p->s.lane_waits;
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
