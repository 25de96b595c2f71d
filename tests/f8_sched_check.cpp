// Stand-alone check of the F plan's host decisions (csrc/f8_sched.h), host only: no device.
// Built and run by tests/test_f8_sched_cpu.py; exits 0 when every check holds.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "f8_sched.h"

namespace f8 = rs::f8;

static int failures = 0;

#define CHECK(cond)                                               \
  do {                                                            \
    if (!(cond)) {                                                \
      std::printf("line %d: %s does not hold\n", __LINE__, #cond); \
      ++failures;                                                 \
    }                                                             \
  } while (0)

// ---- layout ----------------------------------------------------------------------------------
struct Span {
  size_t off, bytes;
};

// the arenas at made-up addresses far apart (nothing is dereferenced)
static void fake_bases(f8::Arenas &a) {
  a.hyp = reinterpret_cast<char *>(uintptr_t(1) << 40);
  a.pts = reinterpret_cast<char *>(uintptr_t(2) << 40);
  a.slot = reinterpret_cast<char *>(uintptr_t(3) << 40);
  a.slot_dev = reinterpret_cast<char *>(uintptr_t(4) << 40);
  a.inl = reinterpret_cast<char *>(uintptr_t(5) << 40);
  a.inl_dev = reinterpret_cast<char *>(uintptr_t(6) << 40);
}

template <class T>
static Span span(const T *p, const char *base, size_t count) {
  return Span{static_cast<size_t>(reinterpret_cast<const char *>(p) - base), sizeof(T) * count};
}

// inside the arena, 256-aligned, disjoint, and nothing but padding between them
static void check_arena(std::vector<Span> v, size_t total) {
  std::sort(v.begin(), v.end(), [](const Span &x, const Span &y) { return x.off < y.off; });
  size_t end = 0;
  for (const Span &s : v) {
    CHECK(s.off % 256 == 0);
    CHECK(s.off == end);  // no overlap, no hole
    CHECK(s.bytes > 0 && s.off + s.bytes <= total);
    end = s.off + (s.bytes + 255) / 256 * 256;
  }
  CHECK(end == total);
}

static std::vector<Span> hyp_spans(const f8::PlanBufs &m, size_t ld) {
  std::vector<Span> v;
  const char *base = m.mem.hyp;
  for (const f8::RunBufs &b : m.buf) {
    v.push_back(span(b.d_F, base, 9 * ld));
    v.push_back(span(b.d_F32, base, 9 * ld));
    v.push_back(span(b.d_counts, base, ld));
    v.push_back(span(b.d_tuples, base, 8 * ld));
    v.push_back(span(b.d_cand, base, ld));
    v.push_back(span(b.d_status, base, rsd::kStatusWords));
    v.push_back(span(b.d_ccount, base, ld));
    v.push_back(span(b.d_cfast, base, ld));
    v.push_back(span(b.d_spec_j, base, rsd::kSelectBlocks));
    v.push_back(span(b.d_cstd, base, ld));
    v.push_back(span(b.d_cnorm, base, ld));
    v.push_back(span(b.d_gdone, base, ld / 64));
    v.push_back(span(b.d_G4, base, ld));
    v.push_back(span(b.d_pw, base, rsd::kPruneWords));
    v.push_back(span(b.d_surv, base, ld));
    v.push_back(span(b.d_gdone_b, base, ld / 64));
    v.push_back(span(b.d_counts_fb, base, ld));
    v.push_back(span(b.d_gdone_fb, base, ld / 64));
    v.push_back(span(b.d_fbw, base, 1));
  }
  v.push_back(span(m.d_carry, base, f8::kLanes + 1));
  return v;
}

static void check_layout(int64_t n, int64_t max_hyp) {
  const size_t ld = static_cast<size_t>((max_hyp + 63) / 64 * 64), np = static_cast<size_t>(n);
  f8::PlanBufs m;
  f8::plan_layout(m, max_hyp, n);  // unbound: sizes only
  CHECK(m.d_carry == nullptr && m.d_pts == nullptr && m.h_slot[0] == nullptr && m.buf[3].d_spec == nullptr);
  const f8::Arenas sizes = m.mem;
  fake_bases(m.mem);
  f8::plan_layout(m, max_hyp, n);
  const f8::Arenas &a = m.mem;
  CHECK(a.hyp_bytes == sizes.hyp_bytes && a.pts_bytes == sizes.pts_bytes &&
        a.slot_bytes == sizes.slot_bytes && a.inl_bytes == sizes.inl_bytes);
  CHECK(ld % 64 == 0 && ld >= static_cast<size_t>(max_hyp) && ld < static_cast<size_t>(max_hyp) + 64);

  const std::vector<Span> hyp = hyp_spans(m, ld);
  check_arena(hyp, a.hyp_bytes);

  std::vector<Span> pts = {span(m.d_p12, a.pts, 4 * np), span(m.d_pts, a.pts, np),
                           span(m.d_pts32q, a.pts, (np + 7) / 8 * 8)};
  for (const f8::RunBufs &b : m.buf) pts.push_back(span(b.d_spec, a.pts, rsd::kSelectBlocks * np));
  check_arena(pts, a.pts_bytes);
  CHECK(sizeof(rsd::Pt) == 32 && sizeof(float4) == 16);

  std::vector<Span> slot, inl;
  for (int k = 0; k < f8::kSlots; ++k) {
    slot.push_back(span(m.h_slot[k], a.slot, 1));
    inl.push_back(span(m.h_inl[k], a.inl, np));
    // the device mapping: the same offsets from the other base
    CHECK(span(m.h_slot_dev[k], a.slot_dev, 1).off == slot.back().off);
    CHECK(span(m.h_inl_dev[k], a.inl_dev, np).off == inl.back().off);
  }
  check_arena(slot, a.slot_bytes);
  check_arena(inl, a.inl_bytes);

  // a regrow (plan_retarget's rule, to hold n + 1 points) moves nothing per hypothesis
  const int64_t cap = std::max<int64_t>(n + 1, n + n / 4);
  f8::plan_layout(m, max_hyp, cap);
  const std::vector<Span> again = hyp_spans(m, ld);
  CHECK(m.mem.hyp_bytes == sizes.hyp_bytes && m.mem.slot_bytes == sizes.slot_bytes);
  CHECK(m.mem.pts_bytes > sizes.pts_bytes && m.mem.inl_bytes >= sizes.inl_bytes);
  for (size_t k = 0; k < hyp.size(); ++k) CHECK(again[k].off == hyp[k].off);
  CHECK(span(m.h_slot[3], m.mem.slot, 1).off == slot[3].off);
}

// ---- placement -------------------------------------------------------------------------------
enum Tok { RUN, RUN_NP, RESULT };

// what rs_f8_plan_run / rs_f8_plan_run_np / rs_f8_plan_result do to the state
static f8::Placement step(f8::Sched &s, Tok t) {
  f8::Placement pl{-1, false, -1};
  if (t == RESULT) {
    if (s.pending) f8::flushed(s);
    return pl;
  }
  if (t == RUN_NP) f8::lane_drained(s, 1);  // the entry point, before its parse
  pl = f8::place(s, t == RUN_NP);
  f8::committed(s, pl.lane);
  return pl;
}

static void replay(f8::Sched &s, const std::vector<Tok> &seq) {
  for (Tok t : seq) step(s, t);
}

static void check_lanes_sequences() {
  f8::Sched s;
  std::vector<Tok> seq;
  const auto batch = [&](int runs) {
    seq.insert(seq.end(), runs, RUN);
    seq.push_back(RESULT);
  };
  for (int k = 0; k < 6; ++k) batch(3);          // 3 runs + result(), in a loop
  for (int b : {5, 20, 1, 7, 2}) batch(b);       // the driver's warm-up + timed runs, odd sizes
  for (int b : {3, 5}) batch(2 * b);             // host tuples mixed with Philox runs
  batch(9);                                      // the timed part: placement does not see timing
  replay(s, seq);
  CHECK(s.lane_waits == 0);
  CHECK(s.runs == 18 + 35 + 16 + 9 && !s.pending && !s.busy[0] && !s.busy[1]);
  replay(s, {RUN, RUN, RUN_NP, RESULT});  // a parity run behind a run in flight on lane 1
  CHECK(s.lane_waits == 1);
}

// every sequence of Philox runs and results of the given length
static void check_all_sequences(int len) {
  for (unsigned bits = 0; bits < (1u << len); ++bits) {
    f8::Sched s;
    bool in_flight = false;  // a run since the last flush
    int prev = 0;
    int64_t flushed_at = 0;  // runs issued at the last flush
    for (int i = 0; i < len; ++i) {
      if (bits >> i & 1) {
        const int k = static_cast<int>(s.runs % f8::kBufs);
        const int was_lane = s.set_lane[k];
        const int64_t was_run = s.set_last_run[k];
        const f8::Placement pl = step(s, RUN);
        CHECK(pl.lane == (in_flight ? 1 - prev : 0));
        CHECK(was_lane == pl.lane || was_run < flushed_at);
        CHECK(!pl.drain1 && pl.guard < 0);
        CHECK(s.set_lane[k] == pl.lane && s.set_last_run[k] == s.runs - 1);
        prev = pl.lane;
        in_flight = true;
      } else {
        step(s, RESULT);
        in_flight = false;
        flushed_at = s.runs;
      }
    }
    CHECK(s.lane_waits == 0);
  }
}

static void check_placement_details() {
  // one lane: always lane 0, never a wait
  f8::Sched one;
  one.overlap = false;
  for (int i = 0; i < 9; ++i) CHECK(step(one, RUN).lane == 0);
  CHECK(one.lane_waits == 0);
  // run, run, run_np: the entry point drains lane 1; the run itself finds it idle, and its set (2)
  // was never used, so no guard
  f8::Sched s;
  step(s, RUN);
  step(s, RUN);
  CHECK(s.busy[0] && s.busy[1] && s.last_lane == 1);
  f8::Placement pl = step(s, RUN_NP);
  CHECK(pl.lane == 0 && !pl.drain1 && pl.guard < 0 && s.lane_waits == 1 && s.synced[1] == 2);
  // the next Philox run goes to lane 1 with set 3 (unused); the one after to lane 0 with set 0,
  // last used on lane 0: still no guard.  Two parity runs later set 1 (run 1, lane 1, complete
  // since the drain at 2) comes back on lane 0: run 1 < synced[1], no wait
  CHECK(step(s, RUN).lane == 1);
  CHECK(step(s, RUN).lane == 0);
  pl = step(s, RUN_NP);  // run 5, set 1: drains lane 1 (run 3) in the entry point
  CHECK(pl.lane == 0 && pl.guard < 0 && s.lane_waits == 2);
  // the set guard proper: run 6 goes to lane 1 with set 2, which the parity run 2 used on lane 0;
  // the host has not waited for lane 0 since (synced[0] = 0) and lane 0 has work: it waits
  pl = step(s, RUN);
  CHECK(pl.lane == 1 && pl.guard == 0 && !pl.drain1 && s.lane_waits == 3);
  CHECK(s.synced[0] == 6 && !s.busy[0] && s.busy[1]);
  // run 7, a parity run: the entry point waits for lane 1; set 3 (run 3, lane 1) is complete
  pl = step(s, RUN_NP);
  CHECK(pl.lane == 0 && pl.guard < 0 && s.lane_waits == 4 && s.synced[1] == 7);
  // run 8 on lane 1 with set 0 (run 4, lane 0), complete since the wait at 6: no guard
  pl = step(s, RUN);
  CHECK(pl.lane == 1 && pl.guard < 0 && s.lane_waits == 4);
  // placing with device tuples while lane 1 is busy asks for the drain itself
  f8::Sched d;
  step(d, RUN);
  step(d, RUN);
  pl = f8::place(d, true);
  CHECK(pl.lane == 0 && pl.drain1 && pl.guard < 0 && d.lane_waits == 1);
  // timing: every k-th run at the plan's level; exclusive when the other lane has work
  CHECK(f8::timing_level(0, 2, 3) == 2 && f8::timing_level(1, 2, 3) == 0 && f8::timing_level(6, 1, 3) == 1);
  CHECK(f8::timing_level(5, 1, 1) == 1 && f8::timing_level(5, 0, 1) == 0);
  f8::Sched t;
  CHECK(!f8::exclusive(t, 0, 1));
  step(t, RUN);
  CHECK(f8::exclusive(t, 1, 1) && f8::exclusive(t, 1, 2) && !f8::exclusive(t, 1, 0) && !f8::exclusive(t, 0, 1));
}

// ---- count path ------------------------------------------------------------------------------
static void check_count_path() {
  const f8::PruneKnobs k;  // the defaults: prune, sample of 32 groups, carry
  f8::Sched s;
  f8::CountPath cp = f8::count_path(s, k, 0, 64 * k.sample, 1.5, true);
  CHECK(!cp.staged && !cp.carried && cp.h0 == 64 * k.sample);  // H <= 64 * prune_sample
  cp = f8::count_path(s, k, 0, 1, 1.5, true);
  CHECK(!cp.staged && cp.h0 == 1);
  // first staged run on a lane: not carried; the second with the same H and threshold: carried
  for (int lane = 0; lane < 2; ++lane) {
    cp = f8::count_path(s, k, lane, 4000, 1.5, true);
    CHECK(cp.staged && !cp.carried && cp.h0 == 2048);
    f8::carry_left(s, lane, 4000, 1.5, true);
  }
  CHECK(s.carry_ok[0] && s.carry_ok[1] && s.carry_H == 4000 && s.carry_thresh == 1.5);
  for (int lane = 0; lane < 2; ++lane) {
    cp = f8::count_path(s, k, lane, 4000, 1.5, true);
    CHECK(cp.staged && cp.carried);
    f8::carry_left(s, lane, 4000, 1.5, true);
  }
  // a change of the threshold, then of H: both lanes dropped, the run is a sample run again
  cp = f8::count_path(s, k, 0, 4000, 2.0, true);
  CHECK(cp.staged && !cp.carried && !s.carry_ok[0] && !s.carry_ok[1]);
  f8::carry_left(s, 0, 4000, 2.0, true);
  CHECK(s.carry_ok[0] && !s.carry_ok[1]);
  cp = f8::count_path(s, k, 1, 4000, 2.0, true);  // lane 1 has no word of its own yet
  CHECK(cp.staged && !cp.carried && s.carry_ok[0]);
  f8::carry_left(s, 1, 4000, 2.0, true);
  cp = f8::count_path(s, k, 0, 3999, 2.0, true);
  CHECK(cp.staged && !cp.carried && !s.carry_ok[0] && !s.carry_ok[1]);
  // set_points / set_count_precision (carry_drop): both lanes
  f8::carry_left(s, 0, 3999, 2.0, true);
  f8::carry_left(s, 1, 3999, 2.0, true);
  f8::carry_drop(s);
  CHECK(!s.carry_ok[0] && !s.carry_ok[1]);
  // fp64 count: never staged, leaves no word, drops the others
  f8::carry_left(s, 0, 3999, 2.0, true);
  cp = f8::count_path(s, k, 0, 3999, 2.0, false);
  CHECK(!cp.staged && !cp.carried && !s.carry_ok[0]);
  f8::carry_left(s, 0, 3999, 2.0, false);
  CHECK(!s.carry_ok[0]);
  // the switches
  f8::PruneKnobs off = k;
  off.prune = 0;
  CHECK(!f8::count_path(s, off, 0, 4000, 1.5, true).staged);
  f8::PruneKnobs nocarry = k;
  nocarry.carry = 0;
  f8::carry_left(s, 0, 4000, 1.5, true);
  cp = f8::count_path(s, nocarry, 0, 4000, 1.5, true);
  CHECK(cp.staged && !cp.carried);
  f8::PruneKnobs one = k;
  one.sample = 1;
  CHECK(f8::count_path(s, one, 0, 65, 1.5, true).staged && f8::count_path(s, one, 0, 65, 1.5, true).h0 == 64);
  CHECK(!f8::count_path(s, one, 0, 64, 1.5, true).staged);
}

static void check_prune_numbers() {
  const f8::PruneKnobs k;
  const int want[4][4] = {{8, 16, 8, 16}, {257, 16, 32, 16}, {600, 20, 75, 16}, {3000, 100, 375, 60}};
  for (const auto &w : want) {
    const f8::PruneNumbers c = f8::prune_numbers(k, w[0], true), s = f8::prune_numbers(k, w[0], false);
    CHECK(c.margin == w[1] && c.min_skip == w[2] && c.gap == w[3] && c.g_first == 0);
    CHECK(s.margin == w[1] && s.min_skip == w[2] && s.gap == 0 && s.g_first == 32);
    // today's expressions
    CHECK(c.margin == std::max(16, w[0] / 30) && c.min_skip == std::max(8, w[0] / 8) &&
          c.gap == std::max(16, w[0] / 50));
  }
  // the overrides and their clamps
  f8::PruneKnobs o;
  o.margin = 5000;
  o.min_skip = 3;
  o.carry_gap = -7;
  o.carry_gap_set = true;
  o.sample = 1 << 30;
  f8::PruneNumbers pn = f8::prune_numbers(o, 600, true);
  CHECK(pn.margin == 600 && pn.min_skip == 8 && pn.gap == -7 && pn.g_first == 0);
  pn = f8::prune_numbers(o, 600, false);
  CHECK(pn.g_first == 1 << 24 && pn.gap == 0);
  o.margin = 0;
  o.min_skip = 100;
  CHECK(f8::prune_numbers(o, 600, false).margin == 0 && f8::prune_numbers(o, 600, false).min_skip == 100);

  // choose_chunk: today's expression
  for (int64_t n : {8, 9, 63, 64, 65, 257, 600, 3000, 1 << 20})
    for (int64_t H : {1, 63, 64, 65, 500, 4000, 1 << 20}) {
      const int64_t groups = (H + 63) / 64;
      int64_t nch = (8192 + groups - 1) / groups;
      nch = std::max<int64_t>(1, std::min<int64_t>(nch, (n + 63) / 64));
      CHECK(f8::choose_chunk(n, H) == static_cast<int>((n + nch - 1) / nch));
    }
  CHECK(f8::choose_chunk(600, 4000) == 60 && f8::choose_chunk(8, 1) == 8);
}

int main() {
  for (int64_t n : {8, 9, 15, 16, 17, 600, 1 << 20})
    for (int64_t max_hyp : {1, 63, 64, 65, 4000}) check_layout(n, max_hyp);
  check_lanes_sequences();
  for (int len = 1; len <= 12; ++len) check_all_sequences(len);
  check_placement_details();
  check_count_path();
  check_prune_numbers();
  if (failures == 0) std::printf("f8 sched ok\n");
  return failures == 0 ? 0 : 1;
}
