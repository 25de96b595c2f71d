// Stand-alone check of the F plan's deferred-recount decision (csrc/f8_sched.h, flush_recounts and
// flush_drops_unread), host only: no device.  Built and run by tests/test_f8_recount_cpu.py; exits
// 0 when every check holds.
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

// ---- the decision, every input ----------------------------------------------------------------
static void truth_table() {
  for (int pending = 0; pending < 2; ++pending)
    for (int carried = 0; carried < 2; ++carried)
      for (int flag = 0; flag < 2; ++flag) {
        const bool rec = f8::flush_recounts(pending, carried, flag, f8::FlushFor::kRead);
        const bool rec_drop = f8::flush_recounts(pending, carried, flag, f8::FlushFor::kDrop);
        const bool lost = f8::flush_drops_unread(pending, carried, flag, f8::FlushFor::kDrop);
        const bool lost_read = f8::flush_drops_unread(pending, carried, flag, f8::FlushFor::kRead);
        // a recount: a carried last run, not yet flushed, marked, and somebody reads it
        CHECK(rec == (pending && carried && flag));
        // a dropping flush never recounts; a reading one never loses a run
        CHECK(!rec_drop);
        CHECK(!lost_read);
        CHECK(lost == (pending && carried && flag));
        // never both at one flush
        CHECK(!(rec && lost_read) && !(rec_drop && lost));
      }
  // the cases by name
  CHECK(f8::flush_recounts(true, true, true, f8::FlushFor::kRead));     // carried, fell back, read
  CHECK(!f8::flush_recounts(true, true, false, f8::FlushFor::kRead));   // carried, exact
  CHECK(!f8::flush_recounts(true, false, true, f8::FlushFor::kRead));   // a stale mark in the slot
  CHECK(!f8::flush_recounts(true, false, false, f8::FlushFor::kRead));  // a sample run
  CHECK(!f8::flush_recounts(true, true, true, f8::FlushFor::kDrop));    // set_points, destroy
  CHECK(!f8::flush_recounts(false, true, true, f8::FlushFor::kRead));   // nothing pending
}

// ---- the plan's use of it (f8_plan.hip, plan_flush / plan_wait / plan_run) over call sequences -
// What the host keeps, with the scheduler's own state: the slot flags stand for the pinned headers
// (a run's tail sets or clears its slot's flag; complete at the flush).
struct Model {
  f8::Sched s;
  bool carried[f8::kBufs] = {};
  bool flag[f8::kSlots] = {true, true, true, true};  // pinned memory starts with anything
  bool unread_dropped = false;
  int64_t recounts = 0;

  void run(bool is_carried, bool falls_back) {
    const int k = static_cast<int>(s.runs % f8::kBufs);
    const f8::Placement pl = f8::place(s, false);
    carried[k] = is_carried;
    flag[s.runs % f8::kSlots] = is_carried && falls_back;
    f8::committed(s, pl.lane);
    unread_dropped = false;
  }
  void flush(f8::FlushFor why) {
    const bool pending = s.pending && s.runs > 0;
    const bool c = pending && carried[(s.runs - 1) % f8::kBufs];
    const bool m = c && flag[(s.runs - 1) % f8::kSlots];
    f8::flushed(s);
    if (f8::flush_drops_unread(pending, c, m, why)) unread_dropped = true;
    if (f8::flush_recounts(pending, c, m, why)) {
      ++recounts;
      flag[(s.runs - 1) % f8::kSlots] = false;  // the second pass of the tail fills the slot
    }
  }
  // an accessor: false when it has to refuse
  bool read() {
    if (s.runs == 0) return false;
    if (s.pending) {
      flush(f8::FlushFor::kRead);
      return true;
    }
    return !unread_dropped;
  }
};

static void sequences() {
  // every sequence of up to 9 calls out of: a sample run, a carried run that is exact, a carried
  // run that falls back, a read, a dropping flush
  const int kCalls = 5, kLen = 9;
  std::vector<int> seq(kLen, 0);
  int64_t total = 1;
  for (int i = 0; i < kLen; ++i) total *= kCalls;
  for (int64_t code = 0; code < total; ++code) {
    int64_t c = code;
    for (int i = 0; i < kLen; ++i) {
      seq[i] = static_cast<int>(c % kCalls);
      c /= kCalls;
    }
    Model m;
    int64_t want = 0;        // recounts: reads whose last run fell back and was not yet flushed
    int last = -1;           // the last run's kind, -1 none
    bool flushed = true, lost = false;
    for (int i = 0; i < kLen; ++i) {
      switch (seq[i]) {
        case 0: case 1: case 2:
          m.run(seq[i] != 0, seq[i] == 2);
          last = seq[i];
          flushed = false;
          lost = false;
          break;
        case 3: {
          const bool ok = m.read();
          if (last < 0) {
            CHECK(!ok);
            break;
          }
          if (!flushed && last == 2) ++want;
          flushed = true;
          CHECK(ok == !lost);
          // what is read is complete: no mark left on the last run's slot
          if (ok) CHECK(!(m.carried[(m.s.runs - 1) % f8::kBufs] && m.flag[(m.s.runs - 1) % f8::kSlots]));
          break;
        }
        case 4:
          m.flush(f8::FlushFor::kDrop);
          if (!flushed && last == 2) lost = true;
          flushed = true;
          break;
      }
      CHECK(m.recounts == want);
      if (failures > 20) return;
    }
  }
}

int main() {
  truth_table();
  sequences();
  if (failures) {
    std::printf("%d checks failed\n", failures);
    return 1;
  }
  std::printf("f8 recount ok\n");
  return 0;
}
