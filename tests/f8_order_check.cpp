// Stand-alone check of the F plan's point order (csrc/f8_order.h), host only: no device.
// Built and run by tests/test_f8_order_cpu.py; exits 0 when every check holds.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>

#include "f8_order.h"

namespace f8 = rs::f8;

static int failures = 0;

#define CHECK(cond)                                               \
  do {                                                            \
    if (!(cond)) {                                                \
      std::printf("line %d: %s does not hold\n", __LINE__, #cond); \
      ++failures;                                                 \
    }                                                             \
  } while (0)

static bool is_identity(const std::vector<int32_t> &perm) {
  for (size_t i = 0; i < perm.size(); ++i)
    if (perm[i] != static_cast<int32_t>(i)) return false;
  return true;
}

static bool is_permutation(const std::vector<int32_t> &perm) {
  std::vector<int> seen(perm.size(), 0);
  for (int32_t v : perm) {
    if (v < 0 || static_cast<size_t>(v) >= perm.size() || seen[v]) return false;
    seen[v] = 1;
  }
  return true;
}

// the builder on the subset `bits` of [0, n) as the winner's inlier list
static int64_t build(int n, unsigned bits, int64_t best_count, std::vector<int32_t> &perm) {
  std::vector<int> inl;
  for (int i = 0; i < n; ++i)
    if ((bits >> i) & 1u) inl.push_back(i);
  perm.assign(n, -7);
  std::vector<unsigned char> mark(n, 0xAA);
  return f8::order_outliers_first(inl.data(), static_cast<int64_t>(inl.size()), best_count, n,
                                  perm.data(), mark.data());
}

// every subset pattern of every n <= 12: a permutation whatever the list; the winner's outliers
// first and its inliers after them, each ascending; the identity when there is nothing to order by
static void check_every_subset() {
  for (int n = 1; n <= 12; ++n)
    for (unsigned bits = 0; bits < (1u << n); ++bits) {
      const int k = __builtin_popcount(bits);
      std::vector<int32_t> perm;
      // the count the plan passes: the size of the list
      int64_t first = build(n, bits, k, perm);
      CHECK(is_permutation(perm));
      if (k <= f8::kOrderMinCount || k == n) CHECK(first == 0 && is_identity(perm));
      // a count above the floor, so that small lists are ordered too
      first = build(n, bits, f8::kOrderMinCount + 1, perm);
      CHECK(is_permutation(perm));
      if (k == 0 || k == n) {
        CHECK(first == 0 && is_identity(perm));
        continue;
      }
      CHECK(first == n - k);
      for (int i = 0; i < n; ++i) {
        const bool inl = (bits >> perm[i]) & 1u;
        CHECK(inl == (i >= first));
        if (i > 0 && i != first) CHECK(perm[i - 1] < perm[i]);
      }
    }
}

static void check_identity_cases() {
  const int n = 40;
  std::vector<int32_t> perm(n);
  std::vector<unsigned char> mark(n);
  std::vector<int> inl;
  for (int i = 0; i < n; i += 2) inl.push_back(i);  // 20 inliers
  const int64_t k = static_cast<int64_t>(inl.size());
  auto run = [&](const int *l, int64_t nl, int64_t best) {
    std::fill(perm.begin(), perm.end(), -1);
    return f8::order_outliers_first(l, nl, best, n, perm.data(), mark.data());
  };
  CHECK(run(inl.data(), k, k) == n - k && !is_identity(perm) && is_permutation(perm));
  for (int64_t best : {-1, 0, 1, 8}) CHECK(run(inl.data(), k, best) == 0 && is_identity(perm));
  CHECK(run(inl.data(), k, 9) == n - k);
  CHECK(run(inl.data(), 0, k) == 0 && is_identity(perm));       // an empty list
  CHECK(run(nullptr, k, k) == 0 && is_identity(perm));
  std::vector<int> all(n);
  for (int i = 0; i < n; ++i) all[i] = i;
  CHECK(run(all.data(), n, n) == 0 && is_identity(perm));        // an empty outlier set
  CHECK(run(all.data(), n + 5, n) == 0 && is_identity(perm));    // a list longer than n is not read
  // a list that is no set of indices of [0, n) is not followed
  std::vector<int> bad = inl;
  bad[3] = n;
  CHECK(run(bad.data(), k, k) == 0 && is_identity(perm));
  bad[3] = -1;
  CHECK(run(bad.data(), k, k) == 0 && is_identity(perm));
  bad[3] = bad[2];
  CHECK(run(bad.data(), k, k) == 0 && is_identity(perm));
  // an unsorted list of distinct indices orders as its set does
  std::vector<int> rev(inl.rbegin(), inl.rend());
  std::vector<int32_t> want(n);
  CHECK(run(inl.data(), k, k) == n - k);
  want = perm;
  CHECK(run(rev.data(), k, k) == n - k && perm == want);
}

static void check_installs() {
  CHECK(!f8::order_installs(true, false, 0) && !f8::order_installs(true, false, 1));
  CHECK(f8::order_installs(true, false, 2) && f8::order_installs(true, false, 300));
  CHECK(!f8::order_installs(false, false, 2) && !f8::order_installs(true, true, 2));
  // the margin: n / 60 (at least 16) only while an order is installed and none was given
  const f8::PruneKnobs k;
  for (int n : {8, 257, 600, 2000, 10000}) {
    const int m = f8::prune_numbers(k, n, true).margin;
    CHECK(f8::order_margin(m, false, n, false) == m && f8::order_margin(m, true, n, true) == m);
    CHECK(f8::order_margin(m, false, n, true) == std::max(16, n / 60));
    CHECK(f8::order_margin(m, false, n, true) <= m);
  }
  CHECK(f8::order_margin(66, false, 2000, true) == 33 && f8::order_margin(16, false, 257, true) == 16);
}

static void check_layout() {
  for (int64_t n : {8, 9, 15, 16, 17, 257, 600, 1 << 20}) {
    f8::OrderBufs o;
    f8::order_layout(o, nullptr, n);
    CHECK(o.d_perm == nullptr && o.d_pts == nullptr && o.d_pts32q == nullptr && o.bytes > 0);
    const size_t bytes = o.bytes;
    char *base = reinterpret_cast<char *>(uintptr_t(2) << 40);
    f8::order_layout(o, base, n);
    const size_t np = static_cast<size_t>(n), npad = (np + 7) / 8 * 8;
    const size_t off[3] = {static_cast<size_t>(reinterpret_cast<char *>(o.d_perm) - base),
                           static_cast<size_t>(reinterpret_cast<char *>(o.d_pts) - base),
                           static_cast<size_t>(reinterpret_cast<char *>(o.d_pts32q) - base)};
    const size_t len[3] = {sizeof(int32_t) * np, sizeof(rsd::Pt) * np, sizeof(float4) * npad};
    size_t end = 0;
    for (int k = 0; k < 3; ++k) {
      CHECK(off[k] % 256 == 0 && off[k] == end);
      end = off[k] + (len[k] + 255) / 256 * 256;
    }
    CHECK(end == bytes && o.bytes == bytes);
  }
}

// The drop rule under the permuted order, on random planes.  inl[h][i]: point i is an inlier of
// hypothesis h; cert[h][i]: the screen certifies it an outlier (one-sided: never an inlier).  The
// prefix stage sums the certificates of the first K points of the order, c' = K - o, and drops h
// when c' + (n - K) < L - 1.  Whatever the permutation: a hypothesis with full count >= L - 1
// survives, and a dropped one has full count <= c' + (n - K).
static void check_rule_on_planes() {
  std::mt19937 rng(12345);
  int dropped_all = 0, fewer = 0, more = 0;
  for (int trial = 0; trial < 200; ++trial) {
    const int n = 16 + static_cast<int>(rng() % 240), H = 64;
    const double p_good = 0.3 + 0.5 * (rng() % 1000) / 1000.0;
    std::vector<unsigned char> truth(n);
    for (auto &t : truth) t = (rng() % 1000) < 1000 * p_good;
    std::vector<std::vector<unsigned char>> inl(H, std::vector<unsigned char>(n)), cert = inl;
    std::vector<int> full(H, 0);
    for (int h = 0; h < H; ++h) {
      // a few good models (most of the true inliers), the others near chance
      const bool good = h % 8 == 0;
      for (int i = 0; i < n; ++i) {
        const unsigned r = rng() % 1000;
        inl[h][i] = good ? (truth[i] ? r < 950 : r < 30) : r < 60;
        cert[h][i] = !inl[h][i] && (rng() % 1000) < 900;  // most outliers are certified
        full[h] += inl[h][i];
      }
    }
    // the winner and its order; the bound as the carried run has it
    const int win = static_cast<int>(std::max_element(full.begin(), full.end()) - full.begin());
    std::vector<int> list;
    for (int i = 0; i < n; ++i)
      if (inl[win][i]) list.push_back(i);
    std::vector<int32_t> perm(n), ident(n);
    std::vector<unsigned char> mark(n);
    f8::order_outliers_first(list.data(), static_cast<int64_t>(list.size()), full[win], n,
                             perm.data(), mark.data());
    for (int i = 0; i < n; ++i) ident[i] = i;
    CHECK(is_permutation(perm));
    const int L = full[win] - static_cast<int>(rng() % 8), m = static_cast<int>(rng() % 24);
    const int K = std::min(n / 8 * 8, std::max(8, (n - L + m + 7) / 8 * 8));
    int surv[2] = {0, 0};
    for (int which = 0; which < 2; ++which) {
      const std::vector<int32_t> &ord = which ? perm : ident;
      for (int h = 0; h < H; ++h) {
        int o = 0;
        for (int i = 0; i < K; ++i) o += cert[h][ord[i]];
        const int cu = K - o;
        const bool keep = cu + (n - K) >= L - 1;
        if (full[h] >= L - 1) CHECK(keep);
        if (!keep) {
          CHECK(full[h] <= cu + (n - K));
          ++dropped_all;
        }
        surv[which] += keep;
      }
    }
    fewer += surv[1] < surv[0];
    more += surv[1] > surv[0];
  }
  CHECK(dropped_all > 0);  // the rule was exercised
  std::printf("planes: outliers first left fewer survivors in %d of 200, more in %d\n", fewer, more);
}

int main() {
  check_every_subset();
  check_identity_cases();
  check_installs();
  check_layout();
  check_rule_on_planes();
  if (failures == 0) std::printf("f8 order ok\n");
  return failures == 0 ? 0 : 1;
}
