// Stand-alone check of rs::Layout's arithmetic (csrc/host.h), host only: no device, no context.
// Built and run by tests/test_host_layout_cpu.py; exits 0 when every check holds.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "host.h"

static int failures = 0;

#define CHECK(cond)                                               \
  do {                                                            \
    if (!(cond)) {                                                \
      std::printf("line %d: %s does not hold\n", __LINE__, #cond); \
      ++failures;                                                 \
    }                                                             \
  } while (0)

int main() {
  // zeros (first, in the middle, doubled, last), non-multiples of 256, exactly 256, above 4 GiB
  const std::vector<size_t> sizes = {0,   1,    255, 256, 257, 0, 0, 1000, (size_t(5) << 30) + 3,
                                     0,   4096, 12,  0};
  const size_t n = sizes.size();
  std::vector<size_t> want(n + 1, 0);
  for (size_t k = 0; k < n; ++k) want[k + 1] = want[k] + (sizes[k] + 255) / 256 * 256;

  rs::Layout L;
  std::vector<rs::Layout::Buf<char>> b;
  for (size_t s : sizes) b.push_back(L.add<char>(s));
  for (size_t k = 0; k < n; ++k) {
    CHECK(b[k].off == want[k]);
    CHECK(b[k].bytes == sizes[k]);
    CHECK(L.upto(b[k]) == want[k]);
    CHECK(L.from(b[k]) == want[n] - want[k]);  // "from buffer k to the end"
    if (sizes[k] == 0 && k + 1 < n) CHECK(b[k].off == b[k + 1].off);
    for (size_t j = k; j < n; ++j) CHECK(L.span(b[k], b[j]) == want[j] - want[k]);
  }
  CHECK(L.total() == want[n]);
  CHECK(want[n] > (size_t(1) << 32));
  CHECK(rs::align256(0) == 0 && rs::align256(1) == 256 && rs::align256(256) == 256 &&
        rs::align256(257) == 512);
  CHECK(rs::blocks(0, 256) == 0 && rs::blocks(1, 256) == 1 && rs::blocks(256, 256) == 1 &&
        rs::blocks(257, 256) == 2 && rs::blocks((int64_t(1) << 33) + 1, 128) == (1u << 26) + 1);

  // element types scale the count; add_bytes takes the size as given
  rs::Layout T;
  const auto d = T.add<double>(3);
  const auto i = T.add<int32_t>(65);
  const auto z = T.add<int64_t>(0);
  const auto r = T.add_bytes<double>(100);
  CHECK(d.off == 0 && d.bytes == 24);
  CHECK(i.off == 256 && i.bytes == 260);
  CHECK(z.off == 768 && z.bytes == 0 && r.off == 768 && r.bytes == 100);
  CHECK(T.total() == 1024);

  // the handles' pointers: the same offsets from the device base and from the pinned mirror
  std::vector<char> dev(T.total()), host(T.total());
  T.bind(dev.data(), host.data());
  CHECK(T.dev() == dev.data() && T.host() == host.data());
  CHECK(reinterpret_cast<char *>(i.dev()) == dev.data() + 256);
  CHECK(reinterpret_cast<char *>(i.host()) == host.data() + 256);
  CHECK(reinterpret_cast<char *>(r.dev()) == dev.data() + 768);

  // packed layouts (pad 1) and a start moved up to a multiple
  rs::Layout P(1);
  const auto p0 = P.add<char>(5);
  const auto p1 = P.add<double>(2);
  const auto p2 = P.add<char>(0);
  CHECK(p0.off == 0 && p1.off == 5 && p2.off == 21 && P.total() == 21);
  CHECK(P.skip_to(64) == 43 && P.total() == 64 && P.skip_to(64) == 0);
  const auto p3 = P.add<char>(7);
  CHECK(p3.off == 64 && P.total() == 71 && P.from(p1) == 66);

  if (failures == 0) std::printf("layout ok\n");
  return failures == 0 ? 0 : 1;
}
