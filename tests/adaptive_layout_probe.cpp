// adaptive_layout_probe.cpp — test-only sweep of split_list
// (go-raytracing_amd/csrc/wave_layout.h): how a pixel list that is already on
// the device is cut into the twins' parts.  Built with g++ under
// AddressSanitizer + UBSan by tests/test_adaptive_layout.py; needs no device.
//
// usage: adaptive_layout_probe      prints {"cases": N, "fails": F}; exit 1 if F
#include <cstdint>
#include <cstdio>

#include "../go-raytracing_amd/csrc/wave_layout.h"

using namespace rtg;

namespace {

long g_cases = 0, g_fails = 0;

#define EXPECT(cond, ...)                                      \
  do {                                                         \
    if (!(cond)) {                                             \
      if (++g_fails <= 20) {                                   \
        fprintf(stderr, "%s:%d: %s: ", __FILE__, __LINE__, #cond); \
        fprintf(stderr, __VA_ARGS__);                          \
        fputc('\n', stderr);                                   \
      }                                                        \
    }                                                          \
  } while (0)

void check(uint32_t n, int nt) {
  ++g_cases;
  uint32_t part[kMaxTwins];
  for (int t = 0; t < kMaxTwins; ++t) part[t] = 0xDEADBEEFu;
  split_list(n, nt, part);
  uint64_t sum = 0;
  for (int t = 0; t < kMaxTwins; ++t) {
    if (t >= nt) {
      EXPECT(part[t] == 0, "n %u nt %d: part %d = %u beyond the twins", n, nt, t, part[t]);
      continue;
    }
    // contiguous: part t starts where the parts before it end, at n * t / nt
    EXPECT(sum == uint64_t(n) * uint64_t(t) / uint64_t(nt), "n %u nt %d: part %d starts at %llu", n, nt, t,
           (unsigned long long)sum);
    EXPECT(part[t] != 0 || n < uint32_t(nt), "n %u nt %d: part %d is empty", n, nt, t);
    sum += part[t];
  }
  EXPECT(sum == n, "n %u nt %d: parts sum to %llu", n, nt, (unsigned long long)sum);
  // the twin count render_wave uses: never more twins than pixels
  WaveKnobs k;
  k.streams = nt;
  const int chosen = choose_twins(k, false, false, n, 16, n);
  EXPECT(chosen >= 1 && (n == 0 || uint32_t(chosen) <= n) && chosen <= nt, "n %u nt %d: choose_twins gave %d", n, nt,
         chosen);
  if (n > 0) {
    split_list(n, chosen, part);
    for (int t = 0; t < chosen; ++t) EXPECT(part[t] != 0, "n %u, %d twins chosen: part %d is empty", n, chosen, t);
  }
}

}  // namespace

int main() {
  const uint32_t ns[] = {0u, 1u, 2u, 3u, 255u, 256u, 257u, 2147483647u};
  for (uint32_t n : ns)
    for (int nt = 1; nt <= 3; ++nt) check(n, nt);
  // also the largest id count, and every twin count
  for (int nt = 1; nt <= kMaxTwins; ++nt) {
    check(4294967295u, nt);
    check(1000003u, nt);
  }
  printf("{\"cases\": %ld, \"fails\": %ld}\n", g_cases, g_fails);
  return g_fails ? 1 : 0;
}
