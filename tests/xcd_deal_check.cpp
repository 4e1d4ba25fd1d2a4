// Host-only check of the dealt hot-first map (memgraph_amd/csrc/mgx_xcd_deal.h),
// compiled and run by tests/test_xcd_deal_cpu.py. For every V given by the
// ranges on the command line (pairs "lo hi", inclusive):
//   - off is non-decreasing with off[0] = 0 and off[8] = V;
//   - the map is a bijection onto [0, V);
//   - stripe x is exactly [off[x], off[x+1]): position p, which is dealt to
//     stripe (p / 16) % 8, lands inside it, and the stripe sizes add up;
//   - positions p and p + 1 of one granule map to adjacent ids.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../memgraph_amd/csrc/mgx_xcd_deal.h"

static int check(int64_t V) {
  int64_t off[kXcdStripes + 1];
  for (int x = 0; x <= kXcdStripes; ++x) off[x] = mgx_xcd_stripe_off(V, x);
  if (off[0] != 0 || off[kXcdStripes] != V) {
    std::printf("V=%lld: off[0]=%lld off[8]=%lld\n", (long long)V, (long long)off[0],
                (long long)off[kXcdStripes]);
    return 1;
  }
  for (int x = 0; x < kXcdStripes; ++x) {
    if (off[x] > off[x + 1]) {
      std::printf("V=%lld: off decreases at %d\n", (long long)V, x);
      return 1;
    }
  }
  std::vector<uint8_t> seen((size_t)V, 0);
  std::vector<int64_t> in_stripe(kXcdStripes, 0);
  int64_t prev = -1;
  for (int64_t p = 0; p < V; ++p) {
    const int64_t id = mgx_xcd_deal(p, V);
    const int x = (int)((p / kXcdGranule) % kXcdStripes);
    if (id < 0 || id >= V) {
      std::printf("V=%lld p=%lld: id %lld out of range\n", (long long)V, (long long)p,
                  (long long)id);
      return 1;
    }
    if (seen[(size_t)id]) {
      std::printf("V=%lld p=%lld: id %lld hit twice\n", (long long)V, (long long)p,
                  (long long)id);
      return 1;
    }
    seen[(size_t)id] = 1;
    if (id < off[x] || id >= off[x + 1]) {
      std::printf("V=%lld p=%lld: id %lld outside stripe %d [%lld, %lld)\n", (long long)V,
                  (long long)p, (long long)id, x, (long long)off[x], (long long)off[x + 1]);
      return 1;
    }
    ++in_stripe[x];
    if (p % kXcdGranule != 0 && id != prev + 1) {
      std::printf("V=%lld p=%lld: id %lld not adjacent to %lld\n", (long long)V, (long long)p,
                  (long long)id, (long long)prev);
      return 1;
    }
    prev = id;
  }
  // Injective into [0, V) over V positions: a bijection. Each stripe's range
  // is filled exactly by the positions dealt to it.
  for (int x = 0; x < kXcdStripes; ++x) {
    if (in_stripe[x] != off[x + 1] - off[x]) {
      std::printf("V=%lld: stripe %d holds %lld of %lld\n", (long long)V, x,
                  (long long)in_stripe[x], (long long)(off[x + 1] - off[x]));
      return 1;
    }
  }
  return 0;
}

int main(int argc, char **argv) {
  int64_t checked = 0;
  for (int a = 1; a + 1 < argc; a += 2) {
    for (int64_t V = std::atoll(argv[a]); V <= std::atoll(argv[a + 1]); ++V) {
      if (check(V)) return 1;
      ++checked;
    }
  }
  std::printf("ok %lld\n", (long long)checked);
  return 0;
}
