// Host-only check of the offset rule of the stripe-major column stream
// (memgraph_amd/csrc/mgx_xcd_stream.h), compiled and run by
// tests/test_xcd_stream_cpu.py. For every seed on the command line ("lo hi",
// inclusive) it draws 8 stripes of segments (lo, len) in the four sections'
// length ranges, lays them out as the build does - per stripe the sections
// 3, 2, 1, 0, an exclusive sum of the allotments from the stripe's base, the
// next base rounded up - and checks that
//   - a segment of the 64- and 256-lane sections starts at an offset = lo
//     (mod 4), inside an allotment that is a multiple of 4 at a multiple of 4;
//   - a segment of the 4- and 16-lane sections fills its allotment exactly;
//   - every segment lies inside its allotment, allotments follow each other
//     without gap or overlap, so no two segments overlap;
//   - a stripe's length is the sum of its allotments, every stripe's window
//     starts at a multiple of kXcdStreamAlign ints and the padding between two
//     stripes is less than that.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../memgraph_amd/csrc/mgx_xcd_stream.h"

static uint64_t next(uint64_t &s) {  // splitmix64
  uint64_t z = (s += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

static int check(uint64_t seed) {
  uint64_t s = seed;
  const uint32_t min_len[4] = {1, 8, 64, 1024}, max_len[4] = {7, 63, 1023, 5000};
  uint64_t base = 0;
  for (int x = 0; x < kXcdStripes; ++x) {
    if (base % kXcdStreamAlign != 0) {
      std::printf("seed %llu stripe %d: base %llu\n", (unsigned long long)seed, x,
                  (unsigned long long)base);
      return 1;
    }
    uint64_t pos = base, sum = 0;
    for (int sec = 3; sec >= 0; --sec) {
      const bool aligned = mgx_xcd_seg_aligned(sec);
      if (aligned != (sec >= 2)) return 1;
      const int n = (int)(next(s) % 40);  // 0 = an empty section
      for (int i = 0; i < n; ++i) {
        const uint32_t lo = (uint32_t)(next(s) % 0xFFFF0000ull);
        const uint32_t len =
            min_len[sec] + (uint32_t)(next(s) % (max_len[sec] - min_len[sec] + 1));
        const uint32_t allot = mgx_xcd_seg_allot(lo, len, aligned);
        const uint32_t start = mgx_xcd_seg_start((uint32_t)pos, lo, aligned);
        bool ok = start >= pos && (uint64_t)start + len <= pos + allot;
        if (aligned) {
          ok = ok && start % 4 == lo % 4 && pos % 4 == 0 && allot % 4 == 0 &&
               start - pos < 4 && pos + allot - (start + len) < 4;
        } else {
          ok = ok && start == pos && allot == len;
        }
        if (!ok) {
          std::printf("seed %llu stripe %d sec %d: lo %u len %u -> pos %llu start %u allot %u\n",
                      (unsigned long long)seed, x, sec, lo, len, (unsigned long long)pos, start,
                      allot);
          return 1;
        }
        pos += allot;  // the exclusive sum: the next allotment starts here
        sum += allot;
      }
    }
    if (pos - base != sum) return 1;
    const uint64_t nb = mgx_xcd_stream_round(pos);
    if (nb < pos || nb - pos >= kXcdStreamAlign || nb % kXcdStreamAlign != 0) {
      std::printf("seed %llu stripe %d: end %llu rounds to %llu\n", (unsigned long long)seed, x,
                  (unsigned long long)pos, (unsigned long long)nb);
      return 1;
    }
    base = nb;
  }
  return 0;
}

int main(int argc, char **argv) {
  long long checked = 0;
  for (int a = 1; a + 1 < argc; a += 2) {
    for (long long seed = std::atoll(argv[a]); seed <= std::atoll(argv[a + 1]); ++seed) {
      if (check((uint64_t)seed)) return 1;
      ++checked;
    }
  }
  std::printf("ok %lld\n", checked);
  return 0;
}
