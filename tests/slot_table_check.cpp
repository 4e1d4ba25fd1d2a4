// Host-only check of the online modules' slot table and capacity rule
// (memgraph_amd/csrc/mgx_slot_table.h), compiled and run by
// tests/test_slot_table_cpu.py. For every seed on the command line ("lo hi",
// inclusive) it drives an mgx_slot_table and a naive std::map model with the
// same random sequence of create / find / kill / revive / map_dense over a
// small id range (negative ids included) and checks after every step that
//   - slot_of returns the known slot, or the next dense one with the given
//     alive flag; a slot is never reused and never changes its id;
//   - find returns -1 exactly for the ids never created;
//   - size, slot2mg and alive agree with the model;
//   - map_dense returns max(V, 1) entries; with `create` every id has a slot
//     and all_known is true; without, an id that is unknown or not alive maps
//     to -1 and clears all_known, and the table does not change.
// It also checks mgx_grown_cap on random (current, first, need): the result
// is current when need <= current, else >= need, a power-of-two multiple of
// the start (current, or first for an empty array) and the smallest such.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <vector>

#include "../memgraph_amd/csrc/mgx_slot_table.h"

static uint64_t next(uint64_t &s) {  // splitmix64
  uint64_t z = (s += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

struct Model {
  std::map<int64_t, int32_t> slot;  // id -> slot
  std::vector<int64_t> ids;         // slot -> id, in creation order
  std::vector<uint8_t> alive;
  int32_t find(int64_t mg) const {
    auto it = slot.find(mg);
    return it == slot.end() ? -1 : it->second;
  }
  int32_t slot_of(int64_t mg, uint8_t a) {
    if (find(mg) >= 0) return find(mg);
    slot[mg] = (int32_t)ids.size();
    ids.push_back(mg);
    alive.push_back(a);
    return slot[mg];
  }
};

static bool same(const mgx_slot_table &t, const Model &m) {
  if (t.size() != (int64_t)m.ids.size() || t.slot2mg != m.ids || t.alive != m.alive ||
      t.mg2slot.size() != m.slot.size())
    return false;
  for (auto &kv : m.slot)
    if (t.find(kv.first) != kv.second) return false;
  return true;
}

#define FAIL(...)                                         \
  do {                                                    \
    std::printf("seed %llu step %d: ", (unsigned long long)seed, step); \
    std::printf(__VA_ARGS__);                             \
    std::printf("\n");                                    \
    return 1;                                             \
  } while (0)

static int check_table(uint64_t seed) {
  uint64_t s = seed;
  mgx_slot_table t;
  Model m;
  const int64_t range = 4 + (int64_t)(next(s) % 40);  // ids in [-range/2, range/2)
  auto draw_id = [&]() { return (int64_t)(next(s) % (uint64_t)range) - range / 2; };
  const int steps = 20 + (int)(next(s) % 60);
  for (int step = 0; step < steps; ++step) {
    const int op = (int)(next(s) % 5);
    if (op == 0) {  // create
      const int64_t id = draw_id();
      const uint8_t a = (uint8_t)(next(s) & 1);
      const int32_t want = m.slot_of(id, a);
      if (t.slot_of(id, a) != want) FAIL("slot_of(%lld) != %d", (long long)id, want);
    } else if (op == 1) {  // find
      const int64_t id = draw_id();
      if (t.find(id) != m.find(id)) FAIL("find(%lld) != %d", (long long)id, m.find(id));
    } else if (op == 2 || op == 3) {  // kill / revive
      const int64_t id = draw_id();
      const int32_t sl = t.find(id);
      if (sl != m.find(id)) FAIL("find(%lld) != %d", (long long)id, m.find(id));
      if (sl >= 0) t.alive[sl] = m.alive[sl] = (uint8_t)(op == 3);
    } else {  // map_dense over V ids, repeats allowed, V = 0 included
      const int64_t V = (int64_t)(next(s) % 12);
      const bool create = (next(s) & 1) != 0;
      const uint8_t a = (uint8_t)(next(s) & 1);
      std::vector<int64_t> ids(V);
      for (auto &id : ids) id = draw_id();
      std::vector<int32_t> want(V > 0 ? V : 1, -1);
      bool want_known = true;
      for (int64_t v = 0; v < V; ++v) {
        if (create) {
          want[v] = m.slot_of(ids[v], a);
        } else {
          const int32_t sl = m.find(ids[v]);
          want[v] = sl >= 0 && m.alive[sl] ? sl : -1;
          if (want[v] < 0) want_known = false;
        }
      }
      std::vector<int32_t> got(3, 7);  // stale contents must not survive
      bool known = !want_known;
      t.map_dense(ids.data(), V, create, &got, &known, a);
      if (got != want) FAIL("map_dense(V=%lld, create=%d): wrong d2s", (long long)V, create);
      if (known != want_known) FAIL("map_dense(V=%lld, create=%d): all_known", (long long)V, create);
      t.map_dense(ids.data(), V, /*create=*/false, &got, nullptr);  // a null all_known is allowed
    }
    if (!same(t, m)) FAIL("table and model differ");
  }
  return 0;
}

static int check_grown_cap(uint64_t seed) {
  uint64_t s = seed;
  const int step = -1;
  for (int i = 0; i < 50; ++i) {
    const int64_t first = 1 + (int64_t)(next(s) % 5000);
    int64_t current = 0;
    if (next(s) & 1) current = first << (next(s) % 12);
    const int64_t need = (int64_t)(next(s) % (uint64_t)(4 * (current > 0 ? current : first) + 2)) -
                         (int64_t)(next(s) % 2);  // -1 .. about 4x
    const int64_t got = mgx_grown_cap(current, first, need);
    if (need <= current) {
      if (got != current) FAIL("grown_cap(%lld, %lld, %lld) = %lld", (long long)current,
                               (long long)first, (long long)need, (long long)got);
      continue;
    }
    const int64_t start = current > 0 ? current : first;
    int64_t q = got / start;
    const bool multiple = got % start == 0 && q >= 1 && (q & (q - 1)) == 0;
    const bool smallest = got == start || got / 2 < need;
    if (got < need || !multiple || !smallest)
      FAIL("grown_cap(%lld, %lld, %lld) = %lld", (long long)current, (long long)first,
           (long long)need, (long long)got);
  }
  return 0;
}

int main(int argc, char **argv) {
  long long checked = 0;
  for (int a = 1; a + 1 < argc; a += 2) {
    for (long long seed = std::atoll(argv[a]); seed <= std::atoll(argv[a + 1]); ++seed) {
      if (check_table((uint64_t)seed) || check_grown_cap((uint64_t)seed)) return 1;
      ++checked;
    }
  }
  std::printf("ok %lld\n", checked);
  return 0;
}
