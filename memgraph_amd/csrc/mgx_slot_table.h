// Host side of the online modules' persistent state: the slot table that keeps
// a vertex's identity across graph changes, and the capacity rule of their
// grow-only device arrays (mgx_online.h). Plain C++17, no HIP: the CPU check
// tests/slot_table_check.cpp includes this file alone.
#ifndef MGX_SLOT_TABLE_H
#define MGX_SLOT_TABLE_H

#include <cstdint>
#include <unordered_map>
#include <vector>

// memgraph id <-> slot. Slots are dense, handed out in order of first sight and
// never reused; `alive` says whether the slot's vertex is part of the state now.
struct mgx_slot_table {
  std::unordered_map<int64_t, int32_t> mg2slot;
  std::vector<int64_t> slot2mg;
  std::vector<uint8_t> alive;

  int64_t size() const { return (int64_t)slot2mg.size(); }

  int32_t find(int64_t mg) const {  // -1 when absent
    auto it = mg2slot.find(mg);
    return it == mg2slot.end() ? -1 : it->second;
  }

  // Slot of mg, created with alive = alive_init when absent.
  int32_t slot_of(int64_t mg, uint8_t alive_init) {
    const int32_t known = find(mg);
    if (known >= 0) return known;
    const int32_t s = (int32_t)slot2mg.size();
    mg2slot.emplace(mg, s);
    slot2mg.push_back(mg);
    alive.push_back(alive_init);
    return s;
  }

  // d2s[v] = slot of dense vertex v, max(V, 1) entries. With `create` every id
  // gets a slot (new ones with alive = alive_init); without, an id that is
  // unknown or not alive maps to -1 and clears *all_known (nullable).
  void map_dense(const int64_t *dense_to_mg, int64_t V, bool create, std::vector<int32_t> *d2s,
                 bool *all_known, uint8_t alive_init = 0) {
    d2s->assign(V > 0 ? V : 1, -1);
    bool known = true;
    for (int64_t v = 0; v < V; ++v) {
      int32_t s = create ? slot_of(dense_to_mg[v], alive_init) : find(dense_to_mg[v]);
      if (s >= 0 && !create && !alive[s]) s = -1;
      if (s < 0) known = false;
      (*d2s)[v] = s;
    }
    if (all_known) *all_known = known;
  }
};

// Capacity of a grow-only array that holds `current` elements' room and must
// hold `need`: unchanged when it already does, else `current` (or `first` for
// an array that has no block yet) doubled until it does.
inline int64_t mgx_grown_cap(int64_t current, int64_t first, int64_t need) {
  if (need <= current) return current;
  int64_t cap = current > 0 ? current : (first > 0 ? first : 1);
  while (cap < need) cap *= 2;
  return cap;
}

#endif  // MGX_SLOT_TABLE_H
