// bridges.so — drop-in replacement for the reference bridges module
// (src/mage/cpp/bridges_module/bridges_module.cpp), GPU-backed.
//
// Registered signature reproduced exactly (bridges_module.cpp:62-66):
//   bridges.get() -> (node_from: node, node_to: node)
// The row set and each row's orientation (the bridge edge's own from/to,
// bridges_module.cpp:39-50) match the reference. Row ORDER is edge scan order
// here; the reference's is DFS post-order, which depends on its traversal
// order, and its e2e tests ORDER BY (parity traps).

#include <algorithm>

#include "module_common.hpp"

namespace {

using namespace mgx_module;

constexpr const char *kProcedureGet = "get";
constexpr const char *kFieldNodeFrom = "node_from";
constexpr const char *kFieldNodeTo = "node_to";

void GetBridges(mgp_list * /*args*/, mgp_graph *graph, mgp_result *result, mgp_memory *memory) {
  try {
    ScanResult scan = ScanGraph(graph, memory, Numbering::kVertexScanOrder);
    const int64_t V = (int64_t)scan.dense_to_mg.size();
    if (V == 0) return;

    mgx_context *ctx = Ctx();
    GraphGuard gg{ctx};
    CheckMgx(mgx_graph_from_coo(ctx, scan.src.data(), scan.dst.data(), nullptr, V,
                                (int64_t)scan.src.size(), MGX_BUILD_SYM_CSR, &gg.g),
             "mgx_graph_from_coo");
    std::vector<int64_t> bu(V), bv(V);
    int64_t n_bridges = 0;
    CheckMgx(mgx_bridges(ctx, gg.g, bu.data(), bv.data(), &n_bridges, nullptr), "mgx_bridges");
    if (n_bridges == 0) return;

    // The library's pairs are (min, max) sorted by pair. A bridge pair has
    // multiplicity 1, so exactly one scanned edge carries it: emit that edge,
    // in scan order, in its own direction.
    std::vector<uint64_t> keys((size_t)n_bridges);
    for (int64_t i = 0; i < n_bridges; ++i) keys[i] = ((uint64_t)bu[i] << 32) | (uint64_t)bv[i];
    for (size_t e = 0; e < scan.src.size(); ++e) {
      const int64_t a = std::min(scan.src[e], scan.dst[e]);
      const int64_t b = std::max(scan.src[e], scan.dst[e]);
      if (!std::binary_search(keys.begin(), keys.end(), ((uint64_t)a << 32) | (uint64_t)b))
        continue;
      EmitNodePairRecord(graph, result, memory, scan.dense_to_mg[scan.src[e]], kFieldNodeFrom,
                         scan.dense_to_mg[scan.dst[e]], kFieldNodeTo,
                         [](mgp_result_record *) {});
    }
  } catch (const std::exception &e) {
    (void)mgp_result_set_error_msg(result, e.what());
    return;
  }
}

}  // namespace

extern "C" int mgp_init_module(struct mgp_module *module, struct mgp_memory * /*memory*/) {
  try {
    mgp_proc *proc = nullptr;
    Check(mgp_module_add_read_procedure(module, kProcedureGet, GetBridges, &proc),
          "add_read_procedure");
    mgp_type *t_node = nullptr;
    Check(mgp_type_node(&t_node), "type_node");
    Check(mgp_proc_add_result(proc, kFieldNodeFrom, t_node), "add_result");
    Check(mgp_proc_add_result(proc, kFieldNodeTo, t_node), "add_result");
  } catch (const std::exception &) {
    return 1;
  }
  return 0;
}

extern "C" int mgp_shutdown_module() { return 0; }
