// node_similarity.so — drop-in replacement for the topological half of the
// reference MAGE node similarity module
// (src/mage/cpp/node_similarity_module/node_similarity_module.cpp), GPU-backed.
//
// Registered signatures reproduced exactly (node_similarity_module.cpp:153-188):
//   node_similarity.jaccard()
//   node_similarity.overlap()
//   node_similarity.jaccard_pairwise(src_nodes: list<node>, dst_nodes: list<node>)
//   node_similarity.overlap_pairwise(src_nodes: list<node>, dst_nodes: list<node>)
//   each -> (node1: node, node2: node, similarity: float)
// Rows come in the reference's order: all-pairs is row-major i < j over the
// vertex scan (CalculateSimilarityCartesian, node_similarity.hpp:163-200),
// pairwise is list order (CalculateSimilarityPairwise, :126-158).
// cosine / cosine_pairwise are NOT registered: they are dot products of a
// node property vector, not graph topology (out of scope).

#include "module_common.hpp"

namespace {

using namespace mgx_module;

constexpr const char *kFieldNode1 = "node1";
constexpr const char *kFieldNode2 = "node2";
constexpr const char *kFieldSimilarity = "similarity";
constexpr const char *kArgSrcNodes = "src_nodes";
constexpr const char *kArgDstNodes = "dst_nodes";

mgp_list *ArgList(mgp_list *args, size_t i) {
  mgp_value *v = nullptr;
  Check(mgp_list_at(args, i, &v), "list_at");
  mgp_list *out = nullptr;
  Check(mgp_value_get_list(v, &out), "value_get_list");
  return out;
}

std::vector<int64_t> NodeListIds(mgp_list *nodes) {
  size_t n = 0;
  Check(mgp_list_size(nodes, &n), "list_size");
  std::vector<int64_t> ids(n);
  for (size_t i = 0; i < n; ++i) {
    mgp_value *v = nullptr;
    Check(mgp_list_at(nodes, i, &v), "list_at(nodes)");
    mgp_vertex *vert = nullptr;
    Check(mgp_value_get_vertex(v, &vert), "value_get_vertex");
    mgp_vertex_id vid{0};
    Check(mgp_vertex_get_id(vert, &vid), "vertex_get_id");
    ids[i] = vid.as_int;
  }
  return ids;
}

void AllPairs(mgp_graph *graph, mgp_result *result, mgp_memory *memory, int metric) {
  try {
    ScanResult scan = ScanGraph(graph, memory, Numbering::kVertexScanOrder);
    const int64_t V = (int64_t)scan.dense_to_mg.size();
    if (V < 2) return;
    mgx_context *ctx = Ctx();
    GraphGuard gg{ctx};
    CheckMgx(mgx_graph_from_coo(ctx, scan.src.data(), scan.dst.data(), nullptr, V,
                                (int64_t)scan.src.size(), MGX_BUILD_OUT_CSR, &gg.g),
             "mgx_graph_from_coo");
    // Past 65536 nodes the library answers MGX_ERR_TOO_LARGE before it
    // touches the buffer, which becomes the error message: size nothing.
    std::vector<double> sim;
    if (V <= 65536) sim.resize((size_t)(V * (V - 1) / 2));
    CheckMgx(mgx_similarity_all(ctx, gg.g, metric, sim.data(), nullptr), "mgx_similarity_all");
    size_t k = 0;
    for (int64_t i = 0; i < V; ++i) {
      if (mgp_must_abort(graph)) throw MgpError("query aborted");
      for (int64_t j = i + 1; j < V; ++j, ++k) {
        const double s = sim[k];
        EmitNodePairRecord(graph, result, memory, scan.dense_to_mg[i], kFieldNode1,
                           scan.dense_to_mg[j], kFieldNode2, [&](mgp_result_record *rec) {
                             InsertDouble(rec, kFieldSimilarity, s, memory);
                           });
      }
    }
  } catch (const std::exception &e) {
    (void)mgp_result_set_error_msg(result, e.what());
  }
}

void Pairwise(mgp_list *args, mgp_graph *graph, mgp_result *result, mgp_memory *memory,
              int metric) {
  try {
    const std::vector<int64_t> src_ids = NodeListIds(ArgList(args, 0));
    const std::vector<int64_t> dst_ids = NodeListIds(ArgList(args, 1));
    if (src_ids.size() != dst_ids.size()) {
      // node_similarity.hpp:129-131
      throw std::runtime_error("The node lists must be the same length.");
    }
    if (src_ids.empty()) return;
    ScanResult scan = ScanGraph(graph, memory, Numbering::kVertexScanOrder);
    const int64_t V = (int64_t)scan.dense_to_mg.size();
    std::unordered_map<int64_t, int64_t> mg_to_dense;
    mg_to_dense.reserve((size_t)V * 2);
    for (int64_t d = 0; d < V; ++d) mg_to_dense.emplace(scan.dense_to_mg[d], d);
    const size_t n = src_ids.size();
    std::vector<int64_t> u(n), v(n);
    for (size_t i = 0; i < n; ++i) {
      auto a = mg_to_dense.find(src_ids[i]);
      auto b = mg_to_dense.find(dst_ids[i]);
      if (a == mg_to_dense.end() || b == mg_to_dense.end())
        throw MgpError("node_similarity: a listed node is not in the graph");
      u[i] = a->second;
      v[i] = b->second;
    }
    mgx_context *ctx = Ctx();
    GraphGuard gg{ctx};
    CheckMgx(mgx_graph_from_coo(ctx, scan.src.data(), scan.dst.data(), nullptr, V,
                                (int64_t)scan.src.size(), MGX_BUILD_OUT_CSR, &gg.g),
             "mgx_graph_from_coo");
    std::vector<double> sim(n);
    CheckMgx(mgx_similarity_pairs(ctx, gg.g, metric, MGX_SIM_AUTO, u.data(), v.data(),
                                  (int64_t)n, sim.data(), nullptr, nullptr),
             "mgx_similarity_pairs");
    for (size_t i = 0; i < n; ++i) {
      const double s = sim[i];
      EmitNodePairRecord(graph, result, memory, src_ids[i], kFieldNode1, dst_ids[i],
                         kFieldNode2, [&](mgp_result_record *rec) {
                           InsertDouble(rec, kFieldSimilarity, s, memory);
                         });
    }
  } catch (const std::exception &e) {
    (void)mgp_result_set_error_msg(result, e.what());
  }
}

void Jaccard(mgp_list *, mgp_graph *graph, mgp_result *result, mgp_memory *memory) {
  AllPairs(graph, result, memory, MGX_SIM_JACCARD);
}
void Overlap(mgp_list *, mgp_graph *graph, mgp_result *result, mgp_memory *memory) {
  AllPairs(graph, result, memory, MGX_SIM_OVERLAP);
}
void JaccardPairwise(mgp_list *args, mgp_graph *graph, mgp_result *result,
                     mgp_memory *memory) {
  Pairwise(args, graph, result, memory, MGX_SIM_JACCARD);
}
void OverlapPairwise(mgp_list *args, mgp_graph *graph, mgp_result *result,
                     mgp_memory *memory) {
  Pairwise(args, graph, result, memory, MGX_SIM_OVERLAP);
}

}  // namespace

extern "C" int mgp_init_module(struct mgp_module *module, struct mgp_memory *) {
  try {
    mgp_type *t_float = nullptr, *t_node = nullptr, *t_list_node = nullptr;
    Check(mgp_type_float(&t_float), "type_float");
    Check(mgp_type_node(&t_node), "type_node");
    Check(mgp_type_list(t_node, &t_list_node), "type_list(node)");
    auto add = [&](const char *name, mgp_proc_cb cb, bool pairwise) {
      mgp_proc *proc = nullptr;
      Check(mgp_module_add_read_procedure(module, name, cb, &proc), "add_read_procedure");
      if (pairwise) {
        Check(mgp_proc_add_arg(proc, kArgSrcNodes, t_list_node), "arg");
        Check(mgp_proc_add_arg(proc, kArgDstNodes, t_list_node), "arg");
      }
      Check(mgp_proc_add_result(proc, kFieldNode1, t_node), "add_result");
      Check(mgp_proc_add_result(proc, kFieldNode2, t_node), "add_result");
      Check(mgp_proc_add_result(proc, kFieldSimilarity, t_float), "add_result");
    };
    // Registration order of node_similarity_module.cpp:169-173.
    add("jaccard", Jaccard, false);
    add("jaccard_pairwise", JaccardPairwise, true);
    add("overlap", Overlap, false);
    add("overlap_pairwise", OverlapPairwise, true);
  } catch (const std::exception &) {
    return 1;
  }
  return 0;
}

extern "C" int mgp_shutdown_module() { return 0; }
