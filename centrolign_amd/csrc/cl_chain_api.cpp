// cl_chain_api.cpp — host side of the chaining seams (include/centrolign_amd.h): cl_chain_sparse_affine / cl_chain_sparse
// (the Anchorer's chaining DPs, include/centrolign/anchorer.hpp:1511-2547, with the DP itself on the GPU,
// chain_kernels.hip) and cl_anchor_chain (Anchorer::anchor_chain, :958-1329, with fill-in re-anchoring :619-956).
//
// chain_dp_batch — K independent chaining instances in one device pass — lives in chain_dp.hpp (cl_chain_prep.cpp: the host preparation, cl_chain_device.cpp: the
// driver and the device phases, cl_chain_traceback.cpp: the optimum and the backpointers); this file holds the C entry points, cl_anchor_chain, match
// selection, fill-in and the masks.
#include <algorithm>
#include <array>
#include <chrono>
#include <condition_variable>
#include <mutex>
#include <unistd.h>
#include <functional>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <numeric>
#include <unordered_map>
#include <vector>

#include "chain_dp.hpp"

using namespace clchain;

extern "C" {

void cl_chain_params_default(cl_chain_params* p) {
    // src/parameters.cpp:39-59
    const double go[3] = {1.25, 50.0, 5000.0}, ge[3] = {2.5, 0.1, 0.0015};
    for (int i = 0; i < 3; ++i) { p->gap_open[i] = go[i]; p->gap_extend[i] = ge[i]; }
    p->anchor_score_function = 2;
    p->pair_count_power = 0.5;
    p->length_intercept = 2250.0;
    p->length_decay_power = 2.0;
    p->global_anchoring = 1;   // src/parameters.cpp:60
}

void cl_chain_result_free(cl_chain_result* r) {
    if (!r) return;
    free(r->anchors);
    free(r->dp);
    memset(r, 0, sizeof(*r));
}

}  // extern "C"

// one instance on the two merge graphs (with their sentinels); global anchoring = chains start at the nodes after the
// source sentinel and end at the nodes before the sink sentinel (anchorer.hpp:1069-1076)
static ChainSub whole_graph_instance(const cl_base_graph* g1, const cl_base_graph* g2, const cl_match_sets* ms, uint64_t num_match_sets,
                                     bool global_anchoring) {
    ChainSub sb;
    sb.g[0] = g1; sb.g[1] = g2;
    sb.ms = ms;
    sb.num_match_sets = num_match_sets;
    sb.anchored = global_anchoring;
    if (global_anchoring)
        for (int side = 0; side < 2; ++side) {
            const cl_base_graph* g = sb.g[side];
            sb.src[side].assign(g->next_idx + g->next_off[g->src_id], g->next_idx + g->next_off[g->src_id + 1]);
            sb.snk[side].assign(g->prev_idx + g->prev_off[g->snk_id], g->prev_idx + g->prev_off[g->snk_id + 1]);
        }
    return sb;
}

static int chain_dp_impl(cl_context* ctx, const cl_base_graph* g1, const cl_base_graph* g2, const cl_match_sets* ms,
                         uint64_t num_match_sets, const cl_chain_params* cp, double local_scale, int want_dp, bool sparse,
                         cl_chain_result* out) {
    if (!ctx || !g1 || !g2 || !ms || !cp || !out) { cl_set_error(ctx, "null argument"); return CL_ERR_INVALID_ARGUMENT; }
    memset(out, 0, sizeof(*out));
    if (num_match_sets > ms->n_sets) { cl_set_error(ctx, "num_match_sets exceeds the number of sets"); return CL_ERR_INVALID_ARGUMENT; }
    std::vector<ChainSub> subs(1, whole_graph_instance(g1, g2, ms, num_match_sets, cp->global_anchoring != 0));
    std::vector<ChainSubResult> res;
    ChainTimings tm;
    std::vector<float> dp;
    const int rc = chain_dp_batch(ctx, subs, cp, local_scale, sparse, res, tm, want_dp ? &dp : nullptr);
    if (rc) return rc;
    out->n_pairs = tm.n_pairs;
    out->device_ms = tm.device_ms; out->prep_ms = tm.prep_ms; out->index_ms = tm.index_ms; out->traceback_ms = tm.traceback_ms;
    const ChainSubResult& r = res[0];
    const size_t na = r.chain.size() / 3;
    out->n_anchors = na;
    out->n_ties = r.n_ties;
    out->anchors = (uint32_t*)malloc((na ? na : 1) * 3 * sizeof(uint32_t));
    if (want_dp) out->dp = (float*)malloc((dp.size() ? dp.size() : 1) * sizeof(float));
    if (!out->anchors || (want_dp && !out->dp)) { cl_chain_result_free(out); return CL_ERR_OUT_OF_MEMORY; }
    if (na) memcpy(out->anchors, r.chain.data(), r.chain.size() * sizeof(uint32_t));
    if (want_dp && !dp.empty()) memcpy(out->dp, dp.data(), dp.size() * sizeof(float));
    if (!sparse && subs[0].anchored && na) {
        out->gap_before_first = r.gap[0]; out->gap_score_before_first = r.gap_score[0];
        out->gap_after_last = r.gap[na]; out->gap_score_after_last = r.gap_score[na];
    }
    return CL_OK;
}

extern "C" {

int cl_chain_sparse_affine(cl_context* ctx, const cl_base_graph* g1, const cl_base_graph* g2, const cl_match_sets* ms,
                           uint64_t num_match_sets, const cl_chain_params* cp, double local_scale, int want_dp,
                           cl_chain_result* out) {
    cl_bind_device(ctx);
    return chain_dp_impl(ctx, g1, g2, ms, num_match_sets, cp, local_scale, want_dp, false, out);
}

int cl_chain_sparse(cl_context* ctx, const cl_base_graph* g1, const cl_base_graph* g2, const cl_match_sets* ms,
                    uint64_t num_match_sets, const cl_chain_params* cp, int want_dp, cl_chain_result* out) {
    cl_bind_device(ctx);
    return chain_dp_impl(ctx, g1, g2, ms, num_match_sets, cp, 1.0, want_dp, true, out);
}

}  // extern "C"

// exhaustive_chain_dp with score_edges == false (anchorer.hpp:1342-1509 as dispatched at :1229-1232) and
// AnchorGraph::heaviest_weight_path (src/anchorer.cpp:68-133).  The reference materialises every edge; here an edge is the
// reachability test itself, evaluated twice per ordered pair (once for the in-degrees of Kahn's algorithm, once when the
// source node is popped), so a few tens of thousands of match pairs stay within memory.  Node order, edge order (ascending
// target id), the LIFO stack of topological_order.hpp:12-60 and the strict '>' updates decide ties exactly as there.
extern "C" int cl_chain_exhaustive(cl_context* ctx, const cl_base_graph* g1, const cl_base_graph* g2, const cl_match_sets* ms,
                                   uint64_t num_match_sets, const cl_chain_params* cp, cl_chain_result* out) {
    if (!g1 || !g2 || !ms || !cp || !out) { cl_set_error(ctx, "null argument"); return CL_ERR_INVALID_ARGUMENT; }
    memset(out, 0, sizeof(*out));
    if (num_match_sets > ms->n_sets) { cl_set_error(ctx, "num_match_sets exceeds the number of sets"); return CL_ERR_INVALID_ARGUMENT; }
    clhost::PathMergeTable x1, x2;
    if (!x1.build(*g1) || !x2.build(*g2)) { cl_set_error(ctx, "graph is not acyclic"); return CL_ERR_CYCLIC_GRAPH; }
    const ChainSub sb = whole_graph_instance(g1, g2, ms, num_match_sets, cp->global_anchoring != 0);
    const double lowest = std::numeric_limits<double>::lowest();
    struct Node { uint32_t set, i1, i2, b1, e1, b2, e2; double weight, initial, final_w; };
    std::vector<Node> nodes;
    for (uint64_t s = 0; s < num_match_sets; ++s) {
        const uint64_t a0 = ms->set_off1[s], a1 = ms->set_off1[s + 1], c0 = ms->set_off2[s], c1 = ms->set_off2[s + 1];
        if (a0 == a1) continue;
        const double w = anchor_weight(*cp, ms->count1[s], ms->count2[s], ms->walk_off1[a0 + 1] - ms->walk_off1[a0], ms->full_length[s]);
        for (uint64_t j = a0; j < a1; ++j)
            for (uint64_t q = c0; q < c1; ++q) {
                Node nd{(uint32_t)s, (uint32_t)(j - a0), (uint32_t)(q - c0), ms->nodes1[ms->walk_off1[j]], ms->nodes1[ms->walk_off1[j + 1] - 1],
                        ms->nodes2[ms->walk_off2[q]], ms->nodes2[ms->walk_off2[q + 1] - 1], w, 0.0, 0.0};
                if (sb.anchored) {
                    nd.initial = lowest;
                    for (uint32_t a : sb.src[0]) for (uint32_t b : sb.src[1])
                        if ((a == nd.b1 || x1.reachable(a, nd.b1)) && (b == nd.b2 || x2.reachable(b, nd.b2))) nd.initial = 0.0;
                    nd.final_w = lowest;
                    for (uint32_t a : sb.snk[0]) for (uint32_t b : sb.snk[1])
                        if ((a == nd.e1 || x1.reachable(nd.e1, a)) && (b == nd.e2 || x2.reachable(nd.e2, b))) nd.final_w = 0.0;
                }
                nodes.push_back(nd);
            }
    }
    const size_t N = nodes.size();
    out->n_pairs = N;
    auto edge = [&](size_t i, size_t j) { return x1.reachable(nodes[i].e1, nodes[j].b1) && x2.reachable(nodes[i].e2, nodes[j].b2); };
    std::vector<uint32_t> indeg(N, 0);
    cl_parallel_for(N, [&](uint64_t jb, uint64_t je) {
        for (size_t j = jb; j < je; ++j) {
            uint32_t d = 0;
            for (size_t i = 0; i < N; ++i) d += edge(i, j) ? 1u : 0u;
            indeg[j] = d;
        }
    }, 64);
    std::vector<double> dp(N);
    std::vector<size_t> back(N, SIZE_MAX), stack;
    for (size_t i = 0; i < N; ++i) { dp[i] = nodes[i].initial; if (!indeg[i]) stack.push_back(i); }
    size_t max_id = SIZE_MAX, seen = 0;
    double max_weight = 0.0;   // min_score: edges are not scored
    while (!stack.empty()) {
        const size_t v = stack.back();
        stack.pop_back();
        ++seen;
        const bool live = dp[v] != lowest;
        if (live) {
            dp[v] += nodes[v].weight;
            if (nodes[v].final_w != lowest && dp[v] + nodes[v].final_w > max_weight) { max_id = v; max_weight = dp[v] + nodes[v].final_w; }
        }
        for (size_t j = 0; j < N; ++j) {
            if (!edge(v, j)) continue;
            if (live && dp[v] + 0.0 > dp[j]) { dp[j] = dp[v] + 0.0; back[j] = v; }
            if (--indeg[j] == 0) stack.push_back(j);
        }
    }
    if (seen != N) { cl_set_error(ctx, "anchor graph is not acyclic"); return CL_ERR_CYCLIC_GRAPH; }
    std::vector<size_t> path;
    for (size_t v = max_id; v != SIZE_MAX; v = back[v]) path.push_back(v);
    std::reverse(path.begin(), path.end());
    out->n_anchors = path.size();
    out->anchors = (uint32_t*)malloc((path.empty() ? 1 : path.size()) * 3 * sizeof(uint32_t));
    if (!out->anchors) return CL_ERR_OUT_OF_MEMORY;
    for (size_t i = 0; i < path.size(); ++i) {
        out->anchors[3 * i] = nodes[path[i]].set;
        out->anchors[3 * i + 1] = nodes[path[i]].i1;
        out->anchors[3 * i + 2] = nodes[path[i]].i2;
    }
    return CL_OK;
}

// =====================================================================================================================
// Anchorer::anchor_chain without fill-in re-anchoring and branch splitting:
//   budgeted greedy match selection + reorder      include/centrolign/anchorer.hpp:1108-1173
//   graph swap to save memory                       :1175-1192, 1309-1322
//   estimate_score_scale                            :998-1047  (sparse_chain_dp + extract_graphs_between + source_sink_minmax)
//   sparse_affine_chain_dp with the estimated scale :985, 1050-1089
//   gap / score annotation of the chain             :2443-2468, 1331-1339
// =====================================================================================================================
namespace {

struct OwnedMatchSets {
    std::vector<uint64_t> set_off1{0}, walk_off1{0}, set_off2{0}, walk_off2{0}, count1, count2, full_length;
    std::vector<uint32_t> nodes1, nodes2;
    cl_match_sets view() const {
        return cl_match_sets{count1.size(), set_off1.data(), walk_off1.data(), nodes1.data(), set_off2.data(), walk_off2.data(),
                             nodes2.data(), count1.data(), count2.data(), full_length.data()};
    }
};

// anchorer.hpp:1108-1173 on a permutation of the original set indices: `cur` is the current order of the caller's
// vector; returns the number of leading sets that take part
uint64_t select_matches(const cl_match_sets& ms, const cl_chain_params& cp, std::vector<uint64_t>& cur, uint64_t local_max) {
    const size_t n = cur.size();
    auto n_pairs = [&](uint64_t s) { return (ms.set_off1[s + 1] - ms.set_off1[s]) * (ms.set_off2[s + 1] - ms.set_off2[s]); };
    uint64_t total = 0;
    for (uint64_t s : cur) total += n_pairs(s);
    if (total <= local_max) return n;
    // the sort key and the weight at the set's own length, evaluated once per set (two pow() each) on the pool's threads: 150 000 - 310 000 sets per merge of 10 x 1 Mbp
    std::vector<double> wfull(n), wlen(n);
    std::atomic<bool> plain{true};   // no NaN among the keys (anchor weights of counts >= 1 never are): the radix order below is then the comparison sort's
    cl_parallel_for(n, [&](uint64_t b, uint64_t e) {
        bool ok = true;
        for (uint64_t i = b; i < e; ++i) {
            const uint64_t s = cur[i];
            wfull[i] = anchor_weight(cp, ms.count1[s], ms.count2[s], ms.full_length[s], ms.full_length[s]);
            const uint64_t w0 = ms.set_off1[s];
            const uint64_t len = ms.walk_off1[w0 + 1] - ms.walk_off1[w0];
            wlen[i] = anchor_weight(cp, ms.count1[s], ms.count2[s], len, len);
            ok = ok && wfull[i] == wfull[i];
        }
        if (!ok) plain = false;
    }, 8192);
    std::vector<uint32_t> order(n);
    std::iota(order.begin(), order.end(), 0u);
    if (plain && n >= 4096 && n < (1ull << 32)) {
        // std::stable_sort(order, wfull[i] > wfull[j]) as a stable LSD radix sort on the order-preserving integer image of the doubles (descending; -0.0 == +0.0
        // as the comparison has it): four passes of 16 bits over the indices instead of n log n comparisons through two indirections
        std::vector<uint64_t> key(n);
        for (size_t i = 0; i < n; ++i) {
            double w = wfull[i];
            if (w == 0.0) w = 0.0;   // -0.0 -> +0.0
            uint64_t b;
            memcpy(&b, &w, 8);
            b = (b >> 63) ? ~b : b | 0x8000000000000000ull;   // ascending in the double's order ...
            key[i] = ~b;                                        // ... descending
        }
        std::vector<uint32_t> tmp(n);
        std::vector<uint32_t> cnt(65536 + 1);
        for (int pass = 0; pass < 4; ++pass) {
            const int sh = 16 * pass;
            std::fill(cnt.begin(), cnt.end(), 0u);
            for (size_t i = 0; i < n; ++i) ++cnt[((key[i] >> sh) & 0xFFFF) + 1];
            if (cnt[((key[0] >> sh) & 0xFFFF) + 1] == n) continue;   // every key has this digit
            for (size_t d = 0; d < 65536; ++d) cnt[d + 1] += cnt[d];
            for (size_t k = 0; k < n; ++k) { const uint32_t i = order[k]; tmp[cnt[(key[i] >> sh) & 0xFFFF]++] = i; }
            order.swap(tmp);
        }
    } else {
        std::stable_sort(order.begin(), order.end(), [&](uint32_t i, uint32_t j) { return wfull[i] > wfull[j]; });
    }
    size_t removed = 0;
    uint64_t left = local_max;
    for (size_t i = 0; i < order.size(); ++i) {
        const uint64_t s = cur[order[i]];
        if (wlen[order[i]] < 0.0) { removed += order.size() - i; break; }
        const uint64_t pc = n_pairs(s);
        if (left >= pc) { left -= pc; std::swap(order[i - removed], order[i]); }
        else ++removed;
    }
    std::vector<uint64_t> next(n);
    for (size_t k = 0; k < n; ++k) next[k] = cur[order[k]];  // reorder(matches, invert(order)): new[k] = old[order[k]]
    cur.swap(next);
    return n - removed;
}

// anchor_t on the host (include/centrolign/anchorer.hpp:36-57), walks in parent-graph ids
struct HAnchor {
    std::vector<uint32_t> w1, w2;
    uint64_t count1 = 0, count2 = 0, full_length = 0, match_set = 0, idx1 = 0, idx2 = 0;
    double score = 0.0, gsb = 0.0, gsa = 0.0;
    int64_t gb = 0, ga = 0;
};

// node -> ids of the paths through it, ascending (StepIndex, include/centrolign/step_index.hpp:38-46)
struct PathsOfNode {
    std::vector<uint64_t> off;
    std::vector<uint32_t> path;
    void build(const cl_base_graph& g) {
        off.assign(g.n_nodes + 1, 0);
        for (uint64_t i = 0; i < g.path_off[g.n_paths]; ++i) ++off[g.path_nodes[i] + 1];
        for (uint64_t v = 0; v < g.n_nodes; ++v) off[v + 1] += off[v];
        path.resize(off[g.n_nodes]);
        std::vector<uint64_t> fill(off.begin(), off.end() - 1);
        for (uint64_t p = 0; p < g.n_paths; ++p)
            for (uint64_t i = g.path_off[p]; i < g.path_off[p + 1]; ++i) path[fill[g.path_nodes[i]]++] = (uint32_t)p;
    }
};

// one side of one fill-in subproblem: the extracted subgraph with the parent's paths projected onto it
// (Extractor::project_paths / do_project, anchorer.hpp:586-615)
struct FillSide {
    std::vector<uint64_t> path_off{0};
    std::vector<uint32_t> path_nodes, tag;
    cl_base_graph view;
    void project(const clhost::OwnedBatch::Side& sd, uint64_t k, const PathsOfNode& steps, uint32_t tag_base) {
        const uint64_t b = sd.node_off[k], n = sd.node_off[k + 1] - b;
        view = cl_base_graph{n, sd.label.data() + b, sd.next_off.data() + b, sd.next_idx.data(), sd.prev_off.data() + b, sd.prev_idx.data(),
                             0, nullptr, nullptr, UINT64_MAX, UINT64_MAX};
        std::vector<uint32_t> order;
        clhost::topological_order(view, order);
        std::vector<std::vector<uint32_t>> paths;
        std::unordered_map<uint32_t, uint32_t> local_of;   // parent path -> projected path, numbered by first encounter
        for (uint32_t v : order) {
            const uint64_t parent = sd.back[b + v];
            for (uint64_t i = steps.off[parent]; i < steps.off[parent + 1]; ++i) {
                auto it = local_of.find(steps.path[i]);
                if (it == local_of.end()) {
                    it = local_of.emplace(steps.path[i], (uint32_t)paths.size()).first;
                    paths.emplace_back();
                    tag.push_back(tag_base + steps.path[i]);
                }
                paths[it->second].push_back(v);
            }
        }
        for (auto& pth : paths) {
            path_nodes.insert(path_nodes.end(), pth.begin(), pth.end());
            path_off.push_back(path_nodes.size());
        }
        view.n_paths = paths.size();
        view.path_off = path_off.data();
        view.path_nodes = path_nodes.data();
    }
};

}  // namespace

extern "C" {

void cl_anchor_chain_result_free(cl_anchor_chain_result* r) {
    if (!r) return;
    free(r->anchors); free(r->gap_before); free(r->gap_after); free(r->gap_score_before); free(r->gap_score_after);
    free(r->score); free(r->set_order); free(r->walk_off); free(r->walk1); free(r->walk2); free(r->count1); free(r->count2);
    free(r->full_length);
    memset(r, 0, sizeof(*r));
}

}  // extern "C"

// scale_only: stop after estimate_score_scale (out->scale is the only field set)
// masked matches: sorted (set, idx1, idx2) triples in the indexing of the caller's sets (anchorer.hpp:144)
struct MaskSet {
    std::vector<std::array<uint64_t, 3>> v;
    bool has(uint64_t s, uint64_t a, uint64_t b) const { return std::binary_search(v.begin(), v.end(), std::array<uint64_t, 3>{s, a, b}); }
};

static int anchor_chain_impl(cl_context* ctx, const cl_base_graph* g1, const cl_base_graph* g2, const cl_match_sets* ms,
                             const cl_anchor_params* ap, cl_anchor_chain_result* out, bool scale_only, const MaskSet* mask = nullptr,
                             const double* override_scale = nullptr, bool keep_scale_chain = false) {
    if (!ctx || !g1 || !g2 || !ms || !ap || !out) { cl_set_error(ctx, "null argument"); return CL_ERR_INVALID_ARGUMENT; }
    memset(out, 0, sizeof(*out));
    if (ctx->poisoned) { cl_set_error(ctx, "this context was given up after a merge-group wait expired: destroy it and make a new one"); return CL_ERR_HIP; }
    const cl_chain_params& cp = ap->chain;
    // the CLI's -g (Anchorer::chaining_algorithm): Sparse chains on ChainMerge tables, without a scale estimate (anchorer.hpp:975-984, core.hpp:350-357)
    const int algo = ap->chaining_algorithm_plus_one ? ap->chaining_algorithm_plus_one - 1 : 2;
    if (algo != 1 && algo != 2) { cl_set_error(ctx, "chaining algorithm %d is not offered by cl_anchor_chain (1 = Sparse, 2 = SparseAffine; Exhaustive: cl_chain_exhaustive)", algo); return CL_ERR_INVALID_ARGUMENT; }
    const bool sparse_algo = algo == 1;
    clhost::PathMergeTable own_x1, own_x2;
    const clhost::PathMergeTable* const sx1 = cl_shared_table(g1), * const sx2 = cl_shared_table(g2);   // cl_core_align's, when it is the caller
    if ((!sx1 && !(sparse_algo ? own_x1.build_chain_merge(*g1) : own_x1.build(*g1))) || (!sx2 && !(sparse_algo ? own_x2.build_chain_merge(*g2) : own_x2.build(*g2)))) {
        cl_set_error(ctx, "graph is not acyclic");
        return CL_ERR_CYCLIC_GRAPH;
    }
    const clhost::PathMergeTable& x1 = sx1 ? *sx1 : own_x1;
    const clhost::PathMergeTable& x2 = sx2 ? *sx2 : own_x2;
    // anchorer.hpp:1175: the DP runs with the graphs swapped when that makes its tables smaller
    const bool swap = g1->n_nodes * x1.chain_size() > g2->n_nodes * x2.chain_size();
    // CL_CHAIN_TIMING=1: host phase times on stderr
    const bool timing = getenv("CL_CHAIN_TIMING") != nullptr;
    auto now = [] { return std::chrono::steady_clock::now(); };
    auto lap = [&](const char* what, std::chrono::steady_clock::time_point& t) {
        if (timing) fprintf(stderr, "[cl_anchor_chain] %-28s %8.1f ms\n", what, std::chrono::duration<double, std::milli>(now() - t).count());
        t = now();
    };
    auto t_pre = now();
    PostSwitchTable sw1, sw2;
    PathsOfNode steps1, steps2;
    GraphOrder order_dp1;   // of the graph that plays graph 1 in the DPs
    const bool small_graphs = (g1->n_nodes + 1) * (g1->n_paths + 1) + (g2->n_nodes + 1) * (g2->n_paths + 1) < (1u << 18);
    cl_pool_run(small_graphs ? 1 : 5, [&](unsigned t0) {
      for (unsigned t = t0; t < 5; t += small_graphs ? 1 : 5) {
        if (t == 0) sw1.build(*g1, x1);
        else if (t == 1) sw2.build(*g2, x2);
        else if (t == 4) order_dp1.build(swap ? *g2 : *g1);
        else if (!ap->do_fill_in_anchoring) continue;
        else if (t == 2) steps1.build(*g1);
        else steps2.build(*g2);
      }
    });
    lap("post-switch tables, paths of nodes", t_pre);
    std::vector<uint64_t> cur(ms->n_sets);
    std::iota(cur.begin(), cur.end(), (uint64_t)0);

    // walks of (position in `cur`, idx) on the caller's sets
    auto walk = [&](int side, uint64_t set_pos, uint32_t idx, const uint32_t*& b, const uint32_t*& e) {
        const uint64_t s = cur[set_pos];
        const uint64_t w = (side ? ms->set_off2 : ms->set_off1)[s] + idx;
        const uint64_t* wo = side ? ms->walk_off2 : ms->walk_off1;
        const uint32_t* nd = side ? ms->nodes2 : ms->nodes1;
        b = nd + wo[w]; e = nd + wo[w + 1];
    };

    // ---- fill_in_anchor_chain (anchorer.hpp:619-699): re-anchor inside every gap of the chain with the matches that lie
    //      wholly inside it; all the gaps' DPs run as one batched device pass
    auto fill_in = [&](std::vector<HAnchor>& anchors, bool sparse, double anchor_scale) -> int {
        if (anchors.empty()) return CL_OK;
        auto t = now();
        std::vector<uint64_t> seg_off{0, anchors.size()}, walk_off{0};
        std::vector<uint32_t> w1, w2;
        for (const HAnchor& a : anchors) {
            w1.insert(w1.end(), a.w1.begin(), a.w1.end());
            w2.insert(w2.end(), a.w2.begin(), a.w2.end());
            walk_off.push_back(w1.size());
        }
        cl_anchor_segments sg{1, seg_off.data(), walk_off.data(), w1.data(), w2.data()};
        clhost::OwnedBatch ob;
        int rc = clhost::extract_stitch_batch(*g1, *g2, sg, ob, &x1, &x2);
        if (rc) { cl_set_error(ctx, "extraction failed"); return rc; }
        lap("fill-in: extraction", t);
        const size_t K = ob.only_del.size();
        // divvy_matches (anchorer.hpp:701-798): a walk goes to the gap that holds both its ends
        const uint32_t none = 0xFFFFFFFFu;
        std::vector<std::pair<uint32_t, uint32_t>> ft[2];
        for (int side = 0; side < 2; ++side) {
            ft[side].assign((side ? g2 : g1)->n_nodes, std::make_pair(none, none));
            const auto& sd = ob.side[side];
            for (size_t k = 0; k < K; ++k)
                for (uint64_t v = sd.node_off[k]; v < sd.node_off[k + 1]; ++v) ft[side][sd.back[v]] = std::make_pair((uint32_t)k, (uint32_t)(v - sd.node_off[k]));
        }
        struct Divvied {
            OwnedMatchSets sets;
            std::vector<uint64_t> origin_set;
            std::vector<std::vector<uint32_t>> origin_idx1, origin_idx2;
        };
        std::vector<Divvied> dv(K);
        struct Pending { uint32_t k; std::vector<std::vector<uint32_t>> walks1, walks2; std::vector<uint32_t> idx1, idx2; };
        // the sets are independent: gather each set's walks per gap in parallel, then append to the gaps in set order
        std::vector<std::vector<Pending>> pend_of(cur.size());
        cl_parallel_for(cur.size(), [&](uint64_t pos_begin, uint64_t pos_end) {
        for (size_t pos = pos_begin; pos < pos_end; ++pos) {
            const uint64_t s = cur[pos];
            std::vector<Pending>& pend = pend_of[pos];
            for (uint64_t j = 0; j < ms->set_off1[s + 1] - ms->set_off1[s]; ++j) {
                const uint32_t *b, *e;
                walk(0, pos, (uint32_t)j, b, e);
                const uint32_t k = ft[0][b[0]].first;
                if (k == none || k != ft[0][e[-1]].first) continue;
                auto it = std::find_if(pend.begin(), pend.end(), [&](const Pending& q) { return q.k == k; });
                if (it == pend.end()) { pend.emplace_back(); pend.back().k = k; it = pend.end() - 1; }
                it->idx1.push_back((uint32_t)j);
                it->walks1.emplace_back();
                for (const uint32_t* v = b; v != e; ++v) it->walks1.back().push_back(ft[0][*v].second);
            }
            if (pend.empty()) continue;
            for (uint64_t j = 0; j < ms->set_off2[s + 1] - ms->set_off2[s]; ++j) {
                const uint32_t *b, *e;
                walk(1, pos, (uint32_t)j, b, e);
                const uint32_t k = ft[1][b[0]].first;
                auto it = std::find_if(pend.begin(), pend.end(), [&](const Pending& q) { return q.k == k; });
                if (it == pend.end() || k != ft[1][e[-1]].first) continue;
                it->idx2.push_back((uint32_t)j);
                it->walks2.emplace_back();
                for (const uint32_t* v = b; v != e; ++v) it->walks2.back().push_back(ft[1][*v].second);
            }
        }
        }, 2048);
        for (size_t pos = 0; pos < cur.size(); ++pos) {
            const uint64_t s = cur[pos];
            for (Pending& q : pend_of[pos]) {
                if (q.walks2.empty()) continue;
                Divvied& d = dv[q.k];
                for (auto& w : q.walks1) { d.sets.nodes1.insert(d.sets.nodes1.end(), w.begin(), w.end()); d.sets.walk_off1.push_back(d.sets.nodes1.size()); }
                d.sets.set_off1.push_back(d.sets.walk_off1.size() - 1);
                for (auto& w : q.walks2) { d.sets.nodes2.insert(d.sets.nodes2.end(), w.begin(), w.end()); d.sets.walk_off2.push_back(d.sets.nodes2.size()); }
                d.sets.set_off2.push_back(d.sets.walk_off2.size() - 1);
                d.sets.count1.push_back(ms->count1[s]);
                d.sets.count2.push_back(ms->count2[s]);
                d.sets.full_length.push_back(ms->full_length[s]);
                d.origin_set.push_back(pos);
                d.origin_idx1.push_back(std::move(q.idx1));
                d.origin_idx2.push_back(std::move(q.idx2));
            }
        }
        lap("fill-in: divvy", t);
        // assign_reanchor_budget (src/anchorer.cpp:136-154)
        uint64_t total = 0;
        auto matrix_size = [&](size_t k) { return (ob.side[0].node_off[k + 1] - ob.side[0].node_off[k] + 1) * (ob.side[1].node_off[k + 1] - ob.side[1].node_off[k] + 1); };
        for (size_t k = 0; k < K; ++k) total += matrix_size(k);
        // the instances: inner anchor_chain (anchorer.hpp:1091-1329) on the gap's subgraphs with their sources / sinks
        struct Inst { size_t k; bool swap; std::vector<uint64_t> order; cl_match_sets view; FillSide side[2]; };
        std::vector<std::unique_ptr<Inst>> inst;
        std::vector<ChainSub> subs;
        for (size_t k = 0; k < K; ++k) {
            if (dv[k].origin_set.empty()) continue;
            inst.emplace_back(new Inst());
            Inst& in = *inst.back();
            in.k = k;
            in.side[0].project(ob.side[0], k, steps1, 0);
            in.side[1].project(ob.side[1], k, steps2, (uint32_t)g1->n_paths);
            in.swap = in.side[0].view.n_nodes * in.side[0].view.n_paths > in.side[1].view.n_nodes * in.side[1].view.n_paths;
            in.view = dv[k].sets.view();
            in.order.resize(in.view.n_sets);
            std::iota(in.order.begin(), in.order.end(), (uint64_t)0);
            const uint64_t budget = (uint64_t)ceil((double)ap->max_num_match_pairs * (double)matrix_size(k) / (double)total);
            const uint64_t n_use = select_matches(in.view, cp, in.order, budget);
            ChainSub sb;
            sb.tableau = false;
            sb.chain_merge = sparse_algo;
            sb.ms = &in.view;
            sb.order = in.order.data();
            sb.swap_sides = in.swap;
            sb.num_match_sets = n_use;
            sb.anchored = true;
            if (mask) {   // a divvied pair is masked if the pair it came from is (anchorer.hpp:662-680)
                const Divvied* dk = &dv[k];
                const std::vector<uint64_t>* order_now = &cur;
                sb.masked = [mask, dk, order_now](uint64_t set, uint32_t i1, uint32_t i2) {
                    return mask->has((*order_now)[dk->origin_set[set]], dk->origin_idx1[set][i1], dk->origin_idx2[set][i2]);
                };
            }
            for (int d = 0; d < 2; ++d) {
                const int from = in.swap ? 1 - d : d;
                const auto& sd = ob.side[from];
                sb.g[d] = &in.side[from].view;
                sb.tag[d] = in.side[from].tag;
                sb.src[d].assign(sd.src_idx.begin() + sd.src_off[k], sd.src_idx.begin() + sd.src_off[k + 1]);
                sb.snk[d].assign(sd.snk_idx.begin() + sd.snk_off[k], sd.snk_idx.begin() + sd.snk_off[k + 1]);
            }
            subs.push_back(std::move(sb));
        }
        lap("fill-in: instances", t);
        std::vector<ChainSubResult> res;
        if (!subs.empty()) {
            ChainTimings tm;
            rc = chain_dp_batch(ctx, subs, &cp, anchor_scale, sparse, res, tm, nullptr);
            if (rc) return rc;
            out->fill_in_pairs += tm.n_pairs;
            out->fill_in_device_ms += tm.device_ms;
        }
        lap("fill-in: batched DP", t);
        // translate the gap chains back (inner un-swap, anchorer.hpp:1309-1322) and merge (src/anchorer.cpp:157-222)
        std::vector<std::vector<HAnchor>> fill(K);
        for (size_t q = 0; q < inst.size(); ++q) {
            const Inst& in = *inst[q];
            const ChainSubResult& r = res[q];
            out->n_ties += r.n_ties;
            const Divvied& d = dv[in.k];
            const size_t na = r.chain.size() / 3;
            for (size_t i = 0; i < na; ++i) {
                const uint32_t pos = r.chain[3 * i];
                uint32_t a = r.chain[3 * i + 1], b = r.chain[3 * i + 2];
                if (in.swap) std::swap(a, b);
                const uint64_t set = in.order[pos];
                HAnchor h;
                for (int side = 0; side < 2; ++side) {
                    const auto& so = side ? d.sets.set_off2 : d.sets.set_off1;
                    const auto& wo = side ? d.sets.walk_off2 : d.sets.walk_off1;
                    const auto& nd = side ? d.sets.nodes2 : d.sets.nodes1;
                    const uint64_t w = so[set] + (side ? b : a);
                    auto& dst = side ? h.w2 : h.w1;
                    for (uint64_t v = wo[w]; v < wo[w + 1]; ++v) dst.push_back((uint32_t)ob.side[side].back[ob.side[side].node_off[in.k] + nd[v]]);
                }
                h.count1 = d.sets.count1[set]; h.count2 = d.sets.count2[set]; h.full_length = d.sets.full_length[set];
                h.score = anchor_weight(cp, h.count1, h.count2, h.w1.size(), h.full_length);
                // identity: the reference indexes its origin table with the POSITION in the (possibly reordered) gap match
                // sets (src/anchorer.cpp:207-212), kept as is; out of range -> all ones
                h.match_set = d.origin_set[pos];
                h.idx1 = a < d.origin_idx1[pos].size() ? d.origin_idx1[pos][a] : UINT64_MAX;
                h.idx2 = b < d.origin_idx2[pos].size() ? d.origin_idx2[pos][b] : UINT64_MAX;
                if (!sparse) {
                    h.gb = in.swap ? -r.gap[i] : r.gap[i];
                    h.ga = in.swap ? -r.gap[i + 1] : r.gap[i + 1];
                    h.gsb = r.gap_score[i];
                    h.gsa = r.gap_score[i + 1];
                }
                fill[in.k].push_back(std::move(h));
            }
        }
        std::vector<HAnchor> merged;
        for (size_t k = 0; k < K; ++k) {
            if (k != 0) {
                HAnchor& a = anchors[k - 1];
                if (!merged.empty()) { a.gb = merged.back().ga; a.gsb = merged.back().gsa; }
                merged.push_back(std::move(a));
            }
            for (size_t j = 0; j < fill[k].size(); ++j) {
                if (j == 0 && !merged.empty()) { merged.back().gsa = fill[k][j].gsb; merged.back().ga = fill[k][j].gb; }
                merged.push_back(std::move(fill[k][j]));
            }
        }
        anchors.swap(merged);
        lap("fill-in: merge", t);
        return CL_OK;
    };

    // ---- anchor_chain with a given algorithm and scale (anchorer.hpp:1050-1089)
    auto run = [&](bool sparse, double anchor_scale, std::vector<HAnchor>& anchors) -> int {
        const uint64_t local_max = std::min<uint64_t>((uint64_t)llround((anchor_scale / ap->score_scale) * (double)ap->max_num_match_pairs),
                                                     ap->max_num_match_pairs);
        auto t = now();
        const uint64_t n_use = select_matches(*ms, cp, cur, local_max);
        lap(sparse ? "sparse: select" : "affine: select", t);
        std::vector<ChainSub> subs(1, whole_graph_instance(swap ? g2 : g1, swap ? g1 : g2, ms, n_use, cp.global_anchoring != 0));
        subs[0].order = cur.data();
        subs[0].swap_sides = swap;
        if (mask) subs[0].masked = [mask](uint64_t set, uint32_t i1, uint32_t i2) { return mask->has(set, i1, i2); };
        subs[0].x[0] = swap ? &x2 : &x1; subs[0].x[1] = swap ? &x1 : &x2;
        subs[0].sw[0] = swap ? &sw2 : &sw1; subs[0].sw[1] = swap ? &sw1 : &sw2;
        subs[0].order1 = &order_dp1;
        std::vector<ChainSubResult> res;
        ChainTimings tm;
        int rc = chain_dp_batch(ctx, subs, &cp, anchor_scale, sparse, res, tm, nullptr);
        if (rc) return rc;
        lap(sparse ? "sparse: chain DP" : "affine: chain DP", t);
        if (timing) fprintf(stderr, "[cl_anchor_chain]   prep %.1f device %.1f index %.1f traceback %.1f ms, %llu pairs, %u combinations\n", tm.prep_ms, tm.device_ms, tm.index_ms, tm.traceback_ms, (unsigned long long)tm.n_pairs, tm.n_combos);
        out->dp_device_ms += tm.device_ms;
        out->dp_pair_evals += tm.pair_evals;
        if (!sparse) { out->dp_match_pairs = tm.n_pairs; out->dp_combinations = tm.n_combos; }
        out->n_ties += res[0].n_ties;
        const ChainSubResult& r = res[0];
        const size_t na = r.chain.size() / 3;
        anchors.assign(na, HAnchor());
        cl_parallel_for(na, [&](uint64_t i_begin, uint64_t i_end) {
        for (size_t i = i_begin; i < i_end; ++i) {
            HAnchor& h = anchors[i];
            h.match_set = r.chain[3 * i];
            h.idx1 = r.chain[3 * i + 1];
            h.idx2 = r.chain[3 * i + 2];
            if (swap) std::swap(h.idx1, h.idx2);
            const uint32_t *b, *e;
            walk(0, h.match_set, (uint32_t)h.idx1, b, e);
            h.w1.assign(b, e);
            walk(1, h.match_set, (uint32_t)h.idx2, b, e);
            h.w2.assign(b, e);
            const uint64_t s = cur[h.match_set];
            h.count1 = ms->count1[s]; h.count2 = ms->count2[s]; h.full_length = ms->full_length[s];
            h.score = anchor_weight(cp, h.count1, h.count2, h.w1.size(), h.full_length);
            if (!sparse) {   // annotation in the DP's orientation, negated back at anchorer.hpp:1318-1320
                h.gb = swap ? -r.gap[i] : r.gap[i];
                h.ga = swap ? -r.gap[i + 1] : r.gap[i + 1];
                h.gsb = r.gap_score[i];
                h.gsa = r.gap_score[i + 1];
            }
        }
        }, 512);
        lap("anchors", t);
        if (ap->do_fill_in_anchoring) return fill_in(anchors, sparse, anchor_scale);
        return CL_OK;
    };

    // ---- estimate_score_scale (anchorer.hpp:998-1047)
    double scale = 1.0;
    int rc;
    std::vector<HAnchor> sc;   // the chain of the estimate: estimate_score_scale's chain_out (anchorer.hpp:1042-1044)
    if (override_scale && !scale_only) scale = *override_scale;   // anchorer.hpp:975-978
    else if (sparse_algo && !scale_only) scale = 1.0;             // (:979: the estimate only adjusts gap penalties, which Sparse does not have)
    else if (ap->autocalibrate_gap_penalties) {
        if ((rc = run(true, 1.0, sc))) return rc;
        auto t = now();
        double total_weight = 0.0;
        uint64_t total_length = 0;
        const size_t na = sc.size();
        std::vector<uint64_t> seg_off{0, na}, walk_off{0};
        std::vector<uint32_t> w1, w2;
        for (const HAnchor& a : sc) {
            total_weight += anchor_weight(cp, a.count1, a.count2, a.w1.size(), a.full_length);
            total_length += a.w1.size();
            w1.insert(w1.end(), a.w1.begin(), a.w1.end());
            w2.insert(w2.end(), a.w2.begin(), a.w2.end());
            walk_off.push_back(w1.size());
        }
        cl_anchor_segments sg{na ? 1u : 0u, seg_off.data(), walk_off.data(), w1.data(), w2.data()};
        clhost::OwnedBatch ob;
        if ((rc = clhost::extract_stitch_batch(*g1, *g2, sg, ob, &x1, &x2))) { cl_set_error(ctx, "extraction failed"); return rc; }
        for (uint64_t k = 0; k < ob.only_del.size(); ++k) {
            uint64_t fill = UINT64_MAX;
            for (int side = 0; side < 2; ++side) {
                const auto& sd = ob.side[side];
                if (sd.node_off[k + 1] == sd.node_off[k]) fill = 0;
                else fill = std::min<uint64_t>(fill, (uint64_t)min_source_sink(sd, k));
            }
            total_length += fill;
        }
        scale = total_weight / (double)total_length;
        lap("scale estimate: extraction", t);
    }
    out->scale = scale;
    if (scale_only && !keep_scale_chain) return CL_OK;

    // ---- the affine chain (or, for cl_leaf_calibrate, the estimate's own chain)
    std::vector<HAnchor> ch;
    if (scale_only) ch.swap(sc);
    else if ((rc = run(sparse_algo, scale, ch))) return rc;
    const size_t na = ch.size();
    uint64_t total_walk = 0;
    for (const HAnchor& a : ch) total_walk += a.w1.size();
    out->n_anchors = na;
    out->n_sets = cur.size();
    const size_t na1 = na ? na : 1;
    out->anchors = (uint64_t*)malloc(na1 * 3 * sizeof(uint64_t));
    out->gap_before = (int64_t*)calloc(na1, sizeof(int64_t));
    out->gap_after = (int64_t*)calloc(na1, sizeof(int64_t));
    out->gap_score_before = (double*)calloc(na1, sizeof(double));
    out->gap_score_after = (double*)calloc(na1, sizeof(double));
    out->score = (double*)calloc(na1, sizeof(double));
    out->count1 = (uint64_t*)calloc(na1, sizeof(uint64_t));
    out->count2 = (uint64_t*)calloc(na1, sizeof(uint64_t));
    out->full_length = (uint64_t*)calloc(na1, sizeof(uint64_t));
    out->walk_off = (uint64_t*)calloc(na + 1, sizeof(uint64_t));
    out->walk1 = (uint32_t*)malloc((total_walk ? total_walk : 1) * sizeof(uint32_t));
    out->walk2 = (uint32_t*)malloc((total_walk ? total_walk : 1) * sizeof(uint32_t));
    out->set_order = (uint64_t*)malloc((cur.size() ? cur.size() : 1) * sizeof(uint64_t));
    if (!out->anchors || !out->gap_before || !out->gap_after || !out->gap_score_before || !out->gap_score_after || !out->score ||
        !out->count1 || !out->count2 || !out->full_length || !out->walk_off || !out->walk1 || !out->walk2 || !out->set_order) {
        cl_anchor_chain_result_free(out);
        return CL_ERR_OUT_OF_MEMORY;
    }
    memcpy(out->set_order, cur.data(), cur.size() * sizeof(uint64_t));
    uint64_t wpos = 0;
    for (size_t i = 0; i < na; ++i) {
        const HAnchor& a = ch[i];
        out->anchors[3 * i] = a.match_set; out->anchors[3 * i + 1] = a.idx1; out->anchors[3 * i + 2] = a.idx2;
        out->gap_before[i] = a.gb; out->gap_after[i] = a.ga;
        out->gap_score_before[i] = a.gsb; out->gap_score_after[i] = a.gsa;
        out->score[i] = a.score;
        out->count1[i] = a.count1; out->count2[i] = a.count2; out->full_length[i] = a.full_length;
        memcpy(out->walk1 + wpos, a.w1.data(), a.w1.size() * sizeof(uint32_t));
        memcpy(out->walk2 + wpos, a.w2.data(), a.w2.size() * sizeof(uint32_t));
        wpos += a.w1.size();
        out->walk_off[i + 1] = wpos;
    }
    return CL_OK;
}

extern "C" {

int cl_anchor_chain(cl_context* ctx, const cl_base_graph* g1, const cl_base_graph* g2, const cl_match_sets* ms,
                    const cl_anchor_params* ap, cl_anchor_chain_result* out) {
    return anchor_chain_impl(ctx, g1, g2, ms, ap, out, false);
}

int cl_anchor_chain_masked(cl_context* ctx, const cl_base_graph* g1, const cl_base_graph* g2, const cl_match_sets* ms, const cl_anchor_params* ap,
                           const uint64_t* masked, uint64_t n_masked, const double* override_scale, cl_anchor_chain_result* out) {
    cl_bind_device(ctx);
    if (n_masked && !masked) { cl_set_error(ctx, "null mask"); return CL_ERR_INVALID_ARGUMENT; }
    MaskSet mask;
    mask.v.resize(n_masked);
    for (uint64_t i = 0; i < n_masked; ++i) mask.v[i] = {masked[3 * i], masked[3 * i + 1], masked[3 * i + 2]};
    std::sort(mask.v.begin(), mask.v.end());
    mask.v.erase(std::unique(mask.v.begin(), mask.v.end()), mask.v.end());
    return anchor_chain_impl(ctx, g1, g2, ms, ap, out, false, n_masked ? &mask : nullptr, override_scale);
}

// Core::generate_diagonal_mask (src/core.cpp:301-321): in a self-comparison, the pairs of a set whose two walks start at the same node
int cl_generate_diagonal_mask(const cl_match_sets* ms, uint64_t** masked_out, uint64_t* n_masked_out) {
    if (!ms || !masked_out || !n_masked_out) return CL_ERR_INVALID_ARGUMENT;
    std::vector<uint64_t> m;
    std::unordered_map<uint32_t, uint64_t> start_to_idx;
    for (uint64_t s = 0; s < ms->n_sets; ++s) {
        start_to_idx.clear();
        for (uint64_t j = ms->set_off1[s]; j < ms->set_off1[s + 1]; ++j) start_to_idx[ms->nodes1[ms->walk_off1[j]]] = j - ms->set_off1[s];   // the last walk wins (:309-311)
        for (uint64_t k = ms->set_off2[s]; k < ms->set_off2[s + 1]; ++k) {
            auto it = start_to_idx.find(ms->nodes2[ms->walk_off2[k]]);
            if (it != start_to_idx.end()) { m.push_back(s); m.push_back(it->second); m.push_back(k - ms->set_off2[s]); }
        }
    }
    *n_masked_out = m.size() / 3;
    *masked_out = (uint64_t*)malloc((m.size() ? m.size() : 1) * sizeof(uint64_t));
    if (!*masked_out) return CL_ERR_OUT_OF_MEMORY;
    if (!m.empty()) memcpy(*masked_out, m.data(), m.size() * sizeof(uint64_t));
    return CL_OK;
}

// Core::update_mask (src/core.cpp:323-372): every pair (set, j, k) in which some position of walk1 j and the same position of walk2 k are a
// node pair of the chain (or its mirror image) is added to the mask.  The result is the union, sorted, without duplicates.
int cl_update_mask(const cl_match_sets* ms, uint64_t n_chain_pairs, const uint32_t* chain_walk1, const uint32_t* chain_walk2, int mask_reciprocal,
                   const uint64_t* masked, uint64_t n_masked, uint64_t** masked_out, uint64_t* n_masked_out) {
    if (!ms || !masked_out || !n_masked_out || (n_chain_pairs && (!chain_walk1 || !chain_walk2)) || (n_masked && !masked)) return CL_ERR_INVALID_ARGUMENT;
    std::unordered_map<uint32_t, uint32_t> paired;   // later pairs overwrite earlier ones (:330-337)
    for (uint64_t i = 0; i < n_chain_pairs; ++i) {
        paired[chain_walk1[i]] = chain_walk2[i];
        if (mask_reciprocal) paired[chain_walk2[i]] = chain_walk1[i];
    }
    std::vector<std::array<uint64_t, 3>> m(n_masked);
    for (uint64_t i = 0; i < n_masked; ++i) m[i] = {masked[3 * i], masked[3 * i + 1], masked[3 * i + 2]};
    std::unordered_map<uint64_t, std::vector<uint32_t>> walk2_node;   // (position << 32 | node) -> walk2 indexes
    for (uint64_t s = 0; s < ms->n_sets; ++s) {
        walk2_node.clear();
        const uint64_t n1 = ms->set_off1[s + 1] - ms->set_off1[s], n2 = ms->set_off2[s + 1] - ms->set_off2[s];
        for (uint64_t k = 0; k < n2; ++k) {
            const uint64_t w = ms->set_off2[s] + k;
            for (uint64_t l = ms->walk_off2[w]; l < ms->walk_off2[w + 1]; ++l) walk2_node[((l - ms->walk_off2[w]) << 32) | ms->nodes2[l]].push_back((uint32_t)k);
        }
        for (uint64_t j = 0; j < n1; ++j) {
            const uint64_t w = ms->set_off1[s] + j;
            for (uint64_t l = ms->walk_off1[w]; l < ms->walk_off1[w + 1]; ++l) {
                auto it = paired.find(ms->nodes1[l]);
                if (it == paired.end()) continue;
                auto it2 = walk2_node.find(((l - ms->walk_off1[w]) << 32) | it->second);
                if (it2 == walk2_node.end()) continue;
                for (uint32_t k : it2->second) m.push_back({s, j, (uint64_t)k});
            }
        }
    }
    std::sort(m.begin(), m.end());
    m.erase(std::unique(m.begin(), m.end()), m.end());
    *n_masked_out = m.size();
    *masked_out = (uint64_t*)malloc((m.size() ? m.size() : 1) * 3 * sizeof(uint64_t));
    if (!*masked_out) return CL_ERR_OUT_OF_MEMORY;
    for (size_t i = 0; i < m.size(); ++i) { (*masked_out)[3 * i] = m[i][0]; (*masked_out)[3 * i + 1] = m[i][1]; (*masked_out)[3 * i + 2] = m[i][2]; }
    return CL_OK;
}

// Anchorer::estimate_score_scale with its chain_out (anchorer.hpp:998-1047): out->scale and the chain the estimate was made on
int cl_estimate_score_scale_chain(cl_context* ctx, const cl_base_graph* g1, const cl_base_graph* g2, const cl_match_sets* ms,
                                  const cl_anchor_params* ap, cl_anchor_chain_result* out) {
    cl_bind_device(ctx);
    if (!ap || !out) return CL_ERR_INVALID_ARGUMENT;
    cl_anchor_params p = *ap;
    p.autocalibrate_gap_penalties = 1;
    return anchor_chain_impl(ctx, g1, g2, ms, &p, out, true, nullptr, nullptr, true);
}

int cl_estimate_score_scale(cl_context* ctx, const cl_base_graph* g1, const cl_base_graph* g2, const cl_match_sets* ms,
                            const cl_anchor_params* ap, double* scale_out) {
    cl_bind_device(ctx);
    if (!ap || !scale_out) return CL_ERR_INVALID_ARGUMENT;
    cl_anchor_params p = *ap;
    p.autocalibrate_gap_penalties = 1;
    cl_anchor_chain_result r;
    const int rc = anchor_chain_impl(ctx, g1, g2, ms, &p, &r, true);
    if (rc) return rc;
    *scale_out = r.scale;
    return CL_OK;
}

}  // extern "C"
