// cl_stitch_plan_api.cpp — a stitch plan's construction (cl_stitch_plan_create), phase by phase.
//
// Mirrors, for a whole batch of between-anchor subproblems at once, what the reference does per
// subproblem on one CPU thread:
//   Stitcher::subalign      (src/stitcher.cpp:24-78)              -> choose_num_pw(), translate in collect
//   Stitcher::do_alignment  (include/centrolign/stitcher.hpp:237-370) -> route_problem()
//   pure_deletion_alignment (include/centrolign/alignment.hpp:1178-1210) -> pure_deletion() (host, O(n))
//   po_poa                  (alignment.hpp:753-1163)              -> packed to rank space here, DP + traceback
//                                                                    on the GPU (popoa_kernels.hip)
// The phases: validate the arguments; pack every subproblem (route -> host route | both graphs into rank space -> which kernel takes the pair); append the
// parts in order; form the launch groups, family by family; the persistent one-wave launch and the narrow launch over the group list; estimate and order;
// upload and allocate.  Everything up to the upload is plain host code: the two device facts it needs (how many workgroups of the persistent / the narrow
// kernel are resident at once) are handed in.  The plan is run by cl_stitch_exec_api.cpp; stitch_plan.hpp is what the two share.
// Also here, with the helpers they share with the packer: the host-only entry points cl_host_route_align, cl_stitch_rank_order and cl_stitch_sys_choice.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <new>
#include <string>
#include <thread>
#include <unordered_map>
#include <vector>

#include "cl_internal.hpp"
#include "popoa_device.h"
#include "stitch_plan.hpp"
#include "wfa_host.hpp"

#define set_error cl_set_error

namespace {

// ---- one graph of one problem, as a view into the flat batch -------------------------------------------
struct GraphView {
    uint64_t n = 0;
    const uint8_t* label = nullptr;
    const uint64_t* prev_off = nullptr;  // n+1 entries, absolute into prev_idx
    const uint32_t* prev_idx = nullptr;
    const uint64_t* next_off = nullptr;  // may be null
    const uint32_t* next_idx = nullptr;
    uint64_t n_src = 0, n_snk = 0;
    const uint32_t* src = nullptr;
    const uint32_t* snk = nullptr;
};

GraphView view(const cl_graph_side& s, uint64_t k) {
    GraphView g;
    uint64_t b = s.node_off[k];
    g.n = s.node_off[k + 1] - b;
    g.label = s.label + b;
    g.prev_off = s.prev_off + b;
    g.prev_idx = s.prev_idx;
    g.next_off = s.next_off ? s.next_off + b : nullptr;
    g.next_idx = s.next_idx;
    g.n_src = s.src_off[k + 1] - s.src_off[k];
    g.src = s.src_idx + s.src_off[k];
    g.n_snk = s.snk_off[k + 1] - s.snk_off[k];
    g.snk = s.snk_idx + s.snk_off[k];
    return g;
}

int validate_side(cl_context* ctx, const cl_graph_side& s, uint64_t n, int which) {
    if (!s.node_off || !s.prev_off || !s.src_off || !s.snk_off) {
        set_error(ctx, "graph side %d: missing offset array", which);
        return CL_ERR_INVALID_ARGUMENT;
    }
    // (the offsets are absolute positions in the side's arrays; they need not start at 0: run_whole hands chunks of a batch on as views)
    for (uint64_t k = 0; k < n; ++k) {
        if (s.node_off[k + 1] < s.node_off[k] || s.src_off[k + 1] < s.src_off[k] || s.snk_off[k + 1] < s.snk_off[k]) {
            set_error(ctx, "graph side %d: offsets not monotone at problem %llu", which, (unsigned long long)k);
            return CL_ERR_INVALID_ARGUMENT;
        }
        uint64_t nn = s.node_off[k + 1] - s.node_off[k];
        if (nn >= (1ull << 31)) {
            set_error(ctx, "graph side %d: problem %llu has too many nodes", which, (unsigned long long)k);
            return CL_ERR_INVALID_ARGUMENT;
        }
        for (uint64_t i = s.src_off[k]; i < s.src_off[k + 1]; ++i)
            if (s.src_idx[i] >= nn) { set_error(ctx, "graph side %d: source id out of range in problem %llu", which, (unsigned long long)k); return CL_ERR_INVALID_ARGUMENT; }
        for (uint64_t i = s.snk_off[k]; i < s.snk_off[k + 1]; ++i)
            if (s.snk_idx[i] >= nn) { set_error(ctx, "graph side %d: sink id out of range in problem %llu", which, (unsigned long long)k); return CL_ERR_INVALID_ARGUMENT; }
        for (uint64_t v = s.node_off[k]; v < s.node_off[k + 1]; ++v) {
            if (s.prev_off[v + 1] < s.prev_off[v]) { set_error(ctx, "graph side %d: prev_off not monotone", which); return CL_ERR_INVALID_ARGUMENT; }
            for (uint64_t e = s.prev_off[v]; e < s.prev_off[v + 1]; ++e)
                if (s.prev_idx[e] >= nn) { set_error(ctx, "graph side %d: predecessor id out of range in problem %llu", which, (unsigned long long)k); return CL_ERR_INVALID_ARGUMENT; }
        }
    }
    return CL_OK;
}

// next lists (ids local), derived from prev lists when the caller did not pass them.  Only the order inside
// a list could differ from BaseGraph's, and nothing downstream depends on it.
struct NextLists {
    std::vector<uint64_t> off;
    std::vector<uint32_t> idx;
    const uint64_t* o = nullptr;
    const uint32_t* i = nullptr;
    uint64_t base = 0;  // o[v] - base indexes i when derived; absolute otherwise
    void build(const GraphView& g) {
        if (g.next_off) { o = g.next_off; i = g.next_idx; base = 0; return; }
        uint64_t n = g.n;
        off.assign(n + 2, 0);
        for (uint64_t v = 0; v < n; ++v)
            for (uint64_t e = g.prev_off[v]; e < g.prev_off[v + 1]; ++e) off[g.prev_idx[e] + 2]++;
        for (uint64_t v = 0; v < n; ++v) off[v + 2] += off[v + 1];
        idx.resize(off[n + 1] ? off[n + 1] : 1);
        for (uint64_t v = 0; v < n; ++v)
            for (uint64_t e = g.prev_off[v]; e < g.prev_off[v + 1]; ++e) idx[off[g.prev_idx[e] + 1]++] = (uint32_t)v;
        o = off.data(); i = idx.data(); base = 0;
    }
    uint64_t begin(uint64_t v) const { return o[v]; }
    uint64_t end(uint64_t v) const { return o[v + 1]; }
};

// Kahn's algorithm, LIFO stack seeded in ascending id order (topological_order.hpp:12-60).
// false if the graph has a cycle.
bool topological_order(const GraphView& g, const NextLists& nx, std::vector<uint32_t>& order,
                       std::vector<uint32_t>& scratch_stack, std::vector<uint32_t>& indeg) {
    uint64_t n = g.n;
    order.clear();
    order.reserve(n);
    scratch_stack.clear();
    indeg.resize(n);
    for (uint64_t v = 0; v < n; ++v) {
        indeg[v] = (uint32_t)(g.prev_off[v + 1] - g.prev_off[v]);
        if (indeg[v] == 0) scratch_stack.push_back((uint32_t)v);
    }
    while (!scratch_stack.empty()) {
        uint32_t v = scratch_stack.back();
        scratch_stack.pop_back();
        order.push_back(v);
        for (uint64_t e = nx.begin(v); e < nx.end(v); ++e) {
            uint32_t w = nx.i[e];
            if (--indeg[w] == 0) scratch_stack.push_back(w);
        }
    }
    return order.size() == n;
}

// Which topological order the DEVICE ranks a subgraph's nodes by.  Nothing in the result depends on it: the DP's values are those of any topological order and every
// tie of the traceback is decided by the order of a node's previous() list and of the sink list, both of which are kept as they come.  What depends
// on it is how far back a row (column) of the matrix reads.  The reference's order (Kahn with a LIFO stack, topological_order.hpp:12-60) lays the branches of a bubble
// out one after the other: the second branch's first node and the node that closes the bubble read a whole branch back — a "far fork", which the register kernel
// cannot take, which deepens the systolic kernels' rings by the branch length, and which on BOTH sides of a large pair left only the anti-diagonal sweep.  The LEVEL
// order (by the longest path from a source, ties in the reference's order) interleaves the branches: inside a bubble of two branches every node reads two ranks back,
// whatever the branches' length; what remains far is the difference of the branches' lengths, once, at the closing node.  Per graph the order with fewer far reads
// (more than four ranks back: the register kernel's reach) wins, then the one with the smaller reach, then the reference's — so chains and graphs whose bubbles are
// single nodes keep the order they had.  CL_RANK_ORDER=lifo|level forces one (measurements, tests).  `order` / `rank` come in as the reference's order and leave as the choice.
// (read when a plan is made, so that a test can make plans both ways)
int rank_order_now() { const char* e = getenv("CL_RANK_ORDER"); return !e ? 0 : !strcmp(e, "lifo") ? 1 : !strcmp(e, "level") ? 2 : 0; }
void choose_rank_order(const GraphView& g, int g_rank_order, std::vector<uint32_t>& order, std::vector<uint32_t>& rank, std::vector<uint32_t>& level, std::vector<uint32_t>& scratch) {
    const uint64_t n = g.n;
    if (g_rank_order == 1 || n < 4) return;
    auto reach = [&](uint64_t& far, uint64_t& longest) {
        far = longest = 0;
        for (uint64_t v = 0; v < n; ++v)
            for (uint64_t e = g.prev_off[v]; e < g.prev_off[v + 1]; ++e) {
                const uint64_t back = rank[v] - rank[g.prev_idx[e]];
                far += back > 4;
                longest = std::max(longest, back);
            }
        for (uint64_t i = 0; i < g.n_src; ++i) {   // a source reads the boundary, index 0
            const uint64_t back = (uint64_t)rank[g.src[i]] + 1;
            far += back > 4;
            longest = std::max(longest, back);
        }
    };
    uint64_t far_ref, longest_ref;
    reach(far_ref, longest_ref);
    if (longest_ref <= 1 + (g.n_src > 1) && g_rank_order != 2) return;   // a chain
    level.assign(n, 0);
    uint32_t deepest = 0;
    for (uint64_t r = 0; r < n; ++r) {
        const uint32_t v = order[r];
        uint32_t l = 0;
        for (uint64_t e = g.prev_off[v]; e < g.prev_off[v + 1]; ++e) l = std::max(l, level[g.prev_idx[e]] + 1);
        level[v] = l;
        deepest = std::max(deepest, l);
    }
    // counting sort by level, stable in the reference's order
    scratch.assign((size_t)deepest + 2, 0);
    for (uint64_t v = 0; v < n; ++v) ++scratch[level[v] + 1];
    for (uint32_t l = 0; l <= deepest; ++l) scratch[l + 1] += scratch[l];
    std::vector<uint32_t> by_level(n);
    for (uint64_t r = 0; r < n; ++r) by_level[scratch[level[order[r]]]++] = order[r];
    std::vector<uint32_t> rank_ref(rank);
    for (uint32_t r = 0; r < n; ++r) rank[by_level[r]] = r;
    uint64_t far_lvl, longest_lvl;
    reach(far_lvl, longest_lvl);
    if (g_rank_order == 2 || far_lvl < far_ref || (far_lvl == far_ref && longest_lvl < longest_ref)) order.swap(by_level);
    else rank.swap(rank_ref);
}

// src/stitcher.cpp:31-52
int choose_num_pw(uint64_t n1, uint64_t n2, const cl_align_params& p) {
    uint64_t cutoffs[2];
    for (int i = 1; i < 3; ++i) {
        if (p.gap_open[i - 1] > p.gap_open[i] || p.gap_extend[i - 1] < p.gap_extend[i]) return CL_ERR_BAD_GAP_PARAMS;
        uint32_t diff_open = p.gap_open[i] - p.gap_open[i - 1];
        uint32_t diff_extend = p.gap_extend[i - 1] - p.gap_extend[i];
        if (diff_extend == 0) return CL_ERR_BAD_GAP_PARAMS;  // the reference would divide by zero
        cutoffs[i - 1] = (diff_open + diff_extend - 1) / diff_extend;
    }
    int c = 0;
    while (c < 2 && n1 > cutoffs[c] && n2 > cutoffs[c]) ++c;
    return c + 1;
}

// Extractor::source_sink_minmax (src/anchorer.cpp:14-23) over minmax_distance (minmax_distance.hpp:16-72)
bool source_sink_minmax(const GraphView& g, int64_t& mn_out, int64_t& mx_out) {
    NextLists nx;
    nx.build(g);
    std::vector<uint32_t> order, st, indeg;
    if (!topological_order(g, nx, order, st, indeg)) return false;
    const int64_t INF = std::numeric_limits<int64_t>::max();
    std::vector<int64_t> mn(g.n, INF), mx(g.n, -1);
    for (uint64_t i = 0; i < g.n_src; ++i) { mn[g.src[i]] = 0; mx[g.src[i]] = 0; }
    for (uint32_t v : order) {
        if (mn[v] == INF) continue;
        for (uint64_t e = nx.begin(v); e < nx.end(v); ++e) {
            uint32_t w = nx.i[e];
            mn[w] = std::min(mn[w], mn[v] + 1);
            mx[w] = std::max(mx[w], mx[v] + 1);
        }
    }
    mn_out = INF;
    mx_out = -1;
    for (uint64_t i = 0; i < g.n_snk; ++i) {
        mn_out = std::min(mn_out, mn[g.snk[i]]);
        mx_out = std::max(mx_out, mx[g.snk[i]]);
    }
    return true;
}

// include/centrolign/stitcher.hpp:268-360
int route_problem(const GraphView& g1, const GraphView& g2, bool only_del, const cl_stitch_params& sp) {
    if (g2.n == 0) return CL_ROUTE_PURE_DELETION_1;
    if (g1.n == 0) return CL_ROUTE_PURE_DELETION_2;
    uint64_t mat = (g1.n + 1) * (g2.n + 1);
    if (mat <= sp.min_wfa_size && (!only_del || mat <= sp.max_trivial_size)) return CL_ROUTE_PO_POA;
    int64_t a1, b1, a2, b2;
    if (!source_sink_minmax(g1, a1, b1) || !source_sink_minmax(g2, a2, b2)) return CL_ERR_CYCLIC_GRAPH;
    uint64_t min1 = (uint64_t)a1, max1 = (uint64_t)b1, min2 = (uint64_t)a2, max2 = (uint64_t)b2;  // size_t in the reference
    if (max1 * sp.deletion_alignment_ratio <= min2 && max1 <= sp.deletion_alignment_short_max_size &&
        min2 >= sp.deletion_alignment_long_min_size)
        return CL_ROUTE_DELETION_WFA_1;
    if (max2 * sp.deletion_alignment_ratio <= min1 && max2 <= sp.deletion_alignment_short_max_size &&
        min1 >= sp.deletion_alignment_long_min_size)
        return CL_ROUTE_DELETION_WFA_2;
    double r = sp.max_wfa_ratio;
    if (mat < sp.max_wfa_size &&
        ((min2 * r >= min1 && min2 <= max1 * r) || (max2 * r >= min1 && max2 <= max1 * r) ||
         (min1 * r >= min2 && min1 <= max2 * r) || (max1 * r >= min2 && max1 <= max2 * r)) &&
        !only_del)
        return CL_ROUTE_PWFA;
    return CL_ROUTE_GREEDY_PARTIAL;
}

// pure_deletion_alignment (alignment.hpp:1178-1210): shortest source->sink path (shortest_path.hpp:32-100)
// emitted as a run of gaps.  Returns the path in LOCAL node ids.
int pure_deletion(const GraphView& g, std::vector<uint32_t>& path) {
    path.clear();
    if (g.n == 0) return CL_OK;
    NextLists nx;
    nx.build(g);
    std::vector<uint32_t> order, st, indeg;
    if (!topological_order(g, nx, order, st, indeg)) return CL_ERR_CYCLIC_GRAPH;
    const uint64_t INF = (uint64_t)std::numeric_limits<int64_t>::max();
    std::vector<uint64_t> dp(g.n, INF);
    for (uint64_t i = 0; i < g.n_src; ++i) dp[g.src[i]] = 0;
    for (uint32_t v : order) {
        uint64_t thru = dp[v] + 1;
        for (uint64_t e = nx.begin(v); e < nx.end(v); ++e) dp[nx.i[e]] = std::min(dp[nx.i[e]], thru);
    }
    uint64_t best = UINT64_MAX;
    for (uint64_t i = 0; i < g.n_snk; ++i) {
        uint32_t v = g.snk[i];
        if (dp[v] != INF && (best == UINT64_MAX || dp[v] < dp[best])) best = v;
    }
    if (best == UINT64_MAX) return CL_OK;
    uint64_t cur = best;
    path.push_back((uint32_t)cur);
    while (dp[cur] != 0) {
        uint64_t nxt = UINT64_MAX;
        for (uint64_t e = g.prev_off[cur]; e < g.prev_off[cur + 1]; ++e)
            if (dp[g.prev_idx[e]] + 1 == dp[cur]) { nxt = g.prev_idx[e]; break; }
        if (nxt == UINT64_MAX) return CL_ERR_INVALID_ARGUMENT;
        cur = nxt;
        path.push_back((uint32_t)cur);
    }
    std::reverse(path.begin(), path.end());
    return CL_OK;
}

// ---- greedy_partial_alignment (include/centrolign/alignment.hpp:1212-1611): do_alignment's route for gaps that look
// unalignable (stitcher.hpp:340-357).  Host algorithm in the reference as well: exact-match paths grown greedily (DFS over
// label-matching node pairs) from the sources and from the sinks, joined by a double deletion along shortest paths;
// overlapping or mutually unreachable match paths are trimmed by bisection on the total trim.
struct GreedyGraph {
    const GraphView* g;
    NextLists nx;
    std::vector<uint32_t> order;
    std::vector<uint64_t> dp;
    bool init(const GraphView& gv) {
        g = &gv;
        nx.build(gv);
        std::vector<uint32_t> st, indeg;
        dp.resize(gv.n);
        return topological_order(gv, nx, order, st, indeg);
    }
    // shortest_path between node sets (shortest_path.hpp:32-100), empty if there is none
    std::vector<uint64_t> shortest(const std::vector<uint64_t>& from, const std::vector<uint64_t>& to) {
        const uint64_t INF = (uint64_t)std::numeric_limits<int64_t>::max();
        std::fill(dp.begin(), dp.end(), INF);
        for (uint64_t v : from) dp[v] = 0;
        for (uint32_t v : order) {
            const uint64_t thru = dp[v] + 1;
            for (uint64_t e = nx.begin(v); e < nx.end(v); ++e) dp[nx.i[e]] = std::min(dp[nx.i[e]], thru);
        }
        uint64_t best = UINT64_MAX;
        for (uint64_t v : to)
            if (dp[v] != INF && (best == UINT64_MAX || dp[v] < dp[best])) best = v;
        std::vector<uint64_t> path;
        if (best == UINT64_MAX) return path;
        path.push_back(best);
        while (dp[path.back()] != 0) {
            const uint64_t cur = path.back();
            uint64_t nxt = UINT64_MAX;
            for (uint64_t e = g->prev_off[cur]; e < g->prev_off[cur + 1]; ++e)
                if (dp[g->prev_idx[e]] + 1 == dp[cur]) { nxt = g->prev_idx[e]; break; }
            if (nxt == UINT64_MAX) break;
            path.push_back(nxt);
        }
        std::reverse(path.begin(), path.end());
        return path;
    }
    bool reaches(uint64_t from, uint64_t to) { return !shortest(std::vector<uint64_t>(1, from), std::vector<uint64_t>(1, to)).empty(); }
};

int greedy_partial_alignment(const GraphView& gv1, const GraphView& gv2, HostAlignment& out) {
    out.clear();
    GreedyGraph g1, g2;
    if (!g1.init(gv1) || !g2.init(gv2)) return CL_ERR_CYCLIC_GRAPH;
    const uint64_t n2 = gv2.n;
    const std::vector<uint64_t> sources1(gv1.src, gv1.src + gv1.n_src), sources2(gv2.src, gv2.src + gv2.n_src);
    const std::vector<uint64_t> sinks1(gv1.snk, gv1.snk + gv1.n_snk), sinks2(gv2.snk, gv2.snk + gv2.n_snk);
    HostAlignment aln_fwd, aln_rev;
    for (int dir = 0; dir < 2; ++dir) {
        const bool forward = dir == 0;
        size_t max_len = 0;
        uint64_t end_key = UINT64_MAX;
        std::unordered_map<uint64_t, uint64_t> back;   // pair key -> predecessor key (UINT64_MAX at a start)
        struct Item { uint64_t a, b; size_t len; };
        std::vector<Item> stack;
        for (uint64_t a : (forward ? sources1 : sinks1))
            for (uint64_t b : (forward ? sources2 : sinks2))
                if (gv1.label[a] == gv2.label[b]) {
                    stack.push_back(Item{a, b, 1});
                    back[a * n2 + b] = UINT64_MAX;
                }
        while (!stack.empty()) {
            const Item it = stack.back();
            stack.pop_back();
            if (it.len > max_len) { max_len = it.len; end_key = it.a * n2 + it.b; }
            const uint64_t b1 = forward ? g1.nx.begin(it.a) : gv1.prev_off[it.a], e1 = forward ? g1.nx.end(it.a) : gv1.prev_off[it.a + 1];
            const uint64_t b2 = forward ? g2.nx.begin(it.b) : gv2.prev_off[it.b], e2 = forward ? g2.nx.end(it.b) : gv2.prev_off[it.b + 1];
            const uint32_t* i1 = forward ? g1.nx.i : gv1.prev_idx;
            const uint32_t* i2 = forward ? g2.nx.i : gv2.prev_idx;
            for (uint64_t x = b1; x < e1; ++x)
                for (uint64_t y = b2; y < e2; ++y) {
                    const uint64_t na = i1[x], nb = i2[y];
                    if (gv1.label[na] == gv2.label[nb] && !back.count(na * n2 + nb)) {
                        back[na * n2 + nb] = it.a * n2 + it.b;
                        stack.push_back(Item{na, nb, it.len + 1});
                    }
                }
        }
        HostAlignment& aln = forward ? aln_fwd : aln_rev;
        while (end_key != UINT64_MAX) {
            aln.emplace_back(end_key / n2, end_key % n2);
            end_key = back.at(end_key);
        }
        if (forward) std::reverse(aln.begin(), aln.end());
    }
    size_t left_trim = 0, right_trim = 0;
    std::vector<uint64_t> path1, path2;
    bool found = false;
    if (aln_fwd.empty() || aln_rev.empty() ||
        (aln_fwd.back().first != aln_rev.front().first && aln_fwd.back().second != aln_rev.front().second)) {
        const std::vector<uint64_t> start1 = aln_fwd.empty() ? sources1 : std::vector<uint64_t>(1, aln_fwd.back().first);
        const std::vector<uint64_t> end1 = aln_rev.empty() ? sinks1 : std::vector<uint64_t>(1, aln_rev.front().first);
        if (!start1.empty() && !end1.empty()) path1 = g1.shortest(start1, end1);
        if (!path1.empty()) {
            const std::vector<uint64_t> start2 = aln_fwd.empty() ? sources2 : std::vector<uint64_t>(1, aln_fwd.back().second);
            const std::vector<uint64_t> end2 = aln_rev.empty() ? sinks2 : std::vector<uint64_t>(1, aln_rev.front().second);
            if (!start2.empty() && !end2.empty()) path2 = g2.shortest(start2, end2);
            if (!path2.empty()) {
                found = true;
                if (!aln_fwd.empty()) { path1.erase(path1.begin()); path2.erase(path2.begin()); }
                if (!aln_rev.empty()) { path1.pop_back(); path2.pop_back(); }
            }
        }
    }
    if (!found) {
        // the reference answers these questions by direct search for the first 8 and through a distance oracle afterwards
        // (alignment.hpp:1477-1497); both decide plain reachability
        auto reachable_after_trim = [&](size_t trim_left, size_t trim_right) {
            bool allow_equal = false;
            HostAlignment left, right;
            if (trim_left == aln_fwd.size()) {
                for (uint64_t a : sources1) for (uint64_t b : sources2) left.emplace_back(a, b);
                allow_equal = true;
            } else left.push_back(aln_fwd[aln_fwd.size() - 1 - trim_left]);
            if (trim_right == aln_rev.size()) {
                for (uint64_t a : sinks1) for (uint64_t b : sinks2) right.emplace_back(a, b);
                allow_equal = true;
            } else right.push_back(aln_rev[trim_right]);
            for (const auto& l : left)
                for (const auto& r : right) {
                    if (!allow_equal && (l.first == r.first || l.second == r.second)) continue;
                    if (g1.reaches(l.first, r.first) && g2.reaches(l.second, r.second)) return true;
                }
            return false;
        };
        int64_t lo = 1, hi = (int64_t)(aln_fwd.size() + aln_rev.size());
        while (lo <= hi) {
            const int64_t total = (lo + hi) / 2;
            bool success = false;
            const size_t l_min = (size_t)std::max<int64_t>(0, total - (int64_t)aln_rev.size());
            const size_t l_max = std::min<size_t>((size_t)total, aln_fwd.size());
            for (size_t l = l_min; l <= l_max; ++l)
                if (reachable_after_trim(l, (size_t)total - l)) {
                    left_trim = l;
                    right_trim = (size_t)total - l;
                    success = true;
                    break;
                }
            if (success) hi = total - 1;
            else lo = total + 1;
        }
        std::vector<uint64_t> from1, from2, to1, to2;
        if (left_trim == aln_fwd.size()) { from1 = sources1; from2 = sources2; }
        else { from1.push_back(aln_fwd[aln_fwd.size() - left_trim - 1].first); from2.push_back(aln_fwd[aln_fwd.size() - left_trim - 1].second); }
        if (right_trim == aln_rev.size()) { to1 = sinks1; to2 = sinks2; }
        else { to1.push_back(aln_rev[right_trim].first); to2.push_back(aln_rev[right_trim].second); }
        path1 = g1.shortest(from1, to1);
        path2 = g2.shortest(from2, to2);
        if (left_trim != aln_fwd.size()) { if (!path1.empty()) path1.erase(path1.begin()); if (!path2.empty()) path2.erase(path2.begin()); }
        if (right_trim != aln_rev.size()) { if (!path1.empty()) path1.pop_back(); if (!path2.empty()) path2.pop_back(); }
    }
    for (size_t i = 0; i + left_trim < aln_fwd.size(); ++i) out.push_back(aln_fwd[i]);
    for (uint64_t v : path1) out.emplace_back(v, CL_GAP);
    for (uint64_t v : path2) out.emplace_back(CL_GAP, v);
    for (size_t i = right_trim; i < aln_rev.size(); ++i) out.push_back(aln_rev[i]);
    return CL_OK;
}

// ---- the wavefront heuristics of do_alignment (stitcher.hpp:304-339), wfa_host.hpp
bool wfa_side(const GraphView& g, clwfa::Side& out) {
    if (!g.next_off) return false;   // the wavefronts expand next() lists in the reference's order
    out.n = g.n;
    out.label = g.label;
    out.next.assign(g.n, {});
    out.prev.assign(g.n, {});
    for (uint64_t v = 0; v < g.n; ++v) {
        out.next[v].assign(g.next_idx + g.next_off[v], g.next_idx + g.next_off[v + 1]);
        out.prev[v].assign(g.prev_idx + g.prev_off[v], g.prev_idx + g.prev_off[v + 1]);
    }
    out.sources.assign(g.src, g.src + g.n_src);
    out.sinks.assign(g.snk, g.snk + g.n_snk);
    NextLists nx;
    nx.build(g);
    std::vector<uint32_t> order, st, indeg;
    if (!topological_order(g, nx, order, st, indeg)) return false;
    out.order.assign(order.begin(), order.end());
    return true;
}

// every route of do_alignment that the reference runs on the host: pure deletion, greedy, deletion-WFA, pruned WFA
int host_route_alignment(int route, const GraphView& g1, const GraphView& g2, int npw, const cl_stitch_params& sp, HostAlignment& out) {
    out.clear();
    if (route == CL_ROUTE_PURE_DELETION_1 || route == CL_ROUTE_PURE_DELETION_2) {
        std::vector<uint32_t> path;
        const int rc = pure_deletion(route == CL_ROUTE_PURE_DELETION_1 ? g1 : g2, path);
        if (rc) return rc;
        for (uint32_t v : path) out.push_back(route == CL_ROUTE_PURE_DELETION_1 ? std::make_pair((uint64_t)v, (uint64_t)CL_GAP) : std::make_pair((uint64_t)CL_GAP, (uint64_t)v));
        return CL_OK;
    }
    if (route == CL_ROUTE_GREEDY_PARTIAL) {
        if (!g1.next_off || !g2.next_off) return CL_ERR_INVALID_ARGUMENT;
        return greedy_partial_alignment(g1, g2, out);
    }
    if (route != CL_ROUTE_DELETION_WFA_1 && route != CL_ROUTE_DELETION_WFA_2 && route != CL_ROUTE_PWFA) return CL_ERR_UNSUPPORTED_ROUTE;
    clwfa::Side s1, s2;
    if (!wfa_side(g1, s1) || !wfa_side(g2, s2)) return (g1.next_off && g2.next_off) ? CL_ERR_CYCLIC_GRAPH : CL_ERR_INVALID_ARGUMENT;
    const cl_align_params& ap = sp.alignment_params;
    const clwfa::WfaParams wp = clwfa::to_wfa_params(ap.match, ap.mismatch, ap.gap_open, ap.gap_extend, npw);   // the truncated parameters of subalign
    clwfa::Alignment aln;
    if (route == CL_ROUTE_PWFA) aln = clwfa::pwfa_po_poa(s1, s2, wp, (int64_t)(2 * sp.wfa_pruning_dist));
    else if (route == CL_ROUTE_DELETION_WFA_1) aln = clwfa::deletion_wfa_po_poa(s1, s2, wp);
    else {
        aln = clwfa::deletion_wfa_po_poa(s2, s1, wp);
        for (auto& pr : aln) std::swap(pr.first, pr.second);   // swap_graphs, src/alignment.cpp:41-45
    }
    out.assign(aln.begin(), aln.end());
    return CL_OK;
}

// ---- the switches of plan creation ------------------------------------------------------------------------------------------------------
constexpr uint64_t kSysLdsBytes = 159 * 1024;    // LDS a systolic-DAG workgroup may take (rings of every row + the column records)
constexpr uint64_t kRingLdsBytes = 128 * 1024;  // LDS a general-kernel workgroup may take for its anti-diagonal ring (160 KB per CU); launches are split at 64 KB

// strips of a near-chain pair that one round of popoa_lane_kernel takes = waves of its workgroup: FOUR when the pairs have the compute units to themselves, THREE in a
// plan whose other launches share them.  Measured (profiles/r05_lane_waves_ab.txt): a pair alone, or 150 pairs of 512 x 512 alone on the device, run 20 % faster in rounds
// of four (fewer rounds: 441 x 433 0.66 against 0.80 ms) — but the timed step of 10 x 1 Mbp (116 000 subproblems, sixteen launches side by side) takes 2.23-2.31 ms with
// rounds of three against 2.32-2.43 ms with four: a workgroup's waves meet at a barrier per chunk of 32 steps and run at the pace of the slowest SIMD, and with the other
// kernels' waves on the same SIMDs three are held up less than four.  The plan's size stands for "shared": 2 048 subproblems and more.  CL_LANE_WAVES=3|4 forces one
static uint32_t lane_round_waves(uint64_t n_problems) {
    const char* e = getenv("CL_LANE_WAVES");
    if (e && (*e == '3' || *e == '4')) return (uint32_t)(*e - '0');
    return n_problems >= 2048 ? 3u : 4u;
}
// two chain pairs of 17-32 rows per wave (popoa_linear_duo_kernel): alone on the device 32 x 32 pairs run at 215 instead of 130 G cells/s — but the step of 10 x 1 Mbp
// gets SLOWER with it, 1.79-1.96 against 1.54-1.65 ms (five runs each, docs/design/removed_switch_records/r05_step_spread.txt): the 17 000 such pairs cost the one-pair-per-wave launch nothing
// there (it lasts as long as its longest thin pair, 0.43 ms with or without them) and their workgroups fill idle SIMD slots beside the latency-bound launches; taken out,
// they are one launch more in the step.  So: in plans that have the device to themselves (fewer than 2 048 subproblems), as the register kernel's rounds of four.
// ... or in which such pairs are at least half of everything (a batch of them alone).  CL_LINEAR_DUOS=0|1 forces.  (-1: decided once the plan is packed)
static int duos_forced() { const char* e = getenv("CL_LINEAR_DUOS"); return e && (*e == '0' || *e == '1') ? *e - '0' : -1; }
// test hook / A-B, read at every plan creation (tests switch it inside one process): no register kernel for near-chain pairs (popoa_lane_kernel) — the pairs then take
// the kernels of rounds 1-4 (systolic, strips, rings), which stay the route of everything that is not a near-chain pair
static bool no_lane_now() { const char* e = getenv("CL_NO_LANE"); return e && *e == '1'; }

// what packing a subproblem and choosing its kernel read from the environment, once per plan (what each means: at the function that uses it)
struct PackSwitches {
    int rank_order = 0;                // CL_RANK_ORDER (choose_rank_order)
    uint32_t lane_rw = 4;              // CL_LANE_WAVES (lane_round_waves)
    int duos = -1;                     // CL_LINEAR_DUOS (duos_forced)
    bool no_lane = false;              // CL_NO_LANE
    // test hooks, read at every plan creation like CL_NO_LANE (tests switch them inside one process; bench.py sets CL_NO_STRIP in a child's environment)
    bool force_general = false;        // CL_FORCE_GENERAL: chain x chain and near-chain pairs go to the DAG kernels too (choose_chain, choose_lane, fit_strips)
    bool no_sys = false;               // CL_NO_SYS: no systolic DAG kernel (choose_sys)
    bool no_strip = false;             // CL_NO_STRIP: no strips of rows for large pairs, popoa_strip_kernel (choose_chain, choose_lane, fit_strips)
    bool no_ring = false;              // CL_NO_RING: HBM-plane general kernel only (choose_ring)
    bool span = true;                  // CL_LINEAR_SPAN (choose_chain)
    bool lane_wide = false;            // CL_LANE_WIDE (choose_lane)
    uint64_t lane_max_rows = 1024, lane_min_sweep = 512;   // CL_LANE_MAX_ROWS, CL_LANE_MIN_SWEEP (choose_lane)
    uint64_t strip_rows = 0;           // CL_STRIP_ROWS (fit_strips), once per process
};
PackSwitches read_pack_switches(uint64_t n_problems) {
    PackSwitches sw;
    sw.rank_order = rank_order_now();
    sw.lane_rw = lane_round_waves(n_problems);
    sw.duos = duos_forced();
    sw.no_lane = no_lane_now();
    auto is_one = [](const char* e) { return e && *e == '1'; };
    sw.force_general = is_one(getenv("CL_FORCE_GENERAL"));
    sw.no_sys = is_one(getenv("CL_NO_SYS"));
    sw.no_strip = is_one(getenv("CL_NO_STRIP"));
    sw.no_ring = is_one(getenv("CL_NO_RING"));
    sw.span = [] { const char* e = getenv("CL_LINEAR_SPAN"); return !e || e[0] != '0'; }();   // (read per plan: the tests of the older routes switch it)
    sw.lane_wide = [] { const char* e = getenv("CL_LANE_WIDE"); return e && *e == '1'; }();
    sw.lane_max_rows = [] { const char* e = getenv("CL_LANE_MAX_ROWS"); const long v = e ? atol(e) : 1024; return (uint64_t)(v < 1 ? 1 : v > 1024 ? 1024 : v); }();
    sw.lane_min_sweep = [] { const char* e = getenv("CL_LANE_MIN_SWEEP"); return e ? (uint64_t)atoll(e) : (uint64_t)512; }();   // (read per plan: tests)
    static const uint64_t rows_env = [] { const char* e = getenv("CL_STRIP_ROWS"); const long v = e ? atol(e) : 0; return (uint64_t)(v >= 64 && v <= 768 ? v / 64 * 64 : 0); }();
    sw.strip_rows = rows_env;
    return sw;
}

// ---- packing one subproblem into rank space ------------------------------------------------------------------------------------------------
// host-side packing into rank space.  The subproblems are independent: chunks of them are packed side by side into parts of their own
// (offsets relative to the part) and the parts are appended in order, which gives exactly the arrays of a serial pass
struct PackPart {
    std::vector<uint8_t> lab[2];
    std::vector<uint32_t> poff[2], pidx[2], snk[2], order[2];
    std::vector<uint32_t> ring_need;   // per PO-POA problem: dynamic LDS of the ring / systolic variant (0 = not taken)
    std::vector<uint32_t> sys_aux;     // saved-column lists of the systolic kernel's problems, concatenated
    std::vector<ClStripDesc> strips;   // strip kernel: prob = index into desc of this part; rec_base / hand_* / prog relative to this part
    std::vector<uint4> strip_recs;
    std::vector<uint32_t> strip_lds;   // per strip: dynamic LDS
    uint64_t hand_words = 0;
    std::vector<ClProbDesc> desc;
    std::vector<uint64_t> po_problem;
    std::vector<uint32_t> pd_problem, host_problem;
    std::vector<ChainShape> chain_shape;
    uint64_t plane_cursor = 0, out_cursor = 0, dp_cells = 0, dp_bytes = 0, max_cells = 0, n_linear = 0;
    int rc = CL_OK;
    std::string err;
    PackPart() { poff[0].push_back(0); poff[1].push_back(0); }
    void fail(int code, const char* fmt, ...) {
        if (rc) return;
        rc = code;
        char buf[512];
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(buf, sizeof(buf), fmt, ap);
        va_end(ap);
        err = buf;
    }
};
struct Scratch { std::vector<uint32_t> order, st, indeg, rank; };

// what every subproblem of a plan is packed with
struct PackInput {
    const cl_stitch_batch* batch;
    const cl_stitch_params* params;
    const uint8_t* force_num_pw;   // may be null
    uint64_t n;                    // subproblems of the plan: 2 048 and more stand for "its launches share the device"
    PackSwitches sw;
};

// One PO-POA pair as it lies in its part's rank-space arrays: node j (1-based rank) of side s has the predecessors pidx[s][off[s][j - 1] .. off[s][j]) (ranks + 1) and
// the label lab[s][j - 1] (bit 7: a source, which reads the boundary index 0).  What the kernel choices below look at.
struct PairView {
    const uint32_t* off[2];
    const uint8_t* lab[2];
    const uint32_t* pidx[2];
    uint32_t n1 = 0, n2 = 0;
    int npw = 1;
    uint64_t cells = 0, n_pred = 0;
    uint64_t span[2] = {0, 0};   // how many rows (columns) back the cells of a row (column) read: predecessors, boundary for a source
    int sRow = 0, sCol = 1;      // rows = the shorter graph
    uint64_t n_rows = 0, n_cols = 0;   // (rows: + 1 for the boundary row)
    uint64_t nodes(int s) const { return s == 0 ? n1 : n2; }
};

// What a kernel family answers for a pair: whether it takes it, and then what the pair's descriptor and the part's arrays get.
struct KernelChoice {
    bool taken = false;
    uint64_t lds = 0;                // dynamic LDS of the pair's workgroup (PackPart::ring_need)
    uint16_t pad = 0;                // ClProbDesc::pad
    uint32_t aux_cnt = 0;            // ClProbDesc::aux_cnt
    std::vector<uint32_t> aux;       // the words it appends to the part's aux array (ClProbDesc::aux_base = where they start)
    uint64_t extra_plane_words = 0;  // workspace behind the pair's score planes
};

// one side of a subproblem: topological order, the rank order of choice, then labels, predecessor lists and sinks in rank space appended to the part.
// `linear` stays true while the side is a chain from its one source (rank 0) to its one sink (the last rank)
bool pack_side(const GraphView& g, int s, uint64_t k, int rank_order, PackPart& P, Scratch& S, ClProbDesc& d, uint64_t& span, bool& linear) {
    std::vector<uint32_t>& order = S.order; std::vector<uint32_t>& rank = S.rank;
    NextLists nx;
    nx.build(g);
    if (!topological_order(g, nx, order, S.st, S.indeg)) { P.fail(CL_ERR_CYCLIC_GRAPH, "problem %llu: graph %d is not acyclic", (unsigned long long)k, s + 1); return false; }
    rank.resize(g.n);
    for (uint32_t r = 0; r < g.n; ++r) rank[order[r]] = r;
    choose_rank_order(g, rank_order, order, rank, S.st, S.indeg);
    if (P.lab[s].size() + g.n >= (1ull << 32) || P.pidx[s].size() + (g.prev_off[g.n] - g.prev_off[0]) >= (1ull << 32)) { P.fail(CL_ERR_INVALID_ARGUMENT, "batch too large for 32-bit device offsets"); return false; }
    d.node_base[s] = (uint32_t)P.lab[s].size();
    size_t lab0 = P.lab[s].size();
    for (uint32_t r = 0; r < g.n; ++r) {
        uint32_t v = order[r];
        P.lab[s].push_back(g.label[v] & 0x7f);
        uint64_t deg = g.prev_off[v + 1] - g.prev_off[v];
        for (uint64_t e = g.prev_off[v]; e < g.prev_off[v + 1]; ++e) {
            P.pidx[s].push_back(rank[g.prev_idx[e]] + 1);
            span = std::max<uint64_t>(span, r - rank[g.prev_idx[e]]);
        }
        P.poff[s].push_back((uint32_t)P.pidx[s].size());
        if (r == 0 ? deg != 0 : (deg != 1 || rank[g.prev_idx[g.prev_off[v]]] != r - 1)) linear = false;
        if (g.label[v] & 0x80) { P.fail(CL_ERR_INVALID_ARGUMENT, "labels must be < 128"); return false; }
    }
    for (uint64_t i = 0; i < g.n_src; ++i) {
        P.lab[s][lab0 + rank[g.src[i]]] |= 0x80;
        span = std::max<uint64_t>(span, (uint64_t)rank[g.src[i]] + 1);   // a source reads the boundary index 0
    }
    if (g.n_src != 1 || rank[g.src[0]] != 0) linear = false;
    if (g.n_snk != 1 || rank[g.snk[0]] != g.n - 1) linear = false;
    d.snk_base[s] = (uint32_t)P.snk[s].size();
    d.snk_cnt[s] = (uint32_t)g.n_snk;
    for (uint64_t i = 0; i < g.n_snk; ++i) P.snk[s].push_back(rank[g.snk[i]] + 1);
    P.order[s].insert(P.order[s].end(), order.begin(), order.end());
    return true;
}

// ---- which kernel takes a pair ---------------------------------------------------------------------------------------------------------------
// The chain kernels (popoa_linear.hip) take a pair of two chains; which of them, by the shorter chain's rows (it goes across the lanes; strips of 64 rows are
// pipelined over the waves).
// (a chain pair of 4 096 rows and more would take the chain kernel's ONE workgroup through four and more passes: the strip kernel puts it on
// twenty compute units instead — 6 300 x 6 300: 22.4 -> ≈ 12 ms; such a pair always meets the strip kernel's conditions)
// round 6: chain pairs of more than 1 024 rows span SEVERAL workgroups (popoa_linear_span_kernel, popoa_linear.hip: groups of four strips on different compute units, one
// round): 2 048 x 2 048 and 6 300 x 6 300 leave the sixteen-wave workgroup's rounds / the DAG strip kernel.  CL_LINEAR_SPAN=0: the routing of rounds 4-5 (A/B)
// waves of popoa_linear_kernel's workgroup (rounds of W strips): four for chain pairs of 65-256 rows, eight up to 512 rows, sixteen above (what other counts
// measured: docs/design/stitch_kernels.md, "tried and removed")
struct ChainChoice {
    bool taken = false;
    ChainShape shape;
    uint8_t rows_per_lane = 0;
    bool swap = false;     // graph 2 laid across the lanes
    uint16_t pad = 0;      // read by linear_dispatch
};
ChainChoice choose_chain(uint32_t n1, uint32_t n2, bool linear, const PackInput& in) {
    const PackSwitches& sw = in.sw;
    ChainChoice c;
    const uint32_t nshort = std::min(n1, n2), nlong = std::max(n1, n2);
    const bool span_linear = sw.span && linear && !sw.force_general && nshort > 1024 && nshort <= 40000;
    const bool big_linear = !span_linear && linear && !sw.no_strip && !sw.force_general && nshort >= 4096 && nshort <= 40000;
    c.taken = linear && !sw.force_general && !big_linear;
    if (!c.taken) return c;
    c.swap = n2 < n1;
    c.rows_per_lane = 1;
    const bool no_duos = sw.duos == 0;   // (whether the plan takes the duo kernel at all is decided when every pair is known: decide_duos)
    if (span_linear) c.shape = {LaunchVariant::ChainSpan, 0};   // (the pair's strips over several workgroups)
    else if (nshort <= 16) c.shape = {LaunchVariant::Quads, 0};   // (FOUR pairs per wave, 16 lanes each — popoa_linear_quad_kernel)
    else if (nshort <= 32 && !no_duos) c.shape = {LaunchVariant::Duos, 0};   // (TWO pairs per wave, 32 lanes each — popoa_linear_duo_kernel; see duos_forced)
    else if (nshort <= 64) c.shape = {LaunchVariant::Chain, 1};
    else if (nshort <= 128 && nlong < 300) { c.rows_per_lane = 2; c.shape = {LaunchVariant::Chain, 1}; }
    else if (nshort <= 256) c.shape = {LaunchVariant::Chain, 4};
    else c.shape = {LaunchVariant::Chain, (uint8_t)((nshort <= 512 || in.n >= 2048) ? 8 : 16)};   // (up to eight strips: eight waves — with sixteen, half of them only stand at the barriers; above, sixteen only in plans that have the device to themselves: the one such pair of the 10 x 1 Mbp step as a launch of its own costs the step 3 %, 1.61 against 1.56 ms, three runs each)
    c.pad = (uint16_t)((c.swap ? 1 : 0) | (c.rows_per_lane << 1));
    return c;
}

// The saved-column search of the systolic kernel and of the strips.  A column's predecessors (a source's boundary column 0 included) that lie at most `limit`
// columns back are served by a ring of recent columns per row, the others are SAVED columns with LDS of their own: the near limit decides the ring depth
// (2^log columns: the row side's span + the farthest near distance + 1) against the number of saved columns.  Of the candidate limits the one with the smallest
// footprint wins — LDS is what bounds how many subproblems a CU holds at once.  footprint(log, saved columns) -> bytes.
struct SavedColumns {
    uint64_t bytes = UINT64_MAX;   // the winner's footprint; UINT64_MAX: no candidate stayed within max_cols (and max_log)
    uint64_t limit = 0, near_max = 0;
    uint32_t log = 0;
    std::vector<uint32_t> cols;    // ascending
};
template <class Footprint>
SavedColumns search_saved_columns(const PairView& V, int sC, uint64_t row_span, const uint64_t* limits, size_t n_limits, size_t max_cols, uint32_t min_log, uint32_t max_log, Footprint footprint) {
    const uint32_t* cp = V.off[sC];
    const uint8_t* cl = V.lab[sC];
    const uint64_t n_cols = V.nodes(sC);
    SavedColumns best;
    std::vector<uint32_t> cand;
    for (size_t li = 0; li < n_limits; ++li) {
        const uint64_t limit = limits[li];
        cand.clear();
        uint64_t nm = 0;
        for (uint64_t j = 1; j <= n_cols; ++j) {
            for (uint32_t e = cp[j - 1]; e < cp[j]; ++e) {
                const uint64_t dist = j - V.pidx[sC][e];
                if (dist > limit) cand.push_back(V.pidx[sC][e]); else nm = std::max(nm, dist);
            }
            if (cl[j - 1] & 0x80) { if (j > limit) cand.push_back(0); else nm = std::max(nm, j); }
        }
        std::sort(cand.begin(), cand.end());
        cand.erase(std::unique(cand.begin(), cand.end()), cand.end());
        if (cand.size() > max_cols) continue;
        uint32_t lg = min_log;
        while ((1ull << lg) < row_span + nm + 1 && lg < 14) ++lg;
        if (lg > max_log) break;   // (a larger limit only deepens the ring)
        const uint64_t bytes = footprint(lg, cand.size());
        if (bytes < best.bytes) { best.bytes = bytes; best.limit = limit; best.near_max = nm; best.log = lg; best.cols = cand; }
        if (cand.empty()) break;   // a larger limit only deepens the ring
    }
    return best;
}

// near-chain pairs in registers (popoa_lane_kernel, popoa_lane.h): every node one to four predecessors (a source's boundary index counted), the row
// graph's within 4 ranks, the column graph's within 4 columns or in at most sixteen SAVED columns (two per column at most); rows = the shorter graph.
// Two shapes of the cell: predecessors up to 2 rows / 3 columns back, or 4 / 4
// Which workgroup shapes (measured on one pair alone, profiles/r05_lane_probe.txt and DESIGN.md §4.3): one, two or three ACTIVE waves of a workgroup run a
// step in 0.24 / 0.30 / 0.30 us, four in 0.55 us, eight in 0.93 us; strips dealt to several workgroups (WIDE: groups of three strips, progress words between
// them) pay ~14 us per chunk of 32 steps for the hand-off across compute units (write-through stores against a 64-deep store queue, reads past the caches).
// Inside the timed step of 10 x 1 Mbp (sixteen launches side by side, three runs each): register kernel for pairs up to 192 rows 2.49-2.58 ms, up to 512 or
// 1 024 rows (further rounds of four waves) 2.30-2.35 ms, not at all 2.57 ms — so the default is 1 024 rows (CL_LANE_MAX_ROWS), in one workgroup.
// CL_LANE_WIDE=1 deals pairs above 192 rows to several workgroups (up to 128 groups): parity-tested (tests/test_gpu_parity.py), slower than the strips
// on 5 500 x 5 500 (16.6 against 12.7 ms), off by default
// which pairs: the register kernel wins where a launch lasts as long as its longest sweep (alone on the device: 2 225 x 165 0.88 ms against 1.32 ms on the systolic
// kernel, 2 130 x 35 0.83 against 1.17, 441 x 433 0.60 against 0.71); on the thousands of small pairs that fill a launch's workgroups it issues about as many
// instructions per cell as the systolic kernel and its launches, dealt by (waves, long / short), interleave worse: pairs below CL_LANE_MIN_SWEEP rows + columns
// (default 512) stay where they were
KernelChoice choose_lane(const PairView& V, const PackSwitches& sw) {
    KernelChoice c;
    const uint64_t n_rows = V.n_rows, n_cols = V.n_cols;
    const int sRow = V.sRow, sCol = V.sCol, npw = V.npw;
    const bool lane_wide = sw.lane_wide && n_rows > 193;
    const uint64_t lane_groups = lane_wide ? ((n_rows - 1 + 63) / 64 + 2) / 3 : 1;
    if (sw.no_lane || sw.force_general || lane_groups > 128 || !(lane_wide || n_rows - 1 <= sw.lane_max_rows) || (lane_wide && sw.no_strip) || n_cols >= (1u << 28) || n_rows - 1 + n_cols < sw.lane_min_sweep) return c;
    const uint32_t nR = (uint32_t)n_rows - 1, nCl = (uint32_t)n_cols;
    const uint32_t* rp = V.off[sRow];
    const uint8_t* rl = V.lab[sRow];
    const uint32_t* cp = V.off[sCol];
    const uint8_t* cl = V.lab[sCol];
    uint32_t max_rd = 0;
    bool ok = true;
    for (uint32_t i = 1; i <= nR && ok; ++i) {
        if (rp[i] - rp[i - 1] + (rl[i - 1] >> 7) == 0) ok = false;
        for (uint32_t e = rp[i - 1]; e < rp[i]; ++e) max_rd = std::max(max_rd, i - V.pidx[sRow][e]);
    }
    ok = ok && max_rd <= 4;
    bool take_lane = false;
    uint32_t lane_dr = 0, lane_dc = 0, lane_slots = 0;
    uint64_t lane_lds = 0;
    std::vector<uint32_t>& lane_words = c.aux;
    for (int shape = max_rd <= 2 ? 0 : 1; shape < 2 && ok && !take_lane; ++shape) {
        const uint32_t near = 3u;   // (the lane's history rings hold the last three columns; further back = a saved column)
        std::vector<uint32_t> far;
        uint32_t max_cd = 0;
        bool fits = true;
        for (uint32_t j = 1; j <= nCl && fits; ++j) {
            uint32_t nf = 0;
            if (cp[j] - cp[j - 1] + (cl[j - 1] >> 7) == 0) fits = false;
            for (uint32_t e = cp[j - 1]; e < cp[j]; ++e) {
                const uint32_t dist = j - V.pidx[sCol][e];
                if (dist > near) { far.push_back(V.pidx[sCol][e]); ++nf; } else max_cd = std::max(max_cd, dist);
            }
            if (nf > 2) fits = false;
        }
        std::sort(far.begin(), far.end());
        far.erase(std::unique(far.begin(), far.end()), far.end());
        lane_dr = shape == 0 ? 2 : 4; lane_dc = near; lane_slots = (uint32_t)far.size();
        // LDS of a workgroup: the hand-off window between neighbouring strips ([waves - 1][DR][1 + NumPW][128 columns]) + the saved columns
        const uint64_t lane_w = n_rows - 1 <= 64 ? 1 : sw.lane_rw;
        lane_lds = (lane_w > 1 ? (lane_w - 1) * lane_dr * (1 + npw) * 128 * 4 : 0) + (uint64_t)lane_slots * (lane_dr + (lane_wide ? 192 : n_rows - 1) + 1) * (1 + npw) * 4;
        if (!fits || far.size() > 16 || lane_lds > 150 * 1024) continue;
        take_lane = true;
        // shortest walk from a source, in nodes (the boundary cells' closed form)
        lane_words.assign(1 + 2ull * nR + 2ull * nCl, 0u);   // [0]: a wide pair's first progress word (set when the launch groups are made)
        uint32_t* rowrec = lane_words.data() + 1, *rowdist = rowrec + nR, *colrec = rowdist + nR, *coldist = colrec + nCl;
        for (uint32_t i = 1; i <= nR; ++i) {
            uint32_t mask = 0, best = (rl[i - 1] >> 7) ? 1u : UINT32_MAX;
            for (uint32_t e = rp[i - 1]; e < rp[i]; ++e) {
                const uint32_t pr = V.pidx[sRow][e];
                mask |= 1u << (i - pr - 1);
                best = std::min(best, rowdist[pr - 1] == UINT32_MAX ? UINT32_MAX : rowdist[pr - 1] + 1);
            }
            rowdist[i - 1] = best;
            rowrec[i - 1] = mask | ((uint32_t)(rl[i - 1] >> 7) << 4) | ((uint32_t)(rl[i - 1] & 0x7Fu) << 8);
            if (best == UINT32_MAX) take_lane = false;   // (not reachable from a source: never in an extracted subgraph)
        }
        for (uint32_t j = 1; j <= nCl; ++j) {
            uint32_t mask = 0, nf = 0, slots = 0, best = (cl[j - 1] >> 7) ? 1u : UINT32_MAX;
            for (uint32_t e = cp[j - 1]; e < cp[j]; ++e) {
                const uint32_t q = V.pidx[sCol][e];
                if (j - q <= near) mask |= 1u << (j - q - 1);
                else { slots |= (uint32_t)(std::lower_bound(far.begin(), far.end(), q) - far.begin()) << (20 + 4 * nf); ++nf; }
                best = std::min(best, coldist[q - 1] == UINT32_MAX ? UINT32_MAX : coldist[q - 1] + 1);
            }
            coldist[j - 1] = best;
            const auto self = std::lower_bound(far.begin(), far.end(), j);
            const uint32_t keep = self != far.end() && *self == j ? (1u << 15) | ((uint32_t)(self - far.begin()) << 16) : 0u;
            colrec[j - 1] = mask | ((uint32_t)(cl[j - 1] >> 7) << 4) | (nf << 5) | ((uint32_t)(cl[j - 1] & 0x7Fu) << 8) | keep | slots;
            if (best == UINT32_MAX) take_lane = false;
        }
        if (!take_lane) break;
    }
    if (!take_lane) { c.aux.clear(); return c; }
    c.taken = true;
    c.lds = lane_lds;
    c.pad = (uint16_t)(lane_dr | (lane_dc << 4) | ((uint32_t)(lane_groups - 1) << 8) | (V.n2 < V.n1 ? 0x8000u : 0u));   // DR | DC << 4 | groups - 1 << 8 | rows = graph 2
    c.aux_cnt = lane_slots;   // (aux: sync | rowrec | rowdist | colrec | coldist, popoa_lane.h)
    // the hand-off rows between the strips of 64 rows lie behind the planes: [strips - 1][DR][1 + NumPW][columns]; behind them, for a wide pair, the
    // saved-column cells a group hands to the next: [groups][saved columns][DR]
    const uint64_t n_strips = (n_rows - 1 + 63) / 64;
    c.extra_plane_words = ((n_strips - 1) * lane_dr * (1 + npw) * n_cols + (lane_groups > 1 ? lane_groups * lane_slots * lane_dr : 0) + 3) / 4 * 4;
    return c;
}

// the systolic kernel (popoa_sys_kernel): the shorter graph's rows on the threads, a ring of H columns per row in LDS.  H must
// exceed the row graph's predecessor span plus the column graph's NEAR predecessor distances; columns that are read from
// further away (the fork in front of a long bubble; column 0 for a late source) are SAVED columns with LDS of their own
KernelChoice choose_sys(const PairView& V, const PackSwitches& sw) {
    KernelChoice c;
    if (sw.no_sys || V.n_rows > 1024) return c;
    const uint64_t n_rows = V.n_rows, n_cols = V.n_cols, n_pred = V.n_pred;
    const uint32_t* cp = V.off[V.sCol];   // node j (1-based rank): predecessors pidx[cp[j - 1] .. cp[j])
    uint64_t max_deg = 0;
    for (uint64_t j = 1; j <= n_cols; ++j) max_deg = std::max<uint64_t>(max_deg, cp[j] - cp[j - 1]);
    // the near limit decides the ring depth H (LDS per row) against the number of saved columns (LDS per column)
    const uint64_t cw = V.npw == 1 ? 4 : 8;
    const uint64_t candidates[7] = {2, 4, 8, 32, 128, 512, 2047};   // the kernel's column records hold a near distance in 11 bits
    SavedColumns sc = search_saved_columns(V, V.sCol, V.span[V.sRow], candidates, 7, 32, 0, 14, [&](uint32_t lg, uint64_t n_saved) {
        const uint64_t hw = (1ull << lg) * cw, stride = hw + (cw == 8 ? 4 : 8);   // popoa_sys_kernel's row stride
        return n_rows * stride * 4 + n_saved * n_rows * cw * 4 + n_cols * 8 + n_pred * 4 + n_saved * 4 + 16;
    });
    c.taken = sc.bytes != UINT64_MAX && (1ull << sc.log) >= V.span[V.sRow] + sc.near_max + 1 && sc.bytes <= kSysLdsBytes &&
              max_deg <= 63 && cp[n_cols] - cp[0] < (1u << 17);   // field widths of the column records
    if (!c.taken) return c;
    c.lds = sc.bytes;
    c.pad = (uint16_t)(sc.log | (V.n2 < V.n1 ? 0x8000u : 0u));   // log2 H | rows = graph 2
    c.aux_cnt = (uint32_t)sc.cols.size();
    c.aux.push_back((uint32_t)sc.limit);   // {near limit, the saved columns ascending}
    c.aux.insert(c.aux.end(), sc.cols.begin(), sc.cols.end());
    return c;
}

// strips of rows (popoa_strip_kernel): pairs too large for one workgroup's LDS, one workgroup per strip of S rows, all strips of the pair in
// flight at once.  Taken when the column predecessors (a source's boundary column included) lie inside a ring of at most 64 columns but for at
// most eight SAVED columns, the row graph's predecessors within 32 rows (they become the next strip's ghost rows) and the pair is large enough
struct StripFit {
    bool ok = false;
    int rows_side = 0;          // which graph's nodes are the rows
    uint32_t log = 0, S = 0, n = 0, ghost = 0, limit = 0;   // ring depth, rows per strip, strips, ghost rows, near limit
    uint64_t row_bytes = 0;     // LDS per row: its ring and its saved-column slots
    std::vector<uint32_t> far;  // the saved columns, ascending
};
StripFit fit_strips(const PairView& V, int sR, const PackSwitches& sw) {
    StripFit f;
    f.rows_side = sR;
    const int sC = 1 - sR;
    const uint64_t nRw = V.nodes(sR) + 1ull, nCl = V.nodes(sC);
    if (sw.no_strip || sw.force_general || nRw < 192 || V.cells < 100000 || nCl >= (1u << 28)) return f;
    const uint32_t* cp = V.off[sC];
    const uint32_t* rp = V.off[sR];
    uint64_t max_deg = 0, gd = 0;
    for (uint64_t j = 1; j <= nCl; ++j) max_deg = std::max<uint64_t>(max_deg, cp[j] - cp[j - 1]);
    for (uint64_t i = 1; i < nRw; ++i)
        for (uint32_t e = rp[i - 1]; e < rp[i]; ++e) gd = std::max<uint64_t>(gd, i - V.pidx[sR][e]);
    // the near limit decides the ring depth (LDS per row) against the number of saved columns (LDS per row as well: a slot each): the candidate with
    // the smallest footprint per row wins, as for the systolic kernel
    const uint64_t cw = V.npw == 1 ? 4 : 8;
    const uint64_t limits[6] = {2, 4, 8, 16, 32, 62};
    SavedColumns sc = search_saved_columns(V, sC, V.span[sR], limits, 6, 8, 1, 6, [&](uint32_t lg, uint64_t n_saved) {
        return ((1ull << lg) * cw + (cw == 8 ? 4 : 8)) * 4 + n_saved * cw * 4;
    });
    if (sc.bytes == UINT64_MAX || V.span[sR] > 32 || gd > 32 || max_deg > 63) return f;
    const uint64_t row_bytes = sc.bytes;
    // the largest S (a multiple of 64, at most 768: 1 024 threads less the four ghost waves) whose rings and row lists fit
    auto rec_ring_log = [&](uint64_t n_loc) { uint32_t l = 5; while ((1ull << l) < n_loc + 48) ++l; return l; };   // popoa_strip_kernel's record ring
    auto strip_bytes = [&](uint64_t S) {
        uint64_t worst = 0;
        for (uint64_t a = 0; a < nRw; a += S) {
            const uint64_t hi = std::min(nRw - 1, a + S - 1), lo = std::max<uint64_t>(a, 1);
            const uint64_t edges = hi >= lo ? rp[hi] - rp[lo - 1] : 0, n_loc = (a ? gd : 0) + std::min(S, nRw - a);
            worst = std::max<uint64_t>(worst, n_loc * row_bytes + ((uint64_t)16 << rec_ring_log(n_loc)) + edges * 4 + 64);
        }
        return worst;
    };
    // CL_STRIP_ROWS=64..768 caps the rows per strip (measurements)
    uint64_t S = sw.strip_rows ? sw.strip_rows : 256;   // (measured: a pair's duration hardly depends on the rows per strip between 64 and 768 — a step is a latency chain, not throughput — so strips are kept small: more of them run side by side and each leaves LDS for its neighbours)
    while (S >= 64 && strip_bytes(S) > kSysLdsBytes) S -= 64;
    if (S < 64) return f;
    const uint64_t n = (nRw + S - 1) / S;
    const uint64_t even = ((nRw + n - 1) / n + 63) / 64 * 64;   // the rows dealt evenly
    if (even <= S && strip_bytes(even) <= kSysLdsBytes) S = even;
    f.S = (uint32_t)S; f.n = (uint32_t)((nRw + S - 1) / S); f.ghost = (uint32_t)gd; f.log = sc.log; f.limit = (uint32_t)sc.limit;
    f.row_bytes = row_bytes;
    f.far.swap(sc.cols);
    f.ok = f.n <= 200;   // (all strips of a pair must be resident together: one workgroup per compute unit)
    return f;
}
// the column records of a pair the strips take (one uint4 per column), appended to the part
void append_strip_records(const PairView& V, const StripFit& f, PackPart& P) {
    const int sC = 1 - f.rows_side;
    const uint64_t nCl = V.nodes(sC);
    const uint32_t* cp = V.off[sC];
    const uint8_t* cl = V.lab[sC];
    for (uint64_t j = 1; j <= nCl; ++j) {
        const uint32_t b0 = cp[j - 1], deg = cp[j] - cp[j - 1], l = cl[j - 1], src = l >> 7, nq = deg + src;
        // a predecessor column as a code: that many columns back (below 0x80: inside the ring), or 0x80 | its slot among the saved columns
        auto code = [&](uint32_t q) -> uint32_t {
            if ((uint32_t)j - q <= f.limit) return (uint32_t)j - q;
            return 0x80u | (uint32_t)(std::lower_bound(f.far.begin(), f.far.end(), q) - f.far.begin());
        };
        uint32_t x = 0;
        if (nq >= 1 && nq <= 3) {   // the straight-line cell's three predecessors (8 bits each)
            uint32_t q[3], nl = 0;
            for (uint32_t e = 0; e < deg; ++e) q[nl++] = V.pidx[sC][b0 + e];
            if (src) q[nl++] = 0u;
            for (; nl < 3; ++nl) q[nl] = q[0];
            x = code(q[0]) | (code(q[1]) << 8) | (code(q[2]) << 16);
        }
        // the general cell's predecessor list rides along as distances (z: first two, w: next two, x — free when the straight-line
        // cell does not apply — the fifth and sixth); longer lists are read from HBM
        const bool fast = nq >= 1 && nq <= 3, inl = deg <= 6;
        uint32_t dist[6] = {0, 0, 0, 0, 0, 0};
        for (uint32_t e = 0; e < deg && e < 6; ++e) dist[e] = code(V.pidx[sC][b0 + e]);
        if (!fast && inl) x = dist[4] | (dist[5] << 12);
        // bit 15: this column is itself a saved one, bits 12-14: in that slot
        const auto self = std::lower_bound(f.far.begin(), f.far.end(), (uint32_t)j);
        const uint32_t keep = self != f.far.end() && *self == (uint32_t)j ? 0x8000u | ((uint32_t)(self - f.far.begin()) << 12) : 0u;
        P.strip_recs.push_back(make_uint4(x, keep | (inl ? 1u << 16 : 0u) | (deg << 17) | (fast ? 1u << 23 : 0u) | ((l & 0x7Fu) << 24) | (src << 31),
                                          dist[0] | (dist[1] << 12), dist[2] | (dist[3] << 12)));
    }
}
// the strips' descriptors, their LDS and the pair's hand-off words, appended to the part (rec_base: where the pair's column records start)
void append_strip_descs(const PairView& V, const StripFit& f, uint32_t rec_base, PackPart& P) {
    const int sR = f.rows_side;
    const uint64_t nRw = V.nodes(sR) + 1ull, nCl = V.nodes(1 - sR), cw = V.npw == 1 ? 4 : 8;
    const uint32_t* rp = V.off[sR];
    const uint64_t hand_per = (uint64_t)f.ghost * (nCl + 1) * (cw / 2);
    for (uint32_t j = 0; j < f.n; ++j) {
        ClStripDesc sd{};
        const uint64_t a = (uint64_t)j * f.S;
        sd.prob = (uint32_t)P.desc.size();
        sd.n_ghost = j ? f.ghost : 0;
        sd.row_base = (uint32_t)(a - sd.n_ghost);
        sd.n_real = (uint32_t)std::min<uint64_t>(f.S, nRw - a);
        sd.n_out = j + 1 < f.n ? f.ghost : 0;
        sd.rec_base = rec_base;
        sd.hand_in = P.hand_words + (j ? (uint64_t)(j - 1) * hand_per : 0);
        sd.hand_out = P.hand_words + (uint64_t)j * hand_per;
        sd.prog = (uint32_t)P.strips.size();
        sd.strip = j; sd.n_strips = f.n; sd.logH = f.log;
        uint32_t lrw = 5;
        while ((1ull << lrw) < (uint64_t)sd.n_ghost + sd.n_real + 48) ++lrw;
        sd.logRW = lrw;
        const uint64_t hi = std::min<uint64_t>(nRw - 1, a + f.S - 1), lo = std::max<uint64_t>(a, 1);
        P.strip_lds.push_back((uint32_t)(((uint64_t)sd.n_ghost + sd.n_real) * f.row_bytes + (16ull << lrw) + (hi >= lo ? rp[hi] - rp[lo - 1] : 0) * 4 + 64));
        P.strips.push_back(sd);
    }
    P.hand_words += (uint64_t)(f.n - 1) * hand_per;
}
// rows = the shorter graph; if ITS predecessors reach too far back for ghost rows (a long bubble) and the longer graph's do not, rows = the longer one
KernelChoice choose_strip(const PairView& V, const PackSwitches& sw, PackPart& P) {
    KernelChoice c;
    StripFit f = fit_strips(V, V.sRow, sw);
    if (!f.ok) f = fit_strips(V, V.sCol, sw);
    if (!f.ok) return c;
    const uint32_t rec_base = (uint32_t)P.strip_recs.size();
    append_strip_records(V, f, P);
    append_strip_descs(V, f, rec_base, P);
    c.taken = true;   // (lds 0: a strip launch's LDS is that of its hungriest strip, PackPart::strip_lds)
    c.pad = (uint16_t)(f.log | (f.rows_side == 1 ? 0x8000u : 0u));   // bit 15: the rows are graph 2
    c.aux_cnt = (uint32_t)f.far.size();
    c.aux.push_back(f.limit);   // {near limit, the saved columns ascending}, as for the systolic kernel
    c.aux.insert(c.aux.end(), f.far.begin(), f.far.end());
    return c;
}

// LDS ring of the most recent anti-diagonals (popoa_kernels.hip): span1+span2+1 of them serve every read; when that
// does not fit, as many as do (at least 8) — the rare reads that reach further back go to HBM.  Not taken: the general kernel with its planes in HBM
KernelChoice choose_ring(const PairView& V, const PackSwitches& sw) {
    KernelChoice c;
    const uint64_t width = std::min(V.n1, V.n2) + 1, per_diag = width * (uint64_t)(1 + 2 * V.npw) * 4;
    // the ring variant also stages the subproblem's topology in LDS: offsets, predecessor ranks, labels
    const uint64_t topo_bytes = ((uint64_t)V.n1 + V.n2) * 8 + V.n_pred * 4 + ((uint64_t)V.n1 + V.n2 + 2) * (1 + V.npw) * 4 + 16;   // node records, lists, boundaries
    uint64_t depth = 1;   // a power of two (the kernel masks instead of dividing): enough for every read, or all that fits
    while (depth < V.span[0] + V.span[1] + 1 && 2 * depth * per_diag + topo_bytes <= kRingLdsBytes && depth < 16384) depth *= 2;
    if (sw.no_ring || depth * per_diag + topo_bytes > kRingLdsBytes || !(depth >= 8 || depth >= V.span[0] + V.span[1] + 1)) return c;
    c.taken = true;
    c.pad = (uint16_t)(depth | (depth >= V.span[0] + V.span[1] + 1 ? 0x8000u : 0u));   // bit 15: the ring serves every read
    c.lds = depth * per_diag + topo_bytes;
    return c;
}

// a pair that is not a chain pair: the families in the order of preference — registers, systolic, strips, LDS ring, else planes in HBM.  Sets the descriptor's
// kind / pad / aux fields and appends the family's words to the part
void choose_dag_kernel(const PairView& V, const PackSwitches& sw, PackPart& P, ClProbDesc& d) {
    KernelChoice c = choose_lane(V, sw);
    if (c.taken) d.kind = CL_KIND_LANE;
    else if ((c = choose_sys(V, sw)).taken) d.kind = CL_KIND_SYS;
    else if ((c = choose_strip(V, sw, P)).taken) d.kind = CL_KIND_STRIP;
    else c = choose_ring(V, sw);   // (kind stays CL_KIND_GENERAL)
    if (c.taken) d.pad = c.pad;
    if (d.kind != CL_KIND_GENERAL) {
        d.aux_base = (uint32_t)P.sys_aux.size();
        d.aux_cnt = c.aux_cnt;
        P.sys_aux.insert(P.sys_aux.end(), c.aux.begin(), c.aux.end());
    }
    P.ring_need.push_back(c.taken ? (uint32_t)c.lds : 0u);
    P.plane_cursor += c.extra_plane_words;
}

// one subproblem: route -> (host route | pack both sides into rank space) -> choose the kernel
void pack_one(uint64_t k, const PackInput& in, cl_stitch_plan& pl, PackPart& P, Scratch& S) {
    const cl_stitch_batch* batch = in.batch;
    GraphView g[2] = {view(batch->side[0], k), view(batch->side[1], k)};
    int npw = in.force_num_pw ? in.force_num_pw[k] : choose_num_pw(g[0].n, g[1].n, in.params->alignment_params);
    if (npw < 1 || npw > 3) { P.fail(npw < 0 ? npw : CL_ERR_INVALID_ARGUMENT, npw == CL_ERR_BAD_GAP_PARAMS ? "Affine gap parameters must be increasing in gap open penalty and decreasing in gap extend penalty"
                                                    : "num_pw must be 1, 2 or 3 (problem %llu)", (unsigned long long)k); return; }
    bool only_del = batch->only_deletion_alns && batch->only_deletion_alns[k];
    int route;
    if (in.force_num_pw) route = g[1].n == 0 ? CL_ROUTE_PURE_DELETION_1 : g[0].n == 0 ? CL_ROUTE_PURE_DELETION_2 : CL_ROUTE_PO_POA;
    else route = route_problem(g[0], g[1], only_del, *in.params);
    if (route < 0) { P.fail(route, "problem %llu: subgraph is not acyclic", (unsigned long long)k); return; }
    pl.route[k] = (uint8_t)route;
    pl.num_pw[k] = (uint8_t)npw;
    if (route == CL_ROUTE_PURE_DELETION_1 || route == CL_ROUTE_PURE_DELETION_2) {
        const int rc = pure_deletion(route == CL_ROUTE_PURE_DELETION_1 ? g[0] : g[1], pl.pd_path[k]);
        if (rc) { P.fail(rc, "problem %llu: pure deletion failed", (unsigned long long)k); return; }
        P.pd_problem.push_back((uint32_t)k);
        return;
    }
    if (route != CL_ROUTE_PO_POA) {   // greedy / deletion-WFA / pruned WFA: host algorithms (in the reference too)
        const int rc = host_route_alignment(route, g[0], g[1], npw, *in.params, pl.host_aln[k]);
        if (rc) { P.fail(rc, rc == CL_ERR_INVALID_ARGUMENT ? "problem %llu: route %d needs the next lists of the subgraphs" : "problem %llu: host route %d failed",
                      (unsigned long long)k, route); return; }
        P.host_problem.push_back((uint32_t)k);
        return;
    }
    uint64_t cells = (g[0].n + 1) * (g[1].n + 1);
    if (cells >= (1ull << 30) || g[0].n_src == 0 || g[1].n_src == 0 || g[0].n_snk == 0 || g[1].n_snk == 0) { P.fail(cells >= (1ull << 30) ? CL_ERR_INVALID_ARGUMENT : CL_ERR_UNREACHABLE_SINK, "problem %llu: matrix too large for the device path or no sources/sinks", (unsigned long long)k); return; }
    ClProbDesc d{};
    d.n1 = (uint32_t)g[0].n;
    d.n2 = (uint32_t)g[1].n;
    d.npw = (uint8_t)npw;
    bool linear = true;
    uint64_t span[2] = {0, 0};
    for (int s = 0; s < 2; ++s)
        if (!pack_side(g[s], s, k, in.sw.rank_order, P, S, d, span[s], linear)) return;
    d.plane_base = P.plane_cursor;
    const ChainChoice chain = choose_chain(d.n1, d.n2, linear, in);
    if (chain.taken) {
        d.kind = CL_KIND_LINEAR;
        d.pad = chain.pad;
        P.plane_cursor += (cl_linear_workspace_bytes(std::min(d.n1, d.n2), std::max(d.n1, d.n2), npw, chain.rows_per_lane) + 15) / 16 * 4;
        P.ring_need.push_back(0);
    } else {
        d.kind = CL_KIND_GENERAL;
        P.plane_cursor += (cells * (uint64_t)(1 + 2 * npw) + 3) / 4 * 4;
        PairView V;
        for (int s = 0; s < 2; ++s) { V.off[s] = P.poff[s].data() + d.node_base[s]; V.lab[s] = P.lab[s].data() + d.node_base[s]; V.pidx[s] = P.pidx[s].data(); V.span[s] = span[s]; }
        V.n1 = d.n1; V.n2 = d.n2; V.npw = npw; V.cells = cells;
        V.n_pred = (P.poff[0].back() - P.poff[0][d.node_base[0]]) + (P.poff[1].back() - P.poff[1][d.node_base[1]]);
        V.sRow = d.n2 < d.n1 ? 1 : 0; V.sCol = 1 - V.sRow;
        V.n_rows = std::min(d.n1, d.n2) + 1; V.n_cols = std::max(d.n1, d.n2);
        choose_dag_kernel(V, in.sw, P, d);
    }
    P.chain_shape.push_back(chain.shape);
    if (P.out_cursor + d.n1 + d.n2 >= (1ull << 32)) { P.fail(CL_ERR_INVALID_ARGUMENT, "batch too large for 32-bit output offsets"); return; }
    d.out_base = (uint32_t)P.out_cursor;
    P.out_cursor += d.n1 + d.n2;
    P.desc.push_back(d);
    P.po_problem.push_back(k);
    P.dp_cells += cells;
    P.dp_bytes += cells * 4ull * (1 + 2 * npw);
    P.max_cells = std::max<uint64_t>(P.max_cells, cells);
    if (d.kind == CL_KIND_LINEAR) P.n_linear++;
}

// every subproblem of the batch, chunks of them side by side on the host pool
std::vector<PackPart> pack_parts(const PackInput& in, cl_stitch_plan& pl) {
    const uint64_t n = in.n;
    unsigned hw_threads = std::thread::hardware_concurrency();
    const uint64_t n_parts = std::max<uint64_t>(1, std::min<uint64_t>(std::min<uint64_t>(hw_threads ? hw_threads : 1, 16), n / 256));
    std::vector<PackPart> parts(n_parts);
    cl_pool_run((unsigned)n_parts, [&](unsigned t) {
        Scratch S;
        for (uint64_t k = n * t / n_parts; k < n * (t + 1) / n_parts && !parts[t].rc; ++k) pack_one(k, in, pl, parts[t], S);
    });
    return parts;
}

// the batch in rank space as the device gets it, and what the launch groups are formed from: the parts appended in order
struct Packed {
    std::vector<uint8_t> lab[2];
    std::vector<uint32_t> poff[2], pidx[2], snk[2];
    std::vector<uint32_t> ring_need, aux, strip_lds;   // per PO-POA problem: dynamic LDS (0 = none); ClDeviceBatch::aux; per strip: dynamic LDS
    std::vector<uint4> strip_recs;
    uint64_t hand_words = 0, plane_cursor = 0, out_cursor = 0;
    Packed() { poff[0].push_back(0); poff[1].push_back(0); }
};
// in order: the arrays of a serial pass, and the first failure is the one a serial pass would have met (its text in `err`)
int append_parts(std::vector<PackPart>& parts, cl_stitch_plan& pl, Packed& pk, std::string& err) {
    for (PackPart& P : parts) {
        if (P.rc) { err = P.err; return P.rc; }
        for (int s = 0; s < 2; ++s)
            if (pk.lab[s].size() + P.lab[s].size() >= (1ull << 32) || pk.pidx[s].size() + P.pidx[s].size() >= (1ull << 32)) { err = "batch too large for 32-bit device offsets"; return CL_ERR_INVALID_ARGUMENT; }
        if (pk.out_cursor + P.out_cursor >= (1ull << 32)) { err = "batch too large for 32-bit output offsets"; return CL_ERR_INVALID_ARGUMENT; }
        const uint32_t lab_base[2] = {(uint32_t)pk.lab[0].size(), (uint32_t)pk.lab[1].size()}, pidx_base[2] = {(uint32_t)pk.pidx[0].size(), (uint32_t)pk.pidx[1].size()};
        const uint32_t snk_base[2] = {(uint32_t)pk.snk[0].size(), (uint32_t)pk.snk[1].size()}, aux_base = (uint32_t)pk.aux.size();
        if (pk.strip_recs.size() + P.strip_recs.size() >= (1ull << 32)) { err = "batch too large for 32-bit device offsets"; return CL_ERR_INVALID_ARGUMENT; }
        for (ClStripDesc sd : P.strips) {
            sd.prob += (uint32_t)pl.desc.size();
            sd.rec_base += (uint32_t)pk.strip_recs.size();
            sd.hand_in += pk.hand_words; sd.hand_out += pk.hand_words;
            pl.strips.push_back(sd);
        }
        {   // the progress words are the strips' own indices
            const size_t base = pl.strips.size() - P.strips.size();
            for (size_t i = 0; i < P.strips.size(); ++i) pl.strips[base + i].prog = (uint32_t)(base + i);
        }
        pk.strip_recs.insert(pk.strip_recs.end(), P.strip_recs.begin(), P.strip_recs.end());
        pk.strip_lds.insert(pk.strip_lds.end(), P.strip_lds.begin(), P.strip_lds.end());
        pk.hand_words += P.hand_words;
        for (size_t i = 0; i < P.desc.size(); ++i) {
            ClProbDesc d = P.desc[i];
            for (int s = 0; s < 2; ++s) { d.node_base[s] += lab_base[s]; d.snk_base[s] += snk_base[s]; }
            d.plane_base += pk.plane_cursor;
            d.out_base += (uint32_t)pk.out_cursor;
            if (d.kind == CL_KIND_SYS || d.kind == CL_KIND_STRIP || d.kind == CL_KIND_LANE) d.aux_base += aux_base;
            pl.po_index[P.po_problem[i]] = (int32_t)pl.desc.size();
            pl.desc.push_back(d);
            pl.po_problem.push_back(P.po_problem[i]);
        }
        for (int s = 0; s < 2; ++s) {
            pk.lab[s].insert(pk.lab[s].end(), P.lab[s].begin(), P.lab[s].end());
            for (size_t i = 1; i < P.poff[s].size(); ++i) pk.poff[s].push_back(P.poff[s][i] + pidx_base[s]);
            pk.pidx[s].insert(pk.pidx[s].end(), P.pidx[s].begin(), P.pidx[s].end());
            pk.snk[s].insert(pk.snk[s].end(), P.snk[s].begin(), P.snk[s].end());
            pl.order[s].insert(pl.order[s].end(), P.order[s].begin(), P.order[s].end());
        }
        pk.ring_need.insert(pk.ring_need.end(), P.ring_need.begin(), P.ring_need.end());
        pk.aux.insert(pk.aux.end(), P.sys_aux.begin(), P.sys_aux.end());
        pl.pd_problem.insert(pl.pd_problem.end(), P.pd_problem.begin(), P.pd_problem.end());
        pl.host_problem.insert(pl.host_problem.end(), P.host_problem.begin(), P.host_problem.end());
        pl.chain_shape.insert(pl.chain_shape.end(), P.chain_shape.begin(), P.chain_shape.end());
        pk.plane_cursor += P.plane_cursor;
        pk.out_cursor += P.out_cursor;
        pl.stats.dp_cells += P.dp_cells;
        pl.stats.dp_bytes += P.dp_bytes;
        pl.stats.max_cells = std::max<uint64_t>(pl.stats.max_cells, P.max_cells);
        pl.stats.n_linear += P.n_linear;
        P = PackPart();
    }
    pl.stats.n_problems = pl.n_problems;
    pl.stats.n_po_poa = pl.desc.size();
    return CL_OK;
}

// ---- launch groups ----------------------------------------------------------------------------------------------------------------------------
// One group = one launch: a run of the plan's list of subproblems (plist; the strips have a list of their own), largest matrices / longest sweeps first inside
// a group.  What the group-forming functions below fill, beside cl_stitch_plan::groups:
struct LaunchLists {
    std::vector<uint32_t> plist;
    uint32_t lane_sync_words = 0;   // progress / done words of the wide near-chain pairs and the spanning chain pairs (cl_stitch_plan::d_lane_sync)
    std::vector<uint2> ptasks;      // the persistent chain launch's tasks (empty: no such launch)
};
// what forming the groups reads from the environment (what each means: at the function that uses it)
struct GroupSwitches {
    uint32_t lds_class[5];   // CL_STITCH_LDS_CLASSES, read per plan
    bool persistent, block128, narrow;   // CL_STITCH_PERSISTENT, CL_SYS_BLOCK128, CL_STITCH_NARROW, once per process
};
GroupSwitches read_group_switches() {
    GroupSwitches gs;
    const uint32_t classes[5] = {12 * 1024, 32 * 1024, 64 * 1024, 100 * 1024, (uint32_t)kSysLdsBytes};
    std::copy(classes, classes + 5, gs.lds_class);
    if (const char* e = getenv("CL_STITCH_LDS_CLASSES")) {
        unsigned a = 0, b = 0, c = 0, d = 0;
        if (sscanf(e, "%u,%u,%u,%u", &a, &b, &c, &d) == 4 && a < b && b < c && c < d && d * 1024u < (uint32_t)kSysLdsBytes) { gs.lds_class[0] = a * 1024; gs.lds_class[1] = b * 1024; gs.lds_class[2] = c * 1024; gs.lds_class[3] = d * 1024; }
    }
    static const bool persistent = [] { const char* e = getenv("CL_STITCH_PERSISTENT"); return !e || e[0] != '0'; }();
    static const bool block128 = [] { const char* e = getenv("CL_SYS_BLOCK128"); return e && e[0] == '1'; }();
    static const bool narrow_on = [] { const char* e = getenv("CL_STITCH_NARROW"); return !e || e[0] != '0'; }();
    gs.persistent = persistent; gs.block128 = block128; gs.narrow = narrow_on;
    return gs;
}

inline uint64_t cells_of(const ClProbDesc& d) { return (uint64_t)(d.n1 + 1) * (d.n2 + 1); }
inline uint64_t plane_bytes_of(const ClProbDesc& d) { return cells_of(d) * 4ull * (1 + 2 * d.npw); }
inline uint64_t sweep_of(const ClProbDesc& d) { return (uint64_t)d.n1 + d.n2; }
inline void add_work(LaunchGroup& grp, const ClProbDesc& d) { grp.cells += cells_of(d); grp.bytes += plane_bytes_of(d); }
// a group whose members are plist[grp.first ..]: its count, cells and bytes; the members sorted by `key`, largest first.  false: no members
template <class Key>
bool finish_group(const cl_stitch_plan& pl, LaunchLists& L, LaunchGroup& grp, Key key) {
    grp.count = (uint32_t)L.plist.size() - grp.first;
    if (!grp.count) return false;
    for (uint32_t i = grp.first; i < L.plist.size(); ++i) add_work(grp, pl.desc[L.plist[i]]);
    std::stable_sort(L.plist.begin() + grp.first, L.plist.end(), [&](uint32_t x, uint32_t y) { return key(pl.desc[x]) > key(pl.desc[y]); });
    return true;
}

// two pairs per wave only where it pays (duos_forced): the pairs marked for it run one per wave otherwise — same codes, same workspace
void decide_duos(cl_stitch_plan& pl, int duos) {
    if (duos >= 0) return;
    uint64_t marked = 0;
    for (const ChainShape& cs : pl.chain_shape) marked += cs.variant == LaunchVariant::Duos;
    if (pl.n_problems < 2048 || 2 * marked >= pl.desc.size()) return;
    for (ChainShape& cs : pl.chain_shape)
        if (cs.variant == LaunchVariant::Duos) cs = {LaunchVariant::Chain, 1};
}
// chain kernel: one launch per workgroup shape; the problems are ordered by the length of their sweep
void form_chain_groups(cl_stitch_plan& pl, LaunchLists& L) {
    for (int waves : {16, 8, 4, 3, 1}) {
        LaunchGroup grp;
        grp.variant = LaunchVariant::Chain; grp.waves = waves;
        grp.first = (uint32_t)L.plist.size();
        for (uint32_t i = 0; i < pl.desc.size(); ++i)
            if (pl.chain_shape[i].variant == LaunchVariant::Chain && pl.chain_shape[i].waves == waves) L.plist.push_back(i);
        if (finish_group(pl, L, grp, [](const ClProbDesc& d) { return sweep_of(d) + (d.npw == 3 ? 64 : 0); })) pl.groups.push_back(grp);
    }
}
// small chain pairs, four per wave (popoa_linear_quad_kernel) or two (popoa_linear_duo_kernel): quads / duos of one NumPW, longest first so that a unit's
// pairs are about as long as one another; each NumPW's run is padded to whole units with 0xFFFFFFFF
void form_quad_duo_groups(cl_stitch_plan& pl, LaunchLists& L) {
    for (LaunchVariant variant : {LaunchVariant::Quads, LaunchVariant::Duos}) {
        LaunchGroup grp;
        grp.variant = variant;
        grp.first = (uint32_t)L.plist.size();
        for (int npw = 3; npw >= 1; --npw) {
            std::vector<uint32_t> q;
            for (uint32_t i = 0; i < pl.desc.size(); ++i)
                if (pl.chain_shape[i].variant == variant && pl.desc[i].npw == npw) q.push_back(i);
            std::stable_sort(q.begin(), q.end(), [&](uint32_t x, uint32_t y) { return std::max(pl.desc[x].n1, pl.desc[x].n2) > std::max(pl.desc[y].n1, pl.desc[y].n2); });
            for (uint32_t i : q) {
                L.plist.push_back(i);
                add_work(grp, pl.desc[i]);
            }
            while ((L.plist.size() - grp.first) % (variant == LaunchVariant::Quads ? 4 : 2)) L.plist.push_back(0xFFFFFFFFu);
        }
        grp.count = (uint32_t)L.plist.size() - grp.first;
        if (grp.count) pl.groups.push_back(grp);
    }
}
// The one-wave chain launches (popoa_linear_kernel<1>, quads, duos: tens of thousands of workgroups between them) become ONE persistent launch
// (popoa_chain_persistent_kernel): a grid of as many workgroups as are resident at once pulls tasks from the plan's task list,
// longest first.  Launches that share a hardware queue run one after the other; one launch less per kind is one launch less in that line, and the
// three kinds fill one another's tails.  A task is a run of units of one kind (a pair, a quad, a duo) of at most kChunkUnits units and kChunkSteps
// anti-diagonal steps (a longer unit is a task of its own): a few thousand dequeues a pass instead of one per workgroup.
// (only where there are two or three of the kinds: a batch of one kind keeps that kind's own launch.)  CL_STITCH_PERSISTENT=0: one launch per kind as before (A/B, parity tests)
// resident_workgroups(): cl_chain_persistent_capacity on the plan's device, asked only when the launch is made (0: unknown)
template <class Capacity>
void merge_persistent_chain(cl_stitch_plan& pl, LaunchLists& L, Capacity resident_workgroups) {
    constexpr uint32_t kChunkUnits = 8, kChunkSteps = 512;
    std::vector<size_t> members;
    for (size_t gi = 0; gi < pl.groups.size(); ++gi) {
        const LaunchGroup& g = pl.groups[gi];
        if ((g.variant == LaunchVariant::Chain && g.waves == 1) || g.variant == LaunchVariant::Quads || g.variant == LaunchVariant::Duos) members.push_back(gi);
    }
    std::vector<uint2>& ptasks = L.ptasks;
    std::vector<uint64_t> task_cost;
    LaunchGroup merged;
    merged.variant = LaunchVariant::ChainPersistent;
    merged.first = members.empty() ? 0u : pl.groups[members[0]].first;
    uint32_t end = merged.first;
    bool contiguous = true;
    for (size_t gi : members) {
        const LaunchGroup& g = pl.groups[gi];
        contiguous = contiguous && g.first == end;
        end = g.first + g.count;
        merged.cells += g.cells;
        merged.bytes += g.bytes;
        // the task word's kind (popoa_chain_persistent_kernel): 0 a pair, 1 a quad, 2 a duo
        const uint32_t kind = g.variant == LaunchVariant::Chain ? 0u : g.variant == LaunchVariant::Quads ? 1u : 2u, per_unit = kind == 0 ? 1u : kind == 1 ? 4u : 2u;
        auto unit_cost = [&](uint32_t at) {
            uint64_t c = 0;
            for (uint32_t j = 0; j < per_unit; ++j) {
                const uint32_t x = L.plist[at + j];
                if (x != 0xFFFFFFFFu) c = std::max<uint64_t>(c, sweep_of(pl.desc[x]) + (pl.desc[x].npw == 3 ? 64 : 0));
            }
            return c;
        };
        for (uint32_t at = g.first; at < g.first + g.count;) {
            uint32_t n = 0;
            uint64_t cost = 0;
            while (at + n * per_unit < g.first + g.count && n < kChunkUnits) {
                const uint64_t c = unit_cost(at + n * per_unit);
                if (n && cost + c > kChunkSteps) break;
                cost += c;
                ++n;
            }
            ptasks.push_back(make_uint2(at, kind << 24 | n));
            task_cost.push_back(cost);
            at += n * per_unit;
        }
    }
    if (members.size() <= 1 || !contiguous) {
        ptasks.clear();   // (one kind or none: its own launch, as with CL_STITCH_PERSISTENT=0 — nothing to share its tail with)
        return;
    }
    merged.count = end - merged.first;
    std::vector<uint32_t> idx(ptasks.size());
    for (uint32_t i = 0; i < idx.size(); ++i) idx[i] = i;
    std::stable_sort(idx.begin(), idx.end(), [&](uint32_t x, uint32_t y) { return task_cost[x] > task_cost[y]; });
    std::vector<uint2> sorted(ptasks.size());
    for (size_t i = 0; i < idx.size(); ++i) sorted[i] = ptasks[idx[i]];
    ptasks.swap(sorted);
    uint32_t capacity = resident_workgroups();   // (per plan, on the plan's device: one occupancy query)
    if (!capacity) capacity = 2048u;
    merged.grid = std::min<uint32_t>(capacity, (uint32_t)ptasks.size());
    merged.prog_count = (uint32_t)ptasks.size();
    for (size_t k = members.size(); k-- > 0;) pl.groups.erase(pl.groups.begin() + (std::ptrdiff_t)members[k]);
    pl.groups.push_back(merged);
}
// near-chain pairs in registers: one launch per workgroup shape as well (strips of 64 rows over 1 / 4 / 16 waves), longest sweep first
void form_lane_groups(cl_stitch_plan& pl, const Packed& pk, LaunchLists& L, uint32_t lane_rw) {
    for (int waves : {0, (int)lane_rw, 1}) {   // (one wave per SIMD; no launches of eight waves any more)
        LaunchGroup grp;
        grp.variant = LaunchVariant::Lane; grp.waves = waves;
        grp.first = (uint32_t)L.plist.size();
        for (uint32_t i = 0; i < pl.desc.size(); ++i) {
            const ClProbDesc& d = pl.desc[i];
            const uint32_t rows = std::min(d.n1, d.n2);
            if (d.kind == CL_KIND_LANE && !((d.pad >> 8) & 0x7Fu) && (rows <= 64 ? 1 : (int)lane_rw) == grp.waves) { L.plist.push_back(i); grp.ring_bytes = std::max<uint32_t>(grp.ring_bytes, pk.ring_need[i]); }
        }
        if (finish_group(pl, L, grp, [](const ClProbDesc& d) { return sweep_of(d) + 96ull * (std::min(d.n1, d.n2) / 64); })) pl.groups.push_back(grp);
    }
}
// The two families whose pairs take several workgroups each that wait for one another: a pair's workgroups are consecutive workgroups of one launch — whole pairs,
// at most 224 workgroups per launch, longest sweep first; their progress / done words (two per workgroup) are a run of the plan's lane_sync array, zeroed in front
// of the launch.  workgroups_of(pair) -> how many; bind(pair, first word, workgroups) tells the pair where its words are.
template <class Workgroups, class Bind>
void form_coresident_groups(cl_stitch_plan& pl, const Packed& pk, LaunchLists& L, const LaunchGroup& proto, std::vector<uint32_t> pairs, Workgroups workgroups_of, Bind bind) {
    LaunchGroup grp;
    auto open = [&]() { grp = proto; grp.first = (uint32_t)L.plist.size(); grp.prog_first = L.lane_sync_words; };
    auto close = [&]() {
        grp.count = (uint32_t)L.plist.size() - grp.first;
        grp.prog_count = L.lane_sync_words - grp.prog_first;
        if (grp.count) pl.groups.push_back(grp);
    };
    open();
    std::stable_sort(pairs.begin(), pairs.end(), [&](uint32_t x, uint32_t y) { return sweep_of(pl.desc[x]) > sweep_of(pl.desc[y]); });
    for (uint32_t i : pairs) {
        const uint32_t ng = workgroups_of(pl.desc[i]);
        if ((uint32_t)L.plist.size() - grp.first + ng > 224) { close(); open(); }
        bind(i, L.lane_sync_words, ng);
        L.lane_sync_words += 2 * ng;
        for (uint32_t g2 = 0; g2 < ng; ++g2) L.plist.push_back(i);
        grp.ring_bytes = std::max<uint32_t>(grp.ring_bytes, pk.ring_need[i]);   // (0 for a chain pair)
        add_work(grp, pl.desc[i]);
    }
    close();
}
// wide near-chain pairs (CL_LANE_WIDE=1): a pair's groups of three strips; the first word of the pair's aux record says where its progress words are
void form_wide_lane_groups(cl_stitch_plan& pl, Packed& pk, LaunchLists& L) {
    std::vector<uint32_t> wide;
    for (uint32_t i = 0; i < pl.desc.size(); ++i) if (pl.desc[i].kind == CL_KIND_LANE && ((pl.desc[i].pad >> 8) & 0x7Fu)) wide.push_back(i);
    LaunchGroup proto;
    proto.variant = LaunchVariant::LaneWide; proto.waves = 4;
    form_coresident_groups(pl, pk, L, proto, std::move(wide), [](const ClProbDesc& d) { return ((d.pad >> 8) & 0x7Fu) + 1u; },
                           [&](uint32_t i, uint32_t word, uint32_t) { pk.aux[pl.desc[i].aux_base] = word; });
}
// chain pairs that span several workgroups (popoa_linear_span_kernel): ClProbDesc::aux_base = the pair's first word, aux_cnt = its groups
void form_span_groups(cl_stitch_plan& pl, const Packed& pk, LaunchLists& L) {
    std::vector<uint32_t> span;
    for (uint32_t i = 0; i < pl.desc.size(); ++i) if (pl.chain_shape[i].variant == LaunchVariant::ChainSpan) span.push_back(i);
    LaunchGroup proto;
    proto.variant = LaunchVariant::ChainSpan;
    form_coresident_groups(pl, pk, L, proto, std::move(span), [](const ClProbDesc& d) { return cl_linear_span_groups(std::min(d.n1, d.n2)); },
                           [&](uint32_t i, uint32_t word, uint32_t ng) { pl.desc[i].aux_base = word; pl.desc[i].aux_cnt = ng; });
}
// general kernel: (workgroup size by widest anti-diagonal, NumPW, LDS class), largest matrices first
void form_general_groups(cl_stitch_plan& pl, const Packed& pk, LaunchLists& L) {
    const int blocks[3] = {64, 256, 1024};
    for (int bi = 2; bi >= 0; --bi)
        for (int npw = 3; npw >= 1; --npw)
            for (int ring = 2; ring >= 0; --ring) {   // 2: ring above 64 KB of LDS (one workgroup per CU), 1: ring up to 64 KB, 0: planes in HBM
                LaunchGroup grp;
                grp.variant = LaunchVariant::General; grp.npw = npw; grp.block = blocks[bi];
                grp.first = (uint32_t)L.plist.size();
                for (uint32_t i = 0; i < pl.desc.size(); ++i) {
                    const ClProbDesc& d = pl.desc[i];
                    uint32_t width = std::min(d.n1, d.n2) + 1;
                    int b = width <= 64 ? 0 : width <= 256 ? 1 : 2;
                    const int cls = d.pad == 0 ? 0 : pk.ring_need[i] > 64 * 1024 ? 2 : 1;
                    if (d.kind == CL_KIND_GENERAL && d.npw == npw && b == bi && cls == ring) {
                        L.plist.push_back(i);
                        if (ring) grp.ring_bytes = std::max<uint32_t>(grp.ring_bytes, pk.ring_need[i]);
                    }
                }
                if (finish_group(pl, L, grp, cells_of)) pl.groups.push_back(grp);
            }
}
// systolic DAG kernel: (NumPW, workgroup size, LDS class) — a launch's dynamic LDS is that of its hungriest problem, and LDS decides
// how many workgroups share a CU, so the many small problems must not ride with the few large ones
// CL_STITCH_LDS_CLASSES=a,b,c,d (KB; four boundaries below the ceiling) for measurements
// ... unless the smaller ones are so few that all workgroups of the merged launch are resident at once anyway: a launch lasts as long as its longest sweep
// whatever rides along, and every launch less is a millisecond less on the stream it would have occupied (the streams, not the device, are what a step
// runs out of: 10 x 1 Mbp, sixteen launches a step on eight streams)
// workgroup sizes of the systolic kernel: 64 / 128 / 256 / 1024 threads (round 6: pairs of 65-128 rows — two thirds of the subproblems that used to take 256 threads in
// the step of 10 x 1 Mbp — get two waves instead of four: a barrier between two waves, no idle waves at it).  CL_SYS_BLOCK128=1 for measurements
// (measured and lost: 1.51-1.52 -> 1.61-1.68 ms per step — two more launches on the step's streams; off unless asked for)
// (one wave with two / four rows per lane — popoa_sysr_kernel, commit 2b07e99 — was measured and lost as well: 3.37 against 1.56 ms per step, profiles/r06_rows_per_lane_ab.txt)
void form_sys_groups(cl_stitch_plan& pl, const Packed& pk, LaunchLists& L, const GroupSwitches& gs) {
    const int sys_blocks[4] = {64, 128, 256, 1024};
    for (int bi = 3; bi >= 0; --bi)
        for (int npw = 3; npw >= 1; --npw) {
            std::vector<uint32_t> of_class[5];
            for (uint32_t i = 0; i < pl.desc.size(); ++i) {
                const ClProbDesc& d = pl.desc[i];
                const uint32_t rows = std::min(d.n1, d.n2) + 1;
                const int b = rows <= 64 ? 0 : (rows <= 128 && gs.block128) ? 1 : rows <= 256 ? 2 : 3;
                if (d.kind != CL_KIND_SYS || d.npw != npw || b != bi) continue;
                int c = 0;
                while (c < 4 && pk.ring_need[i] > gs.lds_class[c]) ++c;
                of_class[c].push_back(i);
            }
            LaunchGroup grp;
            auto open = [&]() { grp = LaunchGroup(); grp.variant = LaunchVariant::Sys; grp.npw = npw; grp.block = sys_blocks[bi]; grp.first = (uint32_t)L.plist.size(); };
            auto close = [&]() { if (finish_group(pl, L, grp, cells_of)) pl.groups.push_back(grp); };
            open();
            for (int lc = 4; lc >= 0; --lc) {
                if (of_class[lc].empty()) continue;
                const size_t have = L.plist.size() - grp.first;
                if (have) {
                    const uint64_t per_cu = std::max<uint64_t>(1, std::min<uint64_t>((160u * 1024u) / std::max<uint32_t>(grp.ring_bytes, 1u), 2048u / (uint32_t)sys_blocks[bi]));
                    // all resident at once.  (Also merging classes that leave the newcomers' workgroups per compute unit unchanged was measured and lost: 2.75 against
                    // 2.55 ms per step — the long sweeps of the two classes then share a launch's tail)
                    const bool fits = have + of_class[lc].size() <= 256 * per_cu;
                    if (!fits) { close(); open(); }
                }
                for (uint32_t i : of_class[lc]) {
                    L.plist.push_back(i);
                    grp.ring_bytes = std::max<uint32_t>(grp.ring_bytes, pk.ring_need[i]);
                }
            }
            close();
        }
}
// strips of rows: every strip of a pair is a workgroup of the same launch (they wait for one another: at most 224 workgroups per launch, whole pairs)
void form_strip_groups(cl_stitch_plan& pl, const Packed& pk) {
    for (int npw = 3; npw >= 1; --npw) {
        LaunchGroup grp;
        auto open = [&]() { grp = LaunchGroup(); grp.variant = LaunchVariant::Strip; grp.npw = npw; grp.first = (uint32_t)pl.strip_list.size(); grp.prog_first = UINT32_MAX; };
        auto close = [&]() {
            grp.count = (uint32_t)pl.strip_list.size() - grp.first;
            if (grp.count) pl.groups.push_back(grp);
        };
        open();
        for (size_t i = 0; i < pl.strips.size();) {
            const ClStripDesc& s0 = pl.strips[i];
            const ClProbDesc& d = pl.desc[s0.prob];
            if (d.npw != npw) { i += s0.n_strips; continue; }
            if ((uint32_t)pl.strip_list.size() - grp.first + s0.n_strips > 224) { close(); open(); }
            // a strip's progress word = its position in the launch lists: the words of a launch are one run, zeroed by that launch alone (launches of
            // other NumPW run beside it on other streams and must not have their words touched)
            if (grp.prog_first == UINT32_MAX) grp.prog_first = (uint32_t)pl.strip_list.size();
            uint32_t max_rows = 0;
            for (uint32_t j = 0; j < s0.n_strips; ++j) {
                pl.strips[i + j].prog = (uint32_t)pl.strip_list.size();
                pl.strip_list.push_back((uint32_t)(i + j));
                grp.ring_bytes = std::max(grp.ring_bytes, pk.strip_lds[i + j]);
                max_rows = std::max(max_rows, pl.strips[i + j].n_real);
            }
            grp.prog_count = (uint32_t)pl.strip_list.size() - grp.prog_first;
            grp.block = std::max<int>(grp.block, 256 + (int)((max_rows + 63) / 64 * 64));
            add_work(grp, d);
            grp.est_cost = std::max<uint64_t>(grp.est_cost, sweep_of(d) + 96ull * s0.n_strips);
            i += s0.n_strips;
            ++cl_fallbacks.strip_pairs;
        }
        close();
    }
}

// a group's duration is set by its longest anti-diagonal sweep: that, times the kernel's rough time per step (the strips' estimate is made with the group)
uint64_t estimate_cost(const cl_stitch_plan& pl, const LaunchLists& L, const LaunchGroup& g) {
    if (g.variant == LaunchVariant::Strip) return g.est_cost;
    uint64_t c = 0;
    if (cl_launch_pair_spans_workgroups(g.variant)) {
        // wide: every 64 rows add a lag of three chunks; a spanning chain pair: one round over several workgroups, columns + 1.5 x rows steps
        const uint64_t rows_weight = g.variant == LaunchVariant::LaneWide ? 5 : 3;
        for (uint32_t i = g.first; i < g.first + g.count; ++i) {
            const ClProbDesc& d = pl.desc[L.plist[i]];
            c = std::max<uint64_t>(c, (uint64_t)std::max(d.n1, d.n2) + rows_weight * std::min(d.n1, d.n2) / 2);
        }
        return c / 3;
    }
    for (uint32_t i = g.first; i < g.first + g.count; ++i)
        if (L.plist[i] != 0xFFFFFFFFu) c = std::max<uint64_t>(c, sweep_of(pl.desc[L.plist[i]]));
    // microseconds per anti-diagonal step, roughly: planes in HBM 4-8, LDS ring 1.6-2.5, systolic DAG 0.45, chain 0.2-0.6
    return c * (g.variant == LaunchVariant::General ? (g.ring_bytes ? 5 : 16) : 1);
}

// Launches of few workgroups that last as long as their longest sweep (popoa_lane_kernel<1 / 3 / 4>, popoa_sys_kernel<NPW, 64 / 256> of few pairs) become
// ONE launch (popoa_narrow_kernel): launches that share a hardware queue run one after the other, and in the step of 10 x 1 Mbp lane<3> (66 workgroups,
// 1.3 ms), lane<1> (8, 1.0 ms) and a sys<2, 256> launch (21, 0.6 ms) held their queues for 2.9 ms together.  Every workgroup runs the body of its own
// launch on the same pair; a member is taken, longest sweep first, only while every workgroup of the merged launch is resident at once (compute units x
// the workgroups per compute unit of the merged block size and LDS), so the merged launch lasts about as long as its longest member.  The rest keep
// their launches.  Only in plans of 2 048 subproblems and more (the plans whose launches share the device, as lane_round_waves); CL_STITCH_NARROW=0:
// separate launches (A/B, parity tests)
// ClNarrowRoles::code of a group that may become a member (popoa_narrow_kernel's role), -1: not one
int narrow_role_code(const LaunchGroup& g) {
    if (g.variant == LaunchVariant::Lane) return g.waves == 1 ? 0 : g.waves == 3 ? 1 : g.waves == 4 ? 2 : -1;
    if (g.variant == LaunchVariant::Sys && (g.block == 64 || g.block == 256)) return 3 + 2 * (g.npw - 1) + (g.block == 256);
    return -1;
}
// resident_workgroups(threads, lds): cl_narrow_capacity on the plan's device (0 if the query failed: nothing merges)
template <class Capacity>
void merge_narrow(cl_stitch_plan& pl, const LaunchLists& L, Capacity resident_workgroups) {
    std::vector<size_t> cand;
    for (size_t gi = 0; gi < pl.groups.size(); ++gi) if (narrow_role_code(pl.groups[gi]) >= 0) cand.push_back(gi);
    std::vector<uint64_t> sweep(pl.groups.size(), 0);
    for (size_t gi : cand) {
        const LaunchGroup& g = pl.groups[gi];
        for (uint32_t i = g.first; i < g.first + g.count; ++i) sweep[gi] = std::max<uint64_t>(sweep[gi], sweep_of(pl.desc[L.plist[i]]));
    }
    std::stable_sort(cand.begin(), cand.end(), [&](size_t x, size_t y) { return sweep[x] > sweep[y]; });
    std::vector<size_t> members;
    uint64_t blocks = 0;
    uint32_t lds = 0;
    int threads = 192;
    for (size_t gi : cand) {
        const LaunchGroup& g = pl.groups[gi];
        if (members.size() == (size_t)kNarrowMaxRoles) break;
        const int t = std::max(threads, g.variant == LaunchVariant::Lane ? 64 * g.waves : g.block);
        const uint32_t l = std::max(lds, g.ring_bytes);
        if (l > 159u * 1024u) continue;
        const uint64_t resident = resident_workgroups(t, l);
        if (blocks + g.count > resident) continue;
        members.push_back(gi);
        blocks += g.count;
        lds = l;
        threads = t;
    }
    if (members.size() < 2) return;
    LaunchGroup merged;
    merged.variant = LaunchVariant::Narrow;
    merged.block = threads;
    merged.ring_bytes = lds;
    merged.count = (uint32_t)blocks;
    pl.narrow = ClNarrowRoles{};
    for (size_t gi : members) {
        const LaunchGroup& g = pl.groups[gi];
        const uint32_t r = pl.narrow.n++;
        pl.narrow.end[r] = (r ? pl.narrow.end[r - 1] : 0u) + g.count;
        pl.narrow.first[r] = g.first;
        pl.narrow.code[r] = (uint32_t)narrow_role_code(g);
        merged.cells += g.cells;
        merged.bytes += g.bytes;
        merged.est_cost = std::max(merged.est_cost, g.est_cost);
    }
    std::sort(members.begin(), members.end());
    for (size_t k = members.size(); k-- > 0;) pl.groups.erase(pl.groups.begin() + (std::ptrdiff_t)members[k]);
    pl.groups.push_back(merged);
}

// ---- HBM --------------------------------------------------------------------------------------------------------------------------------------
// uploads the packed batch and the launch lists, allocates the workspace and the outputs, and fills the plan's device views
int upload_plan(cl_context* ctx, cl_stitch_plan* pl, const Packed& pk, LaunchLists& L) {
    int rc;
    const cl_align_params& ap = pl->aparams;
    pl->plist_host = L.plist;
    // (the eleven copies are enqueued and waited for once: the host arrays live to the end of this function)
    if ((rc = pl->d_desc.upload_async(ctx, pl->desc)) || (rc = pl->d_plist.upload_async(ctx, L.plist)) || (rc = pl->d_aux.upload_async(ctx, pk.aux))) return rc;
    for (int s = 0; s < 2; ++s)
        if ((rc = pl->d_lab[s].upload_async(ctx, pk.lab[s])) || (rc = pl->d_poff[s].upload_async(ctx, pk.poff[s])) ||
            (rc = pl->d_pidx[s].upload_async(ctx, pk.pidx[s])) || (rc = pl->d_snk[s].upload_async(ctx, pk.snk[s]))) return rc;
    if (!pl->strips.empty() && ((rc = pl->d_strips.upload_async(ctx, pl->strips)) || (rc = pl->d_strip_recs.upload_async(ctx, pk.strip_recs)) ||
                                (rc = pl->d_strip_list.upload_async(ctx, pl->strip_list)) || (rc = pl->d_progress.alloc(ctx, pl->strips.size())) ||
                                (rc = pl->d_handoff.alloc(ctx, pk.hand_words)))) return rc;
    if (L.lane_sync_words && (rc = pl->d_lane_sync.alloc(ctx, L.lane_sync_words))) return rc;
    const std::vector<uint32_t> phead_zero(2, 0u);
    if (!L.ptasks.empty() && ((rc = pl->d_ptasks.upload_async(ctx, L.ptasks)) || (rc = pl->d_phead.upload_async(ctx, phead_zero)))) return rc;
    pl->sparams.match = (int32_t)ap.match;
    pl->sparams.mismatch = (int32_t)ap.mismatch;
    for (int k = 0; k < 3; ++k) { pl->sparams.oe[k] = (int32_t)(ap.gap_open[k] + ap.gap_extend[k]); pl->sparams.ext[k] = (int32_t)ap.gap_extend[k]; }
    const std::vector<ClScoreParams> sparams_copy(1, pl->sparams);
    if (pl->narrow.n && (rc = pl->d_sparams.upload_async(ctx, sparams_copy))) return rc;
    if (hipStreamSynchronize(ctx->stream) != hipSuccess) { cl_set_error(ctx, "upload failed"); return CL_ERR_HIP; }
    { static const bool dbg = [] { const char* e = getenv("CL_STRIP_DEBUG_FAIL"); return e && *e == '1'; }(); pl->sdev.debug_fail = dbg ? 1u : 0u; }
    pl->sdev.strips = pl->d_strips.p; pl->sdev.recs = pl->d_strip_recs.p; pl->sdev.handoff = pl->d_handoff.p; pl->sdev.progress = pl->d_progress.p;
    if ((rc = pl->d_planes.alloc(ctx, pk.plane_cursor)) || (rc = pl->d_out_pairs.alloc(ctx, pk.out_cursor)) ||
        (rc = pl->d_out_len.alloc(ctx, pl->desc.size())) || (rc = pl->d_out_status.alloc(ctx, pl->desc.size())) ||
        (rc = pl->d_out_score.alloc(ctx, pl->desc.size()))) return rc;
    pl->stats.workspace_bytes = pk.plane_cursor * 4 + pk.out_cursor * 8 + pk.lab[0].size() + pk.lab[1].size() +
                                4 * (pk.poff[0].size() + pk.poff[1].size() + pk.pidx[0].size() + pk.pidx[1].size());
    pl->dev.desc = pl->d_desc.p;
    for (int s = 0; s < 2; ++s) {
        pl->dev.lab[s] = pl->d_lab[s].p; pl->dev.poff[s] = pl->d_poff[s].p; pl->dev.pidx[s] = pl->d_pidx[s].p; pl->dev.snk[s] = pl->d_snk[s].p;
    }
    pl->dev.aux = pl->d_aux.p;
    pl->dev.planes = pl->d_planes.p;
    pl->dev.out_pairs = pl->d_out_pairs.p;
    pl->dev.out_len = pl->d_out_len.p;
    pl->dev.out_score = pl->d_out_score.p;
    pl->dev.out_status = pl->d_out_status.p;
    { const char* e = getenv("CL_SPAN_DEBUG_FAIL"); pl->dev.debug_flags = e && e[0] == '1' ? 1 : 0; }   // test hook: every spanning chain pair reports status 9
    { const char* e = getenv("CL_LANE_CELLS"); if (e && !strcmp(e, "general")) pl->dev.debug_flags |= 2; }   // A/B, tests (read per plan): popoa_lane_kernel's steps that are not the usual one all take the general cell
    { const char* e = getenv("CL_DEBUG_SKIP_TRACEBACK"); pl->dev.skip_traceback = e ? atoi(e) : 0; }   // measurement hook: 1 no traceback, 3 also no plane stores in the systolic kernel
    if (hipEventCreate(&pl->ev_start) != hipSuccess || hipEventCreate(&pl->ev_stop) != hipSuccess) {
        set_error(ctx, "hipEventCreate failed");
        return CL_ERR_HIP;
    }
    return CL_OK;
}

// the arguments of cl_stitch_plan_create: both sides' arrays, and the score magnitudes.
// Magnitudes beyond the fixed limits are taken where the batch keeps every score inside the int32 budget the reference has too:
// (n1 + n2 + 2) x (largest term) < 2^28 for its largest pair, so that nothing added to CL_NEG_INF (-2^30) wraps
int validate_batch(cl_context* ctx, const cl_stitch_batch* batch, const cl_align_params& ap) {
    const uint64_t n = batch->n_problems;
    int rc;
    if ((rc = validate_side(ctx, batch->side[0], n, 1)) || (rc = validate_side(ctx, batch->side[1], n, 2))) return rc;
    bool small = ap.match <= (1u << 20) && ap.mismatch <= (1u << 20);
    uint64_t term = std::max<uint64_t>(ap.match, ap.mismatch);
    for (int k = 0; k < 3; ++k) {
        small = small && ap.gap_open[k] <= (1u << 24) && ap.gap_extend[k] <= (1u << 24);
        term = std::max<uint64_t>(term, (uint64_t)ap.gap_open[k] + ap.gap_extend[k]);
    }
    if (small) return CL_OK;
    uint64_t longest = 0;
    for (uint64_t k = 0; k < n; ++k)
        longest = std::max<uint64_t>(longest, (batch->side[0].node_off[k + 1] - batch->side[0].node_off[k]) + (batch->side[1].node_off[k + 1] - batch->side[1].node_off[k]));
    if (term >= (1ull << 28) || longest >= (1ull << 28) || (longest + 2) * term >= (1ull << 28)) {
        set_error(ctx, "%s: beyond 2^20 (match, mismatch) / 2^24 (gaps) a batch must keep (n1 + n2 + 2) x largest term below 2^28 for its largest pair",
                  ap.match > (1u << 20) || ap.mismatch > (1u << 20) ? "match/mismatch too large" : "gap penalties too large");
        return CL_ERR_INVALID_ARGUMENT;
    }
    return CL_OK;
}

}  // namespace

extern "C" {

int cl_stitch_plan_create(cl_context* ctx, const cl_stitch_batch* batch, const cl_stitch_params* params,
                          const uint8_t* force_num_pw, cl_stitch_plan** plan_out) {
    if (!ctx || !batch || !params || !plan_out) { set_error(ctx, "null argument"); return CL_ERR_INVALID_ARGUMENT; }
    *plan_out = nullptr;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const uint64_t n = batch->n_problems;
    const cl_align_params& ap = params->alignment_params;
    int rc = validate_batch(ctx, batch, ap);
    if (rc) return rc;

    static const bool timing = getenv("CL_STITCH_TIMING") != nullptr;
    auto tp = std::chrono::steady_clock::now();
    auto lap = [&](const char* what) {
        if (timing) fprintf(stderr, "[cl_stitch]     %-20s %8.2f ms\n", what, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tp).count());
        tp = std::chrono::steady_clock::now();
    };
    ClStitchPlanPtr pl(new (std::nothrow) cl_stitch_plan());   // (every error exit below releases it: cl_stitch_plan_free)
    if (!pl) return CL_ERR_OUT_OF_MEMORY;
    pl->n_problems = n;
    pl->aparams = ap;
    pl->route.assign(n, 0);
    pl->num_pw.assign(n, 0);
    pl->po_index.assign(n, -1);
    pl->pd_path.resize(n);
    pl->host_aln.resize(n);
    for (int s = 0; s < 2; ++s) {
        pl->node_off[s].assign(batch->side[s].node_off, batch->side[s].node_off + n + 1);
        if (batch->side[s].back_translation) {
            pl->has_back[s] = true;
            pl->back[s].assign(batch->side[s].back_translation, batch->side[s].back_translation + batch->side[s].node_off[n]);
        }
    }

    // pack: every subproblem routed, packed into rank space and given its kernel, in parts side by side; the parts appended in order
    const PackInput in{batch, params, force_num_pw, n, read_pack_switches(n)};
    std::vector<PackPart> parts = pack_parts(in, *pl);
    Packed pk;
    std::string err;
    if ((rc = append_parts(parts, *pl, pk, err))) { set_error(ctx, "%s", err.c_str()); return rc; }

    // launch groups, family by family (the order of the families is the order of the plan's list)
    const GroupSwitches gs = read_group_switches();
    LaunchLists L;
    decide_duos(*pl, in.sw.duos);
    form_chain_groups(*pl, L);
    form_quad_duo_groups(*pl, L);
    if (gs.persistent) merge_persistent_chain(*pl, L, [&] { return cl_chain_persistent_capacity(ctx->device); });
    form_lane_groups(*pl, pk, L, in.sw.lane_rw);
    form_wide_lane_groups(*pl, pk, L);
    form_span_groups(*pl, pk, L);
    lap("pack + route");   // (the chain and near-chain families' groups have always been inside this lap: it stays where it was, so that the figures stay comparable)
    form_general_groups(*pl, pk, L);
    form_sys_groups(*pl, pk, L, gs);
    form_strip_groups(*pl, pk);
    // longest-running launch first
    for (LaunchGroup& g : pl->groups) g.est_cost = estimate_cost(*pl, L, g);
    if (gs.narrow && n >= 2048) merge_narrow(*pl, L, [&](int threads, uint32_t lds) { return cl_narrow_capacity(ctx->device, threads, lds); });
    std::stable_sort(pl->groups.begin(), pl->groups.end(), [](const LaunchGroup& x, const LaunchGroup& y) { return x.est_cost > y.est_cost; });
    pl->stats.n_launches = pl->groups.size();
    lap("launch groups");

    if ((rc = upload_plan(ctx, pl.get(), pk, L))) return rc;
    lap("allocate + upload");
    *plan_out = pl.release();
    return CL_OK;
}

// host-only: the alignment of ONE subproblem by the route do_alignment takes for it, when that route is a host algorithm
int cl_host_route_align(const cl_stitch_batch* batch, uint64_t k, const cl_stitch_params* sp, int* route_out, uint64_t** pairs_out,
                        uint64_t* n_pairs_out) {
    if (!batch || !sp || !pairs_out || !n_pairs_out || k >= batch->n_problems) return CL_ERR_INVALID_ARGUMENT;
    *pairs_out = nullptr;
    *n_pairs_out = 0;
    const GraphView g1 = view(batch->side[0], k), g2 = view(batch->side[1], k);
    const int npw = choose_num_pw(g1.n, g2.n, sp->alignment_params);
    if (npw < 1 || npw > 3) return npw < 0 ? npw : CL_ERR_INVALID_ARGUMENT;
    const int route = route_problem(g1, g2, batch->only_deletion_alns && batch->only_deletion_alns[k], *sp);
    if (route_out) *route_out = route;
    if (route < 0) return route;
    if (route == CL_ROUTE_PO_POA) return CL_ERR_UNSUPPORTED_ROUTE;   // the device's
    HostAlignment aln;
    const int rc = host_route_alignment(route, g1, g2, npw, *sp, aln);
    if (rc) return rc;
    uint64_t* out = (uint64_t*)malloc((aln.size() ? aln.size() : 1) * 2 * sizeof(uint64_t));
    if (!out) return CL_ERR_OUT_OF_MEMORY;
    const uint64_t nb1 = batch->side[0].node_off[k], nb2 = batch->side[1].node_off[k];
    for (size_t i = 0; i < aln.size(); ++i) {   // translate, src/alignment.cpp:26-39
        uint64_t a = aln[i].first, b = aln[i].second;
        if (a != CL_GAP && batch->side[0].back_translation) a = batch->side[0].back_translation[nb1 + a];
        if (b != CL_GAP && batch->side[1].back_translation) b = batch->side[1].back_translation[nb2 + b];
        out[2 * i] = a;
        out[2 * i + 1] = b;
    }
    *pairs_out = out;
    *n_pairs_out = aln.size();
    return CL_OK;
}

int cl_stitch_rank_order(const cl_stitch_batch* batch, uint64_t k, int side, int mode, uint32_t* order_out, uint32_t* far_reads_out, uint32_t* longest_read_out) {
    if (!batch || k >= batch->n_problems || side < 0 || side > 1 || mode < 0 || mode > 2 || !order_out) return CL_ERR_INVALID_ARGUMENT;
    const GraphView g = view(batch->side[side], k);
    NextLists nx;
    nx.build(g);
    std::vector<uint32_t> order, st, indeg, rank(g.n);
    if (!topological_order(g, nx, order, st, indeg)) return CL_ERR_CYCLIC_GRAPH;
    for (uint32_t r = 0; r < g.n; ++r) rank[order[r]] = r;
    choose_rank_order(g, mode, order, rank, st, indeg);
    uint32_t far = 0, longest = 0;
    for (uint64_t v = 0; v < g.n; ++v) {
        if (order[rank[v]] != v) return CL_ERR_INVALID_ARGUMENT;   // (cannot happen: order and rank are inverse permutations)
        for (uint64_t e = g.prev_off[v]; e < g.prev_off[v + 1]; ++e) {
            const uint32_t back = rank[v] - rank[g.prev_idx[e]];
            far += back > 4;
            longest = std::max(longest, back);
        }
    }
    for (uint64_t i = 0; i < g.n_src; ++i) { far += rank[g.src[i]] + 1 > 4; longest = std::max(longest, rank[g.src[i]] + 1); }
    std::copy(order.begin(), order.end(), order_out);
    if (far_reads_out) *far_reads_out = far;
    if (longest_read_out) *longest_read_out = longest;
    return CL_OK;
}

int cl_stitch_sys_choice(const cl_stitch_batch* batch, uint64_t k, int num_pw, int mode, cl_sys_choice* out, uint32_t* saved_out) {
    if (!batch || k >= batch->n_problems || num_pw < 1 || num_pw > 3 || mode < 0 || mode > 2 || !out) return CL_ERR_INVALID_ARGUMENT;
    *out = cl_sys_choice{};
    const GraphView g[2] = {view(batch->side[0], k), view(batch->side[1], k)};
    if (!g[0].n || !g[1].n || !g[0].n_src || !g[1].n_src) return CL_OK;   // (a pure deletion: no device launch)
    // the pair packed into rank space exactly as pack_one packs it, into a part of its own
    PackPart P;
    Scratch S;
    ClProbDesc d{};
    d.n1 = (uint32_t)g[0].n; d.n2 = (uint32_t)g[1].n; d.npw = (uint8_t)num_pw;
    bool linear = true;
    uint64_t span[2] = {0, 0};
    for (int s = 0; s < 2; ++s)
        if (!pack_side(g[s], s, k, mode, P, S, d, span[s], linear)) return P.rc;
    PairView V;
    for (int s = 0; s < 2; ++s) { V.off[s] = P.poff[s].data() + d.node_base[s]; V.lab[s] = P.lab[s].data() + d.node_base[s]; V.pidx[s] = P.pidx[s].data(); V.span[s] = span[s]; }
    V.n1 = d.n1; V.n2 = d.n2; V.npw = num_pw; V.cells = (g[0].n + 1) * (g[1].n + 1);
    V.n_pred = (P.poff[0].back() - P.poff[0][d.node_base[0]]) + (P.poff[1].back() - P.poff[1][d.node_base[1]]);
    V.sRow = d.n2 < d.n1 ? 1 : 0; V.sCol = 1 - V.sRow;
    V.n_rows = std::min(d.n1, d.n2) + 1; V.n_cols = std::max(d.n1, d.n2);
    const KernelChoice c = choose_sys(V, PackSwitches());
    if (!c.taken) return CL_OK;
    out->taken = 1;
    out->rows_are_graph2 = c.pad >> 15;
    out->log2_depth = c.pad & 31u;
    out->near_limit = c.aux[0];
    out->n_saved = c.aux_cnt;
    out->lds_bytes = (uint32_t)c.lds;
    // the farthest read the ring serves under that limit (a source's boundary column included), as the search counted it
    const uint32_t* cp = V.off[V.sCol];
    for (uint32_t j = 1; j <= V.n_cols; ++j) {
        for (uint32_t e = cp[j - 1]; e < cp[j]; ++e)
            if (j - V.pidx[V.sCol][e] <= out->near_limit) out->near_max = std::max(out->near_max, j - V.pidx[V.sCol][e]);
        if ((V.lab[V.sCol][j - 1] & 0x80) && j <= out->near_limit) out->near_max = std::max(out->near_max, j);
    }
    if (saved_out) std::copy(c.aux.begin() + 1, c.aux.end(), saved_out);
    return CL_OK;
}

}  // extern "C"
