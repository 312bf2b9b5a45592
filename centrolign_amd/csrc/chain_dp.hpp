// chain_dp.hpp — the chaining DP behind cl_chain_api.cpp's seams (chain_dp_batch), cut into phases over three structs:
//   ChainProblem   (cl_chain_prep.cpp)       host only: match pairs, per-instance tables, depth order, weights, combinations, records, queries
//   ChainDev       (cl_chain_device.cpp)     every device buffer and event of one DP, released at scope exit; upload, far-pass setup, enqueue, wait, download
//   ChainTrace     (cl_chain_traceback.cpp)  value index, tie-resolution trees, optimum and traceback
// chain_dp_batch (cl_chain_device.cpp) is the driver; ChainSwitches reads every CL_CHAIN_* variable of the DP, ChainPath says which way a DP goes.
#pragma once
#include <algorithm>
#include <chrono>
#include <cstring>
#include <functional>
#include <thread>
#include <unordered_map>
#include <vector>

#include "chain_device.h"
#include "cl_internal.hpp"
#include "stitch_host.hpp"

hipError_t cl_chain_launch_inter(const ClChainDevice& D, uint32_t block_first, uint32_t block_count, uint32_t src_block_lo,
                                 uint32_t src_block_hi, uint32_t max_recs, uint32_t tile_recs, hipStream_t stream);
hipError_t cl_chain_launch_intra(const ClChainDevice& D, uint32_t block_first, uint32_t block_count, uint32_t near_blocks, hipStream_t stream);
hipError_t cl_chain_launch_group(const ClChainDevice& D, uint32_t s0, uint32_t s1, uint32_t n_group_recs, int* dp_enc, hipStream_t stream);   // chain_kernels.hip: many combinations
hipError_t cl_chain_launch_walk(const ClChainDevice& D, uint32_t first, uint32_t count, hipStream_t stream, hipEvent_t done);
hipError_t cl_chain_launch_walk_fold(const ClChainDevice& D, uint32_t fold, uint32_t first, uint32_t count, hipStream_t stream, hipEvent_t done);
hipError_t cl_chain_launch_walk2(const ClChainDevice& D, uint32_t first, uint32_t count, uint32_t qpt, uint32_t n_help, hipStream_t stream, hipEvent_t done);   // chain_walk2.hip
uint32_t cl_chain_walk2_helpers(uint32_t qpt);
hipError_t cl_chain_launch_own_rec(const ClChainDevice& D, uint32_t max_recs, hipStream_t stream);
hipError_t cl_chain_acc_row(const ClChainDevice& D, uint32_t s, int* out, hipStream_t stream);
hipError_t cl_chain_expand_queries(const uint32_t* fa_qt, const uint32_t* fa_d, const uint32_t* fb_qoff, const uint32_t* fb_d, const uint32_t* combo_tags, uint32_t n_combos,
                                   uint32_t n_pairs, uint32_t* qt, uint32_t* qoff, int32_t* q, hipStream_t stream);
// chain_far.hip
hipError_t cl_chain_far_init(const ClChainDevice& D, const uint32_t* d_base, uint32_t max_padded, uint32_t r_pad, int32_t sig_bias, uint32_t band_shift,
                             uint32_t off_bits, uint32_t* key_off, uint32_t* key_band, uint32_t* idx, hipStream_t stream);
size_t cl_chain_far_sort_temp_bytes(uint32_t n);
hipError_t cl_chain_far_sort32(void* temp, size_t temp_bytes, const uint32_t* keys_in, uint32_t* keys_out, const uint32_t* vals_in, uint32_t* vals_out,
                               uint32_t n, int end_bit, hipStream_t stream);
hipError_t cl_chain_far_node_keys(const uint32_t* order, uint32_t n, uint32_t shift, uint32_t* node_key, hipStream_t stream);
hipError_t cl_chain_far_layout(const uint32_t* perm, const uint32_t* key, uint32_t n, uint32_t* arena, uint32_t ord_off, const uint32_t* ix, uint32_t n_ix,
                               hipStream_t stream);
hipError_t cl_chain_far_seal(const ClChainDevice& D, const ClFarDevice& F, const uint32_t* items, uint32_t item0, uint32_t n_items, uint32_t n_big, hipStream_t stream, hipEvent_t done);
hipError_t cl_chain_far_launch(const ClChainDevice& D, const ClFarDevice& F, uint32_t first, uint32_t count, uint32_t end_block, hipStream_t stream, hipEvent_t done);
hipError_t cl_chain_far_merge(const ClChainDevice& D, const int* slot, uint32_t first, uint32_t count, uint32_t share_n, uint32_t share_i, hipStream_t stream);
hipError_t cl_chain_sort_values(const float* val, uint32_t n, int* keys_in, uint32_t* idx_in, int* keys_out, uint32_t* idx_out,
                                void* temp, size_t* temp_bytes, hipStream_t stream);

namespace clchain {

constexpr uint32_t kNone = 0xFFFFFFFFu;

// post_switch_distances.hpp:44-81; 0xFFFFFFFF = none (the reference's size_t(-1), used modulo 2^32)
struct PostSwitchTable {
    uint64_t n = 0;
    std::vector<uint32_t> d;
    void build(const cl_base_graph& g, const clhost::PathMergeTable& pm) {
        n = g.n_nodes;
        d.assign(pm.chain_size() * n, 0);
        std::vector<uint32_t> order;
        clhost::topological_order(g, order);
        for (uint32_t v : order)
            for (uint64_t p = 0; p < pm.chain_size(); ++p) {
                uint32_t* row = &d[p * n];
                const uint32_t pr = pm.predecessor_index(v, p);
                for (uint64_t e = g.prev_off[v]; e < g.prev_off[v + 1]; ++e) {
                    const uint32_t u = g.prev_idx[e];
                    if (pm.index_on(u, p) == pr) { row[v] = 1; break; }
                    if (pm.predecessor_index(u, p) == pr) {
                        const uint64_t thru = (uint64_t)row[u] + 1;
                        if (row[v] == 0 || row[v] > thru) row[v] = (uint32_t)thru;
                    }
                }
            }
    }
    uint32_t distance(uint64_t v, uint64_t p) const { const uint32_t x = d[p * n + v]; return x == 0 ? kNone : x; }
};

using clhost::anchor_weight;
using clhost::min_source_sink;

inline int enc(float f) { int b; memcpy(&b, &f, 4); if (b == (int)0x80000000) b = 0; return b >= 0 ? b : b ^ 0x7FFFFFFF; }   // -0.0f == +0.0f, as on the device
inline float dec(int k) { int b = k >= 0 ? k : k ^ 0x7FFFFFFF; float f; memcpy(&f, &b, 4); return f; }

// the value index of n stored values, built on the host: recs = the record numbers in ascending order of enc(value), equal keys in record order, and
// keys[i] = enc(val[recs[i]]) — the same order as the device's stable radix sort (chain_sort.hip).  ChainTrace::value_index for a small DP, and
// cl_chain_value_index_host, through which the tests hold the two against each other
inline void value_index_host(const float* val, uint32_t n, int* keys, uint32_t* recs) {
    std::vector<int> key(n);
    for (uint32_t r = 0; r < n; ++r) { key[r] = enc(val[r]); recs[r] = r; }
    std::stable_sort(recs, recs + n, [&](uint32_t a, uint32_t b) { return key[a] < key[b]; });
    for (uint32_t i = 0; i < n; ++i) keys[i] = key[recs[i]];
}

// heap node of the r-th smallest key in a MaxSearchTree / outer OrthogonalMaxSearchTree of n keys
// (implicit complete binary tree filled by an in-order walk, max_search_tree.hpp:113-150)
inline std::vector<uint32_t> heap_of_rank(size_t n) {
    std::vector<uint32_t> h(n);
    size_t next = 0;
    std::vector<std::pair<size_t, bool>> st;
    if (n) st.emplace_back(0, false);
    while (!st.empty()) {
        auto& top = st.back();
        if (!top.second) {
            top.second = true;
            if (2 * top.first + 1 < n) st.emplace_back(2 * top.first + 1, false);
        } else {
            const size_t x = top.first;
            h[next++] = (uint32_t)x;
            st.pop_back();
            if (2 * x + 2 < n) st.emplace_back(2 * x + 2, false);
        }
    }
    return h;
}

inline bool in_subtree(size_t y, size_t x) {
    while (y > x) y = (y - 1) / 2;
    return y == x;
}

// Replays the unit order of range_max over rank interval [rlo, rhi) (max_search_tree.hpp:361-444,
// orthogonal_max_search_tree.hpp:343-544) on a tree of n keys: calls node(x) for the nodes on the search path that lie
// in range and subtree(x) for the off-path subtrees, in the order the reference inspects them; stops at the first
// callback that returns true.
template <class NodeF, class SubF>
void replay_units(size_t n, const std::vector<uint32_t>& rank_of_heap, size_t rlo, size_t rhi, NodeF node, SubF subtree) {
    auto in = [&](size_t x) { return rank_of_heap[x] >= rlo && rank_of_heap[x] < rhi; };
    size_t c = 0;
    while (c < n && !in(c)) c = rank_of_heap[c] >= rhi ? 2 * c + 1 : 2 * c + 2;
    if (c >= n) return;
    if (node(c)) return;
    size_t lc = 2 * c + 1, rc = 2 * c + 2;
    while (lc < n) {
        if (rank_of_heap[lc] >= rlo) {
            if (node(lc)) return;
            if (2 * lc + 2 < n && subtree(2 * lc + 2)) return;
            lc = 2 * lc + 1;
        } else lc = 2 * lc + 2;
    }
    while (rc < n) {
        if (rank_of_heap[rc] < rhi) {
            if (node(rc)) return;
            if (2 * rc + 1 < n && subtree(2 * rc + 1)) return;
            rc = 2 * rc + 2;
        } else rc = 2 * rc + 1;
    }
}

// records ordered by (key, slot): slots are unique, so a placement by slot followed by a stable counting sort on the key
// replaces the comparison sort (the big trees of a 1 Mbp problem hold every match pair)
template <class KeyF, class SlotF>
void sort_by_key_then_slot(std::vector<uint32_t>& items, uint64_t n_slots, KeyF key, SlotF slot, bool already_by_slot = false) {
    if (items.size() < 4096) {
        std::sort(items.begin(), items.end(), [&](uint32_t a, uint32_t b) { return key(a) != key(b) ? key(a) < key(b) : slot(a) < slot(b); });
        return;
    }
    std::vector<uint32_t> by_slot;
    if (already_by_slot) by_slot = items;   // (the caller's list comes in slot order: a run of one shift of the (shift, slot) order)
    else {
        std::vector<uint32_t> at(n_slots, 0xFFFFFFFFu);
        for (uint32_t it : items) at[slot(it)] = it;
        by_slot.reserve(items.size());
        for (uint64_t sl = 0; sl < n_slots; ++sl) if (at[sl] != 0xFFFFFFFFu) by_slot.push_back(at[sl]);
    }
    int64_t lo = INT64_MAX, hi = INT64_MIN;
    for (uint32_t it : by_slot) { lo = std::min<int64_t>(lo, key(it)); hi = std::max<int64_t>(hi, key(it)); }
    if ((uint64_t)(hi - lo) > 64 * (uint64_t)by_slot.size() + (1u << 16)) {   // keys far sparser than items: a comparison sort on the key alone (stable: slot order is kept)
        std::stable_sort(by_slot.begin(), by_slot.end(), [&](uint32_t a, uint32_t b) { return key(a) < key(b); });
        items.swap(by_slot);
        return;
    }
    std::vector<uint32_t> start((size_t)(hi - lo) + 2, 0);
    for (uint32_t it : by_slot) ++start[(size_t)(key(it) - lo) + 1];
    for (size_t i = 1; i < start.size(); ++i) start[i] += start[i - 1];
    for (uint32_t it : by_slot) items[start[(size_t)(key(it) - lo)]++] = it;
}

// a gap-free search tree of the reference, as its sorted key list + implicit heap layout (built on first use)
struct GapFreeTree {
    struct Member { uint32_t off, slot, rec; };
    std::vector<Member> mem;
    std::vector<uint32_t> heap, rank_of_heap;
    bool built = false;
};

struct Combo {
    uint32_t p1 = 0, p2 = 0;
    ClRawVec<uint32_t> rec_s, ins_t, off;   // (filled completely by the record / query passes)
    ClRawVec<int32_t> sigma;
    uint32_t *qt = nullptr, *qoff = nullptr;   // dense queries [M]: slices of ONE block per array for all combinations (ChainProblem: dense_qt / dense_qoff / dense_q) —
    int32_t* q = nullptr;                      // a polishing step runs thousands of small DPs over hundreds of combinations: three heap blocks per combination were most of their "queries" phase
    std::vector<uint32_t> prefix;
    // lazily built for tie resolution, per chaining instance of the batch
    struct SubRecs {
        std::vector<uint32_t> recs;         // the instance's records in this combination
        std::vector<uint32_t> ortho_order;  // ... sorted by (sigma, slot)
        std::vector<uint32_t> ortho_heap, ortho_rank_of_heap;
        std::unordered_map<int32_t, GapFreeTree> diag_tree;
    };
    std::unordered_map<uint32_t, SubRecs> per_sub;
    bool split_built = false;
};

// what the DP needs of its graph 1 alone — topological positions and depths (longest path from a source) — so that the two whole-graph DPs of one cl_anchor_chain
// (the gap-free one of the scale estimate, the affine one) share one walk over the graph
struct GraphOrder {
    std::vector<uint32_t> pos, depth;
    void build(const cl_base_graph& g) {
        std::vector<uint32_t> order;
        clhost::topological_order(g, order);
        pos.resize(g.n_nodes);
        for (uint32_t i = 0; i < order.size(); ++i) pos[order[i]] = i;
        // depth = longest path from a source: a predecessor m of m' ends strictly before m' starts, so
        // depth(b1(m')) >= depth(b1(m)) + len(m); pairs whose start depths fall into one window of min_len consecutive
        // depths can never precede one another and are finalised together on the device ("group")
        depth.assign(g.n_nodes, 0);
        for (uint32_t v : order)
            for (uint64_t e = g.next_off[v]; e < g.next_off[v + 1]; ++e)
                depth[g.next_idx[e]] = std::max(depth[g.next_idx[e]], depth[v] + 1);
    }
};

struct ChainSub {
    const cl_base_graph* g[2] = {nullptr, nullptr};   // DP orientation: g[0] plays graph1
    const GraphOrder* order1 = nullptr;                // of g[0], prebuilt (built here if null)
    bool tableau = true;                               // graphs carry sentinels: PathMerge gets the pseudo-path (path_merge.hpp:148-160)
    bool chain_merge = false;                          // tables built here are ChainMerge tables (the CLI's -g 1: anchorer.hpp:659-660 with XMerge = ChainMerge)
    const cl_match_sets* ms = nullptr;                 // the sets; DP set s = ms set order[s] (identity if null), and with
    const uint64_t* order = nullptr;                   // swap_sides the DP's graph-1 walks are the sets' walks2
    bool swap_sides = false;                           // (anchorer.hpp:1179-1182), without copying anything
    uint64_t num_match_sets = 0;
    const clhost::PathMergeTable* x[2] = {nullptr, nullptr};   // prebuilt tables of g[0], g[1] (built here if null)
    const PostSwitchTable* sw[2] = {nullptr, nullptr};
    bool anchored = false;                             // sources / sinks given (global anchoring, fill-in)
    std::vector<uint32_t> src[2], snk[2];
    std::vector<uint32_t> tag[2];                      // local chain id -> batch-wide chain tag; empty = identity
    // masked matches (anchorer.hpp:144; MatchBank skips them, match_bank.hpp:187-215,252-268): (set of `ms`, idx1, idx2) in the sets' own
    // sides -> true if the pair does not take part in the DP.  Empty = no mask
    std::function<bool(uint64_t, uint32_t, uint32_t)> masked;
};

struct ChainSubResult {
    std::vector<uint32_t> chain;     // (set, idx1, idx2) per anchor, DP orientation
    std::vector<int64_t> gap;        // affine only: [n+1] gap before anchor i; [0] from the sources, [n] to the sinks
    std::vector<double> gap_score;   // (anchorer.hpp:2443-2468)
    uint64_t n_ties = 0;
};

struct ChainTimings { float device_ms = 0, prep_ms = 0, index_ms = 0, traceback_ms = 0; uint64_t n_pairs = 0; double pair_evals = 0; uint32_t n_combos = 0; };

struct SubCtx {
    clhost::PathMergeTable own_x[2];
    PostSwitchTable own_sw[2];
    const clhost::PathMergeTable* x[2] = {nullptr, nullptr};
    const PostSwitchTable* sw[2] = {nullptr, nullptr};
    GraphOrder own_order;
    const uint32_t *pos1 = nullptr, *depth1 = nullptr;
    std::vector<char> has_start, after_end;
    std::vector<std::pair<uint32_t, uint32_t>> walk_marks;   // (first, last node) of every graph-1 walk when some pairs are masked
    uint32_t pair_lo = 0, pair_hi = 0;
    uint32_t off_a = 0, off_b = 0;
    float min_score = 0.0f;
};

struct Pair { uint32_t sub, set, i1, i2, b1, e1, b2, e2; };

// the match sets of an instance as the DP sees them
struct SetView {
    const cl_match_sets* ms;
    const uint64_t* order;
    const uint64_t *so[2], *wo[2];
    const uint32_t* nd[2];
    explicit SetView(const ChainSub& sb) : ms(sb.ms), order(sb.order) {
        const int a = sb.swap_sides ? 1 : 0;
        so[a] = ms->set_off1; wo[a] = ms->walk_off1; nd[a] = ms->nodes1;
        so[1 - a] = ms->set_off2; wo[1 - a] = ms->walk_off2; nd[1 - a] = ms->nodes2;
    }
    uint64_t orig(uint64_t s) const { return order ? order[s] : s; }
    uint64_t n_walks(int side, uint64_t s) const { const uint64_t o = orig(s); return so[side][o + 1] - so[side][o]; }
    uint64_t walk(int side, uint64_t s, uint64_t j) const { return so[side][orig(s)] + j; }
    uint32_t front(int side, uint64_t w) const { return nd[side][wo[side][w]]; }
    uint32_t back(int side, uint64_t w) const { return nd[side][wo[side][w + 1] - 1]; }
    uint64_t length(uint64_t s) const { const uint64_t w = so[0][orig(s)]; return wo[0][w + 1] - wo[0][w]; }   // walks of a set share their length
    double weight(const cl_chain_params& cp, uint64_t s) const {
        const uint64_t o = orig(s);
        return anchor_weight(cp, ms->count1[o], ms->count2[o], length(s), ms->full_length[o]);
    }
};

constexpr int kWalkStalled = -1000;   // internal: the walk kernel's workgroups were not all resident (chain_dp_batch retries without it)

#define CL_CHAIN_TRY(x) do { if (const int rc_ = (x)) return rc_; } while (0)   // (release is the owner's business: ChainDev)

inline float ms_since(std::chrono::steady_clock::time_point t) { return (float)std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t).count(); }

// Every CL_CHAIN_* variable the DP reads, read ONCE per process at the first DP (tests that need another value start a child process).  CL_CHAIN_TIMING alone
// is read at every call (ChainProblem::timing).  docs/ENVIRONMENT.md lists them; the comments at the places that use them say what they are for.
struct ChainSwitches {
    uint64_t par_records_min;      // CL_CHAIN_PAR_RECORDS_MIN: records from which the combinations are numbered in parallel (0 in tests: every size)
    bool dense_queries;            // CL_CHAIN_DENSE_QUERIES=1: the dense query tables of rounds 1-3 (A/B)
    bool old_walk;                 // CL_CHAIN_OLD_WALK=1: the per-block path (A/B)
    uint32_t walk_fold;            // CL_CHAIN_WALK_FOLD=2/3: fold smaller DPs too (tests); 0 = by size
    bool group_forced, group_path; // CL_CHAIN_GROUP_PATH=force: every DP group by group (tests); =0: the one-workgroup per-block kernels of rounds 1-5 (A/B)
    bool walk2;                    // CL_CHAIN_WALK2=0 keeps chain_walk_kernel (A/B)
    uint32_t walk2_qpt, walk2_max; // CL_CHAIN_WALK2_QPT=1/2 the window, CL_CHAIN_WALK2_MAX the most combinations (default 8)
    int walk2_helpers;             // CL_CHAIN_WALK2_HELPERS=n (-1: as many as fit)
    const char* walk_reduce;       // CL_CHAIN_WALK_REDUCE=0/1 pins the exchange between the walk's workgroups (A/B)
    bool walk2_debug;              // CL_CHAIN_WALK2_DEBUG: in-kernel counters and clocks of the walk (status[8..]), printed with CL_CHAIN_TIMING
    bool no_far;                   // CL_CHAIN_NO_FAR_PRUNE
    uint32_t far_lag;              // CL_CHAIN_FAR_LAG=1..kFarLag far launches in flight (0: the default)
    uint64_t far_arena_skip;       // CL_CHAIN_FAR_ARENA_SKIP=<words> left unused in front of the arena (tests: positions beyond 2^32 words on a small DP)
    bool seal_wave;                // CL_CHAIN_SEAL_WAVE: every node sealed by one wave (rounds 2-3, A/B)
    const char* far_mode;          // CL_CHAIN_FAR_MODE: "sweep" / "bb" pin the far pass (A/B)
    bool ext_events;               // CL_CHAIN_EXT_EVENTS=0: hipEventRecord as in rounds 2-3 (A/B)
    bool far_early;                // CL_CHAIN_FAR_WAIT_LATE=1 clears it: far(k) issued as in round 4 (A/B)
    bool skip_far;                 // CL_CHAIN_DEBUG_SKIP_FAR=1 (measurements only, WRONG RESULTS): the DP without its far launches
    bool near_split;               // CL_CHAIN_NEAR_SPLIT=1 (measured SLOWER: 2 x 1 Mbp affine DP 162 -> 230 ms; off unless asked for)
    const char* debug_stall;       // CL_CHAIN_DEBUG_STALL (test hook): "first" = only the shared attempt "stalls"; any other value = every walk does
    const char* lazy_acc;          // CL_CHAIN_LAZY_ACC=0/1 pins how the traceback gets its rows (tests)
};
const ChainSwitches& chain_switches();   // cl_chain_device.cpp

// Which way a DP goes, decided from its sizes and the switches (choose_path, cl_chain_device.cpp).  use_far starts as "large enough" and is cleared by the far-pass
// setup where the pass cannot be had (key widths, arena size, free device memory, ctx->far_last_choice); far_ran is the mode the DP ended in.
struct ChainPath {
    bool use_walk = false;
    uint32_t walk_fold = 0;
    bool use_walk2 = false;
    uint32_t walk2_qpt = 1, walk2_help = 0;
    bool walk_reduce = false, group_path = false, packed = false;
    bool use_far = false;
    uint32_t far_lag = 2;
    const char* far_ran = "none";
    bool lazy_acc = false;
};

// ---- the host side of one DP: everything that is known before the device is touched ------------------------------------------------------
struct ChainProblem {
    cl_context* ctx;
    const std::vector<ChainSub>& subs;
    const cl_chain_params* cp;
    const double local_scale;
    const bool sparse;
    ChainTimings& tm;
    const ChainSwitches& sw;
    const size_t K;
    const bool timing;             // CL_CHAIN_TIMING, read at every call
    const std::chrono::steady_clock::time_point T0;
    std::chrono::steady_clock::time_point tlap;
    ChainProblem(cl_context* c, const std::vector<ChainSub>& s, const cl_chain_params* p, double scale, bool sp, ChainTimings& t)
        : ctx(c), subs(s), cp(p), local_scale(scale), sparse(sp), tm(t), sw(chain_switches()), K(s.size()), timing(getenv("CL_CHAIN_TIMING") != nullptr),
          T0(std::chrono::steady_clock::now()), tlap(T0), sc(s.size()) {}
    void lap(const char* what) {
        if (timing) fprintf(stderr, "[chain_dp_batch]   %-26s %8.1f ms\n", what, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tlap).count());
        tlap = std::chrono::steady_clock::now();
    }

    std::vector<SubCtx> sc;
    std::vector<Pair> pairs;       // in MatchBank iteration order (match_bank.hpp:252-268), instance by instance: slot = position in that order
    uint64_t M = 0, span_a = 0, span_b = 0;
    uint32_t n_tag[2] = {0, 0};
    std::vector<uint32_t> by_s, s_of_slot;   // sorted index -> slot and back
    std::vector<float> weight, init_w, final_term;   // init_w: the value of a chain that STARTS at the pair; final_term: per slot
    std::vector<uint32_t> combo_of;
    std::vector<Combo> combos;
    bool par_numbering = false;
    std::vector<uint32_t> rec_off;
    ClRawVec<uint32_t> rec_combo, rec_pos;
    uint32_t n_blocks = 0;
    bool factored = false;
    ClRawVec<uint32_t> fa_qt, fa_d, fb_qoff, fb_d;   // [tag][M]
    ClRawVec<uint32_t> dense_qt, dense_qoff;         // [combination][M] (the dense tables: small and batched DPs)
    ClRawVec<int32_t> dense_q;

    // the phases, in order (cl_chain_prep.cpp)
    int collect_pairs();
    int build_tables();
    void sort_by_depth();
    void weights();
    void anchoring_terms();
    void records();
    void count_work();
    void queries();

    uint32_t tag_of(uint32_t k, int side, uint32_t p) const { return subs[k].tag[side].empty() ? p : subs[k].tag[side][p]; }
    float score_gap(int32_t gap) const;
    int32_t measure_gap(const SubCtx& c, uint32_t a1, uint32_t a2, uint32_t c1, uint32_t c2) const;
    int32_t gap_from_sources(uint32_t k, uint32_t c1, uint32_t c2) const;
    int32_t gap_to_sinks(uint32_t k, uint32_t a1, uint32_t a2) const;
    void query_at(size_t ci, uint32_t s, uint32_t& qt, uint32_t& qoff, int32_t& q) const;   // the query of pair s in combination ci, whichever way it is kept
    uint32_t max_recs(uint32_t lo, uint32_t hi) const {
        uint32_t m = 0;
        for (const Combo& c : combos) m = std::max(m, c.prefix[hi] - c.prefix[lo]);
        return m;
    }
};

// ---- the device side: the one owner of every buffer and event of a DP --------------------------------------------------------------------
struct ComboDev {
    DevBuf<uint32_t> d_rec_s, d_ins_t, d_off, d_prefix, d_qt, d_qoff, d_own_rec;
    DevBuf<int32_t> d_sigma, d_q;
    DevBuf<float> d_val;
    DevBuf<int> d_acc;
    void release(bool quiesced) {
        d_rec_s.release(quiesced); d_ins_t.release(quiesced); d_off.release(quiesced); d_prefix.release(quiesced); d_qt.release(quiesced); d_qoff.release(quiesced);
        d_sigma.release(quiesced); d_q.release(quiesced); d_val.release(quiesced); d_acc.release(quiesced); d_own_rec.release(quiesced);
    }
};
struct PackLayout;
struct UnitsHeld;

struct ChainDev {
    cl_context* ctx;
    explicit ChainDev(cl_context* c) : ctx(c) {}
    ChainDev(const ChainDev&) = delete;
    ChainDev& operator=(const ChainDev&) = delete;
    // Waits ONCE for the context's streams (cl_ctx_quiesce), gives every block back with quiesced = true and destroys the events.  A poisoned context (a merge-group
    // wait that expired) keeps its blocks: they are left to the stuck stream, releasing them would wait for it
    ~ChainDev();

    std::vector<ComboDev> cd;         // per combination
    DevBuf<ClChainCombo> d_combos;
    DevBuf<float> d_weight, d_init, d_dp;
    DevBuf<uint32_t> d_rec_off, d_rec_combo, d_rec_pos, d_group, d_grp_base, d_grp_total, d_group_end, d_status;
    DevBuf<unsigned long long> d_xch, d_xdp, d_hacc;
    DevBuf<int> d_dp_enc;             // DPs over more combinations than the walk kernels take: the running dp maxima of the per-group path, order-preserving encoding
    DevBuf<char> d_pack;              // a small DP's arrays in one block
    size_t pack_dp_off = 0, pack_acc_stride = 0, pack_down_bytes = 0;
    DevBuf<uint32_t> d_xred;
    DevBuf<int> d_row;                // the traceback's row of query results, when it fetches them step by step
    DevBuf<uint32_t> d_blk_rec, d_blk_q, d_blk_own, d_fa[4], d_ctags;   // factored queries: every combination's arrays as views into a few blocks
    DevBuf<float> d_blk_val;
    DevBuf<int> d_blk_acc;
    DevBuf<int> k_in, k_out;          // value index of the traceback (built on demand)
    DevBuf<uint32_t> i_in, i_out;
    DevBuf<char> vtemp;
    // branch-and-bound far pass (chain_far.hip)
    DevBuf<int> d_far_rec;
    DevBuf<uint32_t> d_far_base, d_far_u32[7], d_far_perm[2 * kFarMaxLevels], d_far_arena, d_far_tab, d_seal_items;
    DevBuf<char> d_far_temp;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    std::vector<hipEvent_t> ev_intra, ev_far;   // per-block path (the walk path's events are the context's ring events: nothing to destroy)

    ClChainDevice D{};
    ClFarDevice F{};
    std::vector<uint32_t> group_first;   // first pair of every group + M (the per-group path of DPs over more combinations than the walk kernels take)
    std::vector<uint32_t> seal_off;      // [n_macro + 1] into d_seal_items
    std::vector<uint32_t> seal_big;      // [n_macro] how many of a macro-block's items (its first ones) are nodes of 4 096 records or more
    // what came back
    std::vector<float> dp_sorted;
    std::vector<const int*> acc;         // per combination: the stored query results (7 per pair), unless the traceback fetches them row by row
    std::vector<std::vector<int>> acc_own;
    std::vector<char> pack_host;
    std::vector<int> row_host;
    uint32_t row_s = kNone;
    int* row_pin = nullptr;

    // the phases, in order (cl_chain_device.cpp)
    int upload_packed(const ChainProblem& P, const ChainPath& path, const PackLayout& pack);
    int upload_factored(const ChainProblem& P, const ChainPath& path);
    int upload_separate(const ChainProblem& P, const ChainPath& path);
    int upload_groups(const ChainProblem& P, const ChainPath& path);
    void fill_device(const ChainProblem& P, const ChainPath& path);
    int far_setup(const ChainProblem& P, ChainPath& path);
    int create_events(const ChainProblem& P);
    hipError_t enqueue(const ChainProblem& P, ChainPath& path, UnitsHeld& units);
    hipError_t enqueue_walk(const ChainProblem& P, ChainPath& path, hipError_t he);
    hipError_t enqueue_blocks(const ChainProblem& P, hipError_t he);
    void print_path(const ChainProblem& P, const ChainPath& path);
    int wait(const ChainProblem& P, const ChainPath& path, UnitsHeld& units, hipError_t he);
    int download(const ChainProblem& P, const ChainPath& path);
    const int* acc_row(const ChainProblem& P, uint32_t s);   // row of pair s: 7 words per combination
};
int chain_hip_fail(cl_context* ctx, hipError_t e, const char* what);

// ---- the traceback ------------------------------------------------------------------------------------------------------------------------
struct ChainTrace {
    // value index: per combination and tree kind, (encoded stored value, record) sorted by value — built on first use: the
    // traceback touches only the (combination, kind) pairs that win a step of the chain
    std::vector<std::vector<std::vector<int>>> vkeys;
    std::vector<std::vector<std::vector<uint32_t>>> vrecs;
    std::vector<std::vector<char>> vbuilt;
    size_t vtemp_bytes = 0;
    float index_ms = 0;
    double t_split = 0, t_ortho = 0, t_diag = 0, t_gapfree = 0, t_cand = 0;   // CL_CHAIN_TIMING: where the traceback's time goes
    uint64_t n_scanned = 0, n_steps = 0;
    std::unordered_map<uint64_t, GapFreeTree> sparse_trees;   // sparse mode: (chain2 tag, instance) -> tree
    // LAST member: the thread reads the problem's combinations and writes the trees above, and is joined before either goes
    std::thread ortho_prebuild;
    ~ChainTrace() { if (ortho_prebuild.joinable()) ortho_prebuild.join(); }

    void start_prebuild(ChainProblem& P);
    int prepare_index(const ChainProblem& P, ChainDev& dev);
    bool value_index(const ChainProblem& P, ChainDev& dev, size_t ci, int kind);
    Combo::SubRecs& sub_recs(const ChainProblem& P, Combo& c, uint32_t k);
    void ortho_of(const ChainProblem& P, Combo::SubRecs& sr, const Combo& c);
    int trace_instance(ChainProblem& P, const ChainPath& path, ChainDev& dev, uint32_t k, ChainSubResult& res);
    int run(ChainProblem& P, const ChainPath& path, ChainDev& dev, std::vector<ChainSubResult>& results, std::vector<float>* dp_out);
};

int chain_dp_batch(cl_context* ctx, const std::vector<ChainSub>& subs, const cl_chain_params* cp, double local_scale,
                   bool sparse, std::vector<ChainSubResult>& results, ChainTimings& tm, std::vector<float>* dp_out);

}  // namespace clchain
