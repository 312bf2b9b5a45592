// cl_induced_api.cpp — the -A output of the CLI (src/core.cpp:523-591):
//   cl_induced_pairwise_cigars  the CIGARs of many pairs of paths of an acyclic graph in one device pass (kernels: induced_kernels.hip); the
//                               host restatement cl_induced_pairwise_cigar (cl_io_api.cpp) is what it is checked against
//   cl_induced_pairwise_stats   the same alignments as counters (bases and runs per op) in one device pass of their own kernel, no text; it shares
//                               the position tables and the chunking with the call above (induced_batch); host restatement: cl_induced_pairwise_stat
//   cl_induced_pairwise_profiles, cl_induced_gap_events_batch
//                               the same alignments by position: per window of path 1 the columns of each letter, and the I / D runs of a least
//                               length with their places; one kernel each over the same frame, no text; host restatements:
//                               cl_induced_pairwise_profile, cl_induced_gap_events
//   cl_induced_pairwise_agreements
//                               two graphs' alignments of the same pairs compared: a partner pass over graph a and an agreement pass over graph b
//                               through the same frame, each graph on the device once; host restatement: cl_induced_pairwise_agreement
//   cl_induced_cyclic_maf       output_maf(induced_cyclic_pairwise_alignment(...)) (src/alignment.cpp:229-904), the output after cyclisation.
//                               Host code: its core is a Hunt-Szymanski LCS, a dependent chain of binary searches over a threshold row
//                               (DESIGN.md §9); the caller runs pairs in parallel, as the reference does (core.cpp:554-591).
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "cl_internal.hpp"

namespace {

char* c_string(const std::string& s, uint64_t* len_out) {
    char* p = (char*)malloc(s.size() + 1);
    if (!p) return nullptr;
    memcpy(p, s.data(), s.size());
    p[s.size()] = '\0';
    if (len_out) *len_out = s.size();
    return p;
}

constexpr uint64_t kGap = ~(uint64_t)0;
// device working memory of one chunk of cl_induced_pairwise_cigars / _stats: the position tables of the chunk's first paths (4 bytes per node each);
// the text of a write pass is bounded the same way (a single pair's CIGAR may exceed it alone), and so are the windows of a profile pass and the
// events of an event write pass.  A chunk also holds at most kChunkPairs pairs.
constexpr uint64_t kChunkTableBytes = 256ull << 20, kChunkTextBytes = 256ull << 20, kChunkPairs = 2048;
constexpr uint64_t kChunkWindows = (256ull << 20) / sizeof(cl_pair_window), kChunkEvents = (256ull << 20) / sizeof(cl_gap_event);
// cl_induced_pairwise_agreements: the partner words of one group of quads, 4 bytes per step of each quad's path 2 (one quad may exceed it alone)
constexpr uint64_t kChunkPartnerBytes = 256ull << 20;

// ---------------------------------------------------------------- the cyclic MAF -------------------------------------------------------------
using Pair = std::pair<uint64_t, uint64_t>;   // (index on path 1, index on path 2), kGap: none
using Aln = std::vector<Pair>;

// sets and maps keyed by node id for one thread, reused from call to call: a stamp per node tells whether the node is in the current set
struct NodeSets {
    std::vector<uint32_t> stamp[3], value;
    uint32_t cur[3] = {0, 0, 0};
    void fit(uint64_t n_nodes) {
        if (value.size() >= n_nodes) return;
        for (auto& s : stamp) s.assign(n_nodes, 0);
        value.assign(n_nodes, 0);
        cur[0] = cur[1] = cur[2] = 0;
    }
    void clear(int s) {
        if (++cur[s] == 0) { std::fill(stamp[s].begin(), stamp[s].end(), 0); cur[s] = 1; }
    }
    bool has(int s, uint32_t v) const { return stamp[s][v] == cur[s]; }
    bool insert(int s, uint32_t v) {   // true: it was not there
        if (stamp[s][v] == cur[s]) return false;
        stamp[s][v] = cur[s];
        return true;
    }
};
thread_local NodeSets tls_sets;

// align_hs (include/centrolign/alignment.hpp:634-733) of a[0..na) and b[0..nb): sparse LCS over thresholds; a match whose j equals the threshold it
// would replace is dropped.  The occurrence lists of b (descending j per value) are one sorted array instead of a vector per node id.
Aln align_hs(const uint32_t* a, uint64_t na, const uint32_t* b, uint64_t nb) {
    std::vector<uint64_t> occ(nb);   // positions of b sorted by (value, descending position): no two keys are equal
    for (uint64_t j = 0; j < nb; ++j) occ[j] = j;
    std::sort(occ.begin(), occ.end(), [&](uint64_t x, uint64_t y) { return b[x] != b[y] ? b[x] < b[y] : x > y; });
    std::vector<uint64_t> mi, mj;
    std::vector<int64_t> back;              // the match before, -1: the (0, 0) head
    std::vector<int64_t> heads(1, -1);      // score_heads, as match indices
    std::vector<uint64_t> row(1, 0);
    for (uint64_t i = 1; i <= na; ++i) {
        const uint32_t c = a[i - 1];
        auto lo = std::lower_bound(occ.begin(), occ.end(), c, [&](uint64_t x, uint32_t v) { return b[x] < v; });
        for (; lo != occ.end() && b[*lo] == c; ++lo) {
            const uint64_t j = *lo + 1;
            auto it = std::lower_bound(row.begin(), row.end(), j);
            if (it == row.end()) {
                mi.push_back(i); mj.push_back(j); back.push_back(heads.back());
                heads.push_back((int64_t)mi.size() - 1);
                row.push_back(j);
            } else if (*it != j) {
                mi.push_back(i); mj.push_back(j); back.push_back(heads[it - row.begin() - 1]);
                heads[it - row.begin()] = (int64_t)mi.size() - 1;
                *it = j;
            }
        }
    }
    Aln tb;
    int64_t here = heads.back();
    const uint64_t hi = here < 0 ? 0 : mi[here], hj = here < 0 ? 0 : mj[here];
    for (uint64_t i = na; i > hi; --i) tb.emplace_back(i - 1, kGap);
    for (uint64_t j = nb; j > hj; --j) tb.emplace_back(kGap, j - 1);
    while (here >= 0) {
        tb.emplace_back(mi[here] - 1, mj[here] - 1);
        const int64_t next = back[here];
        const uint64_t ni = next < 0 ? 0 : mi[next], nj = next < 0 ? 0 : mj[next];
        for (uint64_t i = mi[here] - 1; i > ni; --i) tb.emplace_back(i - 1, kGap);
        for (uint64_t j = mj[here] - 1; j > nj; --j) tb.emplace_back(kGap, j - 1);
        here = next;
    }
    std::reverse(tb.begin(), tb.end());
    return tb;
}

// long_common_subsequence_nonrepeating (alignment.hpp:2677-2802): the stretch of the LCS with the most matches in which neither string repeats a value
Aln lcs_nonrepeating(const uint32_t* a, uint64_t na, const uint32_t* b, uint64_t nb) {
    Aln lcs = align_hs(a, na, b, nb);
    std::vector<uint64_t> psum(lcs.size() + 1, 0);
    for (size_t i = 0; i < lcs.size(); ++i) psum[i + 1] = psum[i] + (lcs[i].first != kGap && lcs[i].second != kGap);
    std::vector<size_t> idx1(na), idx2(nb);
    for (size_t i = 0, x1 = 0, x2 = 0; i < lcs.size(); ++i) {
        if (lcs[i].first != kGap) idx1[x1++] = i;
        if (lcs[i].second != kGap) idx2[x2++] = i;
    }
    std::vector<size_t> lim1(na, 0), lim2(nb, 0);
    NodeSets& ns = tls_sets;
    for (int s = 0; s < 2; ++s) {
        const uint32_t* str = s == 0 ? a : b;
        const uint64_t n = s == 0 ? na : nb;
        auto& lim = s == 0 ? lim1 : lim2;
        ns.clear(0);
        size_t max_lim = 0;
        for (size_t i = 0; i < n; ++i) {
            if (!ns.insert(0, str[i])) max_lim = std::max<size_t>(max_lim, ns.value[str[i]] + 1);
            ns.value[str[i]] = (uint32_t)i;
            lim[i] = max_lim;
        }
    }
    size_t ob = 0, oe = 0;
    for (size_t i = 0; i < lcs.size(); ++i) {
        if (lcs[i].first != kGap && lcs[i].second != kGap) {
            const size_t begin = std::max(idx1[lim1[lcs[i].first]], idx2[lim2[lcs[i].second]]);
            if (oe == ob || psum[i + 1] - psum[begin] > psum[oe] - psum[ob]) { ob = begin; oe = i + 1; }
        }
    }
    while (ob < oe && (lcs[ob].first == kGap || lcs[ob].second == kGap)) ++ob;
    Aln out(lcs.begin() + ob, lcs.begin() + oe);
    return out;
}

// induced_cyclic_pairwise_alignment_internal (alignment.cpp:229-330)
void cyclic_internal(const uint32_t* p1, const uint32_t* p2, Pair cb, Pair ce, std::vector<Aln>& alns) {
    Aln aln = lcs_nonrepeating(p1 + cb.first, ce.first - cb.first, p2 + cb.second, ce.second - cb.second);
    if (aln.empty()) return;
    for (auto& ap : aln) {
        if (ap.first != kGap) ap.first += cb.first;
        if (ap.second != kGap) ap.second += cb.second;
    }
    size_t removed = 0;   // short double gaps become mismatches
    for (size_t i = 0; i < aln.size();) {
        if (aln[i].first != kGap && aln[i].second != kGap) { aln[i - removed] = aln[i]; ++i; continue; }
        size_t j = i, gap1 = 0, gap2 = 0;
        while (j < aln.size() && (aln[j].first == kGap || aln[j].second == kGap)) { if (aln[j].first == kGap) ++gap1; else ++gap2; ++j; }
        if (gap1 == gap2 && gap1 <= 4) {
            size_t g1 = i - removed, g2 = g1;
            for (size_t k = i; k < j; ++k) {
                if (aln[k].first == kGap) aln[g2++].second = aln[k].second;
                else aln[g1++].first = aln[k].first;
            }
            removed += gap1;
        } else {
            for (size_t k = i; k < j; ++k) aln[k - removed] = aln[k];
        }
        i = j;
    }
    aln.resize(aln.size() - removed);
    const Pair ab(aln.front().first, aln.front().second), ae(aln.back().first + 1, aln.back().second + 1);
    alns.emplace_back(std::move(aln));
    if (ab.first != cb.first && ab.second != cb.second) cyclic_internal(p1, p2, cb, ab, alns);
    if (ae.first != ce.first && ae.second != ce.second) cyclic_internal(p1, p2, ae, ce, alns);
}

// maximum_noncyclic_extension (alignment.cpp:332-567).  The covered intervals are disjoint and non-empty, so sorting them has no ties.
std::vector<Pair> noncyclic_extension(const uint32_t* path, uint64_t n, const std::vector<Pair>& cov) {
    NodeSets& ns = tls_sets;
    std::vector<std::vector<Pair>> ext(cov.size());
    std::vector<size_t> order(cov.size());
    for (size_t i = 0; i < order.size(); ++i) order[i] = i;
    std::sort(order.begin(), order.end(), [&](size_t i, size_t j) { return cov[i] < cov[j]; });
    for (size_t i = 0; i < order.size(); ++i) {
        auto& extensions = ext[order[i]];
        const Pair& iv = cov[order[i]];
        const size_t left_lim = i == 0 ? 0 : cov[order[i - 1]].second;
        const size_t right_lim = i + 1 == order.size() ? n : cov[order[i + 1]].first;
        ns.clear(0);   // interval_nodes
        for (size_t j = iv.first; j < iv.second; ++j) ns.insert(0, path[j]);
        ns.clear(1);   // left_flank_positions (value: the position)
        size_t n_left = 0;
        for (size_t j = iv.first; j > left_lim; --j) {
            const uint32_t node = path[j - 1];
            if (ns.has(1, node) || ns.has(0, node)) break;
            ns.insert(1, node);
            ns.value[node] = (uint32_t)(j - 1);
            ++n_left;
        }
        Pair curr(iv.first - n_left, iv.second);
        for (size_t j = iv.second; j < right_lim; ++j) {
            const uint32_t node = path[j];
            if (ns.has(0, node)) break;
            if (ns.has(1, node) && ns.value[node] >= curr.first) {
                extensions.push_back(curr);
                curr.first = ns.value[node] + 1;
            }
            ++curr.second;
            ns.insert(0, node);
        }
        extensions.push_back(curr);
    }
    struct Dp { size_t gaps, bases, bp; };
    std::vector<std::vector<Dp>> dp(cov.size());
    for (size_t i = 0; i < order.size(); ++i) {
        const auto& extensions = ext[order[i]];
        const Pair& iv = cov[order[i]];
        auto& col = dp[order[i]];
        col.assign(extensions.size(), Dp{0, 0, (size_t)-1});
        if (i == 0) {
            for (size_t j = 0; j < col.size(); ++j) {
                col[j].gaps = (iv.first != 0 && extensions[j].first == 0) ? 1 : 0;
                col[j].bases = iv.first - extensions[j].first;
            }
            continue;
        }
        const Pair& piv = cov[order[i - 1]];
        const auto& pext = ext[order[i - 1]];
        const auto& pcol = dp[order[i - 1]];
        for (size_t j = 0; j < col.size(); ++j) {
            for (size_t k = 0; k < pcol.size(); ++k) {
                size_t gaps = pcol[k].gaps, bases = pcol[k].bases;
                if (piv.second != iv.first && pext[k].second >= extensions[j].first) {
                    gaps += 1;
                    bases += iv.first - piv.second;
                } else {
                    bases += pext[k].second - piv.second + iv.first - extensions[j].first;
                }
                if (gaps > col[j].gaps || (gaps == col[j].gaps && bases >= col[j].bases)) col[j] = Dp{gaps, bases, k};
            }
        }
    }
    size_t opt = (size_t)-1, opt_gaps = 0, opt_bases = 0;
    if (!order.empty()) {
        const auto& col = dp[order.back()];
        const Pair& iv = cov[order.back()];
        const auto& extensions = ext[order.back()];
        for (size_t j = 0; j < col.size(); ++j) {
            size_t gaps = col[j].gaps, bases = col[j].bases;
            if (iv.second != n && extensions[j].second == n) gaps += 1;
            bases += extensions[j].second - iv.second;
            if (gaps > opt_gaps || (gaps == opt_gaps && bases >= opt_bases)) { opt = j; opt_gaps = gaps; opt_bases = bases; }
        }
    }
    std::vector<Pair> best(cov.size());
    size_t row = opt;
    for (int64_t i = (int64_t)order.size() - 1; i >= 0; --i) {
        best[order[i]] = ext[order[i]][row];
        row = dp[order[i]][row].bp;
        if (i + 1 != (int64_t)order.size()) best[order[i]].second = std::min(best[order[i]].second, best[order[i + 1]].first);
    }
    return best;
}

// induced_cyclic_pairwise_alignment (alignment.cpp:569-846)
std::vector<Aln> induced_cyclic(const uint32_t* p1, uint64_t n1, const uint32_t* p2, uint64_t n2) {
    NodeSets& ns = tls_sets;
    std::vector<Aln> alns;
    cyclic_internal(p1, p2, Pair(0, 0), Pair(n1, n2), alns);
    std::vector<Pair> cov1, cov2;
    for (const auto& a : alns) {
        cov1.emplace_back(a.front().first, a.back().first + 1);
        cov2.emplace_back(a.front().second, a.back().second + 1);
    }
    {   // merge blocks adjacent on both paths unless a node would repeat (disjoint non-empty intervals: no ties in the sorts)
        std::vector<size_t> order1(cov1.size()), order2(cov2.size()), index2(cov2.size());
        for (size_t i = 0; i < order1.size(); ++i) order1[i] = order2[i] = i;
        std::sort(order1.begin(), order1.end(), [&](size_t i, size_t j) { return cov1[i] < cov1[j]; });
        std::sort(order2.begin(), order2.end(), [&](size_t i, size_t j) { return cov2[i] < cov2[j]; });
        for (size_t i = 0; i < order2.size(); ++i) index2[order2[i]] = i;
        std::vector<bool> keep(cov1.size(), true);
        size_t merge_run = 0;
        bool sets_empty = true;
        ns.clear(0);
        ns.clear(1);
        for (size_t i = 1; i < order1.size(); ++i) {
            bool did_merge = false;
            if (index2[order1[i]] == index2[order1[i - 1]] + 1) {
                const size_t head = order1[i - 1 - merge_run];
                if (sets_empty) {
                    for (size_t j = cov1[head].first; j < cov1[head].second; ++j) ns.insert(0, p1[j]);
                    for (size_t j = cov2[head].first; j < cov2[head].second; ++j) ns.insert(1, p2[j]);
                    sets_empty = false;
                }
                bool compatible = true;
                for (size_t j = cov1[head].second; j < cov1[order1[i]].second && compatible; ++j) compatible = ns.insert(0, p1[j]);
                for (size_t j = cov2[head].second; j < cov2[order1[i]].second && compatible; ++j) compatible = ns.insert(1, p2[j]);
                if (compatible) {
                    auto& aln = alns[head];
                    for (size_t j = cov1[head].second; j < cov1[order1[i]].first; ++j) aln.emplace_back(j, kGap);
                    for (size_t j = cov2[head].second; j < cov2[order1[i]].first; ++j) aln.emplace_back(kGap, j);
                    for (const auto& ap : alns[order1[i]]) aln.emplace_back(ap);
                    alns[order1[i]].clear();
                    keep[order1[i]] = false;
                    cov1[head].second = cov1[order1[i]].second;
                    cov2[head].second = cov2[order1[i]].second;
                    did_merge = true;
                }
            }
            if (did_merge) ++merge_run;
            else {
                // (the reference's sets can be non-empty here only after a refused merge: they were filled, so "empty" means cleared)
                ns.clear(0);
                ns.clear(1);
                sets_empty = true;
                merge_run = 0;
            }
        }
        size_t removed = 0;
        for (size_t i = 0; i < alns.size(); ++i) {
            if (!keep[i]) ++removed;
            else if (removed) { cov1[i - removed] = cov1[i]; cov2[i - removed] = cov2[i]; alns[i - removed] = std::move(alns[i]); }
        }
        cov1.resize(cov1.size() - removed);
        cov2.resize(cov2.size() - removed);
        alns.resize(alns.size() - removed);
    }
    const auto ext1 = noncyclic_extension(p1, n1, cov1), ext2 = noncyclic_extension(p2, n2, cov2);
    for (size_t i = 0; i < alns.size(); ++i) {
        auto& aln = alns[i];
        size_t added = 0;
        for (size_t j = ext1[i].first; j < cov1[i].first; ++j) { aln.emplace_back(j, kGap); ++added; }
        for (size_t j = ext2[i].first; j < cov2[i].first; ++j) { aln.emplace_back(kGap, j); ++added; }
        std::rotate(aln.rbegin(), aln.rbegin() + added, aln.rend());
        for (size_t j = cov1[i].second; j < ext1[i].second; ++j) aln.emplace_back(j, kGap);
        for (size_t j = cov2[i].second; j < ext2[i].second; ++j) aln.emplace_back(kGap, j);
    }
    // dangling insertions, split where a node would repeat.  The extended intervals begin at distinct positions (each at or behind the end of
    // the covered interval before it), so sorting by their starts has no ties.
    std::vector<size_t> order(alns.size());
    for (int side = 0; side < 2; ++side) {
        const auto& ext = side == 0 ? ext1 : ext2;
        const uint32_t* p = side == 0 ? p1 : p2;
        const uint64_t n = side == 0 ? n1 : n2;
        for (size_t i = 0; i < order.size(); ++i) order[i] = i;
        std::sort(order.begin(), order.end(), [&](size_t i, size_t j) { return ext[i].first < ext[j].first; });
        for (size_t i = 0; i <= order.size(); ++i) {
            const size_t l = i == 0 ? 0 : ext[order[i - 1]].second, r = i == order.size() ? n : ext[order[i]].first;
            if (l == r) continue;
            ns.clear(0);
            alns.emplace_back();
            for (size_t j = l; j < r; ++j) {
                if (ns.has(0, p[j])) { alns.emplace_back(); ns.clear(0); }
                alns.back().emplace_back(side == 0 ? Pair(j, kGap) : Pair(kGap, j));
                ns.insert(0, p[j]);
            }
        }
    }
    return alns;
}

void maf_row(std::string& out, const std::string& name, uint64_t start, uint64_t size, const Aln& block, bool first, const uint32_t* path,
             const uint8_t* label) {
    out += "s\t"; out += name; out += '\t'; out += std::to_string(start); out += '\t'; out += std::to_string(size); out += "\t+\t";
    static const char dec[] = {'A', 'C', 'G', 'T', 'N'};
    for (const auto& ap : block) {
        const uint64_t x = first ? ap.first : ap.second;
        if (x == kGap) { out += '-'; continue; }
        const uint8_t c = label[path[x]];
        out += c <= 4 ? dec[c] : (char)c;   // above 4: the raw byte (labels above 127 the reference would decode out of its table)
    }
    out += '\n';
}

// ---------------------------------------------- what the device passes over pairs of paths share -----------------------------------------
// One chunk of a batch, ready for a pass of induced_kernels.hip: the jobs (text_off / text_cap zero), the pair each job answers, and the device
// arrays the kernels read (the graph's paths and labels, the chunk's position tables)
struct InducedChunk {
    std::vector<ClInducedJob> jobs;
    std::vector<uint64_t> job_pair;
    const uint32_t* d_nodes;
    uint64_t n_steps;
    const uint8_t* d_label;
    const uint32_t* d_tables;
};

// A graph on the device for the passes over pairs of its paths: paths and labels, uploaded once and only when a pair needs them, and what is
// known about each path — node ids out of range (found on the host, once per path) and nodes met twice (found on the device with the tables)
struct InducedGraph {
    cl_context* ctx;
    const cl_base_graph* g;
    uint64_t n_steps;
    ScopedBuf<uint32_t> d_nodes;
    ScopedBuf<uint8_t> d_label;
    bool on_device = false;
    std::vector<int8_t> bad_ids;
    std::vector<uint8_t> repeated, host_checked;
    std::vector<uint64_t> seen;
    InducedGraph(cl_context* c, const cl_base_graph* graph)
        : ctx(c), g(graph), n_steps(graph->path_off[graph->n_paths]), bad_ids(graph->n_paths, -1), repeated(graph->n_paths, 0), host_checked(graph->n_paths, 0) {}
    bool ids_bad(uint64_t p) {
        if (bad_ids[p] < 0) {
            bad_ids[p] = 0;
            for (uint64_t i = g->path_off[p]; i < g->path_off[p + 1]; ++i) if (g->path_nodes[i] >= g->n_nodes) { bad_ids[p] = 1; break; }
            if (g->path_off[p + 1] - g->path_off[p] >= 0xFFFFFFFFull) bad_ids[p] = 1;   // positions are 32-bit words in the table
        }
        return bad_ids[p] == 1;
    }
    int upload() {
        if (on_device) return CL_OK;
        int rc;
        if ((rc = d_nodes.alloc(ctx, n_steps)) || (rc = d_label.alloc(ctx, g->n_nodes))) return rc;
        HIP_TRY(ctx, cl_copy_sync(ctx, d_nodes.p, g->path_nodes, n_steps * sizeof(uint32_t), hipMemcpyHostToDevice));
        HIP_TRY(ctx, cl_copy_sync(ctx, d_label.p, g->label, g->n_nodes, hipMemcpyHostToDevice));
        on_device = true;
        return CL_OK;
    }
    // the device's repeat check on the host, for a first path no chunk held
    void find_repeats(uint64_t p) {
        if (p >= g->n_paths || ids_bad(p) || repeated[p] || host_checked[p]) return;
        host_checked[p] = 1;
        if (seen.empty()) seen.assign(g->n_nodes, 0);   // seen[v]: 1 + the last path checked here that holds node v
        for (uint64_t i = g->path_off[p]; i < g->path_off[p + 1] && !repeated[p]; ++i) {
            repeated[p] = seen[g->path_nodes[i]] == p + 1;
            seen[g->path_nodes[i]] = p + 1;
        }
    }
    // what cl_induced_pairwise_cigar returns for (a, b), once the device has seen a's table: a path index out of range, then a path-1 node id out
    // of range or met twice, then a path-2 node id out of range
    int code(uint64_t a, uint64_t b) {
        if (a >= g->n_paths || b >= g->n_paths) return CL_ERR_INVALID_ARGUMENT;
        if (ids_bad(a) || repeated[a]) return CL_ERR_CYCLIC_GRAPH;
        return ids_bad(b) ? CL_ERR_INVALID_ARGUMENT : CL_OK;
    }
};

// Chunks of these pairs of a graph on the device: the pairs the host does not refuse, ordered by first path and cut into chunks, each chunk's
// position tables (scatter + check), then pass(chunk) for the entry point's own kernels and copies.  Afterwards dg.code() holds for every pair.
template <class Pass>
int induced_chunks(InducedGraph& dg, const uint64_t* pairs, uint64_t n_pairs, Pass&& pass) {
    cl_context* ctx = dg.ctx;
    const cl_base_graph* g = dg.g;
    std::vector<uint64_t> todo;   // pairs whose path 1 gets a position table, ordered by path 1
    for (uint64_t k = 0; k < n_pairs; ++k) {
        const uint64_t a = pairs[2 * k], b = pairs[2 * k + 1];
        if (a >= g->n_paths || b >= g->n_paths || dg.ids_bad(a)) continue;
        todo.push_back(k);
    }
    std::stable_sort(todo.begin(), todo.end(), [&](uint64_t x, uint64_t y) { return pairs[2 * x] < pairs[2 * y]; });
    int rc;
    if (!todo.empty() && (rc = dg.upload())) return rc;
    const uint64_t table_bytes = std::max<uint64_t>(g->n_nodes, 1) * sizeof(uint32_t);
    for (size_t c0 = 0; c0 < todo.size();) {
        // one chunk: up to kChunkPairs pairs whose first paths' tables fit in kChunkTableBytes (at least one first path)
        std::vector<uint64_t> firsts;
        size_t c1 = c0;
        while (c1 < todo.size() && c1 - c0 < kChunkPairs) {
            const uint64_t p = pairs[2 * todo[c1]];
            if (firsts.empty() || firsts.back() != p) {
                if (!firsts.empty() && (firsts.size() + 1) * table_bytes > kChunkTableBytes) break;
                firsts.push_back(p);
            }
            ++c1;
        }
        ScopedBuf<uint32_t> d_tables, d_rep;
        if ((rc = d_tables.alloc(ctx, firsts.size() * (table_bytes / sizeof(uint32_t))))) return rc;
        if ((rc = d_rep.alloc(ctx, firsts.size()))) return rc;
        HIP_TRY(ctx, hipMemsetAsync(d_rep.p, 0, firsts.size() * sizeof(uint32_t), ctx->stream));
        for (size_t f = 0; f < firsts.size(); ++f)
            HIP_TRY(ctx, cl_launch_induced_table(dg.d_nodes.p + g->path_off[firsts[f]], g->path_off[firsts[f] + 1] - g->path_off[firsts[f]],
                                                 d_tables.p + f * (table_bytes / sizeof(uint32_t)), g->n_nodes, d_rep.p + f, ctx->stream));
        InducedChunk chunk{{}, {}, dg.d_nodes.p, dg.n_steps, dg.d_label.p, d_tables.p};
        for (size_t t = c0, f = 0; t < c1; ++t) {
            const uint64_t k = todo[t], a = pairs[2 * k], b = pairs[2 * k + 1];
            while (firsts[f] != a) ++f;
            if (dg.ids_bad(b)) continue;   // decided on the host (after the device's repeat check)
            chunk.jobs.push_back(ClInducedJob{g->path_off[a], g->path_off[a + 1] - g->path_off[a], g->path_off[b], g->path_off[b + 1] - g->path_off[b],
                                              f * (table_bytes / sizeof(uint32_t)), 0, 0});
            chunk.job_pair.push_back(k);
        }
        if ((rc = pass(chunk))) return rc;
        std::vector<uint32_t> rep(firsts.size());
        HIP_TRY(ctx, cl_copy_sync(ctx, rep.data(), d_rep.p, rep.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
        for (size_t f = 0; f < firsts.size(); ++f) dg.repeated[firsts[f]] |= rep[f] != 0;
        c0 = c1;
    }
    return CL_OK;
}

// The frame of cl_induced_pairwise_cigars, _stats, _profiles and cl_induced_gap_events_batch: the graph on the device, chunks of the pairs with
// pass(chunk) for each, and at the end the code of the first failing pair (cl_induced_pairwise_cigar's order of checks).
template <class Pass>
int induced_batch(cl_context* ctx, const cl_base_graph* g, const uint64_t* pairs, uint64_t n_pairs, Pass&& pass) {
    InducedGraph dg(ctx, g);
    const int rc = induced_chunks(dg, pairs, n_pairs, pass);
    if (rc) return rc;
    for (uint64_t k = 0; k < n_pairs; ++k) {   // the first failing pair decides
        const int e = dg.code(pairs[2 * k], pairs[2 * k + 1]);
        if (e != CL_OK) {
            cl_set_error(ctx, "induced pairwise alignment of paths %llu and %llu (pair %llu): %s", (unsigned long long)pairs[2 * k],
                         (unsigned long long)pairs[2 * k + 1], (unsigned long long)k, e == CL_ERR_CYCLIC_GRAPH ? "the first path follows a cycle" : "invalid path");
            return e;
        }
    }
    return CL_OK;
}

}  // namespace

extern "C" {

int cl_induced_cyclic_maf(const cl_base_graph* g, uint64_t path1, uint64_t path2, const char* name1, const char* name2, char** text_out, uint64_t* len_out) {
    if (!g || !text_out || !name1 || !name2 || path1 >= g->n_paths || path2 >= g->n_paths) return CL_ERR_INVALID_ARGUMENT;
    *text_out = nullptr;
    const uint32_t* p1 = g->path_nodes + g->path_off[path1];
    const uint32_t* p2 = g->path_nodes + g->path_off[path2];
    const uint64_t n1 = g->path_off[path1 + 1] - g->path_off[path1], n2 = g->path_off[path2 + 1] - g->path_off[path2];
    for (uint64_t i = 0; i < n1; ++i) if (p1[i] >= g->n_nodes) return CL_ERR_INVALID_ARGUMENT;
    for (uint64_t i = 0; i < n2; ++i) if (p2[i] >= g->n_nodes) return CL_ERR_INVALID_ARGUMENT;
    std::string out;
    try {
        tls_sets.fit(g->n_nodes);
        const std::vector<Aln> blocks = induced_cyclic(p1, n1, p2, n2);
        const std::string s1 = name1, s2 = name2;
        out = "track name=" + s1 + "_vs_" + s2 + "_induced\n##maf version=1\n";
        for (const auto& block : blocks) {   // output_maf (alignment.cpp:848-904)
            uint64_t start1 = kGap, start2 = kGap, size1 = 0, size2 = 0;
            for (const auto& ap : block) {
                if (ap.first != kGap) { if (start1 == kGap) start1 = ap.first; ++size1; }
                if (ap.second != kGap) { if (start2 == kGap) start2 = ap.second; ++size2; }
            }
            out += "\na\n";
            maf_row(out, s1, start1 == kGap ? n1 : start1, size1, block, true, p1, g->label);
            maf_row(out, s2, start2 == kGap ? n2 : start2, size2, block, false, p2, g->label);
        }
    } catch (const std::bad_alloc&) {
        return CL_ERR_OUT_OF_MEMORY;
    }
    *text_out = c_string(out, len_out);
    return *text_out ? CL_OK : CL_ERR_OUT_OF_MEMORY;
}

int cl_induced_pairwise_cigars(cl_context* ctx, const cl_base_graph* g, const uint64_t* pairs, uint64_t n_pairs, char** text_out, uint64_t* offsets_out) {
    cl_bind_device(ctx);
    if (!ctx || !g || (n_pairs && !pairs) || !text_out || !offsets_out) return CL_ERR_INVALID_ARGUMENT;
    *text_out = nullptr;
    std::vector<std::string> texts(n_pairs);
    int rc = induced_batch(ctx, g, pairs, n_pairs, [&](InducedChunk& c) -> int {
        std::vector<ClInducedJob>& jobs = c.jobs;
        int rc;
        ScopedBuf<ClInducedJob> d_jobs;
        ScopedBuf<int64_t> d_len;
        std::vector<int64_t> len(jobs.size());
        if ((rc = d_jobs.upload(ctx, jobs)) || (rc = d_len.alloc(ctx, jobs.size()))) return rc;
        HIP_TRY(ctx, cl_launch_induced_runs(false, d_jobs.p, (uint32_t)jobs.size(), c.d_nodes, c.n_steps, c.d_label, g->n_nodes, c.d_tables, d_len.p, nullptr, ctx->stream));
        HIP_TRY(ctx, cl_copy_sync(ctx, len.data(), d_len.p, len.size() * sizeof(int64_t), hipMemcpyDeviceToHost));
        // write passes over groups of jobs whose text fits in kChunkTextBytes (at least one job)
        for (size_t w0 = 0; w0 < jobs.size();) {
            size_t w1 = w0;
            uint64_t bytes = 0;
            while (w1 < jobs.size() && (w1 == w0 || bytes + (uint64_t)len[w1] <= kChunkTextBytes)) {
                jobs[w1].text_off = bytes;
                jobs[w1].text_cap = (uint64_t)len[w1];
                bytes += (uint64_t)len[w1];
                ++w1;
            }
            ScopedBuf<char> d_text;
            std::vector<ClInducedJob> sub(jobs.begin() + w0, jobs.begin() + w1);
            std::vector<char> host(bytes);
            if ((rc = d_jobs.upload(ctx, sub)) || (rc = d_text.alloc(ctx, bytes))) return rc;
            HIP_TRY(ctx, cl_launch_induced_runs(true, d_jobs.p, (uint32_t)sub.size(), c.d_nodes, c.n_steps, c.d_label, g->n_nodes, c.d_tables, nullptr, d_text.p, ctx->stream));
            HIP_TRY(ctx, cl_copy_sync(ctx, host.data(), d_text.p, bytes, hipMemcpyDeviceToHost));
            for (size_t j = w0; j < w1; ++j) texts[c.job_pair[j]].assign(host.data() + jobs[j].text_off, (size_t)jobs[j].text_cap);
            w0 = w1;
        }
        return CL_OK;
    });
    if (rc) return rc;
    uint64_t total = 0;
    for (uint64_t k = 0; k < n_pairs; ++k) { offsets_out[k] = total; total += texts[k].size(); }
    offsets_out[n_pairs] = total;
    char* out = (char*)malloc(total + 1);
    if (!out) return CL_ERR_OUT_OF_MEMORY;
    for (uint64_t k = 0; k < n_pairs; ++k) memcpy(out + offsets_out[k], texts[k].data(), texts[k].size());
    out[total] = '\0';
    *text_out = out;
    return CL_OK;
}

int cl_induced_pairwise_stats(cl_context* ctx, const cl_base_graph* g, const uint64_t* pairs, uint64_t n_pairs, cl_pair_stats* out) {
    cl_bind_device(ctx);
    if (!ctx || !g || (n_pairs && (!pairs || !out))) return CL_ERR_INVALID_ARGUMENT;
    return induced_batch(ctx, g, pairs, n_pairs, [&](InducedChunk& c) -> int {
        int rc;
        ScopedBuf<ClInducedJob> d_jobs;
        ScopedBuf<cl_pair_stats> d_stats;
        std::vector<cl_pair_stats> stats(c.jobs.size());
        if ((rc = d_jobs.upload(ctx, c.jobs)) || (rc = d_stats.alloc(ctx, c.jobs.size()))) return rc;
        HIP_TRY(ctx, cl_launch_induced_stats(d_jobs.p, (uint32_t)c.jobs.size(), c.d_nodes, c.n_steps, c.d_label, g->n_nodes, c.d_tables, d_stats.p, ctx->stream));
        HIP_TRY(ctx, cl_copy_sync(ctx, stats.data(), d_stats.p, stats.size() * sizeof(cl_pair_stats), hipMemcpyDeviceToHost));
        for (size_t j = 0; j < stats.size(); ++j) out[c.job_pair[j]] = stats[j];
        return CL_OK;
    });
}

int cl_induced_pairwise_profiles(cl_context* ctx, const cl_base_graph* g, const uint64_t* pairs, uint64_t n_pairs, uint64_t window, cl_pair_window** out,
                                 uint64_t* offsets_out) {
    cl_bind_device(ctx);
    if (!ctx || !g || (n_pairs && !pairs) || !out || !offsets_out) return CL_ERR_INVALID_ARGUMENT;
    *out = nullptr;
    if (window == 0) { cl_set_error(ctx, "the window of a pairwise profile must be at least 1"); return CL_ERR_INVALID_ARGUMENT; }
    // a pair's windows follow from the length of its first path: the result's layout is known before the device runs
    auto n_windows = [&](uint64_t n1) { return std::max<uint64_t>(1, n1 / window + (n1 % window != 0)); };
    uint64_t total = 0;
    for (uint64_t k = 0; k < n_pairs; ++k) {
        offsets_out[k] = total;
        const uint64_t a = pairs[2 * k];
        if (a < g->n_paths && pairs[2 * k + 1] < g->n_paths) total += n_windows(g->path_off[a + 1] - g->path_off[a]);
    }
    offsets_out[n_pairs] = total;
    cl_pair_window* win = (cl_pair_window*)malloc(std::max<uint64_t>(total, 1) * sizeof(cl_pair_window));
    if (!win) return CL_ERR_OUT_OF_MEMORY;
    const uint64_t width = std::min<uint64_t>(window, 1ull << 40);   // (beyond any path: one window either way; the kernel computes in int64_t)
    std::vector<cl_pair_window> host;
    const int rc = induced_batch(ctx, g, pairs, n_pairs, [&](InducedChunk& c) -> int {
        std::vector<ClInducedJob>& jobs = c.jobs;
        int rc;
        // passes over groups of jobs whose windows fit in kChunkWindows (at least one job)
        for (size_t w0 = 0; w0 < jobs.size();) {
            size_t w1 = w0;
            uint64_t n = 0;
            while (w1 < jobs.size() && (w1 == w0 || n + n_windows(jobs[w1].n1) <= kChunkWindows)) {
                jobs[w1].text_off = n;
                jobs[w1].text_cap = n_windows(jobs[w1].n1);
                n += jobs[w1].text_cap;
                ++w1;
            }
            ScopedBuf<ClInducedJob> d_jobs;
            ScopedBuf<cl_pair_window> d_win;
            std::vector<ClInducedJob> sub(jobs.begin() + w0, jobs.begin() + w1);
            if (host.size() < n) host.resize(n);
            if ((rc = d_jobs.upload(ctx, sub)) || (rc = d_win.alloc(ctx, n))) return rc;
            HIP_TRY(ctx, hipMemsetAsync(d_win.p, 0, n * sizeof(cl_pair_window), ctx->stream));
            HIP_TRY(ctx, cl_launch_induced_profile(d_jobs.p, (uint32_t)sub.size(), c.d_nodes, c.n_steps, c.d_label, g->n_nodes, c.d_tables, width, d_win.p, ctx->stream));
            HIP_TRY(ctx, cl_copy_sync(ctx, host.data(), d_win.p, n * sizeof(cl_pair_window), hipMemcpyDeviceToHost));
            for (size_t j = w0; j < w1; ++j) memcpy(win + offsets_out[c.job_pair[j]], host.data() + jobs[j].text_off, jobs[j].text_cap * sizeof(cl_pair_window));
            w0 = w1;
        }
        return CL_OK;
    });
    if (rc) { free(win); return rc; }
    *out = win;
    return CL_OK;
}

int cl_induced_gap_events_batch(cl_context* ctx, const cl_base_graph* g, const uint64_t* pairs, uint64_t n_pairs, uint64_t min_len, cl_gap_event** out,
                                uint64_t* offsets_out) {
    cl_bind_device(ctx);
    if (!ctx || !g || (n_pairs && !pairs) || !out || !offsets_out) return CL_ERR_INVALID_ARGUMENT;
    *out = nullptr;
    if (min_len == 0) { cl_set_error(ctx, "the least length of a gap event must be at least 1"); return CL_ERR_INVALID_ARGUMENT; }
    std::vector<std::vector<cl_gap_event>> events(n_pairs);
    std::vector<cl_gap_event> host;
    int rc = induced_batch(ctx, g, pairs, n_pairs, [&](InducedChunk& c) -> int {
        std::vector<ClInducedJob>& jobs = c.jobs;
        int rc;
        ScopedBuf<ClInducedJob> d_jobs;
        ScopedBuf<int64_t> d_cnt;
        std::vector<int64_t> cnt(jobs.size());
        if ((rc = d_jobs.upload(ctx, jobs)) || (rc = d_cnt.alloc(ctx, jobs.size()))) return rc;
        HIP_TRY(ctx, cl_launch_induced_events(false, d_jobs.p, (uint32_t)jobs.size(), c.d_nodes, c.n_steps, c.d_label, g->n_nodes, c.d_tables, min_len, d_cnt.p, nullptr, ctx->stream));
        HIP_TRY(ctx, cl_copy_sync(ctx, cnt.data(), d_cnt.p, cnt.size() * sizeof(int64_t), hipMemcpyDeviceToHost));
        // write passes over groups of jobs whose events fit in kChunkEvents (at least one job)
        for (size_t w0 = 0; w0 < jobs.size();) {
            size_t w1 = w0;
            uint64_t n = 0;
            while (w1 < jobs.size() && (w1 == w0 || n + (uint64_t)cnt[w1] <= kChunkEvents)) {
                jobs[w1].text_off = n;
                jobs[w1].text_cap = (uint64_t)cnt[w1];
                n += (uint64_t)cnt[w1];
                ++w1;
            }
            if (n) {
                ScopedBuf<cl_gap_event> d_ev;
                std::vector<ClInducedJob> sub(jobs.begin() + w0, jobs.begin() + w1);
                if (host.size() < n) host.resize(n);
                if ((rc = d_jobs.upload(ctx, sub)) || (rc = d_ev.alloc(ctx, n))) return rc;
                HIP_TRY(ctx, cl_launch_induced_events(true, d_jobs.p, (uint32_t)sub.size(), c.d_nodes, c.n_steps, c.d_label, g->n_nodes, c.d_tables, min_len, nullptr, d_ev.p, ctx->stream));
                HIP_TRY(ctx, cl_copy_sync(ctx, host.data(), d_ev.p, n * sizeof(cl_gap_event), hipMemcpyDeviceToHost));
                for (size_t j = w0; j < w1; ++j) events[c.job_pair[j]].assign(host.begin() + jobs[j].text_off, host.begin() + jobs[j].text_off + jobs[j].text_cap);
            }
            w0 = w1;
        }
        return CL_OK;
    });
    if (rc) return rc;
    uint64_t total = 0;
    for (uint64_t k = 0; k < n_pairs; ++k) { offsets_out[k] = total; total += events[k].size(); }
    offsets_out[n_pairs] = total;
    cl_gap_event* ev = (cl_gap_event*)malloc(std::max<uint64_t>(total, 1) * sizeof(cl_gap_event));
    if (!ev) return CL_ERR_OUT_OF_MEMORY;
    for (uint64_t k = 0; k < n_pairs; ++k) if (!events[k].empty()) memcpy(ev + offsets_out[k], events[k].data(), events[k].size() * sizeof(cl_gap_event));
    *out = ev;
    return CL_OK;
}

int cl_induced_pairwise_agreements(cl_context* ctx, const cl_base_graph* a, const cl_base_graph* b, const uint64_t* quads, uint64_t n, cl_pair_agreement* out) {
    cl_bind_device(ctx);
    if (!ctx || !a || !b || (n && (!quads || !out))) return CL_ERR_INVALID_ARGUMENT;
    InducedGraph da(ctx, a), db(ctx, b);
    auto len = [](const cl_base_graph* g, uint64_t p) { return g->path_off[p + 1] - g->path_off[p]; };
    // what needs no device: a path index out of range in either graph, lengths that differ, a path 1 whose indices do not fit a partner word.  Such
    // a quad is left out of both passes; its code is decided at the end, behind what the device finds (a first, then b, then the lengths)
    auto host_refuses = [&](const uint64_t* q) {
        if (q[0] >= a->n_paths || q[1] >= a->n_paths || q[2] >= b->n_paths || q[3] >= b->n_paths) return true;
        return len(a, q[0]) != len(b, q[2]) || len(a, q[1]) != len(b, q[3]) || len(a, q[0]) >= 0x7FFFFFFFull;
    };
    std::vector<cl_pair_agreement> host;
    for (uint64_t g0 = 0; g0 < n;) {
        // one group: quads in order whose partner slices fit in kChunkPartnerBytes (at least one quad); slot = the quad's place in the group
        std::vector<uint64_t> pairs_a, pairs_b, slice, quad_of;
        uint64_t words = 0, g1 = g0;
        for (; g1 < n; ++g1) {
            const uint64_t* q = quads + 4 * g1;
            if (host_refuses(q)) continue;
            const uint64_t n2 = len(a, q[1]);
            if (!quad_of.empty() && (words + n2) * sizeof(uint32_t) > kChunkPartnerBytes) break;
            pairs_a.insert(pairs_a.end(), {q[0], q[1]});
            pairs_b.insert(pairs_b.end(), {q[2], q[3]});
            slice.push_back(words);
            quad_of.push_back(g1);
            words += n2;
        }
        const uint64_t slots = quad_of.size();
        if (slots) {
            int rc;
            ScopedBuf<uint32_t> d_partner;
            ScopedBuf<uint64_t> d_counts;
            ScopedBuf<cl_pair_agreement> d_out;
            if ((rc = d_partner.alloc(ctx, words)) || (rc = d_counts.alloc(ctx, 2 * slots)) || (rc = d_out.alloc(ctx, slots))) return rc;
            HIP_TRY(ctx, hipMemsetAsync(d_partner.p, 0xFF, std::max<uint64_t>(words, 1) * sizeof(uint32_t), ctx->stream));
            HIP_TRY(ctx, hipMemsetAsync(d_counts.p, 0, 2 * slots * sizeof(uint64_t), ctx->stream));
            HIP_TRY(ctx, hipMemsetAsync(d_out.p, 0, slots * sizeof(cl_pair_agreement), ctx->stream));
            // both passes find a pair's slice and slot through job_pair: a and b order and chunk the pairs each in their own way
            auto place = [&](InducedChunk& c) {
                for (size_t j = 0; j < c.jobs.size(); ++j) { c.jobs[j].text_off = slice[c.job_pair[j]]; c.jobs[j].text_cap = c.job_pair[j]; }
            };
            rc = induced_chunks(da, pairs_a.data(), slots, [&](InducedChunk& c) -> int {
                int rc;
                ScopedBuf<ClInducedJob> d_jobs;
                place(c);
                if ((rc = d_jobs.upload(ctx, c.jobs))) return rc;
                HIP_TRY(ctx, cl_launch_induced_partner(d_jobs.p, (uint32_t)c.jobs.size(), c.d_nodes, c.n_steps, c.d_label, a->n_nodes, c.d_tables, d_partner.p, d_counts.p, ctx->stream));
                return CL_OK;
            });
            if (rc) return rc;
            rc = induced_chunks(db, pairs_b.data(), slots, [&](InducedChunk& c) -> int {
                int rc;
                ScopedBuf<ClInducedJob> d_jobs;
                place(c);
                if ((rc = d_jobs.upload(ctx, c.jobs))) return rc;
                HIP_TRY(ctx, cl_launch_induced_agreement(d_jobs.p, (uint32_t)c.jobs.size(), c.d_nodes, c.n_steps, c.d_label, b->n_nodes, c.d_tables, d_partner.p, d_counts.p, d_out.p,
                                                         ctx->stream));
                return CL_OK;
            });
            if (rc) return rc;
            host.resize(slots);
            HIP_TRY(ctx, cl_copy_sync(ctx, host.data(), d_out.p, slots * sizeof(cl_pair_agreement), hipMemcpyDeviceToHost));
            for (uint64_t j = 0; j < slots; ++j) out[quad_of[j]] = host[j];
        }
        g0 = g1;
    }
    for (uint64_t k = 0; k < n; ++k) {   // the first failing quad decides: a's code, then b's, then the lengths
        const uint64_t* q = quads + 4 * k;
        if (host_refuses(q)) { da.find_repeats(q[0]); db.find_repeats(q[2]); }   // (no pass saw this quad)
        int e = da.code(q[0], q[1]);
        if (e == CL_OK) e = db.code(q[2], q[3]);
        if (e == CL_OK && host_refuses(q)) e = CL_ERR_INVALID_ARGUMENT;
        if (e != CL_OK) {
            cl_set_error(ctx, "agreement of paths %llu and %llu with paths %llu and %llu (quad %llu): %s", (unsigned long long)q[0], (unsigned long long)q[1],
                         (unsigned long long)q[2], (unsigned long long)q[3], (unsigned long long)k,
                         e == CL_ERR_CYCLIC_GRAPH ? "the first path follows a cycle" : "invalid path, or the two graphs' paths differ in length");
            return e;
        }
    }
    return CL_OK;
}

}  // extern "C"
