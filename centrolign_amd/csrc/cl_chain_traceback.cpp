// cl_chain_traceback.cpp — after the device has produced every DP value (chain_dp.hpp: ChainTrace): the optimum (anchorer.hpp:2483-2499), and for each pair on the
// chain the predecessor the reference would have recorded.  The DP VALUE is a maximum and is order-free, the
// BACKPOINTER is whatever the reference's search trees return among equal maxima: first candidate query in its
// loop order whose value reaches the maximum (strict '>' in MatchBank::update_dp, match_bank.hpp:177), and inside
// that query the tree's traversal rule — first unit met by range_max; inside a cross tree the larger outer index
// (values there are (score, index) pairs, orthogonal_max_search_tree.hpp:76); inside a gap-free subtree the
// earliest inserted (strict '>' in MaxSearchTree::update, max_search_tree.hpp:318-358).  replay_units evaluates that
// rule directly on the sorted keys; it only runs when a maximum is attained more than once.
// The candidate values and gap scores are the reference's arithmetic in its operation order: built with -ffp-contract=off.
#include <cmath>
#include <cstdio>
#include <numeric>

#include "chain_dp.hpp"

namespace clchain {

namespace {
std::chrono::steady_clock::time_point tnow() { return std::chrono::steady_clock::now(); }
void tadd(double& acc_ms, std::chrono::steady_clock::time_point t0) { acc_ms += std::chrono::duration<double, std::milli>(tnow() - t0).count(); }

// members -> (offset, slot) order + the implicit heap layout
void finish_tree(const ChainProblem& P, GapFreeTree* tree, bool by_slot) {
    {
        std::vector<uint32_t> idx(tree->mem.size());
        std::iota(idx.begin(), idx.end(), 0u);
        const auto& m0 = tree->mem;
        sort_by_key_then_slot(idx, P.M, [&](uint32_t i) { return (int64_t)m0[i].off; }, [&](uint32_t i) { return m0[i].slot; }, by_slot);
        std::vector<GapFreeTree::Member> sorted(idx.size());
        for (size_t i = 0; i < idx.size(); ++i) sorted[i] = m0[idx[i]];
        tree->mem.swap(sorted);
    }
    tree->heap = heap_of_rank(tree->mem.size());
    tree->rank_of_heap.resize(tree->mem.size());
    for (size_t r = 0; r < tree->mem.size(); ++r) tree->rank_of_heap[tree->heap[r]] = (uint32_t)r;
    tree->built = true;
}
}  // namespace

// what the traceback's tie resolution needs of every combination — its records in (shift, slot) order with the implicit-heap layout of the
// reference's outer tree — depends on the records alone, not on the DP: built on the pool's threads while the device runs the DP (at the
// root of a ten-sequence tree the traceback spent 70 of its 166 ms building them on first use)
void ChainTrace::start_prebuild(ChainProblem& P) {
    if (P.sparse && P.K == 1 && P.M >= (1u << 16)) {
        // the gap-free DP's trees — one per chain of graph 2, holding every record filed under it, keyed (offset, slot) — depend on the records alone as well: a tie on a
        // tree of 1.25 M members cost the traceback 19 ms on first use (a leaf merge of 10 x 1 Mbp); built here beside the device's DP
        std::vector<uint32_t> p2s;
        for (const Combo& c : P.combos) if (std::find(p2s.begin(), p2s.end(), c.p2) == p2s.end()) p2s.push_back(c.p2);
        for (uint32_t p2 : p2s) sparse_trees[((uint64_t)p2 << 32) | 0u];   // (the map is complete before the thread starts: no insertion races with the traceback)
        ortho_prebuild = std::thread([&, p2s] {
            cl_parallel_for(p2s.size(), [&](uint64_t b, uint64_t e) {
                for (uint64_t i = b; i < e; ++i) {
                    GapFreeTree* tree = &sparse_trees.find(((uint64_t)p2s[i] << 32) | 0u)->second;
                    for (Combo& oc : P.combos)
                        if (oc.p2 == p2s[i])
                            for (uint32_t r = 0; r < oc.rec_s.size(); ++r) tree->mem.push_back(GapFreeTree::Member{oc.off[r], P.by_s[oc.rec_s[r]], r});
                    finish_tree(P, tree, false);
                }
            }, 1);
        });
    }
    if (!P.sparse && P.K == 1 && P.M >= (1u << 16))
        ortho_prebuild = std::thread([&] {
            cl_parallel_for(P.combos.size(), [&](uint64_t b, uint64_t e) {
                for (uint64_t ci = b; ci < e; ++ci) {
                    Combo& c = P.combos[ci];
                    Combo::SubRecs& sr = c.per_sub[0];
                    sr.recs.resize(c.rec_s.size());
                    std::iota(sr.recs.begin(), sr.recs.end(), 0u);
                    sr.ortho_order = sr.recs;
                    sort_by_key_then_slot(sr.ortho_order, P.M, [&](uint32_t r) { return (int64_t)c.sigma[r]; }, [&](uint32_t r) { return P.by_s[c.rec_s[r]]; });
                    sr.ortho_heap = heap_of_rank(sr.ortho_order.size());
                    sr.ortho_rank_of_heap.resize(sr.ortho_order.size());
                    for (size_t r = 0; r < sr.ortho_order.size(); ++r) sr.ortho_rank_of_heap[sr.ortho_heap[r]] = (uint32_t)r;
                    c.split_built = true;
                }
            }, 1);
        });
}

// (a small DP builds its value index on the host)
int ChainTrace::prepare_index(const ChainProblem& P, ChainDev& dev) {
    vkeys.assign(P.combos.size(), std::vector<std::vector<int>>(7));
    vrecs.assign(P.combos.size(), std::vector<std::vector<uint32_t>>(7));
    vbuilt.assign(P.combos.size(), std::vector<char>(7, 0));
    if (dev.d_pack.p) return CL_OK;
    int rc = CL_OK;
    hipError_t he = hipSuccess;
    uint32_t nmax = 0;
    for (const Combo& c : P.combos) nmax = std::max<uint32_t>(nmax, (uint32_t)c.rec_s.size());
    CL_CHAIN_TRY(dev.k_in.alloc(P.ctx, nmax)); CL_CHAIN_TRY(dev.k_out.alloc(P.ctx, nmax)); CL_CHAIN_TRY(dev.i_in.alloc(P.ctx, nmax)); CL_CHAIN_TRY(dev.i_out.alloc(P.ctx, nmax));
    he = cl_chain_sort_values(nullptr, nmax, dev.k_in.p, dev.i_in.p, dev.k_out.p, dev.i_out.p, nullptr, &vtemp_bytes, P.ctx->stream);
    if (he == hipSuccess) { rc = dev.vtemp.alloc(P.ctx, vtemp_bytes); if (rc) he = hipErrorOutOfMemory; }
    if (he != hipSuccess) { cl_set_error(P.ctx, "value index failed: %s", hipGetErrorString(he)); return CL_ERR_HIP; }
    return CL_OK;
}

bool ChainTrace::value_index(const ChainProblem& P, ChainDev& dev, size_t ci, int kind) {
    if (vbuilt[ci][kind]) return true;
    const auto t = std::chrono::steady_clock::now();
    const uint32_t n = (uint32_t)P.combos[ci].rec_s.size();
    if (dev.d_pack.p) {
        // a small DP: the stored values came back with the DP values; the same order as the device's stable radix sort
        const float* val = reinterpret_cast<const float*>(dev.pack_host.data() + ((char*)dev.cd[ci].d_val.p - dev.d_pack.p - dev.pack_dp_off)) + (size_t)kind * n;
        vrecs[ci][kind].resize(n);
        vkeys[ci][kind].resize(n);
        value_index_host(val, n, vkeys[ci][kind].data(), vrecs[ci][kind].data());
        index_ms += ms_since(t);
        vbuilt[ci][kind] = 1;
        return true;
    }
    hipError_t e = cl_chain_sort_values(dev.cd[ci].d_val.p + (size_t)kind * n, n, dev.k_in.p, dev.i_in.p, dev.k_out.p, dev.i_out.p, dev.vtemp.p, &vtemp_bytes, P.ctx->stream);
    vkeys[ci][kind].resize(n);
    vrecs[ci][kind].resize(n);
    if (e == hipSuccess && n) e = hipMemcpyAsync(vkeys[ci][kind].data(), dev.k_out.p, n * 4, hipMemcpyDeviceToHost, P.ctx->stream);
    if (e == hipSuccess && n) e = hipMemcpyAsync(vrecs[ci][kind].data(), dev.i_out.p, n * 4, hipMemcpyDeviceToHost, P.ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(P.ctx->stream);
    index_ms += ms_since(t);
    if (e != hipSuccess) { cl_set_error(P.ctx, "value index failed: %s", hipGetErrorString(e)); return false; }
    vbuilt[ci][kind] = 1;
    return true;
}

// records of one instance inside a combination (the reference's trees belong to ONE chaining call)
Combo::SubRecs& ChainTrace::sub_recs(const ChainProblem& P, Combo& c, uint32_t k) {
    if (!c.split_built) {
        const auto t0 = tnow();
        if (P.K == 1) {
            auto& recs = c.per_sub[0].recs;
            recs.resize(c.rec_s.size());
            std::iota(recs.begin(), recs.end(), 0u);
        } else {
            std::vector<Combo::SubRecs*> of_sub(P.K, nullptr);
            for (uint32_t r = 0; r < c.rec_s.size(); ++r) {
                const uint32_t sub = P.pairs[P.by_s[c.rec_s[r]]].sub;
                if (!of_sub[sub]) of_sub[sub] = &c.per_sub[sub];   // unordered_map: references stay valid across insertions
                of_sub[sub]->recs.push_back(r);
            }
        }
        c.split_built = true;
        tadd(t_split, t0);
    }
    return c.per_sub[k];
}

// an instance's records of one combination in (shift, slot) order with the implicit-heap layout of the reference's outer tree
void ChainTrace::ortho_of(const ChainProblem& P, Combo::SubRecs& sr, const Combo& c) {
    if (!sr.ortho_order.empty()) return;
    const auto t0 = tnow();
    sr.ortho_order = sr.recs;
    sort_by_key_then_slot(sr.ortho_order, P.M, [&](uint32_t r) { return (int64_t)c.sigma[r]; }, [&](uint32_t r) { return P.by_s[c.rec_s[r]]; });
    sr.ortho_heap = heap_of_rank(sr.ortho_order.size());
    sr.ortho_rank_of_heap.resize(sr.ortho_order.size());
    for (size_t r = 0; r < sr.ortho_order.size(); ++r) sr.ortho_rank_of_heap[sr.ortho_heap[r]] = (uint32_t)r;
    tadd(t_ortho, t0);
}

// ---- optimum and traceback (anchorer.hpp:2483-2531) of one instance ---------------------------------------------------
int ChainTrace::trace_instance(ChainProblem& P, const ChainPath& path, ChainDev& dev, uint32_t k, ChainSubResult& res) {
    const SubCtx& sk = P.sc[k];
    if (sk.pair_hi == sk.pair_lo) return CL_OK;
    float opt = CL_CHAIN_NEG;
    uint32_t best_slot = kNone;
    for (uint32_t slot = sk.pair_lo; slot < sk.pair_hi; ++slot) {
        float v = dev.dp_sorted[P.s_of_slot[slot]];
        const float f = P.final_term[slot];
        if (f == CL_CHAIN_NEG) v = f;
        else v += f;
        if (v > opt && v > sk.min_score) { opt = v; best_slot = slot; }
    }
    std::vector<uint32_t> chain_slots;
    std::vector<std::pair<uint32_t, uint32_t>> edges;   // (scratch of the steps below)
    std::vector<uint32_t> cand;
    uint64_t n_ties = 0;
    uint32_t here = best_slot;
    const uint32_t C1 = (uint32_t)sk.x[0]->chain_size(), C2 = (uint32_t)sk.x[1]->chain_size();
    while (here != kNone) {
        ++n_steps;
        chain_slots.push_back(here);
        const uint32_t s = P.s_of_slot[here];
        const float dpv = dev.dp_sorted[s], w = P.weight[s];
        if (!(dpv > P.init_w[s])) break;  // no candidate was strictly greater than the chain that starts here: chain start
        const Pair& p = P.pairs[here];
        // the reference's candidate order: forward edges by the topological position of their source node, then chain1;
        // chain2 ascending; gap-free tree, then trees 0..5 (anchorer.hpp:2352-2413)
        edges.clear();                                      // (position of from-node, p1)
        for (uint32_t p1 = 0; p1 < C1; ++p1) {
            const uint32_t pr = sk.x[0]->predecessor_index(p.b1, p1);
            if (pr == kNone) continue;
            const uint64_t from = sk.x[0]->node_at(p1, pr);
            if (sk.has_start[p.b1] && sk.after_end[from]) edges.emplace_back(sk.pos1[from], p1);
        }
        std::sort(edges.begin(), edges.end());
        const int* arow = nullptr;
        if (path.lazy_acc && !(arow = dev.acc_row(P, s))) { return CL_ERR_HIP; }
        int win_combo = -1, win_kind = -1;
        for (size_t e = 0; e < edges.size() && win_combo < 0; ++e)
            for (uint32_t p2 = 0; p2 < C2 && win_combo < 0; ++p2) {
                const uint32_t ci = P.combo_of[(size_t)P.tag_of(k, 0, edges[e].second) * P.n_tag[1] + P.tag_of(k, 1, p2)];
                if (ci == kNone) continue;  // empty trees
                const int* a = path.lazy_acc ? arow + (size_t)ci * 7 : &dev.acc[ci][(size_t)s * 7];
                uint32_t c_qt, c_qoff;
                int32_t c_q;
                P.query_at(ci, s, c_qt, c_qoff, c_q);
                for (int kind = 0; kind < (P.sparse ? 1 : 7); ++kind) {
                    if (a[kind] == enc(CL_CHAIN_NEG)) continue;
                    const float stored = dec(a[kind]);
                    float cand;
                    if (kind == 0) cand = stored + w;
                    else {
                        const int pw = kind - 1;
                        const double pen = (pw % 2 == 1) ? P.local_scale * (P.cp->gap_open[pw / 2] + P.cp->gap_extend[pw / 2] * (double)c_q)
                                                         : P.local_scale * (P.cp->gap_open[pw / 2] - P.cp->gap_extend[pw / 2] * (double)c_q);
                        cand = (float)((double)(stored + w) - pen);
                    }
                    if (cand == dpv) { win_combo = (int)ci; win_kind = kind; break; }
                }
            }
        if (win_combo < 0) { cl_set_error(P.ctx, "traceback: no candidate reproduces dp of pair %u", here); return CL_ERR_HIP; }
        Combo& c = P.combos[win_combo];
        uint32_t wq_t, wq_off;
        int32_t wq;
        P.query_at((size_t)win_combo, s, wq_t, wq_off, wq);
        // every predecessor whose stored value equals the query's maximum and which lies in the query's range
        cand.clear();
        {
            const auto t0 = tnow();
            const int target = path.lazy_acc ? arow[(size_t)win_combo * 7 + win_kind] : dev.acc[win_combo][(size_t)s * 7 + win_kind];
            if (!value_index(P, dev, (size_t)win_combo, win_kind)) { return CL_ERR_HIP; }
            const auto& keys = vkeys[win_combo][win_kind];
            const auto& recs = vrecs[win_combo][win_kind];
            const uint32_t qt = wq_t, qoff = wq_off;
            const int32_t qq = wq;
            for (size_t i = std::lower_bound(keys.begin(), keys.end(), target) - keys.begin(); i < keys.size() && keys[i] == target; ++i) {
                ++n_scanned;
                const uint32_t r = recs[i];
                if (c.rec_s[r] >= s) continue;
                const int32_t sg = c.sigma[r];
                const bool kind_ok = win_kind == 0 ? sg == qq : ((win_kind - 1) % 2 == 1 ? sg < qq : sg > qq);
                if (kind_ok && c.ins_t[r] <= qt && c.off[r] < qoff) cand.push_back(r);
            }
            tadd(t_cand, t0);
        }
        const uint32_t count = (uint32_t)cand.size();
        if (count == 0) { cl_set_error(P.ctx, "traceback: query of pair %u has no predecessor at its maximum", here); return CL_ERR_HIP; }
        uint32_t win_rec;
        if (count == 1) {
            win_rec = cand[0];
        } else {
            ++n_ties;
            auto slot_of_rec = [&](uint32_t r) { return P.by_s[c.rec_s[r]]; };
            if (win_kind == 0) {
                // gap-free tree of this diagonal: records with the same shift, keyed (offset, match id);
                // inside an off-path subtree the earliest inserted wins, insertion order = (position of e1, slot)
                // members of the tree, as (offset, slot, record-or-none): affine mode -> the records of this combination with
                // the query's shift; sparse mode -> every pair whose e2 is filed under chain2, whatever its chain1
                // (search_trees[i][j] is built from search_tree_data[j] for every i, anchorer.hpp:1581-1592)
                GapFreeTree* tree;
                if (!P.sparse) {
                    Combo::SubRecs& sr = sub_recs(P, c, k);
                    tree = &sr.diag_tree[wq];
                    if (!tree->built) {   // the records of this shift are one run of the (shift, slot) order
                        const auto t0 = tnow();
                        ortho_of(P, sr, c);
                        const int32_t qq = wq;
                        auto it = std::partition_point(sr.ortho_order.begin(), sr.ortho_order.end(), [&](uint32_t r) { return c.sigma[r] < qq; });
                        for (; it != sr.ortho_order.end() && c.sigma[*it] == qq; ++it) tree->mem.push_back(GapFreeTree::Member{c.off[*it], slot_of_rec(*it), *it});
                        tadd(t_diag, t0);
                    }
                } else {
                    tree = &sparse_trees[((uint64_t)c.p2 << 32) | k];
                    if (!tree->built)
                        for (Combo& oc : P.combos)
                            if (oc.p2 == c.p2)
                                for (uint32_t r : sub_recs(P, oc, k).recs) tree->mem.push_back(GapFreeTree::Member{oc.off[r], P.by_s[oc.rec_s[r]], r});
                }
                if (!tree->built) {
                    const auto t0 = tnow();
                    finish_tree(P, tree, !P.sparse);   // (affine: the members are a run of the (shift, slot) order, i.e. in slot order already)
                    tadd(t_gapfree, t0);
                }
                const auto& mem = tree->mem;
                const size_t n = mem.size();
                const auto& h = tree->heap;
                const auto& rank_of_heap = tree->rank_of_heap;
                const size_t rhi = std::partition_point(mem.begin(), mem.end(), [&](const GapFreeTree::Member& m) { return m.off < wq_off; }) - mem.begin();
                std::vector<std::pair<size_t, uint32_t>> ch;  // (heap node, record)
                for (uint32_t r : cand) {
                    const GapFreeTree::Member key{c.off[r], slot_of_rec(r), r};
                    const size_t rk = std::lower_bound(mem.begin(), mem.end(), key, [](const GapFreeTree::Member& a, const GapFreeTree::Member& b) { return a.off != b.off ? a.off < b.off : a.slot < b.slot; }) - mem.begin();
                    ch.emplace_back(h[rk], r);
                }
                auto earlier = [&](uint32_t a, uint32_t b) {
                    const uint32_t pa = sk.pos1[P.pairs[slot_of_rec(a)].e1], pb = sk.pos1[P.pairs[slot_of_rec(b)].e1];
                    return pa != pb ? pa < pb : slot_of_rec(a) < slot_of_rec(b);
                };
                win_rec = kNone;
                replay_units(n, rank_of_heap, 0, rhi,
                             [&](size_t x) { for (auto& e : ch) if (e.first == x) { win_rec = e.second; return true; } return false; },
                             [&](size_t x) {
                                 for (auto& e : ch) if (in_subtree(e.first, x) && (win_rec == kNone || earlier(e.second, win_rec))) win_rec = e.second;
                                 return win_rec != kNone;
                             });
            } else {
                // orthogonal tree of this combination: all its records keyed ((shift, match id), offset); inside a
                // cross tree the values are (score, outer index) pairs, so the larger outer heap index wins
                Combo::SubRecs& sr = sub_recs(P, c, k);
                auto key_less = [&](uint32_t a, uint32_t b) { return c.sigma[a] != c.sigma[b] ? c.sigma[a] < c.sigma[b] : slot_of_rec(a) < slot_of_rec(b); };
                ortho_of(P, sr, c);
                const size_t n = sr.ortho_order.size();
                const int32_t qq = wq;
                const bool odd = (win_kind - 1) % 2 == 1;
                // rank interval of the key1 range: shift < query (odd trees) or shift > query (even trees)
                size_t lo = 0, hi = n;
                auto first_ge = [&](int64_t v) {
                    return (size_t)(std::partition_point(sr.ortho_order.begin(), sr.ortho_order.end(), [&](uint32_t r) { return (int64_t)c.sigma[r] < v; }) - sr.ortho_order.begin());
                };
                if (odd) hi = first_ge(qq);
                else lo = first_ge((int64_t)qq + 1);
                std::vector<std::pair<size_t, uint32_t>> ch;
                for (uint32_t r : cand) {
                    const size_t rk = std::lower_bound(sr.ortho_order.begin(), sr.ortho_order.end(), r, key_less) - sr.ortho_order.begin();
                    ch.emplace_back(sr.ortho_heap[rk], r);
                }
                win_rec = kNone;
                size_t win_heap = 0;
                replay_units(n, sr.ortho_rank_of_heap, lo, hi,
                             [&](size_t x) { for (auto& e : ch) if (e.first == x) { win_rec = e.second; return true; } return false; },
                             [&](size_t x) {
                                 for (auto& e : ch) if (in_subtree(e.first, x) && (win_rec == kNone || e.first > win_heap)) { win_rec = e.second; win_heap = e.first; }
                                 return win_rec != kNone;
                             });
            }
            if (win_rec == kNone) { cl_set_error(P.ctx, "traceback: tie resolution failed for pair %u", here); return CL_ERR_HIP; }
        }
        here = P.by_s[c.rec_s[win_rec]];
        if (chain_slots.size() > P.M) { cl_set_error(P.ctx, "traceback loop"); return CL_ERR_HIP; }
    }
    std::reverse(chain_slots.begin(), chain_slots.end());
    res.n_ties = n_ties;
    const size_t na = chain_slots.size();
    res.chain.resize(3 * na);
    for (size_t i = 0; i < na; ++i) {
        const Pair& p = P.pairs[chain_slots[i]];
        res.chain[3 * i] = p.set;
        res.chain[3 * i + 1] = p.i1;
        res.chain[3 * i + 2] = p.i2;
    }
    if (!P.sparse) {   // gap annotation (anchorer.hpp:2443-2468)
        res.gap.assign(na + 1, 0);
        res.gap_score.assign(na + 1, 0.0);
        for (size_t i = 1; i < na; ++i) {
            const Pair& a = P.pairs[chain_slots[i - 1]];
            const Pair& b = P.pairs[chain_slots[i]];
            const int32_t g = P.measure_gap(sk, a.e1, a.e2, b.b1, b.b2);
            res.gap[i] = g;
            res.gap_score[i] = P.score_gap(g);
        }
        if (P.subs[k].anchored && na) {
            const Pair& f = P.pairs[chain_slots.front()];
            const Pair& l = P.pairs[chain_slots.back()];
            res.gap[0] = P.gap_from_sources(k, f.b1, f.b2);
            res.gap_score[0] = P.score_gap((int32_t)res.gap[0]);
            res.gap[na] = P.gap_to_sinks(k, l.e1, l.e2);
            res.gap_score[na] = P.score_gap((int32_t)res.gap[na]);
        }
    }
    return CL_OK;
}

int ChainTrace::run(ChainProblem& P, const ChainPath& path, ChainDev& dev, std::vector<ChainSubResult>& results, std::vector<float>* dp_out) {
    const auto T1 = std::chrono::steady_clock::now();
    if (const int rc = prepare_index(P, dev)) return rc;
    P.tm.index_ms += ms_since(T1);
    const auto T2 = std::chrono::steady_clock::now();
    for (uint32_t k = 0; k < P.K; ++k)
        if (const int rc = trace_instance(P, path, dev, k, results[k])) return rc;
    P.tm.index_ms += index_ms;
    P.tm.traceback_ms += ms_since(T2) - index_ms;
    if (P.timing) fprintf(stderr, "[chain_dp_batch]   traceback: %llu steps, %llu equal-valued records scanned; split %.1f ortho %.1f by-shift %.1f gap-free trees %.1f candidates (incl. value index) %.1f ms\n",
                        (unsigned long long)n_steps, (unsigned long long)n_scanned, t_split, t_ortho, t_diag, t_gapfree, t_cand);
    P.lap("traceback");
    if (dp_out) {
        dp_out->resize(P.M);
        for (uint32_t slot = 0; slot < P.M; ++slot) (*dp_out)[slot] = dev.dp_sorted[P.s_of_slot[slot]];
    }
    return CL_OK;
}

}  // namespace clchain
