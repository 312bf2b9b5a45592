// cl_chain_prep.cpp — the host-only phases of the chaining DP (chain_dp.hpp: ChainProblem), none of which makes a HIP call; O(M) or O(M log M):
//   * the coordinate system: PathMerge tables (path_merge.hpp:96-277), post-switch distances
//     (post_switch_distances.hpp:44-81), source/query shifts and offsets per (chain1, chain2) (anchorer.hpp:1875-1904),
//     forward-edge existence (forward_edges.hpp:40-53 with the masks of anchorer.hpp:1752-1810), anchor weights
//     (score_function.hpp:51-75);
//   * ordering the match pairs by the topological position of their first graph-1 node, so that every possible
//     predecessor of a pair comes before it.
// The weights and gap scores are the reference's float / double arithmetic in its operation order: this file is built with -ffp-contract=off.
#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstdlib>

#include "chain_dp.hpp"

namespace clchain {

// match pairs in MatchBank iteration order (match_bank.hpp:252-268), instance by instance: slot = position in that order
int ChainProblem::collect_pairs() {
    for (size_t k = 0; k < K; ++k) {
        const ChainSub& sb = subs[k];
        const SetView ms(sb);
        sc[k].pair_lo = (uint32_t)pairs.size();
        if (sb.num_match_sets > sb.ms->n_sets) { cl_set_error(ctx, "num_match_sets exceeds the number of sets"); return CL_ERR_INVALID_ARGUMENT; }
        {   // the sets are the caller's: a walk is a non-empty run of node ids of its graph (anything else would index the tables below out of range)
            std::atomic<uint64_t> bad_set{UINT64_MAX};
            cl_parallel_for(sb.num_match_sets, [&](uint64_t sb0, uint64_t se0) {
                for (uint64_t s = sb0; s < se0; ++s)
                    for (int side = 0; side < 2; ++side) {
                        const uint64_t n_nodes = sb.g[side]->n_nodes;
                        for (uint64_t j = 0; j < ms.n_walks(side, s); ++j) {
                            const uint64_t w = ms.walk(side, s, j);
                            if (ms.wo[side][w + 1] <= ms.wo[side][w] || ms.front(side, w) >= n_nodes || ms.back(side, w) >= n_nodes) { bad_set = s; return; }
                        }
                    }
            }, 4096);
            if (bad_set.load() != UINT64_MAX) {
                const uint64_t s = bad_set.load();
                cl_set_error(ctx, "match set %llu (of %llu) holds an empty walk or a node id outside its graph (%llu and %llu nodes; the set has %llu x %llu walks of length %llu)",
                             (unsigned long long)s, (unsigned long long)sb.num_match_sets, (unsigned long long)sb.g[0]->n_nodes, (unsigned long long)sb.g[1]->n_nodes,
                             (unsigned long long)ms.n_walks(0, s), (unsigned long long)ms.n_walks(1, s), (unsigned long long)(ms.n_walks(0, s) ? ms.length(s) : 0));
                return CL_ERR_INVALID_ARGUMENT;
            }
        }
        if (!sb.masked && sb.num_match_sets >= 4096) {
            // (the usual case, no mask: every set's pairs have their place by a prefix sum over n1 * n2, the sets are filled in side by side)
            const uint64_t ns = sb.num_match_sets;
            std::vector<uint64_t> at(ns + 1, 0);
            bool too_many = false;
            for (uint64_t s = 0; s < ns; ++s) {
                const uint64_t n1 = ms.n_walks(0, s), n2 = ms.n_walks(1, s);
                too_many |= n1 >= 65535 || n2 >= 65535;
                at[s + 1] = at[s] + n1 * n2;
            }
            if (too_many) { cl_set_error(ctx, "a match set has too many walks"); return CL_ERR_INVALID_ARGUMENT; }
            const uint64_t base = pairs.size();
            if (base + at[ns] >= (1ull << 31)) { cl_set_error(ctx, "too many match pairs"); return CL_ERR_INVALID_ARGUMENT; }
            pairs.resize(base + at[ns]);
            cl_parallel_for(ns, [&](uint64_t sb0, uint64_t se0) {
                for (uint64_t s = sb0; s < se0; ++s) {
                    const uint64_t n1 = ms.n_walks(0, s), n2 = ms.n_walks(1, s);
                    Pair* out = pairs.data() + base + at[s];
                    for (uint64_t j = 0; j < n1; ++j) {
                        const uint64_t w1 = ms.walk(0, s, j);
                        const uint32_t b1 = ms.front(0, w1), e1 = ms.back(0, w1);
                        for (uint64_t q = 0; q < n2; ++q) {
                            const uint64_t w2 = ms.walk(1, s, q);
                            *out++ = Pair{(uint32_t)k, (uint32_t)s, (uint32_t)j, (uint32_t)q, b1, e1, ms.front(1, w2), ms.back(1, w2)};
                        }
                    }
                }
            }, 2048);
        } else
        for (uint64_t s = 0; s < sb.num_match_sets; ++s) {
            const uint64_t n1 = ms.n_walks(0, s), n2 = ms.n_walks(1, s);
            if (n1 >= 65535 || n2 >= 65535) { cl_set_error(ctx, "match set %llu has too many walks", (unsigned long long)s); return CL_ERR_INVALID_ARGUMENT; }
            const uint64_t ms_set = sb.order ? sb.order[s] : s;
            for (uint64_t j = 0; j < n1; ++j) {
                const uint64_t w1 = ms.walk(0, s, j);
                const uint32_t b1 = ms.front(0, w1), e1 = ms.back(0, w1);
                if (sb.masked) sc[k].walk_marks.emplace_back(b1, e1);   // the forward-edge masks see every walk, masked or not
                for (uint64_t q = 0; q < n2; ++q) {
                    if (sb.masked && (sb.swap_sides ? sb.masked(ms_set, (uint32_t)q, (uint32_t)j) : sb.masked(ms_set, (uint32_t)j, (uint32_t)q))) continue;
                    const uint64_t w2 = ms.walk(1, s, q);
                    pairs.push_back(Pair{(uint32_t)k, (uint32_t)s, (uint32_t)j, (uint32_t)q, b1, e1, ms.front(1, w2), ms.back(1, w2)});
                }
            }
        }
        if (pairs.size() >= (1ull << 31)) { cl_set_error(ctx, "too many match pairs"); return CL_ERR_INVALID_ARGUMENT; }
        sc[k].pair_hi = (uint32_t)pairs.size();
        if (sc[k].pair_hi > sc[k].pair_lo) { span_a += sb.g[0]->n_nodes + 2; span_b += sb.g[1]->n_nodes + 2; }
    }
    M = pairs.size();
    tm.n_pairs = M;
    if (M == 0) return CL_OK;
    if (span_a >= 0xFFFFFFFFull || span_b >= 0xFFFFFFFFull) { cl_set_error(ctx, "batch too large for 32-bit path coordinates"); return CL_ERR_INVALID_ARGUMENT; }
    return CL_OK;
}

// per-instance coordinate systems; chain tags -> dense combination table
int ChainProblem::build_tables() {
    {
        uint64_t run_a = 0, run_b = span_b;
        for (size_t k = 0; k < K; ++k) {
            SubCtx& c = sc[k];
            if (c.pair_hi == c.pair_lo) continue;
            const ChainSub& sb = subs[k];
            for (int side = 0; side < 2; ++side) {
                if (sb.x[side] && sb.sw[side]) { c.x[side] = sb.x[side]; c.sw[side] = sb.sw[side]; }
                else {
                    if (!(sb.chain_merge ? c.own_x[side].build_chain_merge(*sb.g[side], sb.tableau) : c.own_x[side].build(*sb.g[side], sb.tableau))) { cl_set_error(ctx, "graph is not acyclic"); return CL_ERR_CYCLIC_GRAPH; }
                    c.own_sw[side].build(*sb.g[side], c.own_x[side]);
                    c.x[side] = &c.own_x[side];
                    c.sw[side] = &c.own_sw[side];
                }
                for (uint32_t p = 0; p < c.x[side]->chain_size(); ++p)
                    n_tag[side] = std::max(n_tag[side], (sb.tag[side].empty() ? p : sb.tag[side][p]) + 1);
            }
            run_b -= sb.g[1]->n_nodes + 2;
            c.off_a = (uint32_t)run_a;
            c.off_b = (uint32_t)run_b;
            run_a += sb.g[0]->n_nodes + 2;
            const cl_base_graph& g1 = *sb.g[0];
            const GraphOrder* go = sb.order1;
            if (!go) { c.own_order.build(g1); go = &c.own_order; }
            c.pos1 = go->pos.data();
            c.depth1 = go->depth.data();
            c.has_start.assign(g1.n_nodes, 0);
            c.after_end.assign(g1.n_nodes, 0);
            for (uint32_t s = c.pair_lo; s < c.pair_hi; ++s) { c.has_start[pairs[s].b1] = 1; c.after_end[pairs[s].e1] = 1; }
            for (const auto& m : c.walk_marks) { c.has_start[m.first] = 1; c.after_end[m.second] = 1; }
            // nodes that follow the end of some match (anchorer.hpp:1776-1797)
            std::vector<uint32_t> st;
            for (uint64_t v = 0; v < g1.n_nodes; ++v)
                if (c.after_end[v]) {
                    st.push_back((uint32_t)v);
                    while (!st.empty()) {
                        const uint32_t h = st.back();
                        st.pop_back();
                        for (uint64_t e = g1.next_off[h]; e < g1.next_off[h + 1]; ++e)
                            if (!c.after_end[g1.next_idx[e]]) { c.after_end[g1.next_idx[e]] = 1; st.push_back(g1.next_idx[e]); }
                    }
                }
        }
    }
    return CL_OK;
}

// processing order: by the depth of the pair's first graph-1 node, stable in slot order
void ChainProblem::sort_by_depth() {
    by_s.resize(M);
    {   // counting sort on the depth (stable)
        std::vector<uint32_t> key(M);
        uint32_t max_depth = 0;
        for (uint32_t slot = 0; slot < M; ++slot) { key[slot] = sc[pairs[slot].sub].depth1[pairs[slot].b1]; max_depth = std::max(max_depth, key[slot]); }
        std::vector<uint32_t> start((size_t)max_depth + 2, 0);
        for (uint32_t slot = 0; slot < M; ++slot) ++start[key[slot] + 1];
        for (size_t d = 0; d <= max_depth; ++d) start[d + 1] += start[d];
        for (uint32_t slot = 0; slot < M; ++slot) by_s[start[key[slot]]++] = slot;
    }
    s_of_slot.resize(M);
    for (uint32_t s = 0; s < M; ++s) s_of_slot[by_s[s]] = s;
}

void ChainProblem::weights() {
    weight.resize(M);
    {   // the weight depends on the match set only
        std::vector<std::vector<float>> set_weight(K);
        for (size_t k = 0; k < K; ++k) {
            if (sc[k].pair_hi == sc[k].pair_lo) continue;
            const SetView ms(subs[k]);
            set_weight[k].resize(subs[k].num_match_sets);
            cl_parallel_for(subs[k].num_match_sets, [&](uint64_t b, uint64_t e) {
                for (uint64_t st = b; st < e; ++st)
                    if (ms.n_walks(0, st)) set_weight[k][st] = (float)ms.weight(*cp, st);
            }, 4096);
        }
        cl_parallel_for(M, [&](uint64_t b, uint64_t e) {
            for (uint64_t s = b; s < e; ++s) { const Pair& p = pairs[by_s[s]]; weight[s] = set_weight[p.sub][p.set]; }
        });
    }
}

// Anchored chains (global anchoring, anchorer.hpp:1069-1076; fill-in, :683-693): a chain's first anchor pays the lead
// indel from the sources (affine, :2026-2039) or must be reachable from them (sparse, :1562-1582); its last anchor pays
// the final indel to the sinks (:2426-2438 / :1724-1741).
float ChainProblem::score_gap(int32_t gap) const {   // anchorer.hpp:1929-1944
    float score = CL_CHAIN_NEG;
    if (gap == 0) score = 0.0f;
    else if (gap != INT32_MAX)
        for (int pw = 0; pw < 3; ++pw) score = std::max<float>(score, (float)(-local_scale * (cp->gap_open[pw] + cp->gap_extend[pw] * std::abs(gap))));
    return score;
}
int32_t ChainProblem::measure_gap(const SubCtx& c, uint32_t a1, uint32_t a2, uint32_t c1, uint32_t c2) const {   // anchorer.hpp:1906-1927
    int32_t gap = INT32_MAX;
    if ((a1 == c1 || c.x[0]->reachable(a1, c1)) && (a2 == c2 || c.x[1]->reachable(a2, c2)))
        c.x[0]->for_each_chain_on(a1, [&](uint32_t p1) {
            c.x[1]->for_each_chain_on(a2, [&](uint32_t p2) {
                const uint32_t src = c.x[0]->index_on(a1, p1) - c.x[1]->index_on(a2, p2);
                const uint32_t qry = c.x[0]->predecessor_index(c1, p1) - c.x[1]->predecessor_index(c2, p2) + c.sw[0]->distance(c1, p1) - c.sw[1]->distance(c2, p2);
                const int32_t here_gap = (int32_t)(src - qry);
                if (std::abs(here_gap) < std::abs(gap)) gap = here_gap;
            });
        });
    return gap;
}
// the reference compares |gap| against the SIGNED running value (anchorer.hpp:1954, 1971, 1991)
int32_t ChainProblem::gap_from_sources(uint32_t k, uint32_t c1, uint32_t c2) const {
    int32_t best = INT32_MAX;
    for (uint32_t a : subs[k].src[0]) for (uint32_t b : subs[k].src[1]) { const int32_t h = measure_gap(sc[k], a, b, c1, c2); if (std::abs(h) < best) best = h; }
    return best;
}
int32_t ChainProblem::gap_to_sinks(uint32_t k, uint32_t a1, uint32_t a2) const {
    int32_t best = INT32_MAX;
    for (uint32_t c : subs[k].snk[0]) for (uint32_t d : subs[k].snk[1]) { const int32_t h = measure_gap(sc[k], a1, a2, c, d); if (std::abs(h) < best) best = h; }
    return best;
}

void ChainProblem::anchoring_terms() {
    init_w = weight;
    final_term.assign(M, 0.0f);
    cl_parallel_for(M, [&](uint64_t s_begin, uint64_t s_end) {
    for (uint32_t s = (uint32_t)s_begin; s < s_end; ++s) {
        const uint32_t slot = by_s[s];
        const Pair& p = pairs[slot];
        const ChainSub& sb = subs[p.sub];
        if (!sb.anchored) continue;
        const SubCtx& c = sc[p.sub];
        if (!sparse) {
            const float lead = score_gap(gap_from_sources(p.sub, p.b1, p.b2));
            init_w[s] = lead == CL_CHAIN_NEG ? CL_CHAIN_NEG : weight[s] + lead;
            final_term[slot] = score_gap(gap_to_sinks(p.sub, p.e1, p.e2));
        } else {
            bool f1 = false, f2 = false, t = false;
            for (uint32_t a : sb.src[0]) if (a == p.b1 || c.x[0]->reachable(a, p.b1)) { f1 = true; break; }
            for (uint32_t b : sb.src[1]) if (b == p.b2 || c.x[1]->reachable(b, p.b2)) { f2 = true; break; }
            if (!f1 || !f2) init_w[s] = CL_CHAIN_NEG;
            for (uint32_t a : sb.snk[0]) {
                for (uint32_t b : sb.snk[1])
                    if ((a == p.e1 || c.x[0]->reachable(p.e1, a)) && (b == p.e2 || c.x[1]->reachable(p.e2, b))) { t = true; break; }
                if (t) break;
            }
            final_term[slot] = t ? 0.0f : CL_CHAIN_NEG;
        }
    }
    });
    if (!sparse)   // the score of aligning nothing: one indel from the sources to the sinks (anchorer.hpp:2419-2424)
        for (size_t k = 0; k < K; ++k) {
            if (!subs[k].anchored || sc[k].pair_hi == sc[k].pair_lo) continue;
            int32_t best = INT32_MAX;
            for (uint32_t c : subs[k].snk[0]) for (uint32_t d : subs[k].snk[1]) for (uint32_t a : subs[k].src[0]) for (uint32_t b : subs[k].src[1]) {
                const int32_t h = measure_gap(sc[k], a, b, c, d);
                if (std::abs(h) < best) best = h;
            }
            sc[k].min_score = score_gap(best);
        }
}

// (chain1, chain2) combinations that hold at least one pair; the most populated one goes first (it is the one the
// intra kernel keeps in registers)
void ChainProblem::records() {
    combo_of.assign((size_t)n_tag[0] * n_tag[1], kNone);
    rec_off.assign(M + 1, 0);
    {
        // records per pair: one per (chain through e1, chain through e2); sparse_chain_dp files a match under the first chain
        // of each end only (anchorer.hpp:1621-1630).  Counted and filled in parallel over the pairs, numbered serially: a
        // combination's id is its order of first appearance, a record's position the number of earlier records of its combination
        cl_parallel_for(M, [&](uint64_t s_begin, uint64_t s_end) {
            for (uint64_t s = s_begin; s < s_end; ++s) {
                if (sparse) { rec_off[s + 1] = 1; continue; }
                const Pair& p = pairs[by_s[s]];
                const SubCtx& c = sc[p.sub];
                uint32_t k1 = 0, k2 = 0;
                c.x[0]->for_each_chain_on(p.e1, [&](uint32_t) { ++k1; });
                c.x[1]->for_each_chain_on(p.e2, [&](uint32_t) { ++k2; });
                rec_off[s + 1] = k1 * k2;
            }
        });
        for (uint64_t s = 0; s < M; ++s) rec_off[s + 1] += rec_off[s];
        const uint64_t R = rec_off[M];
        ClRawVec<uint32_t> r_tag(R), r_ins(R), r_off(R);
        ClRawVec<int32_t> r_sig(R);
        cl_parallel_for(M, [&](uint64_t s_begin, uint64_t s_end) {
            for (uint64_t s = s_begin; s < s_end; ++s) {
                const Pair& p = pairs[by_s[s]];
                const SubCtx& c = sc[p.sub];
                uint64_t r = rec_off[s];
                bool first1 = true;
                c.x[0]->for_each_chain_on(p.e1, [&](uint32_t p1) {
                    const bool take1 = !sparse || first1;
                    first1 = false;
                    if (!take1) return;
                    bool first2 = true;
                    c.x[1]->for_each_chain_on(p.e2, [&](uint32_t p2) {
                        const bool take2 = !sparse || first2;
                        first2 = false;
                        if (!take2) return;
                        const uint32_t i1 = c.x[0]->index_on(p.e1, p1), i2 = c.x[1]->index_on(p.e2, p2);
                        r_tag[r] = tag_of(p.sub, 0, p1) * n_tag[1] + tag_of(p.sub, 1, p2);
                        r_ins[r] = i1 + c.off_a;
                        r_off[r] = i2 + c.off_b;
                        r_sig[r] = sparse ? 0 : (int32_t)(i1 - i2);
                        ++r;
                    });
                });
            }
        });
        rec_combo.resize(R);
        rec_pos.resize(R);
        std::vector<uint32_t> combo_size;
        const size_t n_tags = combo_of.size();
        if (R >= sw.par_records_min && R > 0 && n_tags <= 4096) {
            par_numbering = true;
            // the same numbering in parallel: chunks of records count their tags, a combination's id is the order of first appearance of
            // its tag (smallest first record), a record's position the records of its combination in earlier chunks plus those before
            // it in its own
            const uint64_t n_chunks = std::min<uint64_t>(64, (R + (1u << 18) - 1) >> 18), chunk = (R + n_chunks - 1) / n_chunks;
            std::vector<std::vector<uint32_t>> hist(n_chunks, std::vector<uint32_t>(n_tags, 0));
            std::vector<std::vector<uint64_t>> first(n_chunks, std::vector<uint64_t>(n_tags, UINT64_MAX));
            cl_parallel_for(n_chunks, [&](uint64_t cb, uint64_t ce) {
                for (uint64_t c = cb; c < ce; ++c)
                    for (uint64_t r = c * chunk; r < std::min<uint64_t>(R, (c + 1) * chunk); ++r) {
                        const uint32_t t = r_tag[r];
                        if (hist[c][t]++ == 0) first[c][t] = r;
                    }
            }, 1);
            std::vector<std::pair<uint64_t, uint32_t>> order;   // (first record, tag)
            for (uint32_t t = 0; t < n_tags; ++t) {
                uint64_t f = UINT64_MAX;
                for (uint64_t c = 0; c < n_chunks; ++c) f = std::min(f, first[c][t]);
                if (f != UINT64_MAX) order.emplace_back(f, t);
            }
            std::sort(order.begin(), order.end());
            for (const auto& o : order) {
                combo_of[o.second] = (uint32_t)combos.size();
                combos.emplace_back();
                combos.back().p1 = o.second / n_tag[1];
                combos.back().p2 = o.second % n_tag[1];
                combo_size.push_back(0);
            }
            std::vector<std::vector<uint32_t>> base(n_chunks, std::vector<uint32_t>(n_tags, 0));
            for (uint32_t t = 0; t < n_tags; ++t) {
                uint32_t run = 0;
                for (uint64_t c = 0; c < n_chunks; ++c) { base[c][t] = run; run += hist[c][t]; }
                if (combo_of[t] != kNone) combo_size[combo_of[t]] = run;
            }
            cl_parallel_for(n_chunks, [&](uint64_t cb, uint64_t ce) {
                for (uint64_t c = cb; c < ce; ++c) {
                    std::vector<uint32_t>& next = base[c];
                    for (uint64_t r = c * chunk; r < std::min<uint64_t>(R, (c + 1) * chunk); ++r) {
                        rec_combo[r] = combo_of[r_tag[r]];
                        rec_pos[r] = next[r_tag[r]]++;
                    }
                }
            }, 1);
        } else
        for (uint64_t r = 0; r < R; ++r) {
            uint32_t& ci = combo_of[r_tag[r]];
            if (ci == kNone) {
                ci = (uint32_t)combos.size();
                combos.emplace_back();
                combos.back().p1 = r_tag[r] / n_tag[1];
                combos.back().p2 = r_tag[r] % n_tag[1];
                combo_size.push_back(0);
            }
            rec_combo[r] = ci;
            rec_pos[r] = combo_size[ci]++;
        }
        for (size_t ci = 0; ci < combos.size(); ++ci) {
            combos[ci].rec_s.resize(combo_size[ci]);
            combos[ci].ins_t.resize(combo_size[ci]);
            combos[ci].off.resize(combo_size[ci]);
            combos[ci].sigma.resize(combo_size[ci]);
        }
        cl_parallel_for(M, [&](uint64_t s_begin, uint64_t s_end) {
            for (uint64_t s = s_begin; s < s_end; ++s)
                for (uint64_t r = rec_off[s]; r < rec_off[s + 1]; ++r) {
                    Combo& cb = combos[rec_combo[r]];
                    const uint32_t at = rec_pos[r];
                    cb.rec_s[at] = (uint32_t)s;
                    cb.ins_t[at] = r_ins[r];
                    cb.off[at] = r_off[r];
                    cb.sigma[at] = r_sig[r];
                }
        });
    }
    if (combos.size() > 1) {
        size_t big = 0;
        for (size_t c = 1; c < combos.size(); ++c)
            if (combos[c].rec_s.size() > combos[big].rec_s.size()) big = c;
        if (big != 0) {
            std::swap(combos[0], combos[big]);
            for (auto& rc : rec_combo) rc = rc == 0 ? (uint32_t)big : rc == big ? 0u : rc;
            for (auto& v : combo_of) v = v == 0 ? (uint32_t)big : v == big ? 0u : v;
        }
    }
}

void ChainProblem::count_work() {
    if (timing) {
        size_t total = 0, largest = 0;
        for (const Combo& c : combos) { total += c.rec_s.size(); largest = std::max(largest, c.rec_s.size()); }
        fprintf(stderr, "[chain_dp_batch]   %zu pairs, %zu combinations, %zu records (largest combination %zu)\n", (size_t)M, combos.size(), total, largest);
    }
    tm.n_combos = (uint32_t)combos.size();
    for (const Combo& c : combos) tm.pair_evals += 0.5 * (double)c.rec_s.size() * (double)M;
}

void ChainProblem::queries() {
    n_blocks = (uint32_t)((M + kChainBlock - 1) / kChainBlock);
    // The queries are dense — one per pair and combination — but they factor: the insertion bound depends on (pair, chain of graph 1) only, the offset
    // bound on (pair, chain of graph 2), and the shift is a difference of one term of each (all modulo 2^32, as the reference's size_t arithmetic
    // truncated).  A single-instance DP of some size keeps the factors on the host (n_tag[0] + n_tag[1] arrays instead of 3 x combinations: 0.5 GB
    // instead of 9.4 GB at 25 + 25 paths and 1.25 M pairs) and lets the device multiply them out (chain_expand_queries_kernel); the traceback
    // multiplies out the handful it looks at.  CL_CHAIN_DENSE_QUERIES=1: the dense tables of rounds 1-3 (A/B).
    factored = K == 1 && !sw.dense_queries && (uint64_t)combos.size() * M > 100000;
    if (factored) {
        fa_qt.resize((size_t)n_tag[0] * M);
        fb_qoff.resize((size_t)n_tag[1] * M);
        if (!sparse) { fa_d.resize((size_t)n_tag[0] * M); fb_d.resize((size_t)n_tag[1] * M); }
        cl_parallel_for(M, [&](uint64_t s_begin, uint64_t s_end) {
            for (uint32_t s = (uint32_t)s_begin; s < s_end; ++s) {
                const Pair& p = pairs[by_s[s]];
                const SubCtx& c = sc[p.sub];
                const bool start = c.has_start[p.b1];
                for (uint32_t p1 = 0; p1 < c.x[0]->chain_size(); ++p1) {
                    const uint32_t pr = start ? c.x[0]->predecessor_index(p.b1, p1) : kNone;
                    // a forward edge exists only from a node that follows some match end (forward_edges.hpp:40-53)
                    const bool ok = pr != kNone && c.after_end[c.x[0]->node_at(p1, pr)];
                    const size_t at = (size_t)tag_of(p.sub, 0, p1) * M + s;
                    fa_qt[at] = ok ? pr + c.off_a : kNone;
                    if (!sparse) fa_d[at] = ok ? pr + c.sw[0]->distance(p.b1, p1) : 0u;
                }
                for (uint32_t p2 = 0; p2 < c.x[1]->chain_size(); ++p2) {
                    const uint32_t pr2 = c.x[1]->predecessor_index(p.b2, p2);
                    const size_t at = (size_t)tag_of(p.sub, 1, p2) * M + s;
                    fb_qoff[at] = pr2 + 1u + c.off_b;
                    if (!sparse) fb_d[at] = pr2 + c.sw[1]->distance(p.b2, p2);
                }
            }
        });
    } else {
    dense_qt.resize(combos.size() * (size_t)M);
    dense_qoff.resize(combos.size() * (size_t)M);
    dense_q.resize(combos.size() * (size_t)M);
    for (size_t ci = 0; ci < combos.size(); ++ci) { combos[ci].qt = dense_qt.data() + ci * (size_t)M; combos[ci].qoff = dense_qoff.data() + ci * (size_t)M; combos[ci].q = dense_q.data() + ci * (size_t)M; }
    cl_parallel_for(combos.size() * (size_t)M, [&](uint64_t b, uint64_t e) {   // 15 MB per combination at 1.25 M pairs, 25 combinations at the root
        std::fill(dense_qt.data() + b, dense_qt.data() + e, kNone);
        std::memset(dense_qoff.data() + b, 0, (e - b) * sizeof(uint32_t));
        std::memset(dense_q.data() + b, 0, (e - b) * sizeof(int32_t));
    }, 1u << 18);
    cl_parallel_for(M, [&](uint64_t s_begin, uint64_t s_end) {
    for (uint32_t s = (uint32_t)s_begin; s < s_end; ++s) {
        const Pair& p = pairs[by_s[s]];
        const SubCtx& c = sc[p.sub];
        if (!c.has_start[p.b1]) continue;
        for (uint32_t p1 = 0; p1 < c.x[0]->chain_size(); ++p1) {
            const uint32_t pr = c.x[0]->predecessor_index(p.b1, p1);
            // a forward edge exists only from a node that follows some match end (forward_edges.hpp:40-53)
            if (pr == kNone || !c.after_end[c.x[0]->node_at(p1, pr)]) continue;
            for (uint32_t p2 = 0; p2 < c.x[1]->chain_size(); ++p2) {
                const uint32_t ci = combo_of[(size_t)tag_of(p.sub, 0, p1) * n_tag[1] + tag_of(p.sub, 1, p2)];
                if (ci == kNone) continue;
                Combo& cb = combos[ci];
                cb.qt[s] = pr + c.off_a;
                cb.qoff[s] = c.x[1]->predecessor_index(p.b2, p2) + 1u + c.off_b;
                cb.q[s] = sparse ? 0 : (int32_t)(pr - c.x[1]->predecessor_index(p.b2, p2) + c.sw[0]->distance(p.b1, p1) - c.sw[1]->distance(p.b2, p2));
            }
        }
    }
    });
    }
    for (Combo& c : combos) {
        c.prefix.assign(n_blocks + 1, 0);
        size_t r = 0;
        for (uint32_t b = 0; b <= n_blocks; ++b) {
            const uint64_t first = (uint64_t)b * kChainBlock;
            while (r < c.rec_s.size() && c.rec_s[r] < first) ++r;
            c.prefix[b] = (uint32_t)r;
        }
    }
}

void ChainProblem::query_at(size_t ci, uint32_t s, uint32_t& qt, uint32_t& qoff, int32_t& q) const {
    const Combo& c = combos[ci];
    if (!factored) { qt = c.qt[s]; qoff = c.qoff[s]; q = c.q[s]; return; }
    qt = fa_qt[(size_t)c.p1 * M + s];
    if (qt == kNone) { qoff = 0; q = 0; return; }
    qoff = fb_qoff[(size_t)c.p2 * M + s];
    q = sparse ? 0 : (int32_t)(fa_d[(size_t)c.p1 * M + s] - fb_d[(size_t)c.p2 * M + s]);
}

}  // namespace clchain
