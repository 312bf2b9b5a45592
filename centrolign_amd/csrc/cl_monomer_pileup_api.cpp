// cl_monomer_pileup_api.cpp — monomer pileups, consensus and template refinement (the reference has none): the definition on the
// host (cl_monomer_pileup_host), the host half of the device path (cl_monomer_pileup_compute over monomer_pileup_kernels.hip), the consensus
// vote, the refinement loop over both, the seeds and the two text writers.  Integers throughout.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "cl_internal.hpp"

namespace {

constexpr uint64_t kMaxTemplate = 1024, kMaxTemplateBases = 8192;
constexpr uint32_t kMaxRounds = 64, kMaxShare = 1000;

int seq_code(char c) {   // 4: other
    switch (c) {
    case 'A': case 'a': return 0;
    case 'C': case 'c': return 1;
    case 'G': case 'g': return 2;
    case 'T': case 't': return 3;
    default: return 4;
    }
}

struct Plan {
    std::vector<uint8_t> codes;
    std::vector<uint32_t> tmpl_off;
    std::vector<ClPileupBlock> blocks;   // the used blocks, ordered by forward template (stable)
    std::vector<uint32_t> block_m;       // their forward templates
};

int alloc_pileup(const uint64_t* tmpl_len, uint64_t M, cl_monomer_pileup* out) {
    cl_monomer_pileup p;
    memset(&p, 0, sizeof(p));
    p.n_templates = M;
    p.col_off = (uint64_t*)calloc(M + 1, sizeof(uint64_t));
    if (p.col_off) for (uint64_t m = 0; m < M; ++m) p.col_off[m + 1] = p.col_off[m] + tmpl_len[m];
    const uint64_t total = p.col_off ? p.col_off[M] : 0;
    p.columns = (uint32_t*)calloc(total * 6, sizeof(uint32_t));
    p.slots = (uint32_t*)calloc((total + M) * 5, sizeof(uint32_t));
    p.used = (uint64_t*)calloc(M, sizeof(uint64_t));
    p.partial = (uint64_t*)calloc(M, sizeof(uint64_t));
    p.long_ = (uint64_t*)calloc(M, sizeof(uint64_t));
    p.weak = (uint64_t*)calloc(M, sizeof(uint64_t));
    p.score_sum = (int64_t*)calloc(M, sizeof(int64_t));
    if (!p.col_off || !p.columns || !p.slots || !p.used || !p.partial || !p.long_ || !p.weak || !p.score_sum) {
        cl_monomer_pileup_free(&p);
        return CL_ERR_OUT_OF_MEMORY;
    }
    *out = p;
    return CL_OK;
}

// every argument, before a base is read; on success the classes counted in `out` and the used blocks in `plan`
int prepare(cl_context* ctx, const char* const* seqs, const uint64_t* lens, uint64_t n, const char* const* tmpl, const uint64_t* tmpl_len, uint64_t M,
            const cl_monomers_params* p, const cl_monomer_decomposition* dec, uint32_t least_share, cl_monomer_pileup* out, Plan& plan) {
    int rc = cl_monomers_check_arguments(ctx, seqs, lens, n, tmpl, tmpl_len, M, p, plan.codes, plan.tmpl_off);
    if (rc) return rc;
    if (!dec || (dec->n_blocks && !dec->blocks)) { cl_set_error(ctx, "dec: null argument"); return CL_ERR_INVALID_ARGUMENT; }
    if (least_share > kMaxShare) { cl_set_error(ctx, "least_share must lie in 0..%u (per mille), got %u", kMaxShare, least_share); return CL_ERR_INVALID_ARGUMENT; }
    if (dec->n_blocks >= (1ull << 31)) { cl_set_error(ctx, "dec: %llu blocks, 2^31 or more", (unsigned long long)dec->n_blocks); return CL_ERR_INVALID_ARGUMENT; }
    const uint64_t T = M * (uint64_t)p->strands;
    for (uint64_t b = 0; b < dec->n_blocks; ++b) {
        const cl_monomer_block& k = dec->blocks[b];
        const char* what = k.sequence >= n ? "names a sequence that does not exist" : k.monomer >= T ? "names a template that does not exist"
                           : k.start > k.end ? "starts behind its end" : k.end > lens[k.sequence] ? "ends beyond its sequence" : nullptr;
        if (what) { cl_set_error(ctx, "dec: block %llu %s", (unsigned long long)b, what); return CL_ERR_INVALID_ARGUMENT; }
    }
    if ((rc = alloc_pileup(tmpl_len, M, out))) return rc;
    std::vector<uint64_t> seq_start(n + 1, 0);
    for (uint64_t s = 0; s < n; ++s) seq_start[s + 1] = seq_start[s] + lens[s];
    std::vector<uint8_t> is_used(dec->n_blocks, 0);
    for (uint64_t b = 0; b < dec->n_blocks; ++b) {
        const cl_monomer_block& k = dec->blocks[b];
        const uint64_t m = k.monomer % M, len = tmpl_len[m];
        if (k.flags != 0) ++out->partial[m];
        else if ((uint64_t)(k.end - k.start) > 2 * len) ++out->long_[m];
        else if ((int64_t)k.score * 1000 < (int64_t)least_share * p->match * (int64_t)len) ++out->weak[m];
        else { ++out->used[m]; is_used[b] = 1; }
    }
    std::vector<uint64_t> at(M + 1, 0);
    for (uint64_t m = 0; m < M; ++m) at[m + 1] = at[m] + out->used[m];
    plan.blocks.resize(at[M]);
    plan.block_m.resize(at[M]);
    for (uint64_t b = 0; b < dec->n_blocks; ++b) {
        if (!is_used[b]) continue;
        const cl_monomer_block& k = dec->blocks[b];
        const uint64_t m = k.monomer % M, to = at[m]++;
        plan.blocks[to] = ClPileupBlock{(uint32_t)(seq_start[k.sequence] + k.start), k.end - k.start, k.monomer, k.sequence};
        plan.block_m[to] = (uint32_t)m;
    }
    return CL_OK;
}

// one used block by the definition; returns G[n][L]
int32_t align_block(const char* x, uint32_t n, const uint8_t* B, uint32_t L, bool minus, const cl_monomers_params* p, std::vector<int32_t>& G,
                    uint32_t* columns /* of the forward template */, uint32_t* slots) {
    const size_t W = (size_t)L + 1;
    G.resize((size_t)(n + 1) * W);
    for (uint32_t j = 0; j <= L; ++j) G[j] = (int32_t)j * p->deletion;
    for (uint32_t i = 1; i <= n; ++i) {
        const int xb = seq_code(x[i - 1]);
        int32_t* const row = &G[i * W];
        const int32_t* const up = row - W;
        row[0] = (int32_t)i * p->insertion;
        for (uint32_t j = 1; j <= L; ++j)
            row[j] = std::max(std::max(up[j - 1] + (xb == B[j - 1] ? p->match : p->mismatch), up[j] + p->insertion), row[j - 1] + p->deletion);
    }
    auto complement = [&](int c) { return minus && c < 4 ? 3 - c : c; };
    std::vector<int8_t> slot(L + 1, -1);
    uint32_t i = n, j = L;
    while (i > 0 || j > 0) {
        const int xb = i ? seq_code(x[i - 1]) : 4;
        const int32_t g = G[i * W + j];
        if (i && j && g == G[(i - 1) * W + j - 1] + (xb == B[j - 1] ? p->match : p->mismatch)) {
            ++columns[(size_t)(minus ? L - j : j - 1) * 6 + complement(xb)];
            --i, --j;
        } else if (i && g == G[(i - 1) * W + j] + p->insertion) {
            if (!minus || slot[j] < 0) slot[j] = (int8_t)xb;   // +: the first in sequence order is the last one met; -: the last in the block's order
            --i;
        } else {
            ++columns[(size_t)(minus ? L - j : j - 1) * 6 + 5];
            --j;
        }
    }
    for (uint32_t k = 0; k <= L; ++k)
        if (slot[k] >= 0) ++slots[(size_t)(minus ? L - k : k) * 5 + complement(slot[k])];
    return G[(size_t)n * W + L];
}

void free_templates(cl_monomer_templates* t) {
    if (t->templates) for (uint64_t m = 0; m < t->n_templates; ++m) free(t->templates[m]);
    if (t->names) for (uint64_t m = 0; m < t->n_templates; ++m) free(t->names[m]);
    free(t->templates);
    free(t->names);
    free(t->lengths);
    free(t->changed);
    free(t->round);
    memset(t, 0, sizeof(*t));
}

char* copy_string(const std::string& s) {
    char* c = (char*)malloc(s.size() + 1);
    if (c) memcpy(c, s.c_str(), s.size() + 1);
    return c;
}

int fill_templates(const std::vector<std::string>& strings, const std::vector<uint8_t>& changed, const std::vector<std::string>* names, cl_monomer_templates* out) {
    cl_monomer_templates t;
    memset(&t, 0, sizeof(t));
    const uint64_t M = strings.size();
    t.n_templates = M;
    t.templates = (char**)calloc(std::max<uint64_t>(M, 1), sizeof(char*));
    t.lengths = (uint64_t*)calloc(std::max<uint64_t>(M, 1), sizeof(uint64_t));
    t.changed = (uint8_t*)calloc(std::max<uint64_t>(M, 1), 1);
    if (names) t.names = (char**)calloc(std::max<uint64_t>(M, 1), sizeof(char*));
    bool ok = t.templates && t.lengths && t.changed && (!names || t.names);
    for (uint64_t m = 0; ok && m < M; ++m) {
        ok = (t.templates[m] = copy_string(strings[m])) != nullptr;
        t.lengths[m] = strings[m].size();
        t.changed[m] = changed.empty() ? 0 : changed[m];
        if (ok && names) ok = (t.names[m] = copy_string((*names)[m])) != nullptr;
    }
    if (!ok) { free_templates(&t); return CL_ERR_OUT_OF_MEMORY; }
    *out = t;
    return CL_OK;
}

int check_templates(const char* const* tmpl, const uint64_t* tmpl_len, uint64_t M) {
    if (M < 1 || !tmpl || !tmpl_len) { cl_set_error(nullptr, "templates: at least 1 template is needed"); return CL_ERR_INVALID_ARGUMENT; }
    for (uint64_t m = 0; m < M; ++m)
        if (!tmpl[m] || tmpl_len[m] < 1 || tmpl_len[m] > kMaxTemplate) {
            cl_set_error(nullptr, "templates: template %llu has %llu bases, not 1..%llu", (unsigned long long)m, (unsigned long long)tmpl_len[m], (unsigned long long)kMaxTemplate);
            return CL_ERR_INVALID_ARGUMENT;
        }
    return CL_OK;
}

int check_pileup(const cl_monomer_pileup* p, const uint64_t* tmpl_len, uint64_t M) {
    if (!p || !p->col_off || !p->columns || !p->slots || !p->used) { cl_set_error(nullptr, "pileup: null argument"); return CL_ERR_INVALID_ARGUMENT; }
    if (p->n_templates != M) {
        cl_set_error(nullptr, "pileup: it holds %llu templates, %llu were given", (unsigned long long)p->n_templates, (unsigned long long)M);
        return CL_ERR_INVALID_ARGUMENT;
    }
    for (uint64_t m = 0; m < M; ++m)
        if (p->col_off[m + 1] - p->col_off[m] != tmpl_len[m]) {
            cl_set_error(nullptr, "pileup: template %llu has %llu columns there and %llu bases here", (unsigned long long)m,
                         (unsigned long long)(p->col_off[m + 1] - p->col_off[m]), (unsigned long long)tmpl_len[m]);
            return CL_ERR_INVALID_ARGUMENT;
        }
    return CL_OK;
}

void vote(const cl_monomer_pileup* p, const char* const* tmpl, const uint64_t* tmpl_len, uint64_t M, std::vector<std::string>& result, std::vector<uint8_t>& changed) {
    static const char kBase[5] = "ACGT";
    result.assign(M, std::string());
    changed.assign(M, 0);
    for (uint64_t m = 0; m < M; ++m) {
        const uint64_t L = tmpl_len[m], d = p->used[m];
        const std::string old(tmpl[m], L);
        std::string next;
        for (uint64_t c = 0; d > 0 && c <= L; ++c) {
            const uint32_t* s = p->slots + (p->col_off[m] + m + c) * 5;
            const uint64_t inserted = (uint64_t)s[0] + s[1] + s[2] + s[3] + s[4];
            const uint32_t smax = std::max(std::max(s[0], s[1]), std::max(s[2], s[3]));
            if (2 * inserted > d && smax > 0)
                for (int k = 0; k < 4; ++k) if (s[k] == smax) { next += kBase[k]; break; }
            if (c == L) break;
            const uint32_t* col = p->columns + (p->col_off[m] + c) * 6;
            if (2 * (uint64_t)col[5] > d) continue;
            const uint32_t mx = std::max(std::max(col[0], col[1]), std::max(col[2], col[3]));
            const int own = seq_code(old[c]);
            if (mx == 0) next += old[c];
            else if (own < 4 && col[own] == mx) next += kBase[own];
            else for (int k = 0; k < 4; ++k) if (col[k] == mx) { next += kBase[k]; break; }
        }
        if (d == 0 || next.empty() || next.size() > kMaxTemplate) next = old;
        changed[m] = next != old;
        result[m] = next;
    }
}

inline const char* sequences_at(const char* const* seqs, const std::vector<uint64_t>& seq_start, const ClPileupBlock& k) {
    return seqs[k.seq] + (k.text_off - seq_start[k.seq]);
}

int copy_text(const std::string& s, char** text_out, uint64_t* len_out) {
    char* text = copy_string(s);
    if (!text) return CL_ERR_OUT_OF_MEMORY;
    *text_out = text;
    if (len_out) *len_out = s.size();
    return CL_OK;
}

int pileup_any(cl_context* ctx, bool device, const char* const* seqs, const uint64_t* lens, uint64_t n, const char* const* tmpl, const uint64_t* tmpl_len, uint64_t M,
               const cl_monomers_params* p, const cl_monomer_decomposition* dec, uint32_t least_share, cl_monomer_pileup* out) {
    if (out) memset(out, 0, sizeof(*out));
    if (!out || (device && !ctx)) { cl_set_error(ctx, "null argument"); return CL_ERR_INVALID_ARGUMENT; }
    Plan plan;
    cl_monomer_pileup pile;
    memset(&pile, 0, sizeof(pile));
    int rc = prepare(ctx, seqs, lens, n, tmpl, tmpl_len, M, p, dec, least_share, &pile, plan);
    if (rc) return rc;
    const size_t U = plan.blocks.size();
    if (device) {
        std::vector<int32_t> scores;
        const uint64_t total = pile.col_off[M];
        rc = cl_monomer_pileup_device(ctx, seqs, lens, n, plan.codes, plan.tmpl_off, (uint32_t)M, p, plan.blocks, pile.columns, total * 6, pile.slots, (total + M) * 5,
                                      scores, &pile.align_ms, &pile.count_ms);
        if (rc) { cl_monomer_pileup_free(&pile); return rc; }
        for (size_t b = 0; b < U; ++b) pile.score_sum[plan.block_m[b]] += scores[b];
    } else {
        std::vector<uint64_t> seq_start(n + 1, 0);
        for (uint64_t s = 0; s < n; ++s) seq_start[s + 1] = seq_start[s] + lens[s];
        std::vector<int32_t> G;
        for (size_t b = 0; b < U; ++b) {
            const ClPileupBlock& k = plan.blocks[b];
            const uint32_t m = plan.block_m[b], a0 = plan.tmpl_off[k.monomer], L = plan.tmpl_off[k.monomer + 1] - a0;
            const char* x = k.n ? sequences_at(seqs, seq_start, k) : "";
            pile.score_sum[m] += align_block(x, k.n, plan.codes.data() + a0, L, k.monomer >= M, p, G, pile.columns + pile.col_off[m] * 6,
                                             pile.slots + (pile.col_off[m] + m) * 5);
        }
    }
    *out = pile;
    return CL_OK;
}

int refine_any(cl_context* ctx, bool device, const char* const* seqs, const uint64_t* lens, uint64_t n, const char* const* tmpl, const uint64_t* tmpl_len, uint64_t M,
               const cl_monomers_params* p, uint32_t least_share, uint32_t max_rounds, cl_monomer_templates* out) {
    if (out) memset(out, 0, sizeof(*out));
    if (!out || (device && !ctx)) { cl_set_error(ctx, "null argument"); return CL_ERR_INVALID_ARGUMENT; }
    if (max_rounds < 1 || max_rounds > kMaxRounds) { cl_set_error(ctx, "max_rounds must lie in 1..%u, got %u", kMaxRounds, max_rounds); return CL_ERR_INVALID_ARGUMENT; }
    if (least_share > kMaxShare) { cl_set_error(ctx, "least_share must lie in 0..%u (per mille), got %u", kMaxShare, least_share); return CL_ERR_INVALID_ARGUMENT; }
    {
        std::vector<uint8_t> codes;
        std::vector<uint32_t> off;
        const int rc = cl_monomers_check_arguments(ctx, seqs, lens, n, tmpl, tmpl_len, M, p, codes, off);
        if (rc) return rc;
    }
    std::vector<std::string> T(M), first(M);
    for (uint64_t m = 0; m < M; ++m) first[m] = T[m] = std::string(tmpl[m], tmpl_len[m]);
    std::vector<cl_monomer_round> rounds;
    int converged = 0;
    for (uint32_t r = 1; r <= max_rounds; ++r) {
        std::vector<const char*> ptr(M);
        std::vector<uint64_t> len(M);
        for (uint64_t m = 0; m < M; ++m) { ptr[m] = T[m].c_str(); len[m] = T[m].size(); }
        cl_monomer_decomposition dec;
        int rc = device ? cl_monomer_decompose_compute(ctx, seqs, lens, n, ptr.data(), len.data(), M, p, &dec)
                        : cl_monomer_decompose_host(seqs, lens, n, ptr.data(), len.data(), M, p, &dec);
        if (rc) return rc;
        cl_monomer_pileup pile;
        rc = pileup_any(ctx, device, seqs, lens, n, ptr.data(), len.data(), M, p, &dec, least_share, &pile);
        cl_monomer_round round;
        memset(&round, 0, sizeof(round));
        round.blocks = dec.n_blocks;
        round.dp_ms = dec.dp_ms;
        round.trace_ms = dec.trace_ms;
        cl_monomer_decomposition_free(&dec);
        if (rc) return rc;
        std::vector<std::string> next;
        std::vector<uint8_t> changed;
        vote(&pile, ptr.data(), len.data(), M, next, changed);
        for (uint64_t m = 0; m < M; ++m) { round.used += pile.used[m]; round.changed += changed[m]; }
        round.align_ms = pile.align_ms;
        round.count_ms = pile.count_ms;
        cl_monomer_pileup_free(&pile);
        rounds.push_back(round);
        if (round.changed == 0) { converged = 1; break; }
        uint64_t bases = 0;
        for (const std::string& t : next) bases += t.size() * (uint64_t)p->strands;
        if (bases > kMaxTemplateBases) break;   // the next round could not decompose under them
        T.swap(next);
    }
    std::vector<uint8_t> changed(M);
    for (uint64_t m = 0; m < M; ++m) changed[m] = T[m] != first[m];
    cl_monomer_templates t;
    int rc = fill_templates(T, changed, nullptr, &t);
    if (rc) return rc;
    t.rounds = (uint32_t)rounds.size();
    t.converged = converged;
    t.round = (cl_monomer_round*)malloc(rounds.size() * sizeof(cl_monomer_round));
    if (!t.round) { free_templates(&t); return CL_ERR_OUT_OF_MEMORY; }
    memcpy(t.round, rounds.data(), rounds.size() * sizeof(cl_monomer_round));
    *out = t;
    return CL_OK;
}

}  // namespace

extern "C" {

void cl_monomer_pileup_free(cl_monomer_pileup* out) {
    if (!out) return;
    free(out->col_off);
    free(out->columns);
    free(out->slots);
    free(out->used);
    free(out->partial);
    free(out->long_);
    free(out->weak);
    free(out->score_sum);
    memset(out, 0, sizeof(*out));
}

void cl_monomer_templates_free(cl_monomer_templates* out) {
    if (out) free_templates(out);
}

int cl_monomer_pileup_host(const char* const* sequences, const uint64_t* lengths, uint64_t n, const char* const* templates, const uint64_t* template_lengths,
                           uint64_t n_templates, const cl_monomers_params* params, const cl_monomer_decomposition* dec, uint32_t least_share, cl_monomer_pileup* out) {
    return pileup_any(nullptr, false, sequences, lengths, n, templates, template_lengths, n_templates, params, dec, least_share, out);
}

int cl_monomer_pileup_compute(cl_context* ctx, const char* const* sequences, const uint64_t* lengths, uint64_t n, const char* const* templates,
                              const uint64_t* template_lengths, uint64_t n_templates, const cl_monomers_params* params, const cl_monomer_decomposition* dec,
                              uint32_t least_share, cl_monomer_pileup* out) {
    cl_bind_device(ctx);
    return pileup_any(ctx, true, sequences, lengths, n, templates, template_lengths, n_templates, params, dec, least_share, out);
}

int cl_monomer_consensus(const cl_monomer_pileup* pileup, const char* const* templates, const uint64_t* template_lengths, uint64_t n_templates,
                         cl_monomer_templates* out) {
    if (out) memset(out, 0, sizeof(*out));
    if (!out) { cl_set_error(nullptr, "null argument"); return CL_ERR_INVALID_ARGUMENT; }
    int rc = check_templates(templates, template_lengths, n_templates);
    if (rc || (rc = check_pileup(pileup, template_lengths, n_templates))) return rc;
    std::vector<std::string> next;
    std::vector<uint8_t> changed;
    vote(pileup, templates, template_lengths, n_templates, next, changed);
    return fill_templates(next, changed, nullptr, out);
}

int cl_monomer_templates_refine_host(const char* const* sequences, const uint64_t* lengths, uint64_t n, const char* const* templates,
                                     const uint64_t* template_lengths, uint64_t n_templates, const cl_monomers_params* params, uint32_t least_share,
                                     uint32_t max_rounds, cl_monomer_templates* out) {
    return refine_any(nullptr, false, sequences, lengths, n, templates, template_lengths, n_templates, params, least_share, max_rounds, out);
}

int cl_monomer_templates_refine_compute(cl_context* ctx, const char* const* sequences, const uint64_t* lengths, uint64_t n, const char* const* templates,
                                        const uint64_t* template_lengths, uint64_t n_templates, const cl_monomers_params* params, uint32_t least_share,
                                        uint32_t max_rounds, cl_monomer_templates* out) {
    cl_bind_device(ctx);
    return refine_any(ctx, true, sequences, lengths, n, templates, template_lengths, n_templates, params, least_share, max_rounds, out);
}

int cl_monomer_seed_templates(const char* const* sequences, const uint64_t* lengths, uint64_t n, uint32_t period, uint32_t count, uint64_t start, int strands,
                              cl_monomer_templates* out) {
    if (out) memset(out, 0, sizeof(*out));
    if (!out) { cl_set_error(nullptr, "null argument"); return CL_ERR_INVALID_ARGUMENT; }
    if (strands != 1 && strands != 2) { cl_set_error(nullptr, "strands must be 1 or 2, got %d", strands); return CL_ERR_INVALID_ARGUMENT; }
    if (period < 1 || period > kMaxTemplate) { cl_set_error(nullptr, "period must lie in 1..%llu, got %u", (unsigned long long)kMaxTemplate, period); return CL_ERR_INVALID_ARGUMENT; }
    if (count < 1 || (uint64_t)count * period * (uint64_t)strands > kMaxTemplateBases) {
        cl_set_error(nullptr, "count: %u seeds of %u bases are none or more than %llu bases in all (both strands counted)", count, period, (unsigned long long)kMaxTemplateBases);
        return CL_ERR_INVALID_ARGUMENT;
    }
    if (n < 1 || !sequences || !lengths || (lengths[0] && !sequences[0])) { cl_set_error(nullptr, "sequences: seeds are cut from the first sequence, there is none"); return CL_ERR_INVALID_ARGUMENT; }
    const uint64_t need = (uint64_t)count * period;
    if (start > lengths[0] || lengths[0] - start < need) {
        cl_set_error(nullptr, "start: %u seeds of %u bases from base %llu need %llu bases, the first sequence has %llu", count, period, (unsigned long long)start,
                     (unsigned long long)need, (unsigned long long)lengths[0]);
        return CL_ERR_INVALID_ARGUMENT;
    }
    std::vector<std::string> strings(count), names(count);
    for (uint32_t k = 0; k < count; ++k) {
        strings[k].assign(sequences[0] + start + (uint64_t)k * period, period);
        names[k] = "seed" + std::to_string(k + 1);
        bool any = false;
        for (char c : strings[k]) any = any || seq_code(c) < 4;
        if (!any) { cl_set_error(nullptr, "start: seed %u (bases %llu..) holds no character of ACGTacgt", k + 1, (unsigned long long)(start + (uint64_t)k * period)); return CL_ERR_INVALID_ARGUMENT; }
    }
    return fill_templates(strings, std::vector<uint8_t>(), &names, out);
}

int cl_monomer_pileup_tsv(const cl_monomer_pileup* pileup, const char* const* template_names, const char* const* templates, const uint64_t* template_lengths,
                          uint64_t n_templates, char** text_out, uint64_t* len_out) {
    if (text_out) *text_out = nullptr;
    if (len_out) *len_out = 0;
    if (!text_out || !template_names) { cl_set_error(nullptr, "null argument"); return CL_ERR_INVALID_ARGUMENT; }
    int rc = check_templates(templates, template_lengths, n_templates);
    if (rc || (rc = check_pileup(pileup, template_lengths, n_templates))) return rc;
    for (uint64_t m = 0; m < n_templates; ++m)
        if (!template_names[m]) { cl_set_error(nullptr, "template_names: template %llu has no name", (unsigned long long)m); return CL_ERR_INVALID_ARGUMENT; }
    std::string tsv = "monomer\tposition\tbase\tA\tC\tG\tT\tother\tdeleted\tins_A\tins_C\tins_G\tins_T\tins_other\n";
    char num[256];
    static const uint32_t kZero[6] = {0, 0, 0, 0, 0, 0};
    for (uint64_t m = 0; m < n_templates; ++m)
        for (uint64_t j = 0; j <= template_lengths[m]; ++j) {
            const bool end = j == template_lengths[m];
            const uint32_t* c = end ? kZero : pileup->columns + (pileup->col_off[m] + j) * 6;
            const uint32_t* s = pileup->slots + (pileup->col_off[m] + m + j) * 5;
            tsv += template_names[m];
            snprintf(num, sizeof(num), "\t%llu\t%c\t%u\t%u\t%u\t%u\t%u\t%u\t%u\t%u\t%u\t%u\t%u\n", (unsigned long long)j, end ? '.' : templates[m][j], c[0], c[1], c[2], c[3],
                     c[4], c[5], s[0], s[1], s[2], s[3], s[4]);
            tsv += num;
        }
    return copy_text(tsv, text_out, len_out);
}

int cl_monomer_templates_fasta(const char* const* names, const char* const* templates, const uint64_t* template_lengths, uint64_t n_templates, char** text_out,
                               uint64_t* len_out) {
    if (text_out) *text_out = nullptr;
    if (len_out) *len_out = 0;
    if (!text_out || !names) { cl_set_error(nullptr, "null argument"); return CL_ERR_INVALID_ARGUMENT; }
    const int rc = check_templates(templates, template_lengths, n_templates);
    if (rc) return rc;
    std::string fa;
    for (uint64_t m = 0; m < n_templates; ++m) {
        if (!names[m]) { cl_set_error(nullptr, "names: template %llu has no name", (unsigned long long)m); return CL_ERR_INVALID_ARGUMENT; }
        fa += ">";
        fa += names[m];
        fa += "\n";
        fa.append(templates[m], template_lengths[m]);
        fa += "\n";
    }
    return copy_text(fa, text_out, len_out);
}

}  // extern "C"
