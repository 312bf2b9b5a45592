// cl_monomers_api.cpp — monomer decomposition (the reference has none): the definition on the host (cl_monomer_decompose_host), the host half of
// the device path (cl_monomer_decompose_compute over monomers_kernels.hip) and the two TSV writers.  Integers throughout; the one double,
// share = score / (match * len), exists only in the text.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "cl_internal.hpp"

namespace {

constexpr uint64_t kMaxText = 1ull << 30, kMaxTemplate = 1024, kMaxTemplateBases = 8192;
constexpr uint32_t kMaxChunk = 1u << 20, kMinChunk = 64, kMaxOverlap = 1u << 20;
constexpr int32_t kMaxScore = 64;

int seq_code(char c) {   // 4: matches nothing
    switch (c) {
    case 'A': case 'a': return 0;
    case 'C': case 'c': return 1;
    case 'G': case 'g': return 2;
    case 'T': case 't': return 3;
    default: return 4;
    }
}

// every limit of the header; on success the templates' codes (reverse complements behind the forward ones) and the problems in their order
int check_arguments(cl_context* ctx, const char* const* seqs, const uint64_t* lens, uint64_t n, const char* const* tmpl, const uint64_t* tmpl_len, uint64_t M,
                    const cl_monomers_params* p, std::vector<uint8_t>& codes, std::vector<uint32_t>& tmpl_off, std::vector<ClMonomerProblem>& problems) {
    if (!p || (n && (!seqs || !lens))) { cl_set_error(ctx, "null argument"); return CL_ERR_INVALID_ARGUMENT; }
    if (M < 1 || !tmpl || !tmpl_len) { cl_set_error(ctx, "templates: a decomposition needs at least 1 template"); return CL_ERR_INVALID_ARGUMENT; }
    if (p->strands != 1 && p->strands != 2) { cl_set_error(ctx, "strands must be 1 or 2, got %d", p->strands); return CL_ERR_INVALID_ARGUMENT; }
    if (p->match < 1 || p->match > kMaxScore) { cl_set_error(ctx, "match must lie in 1..%d, got %d", kMaxScore, p->match); return CL_ERR_INVALID_ARGUMENT; }
    const struct { const char* name; int32_t v; } penalties[3] = {{"mismatch", p->mismatch}, {"insertion", p->insertion}, {"deletion", p->deletion}};
    for (const auto& q : penalties)
        if (q.v > -1 || q.v < -kMaxScore) { cl_set_error(ctx, "%s must lie in -%d..-1, got %d", q.name, kMaxScore, q.v); return CL_ERR_INVALID_ARGUMENT; }
    if (p->chunk != 0 && (p->chunk < kMinChunk || p->chunk > kMaxChunk)) {
        cl_set_error(ctx, "chunk must be 0 or lie in %u..%u, got %u", kMinChunk, kMaxChunk, p->chunk);
        return CL_ERR_INVALID_ARGUMENT;
    }
    if (p->overlap > kMaxOverlap) { cl_set_error(ctx, "overlap must be at most %u, got %u", kMaxOverlap, p->overlap); return CL_ERR_INVALID_ARGUMENT; }
    uint64_t bases = 0;
    for (uint64_t m = 0; m < M; ++m) {
        if (tmpl_len[m] < 1 || tmpl_len[m] > kMaxTemplate || !tmpl[m]) {
            cl_set_error(ctx, "templates: template %llu has %llu bases, not 1..%llu", (unsigned long long)m, (unsigned long long)tmpl_len[m], (unsigned long long)kMaxTemplate);
            return CL_ERR_INVALID_ARGUMENT;
        }
        if ((bases += tmpl_len[m] * (uint64_t)p->strands) > kMaxTemplateBases) {
            cl_set_error(ctx, "templates: more than %llu template bases in all (both strands counted), at template %llu", (unsigned long long)kMaxTemplateBases,
                         (unsigned long long)m);
            return CL_ERR_INVALID_ARGUMENT;
        }
    }
    uint64_t text = 0;
    for (uint64_t s = 0; s < n; ++s) {
        if (lens[s] && !seqs[s]) { cl_set_error(ctx, "sequences: sequence %llu is null", (unsigned long long)s); return CL_ERR_INVALID_ARGUMENT; }
        if (lens[s] >= kMaxText || (text += lens[s]) >= kMaxText) {
            cl_set_error(ctx, "lengths: the sequences hold 2^30 bases or more (at sequence %llu)", (unsigned long long)s);
            return CL_ERR_INVALID_ARGUMENT;
        }
    }
    if (n >= (1ull << 28)) { cl_set_error(ctx, "n: %llu sequences, 2^28 or more", (unsigned long long)n); return CL_ERR_INVALID_ARGUMENT; }
    codes.clear();
    tmpl_off.assign(1, 0);
    for (uint64_t m = 0; m < M; ++m) {
        for (uint64_t j = 0; j < tmpl_len[m]; ++j) { const int c = seq_code(tmpl[m][j]); codes.push_back((uint8_t)(c > 3 ? 5 : c)); }
        tmpl_off.push_back((uint32_t)codes.size());
    }
    if (p->strands == 2)
        for (uint64_t m = 0; m < M; ++m) {
            for (uint64_t j = tmpl_len[m]; j-- > 0;) { const uint8_t c = codes[tmpl_off[m] + j]; codes.push_back(c > 3 ? c : (uint8_t)(3 - c)); }
            tmpl_off.push_back((uint32_t)codes.size());
        }
    problems.clear();
    uint64_t text_off = 0, rec_off = 0;
    for (uint64_t s = 0; s < n; ++s) {
        const uint64_t L = lens[s], C = p->chunk, V = p->overlap;
        const uint64_t chunks = C ? (L + C - 1) / C : 1;
        for (uint64_t c = 0; c < chunks; ++c) {
            ClMonomerProblem q{};
            const uint64_t lo = C ? (c * C > V ? c * C - V : 0) : 0, hi = C ? std::min(L, (c + 1) * C + V) : L;
            q.text_off = text_off + lo;
            q.rec_off = rec_off;
            q.n = (uint32_t)(hi - lo);
            q.row0 = (uint32_t)lo;
            q.keep_lo = C ? (uint32_t)(c * C) : 0u;
            q.keep_hi = C ? (uint32_t)std::min<uint64_t>((c + 1) * C, 0xFFFFFFFFull) : 0xFFFFFFFFu;
            q.seq = (uint32_t)s;
            rec_off += q.n;
            problems.push_back(q);
        }
        text_off += L;
    }
    return CL_OK;
}

struct Value { int64_t score; int64_t start; };
inline bool better(const Value& a, const Value& b) { return a.score != b.score ? a.score > b.score : a.start > b.start; }
inline Value best(const Value& a, const Value& b) { return better(b, a) ? b : a; }
inline int32_t saturate(int64_t v) { return (int32_t)std::max<int64_t>(INT32_MIN, std::min<int64_t>(INT32_MAX, v)); }

// one problem by the definition: the kept blocks, ascending, in absolute coordinates
void solve_problem(const char* S, const ClMonomerProblem& q, const std::vector<uint8_t>& codes, const std::vector<uint32_t>& tmpl_off, const cl_monomers_params* p,
                   std::vector<cl_monomer_block>& out) {
    const uint64_t n = q.n;
    if (n == 0) return;
    const size_t T = tmpl_off.size() - 1, A = codes.size();
    std::vector<Value> prev(A, Value{0, -1}), cur(A), D(A);   // cells j = 1 .. len_m of every template; cell j = 0 is (E, i)
    std::vector<int64_t> E(n + 1, 0), rec_start(n + 1, 0);
    std::vector<uint32_t> rec_m(n + 1, 0);
    for (uint64_t i = 1; i <= n; ++i) {
        const int sb = seq_code(S[i - 1]);
        const Value zero{E[i - 1], (int64_t)i - 1};
        Value rec{0, 0};
        uint32_t rm = 0;
        for (size_t m = 0; m < T; ++m) {
            const uint32_t a0 = tmpl_off[m], len = tmpl_off[m + 1] - a0;
            for (uint32_t j = 1; j <= len; ++j) {
                const Value& diag = j == 1 ? zero : prev[a0 + j - 2];
                const Value t = best(Value{diag.score + (sb == codes[a0 + j - 1] ? p->match : p->mismatch), diag.start},
                                     Value{prev[a0 + j - 1].score + p->insertion, prev[a0 + j - 1].start});
                D[a0 + j - 1] = j == 1 ? t : best(t, Value{D[a0 + j - 2].score + p->deletion, D[a0 + j - 2].start});
            }
            if (m == 0 || better(D[a0 + len - 1], rec)) { rec = D[a0 + len - 1]; rm = (uint32_t)m; }
        }
        E[i] = rec.score;
        rec_start[i] = rec.start;
        rec_m[i] = rm;
        for (size_t m = 0; m < T; ++m) {
            const uint32_t a0 = tmpl_off[m], len = tmpl_off[m + 1] - a0;
            for (uint32_t j = 1; j <= len; ++j) cur[a0 + j - 1] = best(D[a0 + j - 1], Value{E[i] + (int64_t)j * p->deletion, (int64_t)i});
        }
        prev.swap(cur);
    }
    Value close{0, 0};
    uint32_t close_m = 0, close_j = 0;
    for (size_t m = 0; m < T; ++m) {
        const uint32_t a0 = tmpl_off[m], len = tmpl_off[m + 1] - a0;
        for (uint32_t j = 1; j <= len; ++j)   // ties: the smallest m, then the largest j
            if (close_j == 0 || better(prev[a0 + j - 1], close) || (m == close_m && !better(close, prev[a0 + j - 1]))) { close = prev[a0 + j - 1]; close_m = (uint32_t)m; close_j = j; }
    }
    std::vector<cl_monomer_block> found;   // descending
    auto emit = [&](const Value& v, uint64_t end, uint32_t m, uint32_t flags) {
        const uint64_t start = v.start < 0 ? 0 : (uint64_t)v.start;
        cl_monomer_block b;
        b.sequence = q.seq;
        b.start = (uint32_t)(q.row0 + start);
        b.end = (uint32_t)(q.row0 + end);
        b.monomer = m;
        b.score = saturate(v.score - E[start]);
        b.flags = flags | (v.start < 0 ? CL_MONOMER_PARTIAL_LEFT : 0u);
        if (b.start >= q.keep_lo && b.start < q.keep_hi) found.push_back(b);
        return start;
    };
    uint64_t i = emit(close, n, close_m, close_j < tmpl_off[close_m + 1] - tmpl_off[close_m] ? CL_MONOMER_PARTIAL_RIGHT : 0u);
    while (i > 0) i = emit(Value{E[i], rec_start[i]}, i, rec_m[i], 0u);
    out.insert(out.end(), found.rbegin(), found.rend());
}

int finish(std::vector<cl_monomer_block>& blocks, uint64_t n, uint64_t n_problems, cl_monomer_decomposition* out) {
    cl_monomer_decomposition d;
    memset(&d, 0, sizeof(d));
    d.n_seq = n;
    d.n_blocks = blocks.size();
    d.n_problems = n_problems;
    d.seq_off = (uint64_t*)calloc(n + 1, sizeof(uint64_t));
    d.blocks = (cl_monomer_block*)malloc(std::max<size_t>(blocks.size(), 1) * sizeof(cl_monomer_block));
    if (!d.seq_off || !d.blocks) { cl_monomer_decomposition_free(&d); return CL_ERR_OUT_OF_MEMORY; }
    if (!blocks.empty()) memcpy(d.blocks, blocks.data(), blocks.size() * sizeof(cl_monomer_block));
    for (const cl_monomer_block& b : blocks) ++d.seq_off[b.sequence + 1];
    for (uint64_t s = 0; s < n; ++s) d.seq_off[s + 1] += d.seq_off[s];
    *out = d;
    return CL_OK;
}

int copy_text(const std::string& tsv, char** text_out, uint64_t* len_out) {
    char* text = (char*)malloc(tsv.size() + 1);
    if (!text) return CL_ERR_OUT_OF_MEMORY;
    memcpy(text, tsv.c_str(), tsv.size() + 1);
    *text_out = text;
    if (len_out) *len_out = tsv.size();
    return CL_OK;
}

int check_text_arguments(const cl_monomer_decomposition* d, const char* const* names, const char* const* tmpl_names, const uint64_t* tmpl_len, uint64_t M,
                         const cl_monomers_params* p, char** text_out, uint64_t* len_out) {
    if (text_out) *text_out = nullptr;
    if (len_out) *len_out = 0;
    if (!d || !tmpl_names || !tmpl_len || !p || !text_out || !d->seq_off || (d->n_blocks && !d->blocks) || (d->n_seq && !names)) {
        cl_set_error(nullptr, "null argument");
        return CL_ERR_INVALID_ARGUMENT;
    }
    if (M < 1) { cl_set_error(nullptr, "templates: a decomposition has at least 1 template"); return CL_ERR_INVALID_ARGUMENT; }
    if (p->match < 1) { cl_set_error(nullptr, "match must be at least 1, got %d", p->match); return CL_ERR_INVALID_ARGUMENT; }
    if (p->strands != 1 && p->strands != 2) { cl_set_error(nullptr, "strands must be 1 or 2, got %d", p->strands); return CL_ERR_INVALID_ARGUMENT; }
    for (uint64_t s = 0; s < d->n_seq; ++s)
        if (!names[s]) { cl_set_error(nullptr, "names: sequence %llu has no name", (unsigned long long)s); return CL_ERR_INVALID_ARGUMENT; }
    for (uint64_t m = 0; m < M; ++m)
        if (!tmpl_names[m] || tmpl_len[m] < 1) { cl_set_error(nullptr, "templates: template %llu has no name or no bases", (unsigned long long)m); return CL_ERR_INVALID_ARGUMENT; }
    for (uint64_t b = 0; b < d->n_blocks; ++b)
        if (d->blocks[b].sequence >= d->n_seq || d->blocks[b].monomer >= M * (uint64_t)p->strands) {
            cl_set_error(nullptr, "blocks: block %llu names a sequence or a template that does not exist", (unsigned long long)b);
            return CL_ERR_INVALID_ARGUMENT;
        }
    return CL_OK;
}

}  // namespace

int cl_monomers_check_arguments(cl_context* ctx, const char* const* seqs, const uint64_t* lens, uint64_t n, const char* const* tmpl, const uint64_t* tmpl_len,
                                uint64_t M, const cl_monomers_params* p, std::vector<uint8_t>& codes, std::vector<uint32_t>& tmpl_off) {
    std::vector<ClMonomerProblem> problems;
    return check_arguments(ctx, seqs, lens, n, tmpl, tmpl_len, M, p, codes, tmpl_off, problems);
}

extern "C" {

void cl_monomers_params_default(cl_monomers_params* params) {
    if (!params) return;
    params->match = 1;
    params->mismatch = -1;
    params->insertion = -1;
    params->deletion = -1;
    params->chunk = 4096;
    params->overlap = 512;
    params->strands = 1;
}

void cl_monomer_decomposition_free(cl_monomer_decomposition* out) {
    if (!out) return;
    free(out->seq_off);
    free(out->blocks);
    memset(out, 0, sizeof(*out));
}

int cl_monomer_decompose_host(const char* const* sequences, const uint64_t* lengths, uint64_t n, const char* const* templates, const uint64_t* template_lengths,
                              uint64_t n_templates, const cl_monomers_params* params, cl_monomer_decomposition* out) {
    if (out) memset(out, 0, sizeof(*out));
    if (!out) { cl_set_error(nullptr, "null argument"); return CL_ERR_INVALID_ARGUMENT; }
    std::vector<uint8_t> codes;
    std::vector<uint32_t> tmpl_off;
    std::vector<ClMonomerProblem> problems;
    const int rc = check_arguments(nullptr, sequences, lengths, n, templates, template_lengths, n_templates, params, codes, tmpl_off, problems);
    if (rc) return rc;
    std::vector<cl_monomer_block> blocks;
    for (const ClMonomerProblem& q : problems) solve_problem(sequences[q.seq] + q.row0, q, codes, tmpl_off, params, blocks);
    return finish(blocks, n, problems.size(), out);
}

int cl_monomer_decompose_compute(cl_context* ctx, const char* const* sequences, const uint64_t* lengths, uint64_t n, const char* const* templates,
                                 const uint64_t* template_lengths, uint64_t n_templates, const cl_monomers_params* params, cl_monomer_decomposition* out) {
    cl_bind_device(ctx);
    if (out) memset(out, 0, sizeof(*out));
    if (!ctx || !out) { cl_set_error(ctx, "null argument"); return CL_ERR_INVALID_ARGUMENT; }
    std::vector<uint8_t> codes;
    std::vector<uint32_t> tmpl_off;
    std::vector<ClMonomerProblem> problems;
    int rc = check_arguments(ctx, sequences, lengths, n, templates, template_lengths, n_templates, params, codes, tmpl_off, problems);
    if (rc) return rc;
    std::vector<cl_monomer_block> blocks;
    float dp_ms = 0.f, trace_ms = 0.f;
    if ((rc = cl_monomers_device(ctx, sequences, lengths, n, codes, tmpl_off, params, problems, blocks, &dp_ms, &trace_ms))) return rc;
    if ((rc = finish(blocks, n, problems.size(), out))) return rc;
    out->dp_ms = dp_ms;
    out->trace_ms = trace_ms;
    return CL_OK;
}

int cl_monomers_tsv(const cl_monomer_decomposition* dec, const char* const* names, const char* const* template_names, const uint64_t* template_lengths,
                    uint64_t n_templates, const cl_monomers_params* params, char** text_out, uint64_t* len_out) {
    const int rc = check_text_arguments(dec, names, template_names, template_lengths, n_templates, params, text_out, len_out);
    if (rc) return rc;
    std::string tsv = "sample\tstart\tend\tmonomer\tstrand\tscore\tshare\tpartial\n";
    char num[200];
    static const char* const kPartial[4] = {".", "L", "R", "LR"};
    for (uint64_t i = 0; i < dec->n_blocks; ++i) {
        const cl_monomer_block& b = dec->blocks[i];
        const uint64_t m = b.monomer % n_templates;
        tsv += names[b.sequence];
        snprintf(num, sizeof(num), "\t%u\t%u\t", b.start, b.end);
        tsv += num;
        tsv += template_names[m];
        snprintf(num, sizeof(num), "\t%c\t%d\t%.9g\t%s\n", b.monomer < n_templates ? '+' : '-', b.score,
                 (double)b.score / ((double)params->match * (double)template_lengths[m]), kPartial[b.flags & 3u]);
        tsv += num;
    }
    return copy_text(tsv, text_out, len_out);
}

int cl_monomers_summary_tsv(const cl_monomer_decomposition* dec, const char* const* names, const char* const* template_names, const uint64_t* template_lengths,
                            uint64_t n_templates, const cl_monomers_params* params, char** text_out, uint64_t* len_out) {
    const int rc = check_text_arguments(dec, names, template_names, template_lengths, n_templates, params, text_out, len_out);
    if (rc) return rc;
    std::string tsv = "sample\tmonomer\tstrand\tblocks\tbases\tscore\n";
    char num[200];
    const uint64_t T = n_templates * 2;
    std::vector<uint64_t> count(T), bases(T);
    std::vector<int64_t> score(T);
    for (uint64_t s = 0; s < dec->n_seq; ++s) {
        std::fill(count.begin(), count.end(), 0);
        std::fill(bases.begin(), bases.end(), 0);
        std::fill(score.begin(), score.end(), 0);
        for (uint64_t i = dec->seq_off[s]; i < dec->seq_off[s + 1]; ++i) {
            const cl_monomer_block& b = dec->blocks[i];
            const uint64_t slot = (b.monomer % n_templates) * 2 + (b.monomer < n_templates ? 0 : 1);
            ++count[slot];
            bases[slot] += b.end - b.start;
            score[slot] += b.score;
        }
        for (uint64_t slot = 0; slot < T; ++slot) {
            if (!count[slot]) continue;
            tsv += names[s];
            tsv += "\t";
            tsv += template_names[slot / 2];
            snprintf(num, sizeof(num), "\t%c\t%llu\t%llu\t%lld\n", slot % 2 ? '-' : '+', (unsigned long long)count[slot], (unsigned long long)bases[slot], (long long)score[slot]);
            tsv += num;
        }
    }
    return copy_text(tsv, text_out, len_out);
}

}  // extern "C"
