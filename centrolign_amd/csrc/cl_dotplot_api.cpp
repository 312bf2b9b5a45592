// cl_dotplot_api.cpp — windowed k-mer identity maps ("dot plots"; the reference has none): the definition on the host (cl_kmer_dotplot_host),
// the host half of the device path (cl_kmer_dotplot_compute over dotplot_kernels.hip), the identities and the TSV rows.  The identities are
// doubles that a line of Python restates bit for bit: this file is built without fused multiply-adds (Makefile, FPOFF).
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "cl_internal.hpp"

// dotplot_kernels.hip: distinct[n_windows] and the kept entries in (a, b) order of validated input
int cl_dotplot_device(cl_context* ctx, const char* const* seqs, const uint64_t* lens, uint64_t n, const uint64_t* win_off, int k, uint32_t window, int pairs,
                      uint64_t q, uint32_t tile_windows, uint32_t* distinct, std::vector<cl_dotplot_entry>& entries, float* spectra_ms, float* pairs_ms);

namespace {

constexpr uint32_t kMaxWindow = 1u << 20, kMaxTileWindows = 64;
constexpr uint64_t kMaxText = 1ull << 30;

// the limits of the header; win_off is filled on success
int check_arguments(cl_context* ctx, const char* const* seqs, const uint64_t* lens, uint64_t n, const cl_dotplot_params* p, std::vector<uint64_t>& win_off) {
    if (!p || !seqs || !lens) { cl_set_error(ctx, "null argument"); return CL_ERR_INVALID_ARGUMENT; }
    if (n < 1) { cl_set_error(ctx, "n: a dot plot needs at least 1 sequence"); return CL_ERR_INVALID_ARGUMENT; }
    if (p->k < 1 || p->k > 31) { cl_set_error(ctx, "k must lie in 1..31, got %d", p->k); return CL_ERR_INVALID_ARGUMENT; }
    if (p->window < (uint32_t)p->k || p->window > kMaxWindow) {
        cl_set_error(ctx, "window must lie in k..%u, got %u (k = %d)", kMaxWindow, p->window, p->k);
        return CL_ERR_INVALID_ARGUMENT;
    }
    if (p->pairs != 0 && p->pairs != 1) { cl_set_error(ctx, "pairs must be 0 (all) or 1 (self), got %d", p->pairs); return CL_ERR_INVALID_ARGUMENT; }
    if (!(p->min_identity >= 0.0 && p->min_identity <= 100.0)) {   // (a NaN fails both comparisons)
        cl_set_error(ctx, "min_identity must lie in 0..100, got %g", p->min_identity);
        return CL_ERR_INVALID_ARGUMENT;
    }
    if (p->tile_windows > kMaxTileWindows) { cl_set_error(ctx, "tile_windows must lie in 0..%u, got %u", kMaxTileWindows, p->tile_windows); return CL_ERR_INVALID_ARGUMENT; }
    uint64_t text = 0;
    win_off.assign(1, 0);
    for (uint64_t s = 0; s < n; ++s) {
        if (lens[s] && !seqs[s]) { cl_set_error(ctx, "sequences: sequence %llu is null", (unsigned long long)s); return CL_ERR_INVALID_ARGUMENT; }
        if (lens[s] >= kMaxText || (text += lens[s]) >= kMaxText) {
            cl_set_error(ctx, "lengths: the sequences hold 2^30 bases or more (at sequence %llu)", (unsigned long long)s);
            return CL_ERR_INVALID_ARGUMENT;
        }
        win_off.push_back(win_off.back() + (lens[s] + p->window - 1) / p->window);
    }
    if (win_off.back() >= (1ull << 32)) { cl_set_error(ctx, "window: %llu windows, 2^32 or more", (unsigned long long)win_off.back()); return CL_ERR_INVALID_ARGUMENT; }
    return CL_OK;
}

uint64_t threshold_q(double min_identity, int k) { return (uint64_t)std::ceil(std::ldexp(std::pow(min_identity / 100.0, (double)k), 32)); }

int kmer_code(char c) {   // encode_base for ACGTacgt, 4: not a k-mer character
    switch (c) {
    case 'A': case 'a': return 0;
    case 'C': case 'c': return 1;
    case 'G': case 'g': return 2;
    case 'T': case 't': return 3;
    default: return 4;
    }
}

// everything of a cl_dotplot but distinct, the entries and what follows from them
int start_plot(cl_dotplot& d, uint64_t n, const cl_dotplot_params* p, const std::vector<uint64_t>& win_off) {
    memset(&d, 0, sizeof(d));
    d.n_seq = n;
    d.n_windows = win_off.back();
    d.k = p->k;
    d.window = p->window;
    d.threshold_q = threshold_q(p->min_identity, p->k);
    d.win_off = (uint64_t*)malloc((n + 1) * sizeof(uint64_t));
    d.distinct = (uint32_t*)calloc(std::max<uint64_t>(d.n_windows, 1), sizeof(uint32_t));
    if (!d.win_off || !d.distinct) { cl_dotplot_free(&d); return CL_ERR_OUT_OF_MEMORY; }
    memcpy(d.win_off, win_off.data(), (n + 1) * sizeof(uint64_t));
    return CL_OK;
}

int finish_plot(cl_dotplot& d, const std::vector<cl_dotplot_entry>& entries) {
    d.n_entries = entries.size();
    d.entries = (cl_dotplot_entry*)malloc(std::max<size_t>(entries.size(), 1) * sizeof(cl_dotplot_entry));
    d.identity = (double*)malloc(std::max<size_t>(entries.size(), 1) * sizeof(double));
    if (!d.entries || !d.identity) { cl_dotplot_free(&d); return CL_ERR_OUT_OF_MEMORY; }
    if (!entries.empty()) memcpy(d.entries, entries.data(), entries.size() * sizeof(cl_dotplot_entry));
    const double inv_k = 1.0 / (double)d.k;
    for (size_t e = 0; e < entries.size(); ++e) d.identity[e] = 100.0 * std::pow((double)entries[e].shared / (double)entries[e].denom, inv_k);
    return CL_OK;
}

}  // namespace

extern "C" {

void cl_dotplot_params_default(cl_dotplot_params* params) {
    if (!params) return;
    params->k = 21;
    params->window = 2000;
    params->pairs = 0;
    params->min_identity = 86.0;
    params->tile_windows = 0;
}

void cl_dotplot_free(cl_dotplot* out) {
    if (!out) return;
    free(out->win_off);
    free(out->distinct);
    free(out->entries);
    free(out->identity);
    memset(out, 0, sizeof(*out));
}

int cl_kmer_dotplot_host(const char* const* sequences, const uint64_t* lengths, uint64_t n, const cl_dotplot_params* params, cl_dotplot* out) {
    if (out) memset(out, 0, sizeof(*out));
    if (!out) { cl_set_error(nullptr, "null argument"); return CL_ERR_INVALID_ARGUMENT; }
    std::vector<uint64_t> win_off;
    int rc = check_arguments(nullptr, sequences, lengths, n, params, win_off);
    if (rc) return rc;
    cl_dotplot d;
    if ((rc = start_plot(d, n, params, win_off))) return rc;
    const uint32_t k = (uint32_t)params->k, W = params->window;
    const uint64_t G = d.n_windows, mask = (1ull << (2 * k)) - 1ull;
    std::vector<std::vector<uint64_t>> set(G);   // K_g, ascending
    for (uint64_t s = 0; s < n; ++s) {
        uint64_t kmer = 0, run = 0;   // run: characters of ACGTacgt that end at position p
        for (uint64_t p = 0; p < lengths[s]; ++p) {
            const int c = kmer_code(sequences[s][p]);
            run = c > 3 ? 0 : run + 1;
            kmer = ((kmer << 2) | (uint64_t)(c & 3)) & mask;
            if (run >= k) set[win_off[s] + (p + 1 - k) / W].push_back(kmer);
        }
    }
    for (uint64_t g = 0; g < G; ++g) {
        std::sort(set[g].begin(), set[g].end());
        set[g].erase(std::unique(set[g].begin(), set[g].end()), set[g].end());
        d.distinct[g] = (uint32_t)set[g].size();
    }
    std::vector<cl_dotplot_entry> entries;
    std::vector<uint64_t> both;
    for (uint64_t s = 0; s < n; ++s)
        for (uint64_t a = win_off[s]; a < win_off[s + 1]; ++a) {
            if (set[a].empty()) continue;
            const uint64_t b_end = params->pairs == 1 ? win_off[s + 1] : G;
            for (uint64_t b = a; b < b_end; ++b) {
                if (set[b].empty()) continue;
                both.clear();
                std::set_intersection(set[a].begin(), set[a].end(), set[b].begin(), set[b].end(), std::back_inserter(both));
                const uint64_t shared = both.size(), denom = std::min(d.distinct[a], d.distinct[b]);
                if (shared >= 1 && (shared << 32) >= d.threshold_q * denom) entries.push_back({(uint32_t)a, (uint32_t)b, (uint32_t)shared, (uint32_t)denom});
            }
        }
    if ((rc = finish_plot(d, entries))) return rc;
    *out = d;
    return CL_OK;
}

int cl_kmer_dotplot_compute(cl_context* ctx, const char* const* sequences, const uint64_t* lengths, uint64_t n, const cl_dotplot_params* params, cl_dotplot* out) {
    cl_bind_device(ctx);
    if (out) memset(out, 0, sizeof(*out));
    if (!ctx || !out) { cl_set_error(ctx, "null argument"); return CL_ERR_INVALID_ARGUMENT; }
    std::vector<uint64_t> win_off;
    int rc = check_arguments(ctx, sequences, lengths, n, params, win_off);
    if (rc) return rc;
    cl_dotplot d;
    if ((rc = start_plot(d, n, params, win_off))) return rc;
    std::vector<cl_dotplot_entry> entries;
    rc = cl_dotplot_device(ctx, sequences, lengths, n, win_off.data(), params->k, params->window, params->pairs, d.threshold_q, params->tile_windows, d.distinct,
                           entries, &d.spectra_ms, &d.pairs_ms);
    if (rc) { cl_dotplot_free(&d); return rc; }
    if ((rc = finish_plot(d, entries))) return rc;
    *out = d;
    return CL_OK;
}

int cl_dotplot_tsv(const cl_dotplot* plot, const char* const* names, const uint64_t* lengths, char** text_out, uint64_t* len_out) {
    if (text_out) *text_out = nullptr;
    if (len_out) *len_out = 0;
    if (!plot || !names || !lengths || !text_out || !plot->win_off || (plot->n_entries && (!plot->entries || !plot->identity || !plot->distinct))) {
        cl_set_error(nullptr, "null argument");
        return CL_ERR_INVALID_ARGUMENT;
    }
    for (uint64_t s = 0; s < plot->n_seq; ++s)
        if (!names[s]) { cl_set_error(nullptr, "names: sequence %llu has no name", (unsigned long long)s); return CL_ERR_INVALID_ARGUMENT; }
    std::string tsv = "sample1\tstart1\tend1\tsample2\tstart2\tend2\tshared\tdistinct1\tdistinct2\tidentity\n";
    const uint64_t* off = plot->win_off;
    auto seq_of = [&](uint64_t g) { return (uint64_t)(std::upper_bound(off, off + plot->n_seq + 1, g) - off) - 1; };   // the last s with win_off[s] <= g
    char num[160];
    for (uint64_t e = 0; e < plot->n_entries; ++e) {
        const cl_dotplot_entry& x = plot->entries[e];
        if (x.a >= plot->n_windows || x.b >= plot->n_windows) { cl_set_error(nullptr, "entry %llu names a window out of range", (unsigned long long)e); return CL_ERR_INVALID_ARGUMENT; }
        const uint32_t side[2] = {x.a, x.b};
        for (int i = 0; i < 2; ++i) {
            const uint64_t s = seq_of(side[i]), start = (side[i] - off[s]) * plot->window, end = std::min<uint64_t>(start + plot->window, lengths[s]);
            tsv += names[s];
            snprintf(num, sizeof(num), "\t%llu\t%llu\t", (unsigned long long)start, (unsigned long long)end);
            tsv += num;
        }
        snprintf(num, sizeof(num), "%u\t%u\t%u\t%.9g\n", x.shared, plot->distinct[x.a], plot->distinct[x.b], plot->identity[e]);
        tsv += num;
    }
    char* text = (char*)malloc(tsv.size() + 1);
    if (!text) return CL_ERR_OUT_OF_MEMORY;
    memcpy(text, tsv.c_str(), tsv.size() + 1);
    *text_out = text;
    if (len_out) *len_out = tsv.size();
    return CL_OK;
}

}  // extern "C"
