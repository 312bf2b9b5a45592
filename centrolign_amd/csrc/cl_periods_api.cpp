// cl_periods_api.cpp — repeat period spectra (the reference has none): the definition on the host (cl_period_spectrum_host, cl_period_peaks_host),
// the host half of the device path (cl_period_spectrum_compute over periods_kernels.hip) and the two TSV writers.  Integers throughout; the one
// double, share = count / links, exists only in the text.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "cl_internal.hpp"

// periods_kernels.hip: the four counters and the peaks of all R rows of validated input; hist [R * (D + 1)] or NULL (the rows stay on the device)
int cl_periods_device(cl_context* ctx, const char* const* seqs, const uint64_t* lens, uint64_t n, const uint64_t* win_off, const cl_periods_params* p,
                      uint32_t* kmers, uint32_t* links, uint32_t* far, uint32_t* last, cl_period_peak* peaks, uint32_t* hist, float* links_ms, float* hist_ms);

namespace {

constexpr uint32_t kMaxWindow = 1u << 20, kMaxPeriod = 16383, kMaxPeaks = 16, kMaxRadius = 64;
constexpr uint64_t kMaxText = 1ull << 30, kMaxBins = 1ull << 28;

// the limits of the header but those of the sequences
int check_params(cl_context* ctx, const cl_periods_params* p) {
    if (p->k < 1 || p->k > 31) { cl_set_error(ctx, "k must lie in 1..31, got %d", p->k); return CL_ERR_INVALID_ARGUMENT; }
    if (p->window < 1 || p->window > kMaxWindow) { cl_set_error(ctx, "window must lie in 1..%u, got %u", kMaxWindow, p->window); return CL_ERR_INVALID_ARGUMENT; }
    if (p->max_period < 1 || p->max_period > kMaxPeriod) {
        cl_set_error(ctx, "max_period must lie in 1..%u, got %u", kMaxPeriod, p->max_period);
        return CL_ERR_INVALID_ARGUMENT;
    }
    if (p->n_peaks < 1 || p->n_peaks > kMaxPeaks) { cl_set_error(ctx, "n_peaks must lie in 1..%u, got %u", kMaxPeaks, p->n_peaks); return CL_ERR_INVALID_ARGUMENT; }
    if (p->peak_radius < 1 || p->peak_radius > kMaxRadius) {
        cl_set_error(ctx, "peak_radius must lie in 1..%u, got %u", kMaxRadius, p->peak_radius);
        return CL_ERR_INVALID_ARGUMENT;
    }
    if (p->min_period < 1) { cl_set_error(ctx, "min_period must be at least 1, got %u", p->min_period); return CL_ERR_INVALID_ARGUMENT; }
    if (p->min_count < 1) { cl_set_error(ctx, "min_count must be at least 1, got %u", p->min_count); return CL_ERR_INVALID_ARGUMENT; }
    return CL_OK;
}

// every limit of the header; win_off is filled on success
int check_arguments(cl_context* ctx, const char* const* seqs, const uint64_t* lens, uint64_t n, const cl_periods_params* p, std::vector<uint64_t>& win_off) {
    if (!p || !seqs || !lens) { cl_set_error(ctx, "null argument"); return CL_ERR_INVALID_ARGUMENT; }
    if (n < 1) { cl_set_error(ctx, "n: a period spectrum needs at least 1 sequence"); return CL_ERR_INVALID_ARGUMENT; }
    int rc = check_params(ctx, p);
    if (rc) return rc;
    if (n >= kMaxBins) { cl_set_error(ctx, "n: %llu sequences, 2^28 or more", (unsigned long long)n); return CL_ERR_INVALID_ARGUMENT; }
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
    const uint64_t rows = win_off.back() + n;   // (below 2^31)
    if (rows * ((uint64_t)p->max_period + 1) > kMaxBins) {
        cl_set_error(ctx, "window and max_period: %llu rows of %u bins, more than 2^28 bins in all", (unsigned long long)rows, p->max_period + 1);
        return CL_ERR_INVALID_ARGUMENT;
    }
    return CL_OK;
}

int kmer_code(char c) {   // encode_base for ACGTacgt, 4: not a k-mer character
    switch (c) {
    case 'A': case 'a': return 0;
    case 'C': case 'c': return 1;
    case 'G': case 'g': return 2;
    case 'T': case 't': return 3;
    default: return 4;
    }
}

// a zeroed cl_period_spectrum of the right sizes
int start_spectrum(cl_period_spectrum& d, uint64_t n, const cl_periods_params* p, const std::vector<uint64_t>& win_off) {
    memset(&d, 0, sizeof(d));
    d.n_seq = n;
    d.n_windows = win_off.back();
    d.n_rows = d.n_windows + n;
    d.k = p->k;
    d.window = p->window;
    d.max_period = p->max_period;
    d.n_peaks = p->n_peaks;
    d.win_off = (uint64_t*)malloc((n + 1) * sizeof(uint64_t));
    d.kmers = (uint32_t*)calloc(d.n_rows, sizeof(uint32_t));
    d.links = (uint32_t*)calloc(d.n_rows, sizeof(uint32_t));
    d.far = (uint32_t*)calloc(d.n_rows, sizeof(uint32_t));
    d.last = (uint32_t*)calloc(d.n_rows, sizeof(uint32_t));
    d.peaks = (cl_period_peak*)calloc(d.n_rows * d.n_peaks, sizeof(cl_period_peak));
    if (p->want_hist) d.hist = (uint32_t*)calloc(d.n_rows * ((size_t)d.max_period + 1), sizeof(uint32_t));
    if (!d.win_off || !d.kmers || !d.links || !d.far || !d.last || !d.peaks || (p->want_hist && !d.hist)) { cl_period_spectrum_free(&d); return CL_ERR_OUT_OF_MEMORY; }
    memcpy(d.win_off, win_off.data(), (n + 1) * sizeof(uint64_t));
    return CL_OK;
}

void pick_peaks(const uint32_t* h, uint32_t D, const cl_periods_params* p, cl_period_peak* out) {
    const uint32_t r = p->peak_radius;
    std::vector<std::pair<uint32_t, uint32_t>> found;   // (count, period)
    for (uint64_t d = p->min_period; d <= D; ++d) {
        if (h[d] < p->min_count) continue;
        bool peak = true;
        for (uint64_t e = d > r ? d - r : 1; peak && e < d; ++e) peak = h[d] > h[e];
        for (uint64_t e = d + 1; peak && e <= std::min<uint64_t>(d + r, D); ++e) peak = h[d] >= h[e];
        if (peak) found.push_back({h[d], (uint32_t)d});
    }
    std::sort(found.begin(), found.end(), [](const std::pair<uint32_t, uint32_t>& a, const std::pair<uint32_t, uint32_t>& b) {
        return a.first != b.first ? a.first > b.first : a.second < b.second;
    });
    for (uint32_t i = 0; i < p->n_peaks; ++i) out[i] = i < found.size() ? cl_period_peak{found[i].second, found[i].first} : cl_period_peak{0, 0};
}

int copy_text(const std::string& tsv, char** text_out, uint64_t* len_out) {
    char* text = (char*)malloc(tsv.size() + 1);
    if (!text) return CL_ERR_OUT_OF_MEMORY;
    memcpy(text, tsv.c_str(), tsv.size() + 1);
    *text_out = text;
    if (len_out) *len_out = tsv.size();
    return CL_OK;
}

// the rows both writers go through, in their order: row index, start, end
template <class F>
void for_each_row(const cl_period_spectrum* sp, const uint64_t* lengths, int scope, F&& f) {
    for (uint64_t s = 0; s < sp->n_seq; ++s) {
        if (scope != 2) f(s, sp->n_windows + s, (uint64_t)0, lengths[s]);
        if (scope == 1) continue;
        for (uint64_t g = sp->win_off[s]; g < sp->win_off[s + 1]; ++g) {
            const uint64_t start = (g - sp->win_off[s]) * sp->window;
            f(s, g, start, std::min<uint64_t>(start + sp->window, lengths[s]));
        }
    }
}

int check_text_arguments(const cl_period_spectrum* sp, const char* const* names, const uint64_t* lengths, int scope, char** text_out, uint64_t* len_out) {
    if (text_out) *text_out = nullptr;
    if (len_out) *len_out = 0;
    if (!sp || !names || !lengths || !text_out || !sp->win_off || !sp->kmers || !sp->links || !sp->far || !sp->last || !sp->peaks) {
        cl_set_error(nullptr, "null argument");
        return CL_ERR_INVALID_ARGUMENT;
    }
    if (scope < 0 || scope > 2) { cl_set_error(nullptr, "scope must be 0 (both), 1 (sequences) or 2 (windows), got %d", scope); return CL_ERR_INVALID_ARGUMENT; }
    for (uint64_t s = 0; s < sp->n_seq; ++s)
        if (!names[s]) { cl_set_error(nullptr, "names: sequence %llu has no name", (unsigned long long)s); return CL_ERR_INVALID_ARGUMENT; }
    return CL_OK;
}

}  // namespace

extern "C" {

void cl_periods_params_default(cl_periods_params* params) {
    if (!params) return;
    params->k = 8;
    params->window = 10000;
    params->max_period = 8000;
    params->n_peaks = 3;
    params->peak_radius = 1;
    params->min_period = 1;
    params->min_count = 2;
    params->want_hist = 1;
}

void cl_period_spectrum_free(cl_period_spectrum* out) {
    if (!out) return;
    free(out->win_off);
    free(out->kmers);
    free(out->links);
    free(out->far);
    free(out->last);
    free(out->peaks);
    free(out->hist);
    memset(out, 0, sizeof(*out));
}

int cl_period_peaks_host(const uint32_t* row, uint32_t max_period, const cl_periods_params* params, cl_period_peak* out) {
    if (!row || !params || !out) { cl_set_error(nullptr, "null argument"); return CL_ERR_INVALID_ARGUMENT; }
    cl_periods_params p = *params;
    p.max_period = max_period;
    const int rc = check_params(nullptr, &p);
    if (rc) return rc;
    pick_peaks(row, max_period, &p, out);
    return CL_OK;
}

int cl_period_spectrum_host(const char* const* sequences, const uint64_t* lengths, uint64_t n, const cl_periods_params* params, cl_period_spectrum* out) {
    if (out) memset(out, 0, sizeof(*out));
    if (!out) { cl_set_error(nullptr, "null argument"); return CL_ERR_INVALID_ARGUMENT; }
    std::vector<uint64_t> win_off;
    int rc = check_arguments(nullptr, sequences, lengths, n, params, win_off);
    if (rc) return rc;
    cl_periods_params with_rows = *params;   // the definition always forms the rows
    with_rows.want_hist = 1;
    cl_period_spectrum d;
    if ((rc = start_spectrum(d, n, &with_rows, win_off))) return rc;
    const uint32_t k = (uint32_t)params->k, W = params->window, D = params->max_period;
    const uint64_t G = d.n_windows, mask = (1ull << (2 * k)) - 1ull;
    const size_t bins = (size_t)D + 1;
    std::vector<std::pair<uint64_t, uint64_t>> occ;   // (k-mer, position) of one sequence
    for (uint64_t s = 0; s < n; ++s) {
        occ.clear();
        uint64_t kmer = 0, run = 0;   // run: characters of ACGTacgt that end at position p
        for (uint64_t p = 0; p < lengths[s]; ++p) {
            const int c = kmer_code(sequences[s][p]);
            run = c > 3 ? 0 : run + 1;
            kmer = ((kmer << 2) | (uint64_t)(c & 3)) & mask;
            if (run >= k) occ.push_back({kmer, p + 1 - k});
        }
        std::sort(occ.begin(), occ.end());
        for (size_t j = 0; j < occ.size(); ++j) {
            const uint64_t g = win_off[s] + occ[j].second / W;
            ++d.kmers[g];
            if (j + 1 < occ.size() && occ[j + 1].first == occ[j].first) {
                const uint64_t dist = occ[j + 1].second - occ[j].second;
                if (dist <= D) { ++d.hist[g * bins + dist]; ++d.links[g]; }
                else { ++d.hist[g * bins]; ++d.far[g]; }
            } else {
                ++d.last[g];
            }
        }
        const uint64_t t = G + s;   // the sequence's total
        for (uint64_t g = win_off[s]; g < win_off[s + 1]; ++g) {
            for (size_t b = 0; b < bins; ++b) d.hist[t * bins + b] += d.hist[g * bins + b];
            d.kmers[t] += d.kmers[g]; d.links[t] += d.links[g]; d.far[t] += d.far[g]; d.last[t] += d.last[g];
        }
    }
    for (uint64_t r = 0; r < d.n_rows; ++r) pick_peaks(d.hist + r * bins, D, params, d.peaks + r * d.n_peaks);
    if (!params->want_hist) { free(d.hist); d.hist = nullptr; }
    *out = d;
    return CL_OK;
}

int cl_period_spectrum_compute(cl_context* ctx, const char* const* sequences, const uint64_t* lengths, uint64_t n, const cl_periods_params* params,
                               cl_period_spectrum* out) {
    cl_bind_device(ctx);
    if (out) memset(out, 0, sizeof(*out));
    if (!ctx || !out) { cl_set_error(ctx, "null argument"); return CL_ERR_INVALID_ARGUMENT; }
    std::vector<uint64_t> win_off;
    int rc = check_arguments(ctx, sequences, lengths, n, params, win_off);
    if (rc) return rc;
    cl_period_spectrum d;
    if ((rc = start_spectrum(d, n, params, win_off))) return rc;
    rc = cl_periods_device(ctx, sequences, lengths, n, win_off.data(), params, d.kmers, d.links, d.far, d.last, d.peaks, d.hist, &d.links_ms, &d.hist_ms);
    if (rc) { cl_period_spectrum_free(&d); return rc; }
    *out = d;
    return CL_OK;
}

int cl_periods_tsv(const cl_period_spectrum* sp, const char* const* names, const uint64_t* lengths, int scope, char** text_out, uint64_t* len_out) {
    const int rc = check_text_arguments(sp, names, lengths, scope, text_out, len_out);
    if (rc) return rc;
    std::string tsv = "sample\tstart\tend\tkmers\tlinks\tfar\trank\tperiod\tcount\tshare\n";
    char num[200];
    for_each_row(sp, lengths, scope, [&](uint64_t s, uint64_t row, uint64_t start, uint64_t end) {
        snprintf(num, sizeof(num), "\t%llu\t%llu\t%u\t%u\t%u\t", (unsigned long long)start, (unsigned long long)end, sp->kmers[row], sp->links[row], sp->far[row]);
        const std::string lead = names[s] + std::string(num);
        const cl_period_peak* pk = sp->peaks + row * sp->n_peaks;
        if (pk[0].count == 0) tsv += lead + "0\t0\t0\t0\n";
        for (uint32_t i = 0; i < sp->n_peaks && pk[i].count; ++i) {
            snprintf(num, sizeof(num), "%u\t%u\t%u\t%.9g\n", i + 1, pk[i].period, pk[i].count, (double)pk[i].count / (double)sp->links[row]);
            tsv += lead + num;
        }
    });
    return copy_text(tsv, text_out, len_out);
}

int cl_periods_hist_tsv(const cl_period_spectrum* sp, const char* const* names, const uint64_t* lengths, int scope, char** text_out, uint64_t* len_out) {
    const int rc = check_text_arguments(sp, names, lengths, scope, text_out, len_out);
    if (rc) return rc;
    if (!sp->hist) { cl_set_error(nullptr, "hist: the spectrum was computed with want_hist = 0"); return CL_ERR_INVALID_ARGUMENT; }
    std::string tsv = "sample\tstart\tend\tperiod\tcount\n";
    char num[200];
    const size_t bins = (size_t)sp->max_period + 1;
    for_each_row(sp, lengths, scope, [&](uint64_t s, uint64_t row, uint64_t start, uint64_t end) {
        snprintf(num, sizeof(num), "\t%llu\t%llu\t", (unsigned long long)start, (unsigned long long)end);
        const std::string lead = names[s] + std::string(num);
        for (size_t b = 1; b < bins; ++b) {
            const uint32_t c = sp->hist[row * bins + b];
            if (!c) continue;
            snprintf(num, sizeof(num), "%zu\t%u\n", b, c);
            tsv += lead + num;
        }
    });
    return copy_text(tsv, text_out, len_out);
}

}  // extern "C"
