// cl_strands_api.cpp — strand profiles (the reference has none; its README names inversions as the first limitation): the definition on the host
// (cl_strand_profile_host), the host half of the device path (cl_strand_profile_compute over strands_kernels.hip), the intervals read from a
// profile, the input with them turned back, and the two TSV writers.  Integers throughout.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "cl_internal.hpp"

// strands_kernels.hip: the three window counters, the votes (NULL: they stay on the device) and the distinct canonical k-mers of validated input
int cl_strands_device(cl_context* ctx, const char* const* seqs, const uint64_t* lens, uint64_t n, const uint64_t* win_off, const uint64_t* base_off,
                      const cl_strands_params* p, uint32_t* kmers, uint32_t* forward, uint32_t* reverse, uint8_t* votes, uint64_t* distinct, float* sort_ms,
                      float* vote_ms);

namespace {

constexpr uint32_t kMaxWindow = 1u << 20;
constexpr uint64_t kMaxText = 1ull << 30, kMaxSeqs = 1ull << 28;
enum : uint8_t { NO_KMER = 0, FORWARD = 1, REVERSE = 2, NEUTRAL = 3 };

// every limit of the header; the two offset arrays are filled on success
int check_arguments(cl_context* ctx, const char* const* seqs, const uint64_t* lens, uint64_t n, const cl_strands_params* p, std::vector<uint64_t>& win_off,
                    std::vector<uint64_t>& base_off) {
    if (!p || (n && (!seqs || !lens))) { cl_set_error(ctx, "null argument"); return CL_ERR_INVALID_ARGUMENT; }
    if (p->k < 1 || p->k > 31) { cl_set_error(ctx, "k must lie in 1..31, got %d", p->k); return CL_ERR_INVALID_ARGUMENT; }
    if (p->window < 1 || p->window > kMaxWindow) { cl_set_error(ctx, "window must lie in 1..%u, got %u", kMaxWindow, p->window); return CL_ERR_INVALID_ARGUMENT; }
    if (n >= kMaxSeqs) { cl_set_error(ctx, "n: %llu sequences, 2^28 or more", (unsigned long long)n); return CL_ERR_INVALID_ARGUMENT; }
    win_off.assign(1, 0);
    base_off.assign(1, 0);
    for (uint64_t s = 0; s < n; ++s) {
        if (lens[s] && !seqs[s]) { cl_set_error(ctx, "sequences: sequence %llu is null", (unsigned long long)s); return CL_ERR_INVALID_ARGUMENT; }
        if (lens[s] >= kMaxText || base_off.back() + lens[s] >= kMaxText) {
            cl_set_error(ctx, "lengths: the sequences hold 2^30 bases or more (at sequence %llu)", (unsigned long long)s);
            return CL_ERR_INVALID_ARGUMENT;
        }
        base_off.push_back(base_off.back() + lens[s]);
        win_off.push_back(win_off.back() + (lens[s] + p->window - 1) / p->window);
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

char complement(char c) {
    switch (c) {
    case 'A': return 'T'; case 'C': return 'G'; case 'G': return 'C'; case 'T': return 'A';
    case 'a': return 't'; case 'c': return 'g'; case 'g': return 'c'; case 't': return 'a';
    default: return c;
    }
}

// a zeroed cl_strand_profile of the right sizes
int start_profile(cl_strand_profile& d, uint64_t n, const cl_strands_params* p, const std::vector<uint64_t>& win_off, const std::vector<uint64_t>& base_off) {
    memset(&d, 0, sizeof(d));
    d.n_seq = n;
    d.n_windows = win_off.back();
    d.n_bases = base_off.back();
    d.k = p->k;
    d.window = p->window;
    d.win_off = (uint64_t*)malloc((n + 1) * sizeof(uint64_t));
    d.base_off = (uint64_t*)malloc((n + 1) * sizeof(uint64_t));
    d.kmers = (uint32_t*)calloc(std::max<uint64_t>(d.n_windows, 1), sizeof(uint32_t));
    d.forward = (uint32_t*)calloc(std::max<uint64_t>(d.n_windows, 1), sizeof(uint32_t));
    d.reverse = (uint32_t*)calloc(std::max<uint64_t>(d.n_windows, 1), sizeof(uint32_t));
    if (p->want_votes) d.votes = (uint8_t*)calloc(std::max<uint64_t>(d.n_bases, 1), 1);
    if (!d.win_off || !d.base_off || !d.kmers || !d.forward || !d.reverse || (p->want_votes && !d.votes)) { cl_strand_profile_free(&d); return CL_ERR_OUT_OF_MEMORY; }
    memcpy(d.win_off, win_off.data(), (n + 1) * sizeof(uint64_t));
    memcpy(d.base_off, base_off.data(), (n + 1) * sizeof(uint64_t));
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

bool complete(const cl_strand_profile* pr) {
    return pr && pr->win_off && pr->base_off && pr->kmers && pr->forward && pr->reverse && pr->window >= 1 && pr->window <= kMaxWindow;
}

// the calls of the windows [g0, g1) of one sequence after the inheritance rule: 1 = reverse
std::vector<uint8_t> window_calls(const cl_strand_profile* pr, uint64_t g0, uint64_t g1) {
    const uint64_t nw = g1 - g0;
    std::vector<uint8_t> call(nw, 0);
    int left = -1;   // the call of the nearest decided window to the left, -1: none yet
    for (uint64_t w = 0; w < nw; ++w) {
        const uint32_t f = pr->forward[g0 + w], r = pr->reverse[g0 + w];
        if (f != r) {
            left = r > f ? 1 : 0;
            for (uint64_t u = w; u-- > 0 && call[u] == 2;) call[u] = (uint8_t)left;   // the undecided windows in front of the first decided one
        }
        call[w] = left < 0 ? 2 : (uint8_t)left;
    }
    for (uint8_t& c : call) if (c == 2) c = 0;   // no decided window at all
    return call;
}

}  // namespace

extern "C" {

void cl_strands_params_default(cl_strands_params* params) {
    if (!params) return;
    params->k = 21;
    params->window = 1000;
    params->want_votes = 1;
}

void cl_strand_profile_free(cl_strand_profile* out) {
    if (!out) return;
    free(out->win_off);
    free(out->base_off);
    free(out->kmers);
    free(out->forward);
    free(out->reverse);
    free(out->votes);
    memset(out, 0, sizeof(*out));
}

void cl_strand_intervals_free(cl_strand_interval* intervals) { free(intervals); }

int cl_strand_profile_host(const char* const* sequences, const uint64_t* lengths, uint64_t n, const cl_strands_params* params, cl_strand_profile* out) {
    if (out) memset(out, 0, sizeof(*out));
    if (!out) { cl_set_error(nullptr, "null argument"); return CL_ERR_INVALID_ARGUMENT; }
    std::vector<uint64_t> win_off, base_off;
    int rc = check_arguments(nullptr, sequences, lengths, n, params, win_off, base_off);
    if (rc) return rc;
    cl_strands_params with_votes = *params;   // the definition always forms the votes
    with_votes.want_votes = 1;
    cl_strand_profile d;
    if ((rc = start_profile(d, n, &with_votes, win_off, base_off))) return rc;
    const uint32_t k = (uint32_t)params->k, W = params->window;
    const uint64_t mask = (1ull << (2 * k)) - 1ull;
    struct Occ { uint64_t kmer, rc, at; };
    std::vector<Occ> occ;            // every position with a k-mer: x, rc(x), global position
    std::vector<uint64_t> sorted;    // every x, ascending: count(x) is the length of its range
    for (uint64_t s = 0; s < n; ++s) {
        uint64_t kmer = 0, rev = 0, run = 0;   // run: characters of ACGTacgt that end at position p
        for (uint64_t p = 0; p < lengths[s]; ++p) {
            const int c = kmer_code(sequences[s][p]);
            run = c > 3 ? 0 : run + 1;
            kmer = ((kmer << 2) | (uint64_t)(c & 3)) & mask;
            rev = (rev >> 2) | ((uint64_t)(3 - (c & 3)) << (2 * (k - 1)));
            if (run >= k) occ.push_back({kmer, rev, base_off[s] + p + 1 - k});
        }
    }
    sorted.reserve(occ.size());
    for (const Occ& o : occ) sorted.push_back(o.kmer);
    std::sort(sorted.begin(), sorted.end());
    auto count = [&](uint64_t x) {
        const auto range = std::equal_range(sorted.begin(), sorted.end(), x);
        return (uint64_t)(range.second - range.first);
    };
    uint64_t s = 0;
    for (const Occ& o : occ) {
        while (o.at >= base_off[s + 1]) ++s;
        const uint64_t a = count(o.kmer), b = count(o.rc);
        const uint8_t vote = a + b < 2 || a == b ? NEUTRAL : a > b ? FORWARD : REVERSE;
        const uint64_t g = win_off[s] + (o.at - base_off[s]) / W;
        d.votes[o.at] = vote;
        ++d.kmers[g];
        if (vote == FORWARD) ++d.forward[g];
        if (vote == REVERSE) ++d.reverse[g];
    }
    for (size_t j = 0; j < occ.size(); ++j) sorted[j] = std::min(occ[j].kmer, occ[j].rc);   // the canonical k-mers
    std::sort(sorted.begin(), sorted.end());
    d.distinct = (uint64_t)(std::unique(sorted.begin(), sorted.end()) - sorted.begin());
    if (!params->want_votes) { free(d.votes); d.votes = nullptr; }
    *out = d;
    return CL_OK;
}

int cl_strand_profile_compute(cl_context* ctx, const char* const* sequences, const uint64_t* lengths, uint64_t n, const cl_strands_params* params,
                              cl_strand_profile* out) {
    cl_bind_device(ctx);
    if (out) memset(out, 0, sizeof(*out));
    if (!ctx || !out) { cl_set_error(ctx, "null argument"); return CL_ERR_INVALID_ARGUMENT; }
    std::vector<uint64_t> win_off, base_off;
    int rc = check_arguments(ctx, sequences, lengths, n, params, win_off, base_off);
    if (rc) return rc;
    cl_strand_profile d;
    if ((rc = start_profile(d, n, params, win_off, base_off))) return rc;
    rc = cl_strands_device(ctx, sequences, lengths, n, win_off.data(), base_off.data(), params, d.kmers, d.forward, d.reverse, d.votes, &d.distinct, &d.sort_ms,
                           &d.vote_ms);
    if (rc) { cl_strand_profile_free(&d); return rc; }
    *out = d;
    return CL_OK;
}

int cl_strand_intervals(const cl_strand_profile* pr, uint32_t min_run, cl_strand_interval** intervals_out, uint64_t* n_out) {
    if (intervals_out) *intervals_out = nullptr;
    if (n_out) *n_out = 0;
    if (!complete(pr) || !intervals_out || !n_out) { cl_set_error(nullptr, "null argument"); return CL_ERR_INVALID_ARGUMENT; }
    if (min_run < 1) { cl_set_error(nullptr, "min_run must be at least 1, got %u", min_run); return CL_ERR_INVALID_ARGUMENT; }
    if (pr->n_seq >= kMaxSeqs || pr->base_off[pr->n_seq] >= kMaxText) { cl_set_error(nullptr, "profile: more sequences or bases than a profile holds"); return CL_ERR_INVALID_ARGUMENT; }
    const uint64_t W = pr->window;
    std::vector<cl_strand_interval> found;
    std::vector<int64_t> prefix;   // prefix[i] = v(lo) + ... + v(lo + i - 1) of the stretch a boundary is searched in
    // the largest c in [lo, hi] that maximises sign * (sum of v over [lo, c) - sum of v over [c, hi)) = sign * (2 prefix(c) - total)
    auto boundary = [&](const uint8_t* votes, uint64_t lo, uint64_t hi, int sign) {
        prefix.assign(hi - lo + 1, 0);
        for (uint64_t p = lo; p < hi; ++p) prefix[p - lo + 1] = prefix[p - lo] + (votes[p] == FORWARD ? 1 : votes[p] == REVERSE ? -1 : 0);
        uint64_t best = lo;
        for (uint64_t c = lo; c <= hi; ++c)
            if (sign * prefix[c - lo] >= sign * prefix[best - lo]) best = c;
        return best;
    };
    for (uint64_t s = 0; s < pr->n_seq; ++s) {
        const uint64_t g0 = pr->win_off[s], nw = pr->win_off[s + 1] - g0, len = pr->base_off[s + 1] - pr->base_off[s];
        if (nw != (len + W - 1) / W) { cl_set_error(nullptr, "profile: sequence %llu has %llu windows for %llu bases", (unsigned long long)s, (unsigned long long)nw, (unsigned long long)len); return CL_ERR_INVALID_ARGUMENT; }
        const std::vector<uint8_t> call = window_calls(pr, g0, g0 + nw);
        const uint8_t* votes = pr->votes ? pr->votes + pr->base_off[s] : nullptr;
        uint64_t prev = 0;
        for (uint64_t wa = 0; wa < nw;) {
            if (!call[wa]) { ++wa; continue; }
            uint64_t wb = wa;
            while (wb < nw && call[wb]) ++wb;
            if (wb - wa >= min_run) {
                cl_strand_interval iv;
                memset(&iv, 0, sizeof(iv));
                uint64_t start = wa * W, end = std::min(len, wb * W);
                if (votes) {
                    if (wa > 0) start = boundary(votes, std::max(prev, (wa - 1) * W), std::min(len, (wa + 1) * W), +1);
                    if (wb < nw) end = boundary(votes, std::max(start, (wb - 1) * W), std::min(len, (wb + 1) * W), -1);
                    if (wa > 0 || wb < nw) iv.flags |= 2u;
                    for (uint64_t p = start; p < end; ++p) { iv.forward += votes[p] == FORWARD; iv.reverse += votes[p] == REVERSE; }
                } else {
                    for (uint64_t w = wa; w < wb; ++w) { iv.forward += pr->forward[g0 + w]; iv.reverse += pr->reverse[g0 + w]; }
                }
                if (start == 0 && end == len) iv.flags |= 1u;
                iv.sequence = (uint32_t)s;
                iv.start = (uint32_t)start;
                iv.end = (uint32_t)end;
                iv.windows = (uint32_t)(wb - wa);
                found.push_back(iv);
                prev = end;
            }
            wa = wb;
        }
    }
    cl_strand_interval* list = (cl_strand_interval*)malloc(std::max<size_t>(found.size(), 1) * sizeof(cl_strand_interval));
    if (!list) return CL_ERR_OUT_OF_MEMORY;
    if (!found.empty()) memcpy(list, found.data(), found.size() * sizeof(cl_strand_interval));
    *intervals_out = list;
    *n_out = found.size();
    return CL_OK;
}

int cl_strand_apply(const char* sequence, uint64_t length, uint64_t sequence_index, const cl_strand_interval* intervals, uint64_t n_intervals, char* out) {
    if ((length && (!sequence || !out)) || (n_intervals && !intervals)) { cl_set_error(nullptr, "null argument"); return CL_ERR_INVALID_ARGUMENT; }
    uint64_t prev = 0;
    for (uint64_t i = 0; i < n_intervals; ++i) {
        const cl_strand_interval& iv = intervals[i];
        if (iv.sequence != sequence_index) continue;
        if (iv.start > iv.end || iv.end > length) {
            cl_set_error(nullptr, "intervals: interval %llu, [%u, %u), does not fit its sequence of %llu bases", (unsigned long long)i, iv.start, iv.end, (unsigned long long)length);
            return CL_ERR_INVALID_ARGUMENT;
        }
        if (iv.start < prev) {
            cl_set_error(nullptr, "intervals: interval %llu, [%u, %u), overlaps the one before it or is out of order", (unsigned long long)i, iv.start, iv.end);
            return CL_ERR_INVALID_ARGUMENT;
        }
        prev = iv.end;
    }
    if (out != sequence && length) memmove(out, sequence, length);
    for (uint64_t i = 0; i < n_intervals; ++i) {
        if (intervals[i].sequence != sequence_index) continue;
        for (uint64_t a = intervals[i].start, b = intervals[i].end; a < b; ++a) {
            --b;
            const char left = complement(out[a]);   // (a == b: the middle base is complemented once)
            out[a] = complement(out[b]);
            out[b] = left;
        }
    }
    return CL_OK;
}

int cl_strand_profile_tsv(const cl_strand_profile* pr, const char* const* names, char** text_out, uint64_t* len_out) {
    if (text_out) *text_out = nullptr;
    if (len_out) *len_out = 0;
    if (!complete(pr) || !text_out || (pr->n_seq && !names)) { cl_set_error(nullptr, "null argument"); return CL_ERR_INVALID_ARGUMENT; }
    for (uint64_t s = 0; s < pr->n_seq; ++s)
        if (!names[s]) { cl_set_error(nullptr, "names: sequence %llu has no name", (unsigned long long)s); return CL_ERR_INVALID_ARGUMENT; }
    std::string tsv = "sample\tstart\tend\tkmers\tforward\treverse\tneutral\tcall\n";
    char num[200];
    for (uint64_t s = 0; s < pr->n_seq; ++s) {
        const uint64_t g0 = pr->win_off[s], g1 = pr->win_off[s + 1], len = pr->base_off[s + 1] - pr->base_off[s];
        const std::vector<uint8_t> call = window_calls(pr, g0, g1);
        for (uint64_t g = g0; g < g1; ++g) {
            const uint64_t start = (g - g0) * pr->window;
            snprintf(num, sizeof(num), "\t%llu\t%llu\t%u\t%u\t%u\t%u\t%c\n", (unsigned long long)start, (unsigned long long)std::min<uint64_t>(start + pr->window, len),
                     pr->kmers[g], pr->forward[g], pr->reverse[g], pr->kmers[g] - pr->forward[g] - pr->reverse[g], call[g - g0] ? '-' : '+');
            tsv += names[s];
            tsv += num;
        }
    }
    return copy_text(tsv, text_out, len_out);
}

int cl_strand_intervals_tsv(const cl_strand_interval* intervals, uint64_t n_intervals, const char* const* names, uint64_t n_names, char** text_out,
                            uint64_t* len_out) {
    if (text_out) *text_out = nullptr;
    if (len_out) *len_out = 0;
    if (!text_out || (n_intervals && !intervals) || (n_names && !names)) { cl_set_error(nullptr, "null argument"); return CL_ERR_INVALID_ARGUMENT; }
    for (uint64_t i = 0; i < n_intervals; ++i) {
        if (intervals[i].sequence >= n_names || !names[intervals[i].sequence]) {
            cl_set_error(nullptr, "names: interval %llu lies in sequence %u, which has no name", (unsigned long long)i, intervals[i].sequence);
            return CL_ERR_INVALID_ARGUMENT;
        }
        if (intervals[i].start > intervals[i].end) { cl_set_error(nullptr, "intervals: interval %llu ends before it starts", (unsigned long long)i); return CL_ERR_INVALID_ARGUMENT; }
    }
    std::string tsv = "sample\tstart\tend\tlength\twindows\tforward\treverse\twhole\n";
    char num[200];
    for (uint64_t i = 0; i < n_intervals; ++i) {
        const cl_strand_interval& iv = intervals[i];
        snprintf(num, sizeof(num), "\t%u\t%u\t%u\t%u\t%u\t%u\t%u\n", iv.start, iv.end, iv.end - iv.start, iv.windows, iv.forward, iv.reverse, iv.flags & 1u);
        tsv += names[iv.sequence];
        tsv += num;
    }
    return copy_text(tsv, text_out, len_out);
}

}  // extern "C"
