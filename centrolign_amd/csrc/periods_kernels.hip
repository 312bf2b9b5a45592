// periods_kernels.hip — the device half of cl_period_spectrum_compute (cl_periods_api.cpp): for every window of every sequence the
// histogram of the distances between neighbouring occurrences of a k-mer, the per-sequence totals and the peaks of every row.
//
//   links   one key per text position (the 2k-bit forward-strand k-mer, a flag for the runs that are k-mers), a scan + compaction of the flagged
//           positions with the global position as value, a stable radix sort by k-mer (cl_radix.h): positions ascend inside a k-mer and a
//           sequence's positions are contiguous, so an occurrence's successor is the next sorted element iff its key is equal and it lies in the
//           same sequence.  period_link_kernel emits (window, value) per occurrence, value = d for a link, 0 for "far", kLast for "last"; a
//           second stable sort by window alone and a binary search per window give every window one contiguous segment of values.
//   hist    period_hist_kernel, one workgroup per window in a persistent loop with the row of D + 1 words in LDS: the segment is read coalesced
//           and counted with LDS adds, the row goes to global memory coalesced, links and last come from a workgroup reduction.  No global
//           atomics.  period_total_kernel sums a sequence's window rows (and counters) by column into row G + s.  period_peaks_kernel, one
//           workgroup per row: the row in LDS, the candidate flags of the +-r rule as one bit per bin in a register, then n_peaks rounds of a
//           workgroup arg-max on (count << 32 | ~period).
// No floating point on the device.  LDS per workgroup: the row, (D + 1) * 4 bytes, at most 64 KiB.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "cl_internal.hpp"
#include "cl_radix.h"
#include "kmer_code.h"

namespace {

constexpr uint32_t kBlock = 256;
constexpr uint32_t kRowBlock = 512, kRowWaves = kRowBlock / 64;   // the two row kernels: 32 bins a thread cover the largest row (16 384 bins)
constexpr uint32_t kMaxGrid = 2048;                               // workgroups of the persistent histogram loop
constexpr uint32_t kLast = 0xFFFFFFFFu;                           // the value of an occurrence without a successor
static_assert(kRowBlock * 32 >= 16384, "period_peaks_kernel keeps one candidate bit per bin in a 32-bit register");

// position p of the text: its k-mer, and whether [p, p + k) lies in one sequence and holds only ACGTacgt
__global__ void __launch_bounds__(kBlock) period_keys_kernel(const uint8_t* __restrict__ text, uint32_t n_text, const uint64_t* __restrict__ seq_start, uint32_t n_seq,
                                                             uint32_t k, uint64_t* __restrict__ key, uint32_t* __restrict__ flag) {
    const uint32_t p = blockIdx.x * kBlock + threadIdx.x;
    if (p >= n_text) return;
    uint32_t lo = 0, hi = n_seq;   // the sequence of p: largest s with seq_start[s] <= p (an empty sequence shares its start with the next one)
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) / 2;
        if (seq_start[mid] <= p) lo = mid; else hi = mid;
    }
    uint64_t kmer = 0;
    uint32_t ok = (uint64_t)p + k <= seq_start[lo + 1] ? 1u : 0u;
    for (uint32_t j = 0; ok && j < k; ++j) {
        const uint32_t c = base_code(text[p + j]);
        if (c > 3) ok = 0u;
        kmer = (kmer << 2) | c;
    }
    key[p] = ok ? kmer : 0ull;
    flag[p] = ok;
}

// the flagged (key, position) pairs, in text order, to the front (pos = inclusive scan of the flags)
__global__ void __launch_bounds__(kBlock) period_compact_kernel(const uint64_t* __restrict__ key, const uint32_t* __restrict__ flag, const uint32_t* __restrict__ pos,
                                                                uint32_t n_text, uint64_t* __restrict__ key_out, uint32_t* __restrict__ at_out) {
    const uint32_t p = blockIdx.x * kBlock + threadIdx.x;
    if (p >= n_text || !flag[p]) return;
    key_out[pos[p] - 1] = key[p];
    at_out[pos[p] - 1] = p;
}

// sorted by k-mer, positions ascending inside one: occurrence j's window and its value (d, 0: far, kLast: no successor in its sequence)
__global__ void __launch_bounds__(kBlock) period_link_kernel(const uint64_t* __restrict__ key, const uint32_t* __restrict__ at, uint32_t m,
                                                             const uint64_t* __restrict__ seq_start, const uint64_t* __restrict__ win_off, uint32_t n_seq, uint32_t window,
                                                             uint32_t max_period, uint32_t* __restrict__ win, uint32_t* __restrict__ value) {
    const uint32_t j = blockIdx.x * kBlock + threadIdx.x;
    if (j >= m) return;
    const uint32_t p = at[j];
    uint32_t lo = 0, hi = n_seq;   // the sequence of p, as above
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) / 2;
        if (seq_start[mid] <= p) lo = mid; else hi = mid;
    }
    uint32_t v = kLast;
    if (j + 1 < m && key[j + 1] == key[j]) {
        const uint32_t next = at[j + 1];
        if (next < seq_start[lo + 1]) v = next - p <= max_period ? next - p : 0u;
    }
    win[j] = (uint32_t)(win_off[lo] + (p - seq_start[lo]) / window);
    value[j] = v;
}

// g = 0 .. n_windows: seg_off[g] = the first sorted element of a window >= g
__global__ void __launch_bounds__(kBlock) period_offsets_kernel(const uint32_t* __restrict__ win, uint32_t m, uint32_t n_windows, uint32_t* __restrict__ seg_off) {
    const uint32_t g = blockIdx.x * kBlock + threadIdx.x;
    if (g > n_windows) return;
    uint32_t lo = 0, hi = m;
    if (g < n_windows) {
        while (lo < hi) {
            const uint32_t mid = lo + (hi - lo) / 2;
            if (win[mid] < g) lo = mid + 1; else hi = mid;
        }
    } else {
        lo = m;
    }
    seg_off[g] = lo;
}

__device__ __forceinline__ uint32_t wave_sum(uint32_t x) {
    for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o);
    return x;
}

// Windows g = blockIdx.x, + gridDim.x, ...: hist[g][0 .. D] from the values of segment g, counters[0 .. 3][g] = kmers, links, far, last.
// s_row holds max(D + 1, 2 * kRowWaves) words: the row, then (the row is in global memory by then) the partial sums of the reduction.
// Plain LDS adds: a wave-level peel in front of them (ballot the lanes that hold the first pending lane's value, add their number once) was
// measured and lost on the arrays this is for; it won 0.02 ms only where every link falls in one bin.
__global__ void __launch_bounds__(kRowBlock) period_hist_kernel(const uint32_t* __restrict__ value, const uint32_t* __restrict__ seg_off, uint32_t n_windows,
                                                                uint32_t max_period, uint32_t n_rows, uint32_t* __restrict__ hist, uint32_t* __restrict__ counters) {
    extern __shared__ uint32_t s_row[];
    const uint32_t tid = threadIdx.x, wave = tid >> 6, lane = tid & 63u, bins = max_period + 1;
    for (uint32_t g = blockIdx.x; g < n_windows; g += gridDim.x) {
        const uint32_t begin = seg_off[g], end = seg_off[g + 1];
        for (uint32_t b = tid; b < bins; b += kRowBlock) s_row[b] = 0;
        __syncthreads();
        uint32_t last = 0;
        for (uint32_t i0 = begin; i0 < end; i0 += kRowBlock) {   // (end < 2^30: no wrap)
            const uint32_t i = i0 + tid;
            const uint32_t v = i < end ? value[i] : kLast;
            last += (i < end && v == kLast) ? 1u : 0u;
            if (v != kLast) atomicAdd(&s_row[v], 1u);   // v <= max_period
        }
        __syncthreads();
        const uint32_t far = s_row[0];
        uint32_t links = 0;
        uint32_t* const row = hist + (size_t)g * bins;
        for (uint32_t b = tid; b < bins; b += kRowBlock) {
            const uint32_t c = s_row[b];
            row[b] = c;
            links += b ? c : 0u;
        }
        __syncthreads();   // (the row has been read: its first words now hold the partial sums)
        links = wave_sum(links);
        last = wave_sum(last);
        if (lane == 0) { s_row[wave] = links; s_row[kRowWaves + wave] = last; }
        __syncthreads();
        if (tid == 0) {
            uint32_t sum_links = 0, sum_last = 0;
            for (uint32_t w = 0; w < kRowWaves; ++w) { sum_links += s_row[w]; sum_last += s_row[kRowWaves + w]; }
            counters[g] = end - begin;
            counters[n_rows + g] = sum_links;
            counters[2 * (size_t)n_rows + g] = far;
            counters[3 * (size_t)n_rows + g] = sum_last;
        }
        __syncthreads();   // (s_row is zeroed for the next window)
    }
}

// element t = s * bins + b: row G + s, bin b = the sum of bin b over the windows of s; the thread of bin 0 sums the four counters as well
__global__ void __launch_bounds__(kBlock) period_total_kernel(const uint64_t* __restrict__ win_off, uint32_t n_seq, uint32_t n_windows, uint32_t max_period,
                                                              uint32_t n_rows, uint32_t* __restrict__ hist, uint32_t* __restrict__ counters) {
    const uint32_t bins = max_period + 1;
    const uint64_t t = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (t >= (uint64_t)n_seq * bins) return;
    const uint32_t s = (uint32_t)(t / bins), b = (uint32_t)(t % bins);
    const uint32_t g0 = (uint32_t)win_off[s], g1 = (uint32_t)win_off[s + 1];
    uint32_t sum = 0;
    for (uint32_t g = g0; g < g1; ++g) sum += hist[(size_t)g * bins + b];
    hist[(size_t)(n_windows + s) * bins + b] = sum;
    if (b == 0)
        for (uint32_t c = 0; c < 4; ++c) {
            uint32_t total = 0;
            for (uint32_t g = g0; g < g1; ++g) total += counters[c * (size_t)n_rows + g];
            counters[c * (size_t)n_rows + n_windows + s] = total;
        }
}

__device__ __forceinline__ unsigned long long wave_max(unsigned long long x) {
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long y = __shfl_xor(x, o);
        x = y > x ? y : x;
    }
    return x;
}

// Row blockIdx.x: peaks[row][0 .. n_peaks) by the rule of cl_period_peaks_host.  s_row holds the row's D + 1 words; word 0 (bin 0, "far", no
// period) is where the waves meet in the arg-max: a round takes the largest key (count << 32 | ~period) below the one taken before, first the
// count by an LDS maximum, then the smallest period of that count by an LDS minimum.
__global__ void __launch_bounds__(kRowBlock) period_peaks_kernel(const uint32_t* __restrict__ hist, uint32_t max_period, uint32_t n_peaks, uint32_t radius,
                                                                 uint32_t min_period, uint32_t min_count, uint2* __restrict__ peaks) {
    extern __shared__ uint32_t s_row[];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, bins = max_period + 1;
    const uint32_t* const row = hist + (size_t)blockIdx.x * bins;
    for (uint32_t b = tid; b < bins; b += kRowBlock) s_row[b] = row[b];
    __syncthreads();
    uint32_t candidates = 0;   // bit i: bin tid + i * kRowBlock is a peak
    for (uint32_t i = 0, d = tid; d <= max_period; ++i, d += kRowBlock) {
        if (d < min_period) continue;   // (min_period >= 1: bin 0 is never one)
        const uint32_t c = s_row[d];
        bool peak = c >= min_count;
        const uint32_t left = d > radius ? d - radius : 1u, right = min(d + radius, max_period);
        for (uint32_t e = left; peak && e < d; ++e) peak = c > s_row[e];
        for (uint32_t e = d + 1; peak && e <= right; ++e) peak = c >= s_row[e];
        if (peak) candidates |= 1u << i;
    }
    unsigned long long bound = ~0ull;   // the key taken in the round before (no key has this value: periods are at least 1)
    for (uint32_t round = 0; round < n_peaks; ++round) {
        unsigned long long best = 0;   // (no candidate has count 0)
        for (uint32_t rest = candidates; rest; rest &= rest - 1u) {
            const uint32_t d = tid + (uint32_t)(__ffs((int)rest) - 1) * kRowBlock;
            const unsigned long long key = ((unsigned long long)s_row[d] << 32) | (uint32_t)~d;
            if (key < bound && key > best) best = key;
        }
        best = wave_max(best);
        __syncthreads();   // (the candidate loops above, or the round before, have read word 0's neighbours and word 0)
        if (tid == 0) s_row[0] = 0;
        __syncthreads();
        if (lane == 0 && best) atomicMax(&s_row[0], (uint32_t)(best >> 32));
        __syncthreads();
        const uint32_t count = s_row[0];
        __syncthreads();
        if (tid == 0) s_row[0] = 0xFFFFFFFFu;
        __syncthreads();
        if (lane == 0 && count && (uint32_t)(best >> 32) == count) atomicMin(&s_row[0], ~(uint32_t)best);
        __syncthreads();
        const uint32_t period = count ? s_row[0] : 0u;
        if (tid == 0) peaks[(size_t)blockIdx.x * n_peaks + round] = make_uint2(period, count);
        bound = count ? ((unsigned long long)count << 32) | (uint32_t)~period : 0ull;   // count 0: nothing is left, the remaining slots are {0, 0}
    }
}

}  // namespace

int cl_periods_device(cl_context* ctx, const char* const* seqs, const uint64_t* lens, uint64_t n, const uint64_t* win_off, const cl_periods_params* p,
                      uint32_t* kmers, uint32_t* links, uint32_t* far, uint32_t* last, cl_period_peak* peaks, uint32_t* hist, float* links_ms, float* hist_ms) {
    static_assert(sizeof(cl_period_peak) == sizeof(uint2), "a peak is written as one 8-byte store");
    hipStream_t s = ctx->stream;
    int rc;
    const uint32_t G = (uint32_t)win_off[n], R = G + (uint32_t)n, D = p->max_period, bins = D + 1;   // R * bins <= 2^28 (checked by the caller)
    std::vector<uint64_t> h_start(n + 1, 0);
    for (uint64_t i = 0; i < n; ++i) h_start[i + 1] = h_start[i] + lens[i];
    const uint32_t n_text = (uint32_t)h_start[n];   // < 2^30 (checked by the caller)
    hipEvent_t ev[3];
    for (auto& e : ev) HIP_TRY(ctx, hipEventCreate(&e));
    struct Events { hipEvent_t* e; ~Events() { for (int i = 0; i < 3; ++i) (void)hipEventDestroy(e[i]); } } events{ev};
    HIP_TRY(ctx, hipEventRecord(ev[0], s));

    // ---- links: every window's segment of values ------------------------------------------------------------------------------------------
    ScopedBuf<uint64_t> seq_start, win_off_dev;
    ScopedBuf<uint32_t> value, seg_off;   // what the histogram phase reads
    uint32_t m = 0;
    if (n_text) {
        ScopedBuf<uint8_t> text;
        ScopedBuf<uint64_t> key, key_c;
        ScopedBuf<uint32_t> flag, pos, at_c, at, win;
        ScopedBuf<char> temp;
        const size_t temp_bytes = std::max({clradix::sort_temp_bytes<uint64_t>(n_text), clradix::sort_temp_bytes<uint32_t>(n_text), clradix::scan_temp_bytes(n_text)});
        if ((rc = text.alloc(ctx, n_text)) || (rc = seq_start.alloc(ctx, n + 1)) || (rc = win_off_dev.alloc(ctx, n + 1)) || (rc = key.alloc(ctx, n_text)) ||
            (rc = key_c.alloc(ctx, n_text)) || (rc = flag.alloc(ctx, n_text)) || (rc = pos.alloc(ctx, n_text)) || (rc = at_c.alloc(ctx, n_text)) ||
            (rc = temp.alloc(ctx, temp_bytes)))
            return rc;
        for (uint64_t i = 0; i < n; ++i)
            if (lens[i]) HIP_TRY(ctx, hipMemcpyAsync(text.p + h_start[i], seqs[i], lens[i], hipMemcpyHostToDevice, s));
        HIP_TRY(ctx, hipMemcpyAsync(seq_start.p, h_start.data(), (n + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, s));
        HIP_TRY(ctx, hipMemcpyAsync(win_off_dev.p, win_off, (n + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, s));
        const dim3 text_grid((n_text + kBlock - 1) / kBlock);
        hipLaunchKernelGGL(period_keys_kernel, text_grid, dim3(kBlock), 0, s, text.p, n_text, seq_start.p, (uint32_t)n, (uint32_t)p->k, key.p, flag.p);
        HIP_TRY(ctx, clradix::inclusive_sum(temp.p, temp.n, flag.p, pos.p, n_text, s));
        HIP_TRY(ctx, hipMemcpyAsync(&m, pos.p + (n_text - 1), sizeof(uint32_t), hipMemcpyDeviceToHost, s));
        hipLaunchKernelGGL(period_compact_kernel, text_grid, dim3(kBlock), 0, s, key.p, flag.p, pos.p, n_text, key_c.p, at_c.p);
        HIP_TRY(ctx, hipGetLastError());
        HIP_TRY(ctx, hipStreamSynchronize(s));
        if (m) {
            const dim3 grid((m + kBlock - 1) / kBlock);
            if ((rc = at.alloc(ctx, m)) || (rc = win.alloc(ctx, m)) || (rc = value.alloc(ctx, m)) || (rc = seg_off.alloc(ctx, (size_t)G + 1))) return rc;
            // by k-mer: (key_c, at_c) -> (key, at); then (window, value) of every occurrence -> (win, flag), with one window -> (win, value):
            // the order is already the final one
            HIP_TRY(ctx, clradix::sort_pairs<uint64_t>(temp.p, temp.n, key_c.p, key.p, at_c.p, at.p, m, 0u, 2u * (uint32_t)p->k, s));
            hipLaunchKernelGGL(period_link_kernel, grid, dim3(kBlock), 0, s, key.p, at.p, m, seq_start.p, win_off_dev.p, (uint32_t)n, p->window, D, win.p,
                               G > 1 ? flag.p : value.p);
            HIP_TRY(ctx, hipGetLastError());
            // by window alone, stable: (win, flag) -> (pos, value)
            const uint32_t* win_sorted = win.p;
            if (G > 1) {
                HIP_TRY(ctx, clradix::sort_pairs<uint32_t>(temp.p, temp.n, win.p, pos.p, flag.p, value.p, m, 0u, bits_for(G - 1), s));
                win_sorted = pos.p;
            }
            hipLaunchKernelGGL(period_offsets_kernel, dim3((G + 1 + kBlock - 1) / kBlock), dim3(kBlock), 0, s, win_sorted, m, G, seg_off.p);
            HIP_TRY(ctx, hipGetLastError());
            HIP_TRY(ctx, hipStreamSynchronize(s));   // (the arrays of this block are released at its end)
        }
    }
    HIP_TRY(ctx, hipEventRecord(ev[1], s));

    // ---- hist: window rows, sequence totals, peaks; without a k-mer everything stays zero, as the caller made it ----------------------------
    if (m) {
        ScopedBuf<uint32_t> hist_dev, counters;
        ScopedBuf<uint2> peaks_dev;
        if ((rc = hist_dev.alloc(ctx, (size_t)R * bins)) || (rc = counters.alloc(ctx, 4 * (size_t)R)) || (rc = peaks_dev.alloc(ctx, (size_t)R * p->n_peaks))) return rc;
        const size_t hist_lds = (size_t)std::max(bins, 2 * kRowWaves) * sizeof(uint32_t);
        hipLaunchKernelGGL(period_hist_kernel, dim3(std::min(G, kMaxGrid)), dim3(kRowBlock), hist_lds, s, value.p, seg_off.p, G, D, R, hist_dev.p, counters.p);
        HIP_TRY(ctx, hipGetLastError());
        hipLaunchKernelGGL(period_total_kernel, dim3((uint32_t)((n * bins + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, win_off_dev.p, (uint32_t)n, G, D, R, hist_dev.p,
                           counters.p);
        HIP_TRY(ctx, hipGetLastError());
        hipLaunchKernelGGL(period_peaks_kernel, dim3(R), dim3(kRowBlock), (size_t)bins * sizeof(uint32_t), s, hist_dev.p, D, p->n_peaks, p->peak_radius, p->min_period,
                           p->min_count, peaks_dev.p);
        HIP_TRY(ctx, hipGetLastError());
        HIP_TRY(ctx, hipEventRecord(ev[2], s));
        uint32_t* const into[4] = {kmers, links, far, last};
        for (int c = 0; c < 4; ++c) HIP_TRY(ctx, hipMemcpyAsync(into[c], counters.p + c * (size_t)R, (size_t)R * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
        HIP_TRY(ctx, hipMemcpyAsync(peaks, peaks_dev.p, (size_t)R * p->n_peaks * sizeof(uint2), hipMemcpyDeviceToHost, s));
        if (hist) HIP_TRY(ctx, hipMemcpyAsync(hist, hist_dev.p, (size_t)R * bins * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
        HIP_TRY(ctx, hipStreamSynchronize(s));   // (the device arrays of this block are released at its end)
    } else {
        HIP_TRY(ctx, hipEventRecord(ev[2], s));
        HIP_TRY(ctx, hipStreamSynchronize(s));
    }
    if (links_ms) (void)hipEventElapsedTime(links_ms, ev[0], ev[1]);
    if (hist_ms) (void)hipEventElapsedTime(hist_ms, ev[1], ev[2]);
    return CL_OK;
}
