// strands_kernels.hip — the device half of cl_strand_profile_compute (cl_strands_api.cpp): for every position of the input the vote
// of its k-mer (forward, reverse or neutral against the majority of the input's own k-mer occurrences), and the sums of the votes per window.
//
//   sort    one key per text position: the 2k-bit canonical k-mer min(x, rc(x)); the value word holds the 30-bit global position and, above it,
//           the class of the occurrence (x is the smaller of the pair, the larger, or a palindrome).  A scan + compaction of the positions that
//           have a k-mer, then one stable radix sort by key (cl_radix.h): every occurrence of x and of rc(x) lies in one run.
//   vote    head flags of the runs and the "is the larger" flags, one scan of each: the first gives dense run numbers (the last one is
//           `distinct`), by which the run starts are scattered; the second makes a run's two counts differences of prefix sums, so that no thread
//           walks a run (a k-mer of a HOR array occurs tens of thousands of times and its run spans many workgroups).  strand_vote_kernel writes
//           the vote of every occurrence to its text position, one byte; strand_window_kernel, one wave per window, sums the bytes of a window
//           four at a time and reduces across the wave.
// No atomics, no LDS of its own, no floating point.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "cl_internal.hpp"
#include "cl_radix.h"
#include "kmer_code.h"

namespace {

constexpr uint32_t kBlock = 256, kWaves = kBlock / 64;
constexpr uint32_t kPosBits = 30, kPosMask = (1u << kPosBits) - 1u;   // the text holds fewer than 2^30 bases
enum : uint32_t { SMALLER = 0, LARGER = 1, PALINDROME = 2 };          // x against rc(x)
enum : uint32_t { NO_KMER = 0, FORWARD = 1, REVERSE = 2, NEUTRAL = 3 };

// position p of the text: its canonical k-mer and class, and whether [p, p + k) lies in one sequence and holds only ACGTacgt
__global__ void __launch_bounds__(kBlock) strand_keys_kernel(const uint8_t* __restrict__ text, uint32_t n_text, const uint64_t* __restrict__ seq_start, uint32_t n_seq,
                                                             uint32_t k, uint64_t* __restrict__ key, uint32_t* __restrict__ value, uint32_t* __restrict__ flag) {
    const uint32_t p = blockIdx.x * kBlock + threadIdx.x;
    if (p >= n_text) return;
    uint32_t lo = 0, hi = n_seq;   // the sequence of p: largest s with seq_start[s] <= p (an empty sequence shares its start with the next one)
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) / 2;
        if (seq_start[mid] <= p) lo = mid; else hi = mid;
    }
    uint64_t kmer = 0, rev = 0;
    uint32_t ok = (uint64_t)p + k <= seq_start[lo + 1] ? 1u : 0u;
    for (uint32_t j = 0; ok && j < k; ++j) {
        const uint32_t c = base_code(text[p + j]);
        if (c > 3) ok = 0u;
        kmer = (kmer << 2) | c;
        rev |= (uint64_t)(3u - (c & 3u)) << (2u * j);
    }
    const uint32_t cls = kmer < rev ? SMALLER : kmer > rev ? LARGER : PALINDROME;
    key[p] = ok ? (kmer < rev ? kmer : rev) : 0ull;
    value[p] = p | (cls << kPosBits);
    flag[p] = ok;
}

// the flagged (key, value) pairs, in text order, to the front (pos = inclusive scan of the flags)
__global__ void __launch_bounds__(kBlock) strand_compact_kernel(const uint64_t* __restrict__ key, const uint32_t* __restrict__ value, const uint32_t* __restrict__ flag,
                                                                const uint32_t* __restrict__ pos, uint32_t n_text, uint64_t* __restrict__ key_out,
                                                                uint32_t* __restrict__ value_out) {
    const uint32_t p = blockIdx.x * kBlock + threadIdx.x;
    if (p >= n_text || !flag[p]) return;
    key_out[pos[p] - 1] = key[p];
    value_out[pos[p] - 1] = value[p];
}

// sorted by key: head[j] = occurrence j opens a run, larger[j] = it is the larger of its pair
__global__ void __launch_bounds__(kBlock) strand_flags_kernel(const uint64_t* __restrict__ key, const uint32_t* __restrict__ value, uint32_t m, uint32_t* __restrict__ head,
                                                              uint32_t* __restrict__ larger) {
    const uint32_t j = blockIdx.x * kBlock + threadIdx.x;
    if (j >= m) return;
    head[j] = j == 0 || key[j] != key[j - 1] ? 1u : 0u;
    larger[j] = (value[j] >> kPosBits) == LARGER ? 1u : 0u;
}

// run_no = inclusive scan of head: run r = run_no - 1 starts at run_start[r]; run_start[number of runs] = m
__global__ void __launch_bounds__(kBlock) strand_starts_kernel(const uint32_t* __restrict__ head, const uint32_t* __restrict__ run_no, uint32_t m,
                                                               uint32_t* __restrict__ run_start) {
    const uint32_t j = blockIdx.x * kBlock + threadIdx.x;
    if (j >= m) return;
    if (head[j]) run_start[run_no[j] - 1] = j;
    if (j == m - 1) run_start[run_no[j]] = m;
}

// occurrence j of run [s, e): `high` of the run's occurrences are the larger of the pair (larger_sum = inclusive scan of larger), the others the
// smaller; its own side's count is a, the other b.  votes[position] = its code
__global__ void __launch_bounds__(kBlock) strand_vote_kernel(const uint32_t* __restrict__ value, const uint32_t* __restrict__ run_no, const uint32_t* __restrict__ run_start,
                                                             const uint32_t* __restrict__ larger_sum, uint32_t m, uint8_t* __restrict__ votes) {
    const uint32_t j = blockIdx.x * kBlock + threadIdx.x;
    if (j >= m) return;
    const uint32_t r = run_no[j] - 1, s = run_start[r], e = run_start[r + 1];   // s <= j < e <= m
    const uint32_t high = larger_sum[e - 1] - (s ? larger_sum[s - 1] : 0u), low = e - s - high;
    const uint32_t v = value[j], cls = v >> kPosBits;
    const uint32_t a = cls == LARGER ? high : low, b = cls == LARGER ? low : high;
    uint32_t code = NEUTRAL;   // a palindrome, a + b < 2 (then b = 0, a = 1), a = b
    if (cls != PALINDROME && a + b >= 2u && a != b) code = a > b ? FORWARD : REVERSE;
    votes[v & kPosMask] = (uint8_t)code;
}

// Window g = blockIdx.x * kWaves + wave: counters[g], [G + g], [2 G + g] = the positions of the window with a k-mer, a forward and a reverse vote.
// The votes are read as aligned words of four (the array is padded to whole words), the bytes outside the window masked away; a code has two bits,
// so three population counts a word; the three sums (at most 2^20 each) share one 64-bit word through the wave reduction.
__global__ void __launch_bounds__(kBlock) strand_window_kernel(const uint32_t* __restrict__ votes4, const uint64_t* __restrict__ seq_start, const uint64_t* __restrict__ win_off,
                                                               uint32_t n_seq, uint32_t n_windows, uint32_t window, uint32_t* __restrict__ counters) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t g64 = (uint64_t)blockIdx.x * kWaves + (threadIdx.x >> 6);
    if (g64 >= n_windows) return;   // (a whole wave leaves: no lane of it takes part in the shuffles below)
    const uint32_t g = (uint32_t)g64;
    uint32_t lo = 0, hi = n_seq;   // the sequence of g: largest s with win_off[s] <= g
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) / 2;
        if (win_off[mid] <= g) lo = mid; else hi = mid;
    }
    const uint32_t begin = (uint32_t)(seq_start[lo] + (uint64_t)(g - (uint32_t)win_off[lo]) * window);
    const uint64_t seq_end = seq_start[lo + 1];
    const uint32_t end = (uint64_t)begin + window < seq_end ? begin + window : (uint32_t)seq_end;   // begin < end <= n_text < 2^30
    unsigned long long sums = 0;   // kmers | forward << 21 | reverse << 42
    for (uint32_t w = begin / 4u + lane; w < (end + 3u) / 4u; w += 64u) {
        uint32_t word = votes4[w];
        const uint32_t first = w * 4u;
        if (first < begin) word &= 0xFFFFFFFFu << (8u * (begin - first));            // (begin - first <= 3)
        if (first + 4u > end) word &= 0xFFFFFFFFu >> (8u * (first + 4u - end));      // (first + 4 - end <= 3)
        const uint32_t low = word & 0x01010101u, high = (word >> 1) & 0x01010101u;
        sums += (unsigned long long)__popc(low | high) | ((unsigned long long)__popc(low & ~high) << 21) | ((unsigned long long)__popc(high & ~low) << 42);
    }
    for (int o = 32; o > 0; o >>= 1) sums += __shfl_xor(sums, o);
    if (lane == 0) {
        counters[g] = (uint32_t)(sums & 0x1FFFFFu);
        counters[(size_t)n_windows + g] = (uint32_t)((sums >> 21) & 0x1FFFFFu);
        counters[2 * (size_t)n_windows + g] = (uint32_t)((sums >> 42) & 0x1FFFFFu);
    }
}

}  // namespace

int cl_strands_device(cl_context* ctx, const char* const* seqs, const uint64_t* lens, uint64_t n, const uint64_t* win_off, const uint64_t* base_off,
                      const cl_strands_params* p, uint32_t* kmers, uint32_t* forward, uint32_t* reverse, uint8_t* votes, uint64_t* distinct, float* sort_ms,
                      float* vote_ms) {
    hipStream_t s = ctx->stream;
    int rc;
    const uint32_t G = (uint32_t)win_off[n], n_text = (uint32_t)base_off[n];   // n_text < 2^30 (checked by the caller), G <= n_text
    *distinct = 0;
    hipEvent_t ev[3];
    for (auto& e : ev) HIP_TRY(ctx, hipEventCreate(&e));
    struct Events { hipEvent_t* e; ~Events() { for (int i = 0; i < 3; ++i) (void)hipEventDestroy(e[i]); } } events{ev};
    HIP_TRY(ctx, hipEventRecord(ev[0], s));
    if (!n_text) {   // no base: every array of the caller is empty
        HIP_TRY(ctx, hipEventRecord(ev[1], s));
        HIP_TRY(ctx, hipEventRecord(ev[2], s));
        HIP_TRY(ctx, hipStreamSynchronize(s));
        (void)hipEventElapsedTime(sort_ms, ev[0], ev[1]);
        (void)hipEventElapsedTime(vote_ms, ev[1], ev[2]);
        return CL_OK;
    }

    // ---- sort: the occurrences by canonical k-mer --------------------------------------------------------------------------------------------
    ScopedBuf<uint8_t> text;
    ScopedBuf<uint64_t> seq_start, win_off_dev, key, key_c;
    ScopedBuf<uint32_t> value, value_c, flag, pos, votes4, counters;
    ScopedBuf<char> temp;
    const size_t temp_bytes = std::max(clradix::sort_temp_bytes<uint64_t>(n_text), clradix::scan_temp_bytes(n_text));
    const size_t vote_words = (size_t)n_text / 4 + 1;
    // key_c holds n_text + 1 keys: after the sort it is read as 2 n_text + 2 words, the prefix sums [n_text] and the run starts [at most n_text + 1]
    if ((rc = text.alloc(ctx, n_text)) || (rc = seq_start.alloc(ctx, n + 1)) || (rc = win_off_dev.alloc(ctx, n + 1)) || (rc = key.alloc(ctx, n_text)) ||
        (rc = key_c.alloc(ctx, (size_t)n_text + 1)) || (rc = value.alloc(ctx, n_text)) || (rc = value_c.alloc(ctx, n_text)) || (rc = flag.alloc(ctx, n_text)) ||
        (rc = pos.alloc(ctx, n_text)) || (rc = votes4.alloc(ctx, vote_words)) || (rc = counters.alloc(ctx, 3 * (size_t)G)) || (rc = temp.alloc(ctx, temp_bytes)))
        return rc;
    for (uint64_t i = 0; i < n; ++i)
        if (lens[i]) HIP_TRY(ctx, hipMemcpyAsync(text.p + base_off[i], seqs[i], lens[i], hipMemcpyHostToDevice, s));
    HIP_TRY(ctx, hipMemcpyAsync(seq_start.p, base_off, (n + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, s));
    HIP_TRY(ctx, hipMemcpyAsync(win_off_dev.p, win_off, (n + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, s));
    HIP_TRY(ctx, hipMemsetAsync(votes4.p, 0, vote_words * sizeof(uint32_t), s));
    const dim3 text_grid((n_text + kBlock - 1) / kBlock);
    uint32_t m = 0;
    hipLaunchKernelGGL(strand_keys_kernel, text_grid, dim3(kBlock), 0, s, text.p, n_text, seq_start.p, (uint32_t)n, (uint32_t)p->k, key.p, value.p, flag.p);
    HIP_TRY(ctx, clradix::inclusive_sum(temp.p, temp.n, flag.p, pos.p, n_text, s));
    HIP_TRY(ctx, hipMemcpyAsync(&m, pos.p + (n_text - 1), sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    hipLaunchKernelGGL(strand_compact_kernel, text_grid, dim3(kBlock), 0, s, key.p, value.p, flag.p, pos.p, n_text, key_c.p, value_c.p);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipStreamSynchronize(s));
    // (key_c, value_c) -> (key, value)
    if (m) HIP_TRY(ctx, clradix::sort_pairs<uint64_t>(temp.p, temp.n, key_c.p, key.p, value_c.p, value.p, m, 0u, 2u * (uint32_t)p->k, s));
    HIP_TRY(ctx, hipEventRecord(ev[1], s));

    // ---- vote: runs, their two counts, the votes and the window sums; without a k-mer everything stays zero, as the caller made it ----------
    uint32_t runs = 0;
    if (m) {
        const dim3 grid((m + kBlock - 1) / kBlock);
        uint32_t* const head = flag.p;                                      // [m]
        uint32_t* const run_no = pos.p;                                     // [m]
        uint32_t* const larger = value_c.p;                                 // [m] (the sort has read it)
        uint32_t* const larger_sum = reinterpret_cast<uint32_t*>(key_c.p);  // [m]
        uint32_t* const run_start = larger_sum + n_text;                    // [runs + 1 <= m + 1 <= n_text + 1]
        hipLaunchKernelGGL(strand_flags_kernel, grid, dim3(kBlock), 0, s, key.p, value.p, m, head, larger);
        HIP_TRY(ctx, clradix::inclusive_sum(temp.p, temp.n, head, run_no, m, s));
        HIP_TRY(ctx, clradix::inclusive_sum(temp.p, temp.n, larger, larger_sum, m, s));
        HIP_TRY(ctx, hipMemcpyAsync(&runs, run_no + (m - 1), sizeof(uint32_t), hipMemcpyDeviceToHost, s));
        hipLaunchKernelGGL(strand_starts_kernel, grid, dim3(kBlock), 0, s, head, run_no, m, run_start);
        hipLaunchKernelGGL(strand_vote_kernel, grid, dim3(kBlock), 0, s, value.p, run_no, run_start, larger_sum, m, reinterpret_cast<uint8_t*>(votes4.p));
        hipLaunchKernelGGL(strand_window_kernel, dim3((G + kWaves - 1) / kWaves), dim3(kBlock), 0, s, votes4.p, seq_start.p, win_off_dev.p, (uint32_t)n, G, p->window,
                           counters.p);
        HIP_TRY(ctx, hipGetLastError());
    }
    HIP_TRY(ctx, hipEventRecord(ev[2], s));
    if (m) {
        uint32_t* const into[3] = {kmers, forward, reverse};
        for (int c = 0; c < 3; ++c) HIP_TRY(ctx, hipMemcpyAsync(into[c], counters.p + c * (size_t)G, (size_t)G * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
        if (votes) HIP_TRY(ctx, hipMemcpyAsync(votes, votes4.p, n_text, hipMemcpyDeviceToHost, s));
    }
    HIP_TRY(ctx, hipStreamSynchronize(s));   // (the device arrays are released at the end of this function)
    *distinct = runs;
    (void)hipEventElapsedTime(sort_ms, ev[0], ev[1]);
    (void)hipEventElapsedTime(vote_ms, ev[1], ev[2]);
    return CL_OK;
}
