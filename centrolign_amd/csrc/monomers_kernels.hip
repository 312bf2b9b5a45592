// monomers_kernels.hip — the device half of cl_monomer_decompose_compute (cl_monomers_api.cpp): the row-by-row DP of every problem
// against all templates at once, and the walk back over its records.
//
//   dp      monomer_dp_kernel<R>, one workgroup per problem in a persistent loop.  The templates' cells j = 1 .. len_m lie back to back on one axis;
//           lane t owns the R cells t * R .. t * R + R - 1 and keeps their values in registers.  A value (score, start) is one signed 64-bit word,
//           score << 44 | (start + 1) << 13, so that one comparison decides the order; the low 13 bits are zero in a cell and hold 8191 - m in a
//           candidate for rec[i], which makes "ties to the smallest m" part of the same comparison.  Scores are kept relative to E of the row
//           before (every value of a row is shifted alike, so no comparison changes): they stay within +-2^18 whatever the length of the problem,
//           and E itself is summed up in 64 bits.  A score is added to the high word alone.
//           A row: T in place from the highest cell down (the diagonal of the lane's first cell comes from the lane below by a wave shift, across
//           waves through LDS); X = T - j * deletion; a max-scan of X inside the lane, across the wave with the segment boundaries (the template
//           starts, which never move) folded into six per-lane accept bits, across waves through LDS; D = X + j * deletion; the wave maximum of
//           the templates' last cells; E and the fix-up.  Two barriers a row.  The sequence's bases come 64 rows at a time, one batch ahead, and
//           a row's base is read from a lane of the batch.  Wave 0 keeps row i's record in lane (i - 1) % 64 and stores 64 of them at once.
//   trace   monomer_trace_kernel, one lane per problem, first counting the kept blocks, then (behind cl_radix.h's inclusive sum) writing them in
//           ascending order.
// No global atomics, no scratch, no floating point.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cstdlib>
#include <vector>

#include "cl_internal.hpp"
#include "cl_radix.h"
#include "kmer_code.h"

namespace {

constexpr uint32_t kBlock = 256;
constexpr uint32_t kMaxGrid = 2048;     // workgroups of the persistent DP loop
constexpr uint32_t kMaxWaves = 16;
constexpr int64_t kNone = INT64_MIN;    // below every value
constexpr uint32_t kMetaFirst = 1u << 14, kMetaLast = 1u << 15, kMetaValid = 1u << 16;   // a slot's word: j | base << 11 | flags | m << 17
constexpr uint32_t kCellFirst = 8u, kCellLast = 16u;                                     // a cell's register: (j * deletion) << 12 | flags | base

struct MonomerRecord { int64_t E; uint32_t start1, m; };                  // rec[i]: E[i], start + 1, m
struct MonomerClose { int64_t score; uint32_t start1, m, flags, pad; };   // the closing cell: its score (absolute), start + 1, m, partial-right
struct MonomerScores { int32_t match, mismatch, insertion, deletion; };
static_assert(sizeof(MonomerRecord) == 16 && sizeof(MonomerClose) == 24, "records are stored whole");

__device__ __forceinline__ int64_t add_hi(int64_t v, int32_t hi) { return v + (int64_t)((uint64_t)(uint32_t)hi << 32); }   // hi = score << 12
__device__ __forceinline__ int64_t max64(int64_t a, int64_t b) { return a > b ? a : b; }
__device__ __forceinline__ int64_t up64(int64_t v, unsigned d) { return (int64_t)__shfl_up((long long)v, d, 64); }
__device__ __forceinline__ int64_t wave_max64(int64_t v) {
    for (int o = 32; o > 0; o >>= 1) v = max64(v, (int64_t)__shfl_xor((long long)v, o, 64));
    return v;
}

template <int R> struct MaxThreads { static constexpr int value = R >= 24 ? 256 : R >= 8 ? 512 : 1024; };

template <int R>
__global__ void __launch_bounds__(MaxThreads<R>::value) monomer_dp_kernel(const uint8_t* __restrict__ text, const ClMonomerProblem* __restrict__ problems, uint32_t n_problems,
                                                                          const uint32_t* __restrict__ meta, MonomerScores sc, MonomerRecord* __restrict__ rec,
                                                                          MonomerClose* __restrict__ closing) {
    __shared__ int64_t s_total[kMaxWaves], s_rec[kMaxWaves], s_last[kMaxWaves];
    __shared__ uint32_t s_flag[kMaxWaves], s_key[kMaxWaves];
    const uint32_t tid = threadIdx.x, wave = tid >> 6, lane = tid & 63u, n_waves = blockDim.x >> 6;
    const int32_t match_hi = (int32_t)((uint32_t)sc.match << 12), mismatch_hi = (int32_t)((uint32_t)sc.mismatch << 12), ins_hi = (int32_t)((uint32_t)sc.insertion << 12);

    // ---- what never changes: the lane's cells, where its first template start lies, which lanes and waves a scan value may cross ---------------
    uint32_t cell[R];
    int first_pos = R;
#pragma unroll
    for (int c = R - 1; c >= 0; --c) {
        const uint32_t w = meta[tid * R + c];
        cell[c] = ((uint32_t)((int32_t)(w & 2047u) * sc.deletion) << 12) | ((w >> 11) & 7u) | (w & kMetaFirst ? kCellFirst : 0u) | (w & kMetaLast ? kCellLast : 0u);
        if (w & kMetaFirst) first_pos = c;
    }
    const uint32_t low0 = 8191u - (meta[tid * R] >> 17);   // 8191 - m of the lane's first cell
    const int32_t below_jd = tid ? (int32_t)((uint32_t)((int32_t)(meta[tid * R - 1] & 2047u) * sc.deletion) << 12) : 0;   // of the cell below the lane's first
    uint32_t accept = 0, closed = first_pos < R ? 1u : 0u;   // closed: a template starts in lanes 0 .. lane of this wave
    for (uint32_t k = 0; k < 6; ++k) {
        if (lane >= (1u << k) && !closed) accept |= 1u << k;
        const uint32_t below = (uint32_t)__shfl_up((int)closed, 1u << k, 64);
        if (lane >= (1u << k)) closed |= below;
    }
    const uint32_t closed_below = (uint32_t)__shfl_up((int)closed, 1, 64);
    const bool open = lane == 0 || !closed_below;   // no template starts in lanes 0 .. lane - 1: the carry of the waves below reaches this lane
    if (lane == 63) s_flag[wave] = closed;
    __syncthreads();
    uint32_t wave_from = wave;   // the carry into this wave is the maximum of the totals of waves wave_from .. wave - 1
    while (wave_from > 0) { --wave_from; if (s_flag[wave_from]) break; }

    for (uint32_t p = blockIdx.x; p < n_problems; p += gridDim.x) {
        const ClMonomerProblem q = problems[p];
        const uint32_t n = q.n;
        if (n == 0) continue;   // (uniform; no block)
        const uint8_t* const S = text + q.text_off;
        int64_t h[R];
#pragma unroll
        for (int c = 0; c < R; ++c) h[c] = 0;   // (0, -1)
        int64_t left = 0, E = 0;
        MonomerRecord mine{0, 0, 0};
        uint32_t cur = lane < n ? base_code(S[lane]) : 4u, next = 64u + lane < n ? base_code(S[64u + lane]) : 4u;
        for (uint32_t i = 1; i <= n; ++i) {
            const uint32_t slot = (i - 1u) & 63u;
            if (slot == 0 && i > 1) {
                cur = next;
                next = i + 63u + lane < n ? base_code(S[i + 63u + lane]) : 4u;
            }
            const uint32_t sb = (uint32_t)__builtin_amdgcn_readlane((int)cur, (int)slot);
            const int64_t zero = (int64_t)((uint64_t)i << 13);   // (0, i - 1): cell 0 of every template in the row before
            // T, then X, in place
#pragma unroll
            for (int c = R - 1; c >= 0; --c) {
                int64_t diag = c ? h[c ? c - 1 : 0] : left;
                diag = cell[c] & kCellFirst ? zero : diag;
                const int64_t t = max64(add_hi(diag, (cell[c] & 7u) == sb ? match_hi : mismatch_hi), add_hi(h[c], ins_hi));
                h[c] = add_hi(t, -(int32_t)(cell[c] & ~4095u));
            }
            // the scan inside the lane
            int64_t run = kNone;
#pragma unroll
            for (int c = 0; c < R; ++c) {
                run = cell[c] & kCellFirst ? h[c] : max64(run, h[c]);
                h[c] = run;
            }
            // across the wave, across the waves
            int64_t v = run;
#pragma unroll
            for (uint32_t k = 0; k < 6; ++k) {
                const int64_t y = up64(v, 1u << k);
                if (accept & (1u << k)) v = max64(v, y);
            }
            int64_t carry = up64(v, 1);
            if (lane == 0) carry = kNone;
            if (lane == 63) s_total[wave] = v;
            __syncthreads();
            if (open) for (uint32_t u = wave_from; u < wave; ++u) carry = max64(carry, s_total[u]);
            // D, and the best last cell
            int64_t cand = kNone;
            uint32_t low = low0;
#pragma unroll
            for (int c = 0; c < R; ++c) {
                if (c < first_pos) h[c] = max64(h[c], carry);
                h[c] = add_hi(h[c], (int32_t)(cell[c] & ~4095u));
                if (c > 0 && (cell[c] & kCellFirst)) --low;
                if (cell[c] & kCellLast) cand = max64(cand, h[c] | (int64_t)low);
            }
            cand = wave_max64(cand);
            if (lane == 0) s_rec[wave] = cand;
            if (lane == 63) s_last[wave] = h[R - 1];
            __syncthreads();
            int64_t best = s_rec[0];
            for (uint32_t u = 1; u < n_waves; ++u) best = max64(best, s_rec[u]);
            const int32_t e_hi = (int32_t)((uint64_t)best >> 32) & ~4095;   // (E[i] - E[i - 1]) << 12
            E += (int64_t)(e_hi >> 12);
            // the fix-up; the row is now relative to E[i]
            const uint32_t here = (i + 1u) << 13;   // start = i, in the low word (i + 1 <= 2^30: the high word's share is (i + 1) >> 19)
            const int32_t here_hi = (int32_t)((i + 1u) >> 19);
#pragma unroll
            for (int c = 0; c < R; ++c) {
                const int64_t fix = (int64_t)(((uint64_t)(uint32_t)((int32_t)(cell[c] & ~4095u) + here_hi) << 32) | here);
                h[c] = max64(add_hi(h[c], -e_hi), fix);
            }
            left = up64(h[R - 1], 1);
            if (lane == 0 && wave > 0) {
                const int64_t fix = (int64_t)(((uint64_t)(uint32_t)(below_jd + here_hi) << 32) | here);
                left = max64(add_hi(s_last[wave - 1], -e_hi), fix);
            }
            // the record: lane (i - 1) % 64 of wave 0 keeps it until 64 are there
            if (wave == 0) {
                if (lane == slot) {
                    mine.E = E;
                    mine.start1 = (uint32_t)(((uint64_t)best >> 13) & 0x7FFFFFFFull);
                    mine.m = 8191u - ((uint32_t)best & 8191u);
                }
                if ((slot == 63u || i == n) && lane <= slot) rec[q.rec_off + (i - 1u - slot) + lane] = mine;
            }
        }
        // ---- the closing cell: the largest value, then the smallest m, then the largest j ------------------------------------------------------
        int64_t top = kNone;
        uint32_t top_key = 0;   // (8191 - m) << 12 | j << 1 | last
#pragma unroll
        for (int c = 0; c < R; ++c) {
            const uint32_t w = meta[tid * R + c];
            const uint32_t key = ((8191u - (w >> 17)) << 12) | ((w & 2047u) << 1) | (w & kMetaLast ? 1u : 0u);
            if ((w & kMetaValid) && (h[c] > top || (h[c] == top && key > top_key))) { top = h[c]; top_key = key; }
        }
        const int64_t wave_top = wave_max64(top);
        __syncthreads();   // (s_rec was read in the last row)
        if (lane == 0) s_rec[wave] = wave_top;
        __syncthreads();
        int64_t all_top = s_rec[0];
        for (uint32_t u = 1; u < n_waves; ++u) all_top = max64(all_top, s_rec[u]);
        uint32_t key = top == all_top ? top_key : 0u;
        for (int o = 32; o > 0; o >>= 1) key = max(key, (uint32_t)__shfl_xor((int)key, o, 64));
        if (lane == 0) s_key[wave] = key;
        __syncthreads();
        if (tid == 0) {
            for (uint32_t u = 1; u < n_waves; ++u) key = max(key, s_key[u]);
            MonomerClose cl;
            cl.score = E + (all_top >> 44);
            cl.start1 = (uint32_t)(((uint64_t)all_top >> 13) & 0x7FFFFFFFull);
            cl.m = 8191u - (key >> 12);
            cl.flags = key & 1u ? 0u : CL_MONOMER_PARTIAL_RIGHT;
            cl.pad = 0;
            closing[p] = cl;
        }
        __syncthreads();   // (s_rec and s_key are written again in the next problem)
    }
}

// Problem p: its kept blocks, from the closing cell back.  write = 0: count[p] = their number.  write = 1: count holds the inclusive sums and the
// blocks go to blocks[count[p] - k .. count[p]) in ascending order.
__global__ void __launch_bounds__(kBlock) monomer_trace_kernel(const ClMonomerProblem* __restrict__ problems, uint32_t n_problems, const MonomerRecord* __restrict__ rec,
                                                               const MonomerClose* __restrict__ closing, uint32_t* __restrict__ count, cl_monomer_block* __restrict__ blocks,
                                                               int write) {
    const uint32_t p = blockIdx.x * kBlock + threadIdx.x;
    if (p >= n_problems) return;
    const ClMonomerProblem q = problems[p];
    uint32_t kept = 0;
    if (q.n) {
        const MonomerRecord* const r = rec + q.rec_off;   // r[i - 1] = rec[i]
        const MonomerClose cl = closing[p];
        const uint32_t end_off = write ? count[p] : 0u;
        uint32_t end = q.n, start1 = cl.start1, m = cl.m, flags = cl.flags;
        int64_t score = cl.score;
        for (;;) {
            const uint32_t start = start1 ? start1 - 1u : 0u;
            if (start >= end) break;   // (never: rec[i].start <= i - 1)
            const uint32_t at = q.row0 + start;
            if (at < q.keep_lo) break;   // the starts only descend
            if (at < q.keep_hi) {
                if (write) {
                    const int64_t s = score - (start ? r[start - 1].E : (int64_t)0);
                    cl_monomer_block b;
                    b.sequence = q.seq;
                    b.start = at;
                    b.end = q.row0 + end;
                    b.monomer = m;
                    b.score = (int32_t)(s < (int64_t)INT32_MIN ? (int64_t)INT32_MIN : s > (int64_t)INT32_MAX ? (int64_t)INT32_MAX : s);
                    b.flags = flags | (start1 ? 0u : CL_MONOMER_PARTIAL_LEFT);
                    blocks[end_off - 1u - kept] = b;
                }
                ++kept;
            }
            if (start == 0) break;
            const MonomerRecord t = r[start - 1];
            end = start;
            score = t.E;
            start1 = t.start1;
            m = t.m;
            flags = 0;
        }
    }
    if (!write) count[p] = kept;
}

// Cells a lane: the set the kernel is built for, and the cost model of DESIGN.md §20, fitted to the row steps measured there.  A row of a workgroup
// of W waves with R cells a lane takes about 0.1 R + 0.16 W + 0.3 us while the SIMD has the wave to itself.  A compute unit holds g workgroups
// (kWavesPerSimd, from the compiler's register report, times 4 SIMDs, over W); P problems take P / (CUs * g) rounds, and from 1.5 waves a SIMD on
// the waves of a SIMD wait for each other.  Few problems choose many short lanes, many problems one long one.
constexpr int kCellChoices[5] = {4, 8, 16, 24, 36};
constexpr int kWavesPerSimd[5] = {4, 3, 2, 1, 1};
int max_threads_of(int R) { return R >= 24 ? 256 : R >= 8 ? 512 : 1024; }

int choose_cells(uint32_t A, uint32_t P, uint32_t n_cu, uint32_t* threads) {
    const char* forced = getenv("CL_MONOMERS_CELLS");   // tests put wave and workgroup boundaries inside small template sets with it
    int best = 0;
    double best_cost = 0.0;
    for (int k = 0; k < 5; ++k) {
        const int R = kCellChoices[k];
        const uint32_t waves = ((A + R - 1) / R + 63) / 64;
        if (waves * 64 > (uint32_t)max_threads_of(R)) continue;
        const uint32_t held = std::max(1u, 4u * kWavesPerSimd[k] / waves), resident = std::min(held, (P + n_cu - 1) / n_cu);
        double cost = std::max(1.0, (double)P / ((double)n_cu * held)) * (0.1 * R + 0.16 * waves + 0.3) * std::max(1.0, resident * waves / 4.0 / 1.5);
        if (forced && atoi(forced) == R) cost = 0.0;
        if (!best || cost < best_cost) { best_cost = cost; best = R; *threads = waves * 64; }
    }
    return best;
}

}  // namespace

int cl_monomers_device(cl_context* ctx, const char* const* seqs, const uint64_t* lens, uint64_t n, const std::vector<uint8_t>& codes, const std::vector<uint32_t>& tmpl_off,
                       const cl_monomers_params* p, const std::vector<ClMonomerProblem>& problems, std::vector<cl_monomer_block>& out, float* dp_ms, float* trace_ms) {
    hipStream_t s = ctx->stream;
    int rc;
    out.clear();
    const uint32_t P = (uint32_t)problems.size(), A = (uint32_t)codes.size();   // P <= 2^24 + 2^28, A <= 8192 (checked by the caller)
    if (P == 0) return CL_OK;
    uint32_t threads = 0;
    int n_cu = 0;
    HIP_TRY(ctx, hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, ctx->device));
    const int R = choose_cells(A, P, (uint32_t)std::max(n_cu, 1), &threads);
    if (!R) { cl_set_error(ctx, "templates: no kernel holds %u template bases", A); return CL_ERR_INVALID_ARGUMENT; }
    std::vector<uint32_t> meta((size_t)threads * R, 1u | (5u << 11) | kMetaFirst);   // a slot past the last template: a start of its own that matches nothing
    for (size_t m = 0; m + 1 < tmpl_off.size(); ++m)
        for (uint32_t a = tmpl_off[m]; a < tmpl_off[m + 1]; ++a) {
            const uint32_t j = a - tmpl_off[m] + 1;
            meta[a] = j | ((uint32_t)codes[a] << 11) | (j == 1 ? kMetaFirst : 0u) | (a + 1 == tmpl_off[m + 1] ? kMetaLast : 0u) | kMetaValid | ((uint32_t)m << 17);
        }
    std::vector<uint64_t> h_start(n + 1, 0);
    for (uint64_t i = 0; i < n; ++i) h_start[i + 1] = h_start[i] + lens[i];
    const uint64_t n_text = h_start[n], n_rows = problems.back().rec_off + problems.back().n;
    hipEvent_t ev[3];
    for (auto& e : ev) HIP_TRY(ctx, hipEventCreate(&e));
    struct Events { hipEvent_t* e; ~Events() { for (int i = 0; i < 3; ++i) (void)hipEventDestroy(e[i]); } } events{ev};

    ScopedBuf<uint8_t> text;
    ScopedBuf<ClMonomerProblem> problems_dev;
    ScopedBuf<uint32_t> meta_dev, count, offsets;
    ScopedBuf<MonomerRecord> rec;
    ScopedBuf<MonomerClose> closing;
    ScopedBuf<cl_monomer_block> blocks;
    ScopedBuf<char> temp;
    if ((rc = text.alloc(ctx, n_text)) || (rc = problems_dev.alloc(ctx, P)) || (rc = meta_dev.alloc(ctx, meta.size())) || (rc = count.alloc(ctx, P)) ||
        (rc = offsets.alloc(ctx, P)) || (rc = rec.alloc(ctx, n_rows)) || (rc = closing.alloc(ctx, P)) || (rc = temp.alloc(ctx, clradix::scan_temp_bytes(P))))
        return rc;
    for (uint64_t i = 0; i < n; ++i)
        if (lens[i]) HIP_TRY(ctx, hipMemcpyAsync(text.p + h_start[i], seqs[i], lens[i], hipMemcpyHostToDevice, s));
    HIP_TRY(ctx, hipMemcpyAsync(problems_dev.p, problems.data(), (size_t)P * sizeof(ClMonomerProblem), hipMemcpyHostToDevice, s));
    HIP_TRY(ctx, hipMemcpyAsync(meta_dev.p, meta.data(), meta.size() * sizeof(uint32_t), hipMemcpyHostToDevice, s));
    const MonomerScores sc{p->match, p->mismatch, p->insertion, p->deletion};
    const dim3 grid(std::min(P, kMaxGrid)), block(threads);
    HIP_TRY(ctx, hipEventRecord(ev[0], s));
    switch (R) {
    case 4: hipLaunchKernelGGL(monomer_dp_kernel<4>, grid, block, 0, s, text.p, problems_dev.p, P, meta_dev.p, sc, rec.p, closing.p); break;
    case 8: hipLaunchKernelGGL(monomer_dp_kernel<8>, grid, block, 0, s, text.p, problems_dev.p, P, meta_dev.p, sc, rec.p, closing.p); break;
    case 16: hipLaunchKernelGGL(monomer_dp_kernel<16>, grid, block, 0, s, text.p, problems_dev.p, P, meta_dev.p, sc, rec.p, closing.p); break;
    case 24: hipLaunchKernelGGL(monomer_dp_kernel<24>, grid, block, 0, s, text.p, problems_dev.p, P, meta_dev.p, sc, rec.p, closing.p); break;
    default: hipLaunchKernelGGL(monomer_dp_kernel<36>, grid, block, 0, s, text.p, problems_dev.p, P, meta_dev.p, sc, rec.p, closing.p); break;
    }
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipEventRecord(ev[1], s));
    const dim3 trace_grid((P + kBlock - 1) / kBlock);
    hipLaunchKernelGGL(monomer_trace_kernel, trace_grid, dim3(kBlock), 0, s, problems_dev.p, P, rec.p, closing.p, count.p, (cl_monomer_block*)nullptr, 0);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, clradix::inclusive_sum(temp.p, temp.n, count.p, offsets.p, P, s));
    uint32_t n_blocks = 0;
    HIP_TRY(ctx, hipMemcpyAsync(&n_blocks, offsets.p + (P - 1), sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(ctx, hipStreamSynchronize(s));
    if (n_blocks) {
        if ((rc = blocks.alloc(ctx, n_blocks))) return rc;
        hipLaunchKernelGGL(monomer_trace_kernel, trace_grid, dim3(kBlock), 0, s, problems_dev.p, P, rec.p, closing.p, offsets.p, blocks.p, 1);
        HIP_TRY(ctx, hipGetLastError());
    }
    HIP_TRY(ctx, hipEventRecord(ev[2], s));
    if (n_blocks) {
        out.resize(n_blocks);
        HIP_TRY(ctx, hipMemcpyAsync(out.data(), blocks.p, (size_t)n_blocks * sizeof(cl_monomer_block), hipMemcpyDeviceToHost, s));
    }
    HIP_TRY(ctx, hipStreamSynchronize(s));
    if (dp_ms) (void)hipEventElapsedTime(dp_ms, ev[0], ev[1]);
    if (trace_ms) (void)hipEventElapsedTime(trace_ms, ev[1], ev[2]);
    return CL_OK;
}
