// monomer_pileup_kernels.hip — the device half of cl_monomer_pileup_compute (cl_monomer_pileup_api.cpp): the global alignment of
// every used block to its template with the walk back, and the per-column counts.
//
//   monomer_pileup_kernel<R, LdsBits>, one wave (a workgroup of 64 lanes) per run of consecutive blocks; the blocks come ordered by forward
//   template, so a wave's counts belong to one template for many blocks on end.
//     align   lane t owns the R template columns t R + 1 .. t R + R in registers and works on row s - t + 1 at step s (an anti-diagonal
//             wavefront).  The left neighbour's last cell of the same row is one wave shift a step; its cell of the row before is the value
//             received the step before.  Two direction bits a cell (0 diagonal, 1 insertion, 2 deletion: the order in which the definition's
//             walk tries them) go to one word per (row, lane): in LDS when the batch's longest block allows it, else in a per-wave slab of
//             global memory.  No barrier inside the row loop.
//     walk    the wave walks the bits back from (n, L) (every lane the same walk: the reads are broadcasts) and leaves one code per column and
//             per slot in LDS.
//     count   the lanes add the codes to the wave's own LDS counters of the current template, 64 columns at a time; no two lanes share a
//             counter, so these are plain adds.  When the template changes, and at the end, the non-zero counters are flushed with atomicAdd
//             on the 32-bit global counters.  Integer adds commute: the result does not depend on the order.
// No floating point, no scratch.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "cl_internal.hpp"
#include "kmer_code.h"

namespace {

constexpr uint32_t kLdsBudget = 64u << 10;        // dynamic LDS of one wave; what does not fit sends the direction bits to global memory
constexpr uint32_t kLdsPerCu = 160u << 10;
constexpr uint32_t kMaxWavesPerCu = 8;
constexpr size_t kMaxSlabBytes = (size_t)256 << 20;
constexpr uint32_t kNoBase = 255;

struct PileupScores { int32_t match, mismatch, insertion, deletion; };

template <int R> struct DirWord { using type = uint32_t; };
template <> struct DirWord<1> { using type = uint8_t; };
template <> struct DirWord<2> { using type = uint8_t; };
template <> struct DirWord<3> { using type = uint8_t; };
template <> struct DirWord<4> { using type = uint8_t; };
template <> struct DirWord<8> { using type = uint16_t; };

// the LDS of one wave, in 32-bit words: counters, then the byte arrays (each rounded up to words), then the direction words
struct PileupLayout { uint32_t acc_slot, colcode, slotcode, xs, dirs, words; };
__host__ __device__ inline PileupLayout pileup_layout(uint32_t Lmax, uint32_t n_max, uint32_t dir_bytes /* 0: not in LDS */) {
    PileupLayout l;
    l.acc_slot = Lmax * 6u;
    l.colcode = l.acc_slot + (Lmax + 1u) * 5u;
    l.slotcode = l.colcode + (Lmax + 3u) / 4u;
    l.xs = l.slotcode + (Lmax + 4u) / 4u;
    l.dirs = l.xs + (n_max + 3u) / 4u;
    l.words = l.dirs + (n_max * 64u * dir_bytes + 3u) / 4u;
    return l;
}

template <int R, bool LdsBits>
__global__ void __launch_bounds__(64) monomer_pileup_kernel(const uint8_t* __restrict__ text, const ClPileupBlock* __restrict__ blocks, uint32_t n_blocks,
                                                            const uint8_t* __restrict__ codes, const uint32_t* __restrict__ tmpl_off, uint32_t M,
                                                            const uint32_t* __restrict__ col_off, PileupScores sc, uint32_t Lmax, uint32_t n_max,
                                                            typename DirWord<R>::type* __restrict__ slab, uint32_t* __restrict__ columns, uint32_t* __restrict__ slots,
                                                            int32_t* __restrict__ scores) {
    using Word = typename DirWord<R>::type;
    extern __shared__ uint32_t lds[];
    const PileupLayout lay = pileup_layout(Lmax, n_max, LdsBits ? (uint32_t)sizeof(Word) : 0u);
    uint32_t* const acc_col = lds;
    uint32_t* const acc_slot = lds + lay.acc_slot;
    uint8_t* const colcode = (uint8_t*)(lds + lay.colcode);
    uint8_t* const slotcode = (uint8_t*)(lds + lay.slotcode);
    uint8_t* const xs = (uint8_t*)(lds + lay.xs);
    Word* const dirs = LdsBits ? (Word*)(lds + lay.dirs) : slab + (size_t)blockIdx.x * n_max * 64u;
    const uint32_t lane = threadIdx.x;

    for (uint32_t k = lane; k < lay.colcode; k += 64u) lds[k] = 0u;   // both counter arrays
    __syncthreads();

    auto flush = [&](uint32_t m) {
        const uint32_t len = tmpl_off[m + 1] - tmpl_off[m];
        uint32_t* const col_out = columns + (size_t)col_off[m] * 6u;
        uint32_t* const slot_out = slots + ((size_t)col_off[m] + m) * 5u;
        for (uint32_t k = lane; k < len * 6u; k += 64u) {
            const uint32_t v = acc_col[k];
            if (v) { atomicAdd(col_out + k, v); acc_col[k] = 0u; }
        }
        for (uint32_t k = lane; k < (len + 1u) * 5u; k += 64u) {
            const uint32_t v = acc_slot[k];
            if (v) { atomicAdd(slot_out + k, v); acc_slot[k] = 0u; }
        }
        __syncthreads();
    };

    const uint32_t first = (uint32_t)((uint64_t)blockIdx.x * n_blocks / gridDim.x), end = (uint32_t)((uint64_t)(blockIdx.x + 1u) * n_blocks / gridDim.x);
    uint32_t cur_m = 0xFFFFFFFFu;
    for (uint32_t b = first; b < end; ++b) {
        const ClPileupBlock blk = blocks[b];
        const bool minus = blk.monomer >= M;
        const uint32_t m = minus ? blk.monomer - M : blk.monomer, a0 = tmpl_off[blk.monomer], L = tmpl_off[blk.monomer + 1] - a0, n = blk.n;
        if (m != cur_m) {
            if (cur_m != 0xFFFFFFFFu) flush(cur_m);
            cur_m = m;
        }
        // ---- the block's bases, the lane's template columns, row 0 -----------------------------------------------------------------------------
        for (uint32_t i = lane; i < n; i += 64u) xs[i] = (uint8_t)base_code(text[blk.text_off + i]);
        for (uint32_t j = lane; j <= L; j += 64u) slotcode[j] = (uint8_t)kNoBase;
        uint32_t tb[R];
        int32_t h[R];
#pragma unroll
        for (int c = 0; c < R; ++c) {
            const uint32_t j0 = lane * R + c;   // column j0 + 1
            tb[c] = j0 < L ? codes[a0 + j0] : 5u;
            h[c] = (int32_t)(j0 + 1u) * sc.deletion;
        }
        int32_t last = h[R - 1], left_cur = (int32_t)(lane * R) * sc.deletion, left_prev = left_cur;
        __syncthreads();
        // ---- the wavefront: step s, lane t: row s - t + 1 --------------------------------------------------------------------------------------
        const uint32_t last_lane = (L - 1u) / R, steps = n ? n + last_lane : 0u;
        for (uint32_t s = 0; s < steps; ++s) {
            const int32_t recv = __shfl_up(last, 1, 64);
            left_prev = left_cur;
            left_cur = recv;
            const int32_t i = (int32_t)s - (int32_t)lane + 1;
            const bool active = i >= 1 && i <= (int32_t)n;
            const uint32_t xb = active ? xs[i - 1] : 4u;
            int32_t diag = lane ? left_prev : (i - 1) * sc.insertion, left = lane ? left_cur : i * sc.insertion;
            uint32_t word = 0;
            int32_t g[R];
#pragma unroll
            for (int c = 0; c < R; ++c) {
                const int32_t a = diag + (xb == tb[c] ? sc.match : sc.mismatch), u = h[c] + sc.insertion, d = left + sc.deletion;
                const int32_t best = max(a, max(u, d));
                word |= (a == best ? 0u : u == best ? 1u : 2u) << (2 * c);
                diag = h[c];
                left = best;
                g[c] = best;
            }
            if (active) {
#pragma unroll
                for (int c = 0; c < R; ++c) h[c] = g[c];
                last = g[R - 1];
                dirs[(uint32_t)(i - 1) * 64u + lane] = (Word)word;
            }
        }
        int32_t mine = h[0];
#pragma unroll
        for (int c = 1; c < R; ++c) mine = (L - 1u) % R == (uint32_t)c ? h[c] : mine;
        const int32_t score = __shfl(mine, (int)last_lane, 64);
        if (lane == 0) scores[b] = score;
        if (!LdsBits) __threadfence_block();
        __syncthreads();
        // ---- the walk back, the same in every lane -------------------------------------------------------------------------------------------------
        uint32_t i = n, j = L;
        while (i | j) {
            uint32_t dir;
            if (i == 0) dir = 2u;
            else if (j == 0) dir = 1u;
            else dir = ((uint32_t)dirs[(i - 1u) * 64u + (j - 1u) / R] >> (2u * ((j - 1u) % R))) & 3u;
            if (dir == 0u) {
                colcode[j - 1u] = xs[i - 1u];
                --i, --j;
            } else if (dir == 1u) {
                if (!minus || slotcode[j] == kNoBase) slotcode[j] = xs[i - 1u];   // +: the last one met is the first in sequence order
                --i;
            } else {
                colcode[j - 1u] = 5u;
                --j;
            }
        }
        __syncthreads();
        // ---- the counts of the forward template --------------------------------------------------------------------------------------------------
        for (uint32_t c = lane; c < L; c += 64u) {
            const uint32_t code = colcode[c];
            ++acc_col[(minus ? L - 1u - c : c) * 6u + (minus && code < 4u ? 3u - code : code)];
        }
        for (uint32_t c = lane; c <= L; c += 64u) {
            const uint32_t code = slotcode[c];
            if (code != kNoBase) ++acc_slot[(minus ? L - c : c) * 5u + (minus && code < 4u ? 3u - code : code)];
        }
        __syncthreads();
    }
    if (cur_m != 0xFFFFFFFFu) flush(cur_m);
}

constexpr int kCellChoices[6] = {1, 2, 3, 4, 8, 16};

template <int R>
hipError_t launch(bool lds_bits, dim3 grid, uint32_t lds_bytes, hipStream_t s, const uint8_t* text, const ClPileupBlock* blocks, uint32_t n_blocks, const uint8_t* codes,
                  const uint32_t* tmpl_off, uint32_t M, const uint32_t* col_off, PileupScores sc, uint32_t Lmax, uint32_t n_max, void* slab, uint32_t* columns,
                  uint32_t* slots, int32_t* scores) {
    using Word = typename DirWord<R>::type;
    if (lds_bits)
        hipLaunchKernelGGL((monomer_pileup_kernel<R, true>), grid, dim3(64), lds_bytes, s, text, blocks, n_blocks, codes, tmpl_off, M, col_off, sc, Lmax, n_max, (Word*)nullptr,
                           columns, slots, scores);
    else
        hipLaunchKernelGGL((monomer_pileup_kernel<R, false>), grid, dim3(64), lds_bytes, s, text, blocks, n_blocks, codes, tmpl_off, M, col_off, sc, Lmax, n_max, (Word*)slab,
                           columns, slots, scores);
    return hipGetLastError();
}

}  // namespace

int cl_monomer_pileup_device(cl_context* ctx, const char* const* seqs, const uint64_t* lens, uint64_t n, const std::vector<uint8_t>& codes,
                             const std::vector<uint32_t>& tmpl_off, uint32_t M, const cl_monomers_params* p, const std::vector<ClPileupBlock>& blocks, uint32_t* columns,
                             size_t n_columns, uint32_t* slots, size_t n_slots, std::vector<int32_t>& scores, float* align_ms, float* count_ms) {
    hipStream_t s = ctx->stream;
    int rc;
    const uint32_t U = (uint32_t)blocks.size();   // < 2^31 (checked by the caller)
    scores.assign(U, 0);
    if (U == 0) return CL_OK;   // the counts stay zero
    uint32_t Lmax = 0, n_max = 1;
    std::vector<uint32_t> col_off(M + 1, 0);
    for (uint32_t m = 0; m < M; ++m) {
        col_off[m + 1] = col_off[m] + (tmpl_off[m + 1] - tmpl_off[m]);
        Lmax = std::max(Lmax, tmpl_off[m + 1] - tmpl_off[m]);
    }
    for (const ClPileupBlock& b : blocks) n_max = std::max(n_max, b.n);
    // the cells a lane holds: the fewest that cover the longest template, or what CL_MONOMER_PILEUP_CELLS names if that covers it (tests)
    int R = 0;
    const char* forced = getenv("CL_MONOMER_PILEUP_CELLS");
    for (int k = 5; k >= 0; --k)
        if ((uint32_t)kCellChoices[k] * 64u >= Lmax) R = kCellChoices[k];
    if (forced)
        for (int k = 0; k < 6; ++k)
            if (atoi(forced) == kCellChoices[k] && (uint32_t)kCellChoices[k] * 64u >= Lmax) R = kCellChoices[k];
    if (!R) { cl_set_error(ctx, "templates: no kernel holds a template of %u bases", Lmax); return CL_ERR_INVALID_ARGUMENT; }
    const uint32_t dir_bytes = R <= 4 ? 1u : R == 8 ? 2u : 4u;
    // the direction bits: LDS if one wave's share fits the budget, or as CL_MONOMER_PILEUP_BITS says (lds only where it fits)
    bool lds_bits = pileup_layout(Lmax, n_max, dir_bytes).words * 4u <= kLdsBudget;
    if (const char* where = getenv("CL_MONOMER_PILEUP_BITS"))
        if (!strcmp(where, "global")) lds_bits = false;
    const uint32_t lds_bytes = pileup_layout(Lmax, n_max, lds_bits ? dir_bytes : 0u).words * 4u;
    if (lds_bytes > kLdsBudget) { cl_set_error(ctx, "templates: the counters of a template of %u bases do not fit the LDS", Lmax); return CL_ERR_INVALID_ARGUMENT; }
    int n_cu = 0;
    HIP_TRY(ctx, hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, ctx->device));
    const uint32_t per_cu = std::max(1u, std::min(kMaxWavesPerCu, kLdsPerCu / lds_bytes));
    uint32_t grid = std::min(U, (uint32_t)std::max(n_cu, 1) * per_cu);
    const size_t slab_wave = (size_t)n_max * 64u * dir_bytes;
    if (!lds_bits) grid = (uint32_t)std::max<size_t>(1, std::min<size_t>(grid, kMaxSlabBytes / slab_wave));

    std::vector<uint64_t> h_start(n + 1, 0);
    for (uint64_t i = 0; i < n; ++i) h_start[i + 1] = h_start[i] + lens[i];
    hipEvent_t ev[4];
    for (auto& e : ev) HIP_TRY(ctx, hipEventCreate(&e));
    struct Events { hipEvent_t* e; ~Events() { for (int i = 0; i < 4; ++i) (void)hipEventDestroy(e[i]); } } events{ev};

    ScopedBuf<uint8_t> text, codes_dev, slab;
    ScopedBuf<ClPileupBlock> blocks_dev;
    ScopedBuf<uint32_t> tmpl_off_dev, col_off_dev, counts;   // counts: the columns' counters, then the slots'
    ScopedBuf<int32_t> scores_dev;
    if ((rc = text.alloc(ctx, h_start[n])) || (rc = codes_dev.alloc(ctx, codes.size())) || (rc = blocks_dev.alloc(ctx, U)) || (rc = tmpl_off_dev.alloc(ctx, tmpl_off.size())) ||
        (rc = col_off_dev.alloc(ctx, col_off.size())) || (rc = counts.alloc(ctx, n_columns + n_slots)) || (rc = scores_dev.alloc(ctx, U)) ||
        (rc = slab.alloc(ctx, lds_bits ? 0 : slab_wave * grid)))
        return rc;
    for (uint64_t i = 0; i < n; ++i)
        if (lens[i]) HIP_TRY(ctx, hipMemcpyAsync(text.p + h_start[i], seqs[i], lens[i], hipMemcpyHostToDevice, s));
    HIP_TRY(ctx, hipMemcpyAsync(codes_dev.p, codes.data(), codes.size(), hipMemcpyHostToDevice, s));
    HIP_TRY(ctx, hipMemcpyAsync(blocks_dev.p, blocks.data(), (size_t)U * sizeof(ClPileupBlock), hipMemcpyHostToDevice, s));
    HIP_TRY(ctx, hipMemcpyAsync(tmpl_off_dev.p, tmpl_off.data(), tmpl_off.size() * sizeof(uint32_t), hipMemcpyHostToDevice, s));
    HIP_TRY(ctx, hipMemcpyAsync(col_off_dev.p, col_off.data(), col_off.size() * sizeof(uint32_t), hipMemcpyHostToDevice, s));
    HIP_TRY(ctx, hipEventRecord(ev[0], s));
    HIP_TRY(ctx, hipMemsetAsync(counts.p, 0, (n_columns + n_slots) * sizeof(uint32_t), s));
    HIP_TRY(ctx, hipEventRecord(ev[1], s));
    const PileupScores sc{p->match, p->mismatch, p->insertion, p->deletion};
    const dim3 g(grid);
    hipError_t e;
    switch (R) {
    case 1: e = launch<1>(lds_bits, g, lds_bytes, s, text.p, blocks_dev.p, U, codes_dev.p, tmpl_off_dev.p, M, col_off_dev.p, sc, Lmax, n_max, slab.p, counts.p, counts.p + n_columns, scores_dev.p); break;
    case 2: e = launch<2>(lds_bits, g, lds_bytes, s, text.p, blocks_dev.p, U, codes_dev.p, tmpl_off_dev.p, M, col_off_dev.p, sc, Lmax, n_max, slab.p, counts.p, counts.p + n_columns, scores_dev.p); break;
    case 3: e = launch<3>(lds_bits, g, lds_bytes, s, text.p, blocks_dev.p, U, codes_dev.p, tmpl_off_dev.p, M, col_off_dev.p, sc, Lmax, n_max, slab.p, counts.p, counts.p + n_columns, scores_dev.p); break;
    case 4: e = launch<4>(lds_bits, g, lds_bytes, s, text.p, blocks_dev.p, U, codes_dev.p, tmpl_off_dev.p, M, col_off_dev.p, sc, Lmax, n_max, slab.p, counts.p, counts.p + n_columns, scores_dev.p); break;
    case 8: e = launch<8>(lds_bits, g, lds_bytes, s, text.p, blocks_dev.p, U, codes_dev.p, tmpl_off_dev.p, M, col_off_dev.p, sc, Lmax, n_max, slab.p, counts.p, counts.p + n_columns, scores_dev.p); break;
    default: e = launch<16>(lds_bits, g, lds_bytes, s, text.p, blocks_dev.p, U, codes_dev.p, tmpl_off_dev.p, M, col_off_dev.p, sc, Lmax, n_max, slab.p, counts.p, counts.p + n_columns, scores_dev.p); break;
    }
    HIP_TRY(ctx, e);
    HIP_TRY(ctx, hipEventRecord(ev[2], s));
    HIP_TRY(ctx, hipMemcpyAsync(columns, counts.p, n_columns * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(ctx, hipMemcpyAsync(slots, counts.p + n_columns, n_slots * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(ctx, hipMemcpyAsync(scores.data(), scores_dev.p, (size_t)U * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(ctx, hipEventRecord(ev[3], s));
    HIP_TRY(ctx, hipStreamSynchronize(s));
    float clear_ms = 0.f, fetch_ms = 0.f;
    if (align_ms) (void)hipEventElapsedTime(align_ms, ev[1], ev[2]);
    (void)hipEventElapsedTime(&clear_ms, ev[0], ev[1]);
    (void)hipEventElapsedTime(&fetch_ms, ev[2], ev[3]);
    if (count_ms) *count_ms = clear_ms + fetch_ms;
    return CL_OK;
}
