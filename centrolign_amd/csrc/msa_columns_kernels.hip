// msa_columns_kernels.hip — the MSA as columns (cl_msa_columns_compute, cl_columns_api.cpp): one block of columns [c0, c0 + width) of the
// n_paths x n_cols matrix at a time, held in a device tile of n_paths rows of `stride` bytes (stride: the block width rounded up to 4, so
// that a row begins on a word and the last word of a row lies inside the tile; the padding bytes stay '-').  The column of every node
// (node_col) comes from the host's level pass; the host definition is cl_msa_columns_host.
//
//   msa_fill_kernel      the tile is preset to '-' by the caller; one thread per path step of the block stores its base at
//                        tile[p][col - c0].  blockIdx.y walks the paths, blockIdx.x the steps [lo[p], hi[p]) of the path that fall into the
//                        block (found on the host: a path's columns strictly increase).  Neighbouring lanes hold neighbouring steps, whose
//                        columns mostly are neighbours too.
//   msa_reduce_kernel    one thread per four adjacent columns: one 32-bit load per row (the lanes of a wave read consecutive words), five
//                        counters per column in registers, four 32-byte records written as eight 16-byte stores.  No atomics, no LDS.
//   msa_sites_kernel     <false>: every workgroup counts the flagged columns among its 256 into counts[workgroup]; <true>: with the
//                        exclusive offsets of those counts (summed on the host) every flagged column finds its place k among the block's
//                        sites — the offset, the flagged columns of the waves before (LDS), of the lanes before (ballot) — and stores its
//                        column number and, row by row, its bytes of the tile.  No workgroup waits for another.
// All results are integer counts and bytes: they do not depend on scheduling, nor on how the columns are cut into blocks.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "cl_internal.hpp"

namespace {

constexpr uint32_t kThreads = 256, kWaves = kThreads / 64;

__global__ void __launch_bounds__(kThreads) msa_fill_kernel(const uint32_t* __restrict__ path_nodes, const uint64_t* __restrict__ range, uint64_t n_paths,
                                                            const uint8_t* __restrict__ label, const uint32_t* __restrict__ node_col, uint32_t c0,
                                                            uint32_t width, uint64_t stride, char* __restrict__ tile) {
    const uint64_t t = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    for (uint64_t p = blockIdx.y; p < n_paths; p += gridDim.y) {
        const uint64_t lo = range[2 * p], hi = range[2 * p + 1];
        if (t >= hi - lo) continue;
        const uint32_t v = path_nodes[lo + t];
        const uint32_t c = node_col[v] - c0;
        const uint32_t b = label[v];
        if (c < width) tile[p * stride + c] = b == 0 ? 'A' : b == 1 ? 'C' : b == 2 ? 'G' : b == 3 ? 'T' : 'N';   // (the host has checked both)
    }
}

// the record of one column from its five counts
__device__ __forceinline__ void make_record(const uint32_t (&cnt)[5], uint32_t n_paths, uint32_t min_minor, uint32_t max_gaps, uint4& lo, uint4& hi) {
    const uint32_t gaps = n_paths - (cnt[0] + cnt[1] + cnt[2] + cnt[3] + cnt[4]);
    uint32_t best = cnt[0], consensus = 0;
#pragma unroll
    for (uint32_t k = 1; k < 5; ++k) if (cnt[k] > best) { best = cnt[k]; consensus = k; }
    if (gaps > best) consensus = 5;
    uint32_t m1 = 0, m2 = 0;   // the two largest of A, C, G, T
#pragma unroll
    for (uint32_t k = 0; k < 4; ++k) {
        const uint32_t c = cnt[k];
        m2 = c > m1 ? m1 : (c > m2 ? c : m2);
        m1 = c > m1 ? c : m1;
    }
    const uint32_t flags = (m2 >= min_minor && gaps <= max_gaps ? 1u : 0u) | (gaps > 0 ? 2u : 0u) | (cnt[4] > 0 ? 4u : 0u);
    lo = make_uint4(cnt[0], cnt[1], cnt[2], cnt[3]);
    hi = make_uint4(cnt[4], gaps, consensus, flags);
}

__global__ void __launch_bounds__(kThreads) msa_reduce_kernel(const uint32_t* __restrict__ tile_words, uint64_t n_paths, uint64_t row_words, uint32_t width,
                                                              uint32_t min_minor, uint32_t max_gaps, uint4* __restrict__ records) {
    const uint64_t q = (uint64_t)blockIdx.x * kThreads + threadIdx.x;   // columns 4q .. 4q + 3 of the block
    if (q >= row_words) return;
    uint32_t cnt[4][5] = {};
    const uint32_t* at = tile_words + q;
#pragma unroll 4
    for (uint64_t p = 0; p < n_paths; ++p, at += row_words) {
        const uint32_t w = *at;
#pragma unroll
        for (uint32_t k = 0; k < 4; ++k) {
            const uint32_t b = (w >> (8 * k)) & 0xFFu;
            cnt[k][0] += b == 'A';
            cnt[k][1] += b == 'C';
            cnt[k][2] += b == 'G';
            cnt[k][3] += b == 'T';
            cnt[k][4] += b == 'N';
        }
    }
#pragma unroll
    for (uint32_t k = 0; k < 4; ++k) {
        const uint64_t col = 4 * q + k;
        if (col >= width) break;   // the padding of the last word
        uint4 lo, hi;
        make_record(cnt[k], (uint32_t)n_paths, min_minor, max_gaps, lo, hi);
        records[2 * col] = lo;
        records[2 * col + 1] = hi;
    }
}

// flags of column blockIdx.x * 256 + threadIdx.x of the block.  kWrite false: counts[blockIdx.x] = the flagged ones among them.  kWrite true:
// flagged column j is the block's site k = offsets[blockIdx.x] + (the flagged columns before j in the workgroup): site_col[k] = c0 + j and
// site_rows[p * n_block_sites + k] = tile[p][j] for every row p
template <bool kWrite>
__global__ void __launch_bounds__(kThreads) msa_sites_kernel(const cl_msa_column* __restrict__ records, uint32_t width, uint32_t* __restrict__ counts,
                                                             const uint32_t* __restrict__ offsets, uint64_t c0, const char* __restrict__ tile, uint64_t stride,
                                                             uint64_t n_paths, uint64_t n_block_sites, uint64_t* __restrict__ site_col, char* __restrict__ site_rows) {
    __shared__ uint32_t wave_count[kWaves];
    const uint32_t j = blockIdx.x * kThreads + threadIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const bool site = j < width && (records[j].flags & 1u);
    const unsigned long long mask = __ballot(site);
    if (lane == 0) wave_count[wave] = (uint32_t)__popcll(mask);
    __syncthreads();
    if (!kWrite) {
        if (threadIdx.x == 0) {
            uint32_t n = 0;
            for (uint32_t w = 0; w < kWaves; ++w) n += wave_count[w];
            counts[blockIdx.x] = n;
        }
        return;
    }
    if (!site) return;
    uint64_t k = offsets[blockIdx.x] + (uint32_t)__popcll(mask & ((1ull << lane) - 1));
    for (uint32_t w = 0; w < wave; ++w) k += wave_count[w];
    site_col[k] = c0 + j;
    for (uint64_t p = 0; p < n_paths; ++p) site_rows[p * n_block_sites + k] = tile[p * stride + j];
}

}  // namespace

hipError_t cl_launch_msa_fill(const uint32_t* path_nodes, const uint64_t* range, uint64_t n_paths, uint64_t max_steps, const uint8_t* label,
                              const uint32_t* node_col, uint32_t c0, uint32_t width, uint64_t stride, char* tile, hipStream_t stream) {
    if (n_paths == 0 || max_steps == 0) return hipSuccess;
    const dim3 grid((uint32_t)((max_steps + kThreads - 1) / kThreads), (uint32_t)std::min<uint64_t>(n_paths, 65535));
    hipLaunchKernelGGL(msa_fill_kernel, grid, dim3(kThreads), 0, stream, path_nodes, range, n_paths, label, node_col, c0, width, stride, tile);
    return hipGetLastError();
}

hipError_t cl_launch_msa_reduce(const char* tile, uint64_t n_paths, uint64_t stride, uint32_t width, uint32_t min_minor, uint32_t max_gaps,
                                cl_msa_column* records, hipStream_t stream) {
    if (width == 0) return hipSuccess;
    const uint64_t row_words = stride / 4;
    hipLaunchKernelGGL(msa_reduce_kernel, dim3((uint32_t)((row_words + kThreads - 1) / kThreads)), dim3(kThreads), 0, stream, (const uint32_t*)tile, n_paths,
                       row_words, width, min_minor, max_gaps, (uint4*)records);
    return hipGetLastError();
}

uint32_t cl_msa_site_groups(uint32_t width) { return (width + kThreads - 1) / kThreads; }

hipError_t cl_launch_msa_sites(bool write, const cl_msa_column* records, uint32_t width, uint32_t* counts, const uint32_t* offsets, uint64_t c0,
                               const char* tile, uint64_t stride, uint64_t n_paths, uint64_t n_block_sites, uint64_t* site_col, char* site_rows,
                               hipStream_t stream) {
    if (width == 0) return hipSuccess;
    const dim3 grid(cl_msa_site_groups(width));
    if (write) hipLaunchKernelGGL(msa_sites_kernel<true>, grid, dim3(kThreads), 0, stream, records, width, counts, offsets, c0, tile, stride, n_paths, n_block_sites, site_col, site_rows);
    else hipLaunchKernelGGL(msa_sites_kernel<false>, grid, dim3(kThreads), 0, stream, records, width, counts, offsets, c0, tile, stride, n_paths, n_block_sites, site_col, site_rows);
    return hipGetLastError();
}
