// subaln_kernels.hip — the -s output of one merge: Core::emit_subalignment (src/core.cpp:424-472) writes one line per aligned pair of the merge's
// alignment, each side as (path name, step, base) of StepIndex::path_steps(node).front(), or "-\t-\t-" for a gap.  The entry point is
// cl_subalignment_text (cl_subaln_api.cpp), which adds the two '# sequence set' headers on the host.
//
// Four launches on the context's stream, nothing waits across workgroups:
//   step table   one thread per path step: key (path << 32) | step folded into a per-node u64 with a 64-bit atomicMin.  StepIndex appends the
//                steps of path 0, then path 1, ..., each in step order, so front() is the smallest key: the minimum is the reference's answer
//                for any path, cyclic or not, in whatever order the threads run.  A node on no path keeps UINT64_MAX.
//   lengths      one thread per aligned pair: the line's bytes; a workgroup's sum per 256 pairs.  A node id out of range, or on no path, is
//                reported as the smallest failing pair index.
//   offsets      one workgroup: the exclusive scan of the workgroup sums.
//   write        one thread per aligned pair again: the line's offset is its workgroup's offset plus a workgroup scan of the lengths.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "cl_internal.hpp"

namespace {

constexpr uint32_t kThreads = 256, kWaves = kThreads / 64, kScanThreads = 1024;
constexpr uint64_t kGap = ~(uint64_t)0;

__device__ __forceinline__ uint32_t n_digits(uint32_t v) {
    uint32_t d = 1;
    while (v >= 10) { v /= 10; ++d; }
    return d;
}

// bytes of one side of a line, 0 when the side is invalid
__device__ __forceinline__ uint64_t side_bytes(const ClSubalnSide& s, uint64_t node, bool& bad) {
    if (node == kGap) return 5;   // "-\t-\t-"
    if (node >= s.n_nodes) { bad = true; return 0; }
    const unsigned long long key = s.table[node];
    if (key == ~0ull) { bad = true; return 0; }
    const uint64_t p = key >> 32;
    return (s.name_off[p + 1] - s.name_off[p]) + n_digits((uint32_t)key) + 3;
}

__device__ __forceinline__ char* put_side(const ClSubalnSide& s, uint64_t node, char* out) {
    if (node == kGap) {
        out[0] = '-'; out[1] = '\t'; out[2] = '-'; out[3] = '\t'; out[4] = '-';
        return out + 5;
    }
    const unsigned long long key = s.table[node];
    const uint64_t p = key >> 32;
    uint32_t step = (uint32_t)key;
    for (uint64_t i = s.name_off[p]; i < s.name_off[p + 1]; ++i) *out++ = s.names[i];
    *out++ = '\t';
    const uint32_t nd = n_digits(step);
    for (uint32_t j = nd; j-- > 0;) { out[j] = (char)('0' + step % 10); step /= 10; }
    out += nd;
    *out++ = '\t';
    const uint8_t l = s.label[node];
    *out++ = l == 0 ? 'A' : l == 1 ? 'C' : l == 2 ? 'G' : l == 3 ? 'T' : l == 4 ? 'N' : '\0';   // decode_base (src/utility.cpp:355)
    return out;
}

__device__ __forceinline__ uint64_t line_bytes(const ClSubalnSide& s1, const ClSubalnSide& s2, const uint64_t* pairs, uint64_t k, bool& bad) {
    const uint64_t a = side_bytes(s1, pairs[2 * k], bad);
    const uint64_t b = side_bytes(s2, pairs[2 * k + 1], bad);
    return a + b + 2;
}

// exclusive prefix of v over the workgroup in thread order; total: the workgroup's sum.  lds: kWaves words (blockDim.x == kThreads)
__device__ __forceinline__ uint64_t block_exclusive(uint64_t v, uint64_t* lds, uint64_t& total) {
    const unsigned lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint64_t inc = v;
#pragma unroll
    for (unsigned d = 1; d < 64; d <<= 1) {
        const uint64_t o = (uint64_t)__shfl_up((long long)inc, d, 64);
        if (lane >= d) inc += o;
    }
    if (lane == 63) lds[wave] = inc;
    __syncthreads();
    uint64_t before = 0;
    total = 0;
    for (unsigned w = 0; w < kWaves; ++w) {
        if (w < wave) before += lds[w];
        total += lds[w];
    }
    __syncthreads();
    return before + inc - v;
}

__global__ void subaln_step_table_kernel(const uint64_t* __restrict__ path_off, uint64_t n_paths, const uint32_t* __restrict__ path_nodes,
                                         uint64_t n_nodes, unsigned long long* __restrict__ table) {
    const uint64_t n_steps = path_off[n_paths];
    for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n_steps; i += (uint64_t)gridDim.x * blockDim.x) {
        uint64_t lo = 0, hi = n_paths;   // the path holding step i: the last p with path_off[p] <= i (empty paths hold none)
        while (hi - lo > 1) {
            const uint64_t mid = (lo + hi) / 2;
            if (path_off[mid] <= i) lo = mid; else hi = mid;
        }
        const uint32_t v = path_nodes[i];
        if (v < n_nodes) atomicMin(&table[v], (unsigned long long)((lo << 32) | (i - path_off[lo])));
    }
}

__global__ __launch_bounds__(kThreads) void subaln_len_kernel(ClSubalnSide s1, ClSubalnSide s2, const uint64_t* __restrict__ pairs, uint64_t n,
                                                              uint64_t* __restrict__ block_sum, unsigned long long* __restrict__ first_bad) {
    __shared__ uint64_t lds[kWaves];
    const uint64_t k = blockIdx.x * (uint64_t)kThreads + threadIdx.x;
    bool bad = false;
    const uint64_t len = k < n ? line_bytes(s1, s2, pairs, k, bad) : 0;
    if (bad) atomicMin(first_bad, (unsigned long long)k);
    uint64_t total;
    (void)block_exclusive(len, lds, total);
    if (threadIdx.x == 0) block_sum[blockIdx.x] = total;
}

// in place: v[i] = v[0] + ... + v[i - 1] for i < n, and v[n] = the sum of all
__global__ __launch_bounds__(kScanThreads) void subaln_offsets_kernel(uint64_t* __restrict__ v, uint64_t n) {
    __shared__ uint64_t lds[kScanThreads / 64];
    const unsigned lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint64_t carry = 0;
    for (uint64_t base = 0; base < n; base += kScanThreads) {
        const uint64_t i = base + threadIdx.x;
        const uint64_t x = i < n ? v[i] : 0;
        uint64_t inc = x;
#pragma unroll
        for (unsigned d = 1; d < 64; d <<= 1) {
            const uint64_t o = (uint64_t)__shfl_up((long long)inc, d, 64);
            if (lane >= d) inc += o;
        }
        if (lane == 63) lds[wave] = inc;
        __syncthreads();
        uint64_t before = 0, total = 0;
        for (unsigned w = 0; w < kScanThreads / 64; ++w) {
            if (w < wave) before += lds[w];
            total += lds[w];
        }
        if (i < n) v[i] = carry + before + inc - x;
        carry += total;
        __syncthreads();
    }
    if (threadIdx.x == 0) v[n] = carry;
}

__global__ __launch_bounds__(kThreads) void subaln_write_kernel(ClSubalnSide s1, ClSubalnSide s2, const uint64_t* __restrict__ pairs, uint64_t n,
                                                                const uint64_t* __restrict__ block_off, char* __restrict__ text) {
    __shared__ uint64_t lds[kWaves];
    const uint64_t k = blockIdx.x * (uint64_t)kThreads + threadIdx.x;
    bool bad = false;
    const uint64_t len = k < n ? line_bytes(s1, s2, pairs, k, bad) : 0;
    uint64_t total;
    const uint64_t off = block_off[blockIdx.x] + block_exclusive(len, lds, total);
    if (k >= n || bad) return;   // (a chunk with a bad pair is never written: the host stops after the lengths)
    char* out = put_side(s1, pairs[2 * k], text + off);
    *out++ = '\t';
    out = put_side(s2, pairs[2 * k + 1], out);
    *out = '\n';
}

}  // namespace

hipError_t cl_launch_subaln_step_table(const uint64_t* path_off, uint64_t n_paths, const uint32_t* path_nodes, uint64_t n_steps, uint64_t n_nodes,
                                       unsigned long long* table, hipStream_t stream) {
    hipError_t e = hipMemsetAsync(table, 0xFF, std::max<uint64_t>(n_nodes, 1) * sizeof(unsigned long long), stream);
    if (e != hipSuccess || n_steps == 0 || n_paths == 0) return e;
    const unsigned grid = (unsigned)std::min<uint64_t>((n_steps + 255) / 256, 8192);
    hipLaunchKernelGGL(subaln_step_table_kernel, dim3(grid), dim3(256), 0, stream, path_off, n_paths, path_nodes, n_nodes, table);
    return hipGetLastError();
}

hipError_t cl_launch_subaln_lengths(const ClSubalnSide& s1, const ClSubalnSide& s2, const uint64_t* pairs, uint64_t n, uint64_t* block_off,
                                    unsigned long long* first_bad, hipStream_t stream) {
    const uint64_t blocks = (n + kThreads - 1) / kThreads;
    if (blocks) hipLaunchKernelGGL(subaln_len_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, stream, s1, s2, pairs, n, block_off, first_bad);
    hipLaunchKernelGGL(subaln_offsets_kernel, dim3(1), dim3(kScanThreads), 0, stream, block_off, blocks);
    return hipGetLastError();
}

hipError_t cl_launch_subaln_write(const ClSubalnSide& s1, const ClSubalnSide& s2, const uint64_t* pairs, uint64_t n, const uint64_t* block_off,
                                  char* text, hipStream_t stream) {
    const uint64_t blocks = (n + kThreads - 1) / kThreads;
    if (!blocks) return hipSuccess;
    hipLaunchKernelGGL(subaln_write_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, stream, s1, s2, pairs, n, block_off, text);
    return hipGetLastError();
}

uint64_t cl_subaln_pairs_per_block() { return kThreads; }
