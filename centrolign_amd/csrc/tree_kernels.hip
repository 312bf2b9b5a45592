// tree_kernels.hip — exact k-mer count spectra of many sequences and Σ_x min(c_i(x), c_j(x)) of every pair, the device half of
// cl_kmer_distances_compute (cl_tree_api.cpp; the reference has no counterpart: it takes its guide tree from outside).
//
//   spectra  per group of sequences: one key per text position ((sequence in group) << 2k | forward-strand k-mer, first base most significant)
//            and a flag for the windows that are k-mers, a scan + compaction of the flagged keys, one stable radix sort over the bits in use
//            (cl_radix.h), head flags + scan, and a compaction into distinct (k-mer, count) lists, every sequence's list contiguous and
//            sorted.  The same key / head-flag / scan pattern as the suffix rounds of match_kernels.hip.  Groups: the sequence index has to
//            fit beside the 2k k-mer bits in 64, and a group's positions in the 32-bit counts of cl_radix.h; a sequence is never split, and
//            a sequence's list does not depend on the group it was built in.
//   pairs    every pair i < j: the merge path of the two sorted lists cut into tiles of kPairTile merged items, one workgroup per
//            (pair, tile).  A tile's two diagonal splits come from a wave-wide 64-ary search (log64 of the list length dependent reads),
//            its part of list j goes to LDS, and every element of list i in the tile looks its key up there.  With list i first on equal
//            keys, the equal key of A[x] is B[#B < A[x]], which lies in the tile's B range or is the first B element past it: the LDS copy
//            holds that one more element, so a key whose two copies fall on either side of a tile edge is counted once, by A's tile.
//            Tiles add their integer sums into the pair's 64-bit total with one atomic each: order-free, so the result is deterministic.
// Traffic of the pair phase: (N - 1) · Σ_i |distinct_i| · 12 B (every list is read once per partner, keys and counts).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "cl_internal.hpp"
#include "cl_radix.h"
#include "kmer_code.h"

namespace {

constexpr uint32_t kBlock = 256;
constexpr uint32_t kPairTile = 2048;       // merged items per pair tile ("Guide tree inference"; tests/test_gpu_tree_infer.py aims at it)
constexpr uint64_t kGroupText = 1ull << 30; // text positions per spectra group (beyond that a sequence forms a group of its own)

// position p of the group's text: key = (sequence in group) << 2k | k-mer; flag = the window [p, p + k) lies in one sequence and holds only ACGTacgt
__global__ void __launch_bounds__(kBlock) kmer_keys_kernel(const uint8_t* __restrict__ text, uint32_t n_text, const uint64_t* __restrict__ seq_start,
                                                           uint32_t n_seq, uint32_t k, uint64_t* __restrict__ key, uint32_t* __restrict__ flag) {
    const uint32_t p = blockIdx.x * kBlock + threadIdx.x;
    if (p >= n_text) return;
    uint32_t lo = 0, hi = n_seq;   // the sequence of p: largest s with seq_start[s] <= p
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
    key[p] = ((uint64_t)lo << (2 * k)) | (ok ? kmer : 0ull);
    flag[p] = ok;
}

// the flagged keys, in text order, to the front of key_out (pos = inclusive scan of the flags)
__global__ void __launch_bounds__(kBlock) compact_keys_kernel(const uint64_t* __restrict__ key, const uint32_t* __restrict__ flag, const uint32_t* __restrict__ pos,
                                                              uint32_t n_text, uint64_t* __restrict__ key_out) {
    const uint32_t p = blockIdx.x * kBlock + threadIdx.x;
    if (p >= n_text || !flag[p]) return;
    key_out[pos[p] - 1] = key[p];
}

__global__ void __launch_bounds__(kBlock) head_flags_kernel(const uint64_t* __restrict__ key, uint32_t m, uint32_t* __restrict__ head) {
    const uint32_t j = blockIdx.x * kBlock + threadIdx.x;
    if (j >= m) return;
    head[j] = (j == 0 || key[j] != key[j - 1]) ? 1u : 0u;
}

// distinct key r (0-based) of the group: its k-mer bits, and where its run of equal keys starts
__global__ void __launch_bounds__(kBlock) distinct_kernel(const uint64_t* __restrict__ key, const uint32_t* __restrict__ head, const uint32_t* __restrict__ rank,
                                                          uint32_t m, uint64_t kmer_mask, uint64_t* __restrict__ dkey, uint32_t* __restrict__ dstart) {
    const uint32_t j = blockIdx.x * kBlock + threadIdx.x;
    if (j >= m || !head[j]) return;
    const uint32_t r = rank[j] - 1u;
    dkey[r] = key[j] & kmer_mask;
    dstart[r] = j;
}

__global__ void __launch_bounds__(kBlock) distinct_count_kernel(const uint32_t* __restrict__ dstart, uint32_t n_distinct, uint32_t m, uint32_t* __restrict__ dcnt) {
    const uint32_t r = blockIdx.x * kBlock + threadIdx.x;
    if (r >= n_distinct) return;
    dcnt[r] = (r + 1 < n_distinct ? dstart[r + 1] : m) - dstart[r];
}

// s = 0 .. n_seq: kpos[s] = first sorted key of sequence s (its k-mers: kpos[s] .. kpos[s + 1]), doff[s] = distinct keys before it
__global__ void seq_bounds_kernel(const uint64_t* __restrict__ key, uint32_t m, const uint32_t* __restrict__ rank, uint32_t n_seq, uint32_t shift,
                                  uint64_t* __restrict__ kpos, uint64_t* __restrict__ doff) {
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s > n_seq) return;
    uint32_t lo = 0, hi = m;
    if (s < n_seq) {
        const uint64_t want = (uint64_t)s << shift;
        while (lo < hi) {
            const uint32_t mid = lo + (hi - lo) / 2;
            if (key[mid] < want) lo = mid + 1; else hi = mid;
        }
    } else {
        lo = m;
    }
    kpos[s] = lo;
    doff[s] = lo ? rank[lo - 1] : 0u;
}

// the merge-path split of diagonal d (list A first on equal keys): the number of A elements among the first d merged items.  One wave, 64 probes
// per step: the probes below the split are a prefix of the lanes, and the next range lies between the last of them and the first above.
__device__ uint64_t merge_split(const uint64_t* __restrict__ a, uint64_t na, const uint64_t* __restrict__ b, uint64_t nb, uint64_t d) {
    const uint32_t lane = threadIdx.x & 63u;
    uint64_t lo = d > nb ? d - nb : 0, hi = d < na ? d : na;
    while (lo < hi) {
        const uint64_t step = (hi - lo + 63) / 64, probe = lo + lane * step;
        const bool below = probe < hi && a[probe] <= b[d - 1 - probe];
        const uint32_t cnt = (uint32_t)__popcll(__ballot(below));
        const uint64_t new_lo = cnt ? lo + (cnt - 1) * step + 1 : lo, cap = lo + cnt * step;
        hi = cap < hi ? cap : hi;
        lo = new_lo;
    }
    return lo;
}

__global__ void __launch_bounds__(kBlock) pair_shared_kernel(const uint64_t* __restrict__ dkey, const uint32_t* __restrict__ dcnt, const uint64_t* __restrict__ doff,
                                                             const uint32_t* __restrict__ pair_a, const uint32_t* __restrict__ pair_b,
                                                             const uint64_t* __restrict__ tile_off, uint32_t n_pairs, uint64_t n_tiles,
                                                             unsigned long long* __restrict__ shared) {
    __shared__ uint64_t sb[kPairTile + 1];
    __shared__ uint64_t split[2];
    __shared__ unsigned long long part[kBlock / 64];
    const uint32_t tid = threadIdx.x, wave = tid >> 6, lane = tid & 63u;
    for (uint64_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
        uint32_t lo = 0, hi = n_pairs;   // the pair of tile t: largest p with tile_off[p] <= t
        while (hi - lo > 1) {
            const uint32_t mid = (lo + hi) / 2;
            if (tile_off[mid] <= t) lo = mid; else hi = mid;
        }
        const uint32_t p = lo, ia = pair_a[p], ib = pair_b[p];
        const uint64_t* A = dkey + doff[ia];
        const uint64_t* B = dkey + doff[ib];
        const uint32_t* cA = dcnt + doff[ia];
        const uint32_t* cB = dcnt + doff[ib];
        const uint64_t na = doff[ia + 1] - doff[ia], nb = doff[ib + 1] - doff[ib];
        const uint64_t d0 = (t - tile_off[p]) * kPairTile, d1 = d0 + kPairTile < na + nb ? d0 + kPairTile : na + nb;
        if (wave < 2) {
            const uint64_t i = merge_split(A, na, B, nb, wave ? d1 : d0);
            if (lane == 0) split[wave] = i;
        }
        __syncthreads();
        const uint64_t i0 = split[0], i1 = split[1], j0 = d0 - i0, j1 = d1 - i1;
        const uint32_t nbl = (uint32_t)((j1 < nb ? j1 + 1 : nb) - j0);   // B[j0 .. min(j1, nb - 1)]: at most kPairTile + 1
        for (uint32_t x = tid; x < nbl; x += kBlock) sb[x] = B[j0 + x];
        __syncthreads();
        unsigned long long sum = 0;
        for (uint64_t x = i0 + tid; x < i1; x += kBlock) {
            const uint64_t key = A[x];
            uint32_t l = 0, h = nbl;
            while (l < h) {
                const uint32_t mid = (l + h) / 2;
                if (sb[mid] < key) l = mid + 1; else h = mid;
            }
            if (l < nbl && sb[l] == key) {
                const uint32_t ca = cA[x], cb = cB[j0 + l];
                sum += ca < cb ? ca : cb;
            }
        }
        for (uint32_t off = 32; off; off >>= 1) sum += __shfl_xor(sum, off, 64);
        if (lane == 0) part[wave] = sum;
        __syncthreads();
        if (tid == 0) {
            unsigned long long s = 0;
            for (uint32_t w = 0; w < kBlock / 64; ++w) s += part[w];
            if (s) atomicAdd(&shared[p], s);
        }
        __syncthreads();   // (sb, split and part are reused by the next tile)
    }
}

}  // namespace

int cl_kmer_shared_counts(cl_context* ctx, const char* const* seqs, const uint64_t* lens, uint64_t n, int k, uint64_t* total, uint64_t* shared,
                          float* spectra_ms, float* pairs_ms) {
    hipStream_t s = ctx->stream;
    int rc;
    // groups of consecutive sequences: the sequence index beside the 2k k-mer bits, the positions within kGroupText (or one sequence alone)
    std::vector<uint64_t> group_first{0};
    uint64_t max_text = 0;
    {
        uint64_t text = 0;
        for (uint64_t i = 0; i < n; ++i) {
            if (lens[i] >= 0xFFFFFFFFull) { cl_set_error(ctx, "sequence %llu is too long for a k-mer spectrum (%llu bases)", (unsigned long long)i, (unsigned long long)lens[i]); return CL_ERR_INVALID_ARGUMENT; }
            const uint64_t g = i - group_first.back();
            if (g > 0 && (2u * k + bits_for(g) > 64 || text + lens[i] > kGroupText)) {
                group_first.push_back(i);
                text = 0;
            }
            text += lens[i];
            max_text = std::max(max_text, text);
        }
        group_first.push_back(n);
    }
    DevBuf<uint8_t> text;
    DevBuf<uint64_t> key, key_c, seq_start, kpos, doff_dev, dkey_all, tile_off;
    DevBuf<uint32_t> flag, pos, dstart, dcnt_all, pair_a, pair_b;
    DevBuf<unsigned long long> pair_sum;
    DevBuf<char> temp;
    struct Release {
        std::vector<std::function<void()>> f;
        ~Release() { for (auto& x : f) x(); }
    } release;
    release.f = {[&] { text.release(); }, [&] { key.release(); }, [&] { key_c.release(); }, [&] { seq_start.release(); }, [&] { kpos.release(); },
                 [&] { doff_dev.release(); }, [&] { dkey_all.release(); }, [&] { tile_off.release(); }, [&] { flag.release(); },
                 [&] { pos.release(); }, [&] { dstart.release(); }, [&] { dcnt_all.release(); }, [&] { pair_a.release(); }, [&] { pair_b.release(); },
                 [&] { pair_sum.release(); }, [&] { temp.release(); }};
    uint64_t all_text = 0;
    for (uint64_t i = 0; i < n; ++i) all_text += lens[i];
    // the distinct lists of all sequences: at most one entry per k-mer window
    if ((rc = text.alloc(ctx, max_text)) || (rc = key.alloc(ctx, max_text)) || (rc = key_c.alloc(ctx, max_text)) || (rc = flag.alloc(ctx, max_text)) ||
        (rc = pos.alloc(ctx, max_text)) || (rc = dstart.alloc(ctx, max_text)) || (rc = dkey_all.alloc(ctx, all_text)) || (rc = dcnt_all.alloc(ctx, all_text)) ||
        (rc = seq_start.alloc(ctx, n + 1)) || (rc = kpos.alloc(ctx, n + 1)) || (rc = doff_dev.alloc(ctx, n + 1)))
        return rc;
    {
        const size_t sort_bytes = clradix::sort_temp_bytes<uint64_t>(max_text ? max_text : 1), scan_bytes = clradix::scan_temp_bytes(max_text ? max_text : 1);
        if ((rc = temp.alloc(ctx, std::max(sort_bytes, scan_bytes)))) return rc;
    }
    hipEvent_t ev[3];
    for (auto& e : ev) HIP_TRY(ctx, hipEventCreate(&e));
    struct Events { hipEvent_t* e; ~Events() { for (int i = 0; i < 3; ++i) (void)hipEventDestroy(e[i]); } } events{ev};

    std::vector<uint64_t> doff(n + 1, 0);   // where every sequence's distinct list starts in dkey_all / dcnt_all
    std::vector<uint64_t> h_start, h_kpos, h_doff;
    uint64_t distinct_base = 0;
    HIP_TRY(ctx, hipEventRecord(ev[0], s));
    for (size_t gi = 0; gi + 1 < group_first.size(); ++gi) {
        const uint64_t first = group_first[gi], g = group_first[gi + 1] - first;
        h_start.assign(1, 0);
        for (uint64_t i = 0; i < g; ++i) {
            if (lens[first + i]) HIP_TRY(ctx, hipMemcpyAsync(text.p + h_start.back(), seqs[first + i], lens[first + i], hipMemcpyHostToDevice, s));
            h_start.push_back(h_start.back() + lens[first + i]);
        }
        const uint32_t n_text = (uint32_t)h_start.back();
        HIP_TRY(ctx, hipMemcpyAsync(seq_start.p, h_start.data(), (g + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, s));
        uint32_t m = 0;
        if (n_text) {
            const dim3 grid((n_text + kBlock - 1) / kBlock);
            hipLaunchKernelGGL(kmer_keys_kernel, grid, dim3(kBlock), 0, s, text.p, n_text, seq_start.p, (uint32_t)g, (uint32_t)k, key.p, flag.p);
            HIP_TRY(ctx, clradix::inclusive_sum(temp.p, temp.n, flag.p, pos.p, n_text, s));
            HIP_TRY(ctx, hipMemcpyAsync(&m, pos.p + (n_text - 1), sizeof(uint32_t), hipMemcpyDeviceToHost, s));
            hipLaunchKernelGGL(compact_keys_kernel, grid, dim3(kBlock), 0, s, key.p, flag.p, pos.p, n_text, key_c.p);
            HIP_TRY(ctx, hipStreamSynchronize(s));
        }
        h_kpos.assign(g + 1, 0);
        h_doff.assign(g + 1, 0);
        if (m) {
            const dim3 grid((m + kBlock - 1) / kBlock);
            // sorted keys -> key (the values ride along unused: pos in, flag out)
            const unsigned end_bit = 2u * k + bits_for(g - 1);
            HIP_TRY(ctx, clradix::sort_pairs<uint64_t>(temp.p, temp.n, key_c.p, key.p, pos.p, flag.p, m, 0u, end_bit, s));
            hipLaunchKernelGGL(head_flags_kernel, grid, dim3(kBlock), 0, s, key.p, m, flag.p);
            HIP_TRY(ctx, clradix::inclusive_sum(temp.p, temp.n, flag.p, pos.p, m, s));
            const uint64_t kmer_mask = (1ull << (2 * k)) - 1ull;
            hipLaunchKernelGGL(distinct_kernel, grid, dim3(kBlock), 0, s, key.p, flag.p, pos.p, m, kmer_mask, dkey_all.p + distinct_base, dstart.p);
            hipLaunchKernelGGL(seq_bounds_kernel, dim3((uint32_t)(g + 1 + 63) / 64), dim3(64), 0, s, key.p, m, pos.p, (uint32_t)g, 2u * k, kpos.p, doff_dev.p);
            HIP_TRY(ctx, hipGetLastError());
            HIP_TRY(ctx, hipMemcpyAsync(h_kpos.data(), kpos.p, (g + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
            HIP_TRY(ctx, hipMemcpyAsync(h_doff.data(), doff_dev.p, (g + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
            HIP_TRY(ctx, hipStreamSynchronize(s));
            const uint32_t n_distinct = (uint32_t)h_doff[g];
            hipLaunchKernelGGL(distinct_count_kernel, dim3((n_distinct + kBlock - 1) / kBlock), dim3(kBlock), 0, s, dstart.p, n_distinct, m, dcnt_all.p + distinct_base);
            HIP_TRY(ctx, hipGetLastError());
        }
        for (uint64_t i = 0; i < g; ++i) {
            total[first + i] = h_kpos[i + 1] - h_kpos[i];
            doff[first + i] = distinct_base + h_doff[i];
        }
        distinct_base += h_doff[g];
        doff[first + g] = distinct_base;
        HIP_TRY(ctx, hipStreamSynchronize(s));   // (h_start is refilled for the next group)
    }
    HIP_TRY(ctx, hipEventRecord(ev[1], s));

    // all pairs i < j, in row order
    const uint64_t n_pairs = n * (n - 1) / 2;
    std::vector<uint32_t> pa, pb;
    std::vector<uint64_t> toff{0};
    pa.reserve(n_pairs);
    pb.reserve(n_pairs);
    toff.reserve(n_pairs + 1);
    for (uint64_t i = 0; i < n; ++i)
        for (uint64_t j = i + 1; j < n; ++j) {
            const uint64_t na = doff[i + 1] - doff[i], nb = doff[j + 1] - doff[j];
            pa.push_back((uint32_t)i);
            pb.push_back((uint32_t)j);
            toff.push_back(toff.back() + (na && nb ? (na + nb + kPairTile - 1) / kPairTile : 0));
        }
    std::vector<unsigned long long> h_sum(n_pairs, 0);
    if (toff.back()) {
        if ((rc = pair_a.upload(ctx, pa)) || (rc = pair_b.upload(ctx, pb)) || (rc = tile_off.upload(ctx, toff)) || (rc = doff_dev.upload(ctx, doff)) ||
            (rc = pair_sum.alloc(ctx, n_pairs)))
            return rc;
        HIP_TRY(ctx, hipMemsetAsync(pair_sum.p, 0, n_pairs * sizeof(unsigned long long), s));
        const uint64_t n_tiles = toff.back();
        const uint32_t grid = (uint32_t)std::min<uint64_t>(n_tiles, 16384);
        hipLaunchKernelGGL(pair_shared_kernel, dim3(grid), dim3(kBlock), 0, s, dkey_all.p, dcnt_all.p, doff_dev.p, pair_a.p, pair_b.p, tile_off.p,
                           (uint32_t)n_pairs, n_tiles, pair_sum.p);
        HIP_TRY(ctx, hipGetLastError());
        HIP_TRY(ctx, hipMemcpyAsync(h_sum.data(), pair_sum.p, n_pairs * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    }
    HIP_TRY(ctx, hipEventRecord(ev[2], s));
    HIP_TRY(ctx, hipStreamSynchronize(s));
    for (uint64_t i = 0, p = 0; i < n; ++i) {
        shared[i * n + i] = total[i];
        for (uint64_t j = i + 1; j < n; ++j, ++p) shared[i * n + j] = shared[j * n + i] = h_sum[p];
    }
    if (spectra_ms) (void)hipEventElapsedTime(spectra_ms, ev[0], ev[1]);
    if (pairs_ms) (void)hipEventElapsedTime(pairs_ms, ev[1], ev[2]);
    return CL_OK;
}
