// dotplot_kernels.hip — the device half of cl_kmer_dotplot_compute (cl_dotplot_api.cpp): the distinct k-mers of every window of
// every sequence, and for every pair of windows how many they share, thresholded on the device and returned as a sparse list in (a, b) order.
//
//   spectra  one key per text position (the 2k-bit forward-strand k-mer, a flag for the runs that are k-mers, the global window id as value), a
//            scan + compaction of the flagged positions, a stable radix sort by k-mer (cl_radix.h), head flags + scan: every position now has
//            the dense RANK of its k-mer among the call's distinct k-mers.  A second stable sort by window id alone leaves the ranks ascending
//            inside each window; head flags on (window, rank), a scan and a compaction give every window its ascending list of distinct ranks:
//            32-bit entries whatever k is.  The key / head-flag / scan pattern of tree_kernels.hip.
//   pairs    the windows a call compares form RANGES (all of them: one range; pairs = 1: one per sequence); a range of n windows is cut into
//            ceil(n / T) tile rows and the upper triangle of T x T tiles.  dotplot_tile_kernel, one workgroup per tile in a persistent loop:
//            the lists of the tile's column windows are one contiguous piece of the list array and go through LDS in chunks of kChunk entries
//            (a list longer than a chunk, or cut by a chunk edge, is met in several chunks: the counts add up); every wave takes row windows,
//            128 list elements at a time (two a lane), and looks each up in the part of every column list the chunk holds, a branch-free binary search
//            whose trip count is the same on all lanes; a 64-lane ballot + population count gives the hits, which lane 0 adds to the pair's
//            counter in LDS — a row belongs to one wave, so there are no atomics.  The integer threshold is applied at the tile's end; the
//            tile stores shared (0: not kept) per pair and the number of kept pairs per (row, tile).  Those counts are laid out in output
//            order (tile row, row, tile column), one scan turns them into offsets, and dotplot_write_kernel writes the entries: ascending
//            (a, b) without a sort and without an atomic.  Tiles are processed in batches of whole tile rows, so the per-pair array is
//            bounded (kBatchPairs) and the G x G matrix never exists.
// No floating point on the device.  LDS per workgroup: 32 KiB chunk + 16 KiB counters + 260 B offsets: three workgroups of eight waves a CU (160 KiB).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "cl_internal.hpp"
#include "cl_radix.h"
#include "kmer_code.h"

namespace {

constexpr uint32_t kBlock = 256;
constexpr uint32_t kTileBlock = 512, kTileWaves = kTileBlock / 64;   // the tile kernel: LDS allows three workgroups a CU, eight waves each hide the LDS latency of the searches
constexpr uint32_t kMaxT = 64;              // windows per side of a tile, at most
constexpr uint32_t kChunk = 8192;           // list entries of the column side in LDS at a time
constexpr uint32_t kMaxGrid = 2048;         // workgroups of the persistent tile loop
constexpr uint64_t kBatchPairs = 1u << 24;  // window pairs (tiles * T * T) per batch, unless one tile row alone holds more

// position p of the text: its k-mer, the global window its first base stands in, and whether [p, p + k) lies in one sequence and holds only ACGTacgt
__global__ void __launch_bounds__(kBlock) dotplot_keys_kernel(const uint8_t* __restrict__ text, uint32_t n_text, const uint64_t* __restrict__ seq_start,
                                                              const uint64_t* __restrict__ win_off, uint32_t n_seq, uint32_t k, uint32_t window,
                                                              uint64_t* __restrict__ key, uint32_t* __restrict__ win, uint32_t* __restrict__ flag) {
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
    win[p] = (uint32_t)(win_off[lo] + (p - seq_start[lo]) / window);
    flag[p] = ok;
}

// the flagged (key, window) pairs, in text order, to the front (pos = inclusive scan of the flags)
__global__ void __launch_bounds__(kBlock) dotplot_compact_kernel(const uint64_t* __restrict__ key, const uint32_t* __restrict__ win, const uint32_t* __restrict__ flag,
                                                                 const uint32_t* __restrict__ pos, uint32_t n_text, uint64_t* __restrict__ key_out,
                                                                 uint32_t* __restrict__ win_out) {
    const uint32_t p = blockIdx.x * kBlock + threadIdx.x;
    if (p >= n_text || !flag[p]) return;
    key_out[pos[p] - 1] = key[p];
    win_out[pos[p] - 1] = win[p];
}

__global__ void __launch_bounds__(kBlock) dotplot_kmer_heads_kernel(const uint64_t* __restrict__ key, uint32_t m, uint32_t* __restrict__ head) {
    const uint32_t j = blockIdx.x * kBlock + threadIdx.x;
    if (j >= m) return;
    head[j] = (j == 0 || key[j] != key[j - 1]) ? 1u : 0u;
}

// sorted by window, ranks ascending inside a window: the first of every (window, rank)
__global__ void __launch_bounds__(kBlock) dotplot_list_heads_kernel(const uint32_t* __restrict__ win, const uint32_t* __restrict__ rank, uint32_t m,
                                                                    uint32_t* __restrict__ head) {
    const uint32_t j = blockIdx.x * kBlock + threadIdx.x;
    if (j >= m) return;
    head[j] = (j == 0 || win[j] != win[j - 1] || rank[j] != rank[j - 1]) ? 1u : 0u;
}

__global__ void __launch_bounds__(kBlock) dotplot_list_kernel(const uint32_t* __restrict__ rank, const uint32_t* __restrict__ head, const uint32_t* __restrict__ pos,
                                                              uint32_t m, uint32_t* __restrict__ list) {
    const uint32_t j = blockIdx.x * kBlock + threadIdx.x;
    if (j >= m || !head[j]) return;
    list[pos[j] - 1] = rank[j];
}

// g = 0 .. n_windows: list_off[g] = list entries of the windows before g (pos: the inclusive scan of the list heads)
__global__ void __launch_bounds__(kBlock) dotplot_list_offsets_kernel(const uint32_t* __restrict__ win, const uint32_t* __restrict__ pos, uint32_t m, uint64_t n_windows,
                                                                      uint32_t* __restrict__ list_off) {
    const uint64_t g = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (g > n_windows) return;
    uint32_t lo = 0, hi = m;   // the first sorted position of a window >= g
    if (g < n_windows) {
        while (lo < hi) {
            const uint32_t mid = lo + (hi - lo) / 2;
            if (win[mid] < g) lo = mid + 1; else hi = mid;
        }
    } else {
        lo = m;
    }
    list_off[g] = lo ? pos[lo - 1] : 0u;
}

// A range of windows [lo, hi) whose pairs are compared, and where its tiles start in the call's tile numbering.  Tile numbering inside a range of
// R tile rows: row ti holds the tiles (ti, ti) .. (ti, R - 1), rows in order: tile row ti starts at ti * R - ti * (ti - 1) / 2.
struct TileRange { uint32_t lo, hi; uint64_t tile0; };
struct Tile { uint32_t a0, a1, b0, b1, ti, tj, width; uint64_t row_first; };   // rows [a0, a1), columns [b0, b1); width = tiles of its tile row, the first of which is row_first

__device__ __forceinline__ uint64_t tile_row_start(uint64_t ti, uint64_t R) { return ti * R - ti * (ti - 1) / 2; }   // (ti = 0: the product is 0 before the subtraction wraps)

__device__ Tile decode_tile(const TileRange* __restrict__ ranges, uint32_t n_ranges, uint64_t t, uint32_t T) {
    uint32_t lo = 0, hi = n_ranges;   // the range of tile t: largest i with tile0[i] <= t (no range is empty)
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) / 2;
        if (ranges[mid].tile0 <= t) lo = mid; else hi = mid;
    }
    const TileRange r = ranges[lo];
    const uint64_t R = ((uint64_t)(r.hi - r.lo) + T - 1) / T, local = t - r.tile0;
    uint64_t tl = 0, th = R;   // largest ti with tile_row_start(ti) <= local
    while (th - tl > 1) {
        const uint64_t mid = (tl + th) / 2;
        if (tile_row_start(mid, R) <= local) tl = mid; else th = mid;
    }
    const uint64_t row0 = tile_row_start(tl, R), tj = tl + (local - row0);
    Tile x;
    x.ti = (uint32_t)tl;
    x.tj = (uint32_t)tj;
    x.width = (uint32_t)(R - tl);
    x.row_first = r.tile0 + row0;
    x.a0 = r.lo + (uint32_t)tl * T;
    x.b0 = r.lo + (uint32_t)tj * T;
    x.a1 = (uint32_t)min((uint64_t)x.a0 + T, (uint64_t)r.hi);
    x.b1 = (uint32_t)min((uint64_t)x.b0 + T, (uint64_t)r.hi);
    return x;
}

// tiles [t_begin, t_end) of the call (whole tile rows).  shared_out[(t - t_begin) * T * T + r * T + c] = |K_a n K_b| of a = a0 + r, b = b0 + c if the
// pair is kept, otherwise 0; kept_out[(row_first - t_begin) * T + r * width + (tj - ti)] = kept pairs of row r in this tile: the order of the output.
__global__ void __launch_bounds__(kTileBlock) dotplot_tile_kernel(const uint32_t* __restrict__ list, const uint32_t* __restrict__ list_off,
                                                              const TileRange* __restrict__ ranges, uint32_t n_ranges, uint64_t t_begin, uint64_t t_end, uint32_t T,
                                                              unsigned long long q, uint32_t* __restrict__ shared_out, uint32_t* __restrict__ kept_out) {
    __shared__ uint32_t s_list[kChunk];
    __shared__ uint32_t s_acc[kMaxT * kMaxT];
    __shared__ uint32_t s_off[kMaxT + 1];
    const uint32_t tid = threadIdx.x, wave = tid >> 6, lane = tid & 63u;
    for (uint64_t t = t_begin + blockIdx.x; t < t_end; t += gridDim.x) {
        const Tile x = decode_tile(ranges, n_ranges, t, T);
        const uint32_t na = x.a1 - x.a0, nb = x.b1 - x.b0;
        const bool diagonal = x.ti == x.tj;
        for (uint32_t i = tid; i < T * T; i += kTileBlock) s_acc[i] = 0;
        if (tid <= nb) s_off[tid] = list_off[x.b0 + tid];
        __syncthreads();
        const uint32_t col_begin = s_off[0], col_end = s_off[nb];
        for (uint32_t c0 = col_begin; c0 < col_end; c0 += kChunk) {
            const uint32_t c1 = min(col_end, c0 + kChunk);   // (col_end <= 2^30: no wrap)
            __syncthreads();   // (the chunk before has been read)
            for (uint32_t i = tid; i < c1 - c0; i += kTileBlock) s_list[i] = list[c0 + i];
            __syncthreads();
            for (uint32_t r = wave; r < na; r += kTileWaves) {
                const uint32_t a_begin = list_off[x.a0 + r], a_end = list_off[x.a0 + r + 1];
                const uint32_t c_first = diagonal ? r : 0u;   // b >= a
                for (uint32_t i = a_begin; i < a_end; i += 128u) {   // two keys a lane: two independent searches hide each other's LDS latency
                    const uint32_t key0 = i + lane < a_end ? list[i + lane] : 0xFFFFFFFFu;   // (ranks stay below 2^30)
                    const uint32_t key1 = i + 64u + lane < a_end ? list[i + 64u + lane] : 0xFFFFFFFFu;
                    for (uint32_t c = c_first; c < nb; ++c) {
                        const uint32_t lo = max(s_off[c], c0), hi = min(s_off[c + 1], c1);   // the part of b's list in this chunk
                        if (lo >= hi) continue;
                        uint32_t base0 = lo - c0, base1 = base0, n = hi - lo;   // the last element <= key, if there is one, lies in [base, base + n)
                        while (n > 1) {
                            const uint32_t half = n >> 1;
                            const uint32_t v0 = s_list[base0 + half], v1 = s_list[base1 + half];
                            base0 = v0 <= key0 ? base0 + half : base0;
                            base1 = v1 <= key1 ? base1 + half : base1;
                            n -= half;
                        }
                        const uint32_t v0 = s_list[base0], v1 = s_list[base1];
                        const uint32_t hits = (uint32_t)__popcll(__ballot(v0 == key0)) + (uint32_t)__popcll(__ballot(v1 == key1));
                        if (lane == 0 && hits) s_acc[r * T + c] += hits;
                    }
                }
            }
        }
        __syncthreads();
        uint32_t* const tile_shared = shared_out + (t - t_begin) * T * T;
        uint32_t* const tile_kept = kept_out + (x.row_first - t_begin) * T + (x.tj - x.ti);
        for (uint32_t r = wave; r < T; r += kTileWaves) {
            uint32_t shared = 0;
            if (r < na && lane < nb && lane >= (diagonal ? r : 0u)) {
                const uint32_t da = list_off[x.a0 + r + 1] - list_off[x.a0 + r], db = s_off[lane + 1] - s_off[lane], denom = min(da, db);
                const uint32_t s = s_acc[r * T + lane];
                if (s >= 1u && ((unsigned long long)s << 32) >= q * denom) shared = s;
            }
            if (lane < T) tile_shared[r * T + lane] = shared;
            const uint32_t kept = (uint32_t)__popcll(__ballot(shared != 0u));
            if (lane == 0) tile_kept[(size_t)r * x.width] = kept;
        }
        __syncthreads();   // (s_acc and s_off are reused by the next tile)
    }
}

// kept_incl: the inclusive scan of kept_out.  One wave per (tile, row): the kept pairs of the row, in column order, at the row's offset
__global__ void __launch_bounds__(kTileBlock) dotplot_write_kernel(const uint32_t* __restrict__ list_off, const TileRange* __restrict__ ranges, uint32_t n_ranges,
                                                               uint64_t t_begin, uint64_t t_end, uint32_t T, const uint32_t* __restrict__ shared_in,
                                                               const uint32_t* __restrict__ kept_incl, uint4* __restrict__ entries) {
    const uint32_t tid = threadIdx.x, wave = tid >> 6, lane = tid & 63u;
    for (uint64_t t = t_begin + blockIdx.x; t < t_end; t += gridDim.x) {
        const Tile x = decode_tile(ranges, n_ranges, t, T);
        const uint32_t na = x.a1 - x.a0, nb = x.b1 - x.b0;
        const uint32_t* const tile_shared = shared_in + (t - t_begin) * T * T;
        for (uint32_t r = wave; r < na; r += kTileWaves) {
            const uint64_t at = (x.row_first - t_begin) * T + (uint64_t)r * x.width + (x.tj - x.ti);
            const uint32_t before = at ? kept_incl[at - 1] : 0u;
            const uint32_t shared = lane < nb ? tile_shared[r * T + lane] : 0u;
            const unsigned long long kept = __ballot(shared != 0u);
            if (shared) {
                const uint32_t a = x.a0 + r, b = x.b0 + lane;
                const uint32_t da = list_off[a + 1] - list_off[a], db = list_off[b + 1] - list_off[b];
                entries[before + (uint32_t)__popcll(kept & ((1ull << lane) - 1ull))] = make_uint4(a, b, shared, min(da, db));
            }
        }
    }
}

struct TileRow { uint32_t range; uint64_t first, width; };   // a tile row of a range: its first tile in the call's numbering, and how many it holds

}  // namespace

int cl_dotplot_device(cl_context* ctx, const char* const* seqs, const uint64_t* lens, uint64_t n, const uint64_t* win_off, int k, uint32_t window, int pairs,
                      uint64_t q, uint32_t tile_windows, uint32_t* distinct, std::vector<cl_dotplot_entry>& entries, float* spectra_ms, float* pairs_ms) {
    static_assert(sizeof(cl_dotplot_entry) == sizeof(uint4), "an entry is written as one 16-byte store");
    hipStream_t s = ctx->stream;
    int rc;
    const uint64_t G = win_off[n];
    std::vector<uint64_t> h_start(n + 1, 0);
    for (uint64_t i = 0; i < n; ++i) h_start[i + 1] = h_start[i] + lens[i];
    const uint32_t n_text = (uint32_t)h_start[n];   // < 2^30 (checked by the caller)
    hipEvent_t ev[3];
    for (auto& e : ev) HIP_TRY(ctx, hipEventCreate(&e));
    struct Events { hipEvent_t* e; ~Events() { for (int i = 0; i < 3; ++i) (void)hipEventDestroy(e[i]); } } events{ev};
    HIP_TRY(ctx, hipEventRecord(ev[0], s));

    // ---- spectra: every window's ascending list of distinct k-mer ranks -------------------------------------------------------------------
    ScopedBuf<uint32_t> list, list_off;
    std::vector<uint32_t> h_off(G + 1, 0);
    uint32_t n_list = 0;
    if (n_text && G) {
        ScopedBuf<uint8_t> text;
        ScopedBuf<uint64_t> seq_start, win_off_dev, key, key_c;
        ScopedBuf<uint32_t> win, win_c, flag, pos;
        ScopedBuf<char> temp;
        const size_t temp_bytes = std::max({clradix::sort_temp_bytes<uint64_t>(n_text), clradix::sort_temp_bytes<uint32_t>(n_text), clradix::scan_temp_bytes(n_text)});
        if ((rc = text.alloc(ctx, n_text)) || (rc = seq_start.alloc(ctx, n + 1)) || (rc = win_off_dev.alloc(ctx, n + 1)) || (rc = key.alloc(ctx, n_text)) ||
            (rc = key_c.alloc(ctx, n_text)) || (rc = win.alloc(ctx, n_text)) || (rc = win_c.alloc(ctx, n_text)) || (rc = flag.alloc(ctx, n_text)) ||
            (rc = pos.alloc(ctx, n_text)) || (rc = temp.alloc(ctx, temp_bytes)))
            return rc;
        for (uint64_t i = 0; i < n; ++i)
            if (lens[i]) HIP_TRY(ctx, hipMemcpyAsync(text.p + h_start[i], seqs[i], lens[i], hipMemcpyHostToDevice, s));
        HIP_TRY(ctx, hipMemcpyAsync(seq_start.p, h_start.data(), (n + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, s));
        HIP_TRY(ctx, hipMemcpyAsync(win_off_dev.p, win_off, (n + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, s));
        const dim3 text_grid((n_text + kBlock - 1) / kBlock);
        hipLaunchKernelGGL(dotplot_keys_kernel, text_grid, dim3(kBlock), 0, s, text.p, n_text, seq_start.p, win_off_dev.p, (uint32_t)n, (uint32_t)k, window, key.p, win.p,
                           flag.p);
        HIP_TRY(ctx, clradix::inclusive_sum(temp.p, temp.n, flag.p, pos.p, n_text, s));
        uint32_t m = 0;
        HIP_TRY(ctx, hipMemcpyAsync(&m, pos.p + (n_text - 1), sizeof(uint32_t), hipMemcpyDeviceToHost, s));
        hipLaunchKernelGGL(dotplot_compact_kernel, text_grid, dim3(kBlock), 0, s, key.p, win.p, flag.p, pos.p, n_text, key_c.p, win_c.p);
        HIP_TRY(ctx, hipGetLastError());
        HIP_TRY(ctx, hipStreamSynchronize(s));
        if (m) {
            const dim3 grid((m + kBlock - 1) / kBlock);
            // by k-mer: (key_c, win_c) -> (key, win); rank of every position's k-mer (1-based: the inclusive scan itself) -> pos
            HIP_TRY(ctx, clradix::sort_pairs<uint64_t>(temp.p, temp.n, key_c.p, key.p, win_c.p, win.p, m, 0u, 2u * (uint32_t)k, s));
            hipLaunchKernelGGL(dotplot_kmer_heads_kernel, grid, dim3(kBlock), 0, s, key.p, m, flag.p);
            HIP_TRY(ctx, clradix::inclusive_sum(temp.p, temp.n, flag.p, pos.p, m, s));
            // by window alone, stable: (win, pos) -> (win_c, flag); with one window the order is already that
            const uint32_t* win_sorted = win.p;
            const uint32_t* rank_sorted = pos.p;
            ScopedBuf<uint32_t> rank2, head, head_pos;
            if ((rc = rank2.alloc(ctx, m)) || (rc = head.alloc(ctx, m)) || (rc = head_pos.alloc(ctx, m))) return rc;
            if (G > 1) {
                HIP_TRY(ctx, clradix::sort_pairs<uint32_t>(temp.p, temp.n, win.p, win_c.p, pos.p, rank2.p, m, 0u, bits_for(G - 1), s));
                win_sorted = win_c.p;
                rank_sorted = rank2.p;
            }
            hipLaunchKernelGGL(dotplot_list_heads_kernel, grid, dim3(kBlock), 0, s, win_sorted, rank_sorted, m, head.p);
            HIP_TRY(ctx, clradix::inclusive_sum(temp.p, temp.n, head.p, head_pos.p, m, s));
            HIP_TRY(ctx, hipMemcpyAsync(&n_list, head_pos.p + (m - 1), sizeof(uint32_t), hipMemcpyDeviceToHost, s));
            HIP_TRY(ctx, hipStreamSynchronize(s));
            if ((rc = list.alloc(ctx, n_list)) || (rc = list_off.alloc(ctx, G + 1))) return rc;
            hipLaunchKernelGGL(dotplot_list_kernel, grid, dim3(kBlock), 0, s, rank_sorted, head.p, head_pos.p, m, list.p);
            hipLaunchKernelGGL(dotplot_list_offsets_kernel, dim3((uint32_t)((G + 1 + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, win_sorted, head_pos.p, m, G, list_off.p);
            HIP_TRY(ctx, hipGetLastError());
            HIP_TRY(ctx, hipMemcpyAsync(h_off.data(), list_off.p, (G + 1) * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
            HIP_TRY(ctx, hipStreamSynchronize(s));
        }
    }
    for (uint64_t g = 0; g < G; ++g) distinct[g] = h_off[g + 1] - h_off[g];
    HIP_TRY(ctx, hipEventRecord(ev[1], s));

    // ---- pairs ----------------------------------------------------------------------------------------------------------------------------
    entries.clear();
    if (n_list) {
        std::vector<std::pair<uint32_t, uint32_t>> spans;   // the window ranges whose pairs are compared
        if (pairs == 1) {
            for (uint64_t i = 0; i < n; ++i)
                if (win_off[i + 1] > win_off[i]) spans.push_back({(uint32_t)win_off[i], (uint32_t)win_off[i + 1]});
        } else {
            spans.push_back({0u, (uint32_t)G});
        }
        auto tiles_at = [&](uint32_t T) {
            uint64_t sum = 0;
            for (const auto& sp : spans) { const uint64_t R = ((uint64_t)(sp.second - sp.first) + T - 1) / T; sum += R * (R + 1) / 2; }
            return sum;
        };
        uint32_t T = tile_windows;
        if (T == 0)   // large tiles stage a column list once for many rows; small inputs need tiles enough to fill the device
            for (T = 32; T > 8 && tiles_at(T) < kMaxGrid; T /= 2) {}
        if (G * T >= (1ull << 31)) T = (uint32_t)std::max<uint64_t>(1, (1ull << 31) / G);   // a tile row's counts and entries stay within 32 bits
        std::vector<TileRange> ranges;
        std::vector<TileRow> rows;
        uint64_t n_tiles = 0;
        for (const auto& sp : spans) {
            ranges.push_back({sp.first, sp.second, n_tiles});
            const uint64_t R = ((uint64_t)(sp.second - sp.first) + T - 1) / T;
            for (uint64_t ti = 0; ti < R; ++ti) { rows.push_back({(uint32_t)(ranges.size() - 1), n_tiles, R - ti}); n_tiles += R - ti; }
        }
        ScopedBuf<TileRange> ranges_dev;
        ScopedBuf<uint32_t> shared_dev, kept_dev, kept_incl;
        ScopedBuf<uint4> entries_dev;
        ScopedBuf<char> temp;
        if ((rc = ranges_dev.upload(ctx, ranges))) return rc;
        const uint64_t batch_tiles = std::max<uint64_t>(1, kBatchPairs / ((uint64_t)T * T));
        for (size_t r0 = 0; r0 < rows.size();) {
            size_t r1 = r0 + 1;   // whole tile rows, at least one
            while (r1 < rows.size() && rows[r1].first + rows[r1].width - rows[r0].first <= batch_tiles) ++r1;
            const uint64_t t_begin = rows[r0].first, t_end = rows[r1 - 1].first + rows[r1 - 1].width, nt = t_end - t_begin;
            const uint32_t grid = (uint32_t)std::min<uint64_t>(nt, kMaxGrid);
            if (shared_dev.n < nt * T * T && (rc = shared_dev.alloc(ctx, nt * T * T))) return rc;
            if (kept_dev.n < nt * T && ((rc = kept_dev.alloc(ctx, nt * T)) || (rc = kept_incl.alloc(ctx, nt * T)) || (rc = temp.alloc(ctx, clradix::scan_temp_bytes(nt * T)))))
                return rc;
            hipLaunchKernelGGL(dotplot_tile_kernel, dim3(grid), dim3(kTileBlock), 0, s, list.p, list_off.p, ranges_dev.p, (uint32_t)ranges.size(), t_begin, t_end, T,
                               (unsigned long long)q, shared_dev.p, kept_dev.p);
            HIP_TRY(ctx, hipGetLastError());
            HIP_TRY(ctx, clradix::inclusive_sum(temp.p, temp.n, kept_dev.p, kept_incl.p, nt * T, s));
            uint32_t n_kept = 0;
            HIP_TRY(ctx, hipMemcpyAsync(&n_kept, kept_incl.p + (nt * T - 1), sizeof(uint32_t), hipMemcpyDeviceToHost, s));
            HIP_TRY(ctx, hipStreamSynchronize(s));
            if (n_kept) {
                if (entries_dev.n < n_kept && (rc = entries_dev.alloc(ctx, n_kept))) return rc;
                hipLaunchKernelGGL(dotplot_write_kernel, dim3(grid), dim3(kTileBlock), 0, s, list_off.p, ranges_dev.p, (uint32_t)ranges.size(), t_begin, t_end, T, shared_dev.p,
                                   kept_incl.p, entries_dev.p);
                HIP_TRY(ctx, hipGetLastError());
                const size_t had = entries.size();
                entries.resize(had + n_kept);
                HIP_TRY(ctx, hipMemcpyAsync(entries.data() + had, entries_dev.p, (size_t)n_kept * sizeof(uint4), hipMemcpyDeviceToHost, s));
                HIP_TRY(ctx, hipStreamSynchronize(s));
            }
            r0 = r1;
        }
    }
    HIP_TRY(ctx, hipEventRecord(ev[2], s));
    HIP_TRY(ctx, hipStreamSynchronize(s));
    if (spectra_ms) (void)hipEventElapsedTime(spectra_ms, ev[0], ev[1]);
    if (pairs_ms) (void)hipEventElapsedTime(pairs_ms, ev[1], ev[2]);
    return CL_OK;
}
