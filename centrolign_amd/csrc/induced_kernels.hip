// induced_kernels.hip — the -A output of an acyclic MSA graph for many pairs of paths at once: induced_pairwise_alignment (src/alignment.cpp:130-224)
// printed as explicit_cigar (include/centrolign/alignment.hpp:2804-2843).  The host restatement is cl_induced_pairwise_cigar (cl_io_api.cpp); the
// entry point is cl_induced_pairwise_cigars (cl_induced_api.cpp).
//
// The reference's loop over path 2 has a parallel form.  Step i of path 2 meets path 1 at a_i = pos1[path2[i]] or not at all.  Matched steps, in
// order and numbered k = 0, 1, ..., are emitted at path-1 index e_k = max(j_k, a_k) with j_{k+1} = e_k + 1 and j_0 = 0, i.e.
//     e_k = k + max(0, max_{m <= k} (a_m - m))
// (the reference never moves j backwards: a step that meets path 1 behind j is paired with j itself).  That is a prefix scan of (count, last matched
// step, max(a - rank)) along path 2.  The gap run in front of match k holds the unmatched path-2 steps since the previous match and the e_k - j_k
// skipped path-1 steps; the consolidation rule of :170-224 decides the run on its own (equal counts of at most 4: pairs at last + n + 1, compared
// by label; otherwise all deletions, then all insertions), and the path-2 run after the last match is handled the same way against the rest of
// path 1.  So every matched step yields at most five op tokens, each decided by the step's scan prefix and the labels it reads.
//
// The CIGAR is the run-length encoding of the token stream.  A second scan over (columns, first run start, last run start, text of the runs
// completed in between, last run's op) — a monoid — gives every run's start column and every completed run's text offset.  Two passes of the
// same kernel: the first one only counts each pair's text bytes, the second one writes each run's text when the next run begins.  No array of
// columns or runs is ever stored: per pair the device holds the position table of its path 1 and its own text.
//
// One 1024-thread workgroup per pair walks path 2 in tiles of 4096 steps (4 consecutive steps per thread, two block scans per tile, carries in
// registers).  The gather through pos1 is the only random access; path 2, and path 1 at the emitted indices, stream.
//
// cl_induced_pairwise_stats (induced_stats_kernel) wants the same alignment as numbers: per op the bases and the number of runs.  Scan 1 and the
// tokens are the same; scan 2's monoid becomes (bases per op, runs per op, first op, last op) of a token segment, joined with the run that spans
// the seam counted once.  Only the whole pair's element is wanted, so a tile is reduced in order rather than scanned, in one pass: nothing is
// stored per step and no text exists; each pair's eight counters are written once at the end.
//
// cl_induced_pairwise_profiles (induced_profile_kernel) and cl_induced_gap_events_batch (induced_events_kernel) want the tokens with their places:
// i1 and i2 of the CIGAR walk in front of a token's first column.  These too follow from scan 1 alone: for matched step k the gap run starts at
// (e_prev + 1, last + 1), its D token has length e - e_prev - 1, its I token stands at (e, last + 1) and the match at (e, s).  So neither needs a
// positional scan.  The profile adds every token to the bins of the path-1 windows it covers (integer atomics, reduced per wave first: the result
// does not depend on scheduling); the events kernel counts, then writes, the I and D tokens of at least min_len bases, each of which is one run.
//
// cl_induced_pairwise_agreements compares the alignments two graphs `a` and `b` imply for the same pair of sequences.  The i2 of a CIGAR's '=' / 'X'
// columns strictly increases, so a graph's aligned pairs are a partial map i2 -> i1: induced_partner_kernel walks the tokens of `a` and stores
// that map, one 32-bit word per step of path 2 (the pair's slice of a scratch buffer preset to kNoPos; bit 31: the column is '=' in `a`), and
// induced_agreement_kernel walks the tokens of `b` on the same stream and counts the columns whose word holds their own i1.  Both follow from
// scan 1 alone, like the profile; all sums are integer workgroup sums.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "cl_internal.hpp"

namespace {

constexpr uint32_t kThreads = 1024, kWaves = kThreads / 64, kItems = 4, kTile = kThreads * kItems;
constexpr uint32_t kNoPos = 0xFFFFFFFFu;
constexpr int64_t kNegInf = INT64_MIN / 4;
enum : uint32_t { kOpEq = 0, kOpX = 1, kOpD = 2, kOpI = 3, kOpNone = 4 };

__device__ __forceinline__ int64_t shfl_up64(int64_t v, unsigned d) { return (int64_t)__shfl_up((long long)v, d, 64); }

__device__ __forceinline__ int64_t n_digits(int64_t v) {
    int64_t d = 1;
    while (v >= 10) { v /= 10; ++d; }
    return d;
}
__device__ __forceinline__ int64_t run_width(int64_t len) { return n_digits(len) + 1; }

// scan 1, over path 2: matched steps so far, the last of them, max(a - rank) over them (ranks local to the segment)
struct MatchScan {
    int64_t cnt, last, best;
    static __device__ MatchScan ident() { return {0, -1, kNegInf}; }
    __device__ MatchScan up(unsigned d) const { return {shfl_up64(cnt, d), shfl_up64(last, d), shfl_up64(best, d)}; }
};
__device__ __forceinline__ MatchScan combine(const MatchScan& a, const MatchScan& b) {
    return {a.cnt + b.cnt, a.last > b.last ? a.last : b.last, a.best > b.best - a.cnt ? a.best : b.best - a.cnt};
}

// scan 2, over the op tokens: columns, the first and last run start (relative to the segment, -1: none), text bytes of the runs that begin at
// or after the first start and end at the last one, and the op of the last run begun
struct RunScan {
    int64_t cols, first, last, text;
    uint32_t last_op;
    static __device__ RunScan ident() { return {0, -1, -1, 0, kOpNone}; }
    __device__ RunScan up(unsigned d) const {
        return {shfl_up64(cols, d), shfl_up64(first, d), shfl_up64(last, d), shfl_up64(text, d), (uint32_t)__shfl_up((int)last_op, d, 64)};
    }
};
__device__ __forceinline__ RunScan combine(const RunScan& a, const RunScan& b) {
    if (b.first < 0) return {a.cols + b.cols, a.first, a.last, a.text, a.last_op};
    if (a.first < 0) return {a.cols + b.cols, a.cols + b.first, a.cols + b.last, b.text, b.last_op};
    return {a.cols + b.cols, a.first, a.cols + b.last, a.text + b.text + run_width(a.cols + b.first - a.last), b.last_op};
}

template <class T>
__device__ __forceinline__ T wave_inclusive(T v, unsigned lane) {
#pragma unroll
    for (unsigned d = 1; d < 64; d <<= 1) {
        const T o = v.up(d);
        if (lane >= d) v = combine(o, v);
    }
    return v;
}

// exclusive prefix of v over the workgroup in thread order, and the workgroup's total; lds: kWaves entries
template <class T>
__device__ __forceinline__ T block_exclusive(T v, T* lds, T& total) {
    const unsigned lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const T inc = wave_inclusive(v, lane);
    if (lane == 63) lds[w] = inc;
    __syncthreads();
    if (w == 0) {
        T x = lane < kWaves ? lds[lane] : T::ident();
        x = wave_inclusive(x, lane);
        if (lane < kWaves) lds[lane] = x;
    }
    __syncthreads();
    const T before = w ? lds[w - 1] : T::ident();
    total = lds[kWaves - 1];
    T ex = inc.up(1);
    if (lane == 0) ex = T::ident();
    __syncthreads();
    return combine(before, ex);
}

struct PairView {
    const uint32_t* p1;
    const uint32_t* p2;
    const uint32_t* steps_end;   // end of the graph's path_nodes
    const uint8_t* label;
    uint64_t n_nodes;
    int64_t n1, n2;
};

// '=' or 'X' for path-1 index x1 against path-2 index x2 (0 <= x2 < n2).  x1 can lie past path 1 when path 2 meets path 1's nodes out of order or
// more than once: the host function then reads on into the flat path array, and so does this, as long as that stays inside the array.
__device__ __forceinline__ uint32_t pair_op(const PairView& v, int64_t x1, int64_t x2) {
    const uint32_t* q = v.p1 + x1;
    if (q >= v.steps_end) return kOpX;
    const uint32_t u1 = *q, u2 = v.p2[x2];
    if (u1 >= v.n_nodes) return kOpX;
    return v.label[u1] == v.label[u2] ? kOpEq : kOpX;
}

// the consolidated gap run behind (last1, last2) with g1 unmatched path-2 steps and g2 skipped path-1 steps (alignment.cpp:170-224)
template <class F>
__device__ __forceinline__ void gap_run_tokens(const PairView& v, int64_t last1, int64_t last2, int64_t g1, int64_t g2, F&& tok) {
    if (g1 == g2 && g1 <= 4) {
        for (int64_t n = 0; n < g1; ++n) tok(pair_op(v, last1 + n + 1, last2 + n + 1), (int64_t)1);
    } else {
        if (g2) tok((uint32_t)kOpD, g2);
        if (g1) tok((uint32_t)kOpI, g1);
    }
}

// matched step s with scan-1 prefix x (exclusive) and position a on path 1: the op of the match before it (kOpNone: none), and its tokens
__device__ __forceinline__ uint32_t previous_match_op(const PairView& v, const MatchScan& x) {
    return x.cnt > 0 ? pair_op(v, x.cnt - 1 + (x.best > 0 ? x.best : 0), x.last) : (uint32_t)kOpNone;
}
template <class F>
__device__ __forceinline__ void match_tokens(const PairView& v, const MatchScan& x, int64_t s, int64_t a, F&& tok) {
    const int64_t k = x.cnt;
    const int64_t best = x.best > a - k ? x.best : a - k;
    const int64_t e = k + (best > 0 ? best : 0);
    const int64_t e_prev = k > 0 ? k - 1 + (x.best > 0 ? x.best : 0) : -1;
    gap_run_tokens(v, e_prev, x.last, s - x.last - 1, e - e_prev - 1, tok);
    tok((uint32_t)pair_op(v, e, s), (int64_t)1);
}

// The same tokens with their places: tok(op, cnt, i1, i2), i1 / i2 being the path-1 / path-2 index of the CIGAR walk in front of the token's first
// column.  Every D or I token is one whole run of the CIGAR: a match stands on either side of a gap run.
template <class F>
__device__ __forceinline__ void gap_run_tokens_at(const PairView& v, int64_t last1, int64_t last2, int64_t g1, int64_t g2, F&& tok) {
    if (g1 == g2 && g1 <= 4) {
        for (int64_t n = 0; n < g1; ++n) tok(pair_op(v, last1 + n + 1, last2 + n + 1), (int64_t)1, last1 + n + 1, last2 + n + 1);
    } else {
        if (g2) tok((uint32_t)kOpD, g2, last1 + 1, last2 + 1);
        if (g1) tok((uint32_t)kOpI, g1, last1 + 1 + g2, last2 + 1);
    }
}
template <class F>
__device__ __forceinline__ void match_tokens_at(const PairView& v, const MatchScan& x, int64_t s, int64_t a, F&& tok) {
    const int64_t k = x.cnt;
    const int64_t best = x.best > a - k ? x.best : a - k;
    const int64_t e = k + (best > 0 ? best : 0);
    const int64_t e_prev = k > 0 ? k - 1 + (x.best > 0 ? x.best : 0) : -1;
    gap_run_tokens_at(v, e_prev, x.last, s - x.last - 1, e - e_prev - 1, tok);
    tok((uint32_t)pair_op(v, e, s), (int64_t)1, e, s);
}

// the run scan element of a token sequence that follows a run of op `cur`
struct RunBuilder {
    RunScan r;
    uint32_t cur;
    __device__ explicit RunBuilder(uint32_t prev_op) : r(RunScan::ident()), cur(prev_op) {}
    __device__ void operator()(uint32_t op, int64_t cnt) {
        if (op != cur) {
            if (r.last >= 0) r.text += run_width(r.cols - r.last);
            if (r.first < 0) r.first = r.cols;
            r.last = r.cols;
            r.last_op = op;
            cur = op;
        }
        r.cols += cnt;
    }
};

// cl_induced_pairwise_stats' element of a token segment: bases and runs per op (indexed by kOpEq .. kOpI), the segment's first and last op
// (kOpNone: no token).  Also the builder: tokens are appended with operator().
struct StatScan {
    int64_t n[4], runs[4];
    uint32_t first, last;
    static __device__ StatScan ident() { return {{0, 0, 0, 0}, {0, 0, 0, 0}, kOpNone, kOpNone}; }
    __device__ StatScan down(unsigned d) const {
        StatScan o;
#pragma unroll
        for (uint32_t k = 0; k < 4; ++k) {
            o.n[k] = (int64_t)__shfl_down((long long)n[k], d, 64);
            o.runs[k] = (int64_t)__shfl_down((long long)runs[k], d, 64);
        }
        o.first = (uint32_t)__shfl_down((int)first, d, 64);
        o.last = (uint32_t)__shfl_down((int)last, d, 64);
        return o;
    }
    __device__ void operator()(uint32_t op, int64_t cnt) {
#pragma unroll
        for (uint32_t k = 0; k < 4; ++k) {
            n[k] += op == k ? cnt : 0;
            runs[k] += op == k && op != last;
        }
        if (first == kOpNone) first = op;
        last = op;
    }
};
__device__ __forceinline__ StatScan combine(const StatScan& a, const StatScan& b) {
    StatScan r;
#pragma unroll
    for (uint32_t k = 0; k < 4; ++k) {
        r.n[k] = a.n[k] + b.n[k];
        r.runs[k] = a.runs[k] + b.runs[k] - (a.last == k && b.first == k);   // one run across the seam
    }
    r.first = a.first != kOpNone ? a.first : b.first;
    r.last = b.last != kOpNone ? b.last : a.last;
    return r;
}

// the workgroup's elements combined in thread order; the result is thread 0's alone.  lds: kWaves entries, free to reuse after the next barrier
__device__ __forceinline__ StatScan block_reduce_ordered(StatScan v, StatScan* lds) {
    const unsigned lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (unsigned d = 1; d < 64; d <<= 1) {
        const StatScan o = v.down(d);
        if (lane + d < 64) v = combine(v, o);
    }
    if (lane == 0) lds[w] = v;
    __syncthreads();
    if (w == 0) {
        v = lane < kWaves ? lds[lane] : StatScan::ident();
#pragma unroll
        for (unsigned d = 1; d < kWaves; d <<= 1) {
            const StatScan o = v.down(d);
            if (lane + d < kWaves) v = combine(v, o);
        }
    }
    return v;
}

// the same tokens continuing the absolute state p (p.last, p.last_op: the run in progress; p.text: its text offset): a finished run is written out
struct RunWriter {
    RunScan p;
    char* out;
    int64_t cap;
    __device__ void put(int64_t len, uint32_t op) {
        const int64_t w = run_width(len);
        if (p.text + w <= cap) {
            for (int64_t i = w - 2; i >= 0; --i) { out[p.text + i] = (char)('0' + len % 10); len /= 10; }
            out[p.text + w - 1] = "=XDI"[op & 3];
        }
        p.text += w;
    }
    __device__ void operator()(uint32_t op, int64_t cnt) {
        if (op != p.last_op) {
            if (p.last >= 0) put(p.cols - p.last, p.last_op);
            p.last = p.cols;
            p.last_op = op;
        }
        p.cols += cnt;
    }
};

template <bool kWrite>
__global__ void __launch_bounds__(kThreads) induced_runs_kernel(const ClInducedJob* __restrict__ jobs, const uint32_t* __restrict__ path_nodes, uint64_t n_steps,
                                                               const uint8_t* __restrict__ label, uint64_t n_nodes, const uint32_t* __restrict__ tables,
                                                               int64_t* __restrict__ text_len, char* __restrict__ text) {
    __shared__ MatchScan lds1[kWaves];
    __shared__ RunScan lds2[kWaves];
    const ClInducedJob job = jobs[blockIdx.x];
    const uint32_t* pos = tables + job.table;
    PairView v{path_nodes + job.off1, path_nodes + job.off2, path_nodes + n_steps, label, n_nodes, (int64_t)job.n1, (int64_t)job.n2};
    char* out = kWrite ? text + job.text_off : nullptr;
    const int64_t cap = kWrite ? (int64_t)job.text_cap : 0;
    MatchScan c1 = MatchScan::ident();
    RunScan c2 = RunScan::ident();
    for (int64_t base = 0; base < v.n2; base += kTile) {
        const int64_t s0 = base + (int64_t)threadIdx.x * kItems;
        uint32_t a[kItems];
        MatchScan agg = MatchScan::ident();
#pragma unroll
        for (uint32_t r = 0; r < kItems; ++r) {
            a[r] = kNoPos;
            if (s0 + r < v.n2) a[r] = pos[v.p2[s0 + r]];
            if (a[r] != kNoPos) agg = combine(agg, MatchScan{1, s0 + r, (int64_t)a[r]});
        }
        MatchScan tot1;
        const MatchScan pre1 = combine(c1, block_exclusive(agg, lds1, tot1));
        c1 = combine(c1, tot1);
        RunScan ragg = RunScan::ident();
        MatchScan x = pre1;
#pragma unroll
        for (uint32_t r = 0; r < kItems; ++r) {
            if (a[r] == kNoPos) continue;
            RunBuilder b(previous_match_op(v, x));
            match_tokens(v, x, s0 + r, (int64_t)a[r], [&](uint32_t op, int64_t cnt) { b(op, cnt); });
            ragg = combine(ragg, b.r);
            x = combine(x, MatchScan{1, s0 + r, (int64_t)a[r]});
        }
        RunScan tot2;
        const RunScan pre2 = combine(c2, block_exclusive(ragg, lds2, tot2));
        c2 = combine(c2, tot2);
        if (kWrite) {
            RunWriter wr{pre2, out, cap};   // (the run in progress is the previous match's: the same runs as RunBuilder finds)
            x = pre1;
#pragma unroll
            for (uint32_t r = 0; r < kItems; ++r) {
                if (a[r] == kNoPos) continue;
                match_tokens(v, x, s0 + r, (int64_t)a[r], [&](uint32_t op, int64_t cnt) { wr(op, cnt); });
                x = combine(x, MatchScan{1, s0 + r, (int64_t)a[r]});
            }
        }
    }
    if (threadIdx.x != 0) return;
    // the run after the last match (alignment.cpp:164-167 and the run it ends in)
    const int64_t k = c1.cnt;
    const int64_t e_last = k > 0 ? k - 1 + (c1.best > 0 ? c1.best : 0) : -1;
    const int64_t g2 = v.n1 > e_last + 1 ? v.n1 - e_last - 1 : 0, g1 = v.n2 - 1 - c1.last;
    if (!kWrite) {
        RunBuilder b(previous_match_op(v, c1));
        gap_run_tokens(v, e_last, c1.last, g1, g2, [&](uint32_t op, int64_t cnt) { b(op, cnt); });
        const RunScan all = combine(c2, b.r);
        text_len[blockIdx.x] = all.text + (all.last >= 0 ? run_width(all.cols - all.last) : 0);
    } else {
        RunWriter wr{c2, out, cap};
        gap_run_tokens(v, e_last, c1.last, g1, g2, [&](uint32_t op, int64_t cnt) { wr(op, cnt); });
        if (wr.p.last >= 0) wr.put(wr.p.cols - wr.p.last, wr.p.last_op);
    }
}

// One pass: scan 1 as above, then every thread's tokens go into one StatScan, the tile is reduced in order and thread 0 appends it to the pair's
// element, which it keeps in registers.  (lds2 is written again only after the barriers of the next tile's scan 1, which wave 0 reaches after its reads.)
__global__ void __launch_bounds__(kThreads) induced_stats_kernel(const ClInducedJob* __restrict__ jobs, const uint32_t* __restrict__ path_nodes, uint64_t n_steps,
                                                                const uint8_t* __restrict__ label, uint64_t n_nodes, const uint32_t* __restrict__ tables,
                                                                cl_pair_stats* __restrict__ stats) {
    __shared__ MatchScan lds1[kWaves];
    __shared__ StatScan lds2[kWaves];
    const ClInducedJob job = jobs[blockIdx.x];
    const uint32_t* pos = tables + job.table;
    PairView v{path_nodes + job.off1, path_nodes + job.off2, path_nodes + n_steps, label, n_nodes, (int64_t)job.n1, (int64_t)job.n2};
    MatchScan c1 = MatchScan::ident();
    StatScan c2 = StatScan::ident();
    for (int64_t base = 0; base < v.n2; base += kTile) {
        const int64_t s0 = base + (int64_t)threadIdx.x * kItems;
        uint32_t a[kItems];
        MatchScan agg = MatchScan::ident();
#pragma unroll
        for (uint32_t r = 0; r < kItems; ++r) {
            a[r] = kNoPos;
            if (s0 + r < v.n2) a[r] = pos[v.p2[s0 + r]];
            if (a[r] != kNoPos) agg = combine(agg, MatchScan{1, s0 + r, (int64_t)a[r]});
        }
        MatchScan tot1;
        MatchScan x = combine(c1, block_exclusive(agg, lds1, tot1));
        c1 = combine(c1, tot1);
        StatScan sagg = StatScan::ident();
#pragma unroll
        for (uint32_t r = 0; r < kItems; ++r) {
            if (a[r] == kNoPos) continue;
            match_tokens(v, x, s0 + r, (int64_t)a[r], [&](uint32_t op, int64_t cnt) { sagg(op, cnt); });
            x = combine(x, MatchScan{1, s0 + r, (int64_t)a[r]});
        }
        const StatScan tile = block_reduce_ordered(sagg, lds2);
        if (threadIdx.x == 0) c2 = combine(c2, tile);   // the pair's element lives in thread 0 alone
    }
    if (threadIdx.x != 0) return;
    // the run after the last match, as in induced_runs_kernel
    const int64_t k = c1.cnt;
    const int64_t e_last = k > 0 ? k - 1 + (c1.best > 0 ? c1.best : 0) : -1;
    const int64_t g2 = v.n1 > e_last + 1 ? v.n1 - e_last - 1 : 0, g1 = v.n2 - 1 - c1.last;
    gap_run_tokens(v, e_last, c1.last, g1, g2, [&](uint32_t op, int64_t cnt) { c2(op, cnt); });
    cl_pair_stats out;
    out.eq = (uint64_t)c2.n[kOpEq]; out.x = (uint64_t)c2.n[kOpX]; out.ins = (uint64_t)c2.n[kOpI]; out.del = (uint64_t)c2.n[kOpD];
    out.eq_runs = (uint64_t)c2.runs[kOpEq]; out.x_runs = (uint64_t)c2.runs[kOpX]; out.ins_runs = (uint64_t)c2.runs[kOpI]; out.del_runs = (uint64_t)c2.runs[kOpD];
    stats[blockIdx.x] = out;
}

// ------------------------------------------------------------- windowed profiles --------------------------------------------------------------
// The bins of one pair: n_win windows of `width` path-1 bases, the last one open-ended (it takes every column at or past its start: trailing
// insertions, and path-1 indices past path 1's end, see pair_op).  A thread's tokens come in non-decreasing i1, so it keeps the counts of the
// window it is in in registers and moves on with seek(); a count leaves the registers as one integer atomic per non-zero counter.
struct WindowBins {
    unsigned long long* bins;   // [n_win][4]: eq, x, ins, del (cl_pair_window)
    int64_t width, last;        // last = n_win - 1
    __device__ void add(int64_t w, uint32_t field, uint64_t n) const {
        if (n) atomicAdd(bins + 4 * w + field, (unsigned long long)n);
    }
};
constexpr int64_t kOpenEnd = INT64_MAX;
__device__ __forceinline__ uint32_t field_of_op(uint32_t op) { return op == kOpEq ? 0u : op == kOpX ? 1u : op == kOpI ? 2u : 3u; }   // cl_pair_window's order

struct WindowAcc {
    int64_t w, lo, hi;          // the window the thread is in and its path-1 range [lo, hi); w < 0: none yet
    uint32_t eq, x;
    uint64_t ins, del;
    __device__ WindowAcc() : w(-1), lo(0), hi(0), eq(0), x(0), ins(0), del(0) {}
    __device__ void flush(const WindowBins& b) {
        if (w >= 0) { b.add(w, 0, eq); b.add(w, 1, x); b.add(w, 2, ins); b.add(w, 3, del); }
        eq = x = 0;
        ins = del = 0;
    }
    __device__ void enter(const WindowBins& b, int64_t nw) {   // nw: unclamped window index
        flush(b);
        w = nw < b.last ? nw : b.last;
        lo = w * b.width;
        hi = w < b.last ? lo + b.width : kOpenEnd;
    }
    // move to the window of path-1 index i1 (at or after every index sought before)
    __device__ void seek(const WindowBins& b, int64_t i1) {
        if (w < 0) enter(b, i1 / b.width);
        else if (i1 >= hi) enter(b, i1 - hi < b.width ? w + 1 : i1 / b.width);
    }
    __device__ void count(uint32_t op, int64_t cnt) {
        eq += op == kOpEq ? (uint32_t)cnt : 0;
        x += op == kOpX ? (uint32_t)cnt : 0;
        ins += op == kOpI ? (uint64_t)cnt : 0;
        del += op == kOpD ? (uint64_t)cnt : 0;
    }
};

// The counts the lanes of a wave still hold at the end of a tile, added to the bins: lanes in the same window are neighbours (i1 does not
// decrease along path 2), so the wave sums each segment of equal window with shuffles and the segment's last lane issues its atomics.
__device__ __forceinline__ void wave_flush(const WindowBins& b, WindowAcc& acc) {
    const unsigned lane = threadIdx.x & 63;
    const int64_t up = shfl_up64(acc.w, 1);
    int start = lane == 0 || up != acc.w ? (int)lane : 0;   // the first lane of this lane's segment, after the scan
#pragma unroll
    for (unsigned d = 1; d < 64; d <<= 1) {
        const int o = __shfl_up(start, d, 64);
        if (lane >= d && o > start) start = o;
    }
#pragma unroll
    for (unsigned d = 1; d < 64; d <<= 1) {
        const uint32_t eq = (uint32_t)__shfl_up((int)acc.eq, d, 64), x = (uint32_t)__shfl_up((int)acc.x, d, 64);
        const uint64_t ins = (uint64_t)shfl_up64((int64_t)acc.ins, d), del = (uint64_t)shfl_up64((int64_t)acc.del, d);
        if ((int)lane - (int)d >= start) { acc.eq += eq; acc.x += x; acc.ins += ins; acc.del += del; }
    }
    const int64_t down = (int64_t)__shfl_down((long long)acc.w, 1, 64);
    if (lane != 63 && down == acc.w) acc.eq = acc.x = 0, acc.ins = acc.del = 0;   // not the segment's last lane
    acc.flush(b);
    acc.w = -1;
}

// Scan 1 as in induced_stats_kernel, then every thread adds its tokens to the windows they cover.  A D run is split base by base over its windows:
// the part in the thread's window and the part in the run's last window go through the thread's registers; the whole windows in between get
// `width` each, from the thread itself when they are few and from the 64 lanes of its wave otherwise (a run can cross more windows than a tile
// has threads).  The run after the last match is added by the whole workgroup: its D run can be all of path 1.
__global__ void __launch_bounds__(kThreads) induced_profile_kernel(const ClInducedJob* __restrict__ jobs, const uint32_t* __restrict__ path_nodes, uint64_t n_steps,
                                                                  const uint8_t* __restrict__ label, uint64_t n_nodes, const uint32_t* __restrict__ tables,
                                                                  uint64_t width, cl_pair_window* __restrict__ windows) {
    __shared__ MatchScan lds1[kWaves];
    constexpr int64_t kInlineWindows = 4;
    const ClInducedJob job = jobs[blockIdx.x];
    const uint32_t* pos = tables + job.table;
    PairView v{path_nodes + job.off1, path_nodes + job.off2, path_nodes + n_steps, label, n_nodes, (int64_t)job.n1, (int64_t)job.n2};
    const WindowBins b{(unsigned long long*)(windows + job.text_off), (int64_t)width, (int64_t)job.text_cap - 1};
    const unsigned lane = threadIdx.x & 63;
    MatchScan c1 = MatchScan::ident();
    for (int64_t base = 0; base < v.n2; base += kTile) {
        const int64_t s0 = base + (int64_t)threadIdx.x * kItems;
        uint32_t a[kItems];
        MatchScan agg = MatchScan::ident();
#pragma unroll
        for (uint32_t r = 0; r < kItems; ++r) {
            a[r] = kNoPos;
            if (s0 + r < v.n2) a[r] = pos[v.p2[s0 + r]];
            if (a[r] != kNoPos) agg = combine(agg, MatchScan{1, s0 + r, (int64_t)a[r]});
        }
        MatchScan tot1;
        MatchScan x = combine(c1, block_exclusive(agg, lds1, tot1));
        c1 = combine(c1, tot1);
        WindowAcc acc;
#pragma unroll
        for (uint32_t r = 0; r < kItems; ++r) {
            int64_t whole0 = 0, whole1 = 0;   // the whole windows [whole0, whole1) of this step's D run, left to the wave
            if (a[r] != kNoPos) {
                match_tokens_at(v, x, s0 + r, (int64_t)a[r], [&](uint32_t op, int64_t cnt, int64_t i1, int64_t) {
                    acc.seek(b, i1);
                    if (op != kOpD || i1 + cnt <= acc.hi) { acc.count(op, cnt); return; }
                    const int64_t end = i1 + cnt;
                    acc.count(op, acc.hi - i1);
                    const int64_t w0 = acc.w + 1, at = (end - 1) / b.width, w1 = at < b.last ? at : b.last;   // w0 <= w1: the run goes on past acc.hi
                    if (w1 - w0 <= kInlineWindows) for (int64_t w = w0; w < w1; ++w) b.add(w, 3, (uint64_t)b.width);
                    else { whole0 = w0; whole1 = w1; }
                    acc.enter(b, w1);
                    acc.count(op, end - acc.lo);
                });
                x = combine(x, MatchScan{1, s0 + r, (int64_t)a[r]});
            }
            for (uint64_t m = __ballot(whole1 > whole0); m; m &= m - 1) {
                const int src = __ffsll((unsigned long long)m) - 1;
                const int64_t w0 = (int64_t)__shfl((long long)whole0, src, 64), w1 = (int64_t)__shfl((long long)whole1, src, 64);
                for (int64_t w = w0 + lane; w < w1; w += 64) b.add(w, 3, (uint64_t)b.width);
            }
        }
        wave_flush(b, acc);
    }
    // the run after the last match, as in induced_runs_kernel
    const int64_t k = c1.cnt;
    const int64_t e_last = k > 0 ? k - 1 + (c1.best > 0 ? c1.best : 0) : -1;
    const int64_t g2 = v.n1 > e_last + 1 ? v.n1 - e_last - 1 : 0, g1 = v.n2 - 1 - c1.last;
    gap_run_tokens_at(v, e_last, c1.last, g1, g2, [&](uint32_t op, int64_t cnt, int64_t i1, int64_t) {
        const int64_t end = i1 + cnt, f = i1 / b.width, w0 = f < b.last ? f : b.last;
        if (op != kOpD) {
            if (threadIdx.x == 0) b.add(w0, field_of_op(op), (uint64_t)cnt);
            return;
        }
        const int64_t at = (end - 1) / b.width, w1 = at < b.last ? at : b.last;
        for (int64_t w = w0 + threadIdx.x; w <= w1; w += kThreads) {
            const int64_t lo = w * b.width > i1 ? w * b.width : i1, hi = w < b.last && (w + 1) * b.width < end ? (w + 1) * b.width : end;
            b.add(w, 3, (uint64_t)(hi - lo));
        }
    });
}

// ---------------------------------------------------------------- gap events ------------------------------------------------------------------
struct CountScan {
    int64_t n;
    static __device__ CountScan ident() { return {0}; }
    __device__ CountScan up(unsigned d) const { return {shfl_up64(n, d)}; }
};
__device__ __forceinline__ CountScan combine(const CountScan& a, const CountScan& b) { return {a.n + b.n}; }

// Two passes like induced_runs_kernel.  Counting: every thread counts its D and I tokens of at least min_len bases over all tiles, one workgroup sum
// at the end.  Writing: per tile an exclusive sum of the threads' counts (at most 8 each) places each thread's events behind the tile carry, so
// a pair's events are in CIGAR order.  job.text_off / text_cap: the pair's first event and their number, in elements of `events`.
template <bool kWrite>
__global__ void __launch_bounds__(kThreads) induced_events_kernel(const ClInducedJob* __restrict__ jobs, const uint32_t* __restrict__ path_nodes, uint64_t n_steps,
                                                                 const uint8_t* __restrict__ label, uint64_t n_nodes, const uint32_t* __restrict__ tables,
                                                                 uint64_t min_len, int64_t* __restrict__ n_events, cl_gap_event* __restrict__ events) {
    __shared__ MatchScan lds1[kWaves];
    __shared__ CountScan lds2[kWaves];
    const ClInducedJob job = jobs[blockIdx.x];
    const uint32_t* pos = tables + job.table;
    PairView v{path_nodes + job.off1, path_nodes + job.off2, path_nodes + n_steps, label, n_nodes, (int64_t)job.n1, (int64_t)job.n2};
    cl_gap_event* out = kWrite ? events + job.text_off : nullptr;
    const int64_t cap = kWrite ? (int64_t)job.text_cap : 0, len_min = (int64_t)min_len;
    auto is_event = [&](uint32_t op, int64_t cnt) { return (op == kOpD || op == kOpI) && cnt >= len_min; };
    auto put = [&](int64_t at, uint32_t op, int64_t cnt, int64_t i1, int64_t i2) {
        if (at < cap) out[at] = cl_gap_event{(uint64_t)i1, (uint64_t)i2, (uint64_t)cnt, op == kOpI ? 1u : 0u, 0u};
    };
    MatchScan c1 = MatchScan::ident();
    int64_t carry = 0;   // counting: this thread's events so far; writing: the pair's events in the tiles before
    for (int64_t base = 0; base < v.n2; base += kTile) {
        const int64_t s0 = base + (int64_t)threadIdx.x * kItems;
        uint32_t a[kItems];
        MatchScan agg = MatchScan::ident();
#pragma unroll
        for (uint32_t r = 0; r < kItems; ++r) {
            a[r] = kNoPos;
            if (s0 + r < v.n2) a[r] = pos[v.p2[s0 + r]];
            if (a[r] != kNoPos) agg = combine(agg, MatchScan{1, s0 + r, (int64_t)a[r]});
        }
        MatchScan tot1;
        const MatchScan pre1 = combine(c1, block_exclusive(agg, lds1, tot1));
        c1 = combine(c1, tot1);
        int64_t mine = 0;
        MatchScan x = pre1;
#pragma unroll
        for (uint32_t r = 0; r < kItems; ++r) {
            if (a[r] == kNoPos) continue;
            match_tokens_at(v, x, s0 + r, (int64_t)a[r], [&](uint32_t op, int64_t cnt, int64_t, int64_t) { mine += is_event(op, cnt); });
            x = combine(x, MatchScan{1, s0 + r, (int64_t)a[r]});
        }
        if (!kWrite) { carry += mine; continue; }
        CountScan tot2;
        int64_t at = carry + block_exclusive(CountScan{mine}, lds2, tot2).n;
        carry += tot2.n;
        x = pre1;
#pragma unroll
        for (uint32_t r = 0; r < kItems; ++r) {
            if (a[r] == kNoPos) continue;
            match_tokens_at(v, x, s0 + r, (int64_t)a[r], [&](uint32_t op, int64_t cnt, int64_t i1, int64_t i2) {
                if (is_event(op, cnt)) put(at++, op, cnt, i1, i2);
            });
            x = combine(x, MatchScan{1, s0 + r, (int64_t)a[r]});
        }
    }
    if (!kWrite) {
        CountScan tot2;
        block_exclusive(CountScan{carry}, lds2, tot2);
        carry = tot2.n;
    }
    if (threadIdx.x != 0) return;
    // the run after the last match, as in induced_runs_kernel
    const int64_t k = c1.cnt;
    const int64_t e_last = k > 0 ? k - 1 + (c1.best > 0 ? c1.best : 0) : -1;
    const int64_t g2 = v.n1 > e_last + 1 ? v.n1 - e_last - 1 : 0, g1 = v.n2 - 1 - c1.last;
    gap_run_tokens_at(v, e_last, c1.last, g1, g2, [&](uint32_t op, int64_t cnt, int64_t i1, int64_t i2) {
        if (!is_event(op, cnt)) return;
        if (kWrite) put(carry, op, cnt, i1, i2);
        ++carry;
    });
    if (!kWrite) n_events[blockIdx.x] = carry;
}

// ------------------------------------------------------------ agreement of two graphs ---------------------------------------------------------
// A partner word: the path-1 index a graph aligns a step of path 2 with, bit 31 set where the column is '='; kNoPos: the step is not aligned.
// Path 1 has fewer than 2^31 - 1 steps (the host checks), so no word of an aligned step equals kNoPos.
constexpr uint32_t kPartnerEq = 0x80000000u;

struct SumScan4 {
    uint64_t v[4];
    __device__ SumScan4 down(unsigned d) const {
        SumScan4 o;
#pragma unroll
        for (uint32_t k = 0; k < 4; ++k) o.v[k] = (uint64_t)__shfl_down((long long)v[k], d, 64);
        return o;
    }
};
// the workgroup's sums, in thread 0 alone; lds: kWaves entries
__device__ __forceinline__ SumScan4 block_sum4(SumScan4 s, SumScan4* lds) {
    const unsigned lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (unsigned d = 32; d >= 1; d >>= 1) {
        const SumScan4 o = s.down(d);
#pragma unroll
        for (uint32_t k = 0; k < 4; ++k) s.v[k] += o.v[k];   // (lanes whose partner lies past the wave add a value nobody reads: lane 0's sum is exact)
    }
    if (lane == 0) lds[w] = s;
    __syncthreads();
    if (threadIdx.x == 0)
        for (unsigned i = 1; i < kWaves; ++i)
#pragma unroll
            for (uint32_t k = 0; k < 4; ++k) s.v[k] += lds[i].v[k];
    return s;
}

// Scan 1 as in induced_stats_kernel; every '=' / 'X' token (i1, i2) is counted, and — kStore: graph `a` — stored as partner[i2] where i1 lies on
// path 1, or — !kStore: graph `b` — compared with partner[i2].  A token of a short equal gap run belongs to a step before the thread's own, in
// the previous tile when the thread is a tile's first, and the run after the last match is thread 0's: every store and every load is guarded by
// i2 < n2, the length of the pair's slice.  job.text_off: the slice's first word in `partner`; job.text_cap: the pair's slot in `counts` / `out`.
// kStore: counts[slot] = {aligned_a, eq_a}.  !kStore: out[slot], all 64 bytes, once.
template <bool kStore>
__device__ __forceinline__ void partner_agreement_walk(const ClInducedJob* __restrict__ jobs, const uint32_t* __restrict__ path_nodes, uint64_t n_steps,
                                                       const uint8_t* __restrict__ label, uint64_t n_nodes, const uint32_t* __restrict__ tables,
                                                       uint32_t* partner_words, uint64_t* counts, cl_pair_agreement* out) {
    __shared__ MatchScan lds1[kWaves];
    __shared__ SumScan4 lds2[kWaves];
    const ClInducedJob job = jobs[blockIdx.x];
    const uint32_t* pos = tables + job.table;
    PairView v{path_nodes + job.off1, path_nodes + job.off2, path_nodes + n_steps, label, n_nodes, (int64_t)job.n1, (int64_t)job.n2};
    uint32_t* partner = partner_words + job.text_off;
    SumScan4 sum{{0, 0, 0, 0}};   // aligned, eq, shared, shared_eq
    auto tok = [&](uint32_t op, int64_t, int64_t i1, int64_t i2) {
        if (op > kOpX) return;   // D, I
        sum.v[0] += 1;
        sum.v[1] += op == kOpEq;
        if (i1 < 0 || i1 >= v.n1 || i2 < 0 || i2 >= v.n2) return;   // past path 1: aligned, never shared; i2: the slice's bound
        if (kStore) {
            partner[i2] = (uint32_t)i1 | (op == kOpEq ? kPartnerEq : 0u);
        } else {
            const uint32_t w = partner[i2];
            const bool same = w != kNoPos && (w & ~kPartnerEq) == (uint32_t)i1;
            sum.v[2] += same;
            sum.v[3] += same && (w & kPartnerEq);
        }
    };
    MatchScan c1 = MatchScan::ident();
    for (int64_t base = 0; base < v.n2; base += kTile) {
        const int64_t s0 = base + (int64_t)threadIdx.x * kItems;
        uint32_t a[kItems];
        MatchScan agg = MatchScan::ident();
#pragma unroll
        for (uint32_t r = 0; r < kItems; ++r) {
            a[r] = kNoPos;
            if (s0 + r < v.n2) a[r] = pos[v.p2[s0 + r]];
            if (a[r] != kNoPos) agg = combine(agg, MatchScan{1, s0 + r, (int64_t)a[r]});
        }
        MatchScan tot1;
        MatchScan x = combine(c1, block_exclusive(agg, lds1, tot1));
        c1 = combine(c1, tot1);
#pragma unroll
        for (uint32_t r = 0; r < kItems; ++r) {
            if (a[r] == kNoPos) continue;
            match_tokens_at(v, x, s0 + r, (int64_t)a[r], tok);
            x = combine(x, MatchScan{1, s0 + r, (int64_t)a[r]});
        }
    }
    if (threadIdx.x == 0) {
        // the run after the last match, as in induced_runs_kernel
        const int64_t k = c1.cnt;
        const int64_t e_last = k > 0 ? k - 1 + (c1.best > 0 ? c1.best : 0) : -1;
        const int64_t g2 = v.n1 > e_last + 1 ? v.n1 - e_last - 1 : 0, g1 = v.n2 - 1 - c1.last;
        gap_run_tokens_at(v, e_last, c1.last, g1, g2, tok);
    }
    sum = block_sum4(sum, lds2);
    if (threadIdx.x != 0) return;
    uint64_t* mine = counts + 2 * job.text_cap;
    if (kStore) {
        mine[0] = sum.v[0];
        mine[1] = sum.v[1];
    } else {
        cl_pair_agreement r;
        r.aligned_a = mine[0]; r.aligned_b = sum.v[0]; r.shared = sum.v[2];
        r.eq_a = mine[1]; r.eq_b = sum.v[1]; r.shared_eq = sum.v[3];
        r.n1 = job.n1; r.n2 = job.n2;
        out[job.text_cap] = r;
    }
}
__global__ void __launch_bounds__(kThreads) induced_partner_kernel(const ClInducedJob* __restrict__ jobs, const uint32_t* __restrict__ path_nodes, uint64_t n_steps,
                                                                  const uint8_t* __restrict__ label, uint64_t n_nodes, const uint32_t* __restrict__ tables,
                                                                  uint32_t* __restrict__ partner, uint64_t* __restrict__ counts) {
    partner_agreement_walk<true>(jobs, path_nodes, n_steps, label, n_nodes, tables, partner, counts, nullptr);
}
__global__ void __launch_bounds__(kThreads) induced_agreement_kernel(const ClInducedJob* __restrict__ jobs, const uint32_t* __restrict__ path_nodes, uint64_t n_steps,
                                                                    const uint8_t* __restrict__ label, uint64_t n_nodes, const uint32_t* __restrict__ tables,
                                                                    const uint32_t* __restrict__ partner, const uint64_t* __restrict__ counts,
                                                                    cl_pair_agreement* __restrict__ out) {
    partner_agreement_walk<false>(jobs, path_nodes, n_steps, label, n_nodes, tables, const_cast<uint32_t*>(partner), const_cast<uint64_t*>(counts), out);
}

// pos[path1[i]] = i; a node met twice leaves one of its positions behind, which the check reads back
__global__ void induced_scatter_kernel(const uint32_t* __restrict__ p1, uint64_t n1, uint32_t* __restrict__ pos) {
    for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n1; i += (uint64_t)gridDim.x * blockDim.x) pos[p1[i]] = (uint32_t)i;
}
__global__ void induced_check_kernel(const uint32_t* __restrict__ p1, uint64_t n1, const uint32_t* __restrict__ pos, uint32_t* __restrict__ repeated) {
    for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n1; i += (uint64_t)gridDim.x * blockDim.x)
        if (pos[p1[i]] != (uint32_t)i) *repeated = 1;
}

}  // namespace

hipError_t cl_launch_induced_table(const uint32_t* p1, uint64_t n1, uint32_t* pos, uint64_t n_nodes, uint32_t* repeated, hipStream_t stream) {
    hipError_t e = hipMemsetD32Async((hipDeviceptr_t)pos, (int)kNoPos, n_nodes, stream);
    if (e != hipSuccess || n1 == 0) return e;
    const unsigned grid = (unsigned)std::min<uint64_t>((n1 + 255) / 256, 4096);
    hipLaunchKernelGGL(induced_scatter_kernel, dim3(grid), dim3(256), 0, stream, p1, n1, pos);
    hipLaunchKernelGGL(induced_check_kernel, dim3(grid), dim3(256), 0, stream, p1, n1, pos, repeated);
    return hipGetLastError();
}

hipError_t cl_launch_induced_runs(bool write, const ClInducedJob* jobs, uint32_t n_jobs, const uint32_t* path_nodes, uint64_t n_steps, const uint8_t* label,
                                  uint64_t n_nodes, const uint32_t* tables, int64_t* text_len, char* text, hipStream_t stream) {
    if (n_jobs == 0) return hipSuccess;
    if (write) hipLaunchKernelGGL(induced_runs_kernel<true>, dim3(n_jobs), dim3(kThreads), 0, stream, jobs, path_nodes, n_steps, label, n_nodes, tables, text_len, text);
    else hipLaunchKernelGGL(induced_runs_kernel<false>, dim3(n_jobs), dim3(kThreads), 0, stream, jobs, path_nodes, n_steps, label, n_nodes, tables, text_len, text);
    return hipGetLastError();
}

hipError_t cl_launch_induced_stats(const ClInducedJob* jobs, uint32_t n_jobs, const uint32_t* path_nodes, uint64_t n_steps, const uint8_t* label, uint64_t n_nodes,
                                   const uint32_t* tables, cl_pair_stats* stats, hipStream_t stream) {
    if (n_jobs == 0) return hipSuccess;
    hipLaunchKernelGGL(induced_stats_kernel, dim3(n_jobs), dim3(kThreads), 0, stream, jobs, path_nodes, n_steps, label, n_nodes, tables, stats);
    return hipGetLastError();
}

hipError_t cl_launch_induced_profile(const ClInducedJob* jobs, uint32_t n_jobs, const uint32_t* path_nodes, uint64_t n_steps, const uint8_t* label, uint64_t n_nodes,
                                     const uint32_t* tables, uint64_t window, cl_pair_window* windows, hipStream_t stream) {
    if (n_jobs == 0) return hipSuccess;
    hipLaunchKernelGGL(induced_profile_kernel, dim3(n_jobs), dim3(kThreads), 0, stream, jobs, path_nodes, n_steps, label, n_nodes, tables, window, windows);
    return hipGetLastError();
}

hipError_t cl_launch_induced_events(bool write, const ClInducedJob* jobs, uint32_t n_jobs, const uint32_t* path_nodes, uint64_t n_steps, const uint8_t* label,
                                    uint64_t n_nodes, const uint32_t* tables, uint64_t min_len, int64_t* n_events, cl_gap_event* events, hipStream_t stream) {
    if (n_jobs == 0) return hipSuccess;
    if (write) hipLaunchKernelGGL(induced_events_kernel<true>, dim3(n_jobs), dim3(kThreads), 0, stream, jobs, path_nodes, n_steps, label, n_nodes, tables, min_len, n_events, events);
    else hipLaunchKernelGGL(induced_events_kernel<false>, dim3(n_jobs), dim3(kThreads), 0, stream, jobs, path_nodes, n_steps, label, n_nodes, tables, min_len, n_events, events);
    return hipGetLastError();
}

hipError_t cl_launch_induced_partner(const ClInducedJob* jobs, uint32_t n_jobs, const uint32_t* path_nodes, uint64_t n_steps, const uint8_t* label, uint64_t n_nodes,
                                     const uint32_t* tables, uint32_t* partner, uint64_t* counts, hipStream_t stream) {
    if (n_jobs == 0) return hipSuccess;
    hipLaunchKernelGGL(induced_partner_kernel, dim3(n_jobs), dim3(kThreads), 0, stream, jobs, path_nodes, n_steps, label, n_nodes, tables, partner, counts);
    return hipGetLastError();
}

hipError_t cl_launch_induced_agreement(const ClInducedJob* jobs, uint32_t n_jobs, const uint32_t* path_nodes, uint64_t n_steps, const uint8_t* label, uint64_t n_nodes,
                                       const uint32_t* tables, const uint32_t* partner, const uint64_t* counts, cl_pair_agreement* out, hipStream_t stream) {
    if (n_jobs == 0) return hipSuccess;
    hipLaunchKernelGGL(induced_agreement_kernel, dim3(n_jobs), dim3(kThreads), 0, stream, jobs, path_nodes, n_steps, label, n_nodes, tables, partner, counts, out);
    return hipGetLastError();
}
