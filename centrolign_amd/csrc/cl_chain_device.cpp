// cl_chain_device.cpp — the chaining DP's driver (chain_dp_batch) and its device phases (chain_dp.hpp: ChainDev): upload, far-pass setup, the enqueue loop,
// the wait and the download.  The kernels are chain_kernels.hip, chain_walk2.hip, chain_far.hip and chain_sort.hip.
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <mutex>
#include <unistd.h>

#include "chain_dp.hpp"

namespace clchain {

const ChainSwitches& chain_switches() {
    static const ChainSwitches sw = [] {
        const char *par_min = getenv("CL_CHAIN_PAR_RECORDS_MIN"), *fold = getenv("CL_CHAIN_WALK_FOLD"), *group = getenv("CL_CHAIN_GROUP_PATH"), *walk2 = getenv("CL_CHAIN_WALK2"),
                   *qpt = getenv("CL_CHAIN_WALK2_QPT"), *w2max = getenv("CL_CHAIN_WALK2_MAX"), *helpers = getenv("CL_CHAIN_WALK2_HELPERS"), *lag = getenv("CL_CHAIN_FAR_LAG"),
                   *skip = getenv("CL_CHAIN_FAR_ARENA_SKIP"), *ext = getenv("CL_CHAIN_EXT_EVENTS"), *split = getenv("CL_CHAIN_NEAR_SPLIT");
        ChainSwitches s{};
        s.par_records_min = par_min ? (uint64_t)atoll(par_min) : (uint64_t)(1u << 20);
        s.dense_queries = getenv("CL_CHAIN_DENSE_QUERIES") != nullptr;
        s.old_walk = getenv("CL_CHAIN_OLD_WALK") != nullptr;
        { const int v = fold ? atoi(fold) : 0; s.walk_fold = v == 2 || v == 3 ? (uint32_t)v : 0u; }
        s.group_forced = group && group[0] == 'f';
        s.group_path = !group || group[0] != '0';
        s.walk2 = !walk2 || walk2[0] != '0';
        s.walk2_qpt = qpt && qpt[0] == '2' ? 2u : 1u;
        { const int v = w2max ? atoi(w2max) : 0; s.walk2_max = v > 0 ? (uint32_t)v : 8u; }
        s.walk2_helpers = helpers ? atoi(helpers) : -1;
        s.walk_reduce = getenv("CL_CHAIN_WALK_REDUCE");
        s.walk2_debug = getenv("CL_CHAIN_WALK2_DEBUG") != nullptr;
        s.no_far = getenv("CL_CHAIN_NO_FAR_PRUNE") != nullptr;
        { const int v = lag ? atoi(lag) : 0; s.far_lag = (uint32_t)(v >= 1 && v <= (int)kFarLag ? v : 0); }
        s.far_arena_skip = skip ? (uint64_t)strtoull(skip, nullptr, 10) & ~7ull : 0ull;
        s.seal_wave = getenv("CL_CHAIN_SEAL_WAVE") != nullptr;
        s.far_mode = getenv("CL_CHAIN_FAR_MODE");
        s.ext_events = !ext || ext[0] != '0';
        s.far_early = getenv("CL_CHAIN_FAR_WAIT_LATE") == nullptr;
        s.skip_far = getenv("CL_CHAIN_DEBUG_SKIP_FAR") != nullptr;
        s.near_split = split && split[0] == '1';
        s.debug_stall = getenv("CL_CHAIN_DEBUG_STALL");
        s.lazy_acc = getenv("CL_CHAIN_LAZY_ACC");
        return s;
    }();
    return sw;
}

// The walk's workgroups take a compute unit each (1 024 threads, up to 120 KB of LDS) and wait for one another: the DPs of several contexts of ONE process that are in
// flight together must fit the device together, or a walk gives up its bounded wait and the whole DP is repeated on the per-block kernels — 184 s instead of 11 s for a
// 156-combination merge of 50 x 1 Mbp beside three other workers (round 6, profiles/r06_configs4.json).  So a DP books the compute units its walk launches need before it
// enqueues them and gives them back when the device is done with it; a DP that does not fit beside the ones in flight waits for them (two 156-combination walks never
// fitted 256 units: they took turns by stalling).  Per device; the stall fallback stays for what is left (other processes on the device).
namespace {
struct WalkUnits {
    std::mutex m;
    std::condition_variable cv;
    uint32_t in_use[16] = {};
    static constexpr uint32_t kBudget = 232;   // of 256: the far / near / seal launches of the same DPs need room as well
    void take(int device, uint32_t need) {
        need = std::min(need, kBudget);
        std::unique_lock<std::mutex> lock(m);
        uint32_t& u = in_use[device & 15];
        cv.wait(lock, [&] { return u == 0 || u + need <= kBudget; });
        u += need;
    }
    void give(int device, uint32_t need) {
        need = std::min(need, kBudget);
        { std::lock_guard<std::mutex> lock(m); in_use[device & 15] -= need; }
        cv.notify_all();
    }
};
WalkUnits g_walk_units;
thread_local bool g_walk_exclusive = false;   // this thread's DP books the whole budget (the second attempt after a stall)
}  // namespace
// the booking of one DP: handed back right after the streams have run dry (ChainDev::wait), or at scope exit on an error
struct UnitsHeld { int device; uint32_t n; bool held; ~UnitsHeld() { if (held) g_walk_units.give(device, n); } };

int chain_hip_fail(cl_context* ctx, hipError_t e, const char* what) {
    cl_set_error(ctx, "%s failed: %s", what, hipGetErrorString(e));
    return e == hipErrorOutOfMemory ? CL_ERR_OUT_OF_MEMORY : CL_ERR_HIP;
}

ChainDev::~ChainDev() {
    if (ev0) (void)hipEventDestroy(ev0);
    if (ev1) (void)hipEventDestroy(ev1);
    for (auto e : ev_intra) if (e) (void)hipEventDestroy(e);
    for (auto e : ev_far) if (e) (void)hipEventDestroy(e);
    if (ctx->poisoned) return;   // (device buffers of this DP are left to the stuck stream: releasing them would wait for it)
    cl_ctx_quiesce(ctx);   // once, for the ~40 blocks that go back to the pool below
    for (ComboDev& c : cd) c.release(true);
    for (DevBuf<float>* b : {&d_weight, &d_init, &d_dp, &d_blk_val}) b->release(true);
    for (DevBuf<uint32_t>* b : {&d_rec_off, &d_rec_combo, &d_rec_pos, &d_group, &d_grp_base, &d_grp_total, &d_group_end, &d_status, &d_xred, &d_blk_rec, &d_blk_q, &d_blk_own, &d_ctags, &i_in, &i_out,
                                &d_far_base, &d_far_arena, &d_far_tab, &d_seal_items}) b->release(true);
    for (DevBuf<unsigned long long>* b : {&d_xch, &d_xdp, &d_hacc}) b->release(true);
    for (DevBuf<int>* b : {&d_dp_enc, &d_row, &d_blk_acc, &k_in, &k_out, &d_far_rec}) b->release(true);
    for (DevBuf<char>* b : {&d_pack, &vtemp, &d_far_temp}) b->release(true);
    d_combos.release(true);
    for (auto& b : d_fa) b.release(true);
    for (auto& b : d_far_perm) b.release(true);
    for (auto& b : d_far_u32) b.release(true);
}

// A SMALL DP (the thousands of realignments of a polishing step hold a few hundred match pairs each: 113 copies and 126 stream waits per merge,
// most of its time) packs every array below into ONE device block, filled on the host and sent with one copy; the DP values and every
// combination's query results lie together at its end and come back with one copy.  Large DPs keep an allocation and a copy per array.
struct PackLayout {
    struct PackOff { size_t rec_s, ins_t, off, sigma, prefix, qt, qoff, q, val, own, acc; };
    std::vector<PackOff> po;
    size_t o_combos = 0, o_weight = 0, o_init = 0, o_rec_off = 0, o_rec_combo = 0, o_rec_pos = 0, o_xch = 0, o_status = 0, o_dp = 0, total = 0;
    void lay_out(const ChainProblem& P, bool use_walk) {
        po.assign(P.combos.size(), PackOff{});
        total = 0;
        const uint64_t M = P.M;
        const auto& combos = P.combos;
        auto reserve = [&](size_t bytes) { const size_t at = total; total += (bytes + 255) & ~(size_t)255; return at; };
        for (size_t ci = 0; ci < combos.size(); ++ci) {
            const Combo& c = combos[ci];
            const size_t n = c.rec_s.size();
            po[ci] = PackOff{reserve(n * 4), reserve(n * 4), reserve(n * 4), reserve(n * 4), reserve(c.prefix.size() * 4), reserve(M * 4), reserve(M * 4), reserve(M * 4),
                             0, use_walk ? reserve(M * 4) : 0, 0};
        }
        o_combos = reserve(combos.size() * sizeof(ClChainCombo)); o_weight = reserve(M * 4); o_init = reserve(M * 4); o_rec_off = reserve((M + 1) * 4);
        o_rec_combo = reserve(P.rec_combo.size() * 4); o_rec_pos = reserve(P.rec_pos.size() * 4);
        o_xch = use_walk ? reserve(combos.size() * kChainMacro * sizeof(unsigned long long)) : 0; o_status = use_walk ? reserve(32 * sizeof(uint32_t)) : 0;   // zeroed
        o_dp = reserve(M * 4);   // what comes back: the DP values, every combination's stored values (the traceback's value index) and query results
        for (size_t ci = 0; ci < combos.size(); ++ci) po[ci].val = reserve(7 * combos[ci].rec_s.size() * 4);
        for (size_t ci = 0; ci < combos.size(); ++ci) po[ci].acc = reserve(M * 7 * 4);
    }
};

// (the pack is laid out here: whether a DP is small enough for it depends on the arrays the walk needs)
static ChainPath choose_path(const ChainProblem& P, bool allow_walk, PackLayout& pack) {
    const ChainSwitches& sw = P.sw;
    const size_t C = P.combos.size();
    ChainPath path;
    // the walk kernel (one workgroup per combination, all resident) replaces the per-block intra launches up to
    // kChainWalkMaxCombos combinations; CL_CHAIN_OLD_WALK=1 forces the per-block path (A/B measurements).
    // Beyond kChainWalkMaxCombos a workgroup of the walk takes two or three combinations (chain_walk_fold_kernel: 768 combinations, a root of
    // 27 + 27 paths); CL_CHAIN_WALK_FOLD=2/3 folds smaller DPs too (tests)
    path.walk_fold = std::max<uint32_t>(C > 1 ? sw.walk_fold : 0u, (uint32_t)((C + kChainWalkMaxCombos - 1) / kChainWalkMaxCombos));
    path.use_walk = allow_walk && path.walk_fold <= 3 && !sw.old_walk && !sw.group_forced;
    pack.lay_out(P, path.use_walk);
    path.packed = pack.total <= (2u << 20) && C != 0;
    // the walk over several compute units per combination (chain_walk2.hip: a main workgroup with a window of 128 x qpt queries and helper
    // workgroups for the rest of the macro-block) wherever main + helpers of every combination fit the chip at one workgroup per compute unit;
    // CL_CHAIN_WALK2=0 keeps chain_walk_kernel (A/B), CL_CHAIN_WALK2_QPT=1/2 the window, CL_CHAIN_WALK2_HELPERS=n the helpers (0: the main
    // workgroup evaluates everything itself out of LDS — the path it takes when a helper is late)
    // (window: 2 x 1 Mbp affine / gap-free DP 157 / 90 ms with 128 queries, 165 / 92 ms with 256; 10 x 1 Mbp merges of 1 / 4 / 25 combinations, device time of
    // both DPs on one context: 165 / 285 / 1 158 ms here against 273 / 390 / 874 ms on chain_walk_kernel — at 25 combinations 200 workgroups of 1 024 threads
    // and 120 KB of LDS leave the far and near launches too little of the chip, so the one-workgroup walk stays above CL_CHAIN_WALK2_MAX combinations)
    path.walk2_qpt = sw.walk2_qpt;
    path.walk2_help = cl_chain_walk2_helpers(path.walk2_qpt);
    path.use_walk2 = path.use_walk && path.walk_fold <= 1 && !path.packed && sw.walk2 && C <= sw.walk2_max && ((C + 7) & ~(size_t)7) * (1 + path.walk2_help) <= 256;
    if (sw.walk2_helpers >= 0) path.walk2_help = (uint32_t)std::min(sw.walk2_helpers, 7);
    // the exchange between the walk's workgroups: granule sweep for few combinations, reduction for many (CL_CHAIN_WALK_REDUCE=0/1 pins it: A/B)
    path.walk_reduce = path.use_walk && C > 1 && (path.walk_fold > 1 || (sw.walk_reduce ? sw.walk_reduce[0] == '1' : C > kChainWalkSweepCombos));
    // more combinations than the walk kernels take: group by group, parallel over the combinations (chain_kernels.hip: chain_group_*; CL_CHAIN_GROUP_PATH=0: the one-workgroup
    // per-block kernels of rounds 1-5, A/B; =force: every DP, whatever its combinations (tests))
    path.group_path = sw.group_forced || (sw.group_path && path.walk_fold > 3 && !sw.old_walk);
    // far launches in flight: 4 by default in the affine DP.  Measured: the 2 x 1 Mbp affine DP's device time is 1045 / 540 / 393 / 372 / 340 ms at 1 / 2 / 3 /
    // 4 / 6 in flight (a far launch is 1024 queries, too few to fill the chip alone); the 10 x 1 Mbp MSA with four worker contexts is
    // within 3 % for 2, 3 and 4 and 5 % slower at 6 (the near pass grows with the lag).  CL_CHAIN_FAR_LAG=1..8 for measurements
    // The gap-free DP's far pass opens a tenth of the leaves, so its near pass is what grows: 175 ms at 2 in flight, 253 ms at 4 — it keeps 2
    path.far_lag = sw.far_lag ? sw.far_lag : 2u;   // round 3 (8-ary search trees, leaves scanned by eight lanes): 2 x 1 Mbp affine 313 / 396 / 341 / 393 ms at 2 / 3 / 4 / 6; root of 10 x 1 Mbp 1.22 s at 2, 1.39 s at 4
    const uint32_t n_macro_all = (uint32_t)((P.M + kChainMacro - 1) / kChainMacro);
    path.use_far = path.use_walk && !sw.no_far && n_macro_all >= path.far_lag + 3;
    // Two streams.  The context's stream is the sequential one: per block b the one-workgroup walk of the block, preceded by
    // the "near" pass over the blocks the far launch could not see yet (folded into the walk kernel when there is a single
    // combination).  The bulk is evaluated on an auxiliary stream ("far"): one launch per block (kChainFarGroup = 1), which
    // reads the blocks before b - 1, final once walk(b - 2) is done.  Consecutive far launches alternate between
    // kChainFarStreams auxiliary streams: while their grids are small their latency floors overlap
    // the stored query results of every combination (7 per pair): into the context's page-locked area when it can be had — 35 MB per
    // combination at 1.25 M pairs, 25 combinations at the root of a 10-sequence tree.  Beyond kLazyAccBytes (a root of 25 + 25 paths: 625
    // combinations, 21.9 GB at 1.25 M pairs — 4.3 s of copies into 22 GB of pageable memory, more than the DP itself) nothing is downloaded: the
    // traceback reads the results of the pair it stands on and nothing else, so it fetches that row (7 x combinations words) step by step
    // (chain_acc_row_kernel; a launch, a 17 KB copy and a wait per chain step).  CL_CHAIN_LAZY_ACC=0/1 pins the choice (tests).
    constexpr size_t kLazyAccBytes = 1536ull << 20;
    path.lazy_acc = !path.packed && (sw.lazy_acc ? sw.lazy_acc[0] == '1' : C * (size_t)P.M * 7 * sizeof(int) > kLazyAccBytes);
    return path;
}

int ChainDev::upload_packed(const ChainProblem& P, const ChainPath& path, const PackLayout& pack) {
    std::vector<ClChainCombo> hc(P.combos.size());
    CL_CHAIN_TRY(d_pack.alloc(ctx, pack.total));
    char* dev = d_pack.p;
    std::vector<char> stage(pack.total);
    auto put = [&](size_t at, const void* src, size_t bytes) { if (bytes) memcpy(stage.data() + at, src, bytes); };
    for (size_t ci = 0; ci < P.combos.size(); ++ci) {
        const Combo& c = P.combos[ci];
        ComboDev& dc = cd[ci];
        const size_t n = c.rec_s.size();
        const PackLayout::PackOff& o = pack.po[ci];
        put(o.rec_s, c.rec_s.data(), n * 4); put(o.ins_t, c.ins_t.data(), n * 4); put(o.off, c.off.data(), n * 4); put(o.sigma, c.sigma.data(), n * 4);
        put(o.prefix, c.prefix.data(), c.prefix.size() * 4); put(o.qt, c.qt, P.M * 4); put(o.qoff, c.qoff, P.M * 4); put(o.q, c.q, P.M * 4);
        if (path.use_walk) memset(stage.data() + o.own, 0xFF, P.M * 4);
        int* a = reinterpret_cast<int*>(stage.data() + o.acc);
        for (size_t i = 0; i < (size_t)P.M * 7; ++i) a[i] = enc(CL_CHAIN_NEG);
        dc.d_rec_s.view((uint32_t*)(dev + o.rec_s), n); dc.d_ins_t.view((uint32_t*)(dev + o.ins_t), n); dc.d_off.view((uint32_t*)(dev + o.off), n);
        dc.d_sigma.view((int32_t*)(dev + o.sigma), n); dc.d_prefix.view((uint32_t*)(dev + o.prefix), c.prefix.size());
        dc.d_qt.view((uint32_t*)(dev + o.qt), P.M); dc.d_qoff.view((uint32_t*)(dev + o.qoff), P.M); dc.d_q.view((int32_t*)(dev + o.q), P.M);
        dc.d_val.view((float*)(dev + o.val), 7 * n); dc.d_acc.view((int*)(dev + o.acc), (size_t)P.M * 7);
        if (path.use_walk) dc.d_own_rec.view((uint32_t*)(dev + o.own), P.M);
        hc[ci] = ClChainCombo{(uint32_t)n, dc.d_rec_s.p, dc.d_ins_t.p, dc.d_off.p, dc.d_sigma.p, dc.d_val.p, dc.d_prefix.p,
                              dc.d_qt.p, dc.d_qoff.p, dc.d_q.p, dc.d_acc.p, dc.d_own_rec.p};
    }
    put(pack.o_combos, hc.data(), hc.size() * sizeof(ClChainCombo)); put(pack.o_weight, P.weight.data(), P.M * 4); put(pack.o_init, P.init_w.data(), P.M * 4);
    put(pack.o_rec_off, P.rec_off.data(), (P.M + 1) * 4); put(pack.o_rec_combo, P.rec_combo.data(), P.rec_combo.size() * 4); put(pack.o_rec_pos, P.rec_pos.data(), P.rec_pos.size() * 4);
    d_combos.view((ClChainCombo*)(dev + pack.o_combos), hc.size()); d_weight.view((float*)(dev + pack.o_weight), P.M); d_init.view((float*)(dev + pack.o_init), P.M);
    d_dp.view((float*)(dev + pack.o_dp), P.M);
    if (path.use_walk) { d_xch.view((unsigned long long*)(dev + pack.o_xch), P.combos.size() * kChainMacro); d_status.view((uint32_t*)(dev + pack.o_status), 32); }
    d_rec_off.view((uint32_t*)(dev + pack.o_rec_off), P.M + 1); d_rec_combo.view((uint32_t*)(dev + pack.o_rec_combo), P.rec_combo.size()); d_rec_pos.view((uint32_t*)(dev + pack.o_rec_pos), P.rec_pos.size());
    pack_dp_off = pack.o_dp;
    pack_acc_stride = P.combos.size() > 1 ? pack.po[1].acc - pack.po[0].acc : (((size_t)P.M * 7 * 4 + 255) & ~(size_t)255);
    pack_down_bytes = pack.total - pack.o_dp;
    if (hipMemcpyAsync(dev, stage.data(), pack.total, hipMemcpyHostToDevice, ctx->stream) != hipSuccess || hipStreamSynchronize(ctx->stream) != hipSuccess) {
        cl_set_error(ctx, "upload failed"); return CL_ERR_HIP;
    }
    return CL_OK;
}

// a few blocks instead of eleven allocations and eight copies per combination (625 combinations: 7 000 allocations, 5 000 copies)
int ChainDev::upload_factored(const ChainProblem& P, const ChainPath& path) {
    std::vector<ClChainCombo> hc(P.combos.size());
    const size_t C = P.combos.size();
    std::vector<size_t> rbase(C + 1, 0);
    for (size_t ci = 0; ci < C; ++ci) rbase[ci + 1] = rbase[ci] + P.combos[ci].rec_s.size();
    const size_t R_all = rbase[C], pw = (size_t)P.n_blocks + 1;
    ClRawVec<uint32_t> stage(4 * R_all + C * pw);
    cl_parallel_for(C, [&](uint64_t c_begin, uint64_t c_end) {
        for (uint64_t ci = c_begin; ci < c_end; ++ci) {
            const Combo& c = P.combos[ci];
            const size_t n = c.rec_s.size();
            if (n) {
                memcpy(&stage[rbase[ci]], c.rec_s.data(), n * 4); memcpy(&stage[R_all + rbase[ci]], c.ins_t.data(), n * 4);
                memcpy(&stage[2 * R_all + rbase[ci]], c.off.data(), n * 4); memcpy(&stage[3 * R_all + rbase[ci]], c.sigma.data(), n * 4);
            }
            memcpy(&stage[4 * R_all + ci * pw], c.prefix.data(), pw * 4);
        }
    }, 1);
    std::vector<uint32_t> ctags(2 * C);
    for (size_t ci = 0; ci < C; ++ci) { ctags[2 * ci] = P.combos[ci].p1; ctags[2 * ci + 1] = P.combos[ci].p2; }
    CL_CHAIN_TRY(d_blk_rec.upload_async(ctx, stage));
    CL_CHAIN_TRY(d_ctags.upload_async(ctx, ctags));
    CL_CHAIN_TRY(d_fa[0].upload_async(ctx, P.fa_qt)); CL_CHAIN_TRY(d_fa[1].upload_async(ctx, P.fb_qoff));
    if (!P.sparse) { CL_CHAIN_TRY(d_fa[2].upload_async(ctx, P.fa_d)); CL_CHAIN_TRY(d_fa[3].upload_async(ctx, P.fb_d)); }
    CL_CHAIN_TRY(d_blk_val.alloc(ctx, 7 * R_all));
    CL_CHAIN_TRY(d_blk_q.alloc(ctx, 3 * C * (size_t)P.M));
    CL_CHAIN_TRY(d_blk_acc.alloc(ctx, C * (size_t)P.M * 7));
    CL_CHAIN_TRY(d_blk_own.alloc(ctx, C * (size_t)P.M));
    if (hipMemsetD32Async((hipDeviceptr_t)d_blk_acc.p, enc(CL_CHAIN_NEG), C * (size_t)P.M * 7, ctx->stream) != hipSuccess ||
        hipMemsetAsync(d_blk_own.p, 0xFF, C * (size_t)P.M * sizeof(uint32_t), ctx->stream) != hipSuccess) { cl_set_error(ctx, "hipMemsetAsync failed"); return CL_ERR_HIP; }
    if (cl_chain_expand_queries(d_fa[0].p, d_fa[2].p, d_fa[1].p, d_fa[3].p, d_ctags.p, (uint32_t)C, (uint32_t)P.M, d_blk_q.p, d_blk_q.p + C * (size_t)P.M,
                                (int32_t*)(d_blk_q.p + 2 * C * (size_t)P.M), ctx->stream) != hipSuccess) { cl_set_error(ctx, "query expansion failed"); return CL_ERR_HIP; }
    for (size_t ci = 0; ci < C; ++ci) {
        const Combo& c = P.combos[ci];
        ComboDev& dc = cd[ci];
        const size_t n = c.rec_s.size();
        dc.d_rec_s.view(d_blk_rec.p + rbase[ci], n); dc.d_ins_t.view(d_blk_rec.p + R_all + rbase[ci], n); dc.d_off.view(d_blk_rec.p + 2 * R_all + rbase[ci], n);
        dc.d_sigma.view((int32_t*)(d_blk_rec.p + 3 * R_all + rbase[ci]), n); dc.d_prefix.view(d_blk_rec.p + 4 * R_all + ci * pw, pw);
        dc.d_qt.view(d_blk_q.p + ci * (size_t)P.M, P.M); dc.d_qoff.view(d_blk_q.p + (C + ci) * (size_t)P.M, P.M); dc.d_q.view((int32_t*)(d_blk_q.p + (2 * C + ci) * (size_t)P.M), P.M);
        dc.d_val.view(d_blk_val.p + 7 * rbase[ci], 7 * n); dc.d_acc.view(d_blk_acc.p + ci * (size_t)P.M * 7, (size_t)P.M * 7);
        if (path.use_walk) dc.d_own_rec.view(d_blk_own.p + ci * (size_t)P.M, P.M);
        hc[ci] = ClChainCombo{(uint32_t)n, dc.d_rec_s.p, dc.d_ins_t.p, dc.d_off.p, dc.d_sigma.p, dc.d_val.p, dc.d_prefix.p,
                              dc.d_qt.p, dc.d_qoff.p, dc.d_q.p, dc.d_acc.p, dc.d_own_rec.p};
    }
    CL_CHAIN_TRY(d_combos.upload_async(ctx, hc));
    CL_CHAIN_TRY(d_weight.upload_async(ctx, P.weight));
    CL_CHAIN_TRY(d_init.upload_async(ctx, P.init_w));
    CL_CHAIN_TRY(d_dp.alloc(ctx, P.M));
    CL_CHAIN_TRY(d_rec_off.upload_async(ctx, P.rec_off)); CL_CHAIN_TRY(d_rec_combo.upload_async(ctx, P.rec_combo)); CL_CHAIN_TRY(d_rec_pos.upload_async(ctx, P.rec_pos));
    if (hipStreamSynchronize(ctx->stream) != hipSuccess) { cl_set_error(ctx, "upload failed"); return CL_ERR_HIP; }
    return CL_OK;
}

int ChainDev::upload_separate(const ChainProblem& P, const ChainPath& path) {
    std::vector<ClChainCombo> hc(P.combos.size());
    for (size_t ci = 0; ci < P.combos.size(); ++ci) {
        const Combo& c = P.combos[ci];
        ComboDev& dc = cd[ci];
        // (enqueued only: one wait for all of them below — a merge of small graphs used to spend most of its time in these round trips)
        CL_CHAIN_TRY(dc.d_rec_s.upload_async(ctx, c.rec_s)); CL_CHAIN_TRY(dc.d_ins_t.upload_async(ctx, c.ins_t)); CL_CHAIN_TRY(dc.d_off.upload_async(ctx, c.off));
        CL_CHAIN_TRY(dc.d_sigma.upload_async(ctx, c.sigma)); CL_CHAIN_TRY(dc.d_prefix.upload_async(ctx, c.prefix));
        struct Slice { const void* p; size_t n; const void* data() const { return p; } size_t size() const { return n; } bool empty() const { return n == 0; } };
        CL_CHAIN_TRY(dc.d_qt.upload_async(ctx, Slice{c.qt, (size_t)P.M})); CL_CHAIN_TRY(dc.d_qoff.upload_async(ctx, Slice{c.qoff, (size_t)P.M})); CL_CHAIN_TRY(dc.d_q.upload_async(ctx, Slice{c.q, (size_t)P.M}));
        CL_CHAIN_TRY(dc.d_val.alloc(ctx, 7 * c.rec_s.size()));
        CL_CHAIN_TRY(dc.d_acc.alloc(ctx, P.M * 7));
        if (hipMemsetD32Async((hipDeviceptr_t)dc.d_acc.p, enc(CL_CHAIN_NEG), P.M * 7, ctx->stream) != hipSuccess) { cl_set_error(ctx, "hipMemsetD32Async failed"); return CL_ERR_HIP; }
        if (path.use_walk) {
            CL_CHAIN_TRY(dc.d_own_rec.alloc(ctx, P.M));
            if (hipMemsetAsync(dc.d_own_rec.p, 0xFF, P.M * sizeof(uint32_t), ctx->stream) != hipSuccess) { cl_set_error(ctx, "hipMemsetAsync failed"); return CL_ERR_HIP; }
        }
        hc[ci] = ClChainCombo{(uint32_t)c.rec_s.size(), dc.d_rec_s.p, dc.d_ins_t.p, dc.d_off.p, dc.d_sigma.p, dc.d_val.p, dc.d_prefix.p,
                              dc.d_qt.p, dc.d_qoff.p, dc.d_q.p, dc.d_acc.p, dc.d_own_rec.p};
    }
    CL_CHAIN_TRY(d_combos.upload_async(ctx, hc));
    CL_CHAIN_TRY(d_weight.upload_async(ctx, P.weight));
    CL_CHAIN_TRY(d_init.upload_async(ctx, P.init_w));
    CL_CHAIN_TRY(d_dp.alloc(ctx, P.M));
    CL_CHAIN_TRY(d_rec_off.upload_async(ctx, P.rec_off)); CL_CHAIN_TRY(d_rec_combo.upload_async(ctx, P.rec_combo)); CL_CHAIN_TRY(d_rec_pos.upload_async(ctx, P.rec_pos));
    if (hipStreamSynchronize(ctx->stream) != hipSuccess) { cl_set_error(ctx, "upload failed"); return CL_ERR_HIP; }
    return CL_OK;
}

int ChainDev::upload_groups(const ChainProblem& P, const ChainPath& path) {
    // groups = maximal runs (in depth order) of pairs none of which can precede another: a predecessor m of m' ends
    // strictly before m' starts, so depth(b1(m')) >= depth(b1(m)) + len(m); a run is closed as soon as a pair starts at or
    // beyond the smallest depth(b1) + len of the run.  The device finalises a whole group at once.
    std::vector<uint32_t> group(P.M);
    std::vector<std::vector<uint32_t>> set_len(P.K);
    group_first.clear();
    for (size_t k = 0; k < P.K; ++k) {
        if (P.sc[k].pair_hi == P.sc[k].pair_lo) continue;
        const SetView ms(P.subs[k]);
        set_len[k].resize(P.subs[k].num_match_sets);
        for (uint64_t st = 0; st < P.subs[k].num_match_sets; ++st)
            if (ms.n_walks(0, st)) set_len[k][st] = (uint32_t)ms.length(st);
    }
    uint32_t gid = 0;
    uint64_t min_end = 0;
    for (uint32_t s = 0; s < P.M; ++s) {
        const Pair& p = P.pairs[P.by_s[s]];
        const uint64_t start = P.sc[p.sub].depth1[p.b1], end = start + set_len[p.sub][p.set];
        if (s == 0) min_end = end;
        else if (start >= min_end) { ++gid; min_end = end; }
        else min_end = std::min(min_end, end);
        group[s] = gid;
        if (s == 0 || group[s] != group[s - 1]) group_first.push_back(s);
    }
    group_first.push_back((uint32_t)P.M);
    if (P.timing) {   // groups per block of kChainBlock pairs (each costs the sequential kernel two barriers + one LDS broadcast)
        std::vector<uint32_t> hist;
        for (uint64_t b0 = 0; b0 < P.M; b0 += kChainBlock) {
            const uint64_t b1 = std::min<uint64_t>(P.M, b0 + kChainBlock);
            const uint32_t g = group[b1 - 1] - group[b0] + 1;
            if (hist.size() <= g) hist.resize(g + 1, 0);
            ++hist[g];
        }
        fprintf(stderr, "[chain_dp_batch]   %u groups; groups per block:", gid + 1);
        for (size_t g = 0; g < hist.size(); ++g) if (hist[g]) fprintf(stderr, " %zu:%u", g, hist[g]);
        fprintf(stderr, "\n");
    }
    CL_CHAIN_TRY(d_group.upload_async(ctx, group));       // (these four copies are waited for together at the end of the block)
    std::vector<uint32_t> group_end;
    if (path.use_walk) {
        group_end.resize(P.M);
        for (uint64_t s1 = P.M; s1 > 0;) {
            uint64_t s0 = s1 - 1;
            while (s0 > 0 && group[s0 - 1] == group[s1 - 1]) --s0;
            for (uint64_t s = s0; s < s1; ++s) group_end[s] = (uint32_t)s1;
            s1 = s0;
        }
        CL_CHAIN_TRY(d_group_end.upload_async(ctx, group_end));
        if (path.use_walk2) {
            CL_CHAIN_TRY(d_xdp.alloc(ctx, P.combos.size() * kChainMacro));
            CL_CHAIN_TRY(d_hacc.alloc(ctx, P.combos.size() * kChainMacro * 8));
            if (hipMemsetAsync(d_xdp.p, 0, P.combos.size() * kChainMacro * sizeof(unsigned long long), ctx->stream) != hipSuccess ||
                hipMemsetAsync(d_hacc.p, 0, P.combos.size() * kChainMacro * 8 * sizeof(unsigned long long), ctx->stream) != hipSuccess) { cl_set_error(ctx, "hipMemsetAsync failed"); return CL_ERR_HIP; }
        }
        if (!d_pack.p) {   // (a small DP's pack holds them, zeroed)
            CL_CHAIN_TRY(d_xch.alloc(ctx, P.combos.size() * kChainMacro));
            CL_CHAIN_TRY(d_status.alloc(ctx, 32));
            if (hipMemsetAsync(d_xch.p, 0, P.combos.size() * kChainMacro * sizeof(unsigned long long), ctx->stream) != hipSuccess ||
                hipMemsetAsync(d_status.p, 0, 32 * sizeof(uint32_t), ctx->stream) != hipSuccess) { cl_set_error(ctx, "hipMemsetAsync failed"); return CL_ERR_HIP; }
        }
        if (path.walk_reduce) {
            CL_CHAIN_TRY(d_xred.alloc(ctx, 2 * P.M));
            if (hipMemsetAsync(d_xred.p, 0, 2 * P.M * sizeof(uint32_t), ctx->stream) != hipSuccess) { cl_set_error(ctx, "hipMemsetAsync failed"); return CL_ERR_HIP; }
        }
    }
    // LDS slots of the sequential kernel: records of a (block, group) are laid out in pair order
    std::vector<uint32_t> grp_base(P.M), grp_total(P.M);
    for (uint64_t s0 = 0; s0 < P.M;) {
        const uint64_t block_end = std::min<uint64_t>(P.M, (s0 / kChainBlock + 1) * kChainBlock);
        uint64_t s1 = s0;
        while (s1 < block_end && group[s1] == group[s0]) ++s1;
        const uint32_t total = P.rec_off[s1] - P.rec_off[s0];
        for (uint64_t s = s0; s < s1; ++s) { grp_base[s] = P.rec_off[s] - P.rec_off[s0]; grp_total[s] = total; }
        s0 = s1;
    }
    CL_CHAIN_TRY(d_grp_base.upload_async(ctx, grp_base));
    CL_CHAIN_TRY(d_grp_total.upload_async(ctx, grp_total));
    if (hipStreamSynchronize(ctx->stream) != hipSuccess) { cl_set_error(ctx, "upload failed"); return CL_ERR_HIP; }
    if (path.group_path) {
        std::vector<int> dp0(P.M);
        for (uint64_t s2 = 0; s2 < P.M; ++s2) dp0[s2] = enc(P.init_w[s2]);
        CL_CHAIN_TRY(d_dp_enc.upload(ctx, dp0));
    }
    return CL_OK;
}

void ChainDev::fill_device(const ChainProblem& P, const ChainPath& path) {
    const ChainSwitches& sw = P.sw;
    D.n_pairs = (uint32_t)P.M;
    D.n_combos = (uint32_t)P.combos.size();
    D.combos = d_combos.p;
    D.weight = d_weight.p;
    D.init = d_init.p;
    D.dp = d_dp.p;
    D.rec_off = d_rec_off.p;
    D.rec_combo = d_rec_combo.p;
    D.rec_pos = d_rec_pos.p;
    D.group = d_group.p;
    D.grp_base = d_grp_base.p;
    D.grp_total = d_grp_total.p;
    for (int i = 0; i < 3; ++i) { D.params.gap_open[i] = P.cp->gap_open[i]; D.params.gap_extend[i] = P.cp->gap_extend[i]; }
    D.params.scale = P.local_scale;
    D.sparse = P.sparse ? 1u : 0u;
    D.group_end = d_group_end.p;
    D.xch = d_xch.p;
    D.xred = d_xred.p;
    D.xdp = d_xdp.p;
    D.hacc = d_hacc.p;
    D.debug = path.use_walk2 && sw.walk2_debug ? 1u : 0u;
    D.status = d_status.p;
}

// ---- branch-and-bound far pass: record image, the two static orders per level, the sealing schedule -------------------
int ChainDev::far_setup(const ChainProblem& P, ChainPath& path) {
    if (!path.use_far) return CL_OK;
    const ChainSwitches& sw = P.sw;
    const uint32_t n_macro_all = (uint32_t)((P.M + kChainMacro - 1) / kChainMacro);
    uint32_t max_n = 0;
    int64_t smin = INT64_MAX, smax = INT64_MIN;
    uint32_t max_off = 0;
    {   // extremes of the shifts and offsets: one pass over every record (27 M at the root of ten sequences), combination by combination on the pool's threads
        std::vector<int64_t> lo(P.combos.size(), INT64_MAX), hi(P.combos.size(), INT64_MIN);
        std::vector<uint32_t> mo(P.combos.size(), 0);
        cl_parallel_for(P.combos.size(), [&](uint64_t b, uint64_t e) {
            for (uint64_t ci = b; ci < e; ++ci) {
                const Combo& c = P.combos[ci];
                int32_t l = INT32_MAX, h = INT32_MIN;
                uint32_t m = 0;
                const size_t n = c.rec_s.size();
                for (size_t r = 0; r < n; ++r) { const int32_t sg = c.sigma[r]; l = std::min(l, sg); h = std::max(h, sg); m = std::max(m, c.off[r]); }
                if (n) { lo[ci] = l; hi[ci] = h; mo[ci] = m; }
            }
        }, 1);
        for (size_t ci = 0; ci < P.combos.size(); ++ci) {
            max_n = std::max<uint32_t>(max_n, (uint32_t)P.combos[ci].rec_s.size());
            smin = std::min(smin, lo[ci]); smax = std::max(smax, hi[ci]); max_off = std::max(max_off, mo[ci]);
        }
    }
    uint32_t n_levels = 1;
    while (n_levels < (uint32_t)kFarMaxLevels && (64ull << (kFarFanShift * n_levels)) <= max_n) ++n_levels;
    const uint64_t n_top = 64ull << (kFarFanShift * (n_levels - 1));
    std::vector<uint32_t> base(P.combos.size());
    uint64_t r_pad = 0, max_padded = 0;
    for (size_t ci = 0; ci < P.combos.size(); ++ci) {
        base[ci] = (uint32_t)r_pad;
        const uint64_t padded = (P.combos[ci].rec_s.size() + n_top - 1) / n_top * n_top;
        max_padded = std::max(max_padded, padded);
        r_pad += padded;
    }
    // shift buckets: kFarBandShift wide unless bucket number and offset then do not fit the 32 bits of a
    // bucket key: bucket << off_bits | offset, off_bits enough for the largest offset + 1 (what a query's offset bound can be)
    uint32_t band_shift = (uint32_t)kFarBandShift;
    uint32_t off_bits = 1;
    while (off_bits < 31 && ((uint64_t)max_off + 1) >> off_bits) ++off_bits;
    // buckets are numbered from 1; bucket + 2 must stay below 2^(32 - off_bits) - 1 (the query's upper neighbour bucket, and the padding key above all)
    while (smin != INT64_MAX && band_shift < 30 && (((smax - smin) >> band_shift) + 4) >= (int64_t)((1ull << (32 - off_bits)) - 1)) ++band_shift;
    const int64_t bias = (1ll << band_shift) - smin;
    if (r_pad == 0 || r_pad >= (1ull << 31) || smin == INT64_MAX || smax + bias >= (1ll << 31) || bias >= (1ll << 31) || off_bits >= 28 ||
        (((smax - smin) >> band_shift) + 4) >= (int64_t)((1ull << (32 - off_bits)) - 1)) path.use_far = false;
    if (path.use_far) {
        const uint32_t R = (uint32_t)r_pad;
        F.n_levels = n_levels;
        F.r_pad = R;
        F.sig_bias = (int32_t)bias;
        F.band_shift = band_shift;
        F.off_bits = off_bits;
        double pw = 1e300, omax = 0, emax = 0;
        for (int k = 0; k < 3; ++k) {
            pw = std::min(pw, P.local_scale * (P.cp->gap_open[k] + P.cp->gap_extend[k] * (double)(1ull << band_shift)));
            omax = std::max(omax, P.cp->gap_open[k]);
            emax = std::max(emax, P.cp->gap_extend[k]);
        }
        F.band_pen = P.sparse ? 0.0 : pw;
        F.slack_t0 = P.local_scale * emax * (double)std::max<int64_t>(std::llabs(smin), std::llabs(smax)) + P.local_scale * omax;
        F.slack_e0 = P.local_scale * emax;
        // (the record image — 48 B per padded record — is allocated below, once the arena is known to fit 32-bit offsets: at the root of a 50-sequence MSA
        // it is 33 GB, and round 4 allocated it BEFORE finding out that the far pass could not be used there: the context held 105 GB for a DP of 71)
        CL_CHAIN_TRY(d_far_base.upload(ctx, base));
        D.far_base = d_far_base.p;
        // the arena: per level the two blocked orders (2 R words each) and their index arrays (R / 8, R / 64, ...)
        // Table entries are positions in blocks of 8 words (far_at, chain_far.hip): 2^35 words.  CL_CHAIN_FAR_ARENA_SKIP=<words> leaves that many words unused in
        // front (tests: positions beyond 2^32 words on a small DP; the pages are never touched)
        uint64_t words = sw.far_arena_skip;
        std::vector<uint32_t> tab((size_t)kFarMaxLevels * kFarTabWidth, 0xFFFFFFFFu);
        for (uint32_t l = 0; l < n_levels; ++l) {
            for (int side = 0; side < (P.sparse ? 1 : 2); ++side) {
                tab[l * kFarTabWidth + side] = (uint32_t)(words >> 3);
                words += 2ull * R;
                for (uint32_t j = 0; j <= l; ++j) {
                    tab[l * kFarTabWidth + 2 + side * kFarMaxLevels + j] = (uint32_t)(words >> 3);
                    words += ((uint64_t)R >> (3 * (j + 1))) + 8;
                    words = (words + 7) & ~7ull;    // 32-byte blocks stay aligned
                }
            }
        }
        if (words >= (1ull << 35) - 8) path.use_far = false;
        if (path.use_far && (uint64_t)R >= (1ull << 27)) {
            // a far pass this large (the root of a 50-sequence MSA: 690 M padded records, 185 B each with the sorts' scratch) is taken only if the device has
            // the room now — the DP is correct without it, an allocation that fails half-way would end the merge
            size_t free_b = 0, total_b = 0;
            const uint64_t need = (uint64_t)R * (48 + 7 * 4 + 8 * 2 + n_levels * (P.sparse ? 1 : 2) * 4) + words * 4;
            // ... and only if the context's last affine DP did not end up sweeping all pairs anyway: on 50 x 100 kbp (dense matches: a third of the leaves opened)
            // the DPs of the 156-combination merges choose the sweep, the 625-combination root then does too, and the sweep inside the far pass is 15 % slower than
            // without its structures (163 against 142 s); on 50 x 1 Mbp they choose branch-and-bound (1.3 % opened) and the root takes 36 instead of 196 s
            if (!P.sparse && ctx->far_last_choice == 2) {
                if (P.timing) fprintf(stderr, "[chain_dp_batch]   far pass not taken: the context's last affine DP chose the all-pairs sweep\n");
                path.use_far = false;
            } else
            if (hipMemGetInfo(&free_b, &total_b) != hipSuccess || need + need / 8 + (8ull << 30) > (uint64_t)free_b) {
                if (P.timing) fprintf(stderr, "[chain_dp_batch]   far pass not taken: it needs %.1f GB, the device has %.1f GB free\n", need * 1.125 / 1e9, free_b / 1e9);
                path.use_far = false;
            }
        }
        if (path.use_far) {
        CL_CHAIN_TRY(d_far_rec.alloc(ctx, (size_t)R * 12));
        D.far_rec = d_far_rec.p;
        CL_CHAIN_TRY(d_far_arena.alloc(ctx, words));
        CL_CHAIN_TRY(d_far_tab.upload(ctx, tab));
        F.arena = d_far_arena.p;
        F.tab_dev = d_far_tab.p;
        for (uint32_t l = 0; l < (uint32_t)kFarMaxLevels; ++l) for (int w = 0; w < kFarTabWidth; ++w) F.tab[l][w] = tab[l * kFarTabWidth + w];
        // scratch: 0 key_off, 1 idx, 2 order_off, 3 order_band, 4 node keys in, 5 node keys out / sorted-key sink, 6 key_band
        for (int i = 0; i < 7; ++i) CL_CHAIN_TRY(d_far_u32[i].alloc(ctx, R));
        const size_t temp_bytes = cl_chain_far_sort_temp_bytes(R);
        CL_CHAIN_TRY(d_far_temp.alloc(ctx, temp_bytes));
        hipError_t fe = cl_chain_far_init(D, d_far_base.p, (uint32_t)max_padded, R, F.sig_bias, F.band_shift, F.off_bits, d_far_u32[0].p, d_far_u32[6].p, d_far_u32[1].p, ctx->stream);
        if (fe == hipSuccess) fe = cl_chain_far_sort32(d_far_temp.p, temp_bytes, d_far_u32[0].p, d_far_u32[5].p, d_far_u32[1].p, d_far_u32[2].p, R, 32, ctx->stream);
        if (fe == hipSuccess && !P.sparse) fe = cl_chain_far_sort32(d_far_temp.p, temp_bytes, d_far_u32[6].p, d_far_u32[5].p, d_far_u32[1].p, d_far_u32[3].p, R, 32, ctx->stream);
        for (uint32_t l = 0; l < n_levels && fe == hipSuccess; ++l) {
            const uint32_t shift = kFarLeafShift + kFarFanShift * l;
            int bits = 1;
            while (((uint64_t)R >> shift) >> bits) ++bits;
            DevBuf<uint32_t>& perm_o = d_far_perm[2 * l];
            DevBuf<uint32_t>& perm_b = d_far_perm[2 * l + 1];
            CL_CHAIN_TRY(perm_o.alloc(ctx, R));
            fe = cl_chain_far_node_keys(d_far_u32[2].p, R, shift, d_far_u32[4].p, ctx->stream);
            if (fe == hipSuccess) fe = cl_chain_far_sort32(d_far_temp.p, temp_bytes, d_far_u32[4].p, d_far_u32[5].p, d_far_u32[2].p, perm_o.p, R, bits, ctx->stream);
            if (fe == hipSuccess) fe = cl_chain_far_layout(perm_o.p, d_far_u32[0].p, R, F.arena, F.tab[l][0], &F.tab[l][2], l + 1, ctx->stream);
            F.perm_o[l] = perm_o.p;
            if (!P.sparse) {
                CL_CHAIN_TRY(perm_b.alloc(ctx, R));
                if (fe == hipSuccess) fe = cl_chain_far_node_keys(d_far_u32[3].p, R, shift, d_far_u32[4].p, ctx->stream);
                if (fe == hipSuccess) fe = cl_chain_far_sort32(d_far_temp.p, temp_bytes, d_far_u32[4].p, d_far_u32[5].p, d_far_u32[3].p, perm_b.p, R, bits, ctx->stream);
                if (fe == hipSuccess) fe = cl_chain_far_layout(perm_b.p, d_far_u32[6].p, R, F.arena, F.tab[l][1], &F.tab[l][2 + kFarMaxLevels], l + 1, ctx->stream);
                F.perm_b[l] = perm_b.p;
            } else {   // sparse_chain_dp has no shifts: one order
                F.perm_b[l] = perm_o.p;
            }
        }
        if (fe != hipSuccess) { cl_set_error(ctx, "far pass setup failed: %s", hipGetErrorString(fe)); return CL_ERR_HIP; }
        // sealing schedule: a node is sealed right after the walk of the macro-block that finalises its last record
        std::vector<std::vector<uint32_t>> by_macro(n_macro_all);
        for (size_t ci = 0; ci < P.combos.size(); ++ci) {
            const Combo& c = P.combos[ci];
            const uint64_t nc = c.rec_s.size();
            for (uint32_t l = 0; l < n_levels; ++l) {
                const uint32_t shift = kFarLeafShift + kFarFanShift * l;
                const uint64_t nn = 1ull << shift;
                for (uint64_t a = 0; a < nc; a += nn) {
                    const uint64_t last = std::min(a + nn, nc) - 1;
                    by_macro[c.rec_s[last] / kChainMacro].push_back((l << 28) | (uint32_t)((base[ci] + a) >> shift));
                }
            }
        }
        std::vector<uint32_t> items;
        seal_off.assign(n_macro_all + 1, 0);
        seal_big.assign(n_macro_all, 0);
        for (uint32_t k = 0; k < n_macro_all; ++k) {
            // large nodes first: they get a workgroup each (far_seal_big_kernel), the others a wave each
            std::stable_sort(by_macro[k].begin(), by_macro[k].end(), [](uint32_t a, uint32_t b) { return (a >> 28) > (b >> 28); });
            if (!sw.seal_wave) for (uint32_t it : by_macro[k]) seal_big[k] += (it >> 28) >= 2 ? 1u : 0u;
            items.insert(items.end(), by_macro[k].begin(), by_macro[k].end());
            seal_off[k + 1] = (uint32_t)items.size();
        }
        CL_CHAIN_TRY(d_seal_items.upload(ctx, items));
        for (int i = 0; i < 7; ++i) d_far_u32[i].release();   // scratch
        }
    }
    return CL_OK;
}

int ChainDev::create_events(const ChainProblem& P) {
    if (hipEventCreate(&ev0) != hipSuccess || hipEventCreate(&ev1) != hipSuccess) { cl_set_error(ctx, "hipEventCreate failed"); return CL_ERR_HIP; }
    ev_intra.assign(P.n_blocks, nullptr);
    ev_far.assign(P.n_blocks, nullptr);
    return CL_OK;
}

hipError_t ChainDev::enqueue(const ChainProblem& P, ChainPath& path, UnitsHeld& units) {
    // compute units the walk launches of this DP occupy at a time (see WalkUnits)
    const uint32_t walk_units = !path.use_walk ? 0u : path.use_walk2 ? (uint32_t)(((P.combos.size() + 7) & ~(size_t)7) * (1 + path.walk2_help))
                                                           : (uint32_t)((P.combos.size() + std::max<uint32_t>(path.walk_fold, 1u) - 1) / std::max<uint32_t>(path.walk_fold, 1u));
    units.n = g_walk_exclusive && walk_units ? WalkUnits::kBudget : walk_units;
    if (walk_units && ctx->peers.n <= 1) { g_walk_units.take(ctx->device, units.n); units.held = true; }
    hipError_t he = hipEventRecord(ev0, ctx->stream);
    if (he == hipSuccess) he = hipEventRecord(ctx->ev_fork, ctx->stream);
    for (uint32_t f = 0; f < kChainFarStreams && he == hipSuccess; ++f) he = hipStreamWaitEvent(ctx->aux[f], ctx->ev_fork, 0);
    if (path.use_walk) he = enqueue_walk(P, path, he);
    else if (path.group_path) {
        for (size_t gi = 0; gi + 1 < group_first.size() && he == hipSuccess; ++gi)
            he = cl_chain_launch_group(D, group_first[gi], group_first[gi + 1], P.rec_off[group_first[gi + 1]] - P.rec_off[group_first[gi]], d_dp_enc.p, ctx->stream);
    } else he = enqueue_blocks(P, he);
    if (he == hipSuccess) he = hipEventRecord(ev1, ctx->stream);
    return he;
}

// macro-blocks of kChainMacro pairs: walk(k) on the context's stream is one launch of n_combos workgroups; the records of
// macro-block k - 1 reach k's queries by a brute-force "near" launch in front of it; everything older by a "far" launch on
// an auxiliary stream that may start as soon as walk(k - 2) is done
hipError_t ChainDev::enqueue_walk(const ChainProblem& P, ChainPath& path, hipError_t he) {
    const ChainSwitches& sw = P.sw;
    uint32_t max_n = 0;
    for (const Combo& c : P.combos) max_n = std::max<uint32_t>(max_n, (uint32_t)c.rec_s.size());
    if (he == hipSuccess) he = cl_chain_launch_own_rec(D, max_n, ctx->stream);
    const uint32_t n_macro = (uint32_t)((P.M + kChainMacro - 1) / kChainMacro), bpm = kChainMacro / kChainBlock;
    std::vector<hipEvent_t> ev_walk(n_macro, nullptr), ev_seal(n_macro, nullptr);
    std::vector<hipEvent_t> ring_far(n_macro, nullptr);   // (like ev_walk and ev_seal: the context's ring events, nothing to destroy)
    static_assert(kFarLag + 1 <= (uint32_t)kNumAuxStreams, "one auxiliary stream per far launch in flight plus the sealing stream");
    hipStream_t seal_stream = ctx->aux[path.far_lag];   // right behind the far streams: the context's own streams are few (cl_context_create)
    if (path.use_far) {
        if (he == hipSuccess) he = hipStreamWaitEvent(seal_stream, ctx->ev_fork, 0);
        for (uint32_t f = kChainFarStreams; f < path.far_lag && he == hipSuccess; ++f) he = hipStreamWaitEvent(ctx->aux[f], ctx->ev_fork, 0);
    }
    // Branch-and-bound or sweep?  The far kernels count the leaves they had to open against the leaves in range (status[2..5]).
    // At a few checkpoints the host waits for the launches so far and reads the counts: once they cover enough queries with a
    // long history, more than one leaf in sixteen opened means the sweep is the faster far pass for this input (repeats so
    // dense that every pair is near every other) and it takes over for the rest of the DP.  One decision per DP, taken between
    // launches: nothing is in flight when the mode changes.
    bool far_bb = path.use_far, far_decided = !path.use_far;
    if (path.use_far && sw.far_mode) { far_decided = true; far_bb = sw.far_mode[0] != 's'; }
    // A merge group (cl_peer_api.cpp) shares the far pass of this DP: every member takes the same decision from the same numbers — affine,
    // 2 .. kPeerMaxCombos combinations, at least 16 macro-blocks — and the choice of far pass is not left to counts that differ by member
    auto& peers = ctx->peers;
    const bool shared = path.use_far && far_bb && peers.n > 1 && !P.sparse && P.combos.size() >= 2 && P.combos.size() <= kPeerMaxCombos && n_macro >= 16 &&
                        !(sw.far_mode && sw.far_mode[0] == 's') && peers.epoch + 1 < (1u << 12);
    uint32_t share_epoch = 0;
    if (shared) {
        far_decided = true;
        share_epoch = ++peers.epoch;
        peers.epoch_mark = std::max(peers.epoch_mark, peers.epoch);
        ++peers.shared_dps;
        F.share_n = peers.n;
        F.share_i = peers.me;
        // The ring slots of an inbox are reused by the NEXT shared DP: a member that has gone on to it must not store into a slot another member has
        // not folded yet (round-4 advisor: slots k and k' collide whenever k - k' = 16 mod 32, whatever the epochs' parity).  Every member raises its
        // "done" word in the others' memory when its serial stream has passed the last block of a shared DP; the far streams — the only ones that
        // store into other inboxes — wait for the words of the previous shared DP before their first launch of this one
        for (uint32_t m = 0; m < peers.n && he == hipSuccess; ++m) {
            if (m == peers.me) continue;
            for (uint32_t f = 0; f < path.far_lag && he == hipSuccess; ++f)
                he = cl_peer_wait_word(ctx, ctx->aux[f], m, peers.flags + kPeerDoneAt + m, peers.last_shared_epoch);
        }
        peers.last_shared_epoch = share_epoch;
    }
    // the events that order the streams ride on the launches that they follow (hipExtLaunchKernel's stop event) instead of being runtime calls of
    // their own: 3 of ~12 calls per macro-block.  CL_CHAIN_EXT_EVENTS=0: hipEventRecord as in rounds 2-3 (A/B)
    // Round 5: far(k) goes out as soon as the seal it waits for has been enqueued — at the end of iteration k - lag - 1 instead of iteration k — so that the
    // serial stream can take far(k)'s event IN FRONT of near(k) (far(k) has had lag + 1 blocks to finish by then) instead of between near(k) and walk(k): there the
    // cross-stream hop sat between two dependent launches of the serial chain (kernel trace, round 4: gap 7.4 | near 22.8 | gap 14.9 | walk 55.2 us against ~7 us
    // for a plain launch-to-launch dependency).  CL_CHAIN_FAR_WAIT_LATE=1: as in round 4 (A/B).  Not inside a merge group (the peers' slots are per iteration)
    std::vector<uint8_t> far_issued(n_macro, 0);   // 1: far(k) is out, 2: ... and was sent early
    auto issue_far_bb = [&](uint32_t kk, bool early) -> hipError_t {
        const uint32_t first_k = kk * kChainMacro, count_k = (uint32_t)std::min<uint64_t>(kChainMacro, P.M - first_k), near_lo_k = (kk - path.far_lag) * bpm;
        hipStream_t far_stream = ctx->aux[kk % path.far_lag];
        // every node inside the records [0, prefix[near_lo]) was sealed by seal(kk - lag - 1) or earlier
        hipError_t e = hipStreamWaitEvent(far_stream, ev_seal[kk - path.far_lag - 1], 0);
        // CL_CHAIN_DEBUG_SKIP_FAR=1 (measurements only, WRONG RESULTS): the DP without its far launches = the serial walk / near chain alone,
        // i.e. what a merge would cost its leader if other devices took the far pass off it
        bool recorded = false;
        if (e == hipSuccess && !sw.skip_far) {
            // (the launch records ring_far[kk] itself: one runtime call less per macro-block)
            if (sw.ext_events) { e = cl_ring_event(ctx, 1, kk, &ring_far[kk]); recorded = e == hipSuccess; }
            if (e == hipSuccess) e = cl_chain_far_launch(D, F, first_k, count_k, near_lo_k, far_stream, recorded ? ring_far[kk] : nullptr);
        }
        if (!recorded) {
            if (e == hipSuccess) e = cl_ring_event(ctx, 1, kk, &ring_far[kk]);
            if (e == hipSuccess) e = hipEventRecord(ring_far[kk], far_stream);
        }
        far_issued[kk] = early ? 2 : 1;
        return e;
    };
    for (uint32_t k = 0; k < n_macro && he == hipSuccess; ++k) {
        if (far_decided && P.timing && path.use_far && k >= 256 && (k & (k - 1)) == 0) {   // (CL_CHAIN_TIMING: how the opened share moves after the decision)
            unsigned long long cnt[2] = {0, 0};
            if (hipStreamSynchronize(ctx->stream) == hipSuccess) {
                for (uint32_t f = 0; f < path.far_lag; ++f) (void)hipStreamSynchronize(ctx->aux[f]);
                if (cl_copy_sync(ctx, cnt, d_status.p + 2, sizeof(cnt), hipMemcpyDeviceToHost) == hipSuccess)
                    fprintf(stderr, "[chain_dp_batch]   far pass after %u macro-blocks: %llu of %llu leaves opened so far (%s)\n", k, cnt[0], cnt[1], far_bb ? "branch-and-bound" : "all-pairs sweep");
            }
        }
        if (!far_decided && k >= 96 && (k & (k - 1)) == 0) {   // k = 128, 256, 512, ...
            he = hipStreamSynchronize(ctx->stream);
            for (uint32_t f = 0; f < path.far_lag && he == hipSuccess; ++f) he = hipStreamSynchronize(ctx->aux[f]);
            unsigned long long cnt[2] = {0, 0};
            if (he == hipSuccess) he = cl_copy_sync(ctx, cnt, d_status.p + 2, sizeof(cnt), hipMemcpyDeviceToHost);
            if (he == hipSuccess && cnt[1] >= (1ull << 22)) {
                far_decided = true;
                far_bb = cnt[0] * 16 <= cnt[1];
                if (!P.sparse) ctx->far_last_choice = far_bb ? 1 : 2;
                if (P.timing) fprintf(stderr, "[chain_dp_batch]   far pass after %u macro-blocks: %llu of %llu leaves opened -> %s\n", k, cnt[0], cnt[1], far_bb ? "branch-and-bound" : "all-pairs sweep");
            }
        }
        const uint32_t first = k * kChainMacro, count = (uint32_t)std::min<uint64_t>(kChainMacro, P.M - first);
        const uint32_t lag = path.use_far ? path.far_lag : 1u;
        const uint32_t b0 = k * bpm, near_lo = k >= lag ? (k - lag) * bpm : 0;
        bool far_recorded = false;
        if (near_lo > 0) {
            hipStream_t far_stream = ctx->aux[k % (path.use_far ? path.far_lag : kChainFarStreams)];
            if (far_issued[k]) far_recorded = true;   // (sent at the end of iteration k - lag - 1)
            else if (path.use_far && far_bb && !shared) { he = issue_far_bb(k, false); far_recorded = true; }
            else if (path.use_far && far_bb) {
                // every node inside the records [0, prefix[near_lo]) was sealed by seal(k - lag - 1) or earlier
                he = hipStreamWaitEvent(far_stream, ev_seal[k - lag - 1], 0);
                {
                    // this member's combinations; what it finds goes into slot k of the others' inboxes, then its arrival word there
                    ClFarDevice Fk = F;
                    // (the slot depends on the epoch's parity too: a member that has gone on to the next shared DP while another still folds the
                    // last blocks of this one then writes the other half of the ring — 2 * lag + 2 <= 18 run-ahead inside a DP was the only bound before)
                    const uint32_t slot = (k + (kPeerRing / 2) * (share_epoch & 1u)) % kPeerRing, word = (share_epoch << 20) | (k + 1);
                    uint32_t o = 0;
                    for (uint32_t m = 0; m < peers.n; ++m) if (m != peers.me) Fk.peer_out[o++] = peers.peer_inbox[m] + (size_t)slot * kPeerSlotInts;
                    if (he == hipSuccess) he = cl_chain_far_launch(D, Fk, first, count, near_lo, far_stream, nullptr);
                    for (uint32_t m = 0; m < peers.n && he == hipSuccess; ++m)
                        if (m != peers.me) he = cl_peer_store_word_op(far_stream, peers.peer_flags[m] + (size_t)peers.me * kPeerRing + slot, word);
                    ++peers.shared_far_launches;
                }
            } else if (path.use_far) {
                // the all-pairs sweep has taken over (see the checkpoints below); same lag, so that sweeps run side by side
                he = hipStreamWaitEvent(far_stream, ev_walk[k - lag - 1], 0);
                if (he == hipSuccess) he = cl_chain_launch_inter(D, first, count, 0, near_lo, P.max_recs(0, near_lo), kChainFarTile, far_stream);
            } else {
                he = hipStreamWaitEvent(far_stream, ev_walk[k - 2], 0);
                const uint32_t recs = P.max_recs(0, near_lo);
                uint32_t tile = kChainFarTile;
                if (P.sparse) {
                    tile = kChainNearTile;
                    while (tile < kChainFarTile && (recs + tile - 1) / tile > kChainFullGrid) tile *= 2;
                }
                if (he == hipSuccess) he = cl_chain_launch_inter(D, first, count, 0, near_lo, recs, tile, far_stream);
            }
            if (!far_recorded) {
                if (he == hipSuccess) he = cl_ring_event(ctx, 1, k, &ring_far[k]);
                if (he == hipSuccess) he = hipEventRecord(ring_far[k], far_stream);
            }
        }
        hipEvent_t ev_near_a = nullptr;
        // the serial stream takes the event of a far(k) that went out early IN FRONT of the near launch (see issue_far_bb above)
        bool far_waited = false;
        if (he == hipSuccess && ring_far[k] && far_issued[k] == 2) { he = hipStreamWaitEvent(ctx->stream, ring_far[k], 0); far_waited = true; }
        if (he == hipSuccess && b0 > near_lo) {
            // the far pass stops at a leaf boundary: the near launch starts there.  Only the records of macro-block k - 1 need walk(k - 1): they
            // are swept on the serial stream; the older macro-blocks of the near range were final one walk earlier and are swept on a stream
            // of their own beside walk(k - 1) — with CL_CHAIN_NEAR_SPLIT=1 only: by default one launch on the serial stream, as in rounds 2-3
            const uint32_t b_split = sw.near_split && k >= 2 ? std::max(near_lo, (k - 1) * bpm) : near_lo;
            ClChainDevice Dn = D;
            if (path.use_far && near_lo > 0) Dn.lo_mask = 63u;
            if (b_split > near_lo) {
                hipStream_t near_stream = ctx->aux[(path.use_far ? path.far_lag : kChainFarStreams) + 1];
                he = hipStreamWaitEvent(near_stream, ev_walk[k - 2], 0);
                if (he == hipSuccess) he = cl_chain_launch_inter(Dn, first, count, near_lo, b_split, P.max_recs(near_lo, b_split) + Dn.lo_mask, kChainNearTile, near_stream);
                if (he == hipSuccess) he = cl_ring_event(ctx, 3, k, &ev_near_a);
                if (he == hipSuccess) he = hipEventRecord(ev_near_a, near_stream);
                Dn.lo_mask = 0;
            }
            if (he == hipSuccess) he = cl_chain_launch_inter(Dn, first, count, b_split, b0, P.max_recs(b_split, b0) + Dn.lo_mask, kChainNearTile, ctx->stream);
        }
        if (he == hipSuccess && ev_near_a) he = hipStreamWaitEvent(ctx->stream, ev_near_a, 0);
        if (he == hipSuccess && ring_far[k] && !far_waited) he = hipStreamWaitEvent(ctx->stream, ring_far[k], 0);
        if (shared && near_lo > 0) {
            // the other members' combinations of this macro-block: wait for their arrival words, fold their slot into the running maxima
            const uint32_t slot = (k + (kPeerRing / 2) * (share_epoch & 1u)) % kPeerRing, word = (share_epoch << 20) | (k + 1);
            for (uint32_t m = 0; m < peers.n && he == hipSuccess; ++m)
                if (m != peers.me) he = cl_peer_wait_word(ctx, ctx->stream, m, peers.flags + (size_t)m * kPeerRing + slot, word);
            if (he == hipSuccess) he = cl_chain_far_merge(D, peers.inbox + (size_t)slot * kPeerSlotInts, first, count, peers.n, peers.me, ctx->stream);
            ++peers.merged_blocks;
        }
        if (he == hipSuccess) he = cl_ring_event(ctx, 0, k, &ev_walk[k]);
        if (he == hipSuccess) he = path.use_walk2 ? cl_chain_launch_walk2(D, first, count, path.walk2_qpt, path.walk2_help, ctx->stream, sw.ext_events ? ev_walk[k] : nullptr)
                                             : path.walk_fold > 1 ? cl_chain_launch_walk_fold(D, path.walk_fold, first, count, ctx->stream, sw.ext_events ? ev_walk[k] : nullptr)
                                             : cl_chain_launch_walk(D, first, count, ctx->stream, sw.ext_events ? ev_walk[k] : nullptr);
        if (he == hipSuccess && !sw.ext_events) he = hipEventRecord(ev_walk[k], ctx->stream);
        if (path.use_far && far_bb && he == hipSuccess && k + path.far_lag + 1 < n_macro) {
            he = hipStreamWaitEvent(seal_stream, ev_walk[k], 0);
            if (he == hipSuccess) he = cl_ring_event(ctx, 2, k, &ev_seal[k]);
            if (he == hipSuccess) he = cl_chain_far_seal(D, F, d_seal_items.p, seal_off[k], seal_off[k + 1] - seal_off[k], seal_big[k], seal_stream, sw.ext_events ? ev_seal[k] : nullptr);
            if (he == hipSuccess && !sw.ext_events) he = hipEventRecord(ev_seal[k], seal_stream);
            if (he == hipSuccess && sw.far_early && !shared) he = issue_far_bb(k + path.far_lag + 1, true);
        }
    }
    if (shared) {   // this member has folded every slot of the DP (stream order: behind its last walk)
        for (uint32_t m = 0; m < peers.n && he == hipSuccess; ++m)
            if (m != peers.me) he = cl_peer_store_word_op(ctx->stream, peers.peer_flags[m] + kPeerDoneAt + peers.me, share_epoch);
    }
    if (path.use_far && he == hipSuccess) he = hipStreamSynchronize(seal_stream);
    if (path.use_far) path.far_ran = far_bb ? "bb" : "sweep";   // (the mode the DP ended in: the automatic choice may leave the branch-and-bound at a checkpoint)
    return he;
}

hipError_t ChainDev::enqueue_blocks(const ChainProblem& P, hipError_t he) {
    static_assert(kChainFarGroup == 1, "a far launch per block");
    for (uint32_t b = 0; b < P.n_blocks && he == hipSuccess; ++b) {
        const uint32_t first = b * kChainBlock, count = (uint32_t)std::min<uint64_t>(kChainBlock, P.M - first);
        const uint32_t near_lo = b > 1 ? b - 1 : 0;   // first block the far launch does not cover
        if (near_lo > 0) {
            // far predecessors: blocks [0, near_lo), final once walk(near_lo - 1) is done
            hipStream_t far_stream = ctx->aux[b % kChainFarStreams];
            he = hipStreamWaitEvent(far_stream, ev_intra[near_lo - 1], 0);
            // a launch ends with one atomic merge per query and workgroup: small tiles (low latency) only where that is
            // cheap — sparse mode has one maximum per query — and while the grid does not fill the chip
            const uint32_t recs = P.max_recs(0, near_lo);
            uint32_t tile = kChainFarTile;
            if (P.sparse) {
                tile = kChainNearTile;
                while (tile < kChainFarTile && (recs + tile - 1) / tile > kChainFullGrid) tile *= 2;
            }
            if (he == hipSuccess) he = cl_chain_launch_inter(D, first, count, 0, near_lo, recs, tile, far_stream);
            if (he == hipSuccess) he = hipEventCreateWithFlags(&ev_far[b], hipEventDisableTiming);
            if (he == hipSuccess) he = hipEventRecord(ev_far[b], far_stream);
        }
        // near predecessors: blocks [near_lo, b), on the sequential stream right after walk(b - 1)
        const bool fuse_near = P.combos.size() == 1;
        if (he == hipSuccess && b > near_lo && !fuse_near) he = cl_chain_launch_inter(D, first, count, near_lo, b, P.max_recs(near_lo, b), kChainNearTile, ctx->stream);
        if (he == hipSuccess && ev_far[b]) he = hipStreamWaitEvent(ctx->stream, ev_far[b], 0);
        if (he == hipSuccess) he = cl_chain_launch_intra(D, first, count, fuse_near ? b - near_lo : 0u, ctx->stream);
        if (he == hipSuccess) he = hipEventCreateWithFlags(&ev_intra[b], hipEventDisableTiming);
        if (he == hipSuccess) he = hipEventRecord(ev_intra[b], ctx->stream);
    }
    return he;
}

void ChainDev::print_path(const ChainProblem& P, const ChainPath& path) {
    std::lock_guard<std::mutex> lock(ctx->pool_mutex);
    fprintf(stderr, "[chain_dp_batch]   device memory held by the context: %.1f MB (%s queries, far pass %s: %u padded records in %u levels, %u + %u tags, walk %s)\n", ctx->dev_live_bytes / 1048576.0,
            P.factored ? "factored" : "dense", path.use_far ? "on" : "off", path.use_far ? F.r_pad : 0u, path.use_far ? F.n_levels : 0u, P.n_tag[0], P.n_tag[1],
            !path.use_walk ? "off" : path.use_walk2 ? "2" : path.walk_fold > 1 ? "fold" : "1");
    // which way the DP went where the number of combinations decides it (tests/test_gpu_combo_sweep.py reads this line)
    fprintf(stderr, "[chain_dp_batch]   path: %s, exchange %s, fold %u, helpers %u, numbering %s, arrays %s, far %s\n", path.use_walk ? "walk" : path.group_path ? "groups" : "per-block",
            !path.use_walk || P.combos.size() < 2 ? "none" : path.use_walk2 ? (path.walk_reduce ? "walk2+reduce" : "walk2") : path.walk_reduce ? "reduce" : "granules", path.use_walk ? std::max<uint32_t>(path.walk_fold, 1u) : 0u,
            path.use_walk2 ? path.walk2_help : 0u, P.par_numbering ? "parallel" : "serial", path.packed ? "packed" : "separate", path.far_ran);
}

int ChainDev::wait(const ChainProblem& P, const ChainPath& path, UnitsHeld& units, hipError_t he) {
    const ChainSwitches& sw = P.sw;
    if (he == hipSuccess && ctx->peers.n > 1) {
        // inside a merge group the serial stream waits for the other members' arrival words: a member that has failed would leave this
        // call waiting for ever, so the wait is a poll with a limit (CL_PEER_TIMEOUT_S, default 600 s); past it the context is unusable
        static const double limit_s = [] { const char* e = getenv("CL_PEER_TIMEOUT_S"); const double v = e ? atof(e) : 600.0; return v > 0 ? v : 600.0; }();
        const auto t_wait = std::chrono::steady_clock::now();
        while ((he = hipStreamQuery(ctx->stream)) == hipErrorNotReady) {
            if (std::chrono::duration<double>(std::chrono::steady_clock::now() - t_wait).count() > limit_s) {
                (void)hipGetLastError();
                ctx->poisoned = true;
                cl_set_error(ctx, "chaining DP: the other members of the merge group did not deliver within %.0f s (a member failed?); this context cannot be used any more", limit_s);
                return CL_ERR_HIP;   // (device buffers of this DP are left to the stuck stream: releasing them would wait for it)
            }
            usleep(50);
        }
        if (he == hipErrorNotReady) he = hipSuccess;
        (void)hipGetLastError();
    }
    if (he == hipSuccess) he = hipStreamSynchronize(ctx->stream);
    for (uint32_t f = 0; f < std::max<uint32_t>(kChainFarStreams, path.far_lag) && he == hipSuccess; ++f) he = hipStreamSynchronize(ctx->aux[f]);
    if (units.held) { g_walk_units.give(ctx->device, units.n); units.held = false; }   // (the device is done with this DP's launches)
    if (he != hipSuccess) return chain_hip_fail(ctx, he, "chaining DP kernels");
    if (path.use_walk) {
        uint32_t status = 0;
        he = cl_copy_sync(ctx, &status, d_status.p, sizeof(status), hipMemcpyDeviceToHost);
        if (he != hipSuccess) return chain_hip_fail(ctx, he, "chaining DP status");
        if (D.debug) {
            uint32_t dbg[32] = {};
            (void)cl_copy_sync(ctx, dbg, d_status.p, sizeof(dbg), hipMemcpyDeviceToHost);
            const double steps = std::max(1u, dbg[8]);
            fprintf(stderr, "[chain_dp_batch]   walk2: %u steps of combination 0, %u queries finalised, %u polled at their finalisation, %u evaluated out of LDS (no helper result); "
                            "wave 0 per step (100 MHz ticks): before the barrier %.1f, in the barrier %.1f, behind it %.1f; helper batches %u, records %u, polls without news %u; wave 0 finalised in %u steps: %.1f ticks before the barrier there, %.1f behind the barrier before; per launch: %.1f ticks in front of the loop, %.1f in it; not asked %u, no granule of the block %u; shader clock %.0f MHz (s_memtime against the 100 MHz s_memrealtime)\n",
                    dbg[8], dbg[9], dbg[10], dbg[11], dbg[12] / steps, dbg[13] / steps, dbg[14] / steps, dbg[16], dbg[17], dbg[18], dbg[19], dbg[20] / (double)std::max(1u, dbg[19]), dbg[21] / (double)std::max(1u, dbg[19]), dbg[22] / (double)std::max(1u, dbg[24]), dbg[23] / (double)std::max(1u, dbg[24]), dbg[25], dbg[26], 100.0 * dbg[27] / (double)std::max(1u, dbg[28]));
        }
        if (sw.debug_stall && !(g_walk_exclusive && !strcmp(sw.debug_stall, "first"))) status = 1;
        if (status != 0) {
            cl_set_error(ctx, "chaining DP: a workgroup of the walk kernel gave up waiting for its siblings (%zu combinations not all resident?)", P.combos.size());
            return kWalkStalled;
        }
    }
    {
        float dev_ms = 0;
        (void)hipEventElapsedTime(&dev_ms, ev0, ev1);
        P.tm.device_ms += dev_ms;
    }
    return CL_OK;
}

int ChainDev::download(const ChainProblem& P, const ChainPath& path) {
    hipError_t he = hipSuccess;
    dp_sorted.resize(P.M);
    acc.assign(P.combos.size(), nullptr);
    if (d_pack.p) {
        // a small DP: its DP values and query results lie together at the end of the block
        pack_host.resize(pack_down_bytes);
        he = cl_copy_sync(ctx, pack_host.data(), d_pack.p + pack_dp_off, pack_down_bytes, hipMemcpyDeviceToHost);
        if (he == hipSuccess) {
            memcpy(dp_sorted.data(), pack_host.data(), P.M * sizeof(float));
            const size_t first_acc = (size_t)((char*)cd[0].d_acc.p - d_pack.p) - pack_dp_off;
            for (size_t ci = 0; ci < P.combos.size(); ++ci) acc[ci] = reinterpret_cast<const int*>(pack_host.data() + first_acc + ci * pack_acc_stride);
        }
    } else
    he = cl_copy_sync(ctx, dp_sorted.data(), d_dp.p, P.M * sizeof(float), hipMemcpyDeviceToHost);
    if (P.timing) fprintf(stderr, "[chain_dp_batch]   traceback rows %s\n", path.lazy_acc ? "on demand" : "downloaded");
    if (he == hipSuccess && path.lazy_acc) {
        CL_CHAIN_TRY(d_row.alloc(ctx, P.combos.size() * 7));
        row_pin = (int*)cl_pinned(ctx, P.combos.size() * 7 * sizeof(int));
        if (!row_pin) { row_host.resize(P.combos.size() * 7); row_pin = row_host.data(); }
    }
    if (he == hipSuccess && !d_pack.p && !path.lazy_acc) {
        const size_t per = (size_t)P.M * 7;
        int* pin = (int*)cl_pinned(ctx, P.combos.size() * per * sizeof(int));
        if (pin) {
            for (size_t ci = 0; ci < P.combos.size() && he == hipSuccess; ++ci) {
                acc[ci] = pin + ci * per;
                he = hipMemcpyAsync(pin + ci * per, cd[ci].d_acc.p, per * sizeof(int), hipMemcpyDeviceToHost, ctx->stream);
            }
            if (he == hipSuccess) he = hipStreamSynchronize(ctx->stream);
        } else {
            acc_own.resize(P.combos.size());
            for (size_t ci = 0; ci < P.combos.size() && he == hipSuccess; ++ci) {
                acc_own[ci].resize(per);
                acc[ci] = acc_own[ci].data();
                he = cl_copy_sync(ctx, acc_own[ci].data(), cd[ci].d_acc.p, per * sizeof(int), hipMemcpyDeviceToHost);
            }
        }
    }
    if (he != hipSuccess) { cl_set_error(ctx, "download failed: %s", hipGetErrorString(he)); return CL_ERR_HIP; }
    return CL_OK;
}

const int* ChainDev::acc_row(const ChainProblem& P, uint32_t s) {
    if (row_s == s) return row_pin;
    hipError_t e = cl_chain_acc_row(D, s, d_row.p, ctx->stream);
    if (e == hipSuccess) e = cl_copy_sync(ctx, row_pin, d_row.p, P.combos.size() * 7 * sizeof(int), hipMemcpyDeviceToHost);
    if (e != hipSuccess) { cl_set_error(ctx, "traceback: fetching the query results of pair %u failed: %s", s, hipGetErrorString(e)); return nullptr; }
    row_s = s;
    return row_pin;
}

// chain_dp_batch: K independent chaining instances in ONE device pass.
//
// sparse == false: sparse_affine_chain_dp (anchorer.hpp:1812-2471); sparse == true: sparse_chain_dp (:1511-1750), which is the
// same sweep with ONE tree per (chain of e1, chain of e2), no shift condition and no gap cost: on the device it is the
// affine machinery with every shift set to 0, so that only the "same diagonal" maximum is ever fed.
//
// Batching (the fill-in re-anchoring of anchorer.hpp:619-699 runs one small DP per gap of the chain, thousands per merge):
// the device only ever COMPARES the path coordinates (index of the end node / predecessor index of the start node), the
// arithmetic uses the shifts, which are stored separately.  Instance k therefore gets its graph-1 coordinates shifted UP by
// the total size of the instances before it and its graph-2 coordinates shifted up by the total size of the instances AFTER
// it: a record of another instance then fails one of the two range conditions (index1 <= query1, index2 < query2), and
// the whole batch is one all-pairs sweep over the concatenated match pairs.
static int chain_dp_batch_impl(cl_context* ctx, const std::vector<ChainSub>& subs, const cl_chain_params* cp, double local_scale,
                               bool sparse, std::vector<ChainSubResult>& results, ChainTimings& tm, std::vector<float>* dp_out, bool allow_walk);

// The walk kernel's workgroups (one per chain combination) wait for one another and must all be resident at once.  That holds whenever the
// device is not packed with OTHER contexts' workgroups; if a bounded wait ever expires, nothing has been decided yet (the status word is
// read before any result is used) and the DP is simply run again on the per-block kernels, which need no co-residency.
int chain_dp_batch(cl_context* ctx, const std::vector<ChainSub>& subs, const cl_chain_params* cp, double local_scale,
                          bool sparse, std::vector<ChainSubResult>& results, ChainTimings& tm, std::vector<float>* dp_out) {
    const ChainTimings before = tm;
    ++cl_fallbacks.chain_dps;
    int rc = chain_dp_batch_impl(ctx, subs, cp, local_scale, sparse, results, tm, dp_out, true);
    if (rc != kWalkStalled) return rc;
    ++cl_fallbacks.walk_stalls;
    if (ctx->peers.n > 1) return CL_ERR_HIP;   // (inside a merge group the other members have gone on with this member's share: no second attempt)
    // round 6: ONE more attempt on the walk kernels with the device's whole walk budget booked for this DP (no other DP of the process in flight beside it) before the
    // per-block kernels, which take minutes where the walk takes seconds (a 156-combination DP of 1.19 M pairs: 184 s against 11 s)
    const char* debug_stall = chain_switches().debug_stall;   // (test hook: "first" = only the shared attempt "stalls"; any other value = every walk does: straight to the per-block kernels)
    if (!debug_stall || !strcmp(debug_stall, "first")) {
        if (getenv("CL_CHAIN_TIMING")) fprintf(stderr, "[chain_dp_batch]   walk kernel stalled: repeating the DP alone on the device\n");
        tm = before;
        g_walk_exclusive = true;
        rc = chain_dp_batch_impl(ctx, subs, cp, local_scale, sparse, results, tm, dp_out, true);
        g_walk_exclusive = false;
        if (rc != kWalkStalled) return rc;
        ++cl_fallbacks.walk_stalls;
    }
    if (getenv("CL_CHAIN_TIMING")) fprintf(stderr, "[chain_dp_batch]   walk kernel stalled: repeating the DP on the per-block kernels\n");
    tm = before;
    rc = chain_dp_batch_impl(ctx, subs, cp, local_scale, sparse, results, tm, dp_out, false);
    return rc == kWalkStalled ? CL_ERR_HIP : rc;
}

// the device phases and the traceback of one attempt: `dev` owns every buffer and event and lets go of them when this returns, whichever way
static int chain_dp_device(ChainProblem& P, std::vector<ChainSubResult>& results, std::vector<float>* dp_out, bool allow_walk) {
    cl_context* ctx = P.ctx;
    PackLayout pack;
    ChainPath path = choose_path(P, allow_walk, pack);
    UnitsHeld units{ctx->device, 0, false};
    ChainDev dev(ctx);
    ChainTrace trace;   // (behind dev: its thread is joined before dev's buffers go)
    dev.cd.resize(P.combos.size());
    CL_CHAIN_TRY(path.packed ? dev.upload_packed(P, path, pack) : P.factored ? dev.upload_factored(P, path) : dev.upload_separate(P, path));
    CL_CHAIN_TRY(dev.upload_groups(P, path));
    dev.fill_device(P, path);
    CL_CHAIN_TRY(dev.far_setup(P, path));
    P.lap("far pass setup");
    P.tm.prep_ms += ms_since(P.T0);
    P.lap("upload");
    CL_CHAIN_TRY(dev.create_events(P));
    trace.start_prebuild(P);
    const hipError_t he = dev.enqueue(P, path, units);
    P.lap("enqueue (host)");
    if (P.timing) dev.print_path(P, path);
    CL_CHAIN_TRY(dev.wait(P, path, units, he));
    P.lap("sync");
    CL_CHAIN_TRY(dev.download(P, path));
    if (trace.ortho_prebuild.joinable()) trace.ortho_prebuild.join();
    P.lap("download");
    CL_CHAIN_TRY(trace.run(P, path, dev, results, dp_out));
    return CL_OK;
}

static int chain_dp_batch_impl(cl_context* ctx, const std::vector<ChainSub>& subs, const cl_chain_params* cp, double local_scale,
                               bool sparse, std::vector<ChainSubResult>& results, ChainTimings& tm, std::vector<float>* dp_out, bool allow_walk) {
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    { const int jrc = cl_stitch_join(ctx); if (jrc) return jrc; }   // (a stitch pass of this context may still be out on the auxiliary streams this DP is about to use)
    results.assign(subs.size(), ChainSubResult());
    ChainProblem P(ctx, subs, cp, local_scale, sparse, tm);
    CL_CHAIN_TRY(P.collect_pairs());
    if (P.M == 0) return CL_OK;
    P.lap("pairs");
    CL_CHAIN_TRY(P.build_tables());
    P.lap("tables");
    P.sort_by_depth();
    P.lap("sort by depth");
    P.weights();
    P.lap("weights");
    P.anchoring_terms();
    P.lap("anchoring terms");
    P.records();
    P.lap("records");
    P.count_work();
    P.queries();
    P.lap("queries");
    CL_CHAIN_TRY(chain_dp_device(P, results, dp_out, allow_walk));
    P.lap("release");
    return CL_OK;
}

}  // namespace clchain
