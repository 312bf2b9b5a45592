// cl_api.cpp — host side of the C ABI declared in include/centrolign_amd.h: the context, errors, the big-block allocator, the host thread pool
// and the small entry points round a stitch (result buffers, batch extraction, cl_stitch / cl_internal_stitch over cl_stitch_batch_align).
// A stitch plan is made in cl_stitch_plan_api.cpp and run in cl_stitch_exec_api.cpp.
// There is no CPU implementation of the DP in this library: without a gfx950 device the entry points
// return CL_ERR_NO_DEVICE.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <new>
#include <string>
#include <unordered_map>
#include <atomic>
#include <condition_variable>
#include <deque>
#include <memory>
#include <thread>
#include <chrono>
#include <vector>

#include "cl_internal.hpp"
#include "popoa_device.h"
#include "stitch_host.hpp"

namespace {

thread_local std::string g_error;

}  // namespace

ClFallbackCounters cl_fallbacks;
std::atomic<size_t> cl_pinned_total{0};

// ClRawVec's storage (cl_internal.hpp): blocks of a megabyte and more come from, and go back to, a per-thread cache (at most kBigCacheCap bytes
// per thread, best fit within 2x); a 64-byte header in front of every block says how large it is
namespace {
constexpr size_t kBigMin = 1u << 20, kBigCacheCap = 6ull << 30;
struct BigHeader { size_t capacity; void* map; size_t map_bytes; };   // map: the block's own mapping (null: malloc'ed)
static_assert(sizeof(BigHeader) <= 64, "header");
void big_release(void* h) noexcept {
    BigHeader* hd = static_cast<BigHeader*>(h);
    if (hd->map) (void)munmap(hd->map, hd->map_bytes); else free(h);
}
// (over all threads of the process the caches keep at most kBigCacheProcessCap: MSA workers and pool threads each have one, and a thread that has
// cached its share after one large merge may never need it again)
constexpr size_t kBigCacheProcessCap = 24ull << 30;
std::atomic<size_t> g_big_cached{0};
struct BigCache {
    std::multimap<size_t, void*> free_blocks;   // capacity -> header
    size_t bytes = 0;
    ~BigCache() { for (auto& b : free_blocks) { g_big_cached -= b.first; big_release(b.second); } }
};
thread_local BigCache t_big_cache;
}
static void* big_alloc_raw(size_t bytes);
// CL_BIG_POISON=1 (tests): every block is handed out filled with 0xA5 — code that relied on fresh mappings being zero shows at once instead of
// after a block has been used before
void* cl_big_alloc(size_t bytes) {
    static const bool poison = getenv("CL_BIG_POISON") != nullptr;
    void* p = big_alloc_raw(bytes);
    if (poison && bytes) memset(p, 0xA5, bytes);
    return p;
}
static void* big_alloc_raw(size_t bytes) {
    if (bytes >= kBigMin) {
        auto it = t_big_cache.free_blocks.lower_bound(bytes);
        if (it != t_big_cache.free_blocks.end() && it->first <= 2 * bytes) {
            void* h = it->second;
            t_big_cache.bytes -= it->first;
            g_big_cached -= it->first;
            t_big_cache.free_blocks.erase(it);
            return static_cast<char*>(h) + 64;
        }
    }
    if (bytes >= kBigMin) {
        // a mapping of its own, advised to use huge pages: first touch then costs a fault per 2 MB instead of per 4 KB (34 ms instead of
        // 120 ms per 900 MB on the MI355X host, scripts/dev/pin_bench.cpp) — and faults take the address-space lock the other workers need
        constexpr size_t kHuge = 2u << 20;
        const size_t len = ((bytes + 64 + kHuge - 1) & ~(kHuge - 1)) + kHuge;
        void* map = mmap(nullptr, len, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS, -1, 0);
        if (map == MAP_FAILED) throw std::bad_alloc();
        char* h = reinterpret_cast<char*>((reinterpret_cast<uintptr_t>(map) + kHuge - 1) & ~(uintptr_t)(kHuge - 1));
        (void)madvise(h, len - kHuge, MADV_HUGEPAGE);
        BigHeader* hd = reinterpret_cast<BigHeader*>(h);
        hd->capacity = bytes; hd->map = map; hd->map_bytes = len;
        return h + 64;
    }
    void* h = malloc(bytes + 64);
    if (!h) throw std::bad_alloc();
    BigHeader* hd = static_cast<BigHeader*>(h);
    hd->capacity = bytes; hd->map = nullptr; hd->map_bytes = 0;
    return static_cast<char*>(h) + 64;
}
void cl_big_free(void* p) noexcept {
    if (!p) return;
    void* h = static_cast<char*>(p) - 64;
    const size_t cap = static_cast<BigHeader*>(h)->capacity;
    if (cap >= kBigMin && t_big_cache.bytes + cap <= kBigCacheCap && g_big_cached.load(std::memory_order_relaxed) + cap <= kBigCacheProcessCap) {
        try { t_big_cache.free_blocks.emplace(cap, h); t_big_cache.bytes += cap; g_big_cached += cap; return; } catch (...) {}
    }
    big_release(h);
}

// A context keeps up to seven streams busy (the chaining DP: walk, two far launches, the sealing stream, copies) and an MSA runs several worker
// contexts; they share the process's hardware queues (GPU_MAX_HW_QUEUES, HIP's default 4).  The library leaves that setting to the host
// application; nothing here depends on a stream having a queue of its own.

void cl_set_error(cl_context* ctx, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_error = buf;
    if (ctx) {   // worker threads of cl_msa report into the caller's context: one writer at a time
        static std::mutex error_mutex;
        std::lock_guard<std::mutex> lock(error_mutex);
        ctx->error = buf;
    }
}
#define set_error cl_set_error

// ---- the process's host thread pool (cl_parallel_for, cl_internal.hpp) ---------------------------------------------------------------
namespace {
struct HostPool {
    struct Batch {
        const std::function<void(unsigned)>* task;
        unsigned n_tasks;
        std::atomic<unsigned> next{1};       // task 0 belongs to the caller
        std::atomic<unsigned> done{0};
        std::mutex m;
        std::condition_variable cv;
    };
    std::mutex m;
    std::condition_variable cv;
    std::deque<std::shared_ptr<Batch>> open;   // batches that still have unclaimed tasks
    std::vector<std::thread> threads;
    unsigned width = 1;
    bool stop = false;
    static thread_local bool is_worker;

    HostPool() {
        const char* e = getenv("CL_HOST_THREADS");
        const int v = e ? atoi(e) : 0;
        const unsigned hw = std::thread::hardware_concurrency();
        width = v > 0 ? (unsigned)v : std::min(hw ? hw : 1u, 32u);
        // more threads than one loop uses: several contexts (MSA workers) run loops at the same time
        const unsigned n_threads = width <= 1 ? 0 : std::min(hw ? hw : 1u, 4 * width) - 1;
        for (unsigned i = 0; i < n_threads; ++i) threads.emplace_back([this] { work(); });
    }
    ~HostPool() {
        { std::lock_guard<std::mutex> lock(m); stop = true; }
        cv.notify_all();
        for (auto& t : threads) t.join();
    }
    static void run_one(Batch& b, unsigned t) {
        (*b.task)(t);
        if (b.done.fetch_add(1) + 1 == b.n_tasks) { std::lock_guard<std::mutex> lock(b.m); b.cv.notify_all(); }
    }
    void work() {
        is_worker = true;
        while (true) {
            std::shared_ptr<Batch> b;
            unsigned t = 0;
            {
                std::unique_lock<std::mutex> lock(m);
                cv.wait(lock, [&] { return stop || !open.empty(); });
                if (stop) return;
                b = open.front();
                t = b->next.fetch_add(1);
                if (t + 1 >= b->n_tasks) open.pop_front();   // this was the last unclaimed task
                if (t >= b->n_tasks) continue;
            }
            run_one(*b, t);
        }
    }
    void run(unsigned n_tasks, const std::function<void(unsigned)>& task) {
        if (n_tasks <= 1 || threads.empty() || is_worker) {   // (a loop inside a pool task runs in place)
            for (unsigned t = 0; t < n_tasks; ++t) task(t);
            return;
        }
        auto b = std::make_shared<Batch>();
        b->task = &task;
        b->n_tasks = n_tasks;
        { std::lock_guard<std::mutex> lock(m); open.push_back(b); }
        cv.notify_all();
        run_one(*b, 0);
        // help with this batch's remaining tasks instead of sleeping, then wait for the ones other threads took
        while (true) {
            unsigned t;
            {
                std::lock_guard<std::mutex> lock(m);
                t = b->next.load();
                if (t >= b->n_tasks) break;
                t = b->next.fetch_add(1);
                if (t + 1 >= b->n_tasks) { auto it = std::find(open.begin(), open.end(), b); if (it != open.end()) open.erase(it); }
                if (t >= b->n_tasks) break;
            }
            run_one(*b, t);
        }
        std::unique_lock<std::mutex> lock(b->m);
        b->cv.wait(lock, [&] { return b->done.load() == b->n_tasks; });
    }
};
thread_local bool HostPool::is_worker = false;
HostPool& host_pool() { static HostPool pool; return pool; }
}  // namespace
void cl_pool_run(unsigned n_tasks, const std::function<void(unsigned)>& task) { host_pool().run(n_tasks, task); }
unsigned cl_pool_width() { return host_pool().width; }

namespace {
std::mutex g_live_mutex;
std::vector<const cl_context*> g_live_contexts;
}
bool cl_context_live(const cl_context* ctx) {
    std::lock_guard<std::mutex> lock(g_live_mutex);
    return std::find(g_live_contexts.begin(), g_live_contexts.end(), ctx) != g_live_contexts.end();
}

extern "C" {

int cl_abi_version(void) { return CL_ABI_VERSION; }

void cl_fallback_counters(cl_fallback_stats* out, int reset) {
    if (out) {
        out->strip_fallbacks = cl_fallbacks.strip_fallbacks.load();
        out->walk_stalls = cl_fallbacks.walk_stalls.load();
        out->chain_dps = cl_fallbacks.chain_dps.load();
        out->stitch_plans = cl_fallbacks.stitch_plans.load();
        out->strip_pairs = cl_fallbacks.strip_pairs.load();
        out->bond_trims_past_the_end = cl_fallbacks.bond_trims_past_the_end.load();
    }
    if (reset) { cl_fallbacks.strip_fallbacks = 0; cl_fallbacks.walk_stalls = 0; cl_fallbacks.chain_dps = 0; cl_fallbacks.stitch_plans = 0; cl_fallbacks.strip_pairs = 0; cl_fallbacks.bond_trims_past_the_end = 0; }
}

void cl_stitch_params_default(cl_stitch_params* p) {
    // src/parameters.cpp:74-85 (the CLI's values; Stitcher's class defaults differ)
    p->alignment_params.match = 20;
    p->alignment_params.mismatch = 80;
    const uint32_t go[3] = {60, 800, 2500}, ge[3] = {30, 5, 1};
    for (int i = 0; i < 3; ++i) { p->alignment_params.gap_open[i] = go[i]; p->alignment_params.gap_extend[i] = ge[i]; }
    p->max_trivial_size = 30000;
    p->min_wfa_size = 40000000;
    p->max_wfa_size = 75000000;
    p->max_wfa_ratio = 1.05;
    p->wfa_pruning_dist = 25;
    p->deletion_alignment_ratio = 8;
    p->deletion_alignment_short_max_size = 1500;
    p->deletion_alignment_long_min_size = 2000;
}

int cl_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

const char* cl_last_error(const cl_context* ctx) { return ctx ? ctx->error.c_str() : g_error.c_str(); }

const char* cl_device_name(const cl_context* ctx) { return ctx ? ctx->name.c_str() : ""; }

cl_context* cl_context_create(int device_ordinal) {
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0) {
        set_error(nullptr, "no HIP device available (%s)", e == hipSuccess ? "device count is 0" : hipGetErrorString(e));
        return nullptr;
    }
    if (device_ordinal < 0 || device_ordinal >= n) {
        set_error(nullptr, "device ordinal %d out of range (0..%d)", device_ordinal, n - 1);
        return nullptr;
    }
    cl_context* ctx = new (std::nothrow) cl_context();
    if (!ctx) return nullptr;
    ctx->device = device_ordinal;
    int callers_device = -1;   // the caller's current device is put back: creating worker contexts on a list of devices must not move the calling thread
    (void)hipGetDevice(&callers_device);
    hipDeviceProp_t prop;
    bool ok = hipSetDevice(device_ordinal) == hipSuccess && hipGetDeviceProperties(&prop, device_ordinal) == hipSuccess &&
              hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking) == hipSuccess &&
              hipEventCreateWithFlags(&ctx->ev_fork, hipEventDisableTiming) == hipSuccess;
    // streams of their own: CL_CTX_STREAMS (default 6: what one chaining DP keeps busy — four far launches in flight, the sealing stream and
    // a spare).  Every stream takes a share of the process's hardware queues (GPU_MAX_HW_QUEUES); streams that share a queue run their
    // launches one after the other, whichever context they belong to, so contexts that work side by side should not hold idle streams
    // (read at every creation: a caller that wants a context with more streams for one purpose — bench.py's resident stitch plan: eight — sets the variable round that call)
    const int n_own = [] { const char* e = getenv("CL_CTX_STREAMS"); int v = e ? atoi(e) : 0; return v >= 1 && v <= kNumAuxStreams ? v : 6; }();
    ctx->n_aux = n_own;
    for (int i = 0; ok && i < kNumAuxStreams; ++i) {
        if (i < n_own) ok = hipStreamCreateWithFlags(&ctx->aux[i], hipStreamNonBlocking) == hipSuccess;
        else ctx->aux[i] = ctx->aux[i % n_own];
        ok = ok && hipEventCreateWithFlags(&ctx->ev_join[i], hipEventDisableTiming) == hipSuccess;
    }
    if (!ok) {
        set_error(nullptr, "HIP context setup failed on device %d: %s", device_ordinal, hipGetErrorString(hipGetLastError()));
        cl_context_destroy(ctx);
        return nullptr;
    }
    ctx->name = std::string(prop.name) + " (" + prop.gcnArchName + ")";
    if (callers_device >= 0 && callers_device != device_ordinal) (void)hipSetDevice(callers_device);
    {
        std::lock_guard<std::mutex> lock(g_live_mutex);
        g_live_contexts.push_back(ctx);
    }
    return ctx;
}

void cl_context_destroy(cl_context* ctx) {
    if (!ctx) return;
    {
        std::lock_guard<std::mutex> lock(g_live_mutex);
        g_live_contexts.erase(std::remove(g_live_contexts.begin(), g_live_contexts.end(), ctx), g_live_contexts.end());
    }
    (void)hipSetDevice(ctx->device);
    for (int i = 0; i < kNumAuxStreams; ++i) {
        if (ctx->aux[i] && i < ctx->n_aux) (void)hipStreamDestroy(ctx->aux[i]);
        if (ctx->ev_join[i]) (void)hipEventDestroy(ctx->ev_join[i]);
    }
    if (ctx->ev_fork) (void)hipEventDestroy(ctx->ev_fork);
    if (ctx->stream) (void)hipStreamDestroy(ctx->stream);
    cl_pinned_release(ctx);
    cl_peers_release(ctx);
    for (auto& ring : ctx->ev_ring) for (hipEvent_t e : ring) if (e) (void)hipEventDestroy(e);
    {
        std::lock_guard<std::mutex> lock(ctx->pool_mutex);
        cl_pool_trim(ctx);
    }
    delete ctx;
}

void cl_stitch_result_free(cl_stitch_result* r) {
    if (!r) return;
    free(r->aln_off); free(r->pairs); free(r->score); free(r->route); free(r->num_pw);
    memset(r, 0, sizeof(*r));
}

int cl_stitch_result_alloc(cl_stitch_result* out, uint64_t n_problems, uint64_t n_pairs) {
    if (!out) return CL_ERR_INVALID_ARGUMENT;
    memset(out, 0, sizeof(*out));
    out->n_problems = n_problems;
    out->aln_off = (uint64_t*)calloc(n_problems + 1, sizeof(uint64_t));
    out->pairs = (uint64_t*)malloc((n_pairs ? n_pairs : 1) * 2 * sizeof(uint64_t));
    out->score = (int64_t*)calloc(n_problems ? n_problems : 1, sizeof(int64_t));
    out->route = (uint8_t*)calloc(n_problems ? n_problems : 1, 1);
    out->num_pw = (uint8_t*)calloc(n_problems ? n_problems : 1, 1);
    if (!out->aln_off || !out->pairs || !out->score || !out->route || !out->num_pw) { cl_stitch_result_free(out); return CL_ERR_OUT_OF_MEMORY; }
    return CL_OK;
}

int cl_context_set_stitch_hook(cl_context* ctx, cl_stitch_hook_fn fn, void* user, uint64_t min_cells) {
    if (!ctx) return CL_ERR_INVALID_ARGUMENT;
    ctx->stitch_hook = fn;
    ctx->stitch_hook_user = fn ? user : nullptr;
    ctx->stitch_hook_min_cells = min_cells;
    return CL_OK;
}



struct cl_owned_batch {
    clhost::OwnedBatch b;
};

int cl_extract_stitch_batch(const cl_base_graph* g1, const cl_base_graph* g2, const cl_anchor_segments* sg, cl_owned_batch** out) {
    if (!g1 || !g2 || !sg || !out) { set_error(nullptr, "null argument"); return CL_ERR_INVALID_ARGUMENT; }
    *out = nullptr;
    for (const cl_base_graph* g : {g1, g2})
        if (g->n_nodes >= (1ull << 32) || g->src_id >= g->n_nodes || g->snk_id >= g->n_nodes) { set_error(nullptr, "bad graph"); return CL_ERR_INVALID_ARGUMENT; }
    cl_owned_batch* ob = new (std::nothrow) cl_owned_batch();
    if (!ob) return CL_ERR_OUT_OF_MEMORY;
    int rc = clhost::extract_stitch_batch(*g1, *g2, *sg, ob->b, cl_shared_table(g1), cl_shared_table(g2));
    if (rc) { set_error(nullptr, rc == CL_ERR_CYCLIC_GRAPH ? "merge graph is not acyclic" : "empty anchor segment"); delete ob; return rc; }
    *out = ob;
    return CL_OK;
}

const cl_stitch_batch* cl_owned_batch_view(cl_owned_batch* b) { return b ? b->b.view() : nullptr; }
void cl_owned_batch_free(cl_owned_batch* b) { delete b; }

void cl_alignment_free(cl_alignment* a) {
    if (!a) return;
    free(a->pairs);
    a->pairs = nullptr;
    a->n_pairs = 0;
}

int cl_stitch(cl_context* ctx, const cl_base_graph* g1, const cl_base_graph* g2, const cl_anchor_segments* sg,
              const cl_stitch_params* params, cl_alignment* out) {
    cl_bind_device(ctx);
    if (!ctx || !g1 || !g2 || !sg || !params || !out) { set_error(ctx, "null argument"); return CL_ERR_INVALID_ARGUMENT; }
    out->n_pairs = 0;
    out->pairs = nullptr;
    static const bool timing = getenv("CL_STITCH_TIMING") != nullptr;
    auto t = std::chrono::steady_clock::now();
    auto lap = [&](const char* what) {
        if (timing) fprintf(stderr, "[cl_stitch] %-24s %8.2f ms\n", what, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t).count());
        t = std::chrono::steady_clock::now();
    };
    cl_owned_batch* ob = nullptr;
    int rc = cl_extract_stitch_batch(g1, g2, sg, &ob);
    if (rc) { if (ctx) ctx->error = g_error; return rc; }
    lap("extraction");
    cl_stitch_result res;
    const cl_stitch_batch* bv = cl_owned_batch_view(ob);
    bool hooked = false;
    if (ctx->stitch_hook) {   // several devices take the merge's subproblems (cl_context_set_stitch_hook)
        uint64_t cells = 0;
        for (uint64_t q = 0; q < bv->n_problems; ++q) {
            const uint64_t a = bv->side[0].node_off[q + 1] - bv->side[0].node_off[q], b = bv->side[1].node_off[q + 1] - bv->side[1].node_off[q];
            if (a && b) cells += (a + 1) * (b + 1);
        }
        hooked = cells >= ctx->stitch_hook_min_cells;
    }
    if (hooked) {
        memset(&res, 0, sizeof(res));
        rc = ctx->stitch_hook(ctx->stitch_hook_user, ctx, bv, params, &res);
        ++ctx->stitch_hook_calls;
        if (!rc && res.n_problems != bv->n_problems) { cl_stitch_result_free(&res); set_error(ctx, "the stitch hook returned %llu results for %llu subproblems", (unsigned long long)res.n_problems, (unsigned long long)bv->n_problems); rc = CL_ERR_INVALID_ARGUMENT; }
        else if (rc) set_error(ctx, "the stitch hook failed (%d)", rc);
    } else rc = cl_stitch_batch_align(ctx, bv, params, &res);
    lap("batch align");
    cl_owned_batch_free(ob);
    if (rc) return rc;
    // stitcher.hpp:157-203: P0 A0 P1 A1 ... every subproblem but the first is preceded by one copied anchor
    uint64_t n_anchor_pairs = sg->n_segments ? sg->walk_off[sg->seg_off[sg->n_segments]] - sg->walk_off[sg->seg_off[0]] : 0;
    uint64_t total = res.aln_off[res.n_problems] + n_anchor_pairs;
    out->pairs = (uint64_t*)malloc((total ? total : 1) * 2 * sizeof(uint64_t));
    if (!out->pairs) { cl_stitch_result_free(&res); return CL_ERR_OUT_OF_MEMORY; }
    uint64_t cur = 0, k = 0;
    auto copy_problem = [&](uint64_t p) {
        uint64_t n = res.aln_off[p + 1] - res.aln_off[p];
        memcpy(out->pairs + 2 * cur, res.pairs + 2 * res.aln_off[p], n * 2 * sizeof(uint64_t));
        cur += n;
    };
    copy_problem(k++);
    for (uint64_t s = 0; s < sg->n_segments; ++s)
        for (uint64_t a = sg->seg_off[s]; a < sg->seg_off[s + 1]; ++a) {
            if (a != sg->seg_off[s]) copy_problem(k++);
            for (uint64_t w = sg->walk_off[a]; w < sg->walk_off[a + 1]; ++w) {
                out->pairs[2 * cur] = sg->walk1[w];
                out->pairs[2 * cur + 1] = sg->walk2[w];
                ++cur;
            }
            if (a + 1 == sg->seg_off[s + 1]) copy_problem(k++);
        }
    out->n_pairs = cur;
    cl_stitch_result_free(&res);
    lap("interleave anchors");
    return CL_OK;
}

// Stitcher::internal_stitch (stitcher.hpp:209-234): a chain of anchors between two places of ONE graph (a tandem duplication found by the
// cyclisation rounds, src/core.cpp:268-269).  The gaps between consecutive anchors are extracted from the graph against itself and aligned
// like any other gap (subalign with only_deletion_alns = false); the output order is the reference's: anchor 0, then for every later anchor
// its own pairs FOLLOWED by the alignment of the gap in front of it (:216-231).
int cl_internal_stitch(cl_context* ctx, const cl_base_graph* g, uint64_t n_anchors, const uint64_t* walk_off, const uint32_t* walk1,
                       const uint32_t* walk2, const cl_stitch_params* params, cl_alignment* out) {
    cl_bind_device(ctx);
    if (!ctx || !g || !params || !out || (n_anchors && (!walk_off || !walk1 || !walk2))) { set_error(ctx, "null argument"); return CL_ERR_INVALID_ARGUMENT; }
    out->n_pairs = 0;
    out->pairs = nullptr;
    if (g->n_nodes >= (1ull << 32) || g->src_id >= g->n_nodes || g->snk_id >= g->n_nodes) { set_error(ctx, "bad graph"); return CL_ERR_INVALID_ARGUMENT; }
    cl_stitch_result res;
    memset(&res, 0, sizeof(res));
    if (n_anchors > 1) {
        clhost::PathMergeTable own;
        const clhost::PathMergeTable* pm = cl_shared_table(g);
        if (!pm) { if (!own.build(*g)) { set_error(ctx, "graph is not acyclic"); return CL_ERR_CYCLIC_GRAPH; } pm = &own; }
        const uint64_t seg_off[2] = {0, n_anchors};
        const cl_anchor_segments sg{1, seg_off, walk_off, walk1, walk2};
        for (uint64_t a = 0; a < n_anchors; ++a) if (walk_off[a + 1] <= walk_off[a]) { set_error(ctx, "empty anchor"); return CL_ERR_INVALID_ARGUMENT; }
        cl_owned_batch ob;
        int rc = clhost::extract_stitch_batch(*g, *g, sg, ob.b, pm, pm, false);
        if (rc) { set_error(ctx, "extraction failed"); return rc; }
        if ((rc = cl_stitch_batch_align(ctx, ob.b.view(), params, &res))) return rc;
        if (res.n_problems != n_anchors - 1) { cl_stitch_result_free(&res); set_error(ctx, "internal_stitch: gap count"); return CL_ERR_INVALID_ARGUMENT; }
    }
    const uint64_t total = (n_anchors ? walk_off[n_anchors] - walk_off[0] : 0) + (res.aln_off ? res.aln_off[res.n_problems] : 0);
    out->pairs = (uint64_t*)malloc((total ? total : 1) * 2 * sizeof(uint64_t));
    if (!out->pairs) { cl_stitch_result_free(&res); return CL_ERR_OUT_OF_MEMORY; }
    uint64_t cur = 0;
    for (uint64_t a = 0; a < n_anchors; ++a) {
        for (uint64_t w = walk_off[a]; w < walk_off[a + 1]; ++w) { out->pairs[2 * cur] = walk1[w]; out->pairs[2 * cur + 1] = walk2[w]; ++cur; }
        if (a) {
            const uint64_t n = res.aln_off[a] - res.aln_off[a - 1];
            memcpy(out->pairs + 2 * cur, res.pairs + 2 * res.aln_off[a - 1], n * 2 * sizeof(uint64_t));
            cur += n;
        }
    }
    out->n_pairs = cur;
    cl_stitch_result_free(&res);
    return CL_OK;
}

}  // extern "C"