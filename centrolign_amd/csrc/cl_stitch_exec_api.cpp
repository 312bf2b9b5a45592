// cl_stitch_exec_api.cpp — a stitch plan's execution: its launches over the context's streams (launch_group, profile_groups, enqueue_groups, cl_stitch_join), the passes
// (cl_stitch_plan_execute / _execute_profiled / _execute_evented / _sync), what a plan reports (_stats, _launch_info), the results (_collect), its release, and the
// one-shot entry points that make, run and collect a plan per chunk of a batch (run_whole / run_chunk: cl_po_poa_batch, cl_stitch_batch_align).
// The plan itself is made in cl_stitch_plan_api.cpp; stitch_plan.hpp is what the two share.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "cl_internal.hpp"
#include "popoa_device.h"
#include "stitch_plan.hpp"

#define set_error cl_set_error

namespace {

int64_t pure_deletion_score(size_t path_len, int npw, const cl_align_params& p) {
    if (path_len == 0) return 0;
    // alignment.hpp:1202-1205 evaluates -open - extend in uint32_t before widening; reproduced literally
    int64_t s = std::numeric_limits<int64_t>::max();
    for (int k = 0; k < npw; ++k) s = std::min<int64_t>(s, (int64_t)(uint32_t)(0u - p.gap_open[k] - p.gap_extend[k]));
    return s;
}

// ---- cl_stitch_plan_collect's helpers ----
// what the launches left per PO-POA problem, on the host
struct PlanOutputs {
    std::vector<uint32_t> len, status;
    std::vector<int32_t> score;
    std::vector<uint2> pairs;
};
int download_outputs(cl_context* ctx, const cl_stitch_plan* pl, PlanOutputs& o) {
    const size_t npo = pl->desc.size();
    o.len.resize(npo); o.status.resize(npo); o.score.resize(npo); o.pairs.resize(pl->d_out_pairs.n);
    if (!npo) return CL_OK;
    HIP_TRY(ctx, cl_copy_sync(ctx, o.len.data(), pl->d_out_len.p, npo * 4, hipMemcpyDeviceToHost));
    HIP_TRY(ctx, cl_copy_sync(ctx, o.status.data(), pl->d_out_status.p, npo * 4, hipMemcpyDeviceToHost));
    HIP_TRY(ctx, cl_copy_sync(ctx, o.score.data(), pl->d_out_score.p, npo * 4, hipMemcpyDeviceToHost));
    if (!o.pairs.empty()) HIP_TRY(ctx, cl_copy_sync(ctx, o.pairs.data(), pl->d_out_pairs.p, o.pairs.size() * sizeof(uint2), hipMemcpyDeviceToHost));
    return CL_OK;
}

// Pairs that gave up waiting (status 9) run again on a kernel that waits for nobody — same planes, same output slots: the list is uploaded, launch(dev, list, count)
// enqueued on the context's stream and waited for, the pairs counted as fallbacks.  `what`: the pairs and the kernel, for the error text
template <class Launch>
int rerun_pairs(cl_context* ctx, cl_stitch_plan* pl, const std::vector<uint32_t>& again, const char* what, Launch launch) {
    DevBuf<uint32_t> d_again;
    int rc = d_again.upload(ctx, again);
    if (rc) return rc;
    ClDeviceBatch dev = pl->dev;
    dev.ticks = nullptr;
    hipError_t e = launch(dev, d_again.p, (uint32_t)again.size());
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    d_again.release();
    if (e != hipSuccess) { set_error(ctx, "re-running %zu %s failed: %s", again.size(), what, hipGetErrorString(e)); return CL_ERR_HIP; }
    pl->stats.n_strip_fallbacks += again.size();
    cl_fallbacks.strip_fallbacks += again.size();
    return CL_OK;
}

}  // namespace

void cl_stitch_plan_free(cl_stitch_plan* pl) {
    if (!pl) return;
    // (one wait for the owning context's streams, then the sixteen blocks go back to its pool: cl_internal.hpp, cl_ctx_quiesce)
    cl_context* owner = pl->d_desc.owner;
    const bool q = owner && cl_context_live(owner);
    if (q) cl_ctx_quiesce(owner);
    pl->d_desc.release(q);
    for (int s = 0; s < 2; ++s) {
        pl->d_lab[s].release(q); pl->d_poff[s].release(q); pl->d_pidx[s].release(q); pl->d_snk[s].release(q);
    }
    pl->d_planes.release(q); pl->d_out_pairs.release(q); pl->d_out_len.release(q); pl->d_out_status.release(q);
    pl->d_plist.release(q); pl->d_out_score.release(q); pl->d_aux.release(q);
    pl->d_strips.release(q); pl->d_strip_recs.release(q); pl->d_strip_list.release(q); pl->d_progress.release(q); pl->d_handoff.release(q);
    pl->d_ticks.release(q); pl->d_lane_sync.release(q); pl->d_ptasks.release(q); pl->d_phead.release(q); pl->d_sparams.release(q);
    for (auto& g : pl->groups) {
        if (g.ev0) (void)hipEventDestroy(g.ev0);
        if (g.ev1) (void)hipEventDestroy(g.ev1);
    }
    if (pl->ev_start) (void)hipEventDestroy(pl->ev_start);
    if (pl->ev_stop) (void)hipEventDestroy(pl->ev_stop);
    delete pl;
}

extern "C" {

// a launch group -> its launcher call: the one place that knows which launcher, with which arguments, a variant is
static hipError_t launch_group(const LaunchGroup& g, cl_stitch_plan* pl, const ClDeviceBatch& dev, hipStream_t stream) {
    const uint32_t* list = pl->d_plist.p + g.first;
    switch (g.variant) {
    case LaunchVariant::Chain: return cl_launch_popoa_linear(g.waves, g.count, dev, list, pl->sparams, stream);
    case LaunchVariant::Quads: return cl_launch_popoa_linear(0, g.count, dev, list, pl->sparams, stream);    // (cl_launch_popoa_linear's W: 0 = four pairs per wave,
    case LaunchVariant::Duos: return cl_launch_popoa_linear(-2, g.count, dev, list, pl->sparams, stream);    //  -2 = two)
    case LaunchVariant::ChainSpan: {   // the pairs' progress / done words start every pass at zero
        hipError_t e = hipMemsetAsync(pl->d_lane_sync.p + g.prog_first, 0, (size_t)g.prog_count * sizeof(uint32_t), stream);
        if (e != hipSuccess) return e;
        return cl_launch_popoa_linear_span(g.count, dev, list, pl->sparams, pl->d_lane_sync.p, stream);
    }
    case LaunchVariant::ChainPersistent:
        return cl_launch_popoa_chain_persistent(g.grid, g.prog_count, dev, pl->d_plist.p, pl->d_ptasks.p, pl->d_phead.p, pl->sparams, stream);
    case LaunchVariant::Lane: return cl_launch_popoa_lane(g.waves, g.count, g.ring_bytes, dev, list, pl->sparams, nullptr, stream);
    case LaunchVariant::LaneWide: {
        hipError_t e = hipMemsetAsync(pl->d_lane_sync.p + g.prog_first, 0, (size_t)g.prog_count * sizeof(uint32_t), stream);
        if (e != hipSuccess) return e;
        return cl_launch_popoa_lane(g.waves, g.count, g.ring_bytes, dev, list, pl->sparams, pl->d_lane_sync.p, stream);
    }
    case LaunchVariant::Sys: return cl_launch_popoa_sys(g.npw, g.block, g.count, g.ring_bytes, dev, list, pl->sparams, stream);
    case LaunchVariant::Strip: {
        // the strips' progress words start every pass at zero (the strips of a launch poll one another's)
        hipError_t e = hipMemsetAsync(pl->d_progress.p + g.prog_first, 0, (size_t)g.prog_count * sizeof(uint32_t), stream);
        if (e != hipSuccess) return e;
        return cl_launch_popoa_strip(g.npw, (uint32_t)g.block, g.count, g.ring_bytes, dev, pl->sdev, pl->d_strip_list.p + g.first, pl->sparams, stream);
    }
    case LaunchVariant::General: return cl_launch_popoa_general(g.npw, g.block, g.count, g.ring_bytes, dev, list, pl->sparams, stream);
    case LaunchVariant::Narrow: return cl_launch_popoa_narrow(g.block, g.count, g.ring_bytes, pl->narrow, dev, pl->d_plist.p, pl->d_sparams.p, stream);
    case LaunchVariant::None: break;
    }
    return hipErrorInvalidValue;
}

// a launch's two tick words (popoa_device.h: pass << 48 | 48 bits of ~start, of end; 100 MHz) -> its duration in microseconds, 0 if the words are not of one pass
static double tick_span_us(unsigned long long w0, unsigned long long w1) {
    constexpr unsigned long long mask = 0xFFFFFFFFFFFFull;
    if (!w0 || !w1 || (w0 >> 48) != (w1 >> 48)) return 0.0;
    const unsigned long long start = ~w0 & mask, end = w1 & mask;
    return end > start ? (double)(end - start) * 1e-2 : 0.0;
}

// The context's stream waits for the stitch launches that were handed to the auxiliary streams.  A pass of a plan does NOT do this by itself any more (second half of
// round 5): the launches of a resident plan's next pass follow this pass's launches in STREAM order (a launch group goes to the same stream in every pass and reads
// and writes nothing but its own subproblems), so passes that are enqueued back to back overlap — a stream starts pass i + 1 when ITS launches of pass i are done —
// instead of leaving every stream idle until the slowest one and two event hops are through (0.25-0.5 ms of 2.3 per step of 10 x 1 Mbp: scripts/dev/step_timeline.py).
// Whatever needs a pass to be complete joins first: cl_stitch_plan_sync / _collect / _execute_profiled / _destroy, a re-dealing of the launches, the chaining DP.
extern "C++" int cl_stitch_join(cl_context* ctx) {   // (C++ linkage: declared in cl_internal.hpp for the chaining DP, not part of the C ABI)
    for (int si = 0; si < kNumAuxStreams && ctx->stitch_join_pending; ++si)
        if (ctx->stitch_join_pending & (1u << si)) {
            HIP_TRY(ctx, hipStreamWaitEvent(ctx->stream, ctx->ev_join[si], 0));
            ctx->stitch_join_pending &= ~(1u << si);
        }
    return CL_OK;
}
static int plan_mark_stop(cl_context* ctx, cl_stitch_plan* pl) {
    int rc = cl_stitch_join(ctx);
    if (rc) return rc;
    if (pl->stop_pending) { HIP_TRY(ctx, hipEventRecord(pl->ev_stop, ctx->stream)); pl->stop_pending = false; }
    return CL_OK;
}

// The profiled pass: every launch ALONE on the context's stream, the device idle before and after, timed by the HOST's clock round
// launch + wait and by the kernel's own.  HIP event pairs read about twice the kernel's duration in the rocprofv3 kernel trace here (round 4: 2.87 ms by events,
// 1.43 ms in the trace for the dominant launch, also with nothing else on the device); the host's clock round launch + wait reads the
// kernel plus ~20 us of launch and wake-up latency, i.e. agrees with the trace within a few per cent for the launches that matter
// (a launch that finds the device idle runs at about half speed — the dominant launch 2.9 ms against 1.45 ms behind another launch, with the
// shader clock already at its top in both cases: whatever ramps, ramps within the first launch — so the duration reported is that of a launch
// behind another one, which is what a launch inside a step is, and what the rocprofv3 kernel trace of a step shows)
static int profile_groups(cl_context* ctx, cl_stitch_plan* pl) {
    { int rc = plan_mark_stop(ctx, pl); if (rc) return rc; }
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    const size_t ng = pl->groups.size();
    if (!pl->d_ticks.p) { int rc = pl->d_ticks.alloc(ctx, 2 * ng); if (rc) return rc; }
    for (size_t gi = 0; gi < ng; ++gi) {
        LaunchGroup& g = pl->groups[gi];
        // the kernel's own clock: first workgroup's start, last workgroup's end (s_memrealtime, 100 MHz) — what the rocprofv3 kernel trace shows;
        // beside it the host's clock round launch + wait
        ClDeviceBatch dev = pl->dev;
        dev.ticks = pl->d_ticks.p + 2 * gi;
        dev.tick_pass = 0xFFFFu;
        HIP_TRY(ctx, launch_group(g, pl, dev, ctx->stream));   // (first run: whatever ramps with the device idle, ramps here)
        HIP_TRY(ctx, hipMemsetAsync(dev.ticks, 0, 2 * sizeof(unsigned long long), ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        const auto t0 = std::chrono::steady_clock::now();
        HIP_TRY(ctx, launch_group(g, pl, dev, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        g.host_idle_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
        unsigned long long got[2] = {0, 0};
        HIP_TRY(ctx, cl_copy_sync(ctx, got, dev.ticks, sizeof(got), hipMemcpyDeviceToHost));
        const double us = tick_span_us(got[0], got[1]);
        g.host_ms = us > 0 ? (float)(us * 1e-3) : g.host_idle_ms;
    }
    return CL_OK;
}

// The concurrent pass: every launch group of the plan enqueued as a fork/join over the context's auxiliary streams.
static int enqueue_groups(cl_context* ctx, cl_stitch_plan* pl) {
    // every launch also leaves its own clock's start / end (two atomics per workgroup): cl_stitch_plan_launch_info reports the durations of the LAST pass,
    // i.e. of launches that overlap with one another as they do in production
    // (the words are not zeroed between passes: a pass's number in their top bits makes its clocks win over every earlier pass's; zeroed when the number wraps and
    // after the profiled pass, whose launches carry the highest number)
    const bool fresh = !pl->d_ticks.p;
    if (fresh && !pl->groups.empty()) { int rc = pl->d_ticks.alloc(ctx, 2 * pl->groups.size()); if (rc) return rc; }
    if (pl->d_ticks.p && (fresh || pl->tick_pass == 0 || pl->tick_pass >= 0xFFFEu)) {
        int rc = plan_mark_stop(ctx, pl);
        if (rc) return rc;
        HIP_TRY(ctx, hipMemsetAsync(pl->d_ticks.p, 0, 2 * pl->groups.size() * sizeof(unsigned long long), ctx->stream));
        pl->tick_pass = 0;
    }
    ++pl->tick_pass;
    // CL_STITCH_DEBUG_CLEAR=1 (tests): every pass first zeroes the plan's per-subproblem outputs, so that a pass whose launches skipped work shows up in what
    // cl_stitch_plan_collect returns instead of leaving the previous pass's values in place
    static const bool debug_clear = [] { const char* e = getenv("CL_STITCH_DEBUG_CLEAR"); return e && e[0] == '1'; }();
    if (debug_clear) {
        { int rc = cl_stitch_join(ctx); if (rc) return rc; }   // (the previous pass may still be writing them on the auxiliary streams)
        HIP_TRY(ctx, hipMemsetAsync(pl->d_out_len.p, 0, pl->desc.size() * sizeof(uint32_t), ctx->stream));
        HIP_TRY(ctx, hipMemsetAsync(pl->d_out_status.p, 0, pl->desc.size() * sizeof(uint32_t), ctx->stream));
        HIP_TRY(ctx, hipMemsetAsync(pl->d_out_score.p, 0, pl->desc.size() * sizeof(int32_t), ctx->stream));
    }
    HIP_TRY(ctx, hipEventRecord(ctx->ev_fork, ctx->stream));
    bool used[kNumAuxStreams] = {};
    // the groups come longest first (cl_stitch_plan_create: estimated duration = longest sweep x the kernel's time per step); each goes to the
    // stream with the least work so far (longest-processing-time rule), so that the one or two long sweeps of a batch start at once on streams
    // of their own and the short launches queue up beside, not behind, them.
    const int n_streams = ctx->n_aux;
    uint64_t load[kNumAuxStreams] = {};
    std::vector<int> stream_of(pl->groups.size());
    for (size_t gi = 0; gi < pl->groups.size(); ++gi) {
        int si = 0;
        for (int t = 1; t < n_streams; ++t) if (load[t] < load[si]) si = t;
        load[si] += std::max<uint64_t>(1, pl->groups[gi].est_cost);
        stream_of[gi] = si;
    }
    static const bool sched_log = getenv("CL_STITCH_SCHED_LOG") != nullptr;   // the deal, once per change of the groups' order: stream, estimated duration, workgroups, kind
    if (sched_log && pl->tick_pass <= 1) {
        fprintf(stderr, "[stitch plan] launches over %d streams (calibrated %d, re-dealings left %d):", n_streams, (int)pl->calibrated, pl->redeals_left);
        for (int t = 0; t < n_streams; ++t) {
            fprintf(stderr, "  s%d %llu us [", t, (unsigned long long)load[t]);
            for (size_t gi = 0; gi < pl->groups.size(); ++gi)
                if (stream_of[gi] == t) fprintf(stderr, " %s/w%d/b%d x%u:%llu", cl_launch_variant_name(pl->groups[gi].variant), pl->groups[gi].waves, pl->groups[gi].grid ? (int)pl->groups[gi].grid : pl->groups[gi].block, pl->groups[gi].count, (unsigned long long)pl->groups[gi].est_cost);
            fprintf(stderr, " ]");
        }
        fprintf(stderr, "\n");
    }
    // In which order the launches are ISSUED: the device starts about four launches at a time (a hardware queue that is handing out a launch's workgroups is busy until
    // the last of them has a compute unit — for the 34 716 workgroups of the short chain pairs that is the launch's whole duration), and in the step of 10 x 1 Mbp the
    // launch that ends the step — 66 long near-chain pairs, 1.27 ms — was started 0.43 ms after the first one (scripts/dev/step_timeline.py).  Launches of few workgroups
    // (at most two per compute unit: resident at once, their queue is free again at once) therefore go first, the wide ones after them; each on the stream the
    // longest-processing-time rule gave it.
    for (int pass = 0; pass < 2; ++pass)
        for (size_t gi = 0; gi < pl->groups.size(); ++gi) {
            const LaunchGroup& g = pl->groups[gi];
            const bool light = g.count <= 512;
            if (light != (pass == 0)) continue;
            const int si = stream_of[gi];
            if (!used[si]) { HIP_TRY(ctx, hipStreamWaitEvent(ctx->aux[si], ctx->ev_fork, 0)); used[si] = true; }
            ClDeviceBatch dev = pl->dev;
            dev.ticks = pl->d_ticks.p ? pl->d_ticks.p + 2 * gi : nullptr;
            dev.tick_pass = pl->tick_pass;
            if (pl->event_pass) {
                LaunchGroup& ge = pl->groups[gi];
                if (!ge.ev0) { HIP_TRY(ctx, hipEventCreate(&ge.ev0)); HIP_TRY(ctx, hipEventCreate(&ge.ev1)); }
                HIP_TRY(ctx, hipEventRecord(ge.ev0, ctx->aux[si]));
            }
            HIP_TRY(ctx, launch_group(g, pl, dev, ctx->aux[si]));
            if (pl->event_pass) { HIP_TRY(ctx, hipEventRecord(pl->groups[gi].ev1, ctx->aux[si])); pl->groups[gi].evented = true; }
        }
    const bool eager_join = [] { const char* e = getenv("CL_STITCH_JOIN"); return e && e[0] == 'e'; }();   // CL_STITCH_JOIN=eager: every pass joins (up to the first half of round 5); read per pass: bench.py times both
    for (int si = 0; si < kNumAuxStreams; ++si)
        if (used[si]) {
            HIP_TRY(ctx, hipEventRecord(ctx->ev_join[si], ctx->aux[si]));
            ctx->stitch_join_pending |= 1u << si;
        }
    pl->stop_pending = true;
    return eager_join ? plan_mark_stop(ctx, pl) : CL_OK;   // (otherwise the end of the pass is marked when somebody joins: plan_mark_stop)
}

// The launches longest first again, by the est_cost a re-deal has just given them.  The tick words belong to the launches in their OLD order: the next pass starts them afresh.
static void sort_groups_by_cost(cl_stitch_plan* pl) {
    std::stable_sort(pl->groups.begin(), pl->groups.end(), [](const LaunchGroup& x, const LaunchGroup& y) { return x.est_cost > y.est_cost; });
    pl->tick_pass = 0;
}

// First re-deal, by the durations measured ALONE: a plan that is executed again (resident inputs, replayed passes) measures its launches ONCE — each alone on the
// device, the host's clock round launch + wait — and deals them over the streams by those durations from then on: a launch lasts as long as its longest sweep at a
// rate that depends on the subproblems' branching (0.25 .. 2.7 us per step), which the estimate of cl_stitch_plan_create cannot know.
// Measured on the 10 x 1 Mbp batches as one plan: 3.03 ms per step with the estimate (the stream that got 1.40 + 0.70 + 0.79 ms sets the
// pace), the sum of the sixteen launches is 12.8 ms over six streams.
static int redeal_by_solo_durations(cl_context* ctx, cl_stitch_plan* pl) {
    int rc = profile_groups(ctx, pl);
    if (rc) return rc;
    for (LaunchGroup& g : pl->groups) g.est_cost = (uint64_t)(g.host_ms * 1000.f) + 1;
    sort_groups_by_cost(pl);
    return CL_OK;
}

// Second re-deal, by the launches' OWN clocks inside the previous pass: a launch alone and the same launch among fifteen others are different things — in the timed
// step of 10 x 1 Mbp the chain kernel's launch of 221 long pairs takes 0.4 ms alone and 1.7 ms in the step (its sixteen waves per workgroup wait for SIMDs they share),
// so the first re-deal put a 0.28 ms launch behind it on its stream, and that stream ended the step 0.2 ms after every other one (scripts/dev/step_timeline.py).  So
// the pass after the first concurrent one deals the launches out again by the durations their own clocks showed (first workgroup's start to last workgroup's end,
// queueing for compute units included — which is what a stream is busy for).  One wait for the stream + one small copy, once per plan: its third pass, which is
// still a warm-up pass of bench.py.  The deal stays as it is where a launch's clocks are not of one pass.
static int redeal_by_in_pass_clocks(cl_context* ctx, cl_stitch_plan* pl) {
    { int rc = plan_mark_stop(ctx, pl); if (rc) return rc; }
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    const size_t ng = pl->groups.size();
    std::vector<unsigned long long> got(2 * ng);
    HIP_TRY(ctx, cl_copy_sync(ctx, got.data(), pl->d_ticks.p, got.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    for (size_t gi = 0; gi < ng; ++gi)
        if (!(tick_span_us(got[2 * gi], got[2 * gi + 1]) > 0)) return CL_OK;
    for (size_t gi = 0; gi < ng; ++gi) pl->groups[gi].est_cost = (uint64_t)tick_span_us(got[2 * gi], got[2 * gi + 1]) + 1;
    sort_groups_by_cost(pl);
    return CL_OK;
}

int cl_stitch_plan_execute(cl_context* ctx, cl_stitch_plan* pl) {
    if (!ctx || !pl) { set_error(ctx, "null argument"); return CL_ERR_INVALID_ARGUMENT; }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    ++cl_fallbacks.stitch_plans;
    // a plan of more than two launches is dealt over the streams again in front of its second pass and, once, in front of the pass after that
    if (pl->groups.size() > 2) {
        int rc = CL_OK;
        if (pl->executed && !pl->calibrated) {
            pl->calibrated = true;
            rc = redeal_by_solo_durations(ctx, pl);
        } else if (pl->calibrated && pl->redeals_left > 0 && pl->d_ticks.p) {
            --pl->redeals_left;
            rc = redeal_by_in_pass_clocks(ctx, pl);
        }
        if (rc) return rc;
    }
    HIP_TRY(ctx, hipEventRecord(pl->ev_start, ctx->stream));
    int rc = enqueue_groups(ctx, pl);
    if (rc) return rc;
    pl->executed = true;
    return CL_OK;
}

int cl_stitch_plan_execute_profiled(cl_context* ctx, cl_stitch_plan* pl) {
    if (!ctx || !pl) { set_error(ctx, "null argument"); return CL_ERR_INVALID_ARGUMENT; }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    { int rc = plan_mark_stop(ctx, pl); if (rc) return rc; }
    HIP_TRY(ctx, hipEventRecord(pl->ev_start, ctx->stream));
    int rc = profile_groups(ctx, pl);
    if (rc) return rc;
    HIP_TRY(ctx, hipEventRecord(pl->ev_stop, ctx->stream));
    pl->executed = true;
    pl->profiled = true;
    pl->tick_pass = 0;   // (the profiled launches left the highest pass number in the tick words: the next concurrent pass zeroes them)
    return CL_OK;
}

// A concurrent pass exactly as cl_stitch_plan_execute enqueues one — the same launches on the same streams, side by side, following the pass before in
// stream order — with a pair of HIP events round every launch ON ITS STREAM.  An event pair spans from the moment the stream reaches the launch (the end of whatever
// preceded it there) to the launch's completion, end-of-kernel cache write-back included: what the rocprofv3 kernel trace of a step shows as the dispatch's duration plus
// the stream's launch gap, i.e. an UPPER bound of the trace's duration where the kernel's own clock (first workgroup's start to last workgroup's end) is a lower bound.
// bench.py prices roofline.frac with these (round-5 verdict: the printed fraction must be the one profiles/ reproduces).
int cl_stitch_plan_execute_evented(cl_context* ctx, cl_stitch_plan* pl) {
    if (!ctx || !pl) { set_error(ctx, "null argument"); return CL_ERR_INVALID_ARGUMENT; }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipEventRecord(pl->ev_start, ctx->stream));
    pl->event_pass = true;
    const int rc = enqueue_groups(ctx, pl);
    pl->event_pass = false;
    if (rc) return rc;
    pl->executed = true;
    return CL_OK;
}

int cl_stitch_plan_sync(cl_context* ctx, cl_stitch_plan* pl, float* ms_out) {
    if (!ctx || !pl) { set_error(ctx, "null argument"); return CL_ERR_INVALID_ARGUMENT; }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    { int rc = plan_mark_stop(ctx, pl); if (rc) return rc; }
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (ms_out) {
        *ms_out = 0.f;   // (from the last pass's enqueue on the stream to its end: with passes enqueued back to back, the time they all took from there)
        if (pl->executed) HIP_TRY(ctx, hipEventElapsedTime(ms_out, pl->ev_start, pl->ev_stop));
    }
    return CL_OK;
}

int cl_stitch_plan_stats(const cl_stitch_plan* pl, cl_plan_stats* out) {
    if (!pl || !out) return CL_ERR_INVALID_ARGUMENT;
    *out = pl->stats;
    return CL_OK;
}

int cl_stitch_plan_launch_count(const cl_stitch_plan* pl) { return pl ? (int)pl->groups.size() : 0; }

// the kernel a launch group reports (cl_launch_info::kernel)
static void launch_kernel_name(const LaunchGroup& g, char* out, size_t cap) {
    switch (g.variant) {
    case LaunchVariant::Narrow: snprintf(out, cap, "popoa_narrow_kernel"); break;
    case LaunchVariant::ChainSpan: snprintf(out, cap, "popoa_linear_span_kernel"); break;
    case LaunchVariant::Quads: snprintf(out, cap, "popoa_linear_quad_kernel"); break;
    case LaunchVariant::Duos: snprintf(out, cap, "popoa_linear_duo_kernel"); break;
    case LaunchVariant::ChainPersistent: snprintf(out, cap, "popoa_chain_persistent_kernel"); break;
    case LaunchVariant::Chain: snprintf(out, cap, "popoa_linear_kernel<%d>", g.waves); break;
    case LaunchVariant::Lane: snprintf(out, cap, "popoa_lane_kernel<%d>", g.waves); break;
    case LaunchVariant::LaneWide: snprintf(out, cap, "popoa_lane_kernel<%d, wide>", g.waves); break;
    case LaunchVariant::Sys: snprintf(out, cap, "popoa_sys_kernel<%d, %d>", g.npw, g.block); break;
    case LaunchVariant::Strip: snprintf(out, cap, "popoa_strip_kernel<%d> x %d", g.npw, g.block); break;
    case LaunchVariant::General: snprintf(out, cap, "%s<%d, %d>", g.ring_bytes ? "popoa_ring_kernel" : "popoa_general_kernel", g.npw, g.block); break;
    case LaunchVariant::None: snprintf(out, cap, "none"); break;
    }
}

int cl_stitch_plan_launch_info(cl_context* ctx, const cl_stitch_plan* pl, int index, cl_launch_info* out) {
    if (!ctx || !pl || !out || index < 0 || index >= (int)pl->groups.size()) return CL_ERR_INVALID_ARGUMENT;
    const LaunchGroup& g = pl->groups[index];
    memset(out, 0, sizeof(*out));
    launch_kernel_name(g, out->kernel, sizeof(out->kernel));
    const bool strips = g.variant == LaunchVariant::Strip, narrow = g.variant == LaunchVariant::Narrow;
    out->n_problems = g.count;
    if (cl_launch_pair_spans_workgroups(g.variant)) {   // (a wide / spanning pair takes a workgroup per group of strips: count the pairs)
        out->n_problems = 0;
        for (uint32_t i = g.first; i < g.first + g.count; ++i) out->n_problems += i == g.first || pl->plist_host[i] != pl->plist_host[i - 1];
    }
    out->dp_cells = g.cells;
    out->dp_bytes = g.bytes;
    const bool chain = g.variant == LaunchVariant::Chain || g.variant == LaunchVariant::ChainSpan || cl_launch_list_padded(g.variant);
    out->lds_bytes = chain ? 0u : g.ring_bytes;
    if (cl_launch_list_padded(g.variant)) {   // (the quads' and duos' lists are padded with "no pair")
        out->n_problems = 0;
        for (uint32_t i = g.first; i < g.first + g.count; ++i) out->n_problems += pl->plist_host[i] != 0xFFFFFFFFu;
    }
    auto sweep_of = [&](uint32_t i) {
        if (!strips && pl->plist_host[i] == 0xFFFFFFFFu) return;
        const ClProbDesc& d = pl->desc[strips ? pl->strips[pl->strip_list[i]].prob : pl->plist_host[i]];
        if (d.n1 + d.n2 > out->max_sweep) { out->max_sweep = d.n1 + d.n2; out->max_n1 = d.n1; out->max_n2 = d.n2; }
    };
    if (narrow) {   // (the members' lists: a workgroup per pair)
        for (uint32_t r = 0; r < pl->narrow.n; ++r)
            for (uint32_t i = 0; i < pl->narrow.end[r] - (r ? pl->narrow.end[r - 1] : 0u); ++i) sweep_of(pl->narrow.first[r] + i);
    }
    for (uint32_t i = g.first; !narrow && i < g.first + g.count; ++i) sweep_of(i);
    if (pl->profiled) out->last_ms = g.host_ms;
    if (g.evented && hipEventQuery(g.ev1) == hipSuccess) {
        float ems = 0.f;
        if (hipEventElapsedTime(&ems, g.ev0, g.ev1) == hipSuccess) out->event_ms = ems;
        else (void)hipGetLastError();
    }
    if (pl->d_ticks.p && pl->executed) {   // the launch's own clock in the last pass (the caller has waited for it: cl_stitch_plan_sync)
        unsigned long long got[2] = {0, 0};
        HIP_TRY(ctx, hipSetDevice(ctx->device));
        if (cl_copy_sync(ctx, got, pl->d_ticks.p + 2 * index, sizeof(got), hipMemcpyDeviceToHost) == hipSuccess && tick_span_us(got[0], got[1]) > 0)
            out->in_pass_ms = (float)(tick_span_us(got[0], got[1]) * 1e-3);
    }
    return CL_OK;
}

int cl_stitch_plan_collect(cl_context* ctx, cl_stitch_plan* pl, cl_stitch_result* out) {
    if (!ctx || !pl || !out) { set_error(ctx, "null argument"); return CL_ERR_INVALID_ARGUMENT; }
    memset(out, 0, sizeof(*out));
    if (!pl->executed && !pl->desc.empty()) { set_error(ctx, "plan was not executed"); return CL_ERR_INVALID_ARGUMENT; }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    { int rc = plan_mark_stop(ctx, pl); if (rc) return rc; }
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    const size_t npo = pl->desc.size();
    PlanOutputs got;
    { int rc = download_outputs(ctx, pl, got); if (rc) return rc; }
    {
        // a chain pair whose groups gave up waiting for one another (popoa_linear_span_kernel) is run again by the one-workgroup chain kernel: same codes, same hand-off rows
        std::vector<uint32_t> chain_again, redo[4];
        // ... and a pair whose strips did (popoa_strip_kernel's waits are bounded, and the strips of a launch can be kept apart by whatever else crowds the device)
        // by the anti-diagonal kernel
        for (size_t i = 0; i < npo; ++i) {
            if (got.status[i] != 9) continue;
            if (pl->desc[i].kind == CL_KIND_LINEAR) chain_again.push_back((uint32_t)i);
            else if (pl->desc[i].kind == CL_KIND_STRIP || pl->desc[i].kind == CL_KIND_LANE) redo[pl->desc[i].npw].push_back((uint32_t)i);
        }
        bool any = false;
        if (!chain_again.empty()) {
            any = true;
            int rc = rerun_pairs(ctx, pl, chain_again, "chain pairs on one workgroup each", [&](const ClDeviceBatch& dev, const uint32_t* list, uint32_t count) {
                return cl_launch_popoa_linear(16, count, dev, list, pl->sparams, ctx->stream); });
            if (rc) return rc;
        }
        for (int npw = 1; npw <= 3; ++npw) {
            if (redo[npw].empty()) continue;
            any = true;
            int rc = rerun_pairs(ctx, pl, redo[npw], "pairs on the anti-diagonal kernel", [&](const ClDeviceBatch& dev, const uint32_t* list, uint32_t count) {
                return cl_launch_popoa_general(npw, 1024, count, 0, dev, list, pl->sparams, ctx->stream); });
            if (rc) return rc;
        }
        if (any) { int rc = download_outputs(ctx, pl, got); if (rc) return rc; }
    }
    const uint64_t n = pl->n_problems;
    uint64_t total = 0;
    for (size_t i = 0; i < npo; ++i) {
        if (got.status[i] != 0) {
            set_error(ctx, "device traceback failed on problem %llu (status %u): no source..sink connection or corrupt input",
                      (unsigned long long)pl->po_problem[i], got.status[i]);
            return CL_ERR_UNREACHABLE_SINK;
        }
        total += got.len[i];
    }
    for (uint32_t k : pl->pd_problem) total += pl->pd_path[k].size();
    for (uint32_t k : pl->host_problem) total += pl->host_aln[k].size();
    out->n_problems = n;
    out->aln_off = (uint64_t*)calloc(n + 1, sizeof(uint64_t));
    out->pairs = (uint64_t*)malloc((total ? total : 1) * 2 * sizeof(uint64_t));
    out->score = (int64_t*)calloc(n ? n : 1, sizeof(int64_t));
    out->route = (uint8_t*)calloc(n ? n : 1, 1);
    out->num_pw = (uint8_t*)calloc(n ? n : 1, 1);
    if (!out->aln_off || !out->pairs || !out->score || !out->route || !out->num_pw) {
        cl_stitch_result_free(out);
        return CL_ERR_OUT_OF_MEMORY;
    }
    uint64_t cur = 0;
    for (uint64_t k = 0; k < n; ++k) {
        out->route[k] = pl->route[k];
        out->num_pw[k] = pl->num_pw[k];
        const uint64_t nb1 = pl->node_off[0][k], nb2 = pl->node_off[1][k];
        if (pl->po_index[k] >= 0) {
            const size_t i = (size_t)pl->po_index[k];
            const ClProbDesc& d = pl->desc[i];
            const uint32_t cap = d.n1 + d.n2;
            const uint32_t len = got.len[i];
            const uint2* src = got.pairs.data() + d.out_base + (cap - len);
            const uint32_t* o1 = pl->order[0].data() + d.node_base[0];
            const uint32_t* o2 = pl->order[1].data() + d.node_base[1];
            for (uint32_t t = 0; t < len; ++t) {
                // rank+1 -> local id -> (translate, src/alignment.cpp:26-39) caller id
                uint64_t a = CL_GAP, b = CL_GAP;
                if (src[t].x) { a = o1[src[t].x - 1]; if (pl->has_back[0]) a = pl->back[0][nb1 + a]; }
                if (src[t].y) { b = o2[src[t].y - 1]; if (pl->has_back[1]) b = pl->back[1][nb2 + b]; }
                out->pairs[2 * cur] = a;
                out->pairs[2 * cur + 1] = b;
                ++cur;
            }
            out->score[k] = got.score[i];
        } else if (pl->route[k] != CL_ROUTE_PURE_DELETION_1 && pl->route[k] != CL_ROUTE_PURE_DELETION_2) {
            for (const auto& pr : pl->host_aln[k]) {
                uint64_t a = pr.first, b = pr.second;
                if (a != CL_GAP && pl->has_back[0]) a = pl->back[0][nb1 + a];
                if (b != CL_GAP && pl->has_back[1]) b = pl->back[1][nb2 + b];
                out->pairs[2 * cur] = a;
                out->pairs[2 * cur + 1] = b;
                ++cur;
            }
            out->score[k] = 0;   // do_alignment does not ask the heuristics for a score (stitcher.hpp:304-345)
        } else {
            const std::vector<uint32_t>& path = pl->pd_path[k];
            const bool first = pl->route[k] == CL_ROUTE_PURE_DELETION_1;
            for (uint32_t v : path) {
                uint64_t id = v;
                if (first) { if (pl->has_back[0]) id = pl->back[0][nb1 + v]; }
                else if (pl->has_back[1]) id = pl->back[1][nb2 + v];
                out->pairs[2 * cur] = first ? id : CL_GAP;       // swap_graphs for the graph2 case (src/alignment.cpp:41-45)
                out->pairs[2 * cur + 1] = first ? CL_GAP : id;
                ++cur;
            }
            out->score[k] = pure_deletion_score(path.size(), pl->num_pw[k], pl->aparams);
        }
        out->aln_off[k + 1] = cur;
    }
    return CL_OK;
}

void cl_stitch_plan_destroy(cl_context* ctx, cl_stitch_plan* pl) {
    if (ctx) (void)hipSetDevice(ctx->device);
    cl_stitch_plan_free(pl);
}

static int run_chunk(cl_context* ctx, const cl_stitch_batch* batch, const cl_stitch_params* sp, const uint8_t* force, cl_stitch_result* out);

// A plan holds one workspace for its whole batch: full score planes for every graph x graph subproblem that is not swept from LDS, addressed
// with 32-bit word offsets.  A merge whose gaps add up to more than that (several graph x graph gaps near the 40 M-cell ceiling of
// min_wfa_size, src/parameters.cpp:79; configs[4]-sized merges) is run as consecutive chunks of subproblems, each a plan of its own on the
// same context, the results appended in order.  CL_STITCH_WORKSPACE_WORDS (default 3 * 2^30 int32 words = 12 GB) for tests.
static int run_whole(cl_context* ctx, const cl_stitch_batch* batch, const cl_stitch_params* sp, const uint8_t* force,
                     cl_stitch_result* out) {
    const char* cap_env = getenv("CL_STITCH_WORKSPACE_WORDS");
    const uint64_t cap = cap_env && atoll(cap_env) > 0 ? (uint64_t)atoll(cap_env) : (3ull << 30);
    const uint64_t n = batch->n_problems;
    std::vector<uint64_t> cuts(1, 0);
    uint64_t acc = 0;
    for (uint64_t k = 0; k < n; ++k) {
        const uint64_t n1 = batch->side[0].node_off[k + 1] - batch->side[0].node_off[k], n2 = batch->side[1].node_off[k + 1] - batch->side[1].node_off[k];
        const uint64_t words = (n1 + 1) * (n2 + 1) * 7;   // the planes of a NumPW = 3 matrix: an upper bound whatever kernel takes it
        if (acc && acc + words > cap) { cuts.push_back(k); acc = 0; }
        acc += words;
    }
    cuts.push_back(n);
    if (cuts.size() == 2) return run_chunk(ctx, batch, sp, force, out);
    memset(out, 0, sizeof(*out));
    std::vector<cl_stitch_result> parts(cuts.size() - 1);
    int rc = CL_OK;
    size_t done = 0;
    for (; done + 1 < cuts.size() && !rc; ++done) {
        cl_stitch_batch sub = *batch;
        const uint64_t a = cuts[done];
        sub.n_problems = cuts[done + 1] - a;
        for (int s = 0; s < 2; ++s) { sub.side[s].node_off += a; sub.side[s].src_off += a; sub.side[s].snk_off += a; }
        if (sub.only_deletion_alns) sub.only_deletion_alns += a;
        rc = run_chunk(ctx, &sub, sp, force ? force + a : nullptr, &parts[done]);
    }
    if (!rc) {
        uint64_t total_pairs = 0;
        for (size_t i = 0; i < done; ++i) total_pairs += parts[i].aln_off[parts[i].n_problems];
        out->n_problems = n;
        out->aln_off = (uint64_t*)malloc((n + 1) * sizeof(uint64_t));
        out->pairs = (uint64_t*)malloc((total_pairs ? total_pairs : 1) * 2 * sizeof(uint64_t));
        out->score = (int64_t*)malloc((n ? n : 1) * sizeof(int64_t));
        out->route = (uint8_t*)malloc(n ? n : 1);
        out->num_pw = (uint8_t*)malloc(n ? n : 1);
        if (!out->aln_off || !out->pairs || !out->score || !out->route || !out->num_pw) { cl_stitch_result_free(out); rc = CL_ERR_OUT_OF_MEMORY; }
        else {
            uint64_t pair_at = 0;
            for (size_t i = 0; i < done; ++i) {
                const cl_stitch_result& p = parts[i];
                const uint64_t a = cuts[i];
                for (uint64_t k = 0; k < p.n_problems; ++k) out->aln_off[a + k] = pair_at + p.aln_off[k];
                memcpy(out->pairs + 2 * pair_at, p.pairs, p.aln_off[p.n_problems] * 2 * sizeof(uint64_t));
                memcpy(out->score + a, p.score, p.n_problems * sizeof(int64_t));
                memcpy(out->route + a, p.route, p.n_problems);
                memcpy(out->num_pw + a, p.num_pw, p.n_problems);
                pair_at += p.aln_off[p.n_problems];
            }
            out->aln_off[n] = pair_at;
        }
    }
    for (size_t i = 0; i < done; ++i) cl_stitch_result_free(&parts[i]);
    return rc;
}

static int run_chunk(cl_context* ctx, const cl_stitch_batch* batch, const cl_stitch_params* sp, const uint8_t* force,
                     cl_stitch_result* out) {
    // CL_STITCH_TIMING=1: host phase times on stderr
    static const bool timing = getenv("CL_STITCH_TIMING") != nullptr;
    auto t = std::chrono::steady_clock::now();
    auto lap = [&](const char* what) {
        if (timing) fprintf(stderr, "[cl_stitch]   %-22s %8.2f ms\n", what, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t).count());
        t = std::chrono::steady_clock::now();
    };
    cl_stitch_plan* pl = nullptr;
    int rc = cl_stitch_plan_create(ctx, batch, sp, force, &pl);
    if (rc) return rc;
    lap("plan (host + upload)");
    rc = cl_stitch_plan_execute(ctx, pl);
    if (!rc && timing) { (void)hipStreamSynchronize(ctx->stream); lap("execute (device)"); }
    if (!rc) rc = cl_stitch_plan_collect(ctx, pl, out);
    lap("collect");
    cl_stitch_plan_destroy(ctx, pl);
    lap("free");
    return rc;
}


int cl_po_poa_batch(cl_context* ctx, const cl_stitch_batch* batch, const uint8_t* num_pw, const cl_align_params* params,
                    cl_stitch_result* out) {
    if (!ctx || !batch || !num_pw || !params || !out) { set_error(ctx, "null argument"); return CL_ERR_INVALID_ARGUMENT; }
    cl_stitch_params sp;
    cl_stitch_params_default(&sp);
    sp.alignment_params = *params;
    return run_whole(ctx, batch, &sp, num_pw, out);
}

int cl_stitch_batch_align(cl_context* ctx, const cl_stitch_batch* batch, const cl_stitch_params* params, cl_stitch_result* out) {
    if (!ctx || !batch || !params || !out) { set_error(ctx, "null argument"); return CL_ERR_INVALID_ARGUMENT; }
    return run_whole(ctx, batch, params, nullptr, out);
}

}  // extern "C"
