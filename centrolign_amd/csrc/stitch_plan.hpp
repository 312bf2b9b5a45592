// stitch_plan.hpp — a stitch plan (cl_stitch_plan): what its construction (cl_stitch_plan_api.cpp) leaves for its execution (cl_stitch_exec_api.cpp).
// Internal to those two translation units; not part of the public ABI.
#ifndef CL_STITCH_PLAN_HPP
#define CL_STITCH_PLAN_HPP

#include <memory>
#include <utility>
#include <vector>

#include "cl_internal.hpp"
#include "popoa_device.h"

// the launchers of the stitch kernels (popoa_kernels.hip, popoa_linear.hip) and the two device facts a plan's construction asks for
hipError_t cl_launch_popoa_lane(int W, uint32_t n_blocks, uint32_t lds_bytes, const ClDeviceBatch& B, const uint32_t* plist, const ClScoreParams& P, uint32_t* lane_sync /* null: one workgroup per pair */, hipStream_t stream);
hipError_t cl_launch_popoa_sys(int npw, int block, uint32_t n_blocks, uint32_t lds_bytes, const ClDeviceBatch& B, const uint32_t* plist,
                               const ClScoreParams& P, hipStream_t stream);
hipError_t cl_launch_popoa_strip(int npw, uint32_t threads, uint32_t n_blocks, uint32_t lds_bytes, const ClDeviceBatch& B, const ClStripDevice& SD, const uint32_t* slist,
                                 const ClScoreParams& P, hipStream_t stream);
hipError_t cl_launch_popoa_general(int npw, int block, uint32_t n_blocks, uint32_t ring_bytes, const ClDeviceBatch& B,
                                   const uint32_t* plist, const ClScoreParams& P, hipStream_t stream);
hipError_t cl_launch_popoa_linear(int W, uint32_t n_blocks, const ClDeviceBatch& B, const uint32_t* plist,
                                  const ClScoreParams& P, hipStream_t stream);
size_t cl_linear_workspace_bytes(uint32_t nr, uint32_t nc, int npw, int R);
hipError_t cl_launch_popoa_linear_span(uint32_t n_blocks, const ClDeviceBatch& B, const uint32_t* plist, const ClScoreParams& P, uint32_t* sync, hipStream_t stream);
uint32_t cl_linear_span_groups(uint32_t nr);
uint32_t cl_chain_persistent_capacity(int device);
uint32_t cl_narrow_capacity(int device, int threads, uint32_t lds_bytes);
hipError_t cl_launch_popoa_narrow(int threads, uint32_t n_blocks, uint32_t lds_bytes, const ClNarrowRoles& R, const ClDeviceBatch& B, const uint32_t* plist,
                                  const ClScoreParams* P, hipStream_t stream);
hipError_t cl_launch_popoa_chain_persistent(uint32_t n_blocks, uint32_t n_tasks, const ClDeviceBatch& B, const uint32_t* plist, const uint2* tasks,
                                            uint32_t* head, const ClScoreParams& P, hipStream_t stream);

typedef std::vector<std::pair<uint64_t, uint64_t>> HostAlignment;   // local node ids, CL_GAP for a gap

// Which launcher call a launch group is.  The device never sees this: what it reads (ClProbDesc::kind, pad, aux_base, aux_cnt, the persistent launch's task words,
// ClNarrowRoles::code) has values of its own.
enum class LaunchVariant : uint8_t {
    None,             // (per subproblem: not a chain pair — its ClProbDesc::kind says which kernel family takes it)
    Chain,            // popoa_linear_kernel<waves>: one chain pair per workgroup of 16 / 8 / 4 / 3 / 1 waves
    Quads,            // popoa_linear_quad_kernel: four chain pairs of at most 16 rows per wave; the list is padded with 0xFFFFFFFF
    Duos,             // popoa_linear_duo_kernel: two chain pairs of 17-32 rows per wave; padded likewise
    ChainSpan,        // popoa_linear_span_kernel: a chain pair's strips over several workgroups; progress words in lane_sync
    ChainPersistent,  // popoa_chain_persistent_kernel: the one-wave chain launches (Chain<1>, Quads, Duos) as one task queue; `grid` workgroups, prog_count tasks
    Lane,             // popoa_lane_kernel<waves>: a near-chain pair per workgroup
    LaneWide,         // popoa_lane_kernel<waves, wide>: a near-chain pair's groups of strips over several workgroups; progress words in lane_sync
    Sys,              // popoa_sys_kernel<npw, block>
    Strip,            // popoa_strip_kernel<npw>: first / count index cl_stitch_plan::strip_list; progress words in d_progress
    General,          // popoa_general_kernel / popoa_ring_kernel<npw, block> (ring_bytes: the ring variant)
    Narrow            // popoa_narrow_kernel: the one launch of the plan's ClNarrowRoles members (cl_stitch_plan::narrow)
};

// the chain kernel a chain pair (ClProbDesc::kind == CL_KIND_LINEAR) runs on: Chain (with its waves), Quads, Duos or ChainSpan; None for every other pair
struct ChainShape {
    LaunchVariant variant = LaunchVariant::None;
    uint8_t waves = 0;
};

struct LaunchGroup {
    LaunchVariant variant = LaunchVariant::None;
    int npw = 0;         // Sys, Strip, General: the members' NumPW (0: mixed)
    int block = 0;       // Sys, Strip, General, Narrow: workgroup size in threads
    int waves = 0;       // Chain, Lane, LaneWide: waves per workgroup
    uint32_t grid = 0;   // ChainPersistent: workgroups of the launch
    uint32_t first = 0;  // into plist
    uint32_t count = 0;
    uint64_t cells = 0, bytes = 0;
    uint32_t ring_bytes = 0;  // dynamic LDS of the launch (general kernel: 0 = planes read from HBM)
    uint32_t prog_first = 0, prog_count = 0;   // the progress words the launch zeroes first (Strip: of d_progress; LaneWide, ChainSpan: of d_lane_sync); ChainPersistent: prog_count = tasks
    uint64_t est_cost = 0;    // longest sweep x the kernel's rough time per step: orders the groups and deals them over the streams
    float host_ms = 0.f;      // the profiled pass: the launch alone on the device, behind another launch (host's clock: two launches - one launch)
    float host_idle_ms = 0.f; // ... and finding the device idle (one launch + wait)
    hipEvent_t ev0 = nullptr, ev1 = nullptr;   // cl_stitch_plan_execute_evented: HIP events round this launch on ITS stream in a concurrent pass
    bool evented = false;
};
// the variant's name in the scheduler's log (CL_STITCH_SCHED_LOG)
inline const char* cl_launch_variant_name(LaunchVariant v) {
    static const char* const names[] = {"none", "chain", "quads", "duos", "chain-span", "chain-persistent", "lane", "lane-wide", "sys", "strip", "general", "narrow"};
    return names[(int)v];
}
// a list padded with 0xFFFFFFFF ("no pair")
inline bool cl_launch_list_padded(LaunchVariant v) { return v == LaunchVariant::Quads || v == LaunchVariant::Duos || v == LaunchVariant::ChainPersistent; }
// a pair takes several consecutive workgroups of the launch, i.e. several entries of the list
inline bool cl_launch_pair_spans_workgroups(LaunchVariant v) { return v == LaunchVariant::LaneWide || v == LaunchVariant::ChainSpan; }

struct cl_stitch_plan {
    uint64_t n_problems = 0;
    cl_align_params aparams{};
    // per input problem
    std::vector<uint8_t> route, num_pw;
    std::vector<int32_t> po_index;                 // index among PO-POA problems or -1
    std::vector<std::vector<uint32_t>> pd_path;    // pure-deletion paths (local ids), indexed by input problem (sparse)
    std::vector<uint32_t> pd_problem;              // list of problems with a pd path
    std::vector<HostAlignment> host_aln;           // alignments made on the host (greedy route), indexed by input problem (sparse)
    std::vector<uint32_t> host_problem;
    // per PO-POA problem
    std::vector<ClProbDesc> desc;
    std::vector<ChainShape> chain_shape;           // which chain kernel takes it (None = not a chain pair)
    std::vector<uint64_t> po_problem;              // input problem index
    std::vector<uint32_t> order[2];                // rank -> local node id, concatenated (node_base)
    // translation back to caller ids
    std::vector<uint64_t> back[2];                 // copy of back_translation (or empty)
    std::vector<uint64_t> node_off[2];
    bool has_back[2] = {false, false};
    // device
    DevBuf<ClProbDesc> d_desc;
    DevBuf<uint32_t> d_aux;
    DevBuf<uint8_t> d_lab[2];
    DevBuf<uint32_t> d_poff[2], d_pidx[2], d_snk[2];
    DevBuf<int32_t> d_planes;
    DevBuf<uint2> d_out_pairs;
    DevBuf<uint32_t> d_out_len, d_out_status, d_plist;
    DevBuf<int32_t> d_out_score;
    // strips of rows (popoa_strip_kernel)
    std::vector<ClStripDesc> strips;
    std::vector<uint32_t> strip_list;              // the strip launch groups' lists (into strips)
    DevBuf<ClStripDesc> d_strips;
    DevBuf<uint4> d_strip_recs;
    DevBuf<uint32_t> d_strip_list, d_progress;
    DevBuf<unsigned long long> d_handoff;
    ClStripDevice sdev{};
    DevBuf<uint32_t> d_lane_sync;                  // wide near-chain pairs (popoa_lane_kernel) and spanning chain pairs: progress / done words per group, zeroed in front of every launch
    DevBuf<unsigned long long> d_ticks;            // [2 per launch group] the launches' own clocks (ClDeviceBatch::ticks), zeroed in front of every pass
    // the persistent launch of the one-wave chain kinds (popoa_chain_persistent_kernel): its task list {first into plist, kind << 24 | units}, longest first,
    // and its two queue words (next task, workgroups done), zero between passes
    DevBuf<uint2> d_ptasks;
    DevBuf<uint32_t> d_phead;
    ClNarrowRoles narrow{};                        // the members of the Narrow group, if there is one (popoa_narrow_kernel)
    DevBuf<ClScoreParams> d_sparams;               // ... and its copy of sparams (only where that group exists)
    std::vector<LaunchGroup> groups;
    ClDeviceBatch dev{};
    ClScoreParams sparams{};
    cl_plan_stats stats{};
    hipEvent_t ev_start = nullptr, ev_stop = nullptr;
    std::vector<uint32_t> plist_host;   // the launch groups' subproblem lists (cl_stitch_plan_launch_info)
    bool executed = false, profiled = false;
    bool calibrated = false;     // the launches have been dealt by their durations measured alone (cl_stitch_plan_execute: the first re-deal)
    int redeals_left = 1;        // ... and how often they are still dealt again by their clocks inside a pass (the second re-deal): once per plan
    uint32_t tick_pass = 0;      // number of the last concurrent pass (ClDeviceBatch::tick_pass), 1 .. 65 535
    bool event_pass = false;     // the pass being enqueued brackets every launch with HIP events (cl_stitch_plan_execute_evented)
    bool stop_pending = false;   // the last pass's end is not marked on the context's stream yet (lazy join)
};

// releases the plan's device blocks and events, then the plan (cl_stitch_exec_api.cpp)
void cl_stitch_plan_free(cl_stitch_plan* pl);
struct ClStitchPlanDeleter { void operator()(cl_stitch_plan* pl) const { cl_stitch_plan_free(pl); } };
typedef std::unique_ptr<cl_stitch_plan, ClStitchPlanDeleter> ClStitchPlanPtr;

#endif
