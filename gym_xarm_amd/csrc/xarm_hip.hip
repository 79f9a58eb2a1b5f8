// xarm_hip.hip - the C ABI (include/xarm_hip.h) of the batched Xarm environments: handles, kernel selection, launches.
// The gfx950 kernels live in xarm_k_*.hip, one translation unit per kernel family (prototypes: xarm_dev.h).
//
// What an environment kind is stands in ONE place, its KindOps entry (KIND_PNP .. KIND_REARRANGE below): dimensions, lanes per
// env, default limits and the init / reset / step / reward launches.  xarm_create validates the config, picks the entry and
// resolves the limits; every other entry point reads a field of h->ops or calls through it.  The caller's buffers travel as a
// StepIO and become kernel arguments in launch_step alone; the fast-step pipelines of PickAndPlace and Handover share one
// fork / join skeleton (pipelined_step); the slots of the device counter block are the CNT_* constants.
//
// PickAndPlace launches (xarm_k_pnp.hip, xarm_k_pnp_coop.hip; cores: xarm_core.h, xarm_coop_core.h):
//   k_step        one thread per environment, one 64-lane wavefront per workgroup.  The fused step keeps an env's whole
//                 working set on chip for all 15 substeps x 50 solver sweeps: ~450 VGPRs of per-env state / solver blocks
//                 (hence 1 wave per SIMD, __launch_bounds__(64)) plus 149 floats per env of LDS (hand Jacobian S, T =
//                 M^-1 S^T, A_hh, table slots: lane-private columns, 38 KB per workgroup).  65 536 envs = 1024 workgroups =
//                 4 per CU; workgroups never communicate, so no XCD-aware remap is needed.
//   k_step_fast_stage + k_step_coop_list_stage   the default for batches above 8 192 envs: the pad-free fast step in stages
//                 (three by default; XARM_PNP_STAGES=1: the one stage {0, 15}), the envs with an active finger-pad row handed
//                 off to the cooperative core from their stage's first substep on; hand-off lists above
//                 XARM_EJECT_COOP_CAP fall back to k_step_from_stage (one stage: k_step).  XarmHandover the same way at every
//                 batch size (xarm_k_handover_coop.hip: k_ho_step_fast + k_ho_step_coop_list, two 16-lane rows per env).
//   k_step_coop / k_reset_coop   one environment per DPP row of 16 lanes (4 per wavefront), impulse-space sweep spread
//                 over the row: the latency-optimal form for small batches and for the resets that follow a step.
//   k_reset       the one-env-per-lane reset, for bulk resets (> coop_limit finished envs in one call).
// HBM is touched once per env step: 54 state floats in, 54 out (structure-of-arrays, lane = env, every load/store a fully
// coalesced 256-B wave access), 4 action floats in and the 24+3+3+1 output floats + 2 flag bytes out (row-major at the
// API edge, 16-B vector stores).  Episodes that end are compacted into a list (one atomic per finished env) and
// re-initialised by the reset kernel inside the same xarm_step call.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <new>
#include "xarm_dev.h"
#include "xarm_render_core.h"
#include "xarm_her_core.h"
#include "xarm_norm_core.h"
#include "xarm_policy_core.h"
#include "xarm_a2c_core.h"
#include "xarm_ppo_core.h"
#include "xarm_sac_core.h"
#include "xarm_sacw_core.h"
#include "xarm_td3_core.h"
#include "xarm_acw_core.h"
#include "xarm_ppow_core.h"
#include "xarm_a2cw_core.h"
#include "xarm_rollout_core.h"
#include "xarm_replay_core.h"
#include "xarm_eval_core.h"

using namespace xd;

struct KindOps;

// ------------------------------------------------------------------------------------- C ABI
struct xarm_handle {
    xarm_config cfg;
    const KindOps *ops;  // the env kind's table entry, picked once by xarm_create
    KParams kp;
    int *done_list;   // [E] episodes that ended in this call (list A)
    int *counters;    // [CNT_INTS], slots CNT_*: the leading step_counter_ints() zeroed by ONE memset at the start of every step
                      // call (no host-side state: a captured step can be replayed)
    int *mask_count;  // [1]
    int coop_step_limit; // PickAndPlace, Reach, Handover (one stick): batches of at most this many envs step on the cooperative kernel
    int fast_pipeline;   // PickAndPlace, larger batches: k_step_fast_stage + hand-off of the envs with finger-pad rows (1) or k_step (0)
    int *eject_list;     // [stages][E] envs handed off by the fast kernel, one list per stage
    // the two reset launches of a pipelined step (xarm_step): episodes that ended in the fast kernel are reset on `side`
    // while the hand-off still runs on the caller's stream, the few that end in the hand-off after it
    int *done_list_b;    // [E] episodes that ended in the hand-off kernels (reset_per_stage: [stages][E], one list per hand-off stage)
    hipStream_t side;
    hipEvent_t ev_fork, ev_join;
    int reset_overlap;   // PickAndPlace pipeline with auto-reset only (xarm_create)
    int reset_per_stage; // reset_overlap and ho_stages > 1: every hand-off stage resets its own finished envs behind its hand-off
                         // (XARM_RESET_PER_STAGE=0: one list B for all stages, reset after the last hand-off)
    // staged step (pipelined_step): the fast kernel runs the step's 15 ticks in ho_stages launches; the envs a stage hands off
    // re-run only the ticks from that stage's first one on the cooperative rows, on a side stream beside the next stage
    static constexpr int MAX_ST = XARM_HO_MAX_STAGES;
    int ho_stages;        // 1 = one fast launch, one hand-off
    int ho_tick[MAX_ST + 1]; // stage c runs the ticks [ho_tick[c], ho_tick[c + 1])
    float *ho_qt;         // [18][stride] joint targets of the step the first stage opened (ho_stages > 1)
    uint8_t *ho_flag;     // [stride] handed off in an earlier stage of this call (every pipelined handle)
    hipStream_t st_side[MAX_ST];
    hipEvent_t st_fork[MAX_ST], st_join[MAX_ST];
    int ho_force_coupled; // test hook (XARM_HO_FORCE_COUPLED=1): every substep of the cooperative Handover step through the coupled sweep
    // StackTower / Rearrange: class-homogeneous wavefronts (xarm_stack_core.h class_layout); null when XARM_*_CLASS_ORDER=0
    uint8_t *class_key;  // [E] row-set class of each env's last substep
    int *class_order;    // [E] slot -> env
    char err[512];
    // timing
    int timing;
    static constexpr int NEV = 1024;
    hipEvent_t ev0[NEV], ev1[NEV], ev2[NEV];   // before the step kernel, after it, after the reset kernels
    int ev_n;
    double ev_ms, ev_reset_ms;
    int64_t ev_launches;
    bool ev_created;
};

// The device counter block.  The class histogram (2 * ncls ints: histogram, then the per-class arrival counters) and the
// hand-off counts of the stages >= 1 SHARE the region from CNT_REGION on: no kind has both a class order and a pipeline.
enum { CNT_DONE = 0,      // episodes that ended in this call (list A)
       CNT_EJECT = 1,     // envs handed off by the first fast stage
       CNT_DONE_B = 2,    // episodes that ended in the hand-off kernels (list B)
       CNT_REGION = 3 };
static constexpr int cnt_stage(int c) { return c == 0 ? (int)CNT_EJECT : CNT_REGION + c; }   // hand-off count of stage c
// episodes that ended in the hand-off of stage c (reset_per_stage; otherwise every stage counts in CNT_DONE_B)
static constexpr int cnt_done_b(int c) { return c == 0 ? (int)CNT_DONE_B : cnt_stage(xarm_handle::MAX_ST) + c; }
constexpr int CNT_STAGE_INTS = cnt_done_b(xarm_handle::MAX_ST) + 1;   // what a staged step clears and xarm_debug_counts reads
constexpr int CNT_INTS = CNT_REGION + 2 * xra::NCLS;                 // the allocation
static_assert(xra::NCLS >= xs::NCLS && CNT_STAGE_INTS <= CNT_INTS, "one counter block serves both class orders and the stage counters");

static char g_err[512] = "";

static int fail(xarm_handle *h, int code, const char *fmt, const char *detail) {
    char *dst = h ? h->err : g_err;
    snprintf(dst, 512, fmt, detail);
    return code;
}
#define HIPCHK(h, call)                                                          \
    do {                                                                         \
        hipError_t _e = (call);                                                  \
        if (_e != hipSuccess) return fail(h, XARM_E_HIP, #call ": %s", hipGetErrorString(_e)); \
    } while (0)

// ------------------------------------------------------------------------------------- launches
// the eight caller buffers of xarm_step; expanded into kernel arguments in launch_step only (the kernels keep their
// __restrict__ pointer parameters)
struct StepIO {
    const float *actions;
    float *obs, *ag, *dg, *reward;
    uint8_t *done, *success;
    float *terminal_obs;
};
// every step kernel: (KParams, the eight buffers, then what the family adds - done list and count, hand-off list, stage ...)
template <typename... KA, typename... A>
static void launch_step(void (*k)(KParams, const float *, float *, float *, float *, float *, uint8_t *, uint8_t *, float *, KA...), unsigned grid,
                        hipStream_t st, const xarm_handle *h, const StepIO &io, A... tail) {
    k<<<dim3(grid), dim3(WG), 0, st>>>(h->kp, io.actions, io.obs, io.ag, io.dg, io.reward, io.done, io.success, io.terminal_obs, tail...);
}
// the Handover kernels are templates over the scene; the cooperative ones also over the test hook FORCE_COUPLED
#define HO_KERNEL(h, K) ((h)->kp.hcfg.use_stand ? K<xh::HandoverStandScene> : K<xh::HandoverScene>)
#define HO_COOP_KERNEL(h, K) \
    ((h)->kp.hcfg.use_stand ? K<xh::HandoverStandScene, false> : ((h)->ho_force_coupled ? K<xh::HandoverScene, true> : K<xh::HandoverScene, false>))

struct KindOps {
    xarm_dims_t dims;
    int steps_field;         // state row of the episode's step counter
    int lanes;               // lanes per env: the grid of a whole-batch launch is lanes * stride / WG
    int reset_coop_default, step_coop_default;   // cooperative reset / step kernels: default limits (0: the kind has none)
    int stages_default;      // fast-step pipeline: default stage count and the variable that overrides it (null: no pipeline)
    const char *stages_env;
    int unstaged_ticks;      // what xarm_stage_info reports as the one stage of an unstaged step (0: nothing)
    int ncls;                // class order: classes and the variable that switches it off (0, null: none)
    const char *class_env;
    void (*init)(xarm_handle *h);
    // reset of the envs in list[0 .. *count) (null: all)
    void (*reset)(xarm_handle *h, const int *list, const int *count, float *obs, float *ag, float *dg, hipStream_t st);
    int (*step)(xarm_handle *h, const StepIO &io, hipStream_t st);
    void (*reward)(xarm_handle *h, const float *ag, const float *g, int64_t n, float *out, hipStream_t st);
    int fixed_reward_type;   // the reward type that cannot be relabelled and xarm_compute_reward's message for it (null: none)
    const char *fixed_reward_msg;
};

static int *slot(const xarm_handle *h, int s) { return h->counters + s; }
static unsigned env_grid(const xarm_handle *h) { return (unsigned)(h->ops->lanes * h->kp.stride / WG); }
static bool small_batch(const xarm_handle *h) { return h->kp.num_envs <= (int64_t)h->coop_step_limit; }   // steps on the cooperative kernel
static int64_t capped(const xarm_handle *h, int limit) { return h->kp.num_envs < (int64_t)limit ? h->kp.num_envs : (int64_t)limit; }
// grid of a cooperative PickAndPlace / Reach launch over at most `cap` envs: four envs per wavefront
static unsigned coop_grid(int64_t cap) { return (unsigned)((cap + COOP_ENVS - 1) / COOP_ENVS); }
// grid of a cooperative Handover launch over at most `cap` envs: two envs per wavefront, grid stride beyond 2 048 workgroups
static unsigned ho_coop_grid(int64_t cap) {
    const int64_t g = (cap + xhc::ROW_ENVS - 1) / xhc::ROW_ENVS;
    return (unsigned)(g < 1 ? 1 : (g > 2048 ? 2048 : g));
}

template <auto K> static void init_with(xarm_handle *h) { K<<<dim3(env_grid(h)), dim3(WG)>>>(h->kp); }

using ResetKernel = void (*)(KParams, const int *, const int *, float *, float *, float *);
// the cooperative kernel takes counts up to kp.coop_limit, the one-env-per-lane (Handover: lane-pair) kernel the rest; both
// are launched, the one out of its range exits at once (the count lives on the device)
// lane_first: the lane kernel in front (the two are exclusive by count, so the order does not touch results) - for a short list at the
// end of a latency chain, where the cooperative kernel does the work and the empty lane launch would otherwise end the chain
static void split_reset(xarm_handle *h, ResetKernel coop, unsigned (*cgrid)(int64_t), ResetKernel lane, const int *list, const int *count,
                        float *obs, float *ag, float *dg, hipStream_t st, bool lane_first = false) {
    const int64_t cap = capped(h, h->kp.coop_limit);
    if (lane_first && h->kp.num_envs > cap) lane<<<dim3(env_grid(h)), dim3(WG), 0, st>>>(h->kp, list, count, obs, ag, dg);
    if (cap > 0) coop<<<dim3(cgrid(cap)), dim3(WG), 0, st>>>(h->kp, list, count, obs, ag, dg);
    if (!lane_first && h->kp.num_envs > cap) lane<<<dim3(env_grid(h)), dim3(WG), 0, st>>>(h->kp, list, count, obs, ag, dg);
}
static void pnp_reset(xarm_handle *h, const int *list, const int *count, float *obs, float *ag, float *dg, hipStream_t st) {
    split_reset(h, k_reset_coop, coop_grid, k_reset, list, count, obs, ag, dg, st);
}
static void reach_reset(xarm_handle *h, const int *list, const int *count, float *obs, float *ag, float *dg, hipStream_t st) {
    split_reset(h, k_reach_reset_coop, coop_grid, k_reach_reset, list, count, obs, ag, dg, st);
}
static void ho_reset(xarm_handle *h, const int *list, const int *count, float *obs, float *ag, float *dg, hipStream_t st) {
    split_reset(h, HO_COOP_KERNEL(h, k_ho_reset_coop), ho_coop_grid, HO_KERNEL(h, k_ho_reset), list, count, obs, ag, dg, st);
}
static void ho2_reset(xarm_handle *h, const int *list, const int *count, float *obs, float *ag, float *dg, hipStream_t st) {
    HO_KERNEL(h, k_ho2_reset)<<<dim3(env_grid(h)), dim3(WG), 0, st>>>(h->kp, list, count, obs, ag, dg);
}
template <auto K>   // StackTower, Rearrange: the reset also writes the env's class key
static void keyed_reset(xarm_handle *h, const int *list, const int *count, float *obs, float *ag, float *dg, hipStream_t st) {
    K<<<dim3(env_grid(h)), dim3(WG), 0, st>>>(h->kp, list, count, obs, ag, dg, h->class_key);
}

template <auto K> static void typed_reward(xarm_handle *h, const float *ag, const float *g, int64_t n, float *out, hipStream_t st) {
    K<<<dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st>>>(h->cfg.reward_type, ag, g, n, out);
}
template <auto K> static void sparse_reward(xarm_handle *h, const float *ag, const float *g, int64_t n, float *out, hipStream_t st) {
    K<<<dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st>>>(ag, g, n, out);
}

// The fast-step pipeline of PickAndPlace and Handover: every env on the pad-free fast step; the ones with an active finger-pad
// row are handed off, untouched, to the cooperative kernel (lists of at most eject_coop_cap envs) or to the one-env-per-lane
// kernel (longer lists) - both launched, the one out of its range exits at once (the count lives on the device).
// STAGED (ho_stages > 1): the fast kernel runs the 15 ticks in ho_stages launches.  An env whose pads come alive in stage c keeps
// the state it had before that stage and re-runs the ticks from the stage's first one in the hand-off kernels - on a side stream,
// beside the next fast stage (16 384 Handover envs are 512 of the 1 024 SIMDs); only the last stage's hand-off, a third of a step
// long, is on the critical path: Handover's fast 0.73 + hand-off 0.69 ms became 0.77 + 0.27.
//   fast        launches fast stage c on the caller's stream
//   handoff     launches the hand-off of stage c on hs (and what belongs behind it on hs: PickAndPlace's per-stage reset)
//   after_fast  hook, after the last fast stage and before its hand-off (null: none)
// The side streams are joined here, or - reset_per_stage - by xarm_step behind the last stage's reset (join_stages).
static int join_stages(xarm_handle *h, hipStream_t st) {
    for (int c = 0; c + 1 < h->ho_stages; c++) HIPCHK(h, hipStreamWaitEvent(st, h->st_join[c], 0));
    return XARM_OK;
}
static int pipelined_step(xarm_handle *h, const StepIO &io, hipStream_t st,
                          void (*fast)(xarm_handle *, const StepIO &, int *elist, int *ecnt, HoStage, hipStream_t),
                          void (*handoff)(xarm_handle *, const StepIO &, int c, int *elist, int *ecnt, HoStage rest, hipStream_t hs),
                          int (*after_fast)(xarm_handle *, const StepIO &, hipStream_t)) {
    static_assert(xm::HO_N_TICKS == xm::PNP_N_SUBSTEPS, "one stage table for both");
    const int nst = h->ho_stages;
    for (int c = 0; c < nst; c++) {
        const HoStage sg{h->ho_tick[c], h->ho_tick[c + 1], h->ho_qt, h->ho_flag};
        int *elist = h->eject_list + (int64_t)c * h->kp.stride, *ecnt = slot(h, cnt_stage(c));
        fast(h, io, elist, ecnt, sg, st);
        hipStream_t hs = st;
        if (c + 1 < nst) {
            hs = h->st_side[c];
            HIPCHK(h, hipEventRecord(h->st_fork[c], st));
            HIPCHK(h, hipStreamWaitEvent(hs, h->st_fork[c], 0));
        } else if (after_fast) {
            const int rc = after_fast(h, io, st);
            if (rc != XARM_OK) return rc;
        }
        // one done list for every kernel of the call (atomic appends), the reset after the last hand-off (PickAndPlace: pnp_handoff)
        const HoStage rest{sg.tick0, xm::HO_N_TICKS, h->ho_qt, h->ho_flag};
        handoff(h, io, c, elist, ecnt, rest, hs);
        if (c + 1 < nst) HIPCHK(h, hipEventRecord(h->st_join[c], hs));
    }
    return h->reset_per_stage ? XARM_OK : join_stages(h, st);
}

// PickAndPlace.  The unstaged pipeline (XARM_PNP_STAGES=1) is the one stage {0, 15} of the same kernels, as for Handover.
static void pnp_fast(xarm_handle *h, const StepIO &io, int *elist, int *ecnt, HoStage sg, hipStream_t st) {
    launch_step(k_step_fast_stage, env_grid(h), st, h, io, h->done_list, slot(h, CNT_DONE), elist, ecnt, sg);
}
// With the reset overlap the episodes that end in the hand-off go to a list of their own (done_list_b): the reset of the ~98 %
// that ended on the fast path need not wait for it.  Without the side stream (XARM_RESET_OVERLAP=0): one list, one reset after
// the hand-off.
// reset_per_stage: the hand-off of stage c appends to a list of its own (b_stage(c)), and every stage but the last resets that list on its
// side stream directly behind its hand-off - stream order is the dependency (terminal_obs / done / success / reward of an env are
// written by its step kernel before its reset), and st_join[c], recorded by pipelined_step behind this, covers the reset.  A finished
// stage-0 hand-off env starts its reset when ITS hand-off ends, not when the last stage's does, and shares reset wavefronts with envs of
// its own stage only (DESIGN.md 4b "Resets per hand-off stage").  The last stage's list: xarm_step, on the caller's stream.
static int b_stage(const xarm_handle *h, int c) { return h->reset_per_stage ? c : 0; }
static int *b_list(const xarm_handle *h, int c) { return h->done_list_b + (int64_t)b_stage(h, c) * h->kp.stride; }
static void pnp_reset_b(xarm_handle *h, const StepIO &io, int c, hipStream_t st) {
    split_reset(h, k_reset_coop, coop_grid, k_reset, b_list(h, c), slot(h, cnt_done_b(b_stage(h, c))), io.obs, io.ag, io.dg, st, h->reset_per_stage != 0);
}
static void pnp_handoff(xarm_handle *h, const StepIO &io, int c, int *elist, int *ecnt, HoStage rest, hipStream_t hs) {
    int *list_b = h->reset_overlap ? b_list(h, c) : h->done_list, *cnt_b = slot(h, h->reset_overlap ? cnt_done_b(b_stage(h, c)) : (int)CNT_DONE);
    const int64_t cap = capped(h, h->kp.eject_coop_cap);
    const unsigned cgrid = coop_grid(cap) < 1024u ? coop_grid(cap) : 1024u;
    launch_step(k_step_coop_list_stage, cgrid, hs, h, io, list_b, cnt_b, elist, ecnt, rest);
    if (h->kp.num_envs > cap) {
        // the long-list fall-back (lists above eject_coop_cap): k_step for an unstaged step, k_step_from_stage for a staged one
        if (h->ho_stages > 1) launch_step(k_step_from_stage, env_grid(h), hs, h, io, list_b, cnt_b, elist, ecnt, rest);
        else launch_step(k_step, env_grid(h), hs, h, io, list_b, cnt_b, elist, ecnt);
    }
    if (h->reset_per_stage && c + 1 < h->ho_stages) pnp_reset_b(h, io, c, hs);
}
// a reset is six sequential ticks of latency on a few hundred wavefronts (2.9 ms), the hand-off 0.55 ms on a few hundred
// others: started after the last fast stage on the side stream, the first reset overlaps the hand-off.  The call still waits
// for the second one - a few dozen envs, but the ones with a finger contact, whose reset carries the pad rows through the
// homing ticks (worth 0.16 ms per call at 16 384 envs, nothing at 65 536) - which is why the staged step resets them
// per hand-off stage (pnp_handoff): the stage-0 envs, the ones that keep the pad rows, start 0.2 ms earlier
static int pnp_overlapped_reset(xarm_handle *h, const StepIO &io, hipStream_t st) {
    if (!h->reset_overlap) return XARM_OK;
    HIPCHK(h, hipEventRecord(h->ev_fork, st));
    HIPCHK(h, hipStreamWaitEvent(h->side, h->ev_fork, 0));
    pnp_reset(h, h->done_list, slot(h, CNT_DONE), io.obs, io.ag, io.dg, h->side);
    HIPCHK(h, hipEventRecord(h->ev_join, h->side));
    return XARM_OK;
}
static int pnp_step(xarm_handle *h, const StepIO &io, hipStream_t st) {
    if (small_batch(h)) launch_step(k_step_coop, coop_grid(h->kp.num_envs), st, h, io, h->done_list, slot(h, CNT_DONE));
    else if (h->fast_pipeline) return pipelined_step(h, io, st, pnp_fast, pnp_handoff, pnp_overlapped_reset);
    else launch_step(k_step, env_grid(h), st, h, io, h->done_list, slot(h, CNT_DONE), nullptr, nullptr);
    return XARM_OK;
}

static int reach_step(xarm_handle *h, const StepIO &io, hipStream_t st) {
    if (small_batch(h)) launch_step(k_reach_step_coop, coop_grid(h->kp.num_envs), st, h, io, h->done_list, slot(h, CNT_DONE));
    else launch_step(k_reach_step, env_grid(h), st, h, io, h->done_list, slot(h, CNT_DONE));
    return XARM_OK;
}

// Handover with one stick.  Its reset is not overlapped: six single-substep ticks, 0.28 ms whether it runs beside the hand-off
// or after it, and the two launches slow each other down when they overlap - 1.78 against 1.76 ms per call
static void ho_fast(xarm_handle *h, const StepIO &io, int *elist, int *ecnt, HoStage sg, hipStream_t st) {
    launch_step(HO_KERNEL(h, k_ho_step_fast), env_grid(h), st, h, io, h->done_list, slot(h, CNT_DONE), elist, ecnt, sg);
}
static void ho_handoff(xarm_handle *h, const StepIO &io, int, int *elist, int *ecnt, HoStage rest, hipStream_t hs) {
    const int64_t cap = capped(h, h->kp.eject_coop_cap);
    launch_step(HO_COOP_KERNEL(h, k_ho_step_coop_list), ho_coop_grid(cap), hs, h, io, h->done_list, slot(h, CNT_DONE), elist, ecnt, rest);
    if (h->kp.num_envs > cap) launch_step(HO_KERNEL(h, k_ho_step), env_grid(h), hs, h, io, h->done_list, slot(h, CNT_DONE), elist, ecnt, rest);
}
static int ho_step(xarm_handle *h, const StepIO &io, hipStream_t st) {
    const HoStage whole{0, xm::HO_N_TICKS, nullptr, nullptr};   // an unstaged step
    // small batch: every env on the cooperative rows, one launch (list == null: all envs; finished episodes -> done_list)
    if (small_batch(h)) launch_step(HO_COOP_KERNEL(h, k_ho_step_coop_list), ho_coop_grid(h->kp.num_envs), st, h, io, h->done_list, slot(h, CNT_DONE),
                                    nullptr, nullptr, whole);
    else if (h->fast_pipeline) return pipelined_step(h, io, st, ho_fast, ho_handoff, nullptr);
    else launch_step(HO_KERNEL(h, k_ho_step), env_grid(h), st, h, io, h->done_list, slot(h, CNT_DONE), nullptr, nullptr, whole);
    return XARM_OK;
}
static int ho2_step(xarm_handle *h, const StepIO &io, hipStream_t st) {
    launch_step(HO_KERNEL(h, k_ho2_step), env_grid(h), st, h, io, h->done_list, slot(h, CNT_DONE));
    return XARM_OK;
}

// StackTower, Rearrange: with the class order, a histogram of the envs' class keys and their placement into class-homogeneous
// wavefronts (class_order) come before the step
template <auto HIST, auto PLACE, auto STEP>
static int class_ordered_step(xarm_handle *h, const StepIO &io, hipStream_t st) {
    if (h->class_key) {
        const unsigned cg = (unsigned)((h->kp.num_envs + 255) / 256);
        int *hist = slot(h, CNT_REGION);
        HIST<<<dim3(cg), dim3(256), 0, st>>>(h->class_key, h->kp.num_envs, hist);
        PLACE<<<dim3(cg), dim3(256), 0, st>>>(h->class_key, h->kp.num_envs, hist, hist + h->ops->ncls, h->class_order, WG / 2);
    }
    launch_step(STEP, env_grid(h), st, h, io, h->done_list, slot(h, CNT_DONE), h->class_order, h->class_key);
    return XARM_OK;
}

static const char NO_RELABEL_CONTACT[] = "xarm_compute_reward: reward_type 'dense' depends on the contact state and cannot be relabelled";
static const char NO_RELABEL_DIFF[] = "xarm_compute_reward: reward_type 'dense_diff' is stateful (d_old) and cannot be relabelled";
static const char NO_RELABEL_GRASP[] = "xarm_compute_reward: reward_type 'dense' depends on the grasp flags and gripper positions and cannot be relabelled";

//  dims: obs, goal, act, state, max_episode_steps, n_substeps | steps field, lanes | reset, step limit defaults | stages | ticks | classes
//  init, reset, step, reward | reward type that cannot be relabelled
static const KindOps KIND_PNP = {
    {xk::OBS_DIM, xk::GOAL_DIM, xk::ACT_DIM, xk::STATE_DIM, xm::PNP_MAX_EPISODE_STEPS, xm::PNP_N_SUBSTEPS}, xk::S_STEPS, 1,
    XARM_RESET_COOP_LIMIT_DEFAULT, XARM_STEP_COOP_LIMIT_DEFAULT, XARM_PNP_STAGES_DEFAULT, "XARM_PNP_STAGES", xm::PNP_N_SUBSTEPS, 0, nullptr,
    init_with<k_init>, pnp_reset, pnp_step, typed_reward<k_compute_reward>, XARM_REWARD_DENSE, NO_RELABEL_CONTACT};
static const KindOps KIND_REACH = {
    {xr::OBS_DIM, xk::GOAL_DIM, xk::ACT_DIM, xr::STATE_DIM, xmr::MAX_EPISODE_STEPS, xmr::N_SUBSTEPS}, xr::R_STEPS, 1,
    XARM_RESET_COOP_LIMIT_DEFAULT, XARM_STEP_COOP_LIMIT_DEFAULT, 0, nullptr, 0, 0, nullptr,
    init_with<k_reach_init>, reach_reset, reach_step, typed_reward<k_reach_compute_reward>, XARM_REACH_REWARD_DENSE_DIFF, NO_RELABEL_DIFF};
static const KindOps KIND_HANDOVER1 = {
    {xh::OBS_DIM, xk::GOAL_DIM, xh::ACT_DIM, xh::STATE_DIM, xm::HO_MAX_EPISODE_STEPS, xm::HO_N_TICKS}, xh::H_STEPS, 2,
    XARM_HO_RESET_COOP_LIMIT_DEFAULT, XARM_HO_STEP_COOP_LIMIT_DEFAULT, XARM_HO_STAGES_DEFAULT, "XARM_HO_STAGES", xm::HO_N_TICKS, 0, nullptr,
    init_with<k_ho_init>, ho_reset, ho_step, sparse_reward<k_ho_compute_reward>, XARM_REWARD_DENSE, NO_RELABEL_GRASP};
static const KindOps KIND_HANDOVER2 = {
    {xh2::OBS_DIM, xh2::GOAL_DIM, xh::ACT_DIM, xh2::STATE_DIM, xm::HO_MAX_EPISODE_STEPS, xm::HO_N_TICKS}, xh2::G_STEPS, 2,
    0, 0, 0, nullptr, xm::HO_N_TICKS, 0, nullptr,
    init_with<k_ho2_init>, ho2_reset, ho2_step, sparse_reward<k_ho2_compute_reward>, XARM_REWARD_DENSE, NO_RELABEL_GRASP};
static const KindOps KIND_STACK = {
    {xs::OBS_DIM, xs::GOAL_DIM, xs::ACT_DIM, xs::STATE_DIM, xm::ST_MAX_EPISODE_STEPS, xm::ST_N_SUBSTEPS}, xs::K_STEPS, 2,
    0, 0, 0, nullptr, 0, xs::NCLS, "XARM_ST_CLASS_ORDER",
    init_with<k_st_init>, keyed_reset<k_st_reset>, class_ordered_step<k_class_hist, k_class_place, k_st_step>, typed_reward<k_st_compute_reward>, -1, nullptr};
static const KindOps KIND_REARRANGE = {
    {xra::OBS_DIM, xra::GOAL_DIM, xra::ACT_DIM, xra::STATE_DIM, xm::RA_MAX_EPISODE_STEPS, xm::ST_N_SUBSTEPS}, xra::K_STEPS, 2,
    0, 0, 0, nullptr, 0, xra::NCLS, "XARM_RA_CLASS_ORDER",
    init_with<k_ra_init>, keyed_reset<k_ra_reset>, class_ordered_step<k_ra_class_hist, k_ra_class_place, k_ra_step>, typed_reward<k_ra_compute_reward>, -1, nullptr};

// how many ints of the counter block a step call of this handle clears
static int step_counter_ints(const xarm_handle *h) {
    if (h->class_key) return CNT_REGION + 2 * h->ops->ncls;
    if (!h->fast_pipeline) return CNT_DONE + 1;
    if (h->ho_stages <= 1) return CNT_REGION;
    return h->reset_per_stage ? CNT_STAGE_INTS : cnt_stage(xarm_handle::MAX_ST) + 1;   // with or without the per-stage list-B counts
}

// integer value of an environment variable that is set and not empty
static bool env_int(const char *name, int *value) {
    const char *ev = getenv(name);
    if (!ev || !*ev) return false;
    *value = atoi(ev);
    return true;
}
// a cooperative-kernel limit: an explicit xarm_config value wins (< 0 = never = 0); the environment variable replaces the
// DEFAULT only, and a non-positive value of it means 0
static int resolve_limit(int cfg_value, int dflt, const char *env_name) {
    int v;
    if (cfg_value != 0) return cfg_value > 0 ? cfg_value : 0;
    return env_int(env_name, &v) ? (v > 0 ? v : 0) : dflt;
}
static int clamp_stages(int n) { return n < 1 ? 1 : (n > xarm_handle::MAX_ST ? xarm_handle::MAX_ST : n); }

// The handle's kernels, events and buffers live on cfg.device.  Every entry point makes that device current for its
// own duration and restores the caller's (torch's) current device on return, so a handle can be created and used
// while another device is current, and several handles on different GPUs can share a process.
struct DeviceGuard {
    int prev;
    bool switched;
    explicit DeviceGuard(int dev) : prev(-1), switched(false) {
        if (hipGetDevice(&prev) == hipSuccess && prev != dev) switched = hipSetDevice(dev) == hipSuccess;
    }
    ~DeviceGuard() { if (switched) hipSetDevice(prev); }
};
#define DEVGUARD(h) DeviceGuard _guard((h)->cfg.device)

static void timing_flush(xarm_handle *h) {
    for (int i = 0; i < h->ev_n; i++) {
        float ms = 0.f;
        if (hipEventSynchronize(h->ev2[i]) == hipSuccess && hipEventElapsedTime(&ms, h->ev0[i], h->ev1[i]) == hipSuccess) {
            h->ev_ms += ms;
            h->ev_launches++;
            if (hipEventElapsedTime(&ms, h->ev1[i], h->ev2[i]) == hipSuccess) h->ev_reset_ms += ms;
        }
    }
    h->ev_n = 0;
}

extern "C" {

// a timing variant built with -DXC_SWEEP_ITERS=n (tools/coop_split.sh) runs fewer solver sweeps: it must never pass for the product
#define XARM_STR2(x) #x
#define XARM_STR(x) XARM_STR2(x)
#ifdef XARM_SWEEP_VARIANT
const char *xarm_version(void) { return "xarm_hip 0.1 (gfx950) TIMING VARIANT sweeps=" XARM_STR(XARM_SWEEP_VARIANT); }
#else
const char *xarm_version(void) { return "xarm_hip 0.1 (gfx950)"; }
#endif

const char *xarm_last_error(const xarm_handle *h) { return h ? h->err : g_err; }

int xarm_create(const xarm_config *cfg, xarm_handle **out) {
    if (!cfg || !out) return fail(nullptr, XARM_E_INVALID, "%s", "xarm_create: null argument");
    const KindOps *ops;
    switch (cfg->env_kind) {
    case XARM_ENV_PICK_AND_PLACE: ops = &KIND_PNP; break;
    case XARM_ENV_REACH: ops = &KIND_REACH; break;
    case XARM_ENV_HANDOVER: ops = cfg->num_obj == 2 ? &KIND_HANDOVER2 : &KIND_HANDOVER1; break;
    case XARM_ENV_STACK_TOWER: ops = &KIND_STACK; break;
    case XARM_ENV_REARRANGE: ops = &KIND_REARRANGE; break;
    default: return fail(nullptr, XARM_E_INVALID, "%s", "xarm_create: unsupported env_kind");
    }
    const bool reach = cfg->env_kind == XARM_ENV_REACH, handover = cfg->env_kind == XARM_ENV_HANDOVER, stack = cfg->env_kind == XARM_ENV_STACK_TOWER;
    const bool rearrange = cfg->env_kind == XARM_ENV_REARRANGE;
    if (stack && cfg->num_obj != 3) return fail(nullptr, XARM_E_INVALID, "%s", "xarm_create: XarmStackTower has num_obj == 3 (xarm_stack_tower.py:19)");
    if (stack && cfg->reward_type > 1) return fail(nullptr, XARM_E_INVALID, "%s", "xarm_create: XarmStackTower reward_type is 0 (sparse) or 1 (-d)");
    if (rearrange && cfg->num_obj != 4) return fail(nullptr, XARM_E_INVALID, "%s", "xarm_create: XarmRearrange has num_obj == 4 (xarm_rearrange.py:20)");
    if (rearrange && cfg->reward_type > 1) return fail(nullptr, XARM_E_INVALID, "%s", "xarm_create: XarmRearrange reward_type is 0 (sparse) or 1 (-d)");
    if (handover && cfg->num_obj != 1 && cfg->num_obj != 2) return fail(nullptr, XARM_E_INVALID, "%s", "xarm_create: XarmHandover supports num_obj 1 or 2");
    if (handover && cfg->num_obj == 2 && cfg->reward_type != 0)
        return fail(nullptr, XARM_E_INVALID, "%s", "xarm_create: XarmHandover with num_obj == 2 takes the sparse reward (the reference's dense branch raises a broadcast error there, xarm_handover.py:187-188)");
    if (!reach && !stack && !rearrange && !handover && cfg->num_obj != 1)
        return fail(nullptr, XARM_E_INVALID, "%s", "xarm_create: XarmPickAndPlace supports num_obj == 1 (with more the reference's own step raises, xarm_pick_and_place.py:289-291)");
    if (handover && cfg->reward_type != 0 && cfg->reward_type != XARM_REWARD_DENSE)
        return fail(nullptr, XARM_E_INVALID, "%s", "xarm_create: XarmHandover reward_type is sparse (hard-wired in the reference, xarm_handover.py:40) or dense (:184-199)");
    if (cfg->use_stand && !handover) return fail(nullptr, XARM_E_INVALID, "%s", "xarm_create: use_stand belongs to XarmHandover (xarm_handover.py:391-392)");
    if (cfg->auto_reset < 0 || cfg->auto_reset > XARM_AUTO_RESET_LAZY) return fail(nullptr, XARM_E_INVALID, "%s", "xarm_create: auto_reset must be 0, 1 or XARM_AUTO_RESET_LAZY");
    if (cfg->auto_reset == XARM_AUTO_RESET_LAZY && cfg->env_kind != XARM_ENV_PICK_AND_PLACE)
        return fail(nullptr, XARM_E_INVALID, "%s", "xarm_create: lazy auto-reset is implemented for XarmPickAndPlace only");
    if (cfg->num_envs <= 0 || cfg->num_envs > (int64_t)1 << 30) return fail(nullptr, XARM_E_INVALID, "%s", "xarm_create: num_envs out of range");
    if (cfg->reward_type < 0 || cfg->reward_type > 2) return fail(nullptr, XARM_E_INVALID, "%s", "xarm_create: unsupported reward_type");
    if (!reach && !stack && !rearrange && cfg->goal_shape != XARM_GOAL_AIR && cfg->goal_shape != XARM_GOAL_GROUND)
        return fail(nullptr, XARM_E_INVALID, "%s", "xarm_create: unsupported goal_shape");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(nullptr, XARM_E_NODEVICE, "%s", "xarm_create: no HIP device");
    if (cfg->device < 0 || cfg->device >= ndev) return fail(nullptr, XARM_E_INVALID, "%s", "xarm_create: bad device ordinal");
    DeviceGuard _guard(cfg->device);
    xarm_handle *h = new (std::nothrow) xarm_handle();
    if (!h) return fail(nullptr, XARM_E_INVALID, "%s", "xarm_create: out of host memory");
    memset(h, 0, sizeof *h);
    h->cfg = *cfg;
    h->ops = ops;
    const int64_t E = cfg->num_envs, stride = (E + WG - 1) / WG * WG;
    h->kp.stride = stride;
    h->kp.num_envs = E;
    h->kp.cfg.seed = cfg->seed;
    h->kp.cfg.env_id_offset = cfg->env_id_offset;
    h->kp.cfg.init_grasp_rate = cfg->init_grasp_rate;
    h->kp.cfg.goal_ground_rate = cfg->goal_ground_rate;
    h->kp.cfg.goal_shape = cfg->goal_shape;
    h->kp.cfg.reward_type = cfg->reward_type;
    h->kp.auto_reset = cfg->auto_reset;
    int v;
    // cooperative reset kernel: default cross-over measured on MI355X (Handover with one stick, two rows per env,
    // against the lane-pair reset: DESIGN.md 10b); 0 disables it
    h->kp.coop_limit = ops->reset_coop_default ? resolve_limit(cfg->reset_coop_limit, ops->reset_coop_default, "XARM_RESET_COOP_LIMIT") : 0;
    // cooperative step kernel: pays while the one-env-per-lane launch would leave SIMDs empty (measured cross-over).
    // Handover (one stick): small batches step on the cooperative rows altogether - 2 048 envs are one round of 1 024 wavefronts
    // and one kernel of ~0.6 ms, where the fast lane-pair kernel (0.72 ms whatever the batch, a latency) plus the hand-off take 1.4
    h->coop_step_limit = ops->step_coop_default ? resolve_limit(cfg->step_coop_limit, ops->step_coop_default, "XARM_STEP_COOP_LIMIT") : 0;
    // fast-step pipeline (PickAndPlace batches above the cooperative limit, Handover with one stick): on unless the caller
    // pinned the one-env-per-lane family (step_coop_limit < 0: gym_xarm_amd.distributed.reproducible_limits('lane')) or
    // XARM_STEP_PIPELINE=0 asks for the plain k_step / k_ho_step
    h->fast_pipeline = (ops->stages_env && cfg->step_coop_limit >= 0 && cfg->auto_reset != XARM_AUTO_RESET_LAZY) ? 1 : 0;
    if (env_int("XARM_STEP_PIPELINE", &v)) h->fast_pipeline = h->fast_pipeline && v != 0;
    h->ho_force_coupled = env_int("XARM_HO_FORCE_COUPLED", &v) && v != 0;
    // staged step: XARM_HO_STAGES=1 / XARM_PNP_STAGES=1 is the unstaged pipeline (one fast launch, one hand-off)
    h->ho_stages = 1;
    if (h->fast_pipeline) h->ho_stages = clamp_stages(env_int(ops->stages_env, &v) ? v : ops->stages_default);
    for (int c = 0; c <= h->ho_stages; c++) h->ho_tick[c] = c * xm::HO_N_TICKS / h->ho_stages;
    // measurement hook: XARM_HO_STAGE_TICKS="3,9" = the interior stage boundaries (increasing, inside 1 .. 14)
    const char *ev = getenv("XARM_HO_STAGE_TICKS");
    if (ev && *ev && h->ho_stages > 1) {
        int c = 1, prev = 0;
        const char *q = ev;
        while (*q && c < h->ho_stages) {
            const int t = atoi(q);
            if (t <= prev || t >= xm::HO_N_TICKS) break;
            h->ho_tick[c++] = prev = t;
            while (*q && *q != ',') q++;
            if (*q == ',') q++;
        }
        if (c != h->ho_stages) for (int k = 0; k <= h->ho_stages; k++) h->ho_tick[k] = k * xm::HO_N_TICKS / h->ho_stages;   // malformed: the default
    }
    const bool handover1 = ops == &KIND_HANDOVER1;
    h->kp.eject_coop_cap = handover1 ? XARM_HO_EJECT_COOP_CAP : XARM_EJECT_COOP_CAP;
    // step_coop_limit == 1 is the pin of reproducible_limits('fast'): every hand-off list steps on the cooperative kernel (it
    // walks the list with a grid stride), so that which kernel steps an env is a function of the handle's config alone
    if (cfg->step_coop_limit == 1) h->kp.eject_coop_cap = 0x7fffffff;
    h->kp.state_dim = ops->dims.state_dim;
    h->kp.hcfg.seed = cfg->seed;
    h->kp.hcfg.env_id_offset = cfg->env_id_offset;
    h->kp.hcfg.same_side_rate = cfg->same_side_rate;
    h->kp.hcfg.goal_shape = cfg->goal_shape;
    h->kp.hcfg.use_stand = handover && cfg->use_stand ? 1 : 0;
    h->kp.hcfg.reward_type = cfg->reward_type == XARM_REWARD_DENSE ? 1 : 0;
    h->kp.rcfg.seed = cfg->seed;
    h->kp.rcfg.env_id_offset = cfg->env_id_offset;
    h->kp.rcfg.reward_type = cfg->reward_type;
    hipError_t e1 = hipMalloc(&h->kp.state, sizeof(float) * h->kp.state_dim * stride);
    hipError_t e2 = hipMalloc(&h->done_list, sizeof(int) * stride);
    hipError_t e3 = hipMalloc(&h->counters, sizeof(int) * CNT_INTS);
    hipError_t e4 = hipMalloc(&h->mask_count, sizeof(int));
    if (e4 == hipSuccess && h->fast_pipeline) {
        e4 = hipMalloc(&h->eject_list, sizeof(int) * stride * h->ho_stages);   // one list per stage
        // the reset overlap is PickAndPlace's (Handover: see ho_fast)
        if (e4 == hipSuccess && cfg->auto_reset && !handover1 && !(env_int("XARM_RESET_OVERLAP", &v) && v == 0)) {
            e4 = hipStreamCreateWithFlags(&h->side, hipStreamNonBlocking);
            if (e4 == hipSuccess) e4 = hipEventCreateWithFlags(&h->ev_fork, hipEventDisableTiming);
            if (e4 == hipSuccess) e4 = hipEventCreateWithFlags(&h->ev_join, hipEventDisableTiming);
            h->reset_overlap = e4 == hipSuccess;
        }
        // one list B per hand-off stage, reset behind that stage's hand-off (pnp_handoff); XARM_RESET_PER_STAGE=0: one list B, one reset
        // after the last hand-off
        h->reset_per_stage = h->reset_overlap && h->ho_stages > 1 && (env_int("XARM_RESET_PER_STAGE", &v) ? v != 0 : XARM_RESET_PER_STAGE_DEFAULT);
        if (e4 == hipSuccess) e4 = hipMalloc(&h->done_list_b, sizeof(int) * stride * (h->reset_per_stage ? h->ho_stages : 1));
    }
    if (e4 == hipSuccess && h->fast_pipeline) {
        // the joint targets travel between stages only; the flags belong to every pipelined handle: k_step_fast_stage marks an env it
        // hands off whatever the stage count
        if (h->ho_stages > 1) e4 = hipMalloc(&h->ho_qt, sizeof(float) * 18 * stride);
        if (e4 == hipSuccess) e4 = hipMalloc(&h->ho_flag, stride);
        if (e4 == hipSuccess) e4 = hipMemset(h->ho_flag, 0, stride);
        for (int c = 0; c + 1 < h->ho_stages && e4 == hipSuccess; c++) {
            int lo = 0, hi = 0;
            hipDeviceGetStreamPriorityRange(&lo, &hi);      // lo = the LEAST urgent (numerically greatest)
            if (env_int("XARM_HO_SIDE_PRIO", &v) && v != 0) e4 = hipStreamCreateWithPriority(&h->st_side[c], hipStreamNonBlocking, lo);
            else e4 = hipStreamCreateWithFlags(&h->st_side[c], hipStreamNonBlocking);
            if (e4 == hipSuccess) e4 = hipEventCreateWithFlags(&h->st_fork[c], hipEventDisableTiming);
            if (e4 == hipSuccess) e4 = hipEventCreateWithFlags(&h->st_join[c], hipEventDisableTiming);
        }
    }
    if (e4 == hipSuccess && ops->class_env && !(env_int(ops->class_env, &v) && v == 0)) {
        e4 = hipMalloc(&h->class_key, stride);
        if (e4 == hipSuccess) e4 = hipMalloc(&h->class_order, sizeof(int) * stride);
        if (e4 == hipSuccess) e4 = hipMemset(h->class_key, 0, stride);
    }
    if (e1 != hipSuccess || e2 != hipSuccess || e3 != hipSuccess || e4 != hipSuccess) {
        fail(nullptr, XARM_E_HIP, "xarm_create: hipMalloc failed: %s", hipGetErrorString(e1 != hipSuccess ? e1 : (e2 != hipSuccess ? e2 : (e3 != hipSuccess ? e3 : e4))));
        xarm_destroy(h);
        return XARM_E_HIP;
    }
    hipMemset(h->kp.state, 0, sizeof(float) * h->kp.state_dim * stride);
    hipMemset(h->counters, 0, sizeof(int) * CNT_INTS);
    hipMemset(h->mask_count, 0, sizeof(int));
    ops->init(h);
    hipError_t e5 = hipDeviceSynchronize();
    if (e5 != hipSuccess) {
        fail(nullptr, XARM_E_HIP, "xarm_create: k_init: %s", hipGetErrorString(e5));
        xarm_destroy(h);
        return XARM_E_HIP;
    }
    *out = h;
    return XARM_OK;
}

int xarm_destroy(xarm_handle *h) {
    if (!h) return XARM_OK;
    DEVGUARD(h);
    hipDeviceSynchronize();
    if (h->ev_created)
        for (int i = 0; i < xarm_handle::NEV; i++) { hipEventDestroy(h->ev0[i]); hipEventDestroy(h->ev1[i]); hipEventDestroy(h->ev2[i]); }
    if (h->kp.state) hipFree(h->kp.state);
    if (h->done_list) hipFree(h->done_list);
    if (h->counters) hipFree(h->counters);
    if (h->mask_count) hipFree(h->mask_count);
    if (h->eject_list) hipFree(h->eject_list);
    if (h->done_list_b) hipFree(h->done_list_b);
    if (h->ev_fork) hipEventDestroy(h->ev_fork);
    if (h->ev_join) hipEventDestroy(h->ev_join);
    if (h->side) hipStreamDestroy(h->side);
    if (h->class_key) hipFree(h->class_key);
    if (h->class_order) hipFree(h->class_order);
    if (h->ho_qt) hipFree(h->ho_qt);
    if (h->ho_flag) hipFree(h->ho_flag);
    for (int c = 0; c < xarm_handle::MAX_ST; c++) {
        if (h->st_fork[c]) hipEventDestroy(h->st_fork[c]);
        if (h->st_join[c]) hipEventDestroy(h->st_join[c]);
        if (h->st_side[c]) hipStreamDestroy(h->st_side[c]);
    }
    delete h;
    return XARM_OK;
}

int xarm_dims(const xarm_handle *h, xarm_dims_t *out) {
    if (!out) return XARM_E_INVALID;
    *out = (h ? h->ops : &KIND_PNP)->dims;
    return XARM_OK;
}

int xarm_reset(xarm_handle *h, const uint8_t *mask_dev, float *obs_dev, float *ag_dev, float *dg_dev, void *stream) {
    if (!h) return XARM_E_INVALID;
    DEVGUARD(h);
    if (obs_dev && (!ag_dev || !dg_dev)) return fail(h, XARM_E_INVALID, "%s", "xarm_reset: goal buffers required with obs");
    hipStream_t st = (hipStream_t)stream;
    if (mask_dev) {
        HIPCHK(h, hipMemsetAsync(h->mask_count, 0, sizeof(int), st));
        k_compact_mask<<<dim3((unsigned)((h->kp.num_envs + 255) / 256)), dim3(256), 0, st>>>(mask_dev, h->kp.num_envs, h->done_list, h->mask_count);
    }
    h->ops->reset(h, mask_dev ? h->done_list : nullptr, mask_dev ? h->mask_count : nullptr, obs_dev, ag_dev, dg_dev, st);
    HIPCHK(h, hipGetLastError());
    return XARM_OK;
}

int xarm_step(xarm_handle *h, const float *actions_dev, float *obs_dev, float *ag_dev, float *dg_dev, float *reward_dev,
              uint8_t *done_dev, uint8_t *success_dev, float *terminal_obs_dev, void *stream) {
    if (!h) return XARM_E_INVALID;
    DEVGUARD(h);
    if (!actions_dev || !obs_dev || !ag_dev || !dg_dev || !reward_dev || !done_dev || !success_dev)
        return fail(h, XARM_E_INVALID, "%s", "xarm_step: null buffer");
    hipStream_t st = (hipStream_t)stream;
    const StepIO io{actions_dev, obs_dev, ag_dev, dg_dev, reward_dev, done_dev, success_dev, terminal_obs_dev};
    const bool timed = h->timing && h->ev_created;
    if (timed && h->ev_n == xarm_handle::NEV) timing_flush(h);
    if (timed) HIPCHK(h, hipEventRecord(h->ev0[h->ev_n], st));
    if (h->kp.auto_reset == XARM_AUTO_RESET_LAZY) {     // PickAndPlace only (xarm_create); no terminal_obs, no counters
        k_step_lazy<<<dim3(env_grid(h)), dim3(WG), 0, st>>>(h->kp, io.actions, io.obs, io.ag, io.dg, io.reward, io.done, io.success);
        if (timed) { HIPCHK(h, hipEventRecord(h->ev1[h->ev_n], st)); HIPCHK(h, hipEventRecord(h->ev2[h->ev_n], st)); h->ev_n++; }
        HIPCHK(h, hipGetLastError());
        return XARM_OK;
    }
    // the call's device-side counters (ended episodes, hand-offs, class histogram): zeroed here, in stream order - the
    // handle keeps no host-side per-step state, so a captured step call replays correctly
    HIPCHK(h, hipMemsetAsync(h->counters, 0, sizeof(int) * step_counter_ints(h), st));
    const int rc = h->ops->step(h, io, st);
    if (rc != XARM_OK) return rc;
    if (timed) HIPCHK(h, hipEventRecord(h->ev1[h->ev_n], st));
    if (h->reset_overlap && !small_batch(h)) {     // the PickAndPlace pipeline reset list A on `side` (pnp_overlapped_reset)
        // list B (reset_per_stage: the last stage's; the earlier stages reset theirs on their side streams, joined here, BEHIND the
        // launch - the last reset waits for its own hand-off only, and the call still ends with every side stream joined)
        pnp_reset_b(h, io, h->ho_stages - 1, st);
        if (h->reset_per_stage) { const int jr = join_stages(h, st); if (jr != XARM_OK) return jr; }
        HIPCHK(h, hipStreamWaitEvent(st, h->ev_join, 0));
    } else if (h->kp.auto_reset)
        h->ops->reset(h, h->done_list, slot(h, CNT_DONE), obs_dev, ag_dev, dg_dev, st);
    if (timed) { HIPCHK(h, hipEventRecord(h->ev2[h->ev_n], st)); h->ev_n++; }
    HIPCHK(h, hipGetLastError());
    return XARM_OK;
}

int xarm_compute_reward(xarm_handle *h, const float *ag_dev, const float *g_dev, int64_t n, float *out_dev, void *stream) {
    if (!h) return XARM_E_INVALID;
    DEVGUARD(h);
    if (n < 0 || (n > 0 && (!ag_dev || !g_dev || !out_dev))) return fail(h, XARM_E_INVALID, "%s", "xarm_compute_reward: bad argument");
    if (h->ops->fixed_reward_msg && h->cfg.reward_type == h->ops->fixed_reward_type) return fail(h, XARM_E_INVALID, "%s", h->ops->fixed_reward_msg);
    if (n == 0) return XARM_OK;
    h->ops->reward(h, ag_dev, g_dev, n, out_dev, (hipStream_t)stream);
    HIPCHK(h, hipGetLastError());
    return XARM_OK;
}

int xarm_get_state(xarm_handle *h, float *state_dev, void *stream) {
    if (!h || !state_dev) return XARM_E_INVALID;
    DEVGUARD(h);
    const int64_t n = h->kp.num_envs * h->kp.state_dim;
    k_get_state<<<dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream>>>(h->kp, state_dev);
    HIPCHK(h, hipGetLastError());
    return XARM_OK;
}
int xarm_set_state(xarm_handle *h, const float *state_dev, void *stream) {
    if (!h || !state_dev) return XARM_E_INVALID;
    DEVGUARD(h);
    const int64_t n = h->kp.num_envs * h->kp.state_dim;
    k_set_state<<<dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream>>>(h->kp, state_dev);
    HIPCHK(h, hipGetLastError());
    return XARM_OK;
}

int xarm_episode_steps(xarm_handle *h, int32_t *steps_dev, void *stream) {
    if (!h || !steps_dev) return XARM_E_INVALID;
    DEVGUARD(h);
    k_episode_steps<<<dim3((unsigned)((h->kp.num_envs + 255) / 256)), dim3(256), 0, (hipStream_t)stream>>>(h->kp, h->ops->steps_field, steps_dev);
    HIPCHK(h, hipGetLastError());
    return XARM_OK;
}

int xarm_debug_substeps(xarm_handle *h, const float *qtarget_dev, int32_t n, void *stream) {
    if (!h || !qtarget_dev || n < 0) return XARM_E_INVALID;
    DEVGUARD(h);
    if (h->ops != &KIND_PNP) return fail(h, XARM_E_INVALID, "%s", "xarm_debug_substeps: PickAndPlace only");
    k_substeps<<<dim3(env_grid(h)), dim3(WG), 0, (hipStream_t)stream>>>(h->kp, qtarget_dev, n);
    HIPCHK(h, hipGetLastError());
    return XARM_OK;
}

int xarm_timing_enable(xarm_handle *h, int32_t enable) {
    if (!h) return XARM_E_INVALID;
    DEVGUARD(h);
    if (enable && !h->ev_created) {
        for (int i = 0; i < xarm_handle::NEV; i++) {
            HIPCHK(h, hipEventCreate(&h->ev0[i]));
            HIPCHK(h, hipEventCreate(&h->ev1[i]));
            HIPCHK(h, hipEventCreate(&h->ev2[i]));
        }
        h->ev_created = true;
    }
    if (enable) { h->ev_n = 0; h->ev_ms = 0; h->ev_reset_ms = 0; h->ev_launches = 0; }
    h->timing = enable;
    return XARM_OK;
}
int xarm_timing_read(xarm_handle *h, double *ms_total, int64_t *launches) {
    if (!h || !ms_total || !launches) return XARM_E_INVALID;
    DEVGUARD(h);
    timing_flush(h);
    *ms_total = h->ev_ms;
    *launches = h->ev_launches;
    return XARM_OK;
}
int xarm_timing_read_reset(xarm_handle *h, double *reset_ms_total, int64_t *launches) {
    if (!h || !reset_ms_total || !launches) return XARM_E_INVALID;
    DEVGUARD(h);
    timing_flush(h);
    *reset_ms_total = h->ev_reset_ms;
    *launches = h->ev_launches;
    return XARM_OK;
}
int xarm_class_keys(xarm_handle *h, uint8_t *keys_dev, void *stream) {
    if (!h || !keys_dev) return XARM_E_INVALID;
    DEVGUARD(h);
    if (!h->class_key) return fail(h, XARM_E_INVALID, "%s", "xarm_class_keys: StackTower / Rearrange handles with the class order enabled only");
    HIPCHK(h, hipMemcpyAsync(keys_dev, h->class_key, (size_t)h->kp.num_envs, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return XARM_OK;
}
int xarm_kernel_limits(const xarm_handle *h, int32_t *reset_coop_limit, int32_t *step_coop_limit) {
    if (!h || !reset_coop_limit || !step_coop_limit) return XARM_E_INVALID;
    *reset_coop_limit = h->kp.coop_limit;
    *step_coop_limit = h->coop_step_limit;
    return XARM_OK;
}
int xarm_debug_counts(xarm_handle *h, int32_t *finished, int32_t *handed_off, void *stream) {
    if (!h || !finished || !handed_off) return XARM_E_INVALID;
    DEVGUARD(h);
    int c[CNT_STAGE_INTS] = {0};
    HIPCHK(h, hipStreamSynchronize((hipStream_t)stream));
    HIPCHK(h, hipMemcpy(c, h->counters, sizeof c, hipMemcpyDeviceToHost));
    *finished = c[CNT_DONE];
    *handed_off = 0;
    if (h->fast_pipeline) for (int k = 0; k < h->ho_stages; k++) *handed_off += c[cnt_stage(k)];   // staged step: one list per stage
    return XARM_OK;
}
int xarm_debug_stage_counts(xarm_handle *h, int32_t *handed_off, int32_t *finished_in_handoff, void *stream) {
    if (!h || !handed_off || !finished_in_handoff) return XARM_E_INVALID;
    DEVGUARD(h);
    int c[CNT_STAGE_INTS] = {0};
    HIPCHK(h, hipStreamSynchronize((hipStream_t)stream));
    HIPCHK(h, hipMemcpy(c, h->counters, sizeof c, hipMemcpyDeviceToHost));
    for (int k = 0; k < XARM_HO_MAX_STAGES; k++) {
        const bool live = h->fast_pipeline && k < h->ho_stages;
        handed_off[k] = live ? c[cnt_stage(k)] : 0;
        finished_in_handoff[k] = (live && h->reset_overlap && (k == 0 || h->reset_per_stage)) ? c[cnt_done_b(k)] : 0;
    }
    return XARM_OK;
}
int xarm_stage_info(const xarm_handle *h, int32_t *stages, int32_t *ticks) {
    if (!h || !stages || !ticks) return XARM_E_INVALID;
    const bool staged = h->fast_pipeline && h->ho_stages > 1 && !small_batch(h);
    *stages = staged ? h->ho_stages : 1;
    for (int c = 0; c <= XARM_HO_MAX_STAGES; c++) ticks[c] = 0;
    if (staged) for (int c = 0; c <= h->ho_stages; c++) ticks[c] = h->ho_tick[c];
    else ticks[1] = h->ops->unstaged_ticks;   // (15 ticks / 15 substeps)
    return XARM_OK;
}
int xarm_pipeline_info(const xarm_handle *h, int32_t *fast_pipeline, int32_t *reset_overlap, int32_t *eject_coop_cap,
                       int32_t *solver_iterations) {
    if (!h || !fast_pipeline || !reset_overlap || !eject_coop_cap || !solver_iterations) return XARM_E_INVALID;
    // (the step limit is 0 for the env kinds without a cooperative step kernel)
    *fast_pipeline = (h->fast_pipeline && !small_batch(h)) ? 1 : 0;
    *reset_overlap = (*fast_pipeline && h->reset_overlap) ? (h->reset_per_stage ? 2 : 1) : 0;
    *eject_coop_cap = h->kp.eject_coop_cap;
#if defined(XARM_SWEEP_VARIANT)
    *solver_iterations = XARM_SWEEP_VARIANT;
#else
    *solver_iterations = xm::NUM_ITERATIONS;
#endif
    return XARM_OK;
}

// ------------------------------------------------------------------------------------- rendering (xarm_k_render.hip)
int xarm_default_camera(const xarm_handle *h, xarm_camera *out) {
    if (!h || !out) return XARM_E_INVALID;
    return xrc_render::rc_default_camera(h->cfg.env_kind, *out) == 0 ? XARM_OK : XARM_E_INVALID;
}

int xarm_render(xarm_handle *h, const xarm_camera *cam, const int32_t *env_ids_dev, int32_t n, uint32_t *rgba_dev, float *depth_dev,
                uint8_t *seg_dev, void *stream) {
    if (!h) return XARM_E_INVALID;
    if (!cam) return fail(h, XARM_E_INVALID, "%s", "xarm_render: cam is NULL");
    if (!rgba_dev) return fail(h, XARM_E_INVALID, "%s", "xarm_render: rgba_dev is NULL");
    if (n < 1 || (int64_t)n > h->kp.num_envs) return fail(h, XARM_E_INVALID, "%s", "xarm_render: need 1 <= n <= num_envs");
    xrc_render::RScene sc;
    if (xrc_render::rc_scene_of(h->cfg.env_kind, h->cfg.num_obj, h->kp.hcfg.use_stand, sc) != 0)
        return fail(h, XARM_E_INVALID, "%s", "xarm_render: unknown env kind");
    xrc_render::RCam rc;
    if (const char *why = xrc_render::rc_make_camera(*cam, rc)) return fail(h, XARM_E_INVALID, "xarm_render: %s", why);
    DEVGUARD(h);
    const int le = xrc_render::launch_render(h->kp.state, h->kp.stride, h->kp.num_envs, sc, rc, env_ids_dev, n, rgba_dev, depth_dev, seg_dev, stream);
    if (le != 0) return fail(h, XARM_E_HIP, "xarm_render: %s", hipGetErrorString((hipError_t)le));
    return XARM_OK;
}

int xarm_view_from_camera(const xarm_camera *cam, float *view16_host) {
    if (!cam || !view16_host) return XARM_E_INVALID;
    float v[XARM_VIEW_FLOATS];
    if (const char *why = xrc_render::rc_view_from_camera(*cam, v)) return fail(nullptr, XARM_E_INVALID, "xarm_view_from_camera: %s", why);
    for (int k = 0; k < XARM_VIEW_FLOATS; k++) view16_host[k] = v[k];
    return XARM_OK;
}

int xarm_default_view(const xarm_handle *h, int32_t which, float *view16_host) {
    if (!h || !view16_host) return XARM_E_INVALID;
    float v[XARM_VIEW_FLOATS];
    if (xrc_render::rc_default_view(h->cfg.env_kind, which, v) != 0)
        return fail(const_cast<xarm_handle *>(h), XARM_E_INVALID, "%s",
                    "xarm_default_view: which must be 0 (world), 1 (wrist of arm 0) or, on a two-arm kind, 2 (wrist of arm 1)");
    for (int k = 0; k < XARM_VIEW_FLOATS; k++) view16_host[k] = v[k];
    return XARM_OK;
}

int xarm_render_views(xarm_handle *h, const float *views_dev, int32_t num_views, int32_t per_env, int32_t width, int32_t height,
                      int32_t flags, const int32_t *env_ids_dev, int32_t n, uint32_t *rgba_dev, float *depth_dev, uint8_t *seg_dev,
                      void *stream) {
    if (!h) return XARM_E_INVALID;
    if (!views_dev) return fail(h, XARM_E_INVALID, "%s", "xarm_render_views: views_dev is NULL");
    if (!rgba_dev) return fail(h, XARM_E_INVALID, "%s", "xarm_render_views: rgba_dev is NULL");
    if (num_views < 1 || num_views > XARM_RENDER_MAX_VIEWS)
        return fail(h, XARM_E_INVALID, "%s", "xarm_render_views: num_views must lie in [1, XARM_RENDER_MAX_VIEWS]");
    if (per_env != 0 && per_env != 1) return fail(h, XARM_E_INVALID, "%s", "xarm_render_views: per_env must be 0 or 1");
    if (!(width >= 1 && width <= XARM_RENDER_MAX_DIM && height >= 1 && height <= XARM_RENDER_MAX_DIM))
        return fail(h, XARM_E_INVALID, "%s", "xarm_render_views: width and height must lie in [1, XARM_RENDER_MAX_DIM]");
    if (n < 1 || (int64_t)n > h->kp.num_envs) return fail(h, XARM_E_INVALID, "%s", "xarm_render_views: need 1 <= n <= num_envs");
    if (flags & ~XARM_RENDER_SHADOWS) return fail(h, XARM_E_INVALID, "%s", "xarm_render_views: unknown flag bits");
    xrc_render::RScene sc;
    if (xrc_render::rc_scene_of(h->cfg.env_kind, h->cfg.num_obj, h->kp.hcfg.use_stand, sc) != 0)
        return fail(h, XARM_E_INVALID, "%s", "xarm_render_views: unknown env kind");
    DEVGUARD(h);
    const int le = xrc_render::launch_render_views(h->kp.state, h->kp.stride, h->kp.num_envs, sc, views_dev, num_views, per_env, width, height,
                                                   flags, env_ids_dev, n, rgba_dev, depth_dev, seg_dev, stream);
    if (le != 0) return fail(h, XARM_E_HIP, "xarm_render_views: %s", hipGetErrorString((hipError_t)le));
    return XARM_OK;
}

// ------------------------------------------------------------------------------------- HER replay (xarm_k_her.hip)
int xarm_her_record_floats(const xarm_her_layout *layout) {
    if (const char *why = xher::layout_error(layout)) return fail(nullptr, XARM_E_INVALID, "xarm_her_record_floats: %s", why);
    return xher::make_layout(*layout).R;
}

int xarm_her_add(const xarm_her_layout *layout, float *ring, int64_t *ep_end, int64_t *ep_first, int64_t *ep_start, int64_t *clock,
                 const float *obs, const float *next_obs, const float *ag, const float *next_ag, const float *dg, const float *act,
                 const float *rew, const uint8_t *done_u8, void *stream) {
    if (const char *why = xher::layout_error(layout)) return fail(nullptr, XARM_E_INVALID, "xarm_her_add: %s", why);
    if (layout->num_envs == 0) return XARM_OK;
    if (!ring || !ep_end || !ep_first || !ep_start || !clock || !obs || !next_obs || !ag || !next_ag || !dg || !act || !rew || !done_u8)
        return fail(nullptr, XARM_E_INVALID, "%s", "xarm_her_add: NULL pointer");
    xher::AddArgs a;
    a.L = xher::make_layout(*layout);
    a.ring = ring; a.ep_end = ep_end; a.ep_first = ep_first; a.ep_start = ep_start; a.clock = clock;
    a.obs = obs; a.next_obs = next_obs; a.ag = ag; a.next_ag = next_ag; a.dg = dg; a.act = act; a.rew = rew; a.done = done_u8;
    const int le = xher::launch_her_add(a, clock, stream);
    if (le != 0) return fail(nullptr, XARM_E_HIP, "xarm_her_add: %s", hipGetErrorString((hipError_t)le));
    return XARM_OK;
}

int xarm_her_sample(const xarm_her_layout *layout, const float *ring, const int64_t *ep_end, const int64_t *ep_first, int64_t *clock,
                    uint64_t seed, int32_t strategy, int32_t batch, int32_t n_her, float *out_obs, float *out_next_obs, float *out_ag,
                    float *out_next_ag, float *out_goal, float *out_act, float *out_rew, uint8_t *out_done_u8, int64_t *out_env_i64,
                    int64_t *out_time_i64, int64_t *out_goal_time_i64, uint8_t *out_ok_u8, int64_t *fail_count_i64, void *stream) {
    if (const char *why = xher::layout_error(layout)) return fail(nullptr, XARM_E_INVALID, "xarm_her_sample: %s", why);
    if (batch < 0) return fail(nullptr, XARM_E_INVALID, "%s", "xarm_her_sample: batch must be >= 0");
    if (n_her < 0 || n_her > batch) return fail(nullptr, XARM_E_INVALID, "%s", "xarm_her_sample: n_her must lie in [0, batch]");
    if (strategy != XARM_HER_FUTURE && strategy != XARM_HER_FINAL && strategy != XARM_HER_EPISODE)
        return fail(nullptr, XARM_E_INVALID, "%s", "xarm_her_sample: unknown strategy (XARM_HER_FUTURE, XARM_HER_FINAL or XARM_HER_EPISODE)");
    if (batch == 0 || layout->num_envs == 0) return XARM_OK;
    if (!ring || !ep_end || !ep_first || !clock || !out_obs || !out_next_obs || !out_ag || !out_next_ag || !out_goal || !out_act || !out_rew ||
        !out_done_u8 || !out_env_i64 || !out_time_i64 || !out_goal_time_i64 || !out_ok_u8 || !fail_count_i64)
        return fail(nullptr, XARM_E_INVALID, "%s", "xarm_her_sample: NULL pointer");
    xher::SampleArgs a;
    a.L = xher::make_layout(*layout);
    a.ring = ring; a.ep_end = ep_end; a.ep_first = ep_first; a.clock = clock; a.seed = seed;
    a.strategy = strategy; a.batch = batch; a.n_her = n_her;
    a.obs = out_obs; a.next_obs = out_next_obs; a.ag = out_ag; a.next_ag = out_next_ag; a.goal = out_goal; a.act = out_act; a.rew = out_rew;
    a.done = out_done_u8; a.ok = out_ok_u8; a.env = out_env_i64; a.time = out_time_i64; a.goal_time = out_goal_time_i64;
    a.fail_count = fail_count_i64;
    const int le = xher::launch_her_sample(a, clock, stream);
    if (le != 0) return fail(nullptr, XARM_E_HIP, "xarm_her_sample: %s", hipGetErrorString((hipError_t)le));
    return XARM_OK;
}

// ------------------------------------------------------------------------------------- uniform replay (xarm_k_replay.hip)
int xarm_replay_record_floats(const xarm_replay_layout *layout) {
    if (const char *why = xrep::layout_error(layout)) return fail(nullptr, XARM_E_INVALID, "xarm_replay_record_floats: %s", why);
    return xrep::make_layout(*layout).R;
}

int xarm_replay_add(const xarm_replay_layout *layout, float *ring, int64_t *clock, const float *obs, const float *ag, const float *dg,
                    const float *next_obs, const float *next_ag, const float *act, const float *rew, const uint8_t *done_u8,
                    const uint8_t *timeout_u8, void *stream) {
    if (const char *why = xrep::layout_error(layout)) return fail(nullptr, XARM_E_INVALID, "xarm_replay_add: %s", why);
    if (layout->num_envs == 0) return XARM_OK;
    if (!ring || !clock || !obs || !next_obs || !act || !rew || !done_u8 || (layout->goal_dim > 0 && (!ag || !dg || !next_ag)))
        return fail(nullptr, XARM_E_INVALID, "%s", "xarm_replay_add: NULL pointer");
    xrep::AddArgs a;
    a.L = xrep::make_layout(*layout);
    a.ring = ring; a.clock = clock; a.obs = obs; a.ag = ag; a.dg = dg; a.next_obs = next_obs; a.next_ag = next_ag; a.act = act; a.rew = rew;
    a.done = done_u8; a.timeout = timeout_u8;
    const int le = xrep::launch_replay_add(a, clock, stream);
    if (le != 0) return fail(nullptr, XARM_E_HIP, "xarm_replay_add: %s", hipGetErrorString((hipError_t)le));
    return XARM_OK;
}

int xarm_replay_sample(const xarm_replay_layout *layout, const float *ring, int64_t *clock, uint64_t seed, int32_t batch,
                       int32_t handle_timeout, const double *stats, double clip_obs, double eps, float *out_obs, float *out_next_obs,
                       float *out_act, float *out_rew, float *out_done, float *out_use, int64_t *out_env_i64, int64_t *out_time_i64,
                       void *stream) {
    if (const char *why = xrep::layout_error(layout)) return fail(nullptr, XARM_E_INVALID, "xarm_replay_sample: %s", why);
    if (batch < 0) return fail(nullptr, XARM_E_INVALID, "%s", "xarm_replay_sample: batch must be >= 0");
    if (stats && !(clip_obs > 0.0)) return fail(nullptr, XARM_E_INVALID, "%s", "xarm_replay_sample: clip_obs must be > 0");
    if (stats && (!(eps > 0.0) || !isfinite(eps))) return fail(nullptr, XARM_E_INVALID, "%s", "xarm_replay_sample: eps must be finite and > 0");
    if (batch == 0 || layout->num_envs == 0) return XARM_OK;
    if (!ring || !clock || !out_obs || !out_next_obs || !out_act || !out_rew || !out_done || !out_use)
        return fail(nullptr, XARM_E_INVALID, "%s", "xarm_replay_sample: NULL pointer");
    xrep::SampleArgs a;
    a.L = xrep::make_layout(*layout);
    a.ring = ring; a.clock = clock; a.seed = seed; a.batch = batch; a.handle_timeout = handle_timeout != 0;
    a.stats = stats; a.clip_obs = clip_obs; a.eps = eps;
    a.obs = out_obs; a.next_obs = out_next_obs; a.act = out_act; a.rew = out_rew; a.done = out_done; a.use = out_use;
    a.env = out_env_i64; a.time = out_time_i64;
    const int le = xrep::launch_replay_sample(a, clock, stream);
    if (le != 0) return fail(nullptr, XARM_E_HIP, "xarm_replay_sample: %s", hipGetErrorString((hipError_t)le));
    return XARM_OK;
}

// ------------------------------------------------------------------------------------- policy evaluation (xarm_k_eval.hip)
static int eval_state(xeval::StepArgs &a, const char *fmt, const xarm_eval_layout *layout, double *cur_ret, int32_t *cur_len,
                      int32_t *count, int32_t *remaining, double *records) {
    if (const char *why = xeval::layout_error(layout)) return fail(nullptr, XARM_E_INVALID, fmt, why);
    if (layout->num_envs > 0 && (!cur_ret || !cur_len || !count || !remaining || !records))
        return fail(nullptr, XARM_E_INVALID, fmt, "NULL pointer");
    a.L = xeval::make_layout(*layout);
    a.cur_ret = cur_ret; a.cur_len = cur_len; a.count = count; a.remaining = remaining; a.records = records;
    a.rew = nullptr; a.done = a.success = a.keep = nullptr;
    return XARM_OK;
}

int xarm_eval_begin(const xarm_eval_layout *layout, double *cur_ret, int32_t *cur_len_i32, int32_t *count_i32, int32_t *remaining_i32,
                    double *records, void *stream) {
    xeval::StepArgs a;
    if (const int rc = eval_state(a, "xarm_eval_begin: %s", layout, cur_ret, cur_len_i32, count_i32, remaining_i32, records)) return rc;
    if (layout->num_envs == 0) return XARM_OK;
    const int le = xeval::launch_eval_begin(a, stream);
    if (le != 0) return fail(nullptr, XARM_E_HIP, "xarm_eval_begin: %s", hipGetErrorString((hipError_t)le));
    return XARM_OK;
}

int xarm_eval_step(const xarm_eval_layout *layout, double *cur_ret, int32_t *cur_len_i32, int32_t *count_i32, int32_t *remaining_i32,
                   double *records, const float *rew, const uint8_t *done_u8, const uint8_t *success_u8, const uint8_t *keep_u8,
                   void *stream) {
    xeval::StepArgs a;
    if (const int rc = eval_state(a, "xarm_eval_step: %s", layout, cur_ret, cur_len_i32, count_i32, remaining_i32, records)) return rc;
    if (layout->num_envs == 0) return XARM_OK;
    if (!rew || !done_u8 || !success_u8) return fail(nullptr, XARM_E_INVALID, "%s", "xarm_eval_step: NULL pointer");
    a.rew = rew; a.done = done_u8; a.success = success_u8; a.keep = keep_u8;
    const int le = xeval::launch_eval_step(a, stream);
    if (le != 0) return fail(nullptr, XARM_E_HIP, "xarm_eval_step: %s", hipGetErrorString((hipError_t)le));
    return XARM_OK;
}

int xarm_eval_summary(const xarm_eval_layout *layout, const int32_t *count_i32, const double *records, double *out_f64, void *stream) {
    if (const char *why = xeval::layout_error(layout)) return fail(nullptr, XARM_E_INVALID, "xarm_eval_summary: %s", why);
    if (layout->num_envs == 0) return XARM_OK;
    if (!count_i32 || !records || !out_f64) return fail(nullptr, XARM_E_INVALID, "%s", "xarm_eval_summary: NULL pointer");
    xeval::SummaryArgs a;
    a.L = xeval::make_layout(*layout);
    a.count = count_i32; a.records = records; a.out = out_f64;
    const int le = xeval::launch_eval_summary(a, stream);
    if (le != 0) return fail(nullptr, XARM_E_HIP, "xarm_eval_summary: %s", hipGetErrorString((hipError_t)le));
    return XARM_OK;
}

// ------------------------------------------------------------------------------------- VecNormalize + monitor (xarm_k_norm.hip)
int xarm_norm_work_bytes(const xarm_norm_layout *layout, int64_t *bytes) {
    if (const char *why = xnorm::layout_error(layout)) return fail(nullptr, XARM_E_INVALID, "xarm_norm_work_bytes: %s", why);
    if (!bytes) return fail(nullptr, XARM_E_INVALID, "%s", "xarm_norm_work_bytes: NULL pointer");
    *bytes = xnorm::work_bytes(xnorm::make_layout(*layout));
    return XARM_OK;
}

static void norm_args(xnorm::Args &a, const xarm_norm_layout *layout, const xarm_norm_params *p, void *work) {
    a.L = xnorm::make_layout(*layout);
    a.clip_obs = p->clip_obs; a.clip_rew = p->clip_reward; a.eps = p->eps; a.gamma = p->gamma; a.t_seconds = p->t_seconds;
    a.update = p->update != 0;
    xnorm::carve_work(a, work);
}

int xarm_norm_obs(const xarm_norm_layout *layout, const xarm_norm_params *params, double *stats, float *ret, void *work,
                  const float *obs, const float *achieved_goal, const float *desired_goal, int32_t zero_ret, float *out_nobs,
                  void *stream) {
    if (const char *why = xnorm::layout_error(layout)) return fail(nullptr, XARM_E_INVALID, "xarm_norm_obs: %s", why);
    if (const char *why = xnorm::params_error(params)) return fail(nullptr, XARM_E_INVALID, "xarm_norm_obs: %s", why);
    if (layout->num_envs == 0) return XARM_OK;
    if (!stats || !work || !obs || !out_nobs || (layout->goal_dim > 0 && (!achieved_goal || !desired_goal)) || (zero_ret && !ret))
        return fail(nullptr, XARM_E_INVALID, "%s", "xarm_norm_obs: NULL pointer");
    xnorm::Args a = {};
    norm_args(a, layout, params, work);
    a.step = 0; a.zero_ret = zero_ret != 0;
    a.stats = stats; a.ret = ret; a.obs = obs; a.ag = achieved_goal; a.dg = desired_goal; a.nobs = out_nobs;
    const int le = xnorm::launch_norm(a, stream);
    if (le != 0) return fail(nullptr, XARM_E_HIP, "xarm_norm_obs: %s", hipGetErrorString((hipError_t)le));
    return XARM_OK;
}

int xarm_norm_step(const xarm_norm_layout *layout, const xarm_norm_params *params, double *stats, float *ret, float *ep_ret,
                   float *ep_len, float *ring, int64_t *n_i64, void *work, const float *obs, const float *achieved_goal,
                   const float *desired_goal, const float *rew, const uint8_t *done_u8, const uint8_t *keep_u8, float *out_nobs,
                   float *out_nrew, void *stream) {
    if (const char *why = xnorm::layout_error(layout)) return fail(nullptr, XARM_E_INVALID, "xarm_norm_step: %s", why);
    if (const char *why = xnorm::params_error(params)) return fail(nullptr, XARM_E_INVALID, "xarm_norm_step: %s", why);
    if (layout->num_envs == 0) return XARM_OK;
    if (!stats || !ret || !ep_ret || !ep_len || !ring || !n_i64 || !work || !obs || !rew || !done_u8 || !out_nobs || !out_nrew ||
        (layout->goal_dim > 0 && (!achieved_goal || !desired_goal)))
        return fail(nullptr, XARM_E_INVALID, "%s", "xarm_norm_step: NULL pointer");
    xnorm::Args a = {};
    norm_args(a, layout, params, work);
    a.step = 1; a.zero_ret = 0;
    a.stats = stats; a.ret = ret; a.ep_ret = ep_ret; a.ep_len = ep_len; a.ring = ring; a.n = n_i64;
    a.obs = obs; a.ag = achieved_goal; a.dg = desired_goal; a.rew = rew; a.done = done_u8; a.keep = keep_u8;
    a.nobs = out_nobs; a.nrew = out_nrew;
    const int le = xnorm::launch_norm(a, stream);
    if (le != 0) return fail(nullptr, XARM_E_HIP, "xarm_norm_step: %s", hipGetErrorString((hipError_t)le));
    return XARM_OK;
}

// ------------------------------------------------------------------------------------------------ MlpPolicy (xarm_k_policy.hip)
int xarm_policy_act(const xarm_policy_layout *layout, const xarm_policy_params *params, const xarm_policy_weights *weights,
                    const double *stats, int64_t *calls_i64, const float *obs, const float *achieved_goal, const float *desired_goal,
                    float *out_action, float *out_env_action, float *out_logp, float *out_value, void *stream) {
    if (const char *why = xpol::layout_error(layout)) return fail(nullptr, XARM_E_INVALID, "xarm_policy_act: %s", why);
    if (const char *why = xpol::params_error(params, stats != nullptr)) return fail(nullptr, XARM_E_INVALID, "xarm_policy_act: %s", why);
    if (!weights) return fail(nullptr, XARM_E_INVALID, "%s", "xarm_policy_act: weights is NULL");
    if (layout->num_envs == 0) return XARM_OK;
    if (const char *why = xpol::pointer_error(layout, params, weights, calls_i64, obs, achieved_goal, desired_goal, out_action, out_env_action,
                                              out_value))
        return fail(nullptr, XARM_E_INVALID, "xarm_policy_act: %s", why);
    xpol::Args a = {};
    xpol::fill_args(a, layout, params, weights);
    a.stats = stats; a.calls = calls_i64; a.x0 = obs; a.x1 = achieved_goal; a.x2 = desired_goal;
    a.action = out_action; a.env_action = out_env_action; a.logp = out_logp; a.value = out_value;
    const int le = xpol::launch_policy(a, calls_i64, stream);
    if (le != 0) return fail(nullptr, XARM_E_HIP, "xarm_policy_act: %s", hipGetErrorString((hipError_t)le));
    return XARM_OK;
}

// ------------------------------------------------------------------------------------------------ A2C update (xarm_k_a2c.hip)
int xarm_a2c_workspace_bytes(const xarm_a2c_layout *layout, int64_t *bytes) {
    if (const char *why = xa2c::layout_error(layout)) return fail(nullptr, XARM_E_INVALID, "xarm_a2c_workspace_bytes: %s", why);
    if (!bytes) return fail(nullptr, XARM_E_INVALID, "%s", "xarm_a2c_workspace_bytes: NULL pointer");
    xa2c::Shape s;
    xa2c::Work k;
    xa2c::fill_shape(s, layout);
    xa2c::fill_work(k, s);
    *bytes = k.total;
    return XARM_OK;
}

int xarm_a2c_update(const xarm_a2c_layout *layout, const xarm_a2c_params *params, const xarm_policy_weights *weights,
                    const xarm_policy_weights *square_avg, const float *obs, const float *action, const float *reward, const float *done,
                    const float *use, const float *last_obs, void *workspace, float *out_returns, float *out_grad, float *out_stats,
                    void *stream) {
    if (const char *why = xa2c::layout_error(layout)) return fail(nullptr, XARM_E_INVALID, "xarm_a2c_update: %s", why);
    if (const char *why = xa2c::params_error(params)) return fail(nullptr, XARM_E_INVALID, "xarm_a2c_update: %s", why);
    if (!weights || !square_avg) return fail(nullptr, XARM_E_INVALID, "%s", "xarm_a2c_update: weights / square_avg is NULL");
    if (layout->num_envs == 0) return XARM_OK;
    if (const char *why = xa2c::pointer_error(layout, weights, square_avg, obs, action, reward, done, last_obs, workspace))
        return fail(nullptr, XARM_E_INVALID, "xarm_a2c_update: %s", why);
    xa2c::Dev d = {};
    xa2c::Work k;
    xa2c::fill_shape(d.s, layout);
    xa2c::fill_hyper(d.h, params);
    xa2c::fill_work(k, d.s);
    xa2c::tensors_of(weights, d.w);
    xa2c::tensors_of(square_avg, d.sq);
    d.pi = xpol::Tower{d.w[0], d.w[1], d.w[2], d.w[3], d.w[4], d.w[5]};
    d.vf = xpol::Tower{d.w[6], d.w[7], d.w[8], d.w[9], d.w[10], d.w[11]};
    d.obs = obs; d.action = action; d.reward = reward; d.done = done; d.use = use; d.last_obs = last_obs;
    char *base = (char *)workspace;
    d.boot = (float *)(base + k.boot); d.mean = (float *)(base + k.mean); d.env = (float *)(base + k.env); d.value = (float *)(base + k.value);
    d.ret = (float *)(base + k.ret); d.partial = (float *)(base + k.partial); d.scal = (double *)(base + k.scal); d.grad = (float *)(base + k.grad);
    d.normpart = (double *)(base + k.normpart);
    d.out_returns = out_returns; d.out_grad = out_grad; d.out_stats = out_stats;
    const int le = xa2c::launch_update(d, stream);
    if (le != 0) return fail(nullptr, XARM_E_HIP, "xarm_a2c_update: %s", hipGetErrorString((hipError_t)le));
    return XARM_OK;
}

// ------------------------------------------------------------------------------------------------ PPO update (xarm_k_ppo.hip)
int xarm_ppo_workspace_bytes(const xarm_ppo_layout *layout, int64_t *bytes) {
    if (const char *why = xppo::layout_error(layout)) return fail(nullptr, XARM_E_INVALID, "xarm_ppo_workspace_bytes: %s", why);
    if (!bytes) return fail(nullptr, XARM_E_INVALID, "%s", "xarm_ppo_workspace_bytes: NULL pointer");
    xppo::Shape s;
    xppo::Work k;
    xppo::fill_shape(s, layout);
    xppo::fill_work(k, s);
    *bytes = k.total;
    return XARM_OK;
}

int xarm_ppo_update(const xarm_ppo_layout *layout, const xarm_ppo_params *params, const xarm_policy_weights *weights,
                    const xarm_policy_weights *exp_avg, const xarm_policy_weights *exp_avg_sq, int64_t *step_i64, const float *obs,
                    const float *action, const float *reward, const float *done, const float *use, const float *last_obs,
                    const float *old_logp, const int32_t *perm, void *workspace, float *out_adv, float *out_returns, float *out_grad,
                    float *out_stats, void *stream) {
    return xarm_ppo_update_opt(layout, params, weights, exp_avg, exp_avg_sq, step_i64, obs, action, reward, done, use, last_obs, old_logp, perm,
                               workspace, out_adv, out_returns, out_grad, out_stats, nullptr, stream);
}

int xarm_ppo_update_opt(const xarm_ppo_layout *layout, const xarm_ppo_params *params, const xarm_policy_weights *weights,
                        const xarm_policy_weights *exp_avg, const xarm_policy_weights *exp_avg_sq, int64_t *step_i64, const float *obs,
                        const float *action, const float *reward, const float *done, const float *use, const float *last_obs,
                        const float *old_logp, const int32_t *perm, void *workspace, float *out_adv, float *out_returns, float *out_grad,
                        float *out_stats, const xarm_ppo_options *options, void *stream) {
    if (const char *why = xppo::layout_error(layout)) return fail(nullptr, XARM_E_INVALID, "xarm_ppo_update: %s", why);
    if (const char *why = xppo::params_error(params)) return fail(nullptr, XARM_E_INVALID, "xarm_ppo_update: %s", why);
    if (const char *why = xppo::options_error(options)) return fail(nullptr, XARM_E_INVALID, "xarm_ppo_update: %s", why);
    if (!weights || !exp_avg || !exp_avg_sq) return fail(nullptr, XARM_E_INVALID, "%s", "xarm_ppo_update: weights / exp_avg / exp_avg_sq is NULL");
    if (layout->num_envs == 0) return XARM_OK;
    if (const char *why = xppo::pointer_error(layout, weights, exp_avg, exp_avg_sq, step_i64, obs, action, reward, done, last_obs, perm, workspace))
        return fail(nullptr, XARM_E_INVALID, "xarm_ppo_update: %s", why);
    xppo::Dev d = {};
    xppo::Work k;
    xppo::fill_shape(d.s, layout);
    xppo::fill_hyper(d.h, params, options);
    xppo::fill_work(k, d.s);
    xa2c::tensors_of(weights, d.w);
    xa2c::tensors_of(exp_avg, d.m);
    xa2c::tensors_of(exp_avg_sq, d.v);
    d.pi = xpol::Tower{d.w[0], d.w[1], d.w[2], d.w[3], d.w[4], d.w[5]};
    d.vf = xpol::Tower{d.w[6], d.w[7], d.w[8], d.w[9], d.w[10], d.w[11]};
    d.step = step_i64;
    d.obs = obs; d.action = action; d.reward = reward; d.done = done; d.use = use; d.last_obs = last_obs; d.old_logp = old_logp; d.perm = perm;
    char *base = (char *)workspace;
    d.boot = (float *)(base + k.boot); d.mean = (float *)(base + k.mean); d.env = (float *)(base + k.env); d.value = (float *)(base + k.value);
    d.adv = (float *)(base + k.adv); d.ret = (float *)(base + k.ret); d.oldlp = (float *)(base + k.oldlp); d.musig = (double *)(base + k.musig);
    d.partial = (float *)(base + k.partial); d.scal = (double *)(base + k.scal); d.grad = (float *)(base + k.grad);
    d.normpart = (double *)(base + k.normpart); d.adam = (float *)(base + k.adam); d.stop = (int *)(d.adam + 2);
    d.out_adv = out_adv; d.out_returns = out_returns; d.out_grad = out_grad; d.out_stats = out_stats;
    const int le = xppo::launch_update(d, stream);
    if (le != 0) return fail(nullptr, XARM_E_HIP, "xarm_ppo_update: %s", hipGetErrorString((hipError_t)le));
    return XARM_OK;
}

// ------------------------------------------------------------------------------------------------ SAC update (xarm_k_sac.hip)
int xarm_sac_workspace_bytes(const xarm_sac_layout *layout, int64_t *bytes) {
    if (const char *why = xsac::layout_error(layout)) return fail(nullptr, XARM_E_INVALID, "xarm_sac_workspace_bytes: %s", why);
    if (!bytes) return fail(nullptr, XARM_E_INVALID, "%s", "xarm_sac_workspace_bytes: NULL pointer");
    xsac::Shape s;
    xsac::Work k;
    xsac::fill_shape(s, layout);
    xsac::fill_work(k, s);
    *bytes = k.total;
    return XARM_OK;
}

int xarm_sac_act(const xarm_sac_layout *layout, const xarm_sac_params *params, const xarm_sac_weights *weights, int64_t *calls_i64,
                 const float *obs, float *out_action, float *out_logp, void *stream) {
    if (const char *why = xsac::layout_error(layout)) return fail(nullptr, XARM_E_INVALID, "xarm_sac_act: %s", why);
    if (!params) return fail(nullptr, XARM_E_INVALID, "%s", "xarm_sac_act: params is NULL");
    if (!weights) return fail(nullptr, XARM_E_INVALID, "%s", "xarm_sac_act: weights is NULL");
    if (layout->batch_size == 0) return XARM_OK;
    if (const char *why = xsac::act_pointer_error(params, weights, calls_i64, obs, out_action)) return fail(nullptr, XARM_E_INVALID, "xarm_sac_act: %s", why);
    xsac::Dev d = {};
    xsac::fill_shape(d.s, layout);
    d.h.seed = params->seed;
    d.h.deterministic = params->deterministic != 0;
    d.actor = xsac::tower_of(weights->actor);
    d.calls = calls_i64; d.obs = obs; d.out_action = out_action; d.out_logp = out_logp;
    const int le = xsac::launch_act(d, stream);
    if (le != 0) return fail(nullptr, XARM_E_HIP, "xarm_sac_act: %s", hipGetErrorString((hipError_t)le));
    return XARM_OK;
}

int xarm_sac_update(const xarm_sac_layout *layout, const xarm_sac_params *params, const xarm_sac_weights *weights,
                    const xarm_sac_weights *exp_avg, const xarm_sac_weights *exp_avg_sq, int64_t *step_i64, const float *obs,
                    const float *next_obs, const float *action, const float *reward, const float *done, const float *use,
                    const float *noise_pi, const float *noise_next, void *workspace, float *out_grad, float *out_dqda, float *out_target,
                    float *out_stats, void *stream) {
    if (const char *why = xsac::layout_error(layout)) return fail(nullptr, XARM_E_INVALID, "xarm_sac_update: %s", why);
    if (const char *why = xsac::params_error(params)) return fail(nullptr, XARM_E_INVALID, "xarm_sac_update: %s", why);
    if (!weights || !exp_avg || !exp_avg_sq) return fail(nullptr, XARM_E_INVALID, "%s", "xarm_sac_update: weights / exp_avg / exp_avg_sq is NULL");
    if (layout->batch_size == 0) return XARM_OK;
    if (const char *why = xsac::pointer_error(weights, exp_avg, exp_avg_sq, step_i64, obs, next_obs, action, reward, done, workspace))
        return fail(nullptr, XARM_E_INVALID, "xarm_sac_update: %s", why);
    xsac::Dev d = {};
    xsac::Work k;
    xsac::fill_shape(d.s, layout);
    xsac::fill_hyper(d.h, params);
    xsac::fill_work(k, d.s);
    xsac::tensors_of(weights, d.w);
    xsac::tensors_of(exp_avg, d.m);
    xsac::tensors_of(exp_avg_sq, d.v);
    for (int i = 0; i < 6; i++) {
        d.tq[i] = const_cast<float *>(weights->q1_target[i]);
        d.tq[6 + i] = const_cast<float *>(weights->q2_target[i]);
    }
    d.actor = xsac::tower_of(weights->actor); d.q1 = xsac::tower_of(weights->q1); d.q2 = xsac::tower_of(weights->q2);
    d.q1t = xsac::tower_of(weights->q1_target); d.q2t = xsac::tower_of(weights->q2_target);
    d.step = step_i64;
    d.obs = obs; d.next_obs = next_obs; d.action = action; d.reward = reward; d.done = done; d.use = use; d.noise_pi = noise_pi; d.noise_next = noise_next;
    char *base = (char *)workspace;
    d.hdr = (float *)(base + k.hdr); d.y = (float *)(base + k.y); d.logp = (float *)(base + k.logp); d.z = (float *)(base + k.z);
    d.xq = (float *)(base + k.xq); d.xpi = (float *)(base + k.xpi); d.qpi = (float *)(base + k.qpi); d.dqda = (float *)(base + k.dqda);
    d.partial = (float *)(base + k.partial); d.scal_rows = (double *)(base + k.scal_rows); d.scal_q = (double *)(base + k.scal_q);
    d.scal_p = (double *)(base + k.scal_p);
    d.out_grad = out_grad; d.out_dqda = out_dqda; d.out_target = out_target; d.out_stats = out_stats;
    const int le = xsac::launch_update(d, stream);
    if (le != 0) return fail(nullptr, XARM_E_HIP, "xarm_sac_update: %s", hipGetErrorString((hipError_t)le));
    return XARM_OK;
}

// ------------------------------------------------------------------------------------------------ wide SAC update (xarm_k_sacw.hip)
int xarm_sacw_workspace_bytes(const xarm_sacw_layout *layout, int64_t *bytes) {
    if (const char *why = xsacw::layout_error(layout)) return fail(nullptr, XARM_E_INVALID, "xarm_sacw_workspace_bytes: %s", why);
    if (!bytes) return fail(nullptr, XARM_E_INVALID, "%s", "xarm_sacw_workspace_bytes: NULL pointer");
    xsacw::Dev d = {};
    xsacw::fill_shape(d.s, layout);
    *bytes = xsacw::fill_work(d, nullptr);
    return XARM_OK;
}

int xarm_sacw_act(const xarm_sacw_layout *layout, const xarm_sac_params *params, const xarm_sacw_weights *weights, int64_t *calls_i64,
                  const float *obs, void *workspace, float *out_action, float *out_logp, void *stream) {
    if (const char *why = xsacw::layout_error(layout)) return fail(nullptr, XARM_E_INVALID, "xarm_sacw_act: %s", why);
    if (!params) return fail(nullptr, XARM_E_INVALID, "%s", "xarm_sacw_act: params is NULL");
    if (!weights) return fail(nullptr, XARM_E_INVALID, "%s", "xarm_sacw_act: weights is NULL");
    if (layout->batch_size == 0) return XARM_OK;
    if (const char *why = xsacw::act_pointer_error(layout, params, weights, calls_i64, obs, workspace, out_action))
        return fail(nullptr, XARM_E_INVALID, "xarm_sacw_act: %s", why);
    xsacw::Dev d = {};
    xsacw::fill_shape(d.s, layout);
    d.h.seed = params->seed;
    d.h.deterministic = params->deterministic != 0;
    for (int i = 0; i < d.s.tp; i++) d.w[i] = const_cast<float *>(weights->actor[i]);
    xsacw::fill_work_act(d, workspace);
    d.calls = calls_i64; d.obs = obs; d.out_action = out_action; d.out_logp = out_logp;
    const int le = xsacw::launch_act(d, stream);
    if (le != 0) return fail(nullptr, XARM_E_HIP, "xarm_sacw_act: %s", hipGetErrorString((hipError_t)le));
    return XARM_OK;
}

int xarm_sacw_update(const xarm_sacw_layout *layout, const xarm_sac_params *params, const xarm_sacw_weights *weights,
                     const xarm_sacw_weights *exp_avg, const xarm_sacw_weights *exp_avg_sq, int64_t *step_i64, const float *obs,
                     const float *next_obs, const float *action, const float *reward, const float *done, const float *use,
                     const float *noise_pi, const float *noise_next, void *workspace, float *out_grad, float *out_dqda, float *out_target,
                     float *out_stats, float *out_q, void *stream) {
    if (const char *why = xsacw::layout_error(layout)) return fail(nullptr, XARM_E_INVALID, "xarm_sacw_update: %s", why);
    if (const char *why = xsac::params_error(params)) return fail(nullptr, XARM_E_INVALID, "xarm_sacw_update: %s", why);
    if (!weights || !exp_avg || !exp_avg_sq) return fail(nullptr, XARM_E_INVALID, "%s", "xarm_sacw_update: weights / exp_avg / exp_avg_sq is NULL");
    if (layout->batch_size == 0) return XARM_OK;
    if (const char *why = xsacw::pointer_error(layout, weights, exp_avg, exp_avg_sq, step_i64, obs, next_obs, action, reward, done, workspace))
        return fail(nullptr, XARM_E_INVALID, "xarm_sacw_update: %s", why);
    xsacw::Dev d = {};
    xsacw::fill_shape(d.s, layout);
    xsac::fill_hyper(d.h, params);
    xsacw::tensors_of(d.s, weights, d.w, d.tq);
    xsacw::tensors_of(d.s, exp_avg, d.m, nullptr);
    xsacw::tensors_of(d.s, exp_avg_sq, d.v, nullptr);
    xsacw::fill_work(d, workspace);
    d.step = step_i64;
    d.obs = obs; d.next_obs = next_obs; d.action = action; d.reward = reward; d.done = done; d.use = use; d.noise_pi = noise_pi; d.noise_next = noise_next;
    d.out_grad = out_grad; d.out_dqda = out_dqda; d.out_target = out_target; d.out_stats = out_stats; d.out_q = out_q;
    const int le = xsacw::launch_update(d, stream);
    if (le != 0) return fail(nullptr, XARM_E_HIP, "xarm_sacw_update: %s", hipGetErrorString((hipError_t)le));
    return XARM_OK;
}

// ------------------------------------------------------------------------------------------------ TD3 update (xarm_k_td3.hip)
int xarm_td3_workspace_bytes(const xarm_sacw_layout *layout, int64_t *bytes) {
    if (const char *why = xsacw::layout_error(layout)) return fail(nullptr, XARM_E_INVALID, "xarm_td3_workspace_bytes: %s", why);
    if (!bytes) return fail(nullptr, XARM_E_INVALID, "%s", "xarm_td3_workspace_bytes: NULL pointer");
    xtd3::Dev d = {};
    xtd3::shape_of(d.s, layout);
    *bytes = xtd3::fill_work(d, nullptr);
    return XARM_OK;
}

int xarm_td3_act(const xarm_sacw_layout *layout, const xarm_td3_params *params, const xarm_td3_weights *weights, int64_t *calls_i64,
                 const float *obs, void *workspace, float *out_action, void *stream) {
    if (const char *why = xsacw::layout_error(layout)) return fail(nullptr, XARM_E_INVALID, "xarm_td3_act: %s", why);
    if (const char *why = xtd3::params_error(params)) return fail(nullptr, XARM_E_INVALID, "xarm_td3_act: %s", why);
    if (!weights) return fail(nullptr, XARM_E_INVALID, "%s", "xarm_td3_act: weights is NULL");
    if (layout->batch_size == 0) return XARM_OK;
    if (const char *why = xtd3::act_pointer_error(layout, params, weights, calls_i64, obs, workspace, out_action))
        return fail(nullptr, XARM_E_INVALID, "xarm_td3_act: %s", why);
    xtd3::Dev d = {};
    xtd3::shape_of(d.s, layout);
    xtd3::fill_hyper(d.h, params);
    for (int i = 0; i < d.s.tp; i++) d.w[i] = const_cast<float *>(weights->actor[i]);
    xtd3::fill_work_act(d, workspace);
    d.calls = calls_i64; d.obs = obs; d.out_action = out_action;
    const int le = xtd3::launch_act(d, stream);
    if (le != 0) return fail(nullptr, XARM_E_HIP, "xarm_td3_act: %s", hipGetErrorString((hipError_t)le));
    return XARM_OK;
}

int xarm_td3_update(const xarm_sacw_layout *layout, const xarm_td3_params *params, const xarm_td3_weights *weights,
                    const xarm_td3_weights *exp_avg, const xarm_td3_weights *exp_avg_sq, int64_t *step_i64, const float *obs,
                    const float *next_obs, const float *action, const float *reward, const float *done, const float *use,
                    const float *noise_next, void *workspace, float *out_grad, float *out_target, float *out_q, float *out_dqda,
                    float *out_stats, void *stream) {
    if (const char *why = xsacw::layout_error(layout)) return fail(nullptr, XARM_E_INVALID, "xarm_td3_update: %s", why);
    if (const char *why = xtd3::params_error(params)) return fail(nullptr, XARM_E_INVALID, "xarm_td3_update: %s", why);
    if (!weights || !exp_avg || !exp_avg_sq) return fail(nullptr, XARM_E_INVALID, "%s", "xarm_td3_update: weights / exp_avg / exp_avg_sq is NULL");
    if (layout->batch_size == 0) return XARM_OK;
    if (const char *why = xtd3::pointer_error(layout, weights, exp_avg, exp_avg_sq, step_i64, obs, next_obs, action, reward, done, workspace))
        return fail(nullptr, XARM_E_INVALID, "xarm_td3_update: %s", why);
    xtd3::Dev d = {};
    xtd3::shape_of(d.s, layout);
    xtd3::fill_hyper(d.h, params);
    xtd3::tensors_of(d.s, weights, d.w, d.tg);
    xtd3::tensors_of(d.s, exp_avg, d.m, nullptr);
    xtd3::tensors_of(d.s, exp_avg_sq, d.v, nullptr);
    xtd3::fill_work(d, workspace);
    d.step = step_i64;
    d.obs = obs; d.next_obs = next_obs; d.action = action; d.reward = reward; d.done = done; d.use = use; d.noise_next = noise_next;
    d.out_grad = out_grad; d.out_target = out_target; d.out_q = out_q; d.out_dqda = out_dqda; d.out_stats = out_stats;
    const int le = xtd3::launch_update(d, stream);
    if (le != 0) return fail(nullptr, XARM_E_HIP, "xarm_td3_update: %s", hipGetErrorString((hipError_t)le));
    return XARM_OK;
}

// ------------------------------------------------------------------------------------------------ wide MlpPolicy (xarm_k_acw.hip)
int xarm_acw_workspace_bytes(const xarm_acw_layout *layout, int64_t *bytes) {
    if (const char *why = xacw::layout_error(layout)) return fail(nullptr, XARM_E_INVALID, "xarm_acw_workspace_bytes: %s", why);
    if (!bytes) return fail(nullptr, XARM_E_INVALID, "%s", "xarm_acw_workspace_bytes: NULL pointer");
    xacw::Dev d = {};
    xacw::fill_shape(d, layout);
    *bytes = xacw::fill_work(d, nullptr);
    return XARM_OK;
}

int xarm_acw_act(const xarm_acw_layout *layout, const xarm_policy_params *params, const xarm_acw_weights *weights, const double *stats,
                 int64_t *calls_i64, const float *obs, const float *achieved_goal, const float *desired_goal, void *workspace, float *out_action,
                 float *out_env_action, float *out_logp, float *out_value, void *stream) {
    if (const char *why = xacw::layout_error(layout)) return fail(nullptr, XARM_E_INVALID, "xarm_acw_act: %s", why);
    if (const char *why = xpol::params_error(params, stats != nullptr)) return fail(nullptr, XARM_E_INVALID, "xarm_acw_act: %s", why);
    if (!weights) return fail(nullptr, XARM_E_INVALID, "%s", "xarm_acw_act: weights is NULL");
    if (layout->num_rows == 0) return XARM_OK;
    if (const char *why = xacw::pointer_error(layout, params, weights, calls_i64, obs, achieved_goal, desired_goal, workspace, out_value))
        return fail(nullptr, XARM_E_INVALID, "xarm_acw_act: %s", why);
    xacw::Dev d = {};
    xacw::fill_dev(d, layout, params, weights, stats, calls_i64, obs, achieved_goal, desired_goal, workspace, out_action, out_env_action, out_logp,
                   out_value);
    const int le = xacw::launch_act(d, calls_i64, stream);
    if (le != 0) return fail(nullptr, XARM_E_HIP, "xarm_acw_act: %s", hipGetErrorString((hipError_t)le));
    return XARM_OK;
}

// ------------------------------------------------------------------------------------------------ wide PPO update (xarm_k_ppow.hip)
int xarm_ppow_workspace_bytes(const xarm_ppow_layout *layout, int64_t *bytes) {
    if (const char *why = xppow::layout_error(layout)) return fail(nullptr, XARM_E_INVALID, "xarm_ppow_workspace_bytes: %s", why);
    if (!bytes) return fail(nullptr, XARM_E_INVALID, "%s", "xarm_ppow_workspace_bytes: NULL pointer");
    xppow::Dev d = {};
    xppow::fill_shape(d, layout);
    *bytes = xppow::fill_work(d, nullptr);
    return XARM_OK;
}

int xarm_ppow_update(const xarm_ppow_layout *layout, const xarm_ppo_params *params, const xarm_acw_weights *weights, const xarm_acw_weights *exp_avg,
                     const xarm_acw_weights *exp_avg_sq, int64_t *step_i64, const float *obs, const float *action, const float *reward,
                     const float *done, const float *use, const float *last_obs, const float *old_logp, const int32_t *perm, void *workspace,
                     float *out_adv, float *out_returns, float *out_grad, float *out_stats, void *stream) {
    return xarm_ppow_update_opt(layout, params, weights, exp_avg, exp_avg_sq, step_i64, obs, action, reward, done, use, last_obs, old_logp, perm,
                                workspace, out_adv, out_returns, out_grad, out_stats, nullptr, stream);
}

int xarm_ppow_update_opt(const xarm_ppow_layout *layout, const xarm_ppo_params *params, const xarm_acw_weights *weights,
                         const xarm_acw_weights *exp_avg, const xarm_acw_weights *exp_avg_sq, int64_t *step_i64, const float *obs,
                         const float *action, const float *reward, const float *done, const float *use, const float *last_obs,
                         const float *old_logp, const int32_t *perm, void *workspace, float *out_adv, float *out_returns, float *out_grad,
                         float *out_stats, const xarm_ppo_options *options, void *stream) {
    if (const char *why = xppow::layout_error(layout)) return fail(nullptr, XARM_E_INVALID, "xarm_ppow_update: %s", why);
    if (const char *why = xppo::params_error(params)) return fail(nullptr, XARM_E_INVALID, "xarm_ppow_update: %s", why);
    if (const char *why = xppo::options_error(options)) return fail(nullptr, XARM_E_INVALID, "xarm_ppow_update: %s", why);
    if (!weights || !exp_avg || !exp_avg_sq) return fail(nullptr, XARM_E_INVALID, "%s", "xarm_ppow_update: weights / exp_avg / exp_avg_sq is NULL");
    if (layout->num_envs == 0) return XARM_OK;
    if (const char *why = xppow::pointer_error(layout, weights, exp_avg, exp_avg_sq, step_i64, obs, action, reward, done, last_obs, perm, workspace))
        return fail(nullptr, XARM_E_INVALID, "xarm_ppow_update: %s", why);
    xppow::Dev d = {};
    xppow::fill_shape(d, layout);
    xppo::fill_hyper(d.h, params, options);
    xppow::tensors_of(d, weights, d.w);
    xppow::tensors_of(d, exp_avg, d.m);
    xppow::tensors_of(d, exp_avg_sq, d.v);
    xppow::fill_work(d, workspace);
    d.step = step_i64;
    d.obs = obs; d.action = action; d.reward = reward; d.done = done; d.use = use; d.last_obs = last_obs; d.old_logp = old_logp; d.perm = perm;
    d.out_adv = out_adv; d.out_returns = out_returns; d.out_grad = out_grad; d.out_stats = out_stats;
    const int le = xppow::launch_update(d, stream);
    if (le != 0) return fail(nullptr, XARM_E_HIP, "xarm_ppow_update: %s", hipGetErrorString((hipError_t)le));
    return XARM_OK;
}

// ------------------------------------------------------------------------------------------------ wide A2C update (xarm_k_a2cw.hip)
int xarm_a2cw_workspace_bytes(const xarm_a2cw_layout *layout, int64_t *bytes) {
    if (const char *why = xa2cw::layout_error(layout)) return fail(nullptr, XARM_E_INVALID, "xarm_a2cw_workspace_bytes: %s", why);
    if (!bytes) return fail(nullptr, XARM_E_INVALID, "%s", "xarm_a2cw_workspace_bytes: NULL pointer");
    xa2cw::Dev d = {};
    xa2cw::fill_shape(d, layout);
    *bytes = xa2cw::fill_work(d, nullptr);
    return XARM_OK;
}

int xarm_a2cw_update(const xarm_a2cw_layout *layout, const xarm_a2c_params *params, const xarm_acw_weights *weights,
                     const xarm_acw_weights *square_avg, const float *obs, const float *action, const float *reward, const float *done,
                     const float *use, const float *last_obs, void *workspace, float *out_returns, float *out_grad, float *out_stats,
                     void *stream) {
    if (const char *why = xa2cw::layout_error(layout)) return fail(nullptr, XARM_E_INVALID, "xarm_a2cw_update: %s", why);
    if (const char *why = xa2c::params_error(params)) return fail(nullptr, XARM_E_INVALID, "xarm_a2cw_update: %s", why);
    if (!weights || !square_avg) return fail(nullptr, XARM_E_INVALID, "%s", "xarm_a2cw_update: weights / square_avg is NULL");
    if (layout->num_envs == 0) return XARM_OK;
    if (const char *why = xa2cw::pointer_error(layout, weights, square_avg, obs, action, reward, done, last_obs, workspace))
        return fail(nullptr, XARM_E_INVALID, "xarm_a2cw_update: %s", why);
    xa2cw::Dev d = {};
    xa2cw::fill_shape(d, layout);
    xa2c::fill_hyper(d.h, params);
    xppow::tensors_of(d, weights, d.w);
    xppow::tensors_of(d, square_avg, d.sq);
    xa2cw::fill_work(d, workspace);
    d.obs = obs; d.action = action; d.reward = reward; d.done = done; d.use = use; d.last_obs = last_obs;
    d.out_returns = out_returns; d.out_grad = out_grad; d.out_stats = out_stats;
    const int le = xa2cw::launch_update(d, stream);
    if (le != 0) return fail(nullptr, XARM_E_HIP, "xarm_a2cw_update: %s", hipGetErrorString((hipError_t)le));
    return XARM_OK;
}


// ------------------------------------------------------------------------------------- device shuffle (xarm_k_rollout.hip)
int xarm_perm_fill(int32_t *perm_i32, int32_t n_epochs, int64_t N, uint64_t seed, int64_t *calls_i64, void *stream) {
    if (const char *why = xroll::perm_error(n_epochs, N)) return fail(nullptr, XARM_E_INVALID, "xarm_perm_fill: %s", why);
    if (N == 0) return XARM_OK;
    if (!perm_i32 || !calls_i64) return fail(nullptr, XARM_E_INVALID, "%s", "xarm_perm_fill: NULL pointer");
    const int le = xroll::launch_perm_fill(perm_i32, n_epochs, N, seed, calls_i64, stream);
    if (le != 0) return fail(nullptr, XARM_E_HIP, "xarm_perm_fill: %s", hipGetErrorString((hipError_t)le));
    return XARM_OK;
}

} // extern "C"
