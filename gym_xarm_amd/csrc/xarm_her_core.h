// xarm_her_core.h - device-resident hindsight-experience replay: one env's part of `add` and one output row's
// part of `sample`.  The kernels are in xarm_k_her.hip; like the render and physics cores this also compiles for the host
// (g++ -DXARM_HOST_BUILD, tests/hostbuild_her/) for the CPU tests.  Every index is integer arithmetic and the payload is
// only copied, so the host build and the device agree bit for bit.
//
//   ring      float32 [T, E, R], one record per (slot, env): obs | next_obs | ag | next_ag | dg | act | rew | done,
//             R = 2 obs_dim + 3 goal_dim + act_dim + 2.  Every offset is int64: T E R passes 2^31 at sizes in use.
//   ep_end    int64 [T, E]: absolute time of the last transition of the entry's episode, -1 while that episode runs
//   ep_first  int64 [T, E]: absolute time of the episode's first transition, written when the episode closes
//   ep_start  int64 [E]: absolute time the env's running episode began
//   clock     int64 [2] = {t, sample_calls}: t transitions per env were added so far.  Slot s holds the absolute time
//             tau = largest tau <= t - 1 with tau mod T = s (not stored); min(t, T) slots are filled.
//
// add (env e): write the record at slot t mod T; if done[e], walk the times max(ep_start[e], t - T + 1) .. t, set ep_end = t
// and ep_first = ep_start[e] there, then ep_start[e] = t + 1.  O(episode length), finished envs only; an env touches only
// its own column.
// pick (row b): candidates are drawn uniformly from the min(t, T) E stored entries with Philox(seed; b, sample_calls,
// attempt) and the first one whose episode is closed (ep_end >= 0) is taken: rejection sampling, exactly uniform over the
// valid entries without ever building their list.  After HER_MAX_TRIES rejected candidates the row fails (ok = 0, all-zero
// row, a device counter counts it): at a valid share v of the stored entries that has probability (1 - v)^64.
#pragma once
#include <stdint.h>
#include "../../include/xarm_hip.h"
#include "xarm_core.h"

#define XARM_HER_MAX_TRIES 64

namespace xher {

enum { FUTURE = XARM_HER_FUTURE, FINAL = XARM_HER_FINAL, EPISODE = XARM_HER_EPISODE };
constexpr uint32_t PHILOX_TAG = 0x48455200u;   // c3 of every draw: keeps the stream apart from the envs' reset draws

struct Layout {
    int64_t E, T;
    int obs, goal, act, R;
    int o_nobs, o_ag, o_nag, o_dg, o_act, o_rew, o_done;   // float offsets inside a record (obs is at 0)
};

inline Layout make_layout(const xarm_her_layout &l) {   // host side of both builds: the kernels get the Layout as an argument
    Layout L;
    L.E = l.num_envs; L.T = l.horizon; L.obs = l.obs_dim; L.goal = l.goal_dim; L.act = l.act_dim;
    L.o_nobs = L.obs; L.o_ag = 2 * L.obs; L.o_nag = L.o_ag + L.goal; L.o_dg = L.o_nag + L.goal; L.o_act = L.o_dg + L.goal;
    L.o_rew = L.o_act + L.act; L.o_done = L.o_rew + 1; L.R = L.o_done + 1;
    return L;
}

// null when the layout is usable, else what is wrong with it
inline const char *layout_error(const xarm_her_layout *l) {
    if (!l) return "layout is NULL";
    if (l->num_envs < 0) return "num_envs must be >= 0";
    if (l->horizon < 2) return "horizon must be >= 2";
    if (l->obs_dim < 1 || l->goal_dim < 1 || l->act_dim < 1) return "obs_dim, goal_dim and act_dim must be >= 1";
    if (l->obs_dim > (1 << 20) || l->goal_dim > (1 << 20) || l->act_dim > (1 << 20)) return "obs_dim, goal_dim and act_dim must be <= 2^20";
    return nullptr;
}

struct AddArgs {
    Layout L;
    float *ring;
    int64_t *ep_end, *ep_first, *ep_start;
    const int64_t *clock;
    const float *obs, *next_obs, *ag, *next_ag, *dg, *act, *rew;   // [E, dim] rows of the step being stored
    const uint8_t *done;
};

struct SampleArgs {
    Layout L;
    const float *ring;
    const int64_t *ep_end, *ep_first, *clock;
    uint64_t seed;
    int32_t strategy, batch, n_her;
    float *obs, *next_obs, *ag, *next_ag, *goal, *act, *rew;        // [batch, dim]
    uint8_t *done, *ok;
    int64_t *env, *time, *goal_time, *fail_count;
};

XARM_HD int64_t rec_index(const Layout &L, int64_t slot, int64_t e) { return (slot * L.E + e) * (int64_t)L.R; }

// high 64 bits of a * b, from 32-bit halves so that g++ and hipcc compute it by the same steps
XARM_HD uint64_t mulhi64(uint64_t a, uint64_t b) {
    const uint64_t a0 = (uint32_t)a, a1 = a >> 32, b0 = (uint32_t)b, b1 = b >> 32;
    const uint64_t p00 = a0 * b0, p01 = a0 * b1, p10 = a1 * b0, p11 = a1 * b1;
    const uint64_t mid = (p00 >> 32) + (uint32_t)p01 + (uint32_t)p10;
    return p11 + (p01 >> 32) + (p10 >> 32) + (mid >> 32);
}
XARM_HD int64_t mulhi32(uint32_t r, int64_t n) { return (int64_t)(((uint64_t)r * (uint64_t)(uint32_t)n) >> 32); }   // uniform on [0, n), n < 2^32

XARM_HD void copy_in(float *dst, const float *src, int n, int lane, int nl) {
    for (int i = lane; i < n; i += nl) dst[i] = src[i];
}

// env e's part of add at time t, spread over the nl lanes of its group (host: lane 0 of 1).  The caller advances the clock.
XARM_HD void her_add_env(const AddArgs &a, int64_t t, int64_t e, int lane, int nl) {
    const Layout &L = a.L;
    if (t < 0) return;
    const int64_t s = t % L.T;
    float *rec = a.ring + rec_index(L, s, e);
    copy_in(rec, a.obs + e * L.obs, L.obs, lane, nl);
    copy_in(rec + L.o_nobs, a.next_obs + e * L.obs, L.obs, lane, nl);
    copy_in(rec + L.o_ag, a.ag + e * L.goal, L.goal, lane, nl);
    copy_in(rec + L.o_nag, a.next_ag + e * L.goal, L.goal, lane, nl);
    copy_in(rec + L.o_dg, a.dg + e * L.goal, L.goal, lane, nl);
    copy_in(rec + L.o_act, a.act + e * L.act, L.act, lane, nl);
    const bool d = a.done[e] != 0;
    if (lane == 0) {
        rec[L.o_rew] = a.rew[e];
        rec[L.o_done] = d ? 1.0f : 0.0f;
    }
    if (!d) {
        if (lane == 0) a.ep_end[s * L.E + e] = -1;
        return;
    }
    // the episode ends with this transition: close every entry of it that is still in the ring (this one included)
    const int64_t start = a.ep_start[e];
    const int64_t oldest = t - L.T + 1;
    for (int64_t tau = (start > oldest ? start : oldest) + lane; tau <= t; tau += nl) {
        const int64_t i = (tau % L.T) * L.E + e;
        a.ep_end[i] = t;
        a.ep_first[i] = start;
    }
    if (lane == 0) a.ep_start[e] = t + 1;
}

struct Pick { int64_t slot, env, t_abs, t_goal; int ok; };

// row b's entry and goal time; a function of (tables, t, calls, seed, strategy, b) alone, so every lane of the row's group
// computes the same one
XARM_HD Pick her_pick(const Layout &L, const int64_t *ep_end, const int64_t *ep_first, int64_t t, int64_t calls, uint64_t seed,
                      int strategy, int64_t b) {
    Pick p;
    p.slot = p.env = p.t_abs = p.t_goal = 0; p.ok = 0;
    const int64_t filled = t < L.T ? t : L.T;
    if (filled <= 0 || L.E <= 0) return p;
    const uint64_t n = (uint64_t)filled * (uint64_t)L.E;
    for (int attempt = 0; attempt < XARM_HER_MAX_TRIES; attempt++) {
        uint32_t o[4];
        xk::philox(seed, (uint32_t)b, (uint32_t)calls, (uint32_t)attempt, PHILOX_TAG + (uint32_t)((uint64_t)calls >> 32), o);
        const uint64_t idx = mulhi64(((uint64_t)o[0] << 32) | o[1], n);   // uniform on [0, n)
        const int64_t end = ep_end[idx];
        if (end < 0) continue;
        p.slot = (int64_t)(idx / (uint64_t)L.E);
        p.env = (int64_t)(idx % (uint64_t)L.E);
        const int64_t last = t - 1;
        p.t_abs = last - ((last - p.slot) % L.T);
        int64_t lo = p.t_abs, hi = end;
        if (strategy == FINAL) lo = end;
        if (strategy == EPISODE) {
            lo = ep_first[idx];
            if (lo < t - L.T) lo = t - L.T;     // the part of the episode that is still in the ring
            if (lo < 0) lo = 0;
        }
        if (hi < lo) hi = lo;                   // never with tables this file wrote: keeps a corrupt table inside the ring
        p.t_goal = lo + mulhi32(o[2], hi - lo + 1);
        p.ok = 1;
        return p;
    }
    return p;
}

XARM_HD void copy_out(float *dst, const float *src, int n, bool ok, int lane, int nl) {
    for (int i = lane; i < n; i += nl) dst[i] = ok ? src[i] : 0.0f;
}

// write row b from its pick: the stored fields, and for a relabelled row (b < n_her) next_ag of the goal record as the goal.
// The reward is the stored one; the caller recomputes rows [0, n_her) with xarm_compute_reward.  Returns 1 for a failed row.
XARM_HD int her_write_row(const SampleArgs &a, const Pick &p, int64_t b, int lane, int nl) {
    const Layout &L = a.L;
    const bool ok = p.ok != 0;
    const float *rec = a.ring + rec_index(L, p.slot, p.env);               // record (0, 0) for a failed row: never read
    const float *grec = a.ring + rec_index(L, ok ? p.t_goal % L.T : 0, p.env);
    copy_out(a.obs + b * L.obs, rec, L.obs, ok, lane, nl);
    copy_out(a.next_obs + b * L.obs, rec + L.o_nobs, L.obs, ok, lane, nl);
    copy_out(a.ag + b * L.goal, rec + L.o_ag, L.goal, ok, lane, nl);
    copy_out(a.next_ag + b * L.goal, rec + L.o_nag, L.goal, ok, lane, nl);
    copy_out(a.goal + b * L.goal, b < a.n_her ? grec + L.o_nag : rec + L.o_dg, L.goal, ok, lane, nl);
    copy_out(a.act + b * L.act, rec + L.o_act, L.act, ok, lane, nl);
    if (lane == 0) {
        a.rew[b] = ok ? rec[L.o_rew] : 0.0f;
        a.done[b] = ok ? (uint8_t)(rec[L.o_done] != 0.0f) : (uint8_t)0;
        a.env[b] = p.env; a.time[b] = p.t_abs; a.goal_time[b] = p.t_goal;   // all 0 for a failed row
        a.ok[b] = (uint8_t)p.ok;
    }
    return ok ? 0 : 1;
}

#if defined(__HIPCC__) && !defined(XARM_HOST_BUILD)
// k_her_add + k_her_tick / k_her_sample + k_her_tick on `stream` (xarm_k_her.hip); return the launches' hipError_t
int launch_her_add(const AddArgs &a, int64_t *clock, void *stream);
int launch_her_sample(const SampleArgs &a, int64_t *clock, void *stream);
#endif

}  // namespace xher
