// xarm_replay_core.h - device-resident uniform replay: stable-baselines3's plain `ReplayBuffer` for the off-policy
// learners on a flat-observation env, or on a goal env without relabelling.  One env's part of `add` and one output row's part of
// `sample`.  The kernels are in xarm_k_replay.hip; like the HER core this also compiles for the host (g++ -DXARM_HOST_BUILD
// -ffp-contract=off, tests/hostbuild_replay/) for the CPU tests.  Every index is integer arithmetic, the payload is copied or
// passes through the float64 expression of xnorm::norm_value, and both builds are compiled with contraction off: the host
// build and the device agree bit for bit.
//
//   ring      float32 [T, E, R], one record per (slot, env): obs | next_obs | action | reward | done | timeout,
//             R = 2 D + A + 3.  D is the width of the learner's flat observation: obs_dim on a flat env (goal_dim = 0), else
//             obs_dim + 2 goal_dim with the row observation | achieved_goal | desired_goal, read through three row pointers
//             as xpol::input_at and xarm_norm_obs read them; next_obs is next_observation | next_achieved_goal | desired_goal.
//             Every offset is int64: T E R passes 2^31 at sizes in use.
//   clock     int64 [2] = {t, sample_calls}: t transitions per env were added so far.  Slot s holds the absolute time
//             tau = largest tau <= t - 1 with tau mod T = s (not stored); min(t, T) slots are filled.
//
// add (env e): write the record at slot t mod T.  No episode bookkeeping: O(E).
// pick (row b): idx = mulhi64(Philox(seed; b, sample_calls, 0, TAG + sample_calls >> 32), min(t, T) E), slot = idx / E,
// env = idx % E: uniform over the stored transitions, no rejection, no atomics.
// row: obs and next_obs [D] (with `stats`, the normaliser's double [2 D + 4], column j as
// xnorm::norm_value(x, mean_j, sqrt(var_j + eps), clip_obs) - xpol::input_at's expression; null: copied), action [A], the raw
// reward, done = stored done && !(handle_timeout && stored timeout) as float32, use = 1.  While the buffer is empty the row
// is all zero with use = 0.
#pragma once
#include <stdint.h>
#include <math.h>
#include "../../include/xarm_hip.h"
#include "xarm_core.h"
#include "xarm_her_core.h"
#include "xarm_norm_core.h"

namespace xrep {

constexpr uint32_t PHILOX_TAG = 0x52504C00u;   // c3 of every draw: apart from the HER buffer's draws and the envs' reset draws

struct Layout {
    int64_t E, T;
    int obs, goal, act, D, R;
    int o_nobs, o_act, o_rew, o_done, o_timeout;   // float offsets inside a record (obs is at 0)
};

inline Layout make_layout(const xarm_replay_layout &l) {   // host side of both builds: the kernels get the Layout as an argument
    Layout L;
    L.E = l.num_envs; L.T = l.horizon; L.obs = l.obs_dim; L.goal = l.goal_dim; L.act = l.act_dim;
    L.D = L.obs + 2 * L.goal;
    L.o_nobs = L.D; L.o_act = 2 * L.D; L.o_rew = L.o_act + L.act; L.o_done = L.o_rew + 1; L.o_timeout = L.o_done + 1;
    L.R = L.o_timeout + 1;
    return L;
}

// null when the layout is usable, else what is wrong with it
inline const char *layout_error(const xarm_replay_layout *l) {
    if (!l) return "layout is NULL";
    if (l->num_envs < 0) return "num_envs must be >= 0";
    if (l->horizon < 1) return "horizon must be >= 1";
    if (l->obs_dim < 1 || l->act_dim < 1) return "obs_dim and act_dim must be >= 1";
    if (l->goal_dim < 0) return "goal_dim must be >= 0";
    if (l->obs_dim > (1 << 20) || l->goal_dim > (1 << 20) || l->act_dim > (1 << 20)) return "obs_dim, goal_dim and act_dim must be <= 2^20";
    return nullptr;
}

struct AddArgs {
    Layout L;
    float *ring;
    const int64_t *clock;
    const float *obs, *ag, *dg, *next_obs, *next_ag, *act, *rew;   // [E, dim] rows of the step being stored; ag / dg / next_ag unused when goal == 0
    const uint8_t *done, *timeout;                                 // timeout may be null: no transition is a truncation
};

struct SampleArgs {
    Layout L;
    const float *ring;
    const int64_t *clock;
    uint64_t seed;
    int32_t batch, handle_timeout;
    const double *stats;                  // nullable: the normaliser's [2 D + 4]
    double clip_obs, eps;
    float *obs, *next_obs, *act, *rew, *done, *use;   // [batch, dim]
    int64_t *env, *time;                  // nullable, for tracing
};

XARM_HD int64_t rec_index(const Layout &L, int64_t slot, int64_t e) { return (slot * L.E + e) * (int64_t)L.R; }

// env e's part of add at time t, spread over the nl lanes of its group (host: lane 0 of 1).  The caller advances the clock.
XARM_HD void replay_add_env(const AddArgs &a, int64_t t, int64_t e, int lane, int nl) {
    const Layout &L = a.L;
    if (t < 0) return;
    float *rec = a.ring + rec_index(L, t % L.T, e);
    xher::copy_in(rec, a.obs + e * L.obs, L.obs, lane, nl);
    xher::copy_in(rec + L.o_nobs, a.next_obs + e * L.obs, L.obs, lane, nl);
    if (L.goal > 0) {
        xher::copy_in(rec + L.obs, a.ag + e * L.goal, L.goal, lane, nl);
        xher::copy_in(rec + L.obs + L.goal, a.dg + e * L.goal, L.goal, lane, nl);
        xher::copy_in(rec + L.o_nobs + L.obs, a.next_ag + e * L.goal, L.goal, lane, nl);
        xher::copy_in(rec + L.o_nobs + L.obs + L.goal, a.dg + e * L.goal, L.goal, lane, nl);
    }
    xher::copy_in(rec + L.o_act, a.act + e * L.act, L.act, lane, nl);
    if (lane == 0) {
        rec[L.o_rew] = a.rew[e];
        rec[L.o_done] = a.done[e] != 0 ? 1.0f : 0.0f;
        rec[L.o_timeout] = (a.timeout != nullptr && a.timeout[e] != 0) ? 1.0f : 0.0f;
    }
}

struct Pick { int64_t slot, env, t_abs; int ok; };

// row b's entry; a function of (t, calls, seed, b) alone, so every lane of the row's group computes the same one
XARM_HD Pick replay_pick(const Layout &L, int64_t t, int64_t calls, uint64_t seed, int64_t b) {
    Pick p;
    p.slot = p.env = p.t_abs = 0; p.ok = 0;
    const int64_t filled = t < L.T ? t : L.T;
    if (filled <= 0 || L.E <= 0) return p;
    const uint64_t n = (uint64_t)filled * (uint64_t)L.E;
    uint32_t o[4];
    xk::philox(seed, (uint32_t)b, (uint32_t)calls, 0u, PHILOX_TAG + (uint32_t)((uint64_t)calls >> 32), o);
    const uint64_t idx = xher::mulhi64(((uint64_t)o[0] << 32) | o[1], n);   // uniform on [0, n)
    p.slot = (int64_t)(idx / (uint64_t)L.E);
    p.env = (int64_t)(idx % (uint64_t)L.E);
    const int64_t last = t - 1;
    p.t_abs = last - ((last - p.slot) % L.T);
    p.ok = 1;
    return p;
}

// D columns of a stored observation row into a learner's row: copied, or normalised with the frozen statistics
XARM_HD void obs_out(const SampleArgs &a, float *dst, const float *src, bool ok, int lane, int nl) {
    const int D = a.L.D;
    for (int j = lane; j < D; j += nl) {
        float x = 0.0f;
        if (ok) {
            x = src[j];
            if (a.stats != nullptr) x = xnorm::norm_value(x, a.stats[j], sqrt(a.stats[D + j] + a.eps), a.clip_obs);
        }
        dst[j] = x;
    }
}

// write row b from its pick
XARM_HD void replay_write_row(const SampleArgs &a, const Pick &p, int64_t b, int lane, int nl) {
    const Layout &L = a.L;
    const bool ok = p.ok != 0;
    const float *rec = a.ring + rec_index(L, p.slot, p.env);               // record (0, 0) for an empty buffer: never read
    obs_out(a, a.obs + b * L.D, rec, ok, lane, nl);
    obs_out(a, a.next_obs + b * L.D, rec + L.o_nobs, ok, lane, nl);
    xher::copy_out(a.act + b * L.act, rec + L.o_act, L.act, ok, lane, nl);
    if (lane == 0) {
        bool d = false;
        if (ok) d = rec[L.o_done] != 0.0f && !(a.handle_timeout != 0 && rec[L.o_timeout] != 0.0f);
        a.rew[b] = ok ? rec[L.o_rew] : 0.0f;
        a.done[b] = d ? 1.0f : 0.0f;
        a.use[b] = ok ? 1.0f : 0.0f;
        if (a.env != nullptr) a.env[b] = p.env;       // 0 for an empty buffer
        if (a.time != nullptr) a.time[b] = p.t_abs;
    }
}

#if defined(__HIPCC__) && !defined(XARM_HOST_BUILD)
// k_replay_add + k_replay_tick / k_replay_sample + k_replay_tick on `stream` (xarm_k_replay.hip); return the launches' hipError_t
int launch_replay_add(const AddArgs &a, int64_t *clock, void *stream);
int launch_replay_sample(const SampleArgs &a, int64_t *clock, void *stream);
#endif

}  // namespace xrep
