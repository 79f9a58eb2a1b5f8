// xarm_td3_core.h - device-resident TD3: one call is one gradient step of stable-baselines3's TD3.train() on a batch drawn
// from a replay buffer - target policy smoothing, the clipped double-Q target, the step of both critics and, on every policy_delay-th
// call, the deterministic actor's step through dq1/da and the Polyak step of all three targets - as a CHAIN of per-layer GEMM launches
// over the wide SAC's passes (xarm_sacw_core.h), for equal-width towers of two or three hidden layers of 64, 128, 192 or
// 256 units, tanh or ReLU.  This file states the chain (run_update, run_act) and every per-row and per-parameter formula ONCE;
// xarm_k_td3.hip executes the jobs on the device and the host build (g++ -DXARM_HOST_BUILD -ffp-contract=off, tests/hostbuild_td3/)
// executes the same jobs with loops over the same workspace, so everything - rows, gradients, parameters, stats - is equal between
// the two builds bit for bit.
//
// Called, not copied: xsacw's Shape, row ranges, jobs, passes (fwd_pass, bd_pass, wg_pass), Gate, row_noise, layout and tower checks and
// HostExec; xsac::target_row (with alpha = 0), polyak; xpol::noise4, tanh_f; xopt::adam, adam_scalars, slice_sum, n_use, tensor_at.
//
//   towers    actor D -> H x L -> A (tanh on the output), critics Dq = D + A -> H x L -> 1; targets of all three
//   smoothing a' = clamp(tanh(actor_target(next_obs)) + clamp(target_policy_noise z, -c, c), -1, 1), c = target_noise_clip;
//             z: Philox keyed (seed, row_offset + row, step at call start), xsacw::row_noise's stream 1, or the given tensor
//   target    y = fmaf(gamma (1 - done), min(q1_t, q2_t)(next_obs | a'), reward)
//   critics   delta_i = 2 (q_i - y) use; g = (float)(sum over ranges / n_use); Adam at count t + 1, t = step at call start
//   delay     flag = (t + 1) % policy_delay != 0, written by row 0 of `head` into the workspace; every launch of the actor phase
//             carries Gate{flag, INT64_MAX}: with the flag up it returns after one uniform read.  The decision is the device's, so a
//             captured call replays correctly, and the launch count is the same on every call
//   actor     a_pi = tanh(actor(obs)); dq1/da under the STEPPED q1 at obs | a_pi from d = 1; output delta -dq1/da_c (1 - a_pi_c^2) use;
//             Adam at count (t + 1) / policy_delay
//   Polyak    target = (1 - tau) target + tau net for the actor and both (stepped) critics, in the actor phase's apply launch
//   stats     critic_loss = (sum (q1 - y)^2 use + sum (q2 - y)^2 use) / n_use (no factor 1/2), actor_loss = -mean q1_pi, q1_pi, target_q =
//             mean y, n_use, actor_stepped, 0, 0; on a delayed call actor_loss and q1_pi are left as the caller's row has them
//   flat      the trained tensors one after the other: actor's 2 (L + 1), q1's, q2's: P floats
#pragma once
#include "xarm_sacw_core.h"

namespace xtd3 {

using xpol::fma32;
using xsac::MAX_A;
using xsacw::Gate;
using xsacw::Shape;
using xsacw::TowerRef;
using xsacw::TP;

constexpr int NTW = 3 * TP;                 // the most trained tensors: three towers
constexpr int RED = xsacw::RED;
constexpr int NSC = 4;                      // scalars (double): use, ((q1 - y)^2 + (q2 - y)^2) use, y use, q1_pi use
constexpr int MODE_DET = 0, MODE_GAUSS = 1, MODE_UNIFORM = 2;
constexpr uint32_t PHILOX_TAG = 0x54443300u; // "TD3\0": the uniform draws of an act call

struct Hyper {
    xsac::Hyper base;                       // adam, gamma, tau, one_m_tau, seed: what xsac::polyak and xsacw::row_noise read
    float sigma, clip, act_noise;
    int policy_delay, mode;
};

struct Dev {
    Shape s;
    Hyper h;
    float *w[NTW], *m[NTW], *v[NTW], *tg[NTW];      // trained: actor, q1, q2; targets in the same order
    int64_t *step, *calls;
    const float *obs, *next_obs, *action, *reward, *done, *use, *noise_next;
    // the workspace
    float *hdr;                     // Adam's two scalars of the critics' step, then of the actor's
    int *flag;                      // the delay gate: 1 on a call without an actor step
    double *scal;                   // NSC sums over rows
    float *y, *ones, *xq, *xpi, *xn;        // per row: y, 1, obs | action, obs | a_pi, next_obs | a'
    float *outN, *outP;             // the raw outputs of actor_target on next_obs and of the actor on obs
    float *hA, *hS, *dH, *dO;       // hidden activations: the actor's on obs, four scratch towers; deltas of two towers; output deltas
    float *qt, *q, *qpi, *dqda, *partial;
    float *out_grad, *out_dqda, *out_target, *out_stats, *out_q, *out_action;
};

inline const char *params_error(const xarm_td3_params *p) {
    if (!p) return "params is NULL";
    if (!(p->gamma >= 0.0 && p->gamma <= 1.0)) return "gamma must lie in [0, 1]";
    if (const char *why = xopt::adam_error(p->lr, p->beta1, p->beta2, p->eps)) return why;
    if (!(p->tau >= 0.0 && p->tau <= 1.0)) return "tau must lie in [0, 1]";
    if (!(p->target_policy_noise >= 0.0) || !(p->target_policy_noise < 1e300)) return "target_policy_noise must be finite and >= 0";
    if (!(p->target_noise_clip >= 0.0) || !(p->target_noise_clip < 1e300)) return "target_noise_clip must be finite and >= 0";
    if (!(p->action_noise >= 0.0) || !(p->action_noise < 1e300)) return "action_noise must be finite and >= 0";
    if (p->policy_delay < 1) return "policy_delay must be >= 1";
    if (p->mode < MODE_DET || p->mode > MODE_UNIFORM) return "mode must be 0 (deterministic), 1 (Gaussian) or 2 (uniform)";
    return nullptr;
}

inline const char *act_pointer_error(const xarm_sacw_layout *l, const xarm_td3_params *p, const xarm_td3_weights *w, const int64_t *calls,
                                     const float *obs, const void *workspace, const float *action) {
    if (!w) return "weights is NULL";
    if (p->mode != MODE_UNIFORM)
        if (const char *why = xsacw::tower_error(w->actor, 2 * (l->n_hidden + 1))) return why;
    if (p->mode != MODE_DET && !calls) return "NULL calls with a stochastic call";
    if (p->mode != MODE_UNIFORM && !obs) return "NULL observation pointer";
    if (!action) return "NULL out_action";
    return xsacw::workspace_error(workspace);
}

inline const char *pointer_error(const xarm_sacw_layout *l, const xarm_td3_weights *w, const xarm_td3_weights *m, const xarm_td3_weights *v,
                                 const int64_t *step, const float *obs, const float *next_obs, const float *action, const float *reward,
                                 const float *done, const void *workspace) {
    if (!w) return "weights is NULL";
    if (!m || !v) return "exp_avg / exp_avg_sq is NULL";
    const int tp = 2 * (l->n_hidden + 1);
    const float *const *towers[6] = {w->actor, w->q1, w->q2, w->actor_target, w->q1_target, w->q2_target};
    for (int i = 0; i < 6; i++)
        if (const char *why = xsacw::tower_error(towers[i], tp)) return why;
    const xarm_td3_weights *st[2] = {m, v};
    for (int k = 0; k < 2; k++)
        for (int i = 0; i < tp; i++)
            if (!st[k]->actor[i] || !st[k]->q1[i] || !st[k]->q2[i]) return k ? "NULL exp_avg_sq pointer" : "NULL exp_avg pointer";
    if (!step) return "step_i64 is NULL";
    if (!obs || !next_obs || !action || !reward || !done) return "NULL obs / next_obs / action / reward / done";
    return xsacw::workspace_error(workspace);
}

// xsacw's Shape for TD3's towers: the actor has A outputs and there is no log_alpha, so NT = 3 tp and P = Pa + 2 Pq
inline void shape_of(Shape &s, const xarm_sacw_layout *l) {
    s.B = l->batch_size; s.D = l->obs_dim; s.A = l->act_dim; s.Dq = s.D + s.A; s.H = l->hidden; s.L = l->n_hidden; s.NL = s.L + 1;
    s.act = l->activation; s.row_offset = l->row_offset; s.tp = 2 * s.NL; s.NT = 3 * s.tp; s.BH = s.B * s.H;
    s.off[0] = 0;
    for (int t = 0; t < 3; t++)
        for (int k = 0; k < s.NL; k++) {
            const int i = t * s.tp + 2 * k;
            const int64_t nin = xsacw::in_of(s, k, t == 0 ? s.D : s.Dq), nout = xsacw::out_of(s, k, t == 0 ? s.A : 1);
            s.off[i + 1] = s.off[i] + nout * nin;
            s.off[i + 2] = s.off[i + 1] + nout;
        }
    s.Pa = s.off[s.tp]; s.Pq = s.off[2 * s.tp] - s.off[s.tp]; s.P = s.off[s.NT];
    xsacw::fill_ranges(s);
}

inline void fill_hyper(Hyper &h, const xarm_td3_params *p) {
    h = Hyper{};
    xopt::fill_adam(h.base.adam, p->lr, p->beta1, p->beta2, p->eps);
    h.base.gamma = (float)p->gamma; h.base.tau = (float)p->tau; h.base.one_m_tau = (float)(1.0 - p->tau); h.base.seed = p->seed;
    h.sigma = (float)p->target_policy_noise; h.clip = (float)p->target_noise_clip; h.act_noise = (float)p->action_noise;
    h.policy_delay = p->policy_delay; h.mode = p->mode;
}

// the trained tensors of a weights struct in the flat order; tg: the targets in the same order
inline void tensors_of(const Shape &s, const xarm_td3_weights *w, float **t, float **tg) {
    for (int i = 0; i < s.tp; i++) {
        t[i] = const_cast<float *>(w->actor[i]);
        t[s.tp + i] = const_cast<float *>(w->q1[i]);
        t[2 * s.tp + i] = const_cast<float *>(w->q2[i]);
        if (tg) {
            tg[i] = const_cast<float *>(w->actor_target[i]);
            tg[s.tp + i] = const_cast<float *>(w->q1_target[i]);
            tg[2 * s.tp + i] = const_cast<float *>(w->q2_target[i]);
        }
    }
}

// carve the workspace (each part 16-byte aligned); returns its size in bytes.  base may be null (size only)
inline int64_t fill_work(Dev &d, void *base) {
    const Shape &s = d.s;
    int64_t at = 0;
    char *b = (char *)base;
    auto take = [&at, b](int64_t floats) { char *o = b ? b + at : nullptr; at += (floats * 4 + 15) & ~(int64_t)15; return (float *)o; };
    const int64_t B = s.B, pmax = s.Pa > 2 * s.Pq ? s.Pa : 2 * s.Pq;
    d.hdr = take(4); d.flag = (int *)take(4); d.scal = (double *)take(2 * NSC);
    d.y = take(B); d.ones = take(B);
    d.xq = take(B * s.Dq); d.xpi = take(B * s.Dq); d.xn = take(B * s.Dq);
    d.outN = take(B * s.A); d.outP = take(B * s.A);
    d.hA = take(s.L * s.BH); d.hS = take(4 * s.L * s.BH); d.dH = take(2 * s.L * s.BH); d.dO = take(2 * B > B * s.A ? 2 * B : B * s.A);
    d.qt = take(2 * B); d.q = take(2 * B); d.qpi = take(B); d.dqda = take(B * s.A);
    d.partial = take((int64_t)s.S * pmax);
    return at;
}

// the act call carves only what it uses
inline int64_t fill_work_act(Dev &d, void *base) {
    int64_t at = 0;
    char *b = (char *)base;
    auto take = [&at, b](int64_t floats) { char *o = b ? b + at : nullptr; at += (floats * 4 + 15) & ~(int64_t)15; return (float *)o; };
    d.outP = take(d.s.B * d.s.A);
    d.hS = take(d.s.L * d.s.BH);
    return at;
}

// ------------------------------------------------------------------------------------------------------------ the rows' parts
XARM_HD float clamp_f(float x, float lo, float hi) { return x < lo ? lo : (x > hi ? hi : x); }

// target policy smoothing of one output: clamp(tanh(out) + clamp(sigma z, -c, c), -1, 1)
XARM_HD float smooth_action(float out, float z, float sigma, float clip) {
    const float t = xpol::tanh_f(out);
    const float nz = clamp_f(sigma * z, -clip, clip);
    return clamp_f(t + nz, -1.0f, 1.0f);
}

// the critics' output delta and loss term of one row and one critic
XARM_HD float critic_delta(float q, float y, float use, float &loss) {
    const float diff = q - y;
    const float two = 2.0f * diff;
    loss = diff * diff * use;
    return two * use;
}

// the deterministic actor's output delta: -dq1/da (1 - a^2) use
XARM_HD float actor_delta(float dq, float a, float use) {
    const float s = fma32(-a, a, 1.0f);
    const float g = dq * s;
    return -g * use;
}

XARM_HD bool delayed(const Dev &d) { return xsacw::gate_shut(Gate{d.flag, INT64_MAX}); }

// row 0 of head: both Adams' scalars and the delay flag of the call that starts at step t0
XARM_HD void head_first(const Dev &d, int64_t t0) {
    const int64_t t = t0 + 1, pd = d.h.policy_delay, ta = t / pd;
    xopt::adam_scalars(d.h.base.adam, t, d.hdr);
    xopt::adam_scalars(d.h.base.adam, ta > 0 ? ta : 1, d.hdr + 2);
    d.flag[0] = t % pd != 0 ? 1 : 0;
}

// behind actor_target's forward: a' of row n, the rows next_obs | a' and obs | action
XARM_HD void head_row(const Dev &d, int64_t n, int64_t t0) {
    const int D = d.s.D, A = d.s.A, Dq = d.s.Dq;
    float z[MAX_A];
    xsacw::row_noise(d.h.base, d.noise_next, d.noise_next != nullptr ? n : d.s.row_offset + n, t0, 1, A, z);
    for (int j = 0; j < D; j++) {
        d.xn[n * Dq + j] = d.next_obs[n * D + j];
        d.xq[n * Dq + j] = d.obs[n * D + j];
    }
#pragma unroll
    for (int c = 0; c < MAX_A; c++)
        if (c < A) {
            d.xn[n * Dq + D + c] = smooth_action(d.outN[n * A + c], z[c], d.h.sigma, d.h.clip);
            d.xq[n * Dq + D + c] = d.action[n * A + c];
        }
    d.ones[n] = 1.0f;
}

// behind the targets' and the critics' forwards: y, the critics' output deltas 2 (q - y) use, three sums
XARM_HD void crit_row(const Dev &d, int64_t n, double *sums) {
    const int64_t B = d.s.B;
    const float u = d.use != nullptr ? d.use[n] : 1.0f;
    const float y = xsac::target_row(d.h.base.gamma, 0.0f, d.reward[n], d.done[n], d.qt[n], d.qt[B + n], 0.0f);
    d.y[n] = y;
    if (d.out_target != nullptr) d.out_target[n] = y;
    sums[0] += (double)u;
    sums[2] += (double)(y * u);
    for (int i = 0; i < 2; i++) {
        const float q = d.q[i * B + n];
        float loss;
        d.dO[i * B + n] = critic_delta(q, y, u, loss);
        if (d.out_q != nullptr) d.out_q[i * B + n] = q;
        sums[1] += (double)loss;
    }
}

// behind the actor's forward on obs: the row obs | a_pi
XARM_HD void api_row(const Dev &d, int64_t n) {
    const int D = d.s.D, A = d.s.A, Dq = d.s.Dq;
    for (int j = 0; j < D; j++) d.xpi[n * Dq + j] = d.obs[n * D + j];
#pragma unroll
    for (int c = 0; c < MAX_A; c++)
        if (c < A) d.xpi[n * Dq + D + c] = xpol::tanh_f(d.outP[n * A + c]);
}

// behind dq1/da: the actor's output deltas [B, A] at dO, one sum
XARM_HD void pi_row(const Dev &d, int64_t n, double *sums) {
    const int D = d.s.D, A = d.s.A, Dq = d.s.Dq;
    const float u = d.use != nullptr ? d.use[n] : 1.0f;
#pragma unroll
    for (int c = 0; c < MAX_A; c++)
        if (c < A) d.dO[n * A + c] = actor_delta(d.dqda[n * A + c], d.xpi[n * Dq + D + c], u);
    sums[3] += (double)(d.qpi[n] * u);
}

XARM_HD double n_use_of(const Dev &d) { return xopt::n_use(d.scal[0]); }

// the reduce and Adam step of trained parameter p; its ranges' partials at part[s pstride]; sc: Adam's two scalars.  Returns the new value
XARM_HD float adam_param(const Dev &d, int64_t p, int i, int64_t e, const float *part, int64_t pstride, const float *sc) {
    const float gf = (float)(xopt::slice_sum(part, d.s.S, pstride) / n_use_of(d));
    if (d.out_grad != nullptr) d.out_grad[p] = gf;
    float m = d.m[i][e], v = d.v[i][e], w = d.w[i][e];
    xopt::adam(d.h.base.adam, sc, gf, m, v, w);
    d.m[i][e] = m;
    d.v[i][e] = v;
    d.w[i][e] = w;
    return w;
}

// the critics' apply: flat parameter p in [Pa, P)
XARM_HD void apply_critic(const Dev &d, int64_t p) {
    const Shape &s = d.s;
    const int i = xopt::tensor_at(s.off, 0, s.NT, p);
    adam_param(d, p, i, p - s.off[i], d.partial + (p - s.Pa), 2 * s.Pq, d.hdr);
}

// the actor phase's apply: flat parameter p in [0, P) - the actor's reduce, Adam and Polyak step; a critic's Polyak step from the stepped critic
XARM_HD void apply_actor(const Dev &d, int64_t p) {
    const Shape &s = d.s;
    const int i = xopt::tensor_at(s.off, 0, s.NT, p);
    const int64_t e = p - s.off[i];
    const float w = p < s.Pa ? adam_param(d, p, i, e, d.partial + p, s.Pa, d.hdr + 2) : d.w[i][e];
    d.tg[i][e] = xsac::polyak(d.h.base, d.tg[i][e], w);
}

// the call's last writes
XARM_HD void finish(const Dev &d) {
    const bool stepped = !delayed(d);
    if (d.out_stats != nullptr) {
        const double n = n_use_of(d);
        float *o = d.out_stats;
        o[0] = (float)(d.scal[1] / n);
        if (stepped) {
            o[1] = (float)(-d.scal[3] / n);
            o[2] = (float)(d.scal[3] / n);
        }
        o[3] = (float)(d.scal[2] / n); o[4] = (float)n; o[5] = stepped ? 1.0f : 0.0f; o[6] = 0.0f; o[7] = 0.0f;
    }
    d.step[0] = d.step[0] + 1;
}

// the act call's row: noise as xarm_sacw_act draws it
XARM_HD void act_row(const Dev &d, int64_t n) {
    const int A = d.s.A, mode = d.h.mode;
    const int64_t calls = mode == MODE_DET ? 0 : d.calls[0], row = d.s.row_offset + n;
#pragma unroll
    for (int b = 0; b < MAX_A / 4; b++) {
        float q[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        if (4 * b < A) {
            if (mode == MODE_GAUSS) xpol::noise4(d.h.base.seed, row, calls, b, q);
            if (mode == MODE_UNIFORM) {
                uint32_t o[4];
                xk::philox(d.h.base.seed, (uint32_t)row, (uint32_t)((uint64_t)row >> 32), (uint32_t)calls,
                           PHILOX_TAG + (uint32_t)b + ((uint32_t)((uint64_t)calls >> 32) << 2), o);
#pragma unroll
                for (int m = 0; m < 4; m++) q[m] = xk::u01<float>(o[m]);
            }
        }
#pragma unroll
        for (int m = 0; m < 4; m++) {
            const int c = 4 * b + m;
            if (c < A) {
                float a;
                if (mode == MODE_UNIFORM) a = fma32(2.0f, q[m], -1.0f);
                else {
                    const float t = xpol::tanh_f(d.outP[n * A + c]);
                    a = mode == MODE_GAUSS ? clamp_f(t + d.h.act_noise * q[m], -1.0f, 1.0f) : t;
                }
                d.out_action[n * A + c] = a;
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------------------ the chain
constexpr int launches(int n_hidden) { return 7 * n_hidden + 14; }
constexpr int act_launches(int n_hidden, int mode) { return mode == MODE_UNIFORM ? 1 : n_hidden + 2; }   // + the tick of a stochastic call

// one TD3 step: 7 L + 14 launches of `ex`, the same for every batch and on delayed and undelayed calls
//   L + 1  actor_target on next_obs                                         1  head: Adam's scalars, the delay flag, a', the rows
//   L + 1  both targets on next_obs | a', both critics on obs | action     1  crit: y, 2 (q - y) use, n_use
//   L      the critics' hidden deltas    1  their weight gradients         1  critics: reduce, Adam
//   gated by the delay flag:
//   L + 1  the actor on obs              1  the row obs | a_pi             L + 1  the STEPPED q1 on obs | a_pi
//   L + 1  its deltas from d = 1 down to dq1/da                            1  pi: the actor's output deltas
//   L      the actor's hidden deltas     1  its weight gradients           1  actor: reduce, Adam; Polyak of the three targets
//   1      finish: stats, step
template <class X> void run_update(const Dev &d, X &ex) {
    const Shape &s = d.s;
    const int tp = s.tp;
    const TowerRef actor = {d.w, s.D, s.A}, q1 = {d.w + tp, s.Dq, 1}, q2 = {d.w + 2 * tp, s.Dq, 1};
    const TowerRef actor_t = {d.tg, s.D, s.A}, q1t = {d.tg + tp, s.Dq, 1}, q2t = {d.tg + 2 * tp, s.Dq, 1};
    float *hs[4] = {d.hS, d.hS + s.L * s.BH, d.hS + 2 * s.L * s.BH, d.hS + 3 * s.L * s.BH};
    float *dh[2] = {d.dH, d.dH + s.L * s.BH};
    const Gate gate = {d.flag, INT64_MAX};      // the actor phase's: shut while the flag is up
    {
        const TowerRef T[1] = {actor_t};
        const float *in[1] = {d.next_obs};
        float *hid[1] = {hs[0]}, *out[1] = {d.outN};
        xsacw::fwd_pass(s, ex, 1, T, in, hid, out);
    }
    ex.head(d);
    {
        const TowerRef T[4] = {q1t, q2t, q1, q2};
        const float *in[4] = {d.xn, d.xn, d.xq, d.xq};
        float *hid[4] = {hs[0], hs[1], hs[2], hs[3]}, *out[4] = {d.qt, d.qt + s.B, d.q, d.q + s.B};
        xsacw::fwd_pass(s, ex, 4, T, in, hid, out);
    }
    ex.crit(d);
    {
        const TowerRef T[2] = {q1, q2};
        const float *in[2] = {d.xq, d.xq}, *dO[2] = {d.dO, d.dO + s.B};
        float *hid[2] = {hs[2], hs[3]};
        const int64_t base[2] = {0, s.Pq};
        const int t0[2] = {tp, 2 * tp};
        xsacw::bd_pass(s, ex, 2, T, dO, hid, dh);
        xsacw::wg_pass(s, d.partial, ex, 2, T, in, dO, hid, dh, base, t0, 2 * s.Pq);
    }
    ex.apply_critics(d);
    {
        const TowerRef T[1] = {actor};
        const float *in[1] = {d.obs};
        float *hid[1] = {d.hA}, *out[1] = {d.outP};
        xsacw::fwd_pass(s, ex, 1, T, in, hid, out, gate);
    }
    ex.api(d);
    {
        const TowerRef T[1] = {q1};
        const float *in[1] = {d.xpi}, *dO[1] = {d.ones};
        float *hid[1] = {hs[0]}, *out[1] = {d.qpi};
        xsacw::fwd_pass(s, ex, 1, T, in, hid, out, gate);
        xsacw::bd_pass(s, ex, 1, T, dO, hid, dh, gate);
        xsacw::Bd f = {};
        f.B = s.B; f.nj = 1; f.maxN = s.A; f.gate = gate;
        xsacw::BdJob &a = f.j[0];
        a.d = dh[0]; a.K = s.H; a.W = q1.p[0]; a.ldw = s.Dq; a.c0 = s.D; a.h = nullptr; a.out = d.dqda; a.out2 = d.out_dqda;
        a.N = s.A; a.mode = xsacw::ACT_NONE; a.vec = xsacw::vec_ok(a.d, a.d, a.K);
        ex.bd(f);
    }
    ex.pi(d);
    {
        const TowerRef T[1] = {actor};
        const float *in[1] = {d.obs}, *dO[1] = {d.dO};
        float *hid[1] = {d.hA};
        const int64_t base[1] = {0};
        const int t0[1] = {0};
        xsacw::bd_pass(s, ex, 1, T, dO, hid, dh, gate);
        xsacw::wg_pass(s, d.partial, ex, 1, T, in, dO, hid, dh, base, t0, s.Pa, gate);
    }
    ex.apply_actor(d);
    ex.finish(d);
}

// the act call: the actor's forward on obs (none in uniform mode), then the row kernel
template <class X> void run_act(const Dev &d, X &ex) {
    if (d.h.mode != MODE_UNIFORM) {
        const TowerRef T[1] = {{d.w, d.s.D, d.s.A}};
        const float *in[1] = {d.obs};
        float *hid[1] = {d.hS}, *out[1] = {d.outP};
        xsacw::fwd_pass(d.s, ex, 1, T, in, hid, out);
    }
    ex.act(d);
}

#if !defined(__HIPCC__) || defined(XARM_HOST_BUILD)
// ---- the host build: the GEMM jobs through xsacw::HostExec's loops, the rest with the device's thread structure as loops
struct HostExec : xsacw::HostExec {
    int count = 0;
    void fwd(const xsacw::Fwd &f) { xsacw::HostExec::fwd(f); count++; }
    void bd(const xsacw::Bd &f) { xsacw::HostExec::bd(f); count++; }
    void wg(const xsacw::Wg &f) { xsacw::HostExec::wg(f); count++; }
    template <class F> static void rows(const Dev &d, int first, int n, F f) {
        double tot[NSC] = {0.0};
        for (int t = 0; t < RED; t++) {
            double sums[NSC] = {0.0};
            for (int64_t r = t; r < d.s.B; r += RED) f(r, sums);
            for (int i = 0; i < NSC; i++) tot[i] += sums[i];
        }
        for (int i = first; i < first + n; i++) d.scal[i] = tot[i];
    }
    void head(const Dev &d) {
        const int64_t t0 = d.step[0];
        head_first(d, t0);
        for (int64_t n = 0; n < d.s.B; n++) head_row(d, n, t0);
        count++;
    }
    void crit(const Dev &d) { rows(d, 0, 3, [&d](int64_t n, double *s) { crit_row(d, n, s); }); count++; }
    void apply_critics(const Dev &d) {
        for (int64_t p = d.s.Pa; p < d.s.P; p++) apply_critic(d, p);
        count++;
    }
    void api(const Dev &d) {
        count++;
        if (delayed(d)) return;
        for (int64_t n = 0; n < d.s.B; n++) api_row(d, n);
    }
    void pi(const Dev &d) {
        count++;
        if (delayed(d)) return;
        rows(d, 3, 1, [&d](int64_t n, double *s) { pi_row(d, n, s); });
    }
    void apply_actor(const Dev &d) {
        count++;
        if (delayed(d)) return;
        for (int64_t p = 0; p < d.s.P; p++) xtd3::apply_actor(d, p);
    }
    void finish(const Dev &d) { xtd3::finish(d); count++; }
    void act(const Dev &d) {
        for (int64_t n = 0; n < d.s.B; n++) act_row(d, n);
        if (d.h.mode != MODE_DET) d.calls[0] += 1;
    }
};
#endif

#if defined(__HIPCC__) && !defined(XARM_HOST_BUILD)
// the launches of one step / one act call on `stream` (xarm_k_td3.hip); returns the launches' hipError_t
int launch_update(const Dev &d, void *stream);
int launch_act(const Dev &d, void *stream);
#endif

}  // namespace xtd3
