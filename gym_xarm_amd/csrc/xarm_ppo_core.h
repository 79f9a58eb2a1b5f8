// xarm_ppo_core.h - device-resident PPO update: one call is one PPO.train() of stable-baselines3 on the stored rollout -
// GAE(lambda) from the values at call start, n_epochs passes over shuffled minibatches, the per-minibatch advantage normalisation, the
// clipped surrogate, the backward of both towers of ActorCritic, torch's clip_grad_norm_ and torch's Adam - stream-ordered on the
// module's own parameter tensors.  The kernels are in xarm_k_ppo.hip; like xarm_a2c_core.h, whose rows, flat order, reduction and clip
// this reuses, it also compiles for the host (g++ -DXARM_HOST_BUILD -ffp-contract=off, tests/hostbuild_ppo/) for the CPU tests.
// adv, ret and the call-start old_logp come from the policy kernel's bits and are equal between the two builds bit for bit; the sums
// over rows are not (each build is repeatable): the device adds a workgroup's rows in float32 and the workgroups' partials in float64
// in workgroup order, the host adds chunks of 64 minibatch positions in float32 and the chunks in float64.
//
//   rows       n = k E + e as in xarm_a2c_core.h; N = T E
//   call start v_k = value(obs_k), v_T = value(last_obs), mean_k: the policy kernel.  old_logp = pi_row's logp of the stored action
//              under those weights, unless the caller hands one in
//   GAE        keep = done_k != 0 ? 0 : 1; delta = fmaf(gamma keep, v_k+1, r_k) - v_k; adv_k = fmaf((gamma lambda) keep, adv_k+1, delta),
//              adv_T = 0; ret_k = adv_k + v_k
//   steps      S = n_epochs M, M = ceil(N / B), B = min(batch_size, N).  Step s = epoch M + m takes the rows
//              perm[epoch][m B .. min((m + 1) B, N)); an entry outside [0, N) is a row with use = 0 and nothing is read through it
//   normalise  per step over its used rows, float64 in position order: n = sum use, mu = sum adv use / n,
//              sigma = sqrt(sum (adv - mu)^2 use / (n - 1)), A^ = (float)((adv - mu) / (sigma + 1e-8)); A^ = adv when n <= 1 or off
//   head       rho = exp_f(logp - old_logp); clipped = (A^ >= 0 and rho > 1 + eps) or (A^ < 0 and rho < 1 - eps);
//              q = clipped ? 0 : -((A^ rho) use); from q on pi_row's deltas (dmean_c = q d_c iv_c, log_std_c: q (d_c d_c iv_c - 1));
//              dvalue = 2 vf_coef ((value - ret) use); mean and value under the weights of the step
//   gradient   g = (float)(sum / n_use), n_use = max(n, 1); log_std: - ent_coef on top; clip as in A2C
//   Adam       t = ++step; xopt::adam_scalars and xopt::adam (xarm_opt_core.h)
//   options    (xarm_ppo_options; both off: every launch, grid and bit as without them)
//              clip_range_vf: value_terms() below, against the row's call-start value v0
//              target_kl: kl_trips() on the float32 approx_kl of the step's stats row.  The workspace holds one int, `stop`: 0, or
//              1 + the step that tripped.  The call-start launch clears it, the step's reduce sets it, and with stop != 0 the launches
//              of every later step (stopped_before) and the apply launch of the tripping step itself (stopped_at) return after one read
//              of it; a stopped step's reduce writes the stats row stopped_row() first.  `step` advances by the applied steps
#pragma once
#include <stdint.h>
#if !defined(__HIPCC__) || defined(XARM_HOST_BUILD)
#include <vector>
#endif
#include "xarm_a2c_core.h"

namespace xppo {

using xa2c::NTENS;
using xa2c::ROWS;
using xpol::fma32;
using xpol::HID;
using xpol::MAX_ACT;
using xpol::Tower;

constexpr int MAX_STEPS = 4096;     // optimiser steps per call
constexpr int NSCAL = 24;           // per-(tower, group) scalars (double): 0 surrogate, 1 value loss, 2 use, 3..18 log_std, 19 kl, 20 clipped
constexpr int NMS = 4;              // per-step doubles of the advantage statistics: mu, sigma, normalise (0 / 1), n
constexpr int RED = xa2c::RED;

struct Shape {
    xa2c::Shape a;                  // E, N, P, T, D, A, off, pstride, NB as in A2C; tiles and G: of one full minibatch
    int64_t B, M, S;
    int n_epochs;
};

struct Hyper {
    float gamma, gl, clip_lo, clip_hi, clip, vf2, max_norm;
    xopt::Adam adam;
    double ent_coef;
    int normalize;
    float vclip;                    // (float)clip_range_vf; 0: off
    double kl_limit;                // 1.5 target_kl; 0: off
};

// byte offsets of the parts of the workspace (each 16-byte aligned)
struct Work {
    int64_t boot, mean, env, value, adv, ret, oldlp, musig, partial, scal, grad, normpart, adam, total;
};

inline xarm_a2c_layout a2c_layout_of(const xarm_ppo_layout *l) {
    const xarm_a2c_layout a = {l->num_envs, l->n_steps, l->obs_dim, l->act_dim, l->hidden};
    return a;
}

inline const char *layout_error(const xarm_ppo_layout *l) {
    if (!l) return "layout is NULL";
    const xarm_a2c_layout a = a2c_layout_of(l);
    if (const char *why = xa2c::layout_error(&a)) return why;
    if (l->n_epochs < 1) return "n_epochs must be >= 1";
    if (l->batch_size < 1) return "batch_size must be >= 1";
    const int64_t N = (int64_t)l->n_steps * l->num_envs;
    const int64_t M = N > 0 ? (N + l->batch_size - 1) / l->batch_size : 0;
    if ((int64_t)l->n_epochs * M > MAX_STEPS) return "n_epochs * ceil(n_steps * num_envs / batch_size) must be <= 4096";
    return nullptr;
}

inline const char *params_error(const xarm_ppo_params *p) {
    if (!p) return "params is NULL";
    if (!(p->gamma >= 0.0 && p->gamma <= 1.0)) return "gamma must lie in [0, 1]";
    if (!(p->gae_lambda >= 0.0 && p->gae_lambda <= 1.0)) return "gae_lambda must lie in [0, 1]";
    if (!(p->clip_range > 0.0) || !(p->clip_range < 1e300)) return "clip_range must be finite and > 0";
    if (const char *why = xopt::adam_error(p->lr, p->beta1, p->beta2, p->eps)) return why;
    if (!(p->max_grad_norm > 0.0)) return "max_grad_norm must be > 0";
    if (!(p->vf_coef > -1e300 && p->vf_coef < 1e300) || !(p->ent_coef > -1e300 && p->ent_coef < 1e300)) return "vf_coef and ent_coef must be finite";
    return nullptr;
}

// the pointers a call with num_envs > 0 reads or writes; null when all are there
inline const char *pointer_error(const xarm_ppo_layout *l, const xarm_policy_weights *w, const xarm_policy_weights *m, const xarm_policy_weights *v,
                                 const int64_t *step, const float *obs, const float *action, const float *reward, const float *done,
                                 const float *last_obs, const int32_t *perm, const void *workspace) {
    if (!w) return "weights is NULL";
    if (!m || !v) return "exp_avg / exp_avg_sq is NULL";
    const xarm_a2c_layout a = a2c_layout_of(l);
    if (const char *why = xa2c::pointer_error(&a, w, w, obs, action, reward, done, last_obs, workspace)) return why;
    float *t[NTENS];
    xa2c::tensors_of(m, t);
    for (int i = 0; i < NTENS; i++)
        if (!t[i]) return "NULL exp_avg pointer";
    xa2c::tensors_of(v, t);
    for (int i = 0; i < NTENS; i++)
        if (!t[i]) return "NULL exp_avg_sq pointer";
    if (!step) return "step_i64 is NULL";
    if (!perm) return "perm is NULL";
    return nullptr;
}

inline void fill_shape(Shape &s, const xarm_ppo_layout *l) {
    const xarm_a2c_layout a = a2c_layout_of(l);
    xa2c::fill_shape(s.a, &a);
    s.n_epochs = l->n_epochs;
    s.B = l->batch_size < s.a.N ? l->batch_size : s.a.N;
    s.M = s.a.N > 0 ? (s.a.N + s.B - 1) / s.B : 0;
    s.S = s.n_epochs * s.M;
    s.a.tiles = (s.B + ROWS - 1) / ROWS;
    s.a.G = (int)(s.a.tiles < xa2c::MAX_GROUPS ? s.a.tiles : xa2c::MAX_GROUPS);
}

inline const char *options_error(const xarm_ppo_options *o) {
    if (!o) return nullptr;
    if (!(o->clip_range_vf >= 0.0) || !(o->clip_range_vf < 1e300)) return "clip_range_vf must be finite and >= 0 (0 = off)";
    if (!(o->target_kl >= 0.0) || !(o->target_kl < 1e300)) return "target_kl must be finite and >= 0 (0 = off)";
    return nullptr;
}

inline void fill_hyper(Hyper &h, const xarm_ppo_params *p, const xarm_ppo_options *o = nullptr) {
    h.gamma = (float)p->gamma; h.gl = (float)(p->gamma * p->gae_lambda);
    h.clip = (float)p->clip_range; h.clip_lo = (float)(1.0 - p->clip_range); h.clip_hi = (float)(1.0 + p->clip_range);
    xopt::fill_adam(h.adam, p->lr, p->beta1, p->beta2, p->eps);
    h.vf2 = (float)(2.0 * p->vf_coef); h.max_norm = (float)p->max_grad_norm; h.ent_coef = p->ent_coef; h.normalize = p->normalize_advantage != 0;
    h.vclip = o ? (float)o->clip_range_vf : 0.0f;
    h.kl_limit = o ? 1.5 * o->target_kl : 0.0;
}

inline void fill_work(Work &k, const Shape &s) {
    int64_t at = 0;
    auto take = [&at](int64_t bytes) { const int64_t o = at; at += (bytes + 15) & ~(int64_t)15; return o; };
    const xa2c::Shape &a = s.a;
    k.boot = take(a.E * 4);
    k.mean = take(a.N * a.A * 4);
    k.env = take(a.N * a.A * 4);
    k.value = take(a.N * 4);
    k.adv = take(a.N * 4);
    k.ret = take(a.N * 4);
    k.oldlp = take(a.N * 4);
    k.musig = take(s.S * NMS * 8);
    k.partial = take(2 * (int64_t)a.G * a.pstride * 4);
    k.scal = take(2 * (int64_t)a.G * NSCAL * 8);
    k.grad = take(a.P * 4);
    k.normpart = take((int64_t)a.NB * 8);
    k.adam = take(16);              // Adam's two scalars; the third word is the KL stop's flag
    k.total = at;
}

// -------------------------------------------------------------------------------------------------- the row's and the parameter's parts
// one step of the GAE recursion: next_value = v_k+1, next_adv = adv_k+1; returns adv_k
XARM_HD float gae_step(float gamma, float gl, float done, float reward, float value, float next_value, float next_adv) {
    const float keep = done != 0.0f ? 0.0f : 1.0f;
    const float delta = fma32(gamma * keep, next_value, reward) - value;
    return fma32(gl * keep, next_adv, delta);
}

// where step s's rows lie in perm (position of its first entry, number of entries)
XARM_HD void step_span(const Shape &s, int64_t step, int64_t &first, int64_t &count) {
    const int64_t epoch = step / s.M, m = step - epoch * s.M, p0 = m * s.B;
    first = epoch * s.a.N + p0;
    count = s.a.N - p0 < s.B ? s.a.N - p0 : s.B;
}

// the batch row of a perm entry, -1 for an entry outside [0, N)
XARM_HD int64_t row_of(int32_t entry, int64_t N) { return (entry >= 0 && (int64_t)entry < N) ? (int64_t)entry : -1; }

XARM_HD float norm_adv(float adv, const double *ms) {
    return ms[2] != 0.0 ? (float)(((double)adv - ms[0]) / (ms[1] + 1e-8)) : adv;
}

// mu, sigma, normalise, n of a step from its two sums
XARM_HD void finish_stats(double *ms, double n, double mu, double sumsq, int normalize) {
    ms[0] = mu;
    ms[1] = n > 1.0 ? __builtin_sqrt(sumsq / (n - 1.0)) : 0.0;
    ms[2] = (normalize && n > 1.0) ? 1.0 : 0.0;
    ms[3] = n;
}

struct RowTerms {
    float q, surr, kl, clipped;     // dlogp's factor, min(rho A^, clamp(rho) A^) use, ((rho - 1) - log rho) use, [|rho - 1| > eps] use
};

XARM_HD RowTerms surrogate(const Hyper &h, float ahat, float logp, float old_logp, float use) {
    const float lr = logp - old_logp;
    const float rho = xpol::exp_f(lr);
    const bool clipped = (ahat >= 0.0f && rho > h.clip_hi) || (ahat < 0.0f && rho < h.clip_lo);
    const float ra = ahat * rho;
    const float rc = rho < h.clip_lo ? h.clip_lo : (rho > h.clip_hi ? h.clip_hi : rho);
    const float ca = rc * ahat;
    const float rm1 = rho - 1.0f;
    RowTerms t;
    t.q = clipped ? 0.0f : -(ra * use);
    t.surr = (ra < ca ? ra : ca) * use;
    t.kl = (rm1 - lr) * use;
    t.clipped = (__builtin_fabsf(rm1) > h.clip ? 1.0f : 0.0f) * use;
    return t;
}

// the value head of a row: its output delta and its term of the value loss.  v: the value under the step's weights, v0: at call start (read
// only with clip_range_vf on).  Inside the range the terms are those of the update without the option, from v itself.  ON = false: for a
// kernel instantiated for calls with the option off (the wide head: its row loop then stays the one basic block it was)
struct ValueTerms {
    float dvalue, loss;
};

template <bool ON = true> XARM_HD ValueTerms value_terms(const Hyper &h, float v, float v0, float ret, float use) {
    ValueTerms t;
    t.dvalue = xa2c::value_delta(h.vf2, v, ret, use);
    t.loss = (ret - v) * (ret - v) * use;
    if (ON && h.vclip > 0.0f && !(__builtin_fabsf(v - v0) <= h.vclip)) {
        const float vp = v > v0 ? v0 + h.vclip : v0 - h.vclip;
        t.dvalue = 0.0f;
        t.loss = (ret - vp) * (ret - vp) * use;
    }
    return t;
}

// the KL stop.  kl: the float32 approx_kl of the step's stats row
XARM_HD bool kl_trips(const Hyper &h, float kl) { return h.kl_limit > 0.0 && (double)kl > h.kl_limit; }
// stop: the workspace's flag, 0 or 1 + the step that tripped.  A launch reads it only with target_kl on
XARM_HD bool stopped_before(const Hyper &h, const int *stop, int64_t st) {
    if (!(h.kl_limit > 0.0)) return false;
    const int f = stop[0];
    return f != 0 && (int64_t)f <= st;
}
XARM_HD bool stopped_at(const Hyper &h, const int *stop) { return h.kl_limit > 0.0 && stop[0] != 0; }
// the stats row of a step behind the one that tripped
XARM_HD void stopped_row(float *o) {
    for (int k = 0; k < 7; k++) o[k] = 0.0f;
    o[7] = 1.0f;
}

#if !defined(__HIPCC__) || defined(XARM_HOST_BUILD)
// ---- the whole update as plain loops (the host build).  w / m / v: the 13 tensors.  out_old_logp [N] (host build only): the call-start
// log-probabilities in use.
inline void host_update(const Shape &s, const Hyper &h, float *const *w, float *const *m, float *const *v, int64_t *step, const float *obs,
                        const float *action, const float *reward, const float *done, const float *use, const float *last_obs, const float *old_logp,
                        const int32_t *perm, float *out_adv, float *out_returns, float *out_grad, float *out_stats, float *out_old_logp) {
    const Tower pi = {w[0], w[1], w[2], w[3], w[4], w[5]}, vf = {w[6], w[7], w[8], w[9], w[10], w[11]};
    const float *log_std = w[12];
    const xa2c::Shape &a = s.a;
    const int D = a.D, A = a.A;
    const int64_t N = a.N;
    std::vector<float> val((size_t)N), adv((size_t)N), ret((size_t)N), olp((size_t)N);
    float nodls[MAX_ACT] = {0.0f};
    for (int64_t n = 0; n < N; n++) {
        float mean[MAX_ACT];
        xpol::tower_row(vf, obs + n * D, D, 1, &val[(size_t)n]);
        if (old_logp) { olp[(size_t)n] = old_logp[n]; continue; }
        xpol::tower_row(pi, obs + n * D, D, A, mean);
        olp[(size_t)n] = xa2c::pi_row<false>(A, mean, 1, action + n * A, log_std, 0.0f, nullptr, 0, nodls);
    }
    for (int64_t e = 0; e < a.E; e++) {
        float nv, na = 0.0f;
        xpol::tower_row(vf, last_obs + e * D, D, 1, &nv);
        for (int k = a.T - 1; k >= 0; k--) {
            const int64_t n = (int64_t)k * a.E + e;
            na = gae_step(h.gamma, h.gl, done[n], reward[n], val[(size_t)n], nv, na);
            nv = val[(size_t)n];
            adv[(size_t)n] = na;
            ret[(size_t)n] = na + nv;
        }
    }
    for (int64_t n = 0; n < N; n++) {
        if (out_adv) out_adv[n] = adv[(size_t)n];
        if (out_returns) out_returns[n] = ret[(size_t)n];
        if (out_old_logp) out_old_logp[n] = olp[(size_t)n];
    }

    std::vector<double> G((size_t)a.P);
    std::vector<float> chunk((size_t)a.P), g((size_t)a.P);
    int stop = 0;
    for (int64_t st = 0; st < s.S; st++) {
        if (stopped_before(h, &stop, st)) {
            if (out_stats) stopped_row(out_stats + st * 8);
            continue;
        }
        int64_t first, count;
        step_span(s, st, first, count);
        double ms[NMS], n = 0.0, sa = 0.0, sv = 0.0;
        for (int64_t i = 0; i < count; i++) {
            const int64_t r = row_of(perm[first + i], N);
            if (r < 0) continue;
            const double u = use ? (double)use[r] : 1.0;
            n += u;
            sa += (double)adv[(size_t)r] * u;
        }
        const double mu = n > 0.0 ? sa / n : 0.0;
        for (int64_t i = 0; i < count; i++) {
            const int64_t r = row_of(perm[first + i], N);
            if (r < 0) continue;
            const double u = use ? (double)use[r] : 1.0, dd = (double)adv[(size_t)r] - mu;
            sv += dd * dd * u;
        }
        finish_stats(ms, n, mu, sv, h.normalize);

        for (int64_t p = 0; p < a.P; p++) { G[(size_t)p] = 0.0; chunk[(size_t)p] = 0.0f; }
        double surr = 0.0, vloss = 0.0, kl = 0.0, clipped = 0.0;
        auto flush = [&]() {
            for (int64_t p = 0; p < a.P; p++) { G[(size_t)p] += (double)chunk[(size_t)p]; chunk[(size_t)p] = 0.0f; }
        };
        for (int64_t i = 0; i < count; i++) {
            const int64_t r = row_of(perm[first + i], N);
            if (r >= 0) {
                const float *x = obs + r * D;
                float h1[HID], h2[HID], g1[HID], g2[HID], mean[MAX_ACT], val_now, d3[MAX_ACT], dls[MAX_ACT] = {0.0f};
                xpol::tower_row_keep(pi, x, D, A, h1, h2, mean);
                xpol::tower_row_keep(vf, x, D, 1, g1, g2, &val_now);
                const float u = use ? use[r] : 1.0f, rt = ret[(size_t)r];
                const float lp = xa2c::pi_row<false>(A, mean, 1, action + r * A, log_std, 0.0f, nullptr, 0, nodls);
                const RowTerms t = surrogate(h, norm_adv(adv[(size_t)r], ms), lp, olp[(size_t)r], u);
                xa2c::pi_row<true>(A, mean, 1, action + r * A, log_std, t.q, d3, 1, dls);
                for (int c = 0; c < A; c++) chunk[(size_t)a.off[12] + c] += dls[c];
                xa2c::host_backward(a, chunk.data(), pi, 0, x, h1, h2, d3, A);
                const ValueTerms vt = value_terms(h, val_now, val[(size_t)r], rt, u);
                xa2c::host_backward(a, chunk.data(), vf, 6, x, g1, g2, &vt.dvalue, 1);
                surr += (double)t.surr; kl += (double)t.kl; clipped += (double)t.clipped;
                vloss += (double)vt.loss;
            }
            if ((i + 1) % ROWS == 0 || i + 1 == count) flush();
        }
        const double n_use = xopt::n_use(n);
        double sum2 = 0.0;
        for (int64_t p = 0; p < a.P; p++) {
            double x = G[(size_t)p] / n_use;
            if (p >= a.off[12]) x -= h.ent_coef;
            g[(size_t)p] = (float)x;
            sum2 += (double)g[(size_t)p] * (double)g[(size_t)p];
        }
        const double ent = xopt::gaussian_entropy(log_std, A);
        const float norm = (float)__builtin_sqrt(sum2), coef = xopt::clip_coef(norm, h.max_norm);
        if (out_grad && st == 0)
            for (int64_t p = 0; p < a.P; p++) out_grad[p] = g[(size_t)p];
        if (out_stats) {
            float *o = out_stats + st * 8;
            o[0] = (float)(-surr / n_use); o[1] = (float)(vloss / n_use); o[2] = (float)ent; o[3] = norm; o[4] = (float)n_use;
            o[5] = (float)(kl / n_use); o[6] = (float)(clipped / n_use); o[7] = 0.0f;
        }
        if (kl_trips(h, (float)(kl / n_use))) {
            stop = (int)st + 1;
            if (out_stats) { out_stats[st * 8 + 3] = 0.0f; out_stats[st * 8 + 7] = 1.0f; }
            continue;
        }
        step[0] += 1;
        float sc[2];
        xopt::adam_scalars(h.adam, step[0], sc);
        for (int i = 0; i < NTENS; i++)
            for (int64_t p = a.off[i]; p < a.off[i + 1]; p++)
                xopt::adam(h.adam, sc, g[(size_t)p] * coef, m[i][p - a.off[i]], v[i][p - a.off[i]], w[i][p - a.off[i]]);
    }
}
#endif

#if defined(__HIPCC__) && !defined(XARM_HOST_BUILD)
struct Dev {
    Shape s;
    Hyper h;
    Tower pi, vf;
    float *w[NTENS], *m[NTENS], *v[NTENS];
    int64_t *step;
    const float *obs, *action, *reward, *done, *use, *last_obs, *old_logp;
    const int32_t *perm;
    float *boot, *mean, *env, *value, *adv, *ret, *oldlp, *partial, *grad, *adam;
    int *stop;                      // the KL stop's flag (adam + 2)
    double *musig, *scal, *normpart;
    float *out_adv, *out_returns, *out_grad, *out_stats;
};
constexpr int FIXED_LAUNCHES = 4, LAUNCHES_PER_STEP = 3;   // two policy calls, GAE + old_logp, the advantage statistics; grad, reduce, apply
// the 4 + 3 S launches of one update on `stream` (xarm_k_ppo.hip); returns the launches' hipError_t
int launch_update(const Dev &d, void *stream);
#endif

}  // namespace xppo
