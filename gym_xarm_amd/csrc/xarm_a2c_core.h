// xarm_a2c_core.h - device-resident A2C update: the update block of gym_xarm_amd/train.py - bootstrap value, n-step
// returns, the backward of both towers of ActorCritic, torch's clip_grad_norm_ and torch's RMSprop - as one stream-ordered call on
// the module's own parameter tensors.  The kernels are in xarm_k_a2c.hip; like xarm_policy_core.h this also compiles for the host
// (g++ -DXARM_HOST_BUILD -ffp-contract=off, tests/hostbuild_a2c/) for the CPU tests.  The forward is the policy's: the chains of
// xarm_policy_core.h (layer1_chains / hidden_chains, tanh_f, exp_f), so value, mean, h1 and h2 of a row are the bits the policy
// kernel computes, and so are the returns.  The sums over rows are NOT specified bit for bit between the two builds (each build is
// repeatable): the device adds a workgroup's rows in float32 and the workgroups' partials in float64 in workgroup order, the host
// adds chunks of 64 rows in float32 and the chunks in float64.
//
//   rows      n = k E + e, k < T = n_steps, e < E = num_envs: obs [N, D], action [N, A], reward / done / use [N]; last_obs [E, D]
//   returns   ret_T = value(last_obs); ret_k = fmaf(gamma keep_k, ret_k+1, reward_k), keep_k = 0 where done_k != 0, else 1
//   row       adv = ret - value; with d_c = a_c - mean_c, iv_c = exp(-2 log_std_c), q = -(adv use):
//             dmean_c = q d_c iv_c, the log_std_c term q (d_c (d_c iv_c) - 1), dvalue = 2 vf_coef ((value - ret) use),
//             logp = sum_c ((-0.5 d_c (d_c iv_c) - log_std_c) - log(2 pi) / 2)
//   backward  d2 = (W3^T d3) (1 - h2^2), d1 = (W2^T d2) (1 - h1^2); dW = sum_rows d (x) input, db = sum_rows d
//   flat      the 13 tensors one after the other in xarm_policy_weights' order: P floats
//   gradient  g = (float)(sum / n_use), n_use = max(sum use, 1); log_std: - ent_coef on top
//   clip      norm = (float) sqrt(sum (double) g^2); then xopt::clip_coef and xopt::rmsprop (xarm_opt_core.h)
#pragma once
#include <stdint.h>
#if !defined(__HIPCC__) || defined(XARM_HOST_BUILD)
#include <vector>
#endif
#include "xarm_policy_core.h"
#include "xarm_opt_core.h"

namespace xa2c {

using xpol::fma32;
using xpol::HID;
using xpol::MAX_ACT;
using xpol::Tower;

constexpr int ROWS = 64;            // rows per tile of the gradient kernel (and per float32 chunk of the host build)
constexpr int MAX_GROUPS = 256;     // workgroups per tower of the gradient kernel; tile i belongs to group i % groups
constexpr int NTENS = 13;
constexpr int NSCAL = 20;           // per-group scalars (double): sum adv logp use, sum (ret - value)^2 use, sum use, 16 log_std sums, 0
constexpr int RED = 256;            // threads per block of the reduce / apply kernels: one flat parameter each
constexpr float HALF_LOG_2PI = 0.918938533204672742f;

struct Shape {
    int64_t E, N, P, tiles, pstride;
    int T, D, A, G, NB;
    int64_t off[NTENS + 1];         // where tensor i starts in the flat gradient
};

struct Hyper {
    float gamma, vf2, max_norm;
    xopt::RmsProp rms;
    double ent_coef;
};

// byte offsets of the parts of the workspace (each 16-byte aligned)
struct Work {
    int64_t boot, mean, env, value, ret, partial, scal, grad, normpart, total;
};

inline const char *layout_error(const xarm_a2c_layout *l) {
    if (!l) return "layout is NULL";
    if (l->num_envs < 0) return "num_envs must be >= 0";
    if (l->n_steps < 1) return "n_steps must be >= 1";
    if ((int64_t)l->n_steps * (int64_t)l->num_envs >= ((int64_t)1 << 31)) return "n_steps * num_envs must be < 2^31";
    if (l->obs_dim < 1 || l->obs_dim > xpol::MAX_DIM) return "obs_dim must lie in [1, XARM_POLICY_MAX_DIM (96)]";
    if (l->act_dim < 1 || l->act_dim > MAX_ACT) return "act_dim must lie in [1, XARM_POLICY_MAX_ACT (16)]";
    if (l->hidden != HID) return "hidden must be XARM_POLICY_HIDDEN (64)";
    return nullptr;
}

inline const char *params_error(const xarm_a2c_params *p) {
    if (!p) return "params is NULL";
    if (!(p->gamma >= 0.0 && p->gamma <= 1.0)) return "gamma must lie in [0, 1]";
    if (!(p->lr >= 0.0) || !(p->lr < 1e300)) return "lr must be finite and >= 0";
    if (!(p->alpha >= 0.0 && p->alpha < 1.0)) return "alpha must lie in [0, 1)";
    if (!(p->eps > 0.0) || !(p->eps < 1e300)) return "eps must be finite and > 0";
    if (!(p->max_grad_norm > 0.0)) return "max_grad_norm must be > 0";
    if (!(p->vf_coef > -1e300 && p->vf_coef < 1e300) || !(p->ent_coef > -1e300 && p->ent_coef < 1e300)) return "vf_coef and ent_coef must be finite";
    return nullptr;
}

inline void tensors_of(const xarm_policy_weights *w, float *(&t)[NTENS]) {
    const float *c[NTENS] = {w->pi_w1, w->pi_b1, w->pi_w2, w->pi_b2, w->pi_w3, w->pi_b3, w->vf_w1, w->vf_b1, w->vf_w2, w->vf_b2, w->vf_w3, w->vf_b3, w->log_std};
    for (int i = 0; i < NTENS; i++) t[i] = const_cast<float *>(c[i]);
}

// the pointers a call with num_envs > 0 reads or writes; null when all are there
inline const char *pointer_error(const xarm_a2c_layout *l, const xarm_policy_weights *w, const xarm_policy_weights *sq, const float *obs,
                                 const float *action, const float *reward, const float *done, const float *last_obs, const void *workspace) {
    if (!w) return "weights is NULL";
    if (!sq) return "square_avg is NULL";
    const xarm_policy_layout pl = {l->num_envs, l->obs_dim, 0, l->act_dim, l->hidden, 0};
    const xarm_policy_params pp = {0, 10.0, 1e-8, 1};
    // the policy's own rules for the weights (all 13 present, b1 / W2 / b2 / W3 16-byte aligned) with the value tower in use
    if (const char *why = xpol::pointer_error(&pl, &pp, w, nullptr, obs, nullptr, nullptr, obs, obs, obs)) return why;
    float *t[NTENS];
    tensors_of(sq, t);
    for (int i = 0; i < NTENS; i++)
        if (!t[i]) return "NULL square_avg pointer";
    if (!action || !reward || !done || !last_obs) return "NULL action / reward / done / last_obs";
    if (!workspace) return "workspace is NULL";
    if (((uintptr_t)workspace & 15u) != 0) return "workspace must be 16-byte aligned";
    return nullptr;
}

inline void fill_shape(Shape &s, const xarm_a2c_layout *l) {
    s.E = l->num_envs; s.T = l->n_steps; s.D = l->obs_dim; s.A = l->act_dim; s.N = s.E * s.T;
    const int64_t n[NTENS] = {HID * s.D, HID, HID * HID, HID, HID * s.A, s.A, HID * s.D, HID, HID * HID, HID, HID, 1, s.A};
    s.off[0] = 0;
    for (int i = 0; i < NTENS; i++) s.off[i + 1] = s.off[i] + n[i];
    s.P = s.off[NTENS];
    s.tiles = (s.N + ROWS - 1) / ROWS;
    s.G = (int)(s.tiles < MAX_GROUPS ? s.tiles : MAX_GROUPS);
    s.pstride = (s.off[6] + 3) & ~(int64_t)3;               // a group's slice holds one tower's gradient (the policy's is the larger)
    s.NB = (int)((s.P + RED - 1) / RED);
}

inline void fill_hyper(Hyper &h, const xarm_a2c_params *p) {
    h.gamma = (float)p->gamma; h.rms.lr = (float)p->lr; h.rms.alpha = (float)p->alpha; h.rms.one_m_alpha = (float)(1.0 - p->alpha);
    h.rms.eps = (float)p->eps; h.vf2 = (float)(2.0 * p->vf_coef); h.max_norm = (float)p->max_grad_norm; h.ent_coef = p->ent_coef;
}

inline void fill_work(Work &k, const Shape &s) {
    int64_t at = 0;
    auto take = [&at](int64_t bytes) { const int64_t o = at; at += (bytes + 15) & ~(int64_t)15; return o; };
    k.boot = take(s.E * 4);
    k.mean = take(s.N * s.A * 4);
    k.env = take(s.N * s.A * 4);
    k.value = take(s.N * 4);
    k.ret = take(s.N * 4);
    k.partial = take(2 * (int64_t)s.G * s.pstride * 4);
    k.scal = take((int64_t)s.G * NSCAL * 8);
    k.grad = take(s.P * 4);
    k.normpart = take((int64_t)s.NB * 8);
    k.total = at;
}

// -------------------------------------------------------------------------------------------------- the row's and the parameter's parts
XARM_HD float return_step(float gamma, float done, float reward, float next) {
    const float keep = done != 0.0f ? 0.0f : 1.0f;
    return fma32(gamma * keep, next, reward);
}

// the policy head of one row with dlogp's factor q given: mean_c at mean[c * ms]; DELTAS: dmean[c * ds] = q d_c iv_c for c < A (mean and dmean
// may be the same memory) and the row's log_std terms added to dls; returns logp
template <bool DELTAS> XARM_HD float pi_row(int A, const float *mean, int ms, const float *action, const float *log_std, float q, float *dmean, int ds,
                                            float (&dls)[MAX_ACT]) {
    float lp = 0.0f;
#pragma unroll
    for (int c = 0; c < MAX_ACT; c++) {
        if (c < A) {
            const float ls = log_std[c];
            const float iv = xpol::exp_f(-2.0f * ls);
            const float d = action[c] - mean[c * ms];
            const float dv = d * iv;
            if (DELTAS) {
                dmean[c * ds] = q * dv;
                const float t = fma32(d, dv, -1.0f);
                dls[c] = fma32(q, t, dls[c]);
            }
            float l = -0.5f * d;
            l = l * dv;
            l = l - ls;
            l = l - HALF_LOG_2PI;
            lp = c == 0 ? l : lp + l;
        }
    }
    return lp;
}

// A2C's head: q = -(adv use)
XARM_HD float pi_deltas(int A, const float *mean, const float *action, const float *log_std, float adv, float use, float *dmean, int ds,
                        float (&dls)[MAX_ACT]) {
    return pi_row<true>(A, mean, 1, action, log_std, -(adv * use), dmean, ds, dls);
}

XARM_HD float value_delta(float vf2, float value, float ret, float use) { return vf2 * ((value - ret) * use); }

#if !defined(__HIPCC__) || defined(XARM_HOST_BUILD)
// one row's backward through one tower (tensors t0 .. t0 + 5 of the flat order), added to the float32 chunk sums
inline void host_backward(const Shape &s, float *chunk, const Tower &T, int t0, const float *x, const float *h1, const float *h2, const float *d3, int nout) {
    const int D = s.D;
    float *gW1 = chunk + s.off[t0], *gb1 = chunk + s.off[t0 + 1], *gW2 = chunk + s.off[t0 + 2], *gb2 = chunk + s.off[t0 + 3],
          *gW3 = chunk + s.off[t0 + 4], *gb3 = chunk + s.off[t0 + 5];
    float d2[HID], d1[HID];
    for (int c = 0; c < nout; c++) {
        for (int j = 0; j < HID; j++) gW3[c * HID + j] = fma32(d3[c], h2[j], gW3[c * HID + j]);
        gb3[c] += d3[c];
    }
    for (int j = 0; j < HID; j++) {
        float pre = 0.0f;
        for (int c = 0; c < nout; c++) pre = fma32(T.W3[c * HID + j], d3[c], pre);
        d2[j] = pre * fma32(-h2[j], h2[j], 1.0f);
    }
    for (int i = 0; i < HID; i++) {
        for (int j = 0; j < HID; j++) gW2[i * HID + j] = fma32(d2[i], h1[j], gW2[i * HID + j]);
        gb2[i] += d2[i];
    }
    for (int j = 0; j < HID; j++) {
        float pre = 0.0f;
        for (int k = 0; k < HID; k++) pre = fma32(T.W2[k * HID + j], d2[k], pre);
        d1[j] = pre * fma32(-h1[j], h1[j], 1.0f);
    }
    for (int i = 0; i < HID; i++) {
        for (int j = 0; j < D; j++) gW1[i * D + j] = fma32(d1[i], x[j], gW1[i * D + j]);
        gb1[i] += d1[i];
    }
}

// ---- the whole update as plain loops (the host build).  w / sq: the 13 tensors.
inline void host_update(const Shape &s, const Hyper &h, float *const *w, float *const *sq, const float *obs, const float *action, const float *reward,
                        const float *done, const float *use, const float *last_obs, float *out_returns, float *out_grad, float *out_stats) {
    const Tower pi = {w[0], w[1], w[2], w[3], w[4], w[5]}, vf = {w[6], w[7], w[8], w[9], w[10], w[11]};
    const float *log_std = w[12];
    const int D = s.D, A = s.A;
    std::vector<float> ret((size_t)s.N);
    for (int64_t e = 0; e < s.E; e++) {
        float r;
        xpol::tower_row(vf, last_obs + e * D, D, 1, &r);
        for (int k = s.T - 1; k >= 0; k--) {
            const int64_t n = (int64_t)k * s.E + e;
            r = return_step(h.gamma, done[n], reward[n], r);
            ret[(size_t)n] = r;
        }
    }
    if (out_returns)
        for (int64_t n = 0; n < s.N; n++) out_returns[n] = ret[(size_t)n];

    std::vector<double> G((size_t)s.P, 0.0);
    std::vector<float> chunk((size_t)s.P, 0.0f);
    double ploss = 0.0, vloss = 0.0, nuse = 0.0;
    auto flush = [&]() {
        for (int64_t p = 0; p < s.P; p++) { G[(size_t)p] += (double)chunk[(size_t)p]; chunk[(size_t)p] = 0.0f; }
    };
    auto backward = [&](const Tower &T, int t0, const float *x, const float *h1, const float *h2, const float *d3, int nout) {
        host_backward(s, chunk.data(), T, t0, x, h1, h2, d3, nout);
    };
    for (int64_t n = 0; n < s.N; n++) {
        const float *x = obs + n * D;
        float h1[HID], h2[HID], g1[HID], g2[HID], mean[MAX_ACT], v, d3[MAX_ACT], dls[MAX_ACT] = {0.0f};
        xpol::tower_row_keep(pi, x, D, A, h1, h2, mean);
        xpol::tower_row_keep(vf, x, D, 1, g1, g2, &v);
        const float u = use ? use[n] : 1.0f, r = ret[(size_t)n], adv = r - v;
        const float lp = pi_deltas(A, mean, action + n * A, log_std, adv, u, d3, 1, dls);
        for (int c = 0; c < A; c++) chunk[(size_t)s.off[12] + c] += dls[c];
        backward(pi, 0, x, h1, h2, d3, A);
        const float dv = value_delta(h.vf2, v, r, u);
        backward(vf, 6, x, g1, g2, &dv, 1);
        ploss += (double)(adv * lp * u);
        vloss += (double)((r - v) * (r - v) * u);
        nuse += (double)u;
        if ((n + 1) % ROWS == 0 || n + 1 == s.N) flush();
    }
    const double n_use = xopt::n_use(nuse);
    std::vector<float> g((size_t)s.P);
    double sum2 = 0.0;
    for (int64_t p = 0; p < s.P; p++) {
        double v = G[(size_t)p] / n_use;
        if (p >= s.off[12]) v -= h.ent_coef;
        g[(size_t)p] = (float)v;
        sum2 += (double)g[(size_t)p] * (double)g[(size_t)p];
    }
    const double ent = xopt::gaussian_entropy(log_std, A);
    const float norm = (float)__builtin_sqrt(sum2), coef = xopt::clip_coef(norm, h.max_norm);
    if (out_grad)
        for (int64_t p = 0; p < s.P; p++) out_grad[p] = g[(size_t)p];
    if (out_stats) {
        for (int i = 0; i < 8; i++) out_stats[i] = 0.0f;
        out_stats[0] = (float)(-ploss / n_use); out_stats[1] = (float)(vloss / n_use); out_stats[2] = (float)ent; out_stats[3] = norm;
        out_stats[4] = (float)n_use;
    }
    for (int i = 0; i < NTENS; i++)
        for (int64_t p = s.off[i]; p < s.off[i + 1]; p++) xopt::rmsprop(h.rms, g[(size_t)p] * coef, sq[i][p - s.off[i]], w[i][p - s.off[i]]);
}
#endif

#if defined(__HIPCC__) && !defined(XARM_HOST_BUILD)
struct Dev {
    Shape s;
    Hyper h;
    Tower pi, vf;
    float *w[NTENS], *sq[NTENS];
    const float *obs, *action, *reward, *done, *use, *last_obs;
    float *boot, *mean, *env, *value, *ret, *partial, *grad;
    double *scal, *normpart;
    float *out_returns, *out_grad, *out_stats;
};
// the six launches of one update on `stream` (xarm_k_a2c.hip); returns the launches' hipError_t
int launch_update(const Dev &d, void *stream);
#endif

}  // namespace xa2c
