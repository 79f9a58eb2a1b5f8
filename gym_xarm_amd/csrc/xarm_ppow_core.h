// xarm_ppow_core.h - wide device-resident PPO update: the update of xarm_ppo_core.h for train.py's
// ActorCritic(net_arch, activation) with equal-width towers of two or three hidden layers of 64, 128, 192 or 256 units, tanh or ReLU.
// As in the wide SAC (xarm_sacw_core.h) a step is a CHAIN of per-layer GEMM launches with the activations in the
// workspace.  This file states the chain (run_update) and every per-row and per-parameter function ONCE; xarm_k_ppow.hip executes them
// on the device, the host build (g++ -DXARM_HOST_BUILD -ffp-contract=off, tests/hostbuild_ppow/) with plain loops over the same
// workspace: everything the call writes - rows, gradient, stats, parameters, the workspace - is equal between them bit for bit.
//
// Called, not copied: the GEMM jobs, passes, row ranges and activation of xarm_sacw_core.h; gae_step, step_span, row_of, norm_adv,
// finish_stats and surrogate of xarm_ppo_core.h; pi_row and value_delta of xarm_a2c_core.h; slice_sum, n_use, gaussian_entropy,
// clip_coef, tensor_at, adam_scalars and adam of xarm_opt_core.h.
//
//   flat order   pi's 2 (L + 1) tensors W1, b1, ..., W_out, b_out, vf's, log_std: NT = 4 (L + 1) + 1 tensors, P parameters
//   call start   under the weights as the call finds them: the forward of vf and pi over the N rollout rows in chunks of at most B rows
//                through the step's own activation buffers (only mean [N, A] and value [N + E] are kept; with old_logp given the pi job
//                is left out), then vf over last_obs in chunks of its OWN launches (Fwd carries one row count for its jobs) into
//                value[N ..]; one launch per row for GAE and old_logp; one launch for all S advantage statistics
//   step s       gather: position i of the step's span of perm -> row i of x, action, A^, ret, old_logp, use (an entry outside [0, N)
//                and the pad behind a short last minibatch: a zero row with use = 0; nothing is read through it) | L + 1 forward
//                launches, two jobs | head (one workgroup): logp, surrogate, both towers' output deltas, log_std's terms, the sums |
//                L delta launches | one weight-gradient launch | reduce | apply
//   sums         over rows: thread t of 256 walks rows t, t + 256, ... in float64, the 256 partials are added in t order.  Over a
//                gradient's rows: sacw's - float32 fmaf chains within one of at most 16 ranges of whole 64-row tiles, the ranges
//                added in float64 in range order, / n_use, rounded once.  The squares of a block of 256 parameters: a fixed tree.
//   options      xarm_ppo_core.h's, through its functions.  clip_range_vf: the gather carries value[r] as one more column, gv0, which
//                lies in dOvf (written by the gather, read and then overwritten by the head of the same row: no workspace is added).
//                target_kl: the stop flag is the third word of adam; gae's row 0 clears it, finish_step sets it, and the gather, head,
//                reduce and apply of a stopped step return on it.  So do the step's GEMM launches, through the job header's gate
//                (xsacw::Gate; null with target_kl off and for every other user of the GEMM kernels): ungated, an update stopped at
//                step 1 of 16 still cost 13.6 of 17.4 ms at 65 536 rows of [256, 256, 256]
#pragma once
#include "xarm_ppo_core.h"
#include "xarm_sacw_core.h"

namespace xppow {

using xpol::MAX_ACT;
using xppo::NMS;
using xppo::NSCAL;
using xsacw::TP;

constexpr int MAX_NT = 2 * TP + 1;
constexpr int RED = xsacw::RED;
static_assert(MAX_NT <= xsacw::MAX_NT, "the flat offsets fit xsacw::Shape");

struct Dev {
    xsacw::Shape g;                 // the step's GEMMs: B rows of one minibatch, D, A, H, L, NL, BH, act, tp, NT, off, P, S, rows
    xppo::Shape p;                  // a.E, a.N, a.T, a.D, a.A, a.P, a.NB; B, M, S, n_epochs
    xppo::Hyper h;
    int64_t CN, CE, Ppi, Ptow;      // call-start chunks over the rollout and over last_obs; pi's parameters, both towers'
    float *w[MAX_NT], *m[MAX_NT], *v[MAX_NT];
    int64_t *step;
    const float *obs, *action, *reward, *done, *use, *last_obs, *old_logp;
    const int32_t *perm;
    // the workspace
    float *mean, *value, *adv, *ret, *oldlp;            // per rollout row (value: N + E)
    double *musig;                                      // [S][NMS]
    float *x, *ga, *gahat, *gret, *golp, *guse;         // the step's gathered rows
    float *gv0;                                         // with clip_range_vf: the rows' call-start values (= dOvf, see above)
    int *stop;                                          // the KL stop's flag (adam + 2)
    float *hid, *dH, *outM, *outV, *dOpi, *dOvf;        // activations and deltas [2][L][B, H], the towers' outputs and output deltas
    float *partial;                                     // [ranges][Ptow]
    double *scal, *normpart;                            // the step's NSCAL sums; a block's sum of squares
    float *grad, *adam;
    float *out_adv, *out_returns, *out_grad, *out_stats;
};

inline xarm_ppo_layout ppo_layout_of(const xarm_ppow_layout *l) {
    const xarm_ppo_layout p = {l->num_envs, l->n_steps, l->obs_dim, l->act_dim, xpol::HID, l->n_epochs, l->batch_size};
    return p;
}

inline const char *layout_error(const xarm_ppow_layout *l) {
    if (!l) return "layout is NULL";
    const xarm_ppo_layout p = ppo_layout_of(l);
    if (const char *why = xppo::layout_error(&p)) return why;
    if (const char *why = xsacw::towers_error(l->hidden, l->n_hidden, l->activation)) return why;
    return nullptr;
}

inline const char *pointer_error(const xarm_ppow_layout *l, const xarm_acw_weights *w, const xarm_acw_weights *m, const xarm_acw_weights *v,
                                 const int64_t *step, const float *obs, const float *action, const float *reward, const float *done,
                                 const float *last_obs, const int32_t *perm, const void *workspace) {
    if (!w) return "weights is NULL";
    if (!m || !v) return "exp_avg / exp_avg_sq is NULL";
    const int tp = 2 * (l->n_hidden + 1);
    if (const char *why = xsacw::tower_error(w->pi, tp)) return why;
    if (const char *why = xsacw::tower_error(w->vf, tp)) return why;
    if (!w->log_std) return "NULL log_std";
    const xarm_acw_weights *st[2] = {m, v};
    for (int k = 0; k < 2; k++) {
        for (int i = 0; i < tp; i++)
            if (!st[k]->pi[i] || !st[k]->vf[i]) return k ? "NULL exp_avg_sq pointer" : "NULL exp_avg pointer";
        if (!st[k]->log_std) return k ? "NULL exp_avg_sq pointer" : "NULL exp_avg pointer";
    }
    if (!step) return "step_i64 is NULL";
    if (!obs || !action || !reward || !done || !last_obs) return "NULL obs / action / reward / done / last_obs";
    if (!perm) return "perm is NULL";
    return xsacw::workspace_error(workspace);
}

// the GEMM shape of an actor-critic of two towers over B rows: the flat offsets of pi's tensors, vf's and log_std, the row ranges; Ppi and
// Ptow: pi's parameters and both towers'.  Shared with the wide A2C update (xarm_a2cw_core.h)
inline void fill_towers(xsacw::Shape &g, int64_t B, int obs_dim, int act_dim, int hidden, int n_hidden, int activation, int64_t &Ppi, int64_t &Ptow) {
    g.B = B; g.D = obs_dim; g.A = act_dim; g.H = hidden; g.L = n_hidden; g.NL = g.L + 1; g.act = activation;
    g.tp = 2 * g.NL; g.NT = 2 * g.tp + 1; g.BH = g.B * g.H;
    g.off[0] = 0;
    for (int t = 0; t < 2; t++)
        for (int k = 0; k < g.NL; k++) {
            const int i = t * g.tp + 2 * k;
            const int64_t nin = xsacw::in_of(g, k, g.D), nout = xsacw::out_of(g, k, t == 0 ? g.A : 1);
            g.off[i + 1] = g.off[i] + nout * nin;
            g.off[i + 2] = g.off[i + 1] + nout;
        }
    g.off[g.NT] = g.off[g.NT - 1] + g.A;
    g.P = g.off[g.NT];
    Ppi = g.off[g.tp]; Ptow = g.off[2 * g.tp];
    xsacw::fill_ranges(g);
}

inline void fill_shape(Dev &d, const xarm_ppow_layout *l) {
    const xarm_ppo_layout pl = ppo_layout_of(l);
    xppo::fill_shape(d.p, &pl);                 // E, N, T, D, A, B, M, S; the 64-64 parameter count is replaced below
    xsacw::Shape &g = d.g;
    fill_towers(g, d.p.B, l->obs_dim, l->act_dim, l->hidden, l->n_hidden, l->activation, d.Ppi, d.Ptow);
    d.p.a.P = g.P;
    d.p.a.NB = (int)((g.P + RED - 1) / RED);
    d.CN = d.p.M;
    d.CE = g.B > 0 ? (d.p.a.E + g.B - 1) / g.B : 0;
}

template <class D> inline void tensors_of(const D &d, const xarm_acw_weights *w, float **t) {
    for (int i = 0; i < d.g.tp; i++) { t[i] = const_cast<float *>(w->pi[i]); t[d.g.tp + i] = const_cast<float *>(w->vf[i]); }
    t[2 * d.g.tp] = const_cast<float *>(w->log_std);
}

// carve the workspace (each part 16-byte aligned); returns its size in bytes.  base may be null (size only)
inline int64_t fill_work(Dev &d, void *base) {
    const xsacw::Shape &g = d.g;
    const int64_t N = d.p.a.N, E = d.p.a.E, B = g.B;
    int64_t at = 0;
    char *b = (char *)base;
    auto take = [&at, b](int64_t floats) { char *o = b ? b + at : nullptr; at += (floats * 4 + 15) & ~(int64_t)15; return (float *)o; };
    d.adam = take(4); d.scal = (double *)take(2 * NSCAL); d.normpart = (double *)take(2 * (int64_t)d.p.a.NB);
    d.musig = (double *)take(2 * d.p.S * NMS);
    d.mean = take(N * g.A); d.value = take(N + E); d.adv = take(N); d.ret = take(N); d.oldlp = take(N);
    d.x = take(B * g.D); d.ga = take(B * g.A); d.gahat = take(B); d.gret = take(B); d.golp = take(B); d.guse = take(B);
    d.hid = take(2 * g.L * g.BH); d.dH = take(2 * g.L * g.BH);
    d.outM = take(B * g.A); d.outV = take(B); d.dOpi = take(B * g.A); d.dOvf = take(B);
    d.partial = take((int64_t)g.S * d.Ptow);
    d.grad = take(g.P);
    d.gv0 = d.dOvf;
    d.stop = b ? (int *)(d.adam + 2) : nullptr;
    return at;
}

// ------------------------------------------------------------------------------------------------------------ the rows' parts
// call start, row n: old_logp of the stored action under the call's weights (unless given); rows n < E: their env's GAE recursion
XARM_HD void gae_row(const Dev &d, int64_t n) {
    const xa2c::Shape &a = d.p.a;
    if (n == 0 && d.h.kl_limit > 0.0) d.stop[0] = 0;
    if (d.old_logp == nullptr) {
        float nodls[MAX_ACT];
        d.oldlp[n] = xa2c::pi_row<false>(a.A, d.mean + n * a.A, 1, d.action + n * a.A, d.w[2 * d.g.tp], 0.0f, nullptr, 0, nodls);
    }
    if (n >= a.E) return;
    float nv = d.value[a.N + n], na = 0.0f;
    for (int k = a.T - 1; k >= 0; k--) {
        const int64_t i = (int64_t)k * a.E + n;
        const float v = d.value[i];
        na = xppo::gae_step(d.h.gamma, d.h.gl, d.done[i], d.reward[i], v, nv, na);
        nv = v;
        const float rt = na + v;
        d.adv[i] = na;
        d.ret[i] = rt;
        if (d.out_adv != nullptr) d.out_adv[i] = na;
        if (d.out_returns != nullptr) d.out_returns[i] = rt;
    }
}

// thread t's part of step st's advantage sums: positions t, t + RED, ... of its span
XARM_HD void adv_sums(const Dev &d, int64_t st, int t, double &n, double &sa) {
    int64_t first, count;
    xppo::step_span(d.p, st, first, count);
    n = 0.0; sa = 0.0;
    for (int64_t i = t; i < count; i += RED) {
        const int64_t r = xppo::row_of(d.perm[first + i], d.p.a.N);
        if (r < 0) continue;
        const double u = d.use != nullptr ? (double)d.use[r] : 1.0;
        n += u;
        sa += (double)d.adv[r] * u;
    }
}
XARM_HD double adv_squares(const Dev &d, int64_t st, int t, double mu) {
    int64_t first, count;
    xppo::step_span(d.p, st, first, count);
    double sv = 0.0;
    for (int64_t i = t; i < count; i += RED) {
        const int64_t r = xppo::row_of(d.perm[first + i], d.p.a.N);
        if (r < 0) continue;
        const double u = d.use != nullptr ? (double)d.use[r] : 1.0, dd = (double)d.adv[r] - mu;
        sv += dd * dd * u;
    }
    return sv;
}
XARM_HD double mean_of(double n, double sa) { return n > 0.0 ? sa / n : 0.0; }

// column j of gathered row i of step st: j < D obs, < D + A action, then A^, ret, old_logp, use and, with clip_range_vf, v0
XARM_HD int gather_width(const Dev &d) { return d.g.D + d.g.A + (d.h.vclip > 0.0f ? 5 : 4); }
XARM_HD void gather_at(const Dev &d, int64_t st, int64_t i, int j) {
    const int D = d.g.D, A = d.g.A;
    int64_t first, count;
    xppo::step_span(d.p, st, first, count);
    const int64_t r = i < count ? xppo::row_of(d.perm[first + i], d.p.a.N) : -1;
    const bool in = r >= 0;
    if (j < D) d.x[i * D + j] = in ? d.obs[r * D + j] : 0.0f;
    else if (j < D + A) d.ga[i * A + (j - D)] = in ? d.action[r * A + (j - D)] : 0.0f;
    else if (j == D + A) d.gahat[i] = in ? xppo::norm_adv(d.adv[r], d.musig + st * NMS) : 0.0f;
    else if (j == D + A + 1) d.gret[i] = in ? d.ret[r] : 0.0f;
    else if (j == D + A + 2) d.golp[i] = in ? (d.old_logp != nullptr ? d.old_logp[r] : d.oldlp[r]) : 0.0f;
    else if (j == D + A + 3) d.guse[i] = in ? (d.use != nullptr ? d.use[r] : 1.0f) : 0.0f;
    else d.gv0[i] = in ? d.value[r] : 0.0f;
}

// behind the step's forward, gathered row i: both towers' output deltas, the row's terms added to sums (xppo's record: 0 surrogate,
// 1 value loss, 2 use, 3 + c log_std_c, 19 kl, 20 clipped).  VCLIP: the call has clip_range_vf on (the launch picks the instantiation)
template <bool VCLIP> XARM_HD void head_row(const Dev &d, int64_t i, double *sums) {
    const int A = d.g.A;
    const float u = d.guse[i], *mean = d.outM + i * A, *act = d.ga + i * A, *log_std = d.w[2 * d.g.tp];
    float dls[MAX_ACT];
#pragma unroll
    for (int c = 0; c < MAX_ACT; c++) dls[c] = 0.0f;
    const float lp = xa2c::pi_row<false>(A, mean, 1, act, log_std, 0.0f, nullptr, 0, dls);
    const xppo::RowTerms t = xppo::surrogate(d.h, d.gahat[i], lp, d.golp[i], u);
    xa2c::pi_row<true>(A, mean, 1, act, log_std, t.q, d.dOpi + i * A, 1, dls);
    const float v = d.outV[i], rt = d.gret[i];
    const xppo::ValueTerms vt = xppo::value_terms<VCLIP>(d.h, v, VCLIP ? d.gv0[i] : v, rt, u);
    d.dOvf[i] = vt.dvalue;
    sums[0] += (double)t.surr; sums[1] += (double)vt.loss; sums[2] += (double)u;
    sums[19] += (double)t.kl; sums[20] += (double)t.clipped;
#pragma unroll
    for (int c = 0; c < MAX_ACT; c++)
        if (c < A) sums[3 + c] += (double)dls[c];
}

// ------------------------------------------------------------------------------------------------------------ the parameters' parts
// (these are templates over the learner's Dev - g, Ptow, partial, scal with slot 2 the sum of use and slots 3 + c log_std's sums, h.ent_coef,
// grad, normpart, out_grad - so that the wide A2C update states none of them again)
template <class D> XARM_HD double n_use_of(const D &d) { return xopt::n_use(d.scal[2]); }

// the step's gradient of flat parameter p, before the clip; scal: the step's sums over rows (d.scal, or a workgroup's copy of them)
template <class D> XARM_HD float param_grad(const D &d, const double *scal, int64_t p) {
    const bool ls = p >= d.Ptow;
    double v = (ls ? scal[3 + (p - d.Ptow)] : xopt::slice_sum(d.partial + p, d.g.S, d.Ptow)) / xopt::n_use(scal[2]);
    if (ls) v -= d.h.ent_coef;
    return (float)v;
}
template <class D> XARM_HD float param_grad(const D &d, int64_t p) { return param_grad(d, d.scal, p); }

// one thread per step, in the reduce launch: the KL stop's decision; step++ and Adam's scalars unless it trips; the stats row (slot 3, the
// norm, is the apply launch's, which a tripping step does not reach)
XARM_HD void finish_step(const Dev &d, int64_t st) {
    const double n_use = n_use_of(d);
    const bool trips = xppo::kl_trips(d.h, (float)(d.scal[19] / n_use));
    if (trips) {
        d.stop[0] = (int)st + 1;
    } else {
        const int64_t t = d.step[0] + 1;
        d.step[0] = t;
        xopt::adam_scalars(d.h.adam, t, d.adam);
    }
    if (d.out_stats == nullptr) return;
    const double ent = xopt::gaussian_entropy(d.w[2 * d.g.tp], d.g.A);
    float *o = d.out_stats + st * 8;
    o[0] = (float)(-d.scal[0] / n_use); o[1] = (float)(d.scal[1] / n_use); o[2] = (float)ent; o[4] = (float)n_use;
    o[5] = (float)(d.scal[19] / n_use); o[6] = (float)(d.scal[20] / n_use); o[7] = trips ? 1.0f : 0.0f;
    if (trips) o[3] = 0.0f;
}
// the reduce launch of a step behind the one that tripped: its stats row, by one thread
XARM_HD void skip_step(const Dev &d, int64_t st) {
    if (d.out_stats != nullptr) xppo::stopped_row(d.out_stats + st * 8);
}

// the norm from normpart's NB blocks in block order; returns the clip coefficient
template <class D> XARM_HD float clip_of(const D &d, int NB, float &norm) {
    double sum2 = 0.0;
    for (int b = 0; b < NB; b++) sum2 += d.normpart[b];
    norm = (float)__builtin_sqrt(sum2);
    return xopt::clip_coef(norm, d.h.max_norm);
}
XARM_HD float clip_of(const Dev &d, float &norm) { return clip_of(d, d.p.a.NB, norm); }

XARM_HD void apply_param(const Dev &d, int64_t p, float coef) {
    const int i = xopt::tensor_at(d.g.off, 0, d.g.NT, p);
    const int64_t e = p - d.g.off[i];
    const float sc[2] = {d.adam[0], d.adam[1]};
    float m = d.m[i][e], v = d.v[i][e], w = d.w[i][e];
    xopt::adam(d.h.adam, sc, d.grad[p] * coef, m, v, w);
    d.m[i][e] = m;
    d.v[i][e] = v;
    d.w[i][e] = w;
}

// ------------------------------------------------------------------------------------------------------------ the chain
// c (L + 1) + 2 + S (2 L + 6) launches, c = M + ceil(E / B) the call-start forward chunks
inline int64_t launches(int n_hidden, int64_t steps, int64_t chunks) { return chunks * (n_hidden + 1) + 2 + steps * (2 * n_hidden + 6); }

template <class X> void run_update(const Dev &d, X &ex) {
    const xsacw::Shape &g = d.g;
    const int tp = g.tp;
    const int64_t N = d.p.a.N, E = d.p.a.E, B = g.B;
    const xsacw::TowerRef pi = {d.w, g.D, g.A}, vf = {d.w + tp, g.D, 1};
    float *hid[2] = {d.hid, d.hid + g.L * g.BH}, *dh[2] = {d.dH, d.dH + g.L * g.BH};
    for (int64_t c = 0; c < d.CN + d.CE; c++) {
        const bool boot = c >= d.CN;
        const int64_t r0 = (boot ? c - d.CN : c) * B, rows = (boot ? E : N) - r0 < B ? (boot ? E : N) - r0 : B;
        xsacw::Shape sc = g;
        sc.B = rows; sc.BH = rows * g.H;
        const xsacw::TowerRef T[2] = {vf, pi};
        const float *in[2] = {(boot ? d.last_obs : d.obs) + r0 * g.D, d.obs + r0 * g.D};
        float *out[2] = {d.value + (boot ? N : 0) + r0, d.mean + r0 * g.A};
        xsacw::fwd_pass(sc, ex, (boot || d.old_logp != nullptr) ? 1 : 2, T, in, hid, out);
    }
    ex.gae(d);
    ex.advstats(d);
    for (int64_t st = 0; st < d.p.S; st++) {
        const xsacw::TowerRef T[2] = {pi, vf};
        const float *in[2] = {d.x, d.x}, *dO[2] = {d.dOpi, d.dOvf};
        float *out[2] = {d.outM, d.outV};
        const int64_t base[2] = {0, d.Ppi};
        const int t0[2] = {0, tp};
        const xsacw::Gate gate = {d.h.kl_limit > 0.0 ? d.stop : nullptr, st};
        ex.gather(d, st);
        xsacw::fwd_pass(g, ex, 2, T, in, hid, out, gate);
        ex.head(d, st);
        xsacw::bd_pass(g, ex, 2, T, dO, hid, dh, gate);
        xsacw::wg_pass(g, d.partial, ex, 2, T, in, dO, hid, dh, base, t0, d.Ptow, gate);
        ex.reduce(d, st);
        ex.apply(d, st);
    }
}

#if !defined(__HIPCC__) || defined(XARM_HOST_BUILD)
// the reduce launch as loops: a block's RED parameters through param_grad into grad (and out_grad when `keep`), the block's squares by the
// device's tree into normpart
template <class D> void host_reduce_blocks(const D &d, int NB, bool keep) {
    for (int b = 0; b < NB; b++) {
        double red[RED];
        for (int t = 0; t < RED; t++) {
            const int64_t p = (int64_t)b * RED + t;
            red[t] = 0.0;
            if (p < d.g.P) {
                const float gf = param_grad(d, p);
                d.grad[p] = gf;
                if (keep && d.out_grad != nullptr) d.out_grad[p] = gf;
                red[t] = (double)gf * (double)gf;
            }
        }
        for (int s = RED / 2; s > 0; s >>= 1)       // the device's block tree
            for (int t = 0; t < s; t++) red[t] += red[t + s];
        d.normpart[b] = red[0];
    }
}

// ---- the host build: the GEMM jobs through xsacw::HostExec's loops, the rest with the device's thread and block structure as loops
struct HostExec : xsacw::HostExec {
    void gae(const Dev &d) {
        for (int64_t n = 0; n < d.p.a.N; n++) gae_row(d, n);
    }
    void advstats(const Dev &d) {
        for (int64_t st = 0; st < d.p.S; st++) {
            double n = 0.0, sa = 0.0, sv = 0.0;
            for (int t = 0; t < RED; t++) {
                double a, b;
                adv_sums(d, st, t, a, b);
                n += a; sa += b;
            }
            const double mu = mean_of(n, sa);
            for (int t = 0; t < RED; t++) sv += adv_squares(d, st, t, mu);
            xppo::finish_stats(d.musig + st * NMS, n, mu, sv, d.h.normalize);
        }
    }
    void gather(const Dev &d, int64_t st) {
        if (xppo::stopped_before(d.h, d.stop, st)) return;
        const int W = gather_width(d);
        for (int64_t i = 0; i < d.g.B; i++)
            for (int j = 0; j < W; j++) gather_at(d, st, i, j);
    }
    void head(const Dev &d, int64_t st) {
        if (xppo::stopped_before(d.h, d.stop, st)) return;
        double tot[NSCAL] = {0.0};
        for (int t = 0; t < RED; t++) {
            double sums[NSCAL] = {0.0};
            for (int64_t i = t; i < d.g.B; i += RED) {
                if (d.h.vclip > 0.0f) head_row<true>(d, i, sums);
                else head_row<false>(d, i, sums);
            }
            for (int k = 0; k < NSCAL; k++) tot[k] += sums[k];
        }
        for (int k = 0; k < NSCAL; k++) d.scal[k] = tot[k];
    }
    void reduce(const Dev &d, int64_t st) {
        if (xppo::stopped_before(d.h, d.stop, st)) { skip_step(d, st); return; }
        host_reduce_blocks(d, d.p.a.NB, st == 0);
        finish_step(d, st);
    }
    void apply(const Dev &d, int64_t st) {
        if (xppo::stopped_at(d.h, d.stop)) return;
        float norm;
        const float coef = clip_of(d, norm);
        if (d.out_stats != nullptr) d.out_stats[st * 8 + 3] = norm;
        for (int64_t p = 0; p < d.g.P; p++) apply_param(d, p, coef);
    }
};
#endif

#if defined(__HIPCC__) && !defined(XARM_HOST_BUILD)
// the launches of one update on `stream` (xarm_k_ppow.hip); returns the launches' hipError_t
int launch_update(const Dev &d, void *stream);
#endif

}  // namespace xppow
