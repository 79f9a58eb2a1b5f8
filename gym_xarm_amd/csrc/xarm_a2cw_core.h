// xarm_a2cw_core.h - wide device-resident A2C update: the update of xarm_a2c_core.h for train.py's
// ActorCritic(net_arch, activation) with equal-width towers of two or three hidden layers of 64, 128, 192 or 256 units, tanh or ReLU.
// It is the wide PPO update's chain (xarm_ppow_core.h) with ONE optimiser step over the whole rollout in the identity
// order - B = N rows, no perm, no gather: the GEMMs read obs [T, E, D] in place - A2C's head and RMSprop.  This file states the chain
// (run_update) and the per-row functions ONCE; xarm_k_a2cw.hip executes them on the device, the host build (g++ -DXARM_HOST_BUILD
// -ffp-contract=off, tests/hostbuild_a2cw/) with plain loops over the same workspace: everything the call writes - returns, gradient,
// stats, parameters, square_avg, the workspace - is equal between them bit for bit.
//
// Called, not copied: the GEMM jobs, passes, row ranges and activation of xarm_sacw_core.h; return_step, pi_row, value_delta, layout_error,
// params_error and fill_hyper of xarm_a2c_core.h; fill_towers, tensors_of, param_grad, clip_of and host_reduce_blocks of
// xarm_ppow_core.h; slice_sum, n_use, gaussian_entropy, clip_coef, tensor_at and rmsprop of xarm_opt_core.h.
//
//   flat order   pi's 2 (L + 1) tensors W1, b1, ..., W_out, b_out, vf's, log_std: NT = 4 (L + 1) + 1 tensors, P parameters
//   chain        vf over last_obs (E rows, L + 1 launches, one job) into value[N ..] | returns (one thread per env) | pi and vf over the N
//                rollout rows (L + 1 launches, two jobs) into mean and value[.. N) | head: both towers' output deltas, log_std's terms, the
//                sums | L delta launches | one weight-gradient launch | reduce | apply: 3 L + 7 launches
//   head         G = min(HEAD_GROUPS, ceil(N / 256)) workgroups of 256 threads: thread t of group g walks rows 256 g + t, + 256 G, ... in
//                float64; a group adds its 256 records in thread order into its slot; the reduce launch adds the G slots in g order
//   sums         over a gradient's rows: sacw's - float32 fmaf chains within one of at most 16 ranges of whole 64-row tiles, the ranges
//                added in float64 in range order, / n_use, rounded once.  The squares of a block of 256 parameters: a fixed tree.
#pragma once
#include "xarm_ppow_core.h"

namespace xa2cw {

using xa2c::NSCAL;              // the record of DESIGN.md 21: 0 sum adv logp use, 1 sum (ret - value)^2 use, 2 sum use, 3 + c log_std_c's sum
using xpol::MAX_ACT;
using xppow::MAX_NT;
using xppow::RED;

constexpr int HEAD_GROUPS = 64;     // the most workgroups of the head launch: 5 x 65 536 rows are 20 rows per thread

struct Dev {
    xsacw::Shape g;                 // the GEMMs over the whole rollout: B = N rows, D, A, H, L, NL, BH, act, tp, NT, off, P, S, rows
    xa2c::Hyper h;
    int64_t E, N, Ppi, Ptow;
    int T, G, NB;                   // steps; head groups; blocks of RED parameters
    float *w[MAX_NT], *sq[MAX_NT];
    const float *obs, *action, *reward, *done, *use, *last_obs;
    // the workspace
    double *scal, *rec, *normpart;                      // the NSCAL sums; the head groups' records [G][NSCAL]; a block's sum of squares
    float *value, *ret;                                 // vf's outputs on the N rollout rows and on last_obs [N + E]; the returns [N]
    float *mean, *dOpi, *dOvf;                          // pi's outputs [N, A]; the towers' output deltas [N, A], [N]
    float *hid, *dH;                                    // activations and deltas [2][L][N, H]
    float *partial, *grad;                              // [ranges][Ptow]; [P]
    float *out_returns, *out_grad, *out_stats;
};

inline xarm_a2c_layout a2c_layout_of(const xarm_a2cw_layout *l) {
    const xarm_a2c_layout a = {l->num_envs, l->n_steps, l->obs_dim, l->act_dim, xpol::HID};
    return a;
}

inline const char *layout_error(const xarm_a2cw_layout *l) {
    if (!l) return "layout is NULL";
    const xarm_a2c_layout a = a2c_layout_of(l);
    if (const char *why = xa2c::layout_error(&a)) return why;
    return xsacw::towers_error(l->hidden, l->n_hidden, l->activation);
}

// the pointers a call with num_envs > 0 reads or writes; null when all are there
inline const char *pointer_error(const xarm_a2cw_layout *l, const xarm_acw_weights *w, const xarm_acw_weights *sq, const float *obs, const float *action,
                                 const float *reward, const float *done, const float *last_obs, const void *workspace) {
    if (!w) return "weights is NULL";
    if (!sq) return "square_avg is NULL";
    const int tp = 2 * (l->n_hidden + 1);
    if (const char *why = xsacw::tower_error(w->pi, tp)) return why;
    if (const char *why = xsacw::tower_error(w->vf, tp)) return why;
    if (!w->log_std) return "NULL log_std";
    for (int i = 0; i < tp; i++)
        if (!sq->pi[i] || !sq->vf[i]) return "NULL square_avg pointer";
    if (!sq->log_std) return "NULL square_avg pointer";
    if (!obs || !action || !reward || !done || !last_obs) return "NULL obs / action / reward / done / last_obs";
    return xsacw::workspace_error(workspace);
}

inline void fill_shape(Dev &d, const xarm_a2cw_layout *l) {
    d.E = l->num_envs; d.T = l->n_steps; d.N = d.E * d.T;
    xppow::fill_towers(d.g, d.N, l->obs_dim, l->act_dim, l->hidden, l->n_hidden, l->activation, d.Ppi, d.Ptow);
    const int64_t groups = (d.N + RED - 1) / RED;
    d.G = (int)(groups < HEAD_GROUPS ? groups : HEAD_GROUPS);
    d.NB = (int)((d.g.P + RED - 1) / RED);
}

// carve the workspace (each part 16-byte aligned); returns its size in bytes.  base may be null (size only)
inline int64_t fill_work(Dev &d, void *base) {
    const xsacw::Shape &g = d.g;
    const int64_t N = d.N;
    int64_t at = 0;
    char *b = (char *)base;
    auto take = [&at, b](int64_t floats) { char *o = b ? b + at : nullptr; at += (floats * 4 + 15) & ~(int64_t)15; return (float *)o; };
    d.scal = (double *)take(2 * NSCAL); d.rec = (double *)take(2 * (int64_t)d.G * NSCAL); d.normpart = (double *)take(2 * (int64_t)d.NB);
    d.value = take(N + d.E); d.ret = take(N);
    d.mean = take(N * g.A); d.dOpi = take(N * g.A); d.dOvf = take(N);
    d.hid = take(2 * g.L * g.BH); d.dH = take(2 * g.L * g.BH);
    d.partial = take((int64_t)g.S * d.Ptow);
    d.grad = take(g.P);
    return at;
}

// ------------------------------------------------------------------------------------------------------------ the rows' parts
// env e: the n-step returns down its T rows from the bootstrap value
XARM_HD void returns_env(const Dev &d, int64_t e) {
    float r = d.value[d.N + e];
    for (int k = d.T - 1; k >= 0; k--) {
        const int64_t n = (int64_t)k * d.E + e;
        r = xa2c::return_step(d.h.gamma, d.done[n], d.reward[n], r);
        d.ret[n] = r;
        if (d.out_returns != nullptr) d.out_returns[n] = r;
    }
}

// behind the forward, row n: both towers' output deltas, the row's terms added to sums
XARM_HD void head_row(const Dev &d, int64_t n, double *sums) {
    const int A = d.g.A;
    const float u = d.use != nullptr ? d.use[n] : 1.0f, v = d.value[n], r = d.ret[n], adv = r - v;
    float dls[MAX_ACT];
#pragma unroll
    for (int c = 0; c < MAX_ACT; c++) dls[c] = 0.0f;
    const float lp = xa2c::pi_row<true>(A, d.mean + n * A, 1, d.action + n * A, d.w[2 * d.g.tp], -(adv * u), d.dOpi + n * A, 1, dls);
    d.dOvf[n] = xa2c::value_delta(d.h.vf2, v, r, u);
    sums[0] += (double)(adv * lp * u); sums[1] += (double)((r - v) * (r - v) * u); sums[2] += (double)u;
#pragma unroll
    for (int c = 0; c < MAX_ACT; c++)
        if (c < A) sums[3 + c] += (double)dls[c];
}

// thread t of head group g: its rows' sums
XARM_HD void head_thread(const Dev &d, int g, int t, double *sums) {
    for (int64_t n = (int64_t)g * RED + t; n < d.N; n += (int64_t)RED * d.G) head_row(d, n, sums);
}

// scalar k of the call: the G groups' slots added in g order
XARM_HD double groups_sum(const Dev &d, int k) {
    double tot = 0.0;
    for (int g = 0; g < d.G; g++) tot += d.rec[(int64_t)g * NSCAL + k];
    return tot;
}

// ------------------------------------------------------------------------------------------------------------ the parameters' parts
// one thread, in the reduce launch: the stats row from the call's sums (slot 3, the norm, is the apply launch's)
XARM_HD void finish_stats(const Dev &d, const double *scal) {
    if (d.out_stats == nullptr) return;
    const double n_use = xopt::n_use(scal[2]);
    float *o = d.out_stats;
    o[0] = (float)(-scal[0] / n_use); o[1] = (float)(scal[1] / n_use); o[2] = (float)xopt::gaussian_entropy(d.w[2 * d.g.tp], d.g.A);
    o[4] = (float)n_use; o[5] = 0.0f; o[6] = 0.0f; o[7] = 0.0f;
}

XARM_HD void apply_param(const Dev &d, int64_t p, float coef) {
    const int i = xopt::tensor_at(d.g.off, 0, d.g.NT, p);
    const int64_t e = p - d.g.off[i];
    float sq = d.sq[i][e], w = d.w[i][e];
    xopt::rmsprop(d.h.rms, d.grad[p] * coef, sq, w);
    d.sq[i][e] = sq;
    d.w[i][e] = w;
}

// ------------------------------------------------------------------------------------------------------------ the chain
constexpr int launches(int n_hidden) { return 3 * n_hidden + 7; }

template <class X> void run_update(const Dev &d, X &ex) {
    const xsacw::Shape &g = d.g;
    const int tp = g.tp;
    const xsacw::TowerRef pi = {d.w, g.D, g.A}, vf = {d.w + tp, g.D, 1};
    float *hid[2] = {d.hid, d.hid + g.L * g.BH}, *dh[2] = {d.dH, d.dH + g.L * g.BH};
    {   // the bootstrap value: vf over last_obs with its own row count, through the activation buffers the rollout's forward rewrites
        xsacw::Shape sb = g;
        sb.B = d.E; sb.BH = d.E * g.H;
        const xsacw::TowerRef T[1] = {vf};
        const float *in[1] = {d.last_obs};
        float *out[1] = {d.value + d.N};
        xsacw::fwd_pass(sb, ex, 1, T, in, hid, out);
    }
    ex.returns(d);
    const xsacw::TowerRef T[2] = {pi, vf};
    const float *in[2] = {d.obs, d.obs}, *dO[2] = {d.dOpi, d.dOvf};
    float *out[2] = {d.mean, d.value};
    const int64_t base[2] = {0, d.Ppi};
    const int t0[2] = {0, tp};
    xsacw::fwd_pass(g, ex, 2, T, in, hid, out);
    ex.head(d);
    xsacw::bd_pass(g, ex, 2, T, dO, hid, dh);
    xsacw::wg_pass(g, d.partial, ex, 2, T, in, dO, hid, dh, base, t0, d.Ptow);
    ex.reduce(d);
    ex.apply(d);
}

#if !defined(__HIPCC__) || defined(XARM_HOST_BUILD)
// ---- the host build: the GEMM jobs through xsacw::HostExec's loops, the rest with the device's thread and block structure as loops
struct HostExec : xsacw::HostExec {
    void returns(const Dev &d) {
        for (int64_t e = 0; e < d.E; e++) returns_env(d, e);
    }
    void head(const Dev &d) {
        for (int g = 0; g < d.G; g++) {
            double tot[NSCAL] = {0.0};
            for (int t = 0; t < RED; t++) {
                double sums[NSCAL] = {0.0};
                head_thread(d, g, t, sums);
                for (int k = 0; k < NSCAL; k++) tot[k] += sums[k];
            }
            for (int k = 0; k < NSCAL; k++) d.rec[(int64_t)g * NSCAL + k] = tot[k];
        }
    }
    void reduce(const Dev &d) {
        for (int k = 0; k < NSCAL; k++) d.scal[k] = groups_sum(d, k);
        xppow::host_reduce_blocks(d, d.NB, true);
        finish_stats(d, d.scal);
    }
    void apply(const Dev &d) {
        float norm;
        const float coef = xppow::clip_of(d, d.NB, norm);
        if (d.out_stats != nullptr) d.out_stats[3] = norm;
        for (int64_t p = 0; p < d.g.P; p++) apply_param(d, p, coef);
    }
};
#endif

#if defined(__HIPCC__) && !defined(XARM_HOST_BUILD)
// the launches of one update on `stream` (xarm_k_a2cw.hip); returns the launches' hipError_t
int launch_update(const Dev &d, void *stream);
#endif

}  // namespace xa2cw
