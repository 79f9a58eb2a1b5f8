// xarm_sacw_core.h - wide device-resident SAC: the step of xarm_sac_core.h for equal-width towers of two or
// three hidden layers of 64, 128, 192 or 256 units, tanh or ReLU - the reference's `net_arch=[256, 256, 256]` among them.  At 256 units
// one layer's weights are 256 KB, more than a CU's LDS, so nothing of 23's fused 64-row tile carries over: a step is a CHAIN of per-layer
// GEMM launches with the activations in the workspace.  This file states the chain (run_update, run_act), the jobs of its three GEMM
// kinds and every per-row and per-parameter formula ONCE; xarm_k_sacw.hip executes the jobs on v_mfma_f32_32x32x2_f32 and the host build
// (g++ -DXARM_HOST_BUILD -ffp-contract=off, tests/hostbuild_sacw/) executes the same jobs with plain loops.  Both builds run the same
// chain over the same workspace, so everything - rows, gradients, parameters, stats - is equal between them bit for bit.
//
//   towers    actor D -> H x L -> 2A, critics and targets Dq = D + A -> H x L -> 1; tensors per tower W1, b1, ..., W_out, b_out
//   forward   out[n][u] = act(chain), chain = fmaf over k ascending from b[u] of x[n][k] W[u][k].  One MFMA adds two k, lane half 0's
//             first: fmaf(x1, w1, fmaf(x0, w0, c)).  An odd K is padded with one zero operand, fmaf(0, 0, acc), in both builds.
//   act       relu(x) = x > 0 ? x : 0, derivative h > 0 ? 1 : 0;  tanh = xpol::tanh_f, derivative fmaf(-h, h, 1)
//   delta     pre[n][i] = fmaf over k ascending from 0 of d[n][k] W[k][c0 + i] (odd K padded alike); out = pre * derivative(h[n][i])
//   wgrad     dW[j][i] = fmaf over a row range's rows n ascending from 0 of d[n][j] x[n][i] (odd count padded alike); the bias is column
//             i = K with x = 1.  Row ranges: the 64-row tiles dealt in order to S = min(16, tiles) contiguous ranges.
//   reduce    g = (float)(sum over ranges, in range order, of (double) partial / n_use)
//   scalars   a sum over rows is 256 float64 sums over the rows t, t + 256, ..., added in t order
//   heads     xsac::actor_head, target_row, actor_deltas, polyak, noise4; finish; xopt::adam, slice_sum, tensor_at (xarm_opt_core.h): called, not copied
#pragma once
#include "xarm_sac_core.h"

namespace xsacw {

using xpol::fma32;
using xsac::Hyper;
using xsac::MAX_A;

constexpr int MAX_L = XARM_SACW_MAX_LAYERS, TP = 2 * (MAX_L + 1), MAX_NT = 3 * TP + 1;
constexpr int MAX_SPLIT = 16;               // the most row ranges of a weight gradient: the partials are MAX_SPLIT gradients at most
constexpr int SPLIT_ROWS = 64;              // a range is whole 64-row tiles
constexpr int RED = 256;                    // threads of the per-row and per-parameter kernels
constexpr int TILE = 32;                    // a GEMM workgroup is one wavefront on one 32 x 32 accumulator tile
constexpr int ACT_TANH = XARM_SACW_TANH, ACT_RELU = XARM_SACW_RELU, ACT_NONE = 2;
constexpr int NSC = 8;                      // scalars (double): use, logp_pi use, (logp_pi + target_entropy) use, (q - y)^2 use, (alpha logp_pi - qmin) use, qmin use

struct Shape {
    int64_t B, BH, P, Pa, Pq, row_offset;
    int D, A, Dq, H, L, NL, act, S, NT, tp;     // NL = L + 1 layers; tp = 2 NL tensors per tower; NT = 3 tp + 1 trained tensors
    int64_t off[MAX_NT + 1];                    // where trained tensor i starts in the flat gradient: actor, q1, q2, log_alpha
    int64_t rows[MAX_SPLIT + 1];                // range s is rows [rows[s], rows[s + 1])
};

// the tower shapes every wide unit accepts
inline const char *towers_error(int hidden, int n_hidden, int activation) {
    if (hidden != 64 && hidden != 128 && hidden != 192 && hidden != 256) return "hidden must be 64, 128, 192 or 256";
    if (n_hidden != 2 && n_hidden != 3) return "n_hidden must be 2 or 3";
    if (activation != ACT_TANH && activation != ACT_RELU) return "activation must be XARM_SACW_TANH or XARM_SACW_RELU";
    return nullptr;
}

inline const char *layout_error(const xarm_sacw_layout *l) {
    if (!l) return "layout is NULL";
    if (l->batch_size < 0) return "batch_size must be >= 0 (and < 2^31)";
    if (l->obs_dim < 1) return "obs_dim must be >= 1";
    if (l->act_dim < 1 || l->act_dim > MAX_A) return "act_dim must lie in [1, XARM_SAC_MAX_ACT (8)]";
    if (l->obs_dim > xpol::MAX_DIM || l->obs_dim + l->act_dim > xpol::MAX_DIM) return "obs_dim + act_dim must be <= XARM_POLICY_MAX_DIM (96)";
    if (const char *why = towers_error(l->hidden, l->n_hidden, l->activation)) return why;
    if (l->row_offset < 0) return "row_offset must be >= 0";
    return nullptr;
}

// all 2 NL tensors of a tower there, b1 .. W_out 16-byte aligned
inline const char *tower_error(const float *const *p, int tp) {
    for (int i = 0; i < tp; i++)
        if (!p[i]) return "NULL weight pointer";
    for (int i = 1; i < tp - 1; i++)
        if (((uintptr_t)p[i] & 15u) != 0) return "the tensors b1 .. W_out must be 16-byte aligned";
    return nullptr;
}

inline const char *workspace_error(const void *workspace) {
    if (!workspace) return "workspace is NULL";
    if (((uintptr_t)workspace & 15u) != 0) return "workspace must be 16-byte aligned";
    return nullptr;
}

inline const char *act_pointer_error(const xarm_sacw_layout *l, const xarm_sac_params *p, const xarm_sacw_weights *w, const int64_t *calls,
                                     const float *obs, const void *workspace, const float *action) {
    if (!w) return "weights is NULL";
    if (const char *why = tower_error(w->actor, 2 * (l->n_hidden + 1))) return why;
    if (!p->deterministic && !calls) return "NULL calls with a stochastic call";
    if (!obs) return "NULL observation pointer";
    if (!action) return "NULL out_action";
    return workspace_error(workspace);
}

inline const char *pointer_error(const xarm_sacw_layout *l, const xarm_sacw_weights *w, const xarm_sacw_weights *m, const xarm_sacw_weights *v,
                                 const int64_t *step, const float *obs, const float *next_obs, const float *action, const float *reward,
                                 const float *done, const void *workspace) {
    if (!w) return "weights is NULL";
    if (!m || !v) return "exp_avg / exp_avg_sq is NULL";
    const int tp = 2 * (l->n_hidden + 1);
    const float *const *towers[5] = {w->actor, w->q1, w->q2, w->q1_target, w->q2_target};
    for (int i = 0; i < 5; i++)
        if (const char *why = tower_error(towers[i], tp)) return why;
    if (!w->log_alpha) return "NULL log_alpha";
    const xarm_sacw_weights *st[2] = {m, v};
    for (int k = 0; k < 2; k++) {
        for (int i = 0; i < tp; i++)
            if (!st[k]->actor[i] || !st[k]->q1[i] || !st[k]->q2[i]) return k ? "NULL exp_avg_sq pointer" : "NULL exp_avg pointer";
        if (!st[k]->log_alpha) return k ? "NULL exp_avg_sq pointer" : "NULL exp_avg pointer";
    }
    if (!step) return "step_i64 is NULL";
    if (!obs || !next_obs || !action || !reward || !done) return "NULL obs / next_obs / action / reward / done";
    return workspace_error(workspace);
}

inline int in_of(const Shape &s, int l, int Din) { return l == 0 ? Din : s.H; }
inline int out_of(const Shape &s, int l, int nout) { return l == s.NL - 1 ? nout : s.H; }

// the row ranges of a weight gradient over s.B rows: the 64-row tiles dealt in order to S = min(16, tiles) contiguous ranges
inline void fill_ranges(Shape &s) {
    const int64_t tiles = (s.B + SPLIT_ROWS - 1) / SPLIT_ROWS;
    s.S = (int)(tiles < MAX_SPLIT ? (tiles > 0 ? tiles : 1) : MAX_SPLIT);
    for (int k = 0; k <= MAX_SPLIT; k++) {
        const int64_t r = k >= s.S ? s.B : (tiles * k / s.S) * SPLIT_ROWS;
        s.rows[k] = r < s.B ? r : s.B;
    }
}

inline void fill_shape(Shape &s, const xarm_sacw_layout *l) {
    s.B = l->batch_size; s.D = l->obs_dim; s.A = l->act_dim; s.Dq = s.D + s.A; s.H = l->hidden; s.L = l->n_hidden; s.NL = s.L + 1;
    s.act = l->activation; s.row_offset = l->row_offset; s.tp = 2 * s.NL; s.NT = 3 * s.tp + 1; s.BH = s.B * s.H;
    s.off[0] = 0;
    for (int t = 0; t < 3; t++)
        for (int k = 0; k < s.NL; k++) {
            const int i = t * s.tp + 2 * k;
            const int64_t nin = in_of(s, k, t == 0 ? s.D : s.Dq), nout = out_of(s, k, t == 0 ? 2 * s.A : 1);
            s.off[i + 1] = s.off[i] + nout * nin;
            s.off[i + 2] = s.off[i + 1] + nout;
        }
    s.off[s.NT] = s.off[s.NT - 1] + 1;
    s.Pa = s.off[s.tp]; s.Pq = s.off[2 * s.tp] - s.off[s.tp]; s.P = s.off[s.NT];
    fill_ranges(s);
}

// the trained tensors of a weights struct in the flat order; tq: the 2 tp target tensors
inline void tensors_of(const Shape &s, const xarm_sacw_weights *w, float **t, float **tq) {
    for (int i = 0; i < s.tp; i++) {
        t[i] = const_cast<float *>(w->actor[i]);
        t[s.tp + i] = const_cast<float *>(w->q1[i]);
        t[2 * s.tp + i] = const_cast<float *>(w->q2[i]);
        if (tq) { tq[i] = const_cast<float *>(w->q1_target[i]); tq[s.tp + i] = const_cast<float *>(w->q2_target[i]); }
    }
    t[3 * s.tp] = const_cast<float *>(w->log_alpha);
}

struct Dev {
    Shape s;
    Hyper h;
    float *w[MAX_NT], *m[MAX_NT], *v[MAX_NT], *tq[2 * TP];
    int64_t *step, *calls;
    const float *obs, *next_obs, *action, *reward, *done, *use, *noise_pi, *noise_next;
    // the workspace
    float *hdr;                     // Adam's two scalars of the step, alpha, 0
    double *scal;                   // NSC sums over rows
    float *y, *logp, *lpn, *z, *ones, *xq, *xpi, *xn;       // per row: y, logp_pi, logp', z_pi, 1, obs | action, obs | a_pi, next_obs | a'
    float *outN, *outP;             // the actor's 2 A raw outputs on next_obs and on obs
    float *hA, *hS, *dH, *dO;       // hidden activations: the actor's on obs [L][B, H], four scratch towers; deltas of two towers; output deltas
    float *qt, *q, *qpi, *dqda, *partial;
    float *out_grad, *out_dqda, *out_target, *out_stats, *out_q, *out_action, *out_logp;
};

// carve the workspace (each part 16-byte aligned); returns its size in bytes.  base may be null (size only)
inline int64_t fill_work(Dev &d, void *base) {
    const Shape &s = d.s;
    int64_t at = 0;
    char *b = (char *)base;
    auto take = [&at, b](int64_t floats) { char *o = b ? b + at : nullptr; at += (floats * 4 + 15) & ~(int64_t)15; return (float *)o; };
    const int64_t B = s.B, pmax = s.Pa > 2 * s.Pq ? s.Pa : 2 * s.Pq;
    d.hdr = take(4); d.scal = (double *)take(2 * NSC);
    d.y = take(B); d.logp = take(B); d.lpn = take(B); d.z = take(B * s.A); d.ones = take(B);
    d.xq = take(B * s.Dq); d.xpi = take(B * s.Dq); d.xn = take(B * s.Dq);
    d.outN = take(B * 2 * s.A); d.outP = take(B * 2 * s.A);
    d.hA = take(s.L * s.BH); d.hS = take(4 * s.L * s.BH); d.dH = take(2 * s.L * s.BH); d.dO = take(2 * B * 2 * MAX_A);
    d.qt = take(2 * B); d.q = take(2 * B); d.qpi = take(2 * B); d.dqda = take(2 * B * s.A);
    d.partial = take((int64_t)s.S * pmax);
    return at;
}

// the act call carves only what it uses
inline int64_t fill_work_act(Dev &d, void *base) {
    int64_t at = 0;
    char *b = (char *)base;
    auto take = [&at, b](int64_t floats) { char *o = b ? b + at : nullptr; at += (floats * 4 + 15) & ~(int64_t)15; return (float *)o; };
    d.outN = take(d.s.B * 2 * d.s.A);
    d.hS = take(d.s.L * d.s.BH);
    return at;
}

// ------------------------------------------------------------------------------------------------------------ the three GEMM jobs
// a launch's gate: null, or a flag in the learner's workspace - 0, or 1 + the optimiser step at which the learner stopped.  A gated launch
// of step `at` returns after one uniform read when the flag names an earlier step.  The wide PPO update's KL stop sets it
// (xarm_ppow_core.h); every other caller leaves the job header's gate null, and the kernels then read nothing
struct Gate { const int *stop; int64_t at; };
XARM_HD bool gate_shut(const Gate &g) {
    if (g.stop == nullptr) return false;
    const int f = g.stop[0];
    return f != 0 && (int64_t)f <= g.at;
}

struct FwdJob { const float *x, *W, *b; float *out; int K, N, act, vec; };                 // out [B, N] = act(x [B, K] W^T + b)
struct Fwd { int64_t B; int nj, maxN; FwdJob j[4]; Gate gate; };
struct BdJob { const float *d, *W, *h; float *out, *out2; int K, ldw, c0, N, mode, vec; }; // out [B, N] = (d [B, K] W[:, c0 : c0 + N]) dact(h); out2 nullable copy
struct Bd { int64_t B; int nj, maxN; BdJob j[2]; Gate gate; };
struct WgJob { const float *d, *x; int N, K; int64_t poff, boff; };                         // range s: partial[s][poff + j K + i], partial[s][boff + j]
struct Wg { int nj, S, maxN, maxK; int64_t pstride; float *partial; int64_t rows[MAX_SPLIT + 1]; WgJob j[2 * (MAX_L + 1)]; Gate gate; };

XARM_HD float act_f(int act, float x) { return act == ACT_RELU ? (x > 0.0f ? x : 0.0f) : (act == ACT_TANH ? xpol::tanh_f(x) : x); }
XARM_HD float dact_f(int act, float h) { return act == ACT_RELU ? (h > 0.0f ? 1.0f : 0.0f) : fma32(-h, h, 1.0f); }
XARM_HD float delta_f(int mode, float pre, float h) { return mode == ACT_NONE ? pre : pre * dact_f(mode, h); }

struct TowerRef { float *const *p; int Din, nout; };

inline int vec_ok(const void *a, const void *b, int K) { return (K % 8 == 0 && (((uintptr_t)a | (uintptr_t)b) & 15u) == 0) ? 1 : 0; }

// layer by layer: tower T[j] on in[j] [B, Din]; hidden layer l of job j goes to hid[j] + l B H, the outputs to out[j] [B, nout]
template <class X> void fwd_pass(const Shape &s, X &ex, int nj, const TowerRef *T, const float *const *in, float *const *hid, float *const *out,
                                 Gate gate = Gate{nullptr, 0}) {
    for (int l = 0; l < s.NL; l++) {
        Fwd f = {};
        f.B = s.B; f.nj = nj; f.gate = gate;
        for (int j = 0; j < nj; j++) {
            FwdJob &a = f.j[j];
            a.x = l == 0 ? in[j] : hid[j] + (l - 1) * s.BH;
            a.W = T[j].p[2 * l]; a.b = T[j].p[2 * l + 1];
            a.out = l == s.NL - 1 ? out[j] : hid[j] + l * s.BH;
            a.K = in_of(s, l, T[j].Din); a.N = out_of(s, l, T[j].nout); a.act = l == s.NL - 1 ? ACT_NONE : s.act;
            a.vec = vec_ok(a.x, a.W, a.K);
            if (a.N > f.maxN) f.maxN = a.N;
        }
        ex.fwd(f);
    }
}

// the hidden deltas of tower T[j] from its output deltas dO[j] [B, nout]: layer l's go to dH[j] + l B H
template <class X> void bd_pass(const Shape &s, X &ex, int nj, const TowerRef *T, const float *const *dO, float *const *hid, float *const *dH,
                                Gate gate = Gate{nullptr, 0}) {
    for (int l = s.L - 1; l >= 0; l--) {
        Bd f = {};
        f.B = s.B; f.nj = nj; f.maxN = s.H; f.gate = gate;
        for (int j = 0; j < nj; j++) {
            BdJob &a = f.j[j];
            a.d = l + 1 == s.NL - 1 ? dO[j] : dH[j] + (l + 1) * s.BH;
            a.K = out_of(s, l + 1, T[j].nout); a.W = T[j].p[2 * (l + 1)]; a.ldw = s.H; a.c0 = 0;
            a.h = hid[j] + l * s.BH; a.out = dH[j] + l * s.BH; a.out2 = nullptr; a.N = s.H; a.mode = s.act;
            a.vec = vec_ok(a.d, a.d, a.K);
        }
        ex.bd(f);
    }
}

// every layer's weight and bias gradient of towers T[j] in one launch; tower j's slice starts at base[j] of a range's partial
template <class X> void wg_pass(const Shape &s, float *partial, X &ex, int nj, const TowerRef *T, const float *const *in, const float *const *dO,
                                float *const *hid, float *const *dH, const int64_t *base, const int *t0, int64_t pstride, Gate gate = Gate{nullptr, 0}) {
    Wg f = {};
    f.S = s.S; f.pstride = pstride; f.partial = partial; f.gate = gate;
    for (int k = 0; k <= MAX_SPLIT; k++) f.rows[k] = s.rows[k];
    for (int j = 0; j < nj; j++)
        for (int l = 0; l < s.NL; l++) {
            WgJob &a = f.j[f.nj++];
            a.d = l == s.NL - 1 ? dO[j] : dH[j] + l * s.BH;
            a.x = l == 0 ? in[j] : hid[j] + (l - 1) * s.BH;
            a.N = out_of(s, l, T[j].nout); a.K = in_of(s, l, T[j].Din);
            a.poff = base[j] + s.off[t0[j] + 2 * l] - s.off[t0[j]];
            a.boff = base[j] + s.off[t0[j] + 2 * l + 1] - s.off[t0[j]];
            if (a.N > f.maxN) f.maxN = a.N;
            if (a.K > f.maxK) f.maxK = a.K;
        }
    ex.wg(f);
}

// ------------------------------------------------------------------------------------------------------------ the rows' parts
// the z of row n: the supplied tensor, or Philox (stream 0: z_pi, 1: z_next)
XARM_HD void row_noise(const Hyper &h, const float *given, int64_t n, int64_t counter, int stream, int A, float (&z)[MAX_A]) {
#pragma unroll
    for (int b = 0; b < MAX_A / 4; b++) {
        float q[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        if (given == nullptr && 4 * b < A) xsac::noise4(h.seed, n, counter, stream, b, q);
#pragma unroll
        for (int m = 0; m < 4; m++) {
            const int c = 4 * b + m;
            z[c] = 0.0f;
            if (c < A) z[c] = given != nullptr ? given[n * A + c] : q[m];
        }
    }
}

// behind the actor's two forwards: both squashed Gaussians of row n, the rows obs | action, obs | a_pi and next_obs | a'
XARM_HD void head_row(const Dev &d, int64_t n, int64_t t0) {
    const int D = d.s.D, A = d.s.A, Dq = d.s.Dq;
    float z[MAX_A], a[MAX_A];
    row_noise(d.h, d.noise_next, n, t0, 1, A, z);
    d.lpn[n] = xsac::actor_head(A, d.outN + n * 2 * A, 1, z, false, a);
    for (int j = 0; j < D; j++) d.xn[n * Dq + j] = d.next_obs[n * D + j];
#pragma unroll
    for (int c = 0; c < MAX_A; c++)
        if (c < A) d.xn[n * Dq + D + c] = a[c];
    row_noise(d.h, d.noise_pi, n, t0, 0, A, z);
    d.logp[n] = xsac::actor_head(A, d.outP + n * 2 * A, 1, z, false, a);
    for (int j = 0; j < D; j++) {
        const float x = d.obs[n * D + j];
        d.xq[n * Dq + j] = x;
        d.xpi[n * Dq + j] = x;
    }
#pragma unroll
    for (int c = 0; c < MAX_A; c++)
        if (c < A) {
            d.xq[n * Dq + D + c] = d.action[n * A + c];
            d.xpi[n * Dq + D + c] = a[c];
            d.z[n * A + c] = z[c];
        }
    d.ones[n] = 1.0f;
}

XARM_HD void head_first(const Dev &d, int64_t t0) {
    xopt::adam_scalars(d.h.adam, t0 + 1, d.hdr);
    d.hdr[2] = xsac::alpha_of(d.h, d.w[d.s.NT - 1]);
    d.hdr[3] = 0.0f;
}

// behind the targets' and the critics' forwards: y, the critics' output deltas (q - y) use, four sums
XARM_HD void crit_row(const Dev &d, int64_t n, double *sums) {
    const int64_t B = d.s.B;
    const float u = d.use != nullptr ? d.use[n] : 1.0f, lp = d.logp[n];
    const float y = xsac::target_row(d.h.gamma, d.hdr[2], d.reward[n], d.done[n], d.qt[n], d.qt[B + n], d.lpn[n]);
    d.y[n] = y;
    if (d.out_target != nullptr) d.out_target[n] = y;
    sums[0] += (double)u;
    sums[1] += (double)(lp * u);
    sums[2] += (double)((lp + d.h.target_entropy) * u);
    for (int i = 0; i < 2; i++) {
        const float q = d.q[i * B + n], diff = q - y;
        d.dO[i * B + n] = diff * u;
        if (d.out_q != nullptr) d.out_q[i * B + n] = q;
        sums[3] += (double)(diff * diff * u);
    }
}

// behind dq/da: the actor's output deltas [B, 2 A] at dO, two sums
XARM_HD void pi_row(const Dev &d, int64_t n, double *sums) {
    const int64_t B = d.s.B;
    const int A = d.s.A;
    const float u = d.use != nullptr ? d.use[n] : 1.0f, alpha = d.hdr[2];
    const float qa = d.qpi[n], qb = d.qpi[B + n];
    const bool second = qb < qa;
    const float qm = second ? qb : qa;
    float out[2 * MAX_A];
#pragma unroll
    for (int c = 0; c < 2 * MAX_A; c++) out[c] = c < 2 * A ? d.outP[n * 2 * A + c] : 0.0f;
    xsac::actor_deltas(A, out, 1, d.z + n * A, alpha, d.dqda + ((second ? B : 0) + n) * A, u);
#pragma unroll
    for (int c = 0; c < 2 * MAX_A; c++)
        if (c < 2 * A) d.dO[n * 2 * A + c] = out[c];
    const float ent = alpha * d.logp[n];
    sums[4] += (double)((ent - qm) * u);
    sums[5] += (double)(qm * u);
}

XARM_HD double n_use_of(const Dev &d) { return xopt::n_use(d.scal[0]); }

// trained parameter p of the flat order, its ranges' partials at part[s pstride]: reduce, Adam, and with `targets` the Polyak step
XARM_HD void apply_param(const Dev &d, int64_t p, const float *part, int64_t pstride, bool targets) {
    const Shape &s = d.s;
    const float gf = (float)(xopt::slice_sum(part, s.S, pstride) / n_use_of(d));
    if (d.out_grad != nullptr) d.out_grad[p] = gf;
    const int i = xopt::tensor_at(s.off, 0, s.NT, p);
    const int64_t e = p - s.off[i];
    const float sc[2] = {d.hdr[0], d.hdr[1]};
    float m = d.m[i][e], v = d.v[i][e], w = d.w[i][e];
    xopt::adam(d.h.adam, sc, gf, m, v, w);
    d.m[i][e] = m;
    d.v[i][e] = v;
    d.w[i][e] = w;
    if (targets) d.tq[i - s.tp][e] = xsac::polyak(d.h, d.tq[i - s.tp][e], w);
}

// the call's last writes: xsac::finish on this step's sums
XARM_HD void finish(const Dev &d) {
    const int la = d.s.NT - 1;
    xsac::finish(d.h, d.hdr, d.hdr[2], n_use_of(d), d.scal[2], d.scal[3], d.scal[4], d.scal[1], d.scal[5], d.w[la], d.m[la], d.v[la],
                 d.out_grad != nullptr ? d.out_grad + (d.s.P - 1) : nullptr, d.out_stats, d.step);
}

// the act call's row: noise as xarm_sac_act draws it
XARM_HD void act_row(const Dev &d, int64_t n) {
    const int A = d.s.A;
    const bool det = d.h.deterministic != 0;
    const int64_t calls = det ? 0 : d.calls[0];
    float z[MAX_A], a[MAX_A];
#pragma unroll
    for (int b = 0; b < MAX_A / 4; b++) {
        float q[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        if (!det && 4 * b < A) xpol::noise4(d.h.seed, d.s.row_offset + n, calls, b, q);
#pragma unroll
        for (int m = 0; m < 4; m++) z[4 * b + m] = q[m];
    }
    const float lp = xsac::actor_head(A, d.outN + n * 2 * A, 1, z, det, a);
#pragma unroll
    for (int c = 0; c < MAX_A; c++)
        if (c < A) d.out_action[n * A + c] = a[c];
    if (d.out_logp != nullptr) d.out_logp[n] = lp;
}

// ------------------------------------------------------------------------------------------------------------ the chain
constexpr int launches(int n_hidden) { return 6 * n_hidden + 11; }
constexpr int act_launches(int n_hidden) { return n_hidden + 2; }   // + the tick of a stochastic call

// one SAC step: 6 L + 11 launches of `ex`, the same for every batch and for a fixed or trained entropy coefficient
//   L + 1  the actor on next_obs and on obs (two jobs a launch)            1  head: a', logp', a_pi, logp_pi, the rows
//   L + 1  both targets on next_obs | a', both critics on obs | action     1  crit: y, (q - y) use, n_use
//   L      the critics' hidden deltas    1  their weight gradients         1  critics: reduce, Adam, Polyak
//   L + 1  the STEPPED critics on obs | a_pi   L + 1  their deltas from d = 1 down to dq/da
//   1      pi: the actor's output deltas       L  its hidden deltas   1  its weight gradients   1  actor: reduce, Adam; log_alpha, stats, step
template <class X> void run_update(const Dev &d, X &ex) {
    const Shape &s = d.s;
    const int tp = s.tp;
    const TowerRef actor = {d.w, s.D, 2 * s.A}, q1 = {d.w + tp, s.Dq, 1}, q2 = {d.w + 2 * tp, s.Dq, 1}, q1t = {d.tq, s.Dq, 1}, q2t = {d.tq + tp, s.Dq, 1};
    float *hs[4] = {d.hS, d.hS + s.L * s.BH, d.hS + 2 * s.L * s.BH, d.hS + 3 * s.L * s.BH};
    float *dh[2] = {d.dH, d.dH + s.L * s.BH};
    {
        const TowerRef T[2] = {actor, actor};
        const float *in[2] = {d.next_obs, d.obs};
        float *hid[2] = {hs[0], d.hA}, *out[2] = {d.outN, d.outP};
        fwd_pass(s, ex, 2, T, in, hid, out);
    }
    ex.head(d);
    {
        const TowerRef T[4] = {q1t, q2t, q1, q2};
        const float *in[4] = {d.xn, d.xn, d.xq, d.xq};
        float *hid[4] = {hs[0], hs[1], hs[2], hs[3]}, *out[4] = {d.qt, d.qt + s.B, d.q, d.q + s.B};
        fwd_pass(s, ex, 4, T, in, hid, out);
    }
    ex.crit(d);
    {
        const TowerRef T[2] = {q1, q2};
        const float *in[2] = {d.xq, d.xq}, *dO[2] = {d.dO, d.dO + s.B};
        float *hid[2] = {hs[2], hs[3]};
        const int64_t base[2] = {0, s.Pq};
        const int t0[2] = {tp, 2 * tp};
        bd_pass(s, ex, 2, T, dO, hid, dh);
        wg_pass(s, d.partial, ex, 2, T, in, dO, hid, dh, base, t0, 2 * s.Pq);
    }
    ex.apply(d, s.Pa, 2 * s.Pq, 2 * s.Pq, true, false);
    {
        const TowerRef T[2] = {q1, q2};
        const float *in[2] = {d.xpi, d.xpi}, *dO[2] = {d.ones, d.ones};
        float *hid[2] = {hs[0], hs[1]}, *out[2] = {d.qpi, d.qpi + s.B};
        fwd_pass(s, ex, 2, T, in, hid, out);
        bd_pass(s, ex, 2, T, dO, hid, dh);
        Bd f = {};
        f.B = s.B; f.nj = 2; f.maxN = s.A;
        for (int j = 0; j < 2; j++) {
            BdJob &a = f.j[j];
            a.d = dh[j]; a.K = s.H; a.W = T[j].p[0]; a.ldw = s.Dq; a.c0 = s.D; a.h = nullptr; a.out = d.dqda + j * s.B * s.A;
            a.out2 = d.out_dqda ? d.out_dqda + j * s.B * s.A : nullptr; a.N = s.A; a.mode = ACT_NONE; a.vec = vec_ok(a.d, a.d, a.K);
        }
        ex.bd(f);
    }
    ex.pi(d);
    {
        const TowerRef T[1] = {actor};
        const float *in[1] = {d.obs}, *dO[1] = {d.dO};
        float *hid[1] = {d.hA};
        const int64_t base[1] = {0};
        const int t0[1] = {0};
        bd_pass(s, ex, 1, T, dO, hid, dh);
        wg_pass(s, d.partial, ex, 1, T, in, dO, hid, dh, base, t0, s.Pa);
    }
    ex.apply(d, 0, s.Pa, s.Pa, false, true);
}

// the act call: the update's own forward on obs, then the head
template <class X> void run_act(const Dev &d, X &ex) {
    const TowerRef T[1] = {{d.w, d.s.D, 2 * d.s.A}};
    const float *in[1] = {d.obs};
    float *hid[1] = {d.hS}, *out[1] = {d.outN};
    fwd_pass(d.s, ex, 1, T, in, hid, out);
    ex.act(d);
}

#if !defined(__HIPCC__) || defined(XARM_HOST_BUILD)
// ---- the host build: the same jobs with plain loops (inner loops run over independent outputs, each output's chain in the stated order)
struct HostExec {
    static float pad(int n, float acc) { return (n & 1) ? fma32(0.0f, 0.0f, acc) : acc; }
    void fwd(const Fwd &f) {
        if (gate_shut(f.gate)) return;
        for (int jn = 0; jn < f.nj; jn++) {
            const FwdJob &a = f.j[jn];
            std::vector<float> Wt((size_t)a.K * a.N), acc((size_t)a.N);
            for (int u = 0; u < a.N; u++)
                for (int k = 0; k < a.K; k++) Wt[(size_t)k * a.N + u] = a.W[(size_t)u * a.K + k];
            for (int64_t n = 0; n < f.B; n++) {
                for (int u = 0; u < a.N; u++) acc[u] = a.b[u];
                for (int k = 0; k < a.K; k++) {
                    const float x = a.x[n * a.K + k];
                    const float *wr = &Wt[(size_t)k * a.N];
                    for (int u = 0; u < a.N; u++) acc[u] = fma32(x, wr[u], acc[u]);
                }
                for (int u = 0; u < a.N; u++) a.out[n * a.N + u] = act_f(a.act, pad(a.K, acc[u]));
            }
        }
    }
    void bd(const Bd &f) {
        if (gate_shut(f.gate)) return;
        for (int jn = 0; jn < f.nj; jn++) {
            const BdJob &a = f.j[jn];
            std::vector<float> acc((size_t)a.N);
            for (int64_t n = 0; n < f.B; n++) {
                for (int i = 0; i < a.N; i++) acc[i] = 0.0f;
                for (int k = 0; k < a.K; k++) {
                    const float dv = a.d[n * a.K + k];
                    const float *wr = a.W + (size_t)k * a.ldw + a.c0;
                    for (int i = 0; i < a.N; i++) acc[i] = fma32(dv, wr[i], acc[i]);
                }
                for (int i = 0; i < a.N; i++) {
                    const float o = delta_f(a.mode, pad(a.K, acc[i]), a.h ? a.h[n * a.N + i] : 0.0f);
                    a.out[n * a.N + i] = o;
                    if (a.out2) a.out2[n * a.N + i] = o;
                }
            }
        }
    }
    void wg(const Wg &f) {
        if (gate_shut(f.gate)) return;
        for (int jn = 0; jn < f.nj; jn++) {
            const WgJob &a = f.j[jn];
            for (int sp = 0; sp < f.S; sp++) {
                float *pw = f.partial + (int64_t)sp * f.pstride + a.poff, *pb = f.partial + (int64_t)sp * f.pstride + a.boff;
                for (int64_t e = 0; e < (int64_t)a.N * a.K; e++) pw[e] = 0.0f;
                for (int j = 0; j < a.N; j++) pb[j] = 0.0f;
                const int64_t n0 = f.rows[sp], n1 = f.rows[sp + 1];
                for (int64_t n = n0; n < n1; n++)
                    for (int j = 0; j < a.N; j++) {
                        const float dv = a.d[n * a.N + j];
                        const float *xr = a.x + n * a.K;
                        float *o = pw + (int64_t)j * a.K;
                        for (int i = 0; i < a.K; i++) o[i] = fma32(dv, xr[i], o[i]);
                        pb[j] = fma32(dv, 1.0f, pb[j]);
                    }
                const int cnt = (int)((n1 - n0) & 1);
                for (int64_t e = 0; e < (int64_t)a.N * a.K; e++) pw[e] = pad(cnt, pw[e]);
                for (int j = 0; j < a.N; j++) pb[j] = pad(cnt, pb[j]);
            }
        }
    }
    template <class F> static void rows(const Dev &d, int first, int count, F f) {
        double tot[NSC] = {0.0};
        for (int t = 0; t < RED; t++) {
            double sums[NSC] = {0.0};
            for (int64_t n = t; n < d.s.B; n += RED) f(n, sums);
            for (int i = 0; i < NSC; i++) tot[i] += sums[i];
        }
        for (int i = first; i < first + count; i++) d.scal[i] = tot[i];
    }
    void head(const Dev &d) {
        const int64_t t0 = d.step[0];
        head_first(d, t0);
        for (int64_t n = 0; n < d.s.B; n++) head_row(d, n, t0);
    }
    void crit(const Dev &d) { rows(d, 0, 4, [&d](int64_t n, double *s) { crit_row(d, n, s); }); }
    void pi(const Dev &d) { rows(d, 4, 2, [&d](int64_t n, double *s) { pi_row(d, n, s); }); }
    void apply(const Dev &d, int64_t p0, int64_t count, int64_t pstride, bool targets, bool last) {
        for (int64_t e = 0; e < count; e++) apply_param(d, p0 + e, d.partial + e, pstride, targets);
        if (last) finish(d);
    }
    void act(const Dev &d) {
        for (int64_t n = 0; n < d.s.B; n++) act_row(d, n);
        if (!d.h.deterministic) d.calls[0] += 1;
    }
};
#endif

#if defined(__HIPCC__) && !defined(XARM_HOST_BUILD)
// the launches of one step / one act call on `stream` (xarm_k_sacw.hip); returns the launches' hipError_t
int launch_update(const Dev &d, void *stream);
int launch_act(const Dev &d, void *stream);
#endif

}  // namespace xsacw
