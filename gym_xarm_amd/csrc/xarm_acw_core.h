// xarm_acw_core.h - wide device-resident MlpPolicy: the act call of xarm_policy_core.h for train.py's
// ActorCritic(net_arch, activation) with equal-width towers of two or three hidden layers of 64, 128, 192 or 256 units, tanh or ReLU.
// At these widths a layer's weights do not fit a CU's LDS, so the fused 32-row tile of xarm_k_policy.hip does not carry over: the call is
// a CHAIN of launches with the activations in a workspace, as in xarm_sacw_core.h, whose forward job (Fwd), pass (fwd_pass), activation
// (act_f) and host loops (HostExec::fwd) this file CALLS.  It states the chain (run_act) and the two per-row functions once;
// xarm_k_acw.hip executes them on the device and the host build (g++ -DXARM_HOST_BUILD -ffp-contract=off, tests/hostbuild_acw/) with
// plain loops over the same workspace, so everything the call writes - the workspace included - is equal between them bit for bit.
//
//   prep     x[n][j] = xpol::input_at: column j of observation | achieved_goal | desired_goal, normalised with the frozen statistics
//            when they are given.  Always run: the GEMM then reads one contiguous 16-byte aligned [B, D] tensor whatever the caller has.
//   forward  xsacw::fwd_pass over two jobs, pi and vf (one job when out_value is null): L + 1 launches
//   head     per row: the Philox draw (xpol::noise4 keyed by seed, row_offset + n, calls, column block), xpol::finish_column per column,
//            logp added in column order, value copied out
//   tick     a stochastic call advances calls behind the head
#pragma once
#include "xarm_sacw_core.h"

namespace xacw {

using xpol::MAX_ACT;
using xsacw::TP;

struct Dev {
    xsacw::Shape s;                 // B, H, L, NL, BH, act, D, A: what fwd_pass reads
    xpol::Args a;                   // rows, seed, statistics, the three row pointers, the four outputs (all nullable here)
    float *pi[TP], *vf[TP];
    int nj;                         // 2 with the value tower, else 1
    float *x, *hid, *mean, *val;    // the workspace: x [B, D], hidden activations [2][L][B, H], mean [B, A], value [B]
};

inline xarm_policy_layout policy_layout_of(const xarm_acw_layout *l) {
    const xarm_policy_layout p = {l->num_rows, l->obs_dim, l->goal_dim, l->act_dim, xpol::HID, l->row_offset};
    return p;
}

inline const char *layout_error(const xarm_acw_layout *l) {
    if (!l) return "layout is NULL";
    const xarm_policy_layout p = policy_layout_of(l);
    if (const char *why = xpol::layout_error(&p)) return why;       // num_rows is the policy ABI's num_envs
    if (const char *why = xsacw::towers_error(l->hidden, l->n_hidden, l->activation)) return why;
    return nullptr;
}

inline const char *pointer_error(const xarm_acw_layout *l, const xarm_policy_params *p, const xarm_acw_weights *w, const int64_t *calls,
                                 const float *obs, const float *ag, const float *dg, const void *workspace, const float *value) {
    if (!w) return "weights is NULL";
    const int tp = 2 * (l->n_hidden + 1);
    if (const char *why = xsacw::tower_error(w->pi, tp)) return why;
    if (!w->log_std) return "NULL log_std";
    if (value)
        if (const char *why = xsacw::tower_error(w->vf, tp)) return why;
    if (!p->deterministic && !calls) return "NULL calls with a stochastic call";
    if (!obs || (l->goal_dim > 0 && (!ag || !dg))) return "NULL observation pointer";
    return xsacw::workspace_error(workspace);
}

inline void fill_shape(Dev &d, const xarm_acw_layout *l) {
    xsacw::Shape &s = d.s;
    s.B = l->num_rows; s.D = l->obs_dim + 2 * l->goal_dim; s.A = l->act_dim; s.H = l->hidden; s.L = l->n_hidden; s.NL = s.L + 1;
    s.act = l->activation; s.row_offset = l->row_offset; s.tp = 2 * s.NL; s.BH = s.B * s.H;
}

// carve the workspace (each part 16-byte aligned); returns its size in bytes.  base may be null (size only)
inline int64_t fill_work(Dev &d, void *base) {
    const xsacw::Shape &s = d.s;
    int64_t at = 0;
    char *b = (char *)base;
    auto take = [&at, b](int64_t floats) { char *o = b ? b + at : nullptr; at += (floats * 4 + 15) & ~(int64_t)15; return (float *)o; };
    d.x = take(s.B * s.D); d.hid = take(2 * s.L * s.BH); d.mean = take(s.B * s.A); d.val = take(s.B);
    return at;
}

inline void fill_dev(Dev &d, const xarm_acw_layout *l, const xarm_policy_params *p, const xarm_acw_weights *w, const double *stats, int64_t *calls,
                     const float *obs, const float *ag, const float *dg, void *workspace, float *action, float *env_action, float *logp, float *value) {
    fill_shape(d, l);
    const xarm_policy_layout pl = policy_layout_of(l);
    xarm_policy_weights none = {};
    none.log_std = w->log_std;
    xpol::fill_args(d.a, &pl, p, &none);
    d.a.stats = stats; d.a.calls = calls; d.a.x0 = obs; d.a.x1 = ag; d.a.x2 = dg;
    d.a.action = action; d.a.env_action = env_action; d.a.logp = logp; d.a.value = value;
    d.nj = value != nullptr ? 2 : 1;
    for (int i = 0; i < d.s.tp; i++) { d.pi[i] = const_cast<float *>(w->pi[i]); d.vf[i] = const_cast<float *>(w->vf[i]); }
    fill_work(d, workspace);
}

// ------------------------------------------------------------------------------------------------------------ the rows' parts
XARM_HD void prep_at(const Dev &d, int64_t n, int j) { d.x[n * d.a.D + j] = xpol::input_at(d.a, n, j); }

// behind the forward: xpol::row's columns on the mean of the workspace
XARM_HD void head_row(const Dev &d, int64_t n) {
    const xpol::Args &a = d.a;
    const int A = a.A;
    const bool det = a.deterministic != 0;
    const int64_t calls = det ? 0 : a.calls[0];
    float lp = 0.0f;
#pragma unroll
    for (int b = 0; b < MAX_ACT / 4; b++) {
        float z[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        if (!det && 4 * b < A) xpol::noise4(a.seed, a.row_offset + n, calls, b, z);
#pragma unroll
        for (int m = 0; m < 4; m++) {
            const int c = 4 * b + m;
            if (c < A) {
                float act, env;
                const float t = xpol::finish_column(d.mean[n * A + c], a.log_std[c], z[m], det, act, env);
                lp = c == 0 ? t : lp + t;
                if (a.action != nullptr) a.action[n * A + c] = act;
                if (a.env_action != nullptr) a.env_action[n * A + c] = env;
            }
        }
    }
    if (a.logp != nullptr) a.logp[n] = lp;
    if (a.value != nullptr) a.value[n] = d.val[n];
}

// ------------------------------------------------------------------------------------------------------------ the chain
constexpr int act_launches(int n_hidden) { return n_hidden + 3; }   // prep, L + 1 forward, head; + the tick of a stochastic call

template <class X> void run_act(const Dev &d, X &ex) {
    const xsacw::Shape &s = d.s;
    ex.prep(d);
    const xsacw::TowerRef T[2] = {{d.pi, s.D, s.A}, {d.vf, s.D, 1}};
    const float *in[2] = {d.x, d.x};
    float *hid[2] = {d.hid, d.hid + s.L * s.BH}, *out[2] = {d.mean, d.val};
    xsacw::fwd_pass(s, ex, d.nj, T, in, hid, out);
    ex.head(d);
}

#if !defined(__HIPCC__) || defined(XARM_HOST_BUILD)
struct HostExec : xsacw::HostExec {
    void prep(const Dev &d) {
        for (int64_t n = 0; n < d.s.B; n++)
            for (int j = 0; j < d.a.D; j++) prep_at(d, n, j);
    }
    void head(const Dev &d) {
        for (int64_t n = 0; n < d.s.B; n++) head_row(d, n);
        if (!d.a.deterministic) const_cast<int64_t *>(d.a.calls)[0] += 1;
    }
};
#endif

#if defined(__HIPCC__) && !defined(XARM_HOST_BUILD)
// the launches of one act call on `stream` (xarm_k_acw.hip); returns the launches' hipError_t
int launch_act(const Dev &d, int64_t *calls, void *stream);
#endif

}  // namespace xacw
