// xarm_policy_core.h - device-resident MlpPolicy: the forward of gym_xarm_amd/train.py's ActorCritic - two 64-64
// tanh towers, a state-independent log_std - with the Gaussian sample, the clamp, the log-probability and the value, as one
// stream-ordered call on the module's own parameter tensors.  The kernel is in xarm_k_policy.hip; like the normaliser core this
// also compiles for the host (g++ -DXARM_HOST_BUILD -ffp-contract=off, tests/hostbuild_policy/) for the CPU tests.  Every
// operation below is a float32 fmaf / + - * / sqrt, an integer or bit operation, or the float64 normalisation expression of
// xarm_norm_core.h, in an order this file fixes; no libm / ocml function is called.  Both builds are compiled with contraction
// off: the host build and the device agree bit for bit, and a row's result depends on that row, the weights, seed,
// row_offset + e and calls alone.
//
//   row      D = obs_dim + 2 goal_dim <= 96 columns through up to three row-major pointers observation | achieved_goal |
//            desired_goal (goal_dim 0: one flat pointer) - xarm_norm_obs's convention
//   stats    nullable double [2 D + 4] in the normaliser's layout.  Set: column j enters the network as
//            xnorm::norm_value(x, mean_j, sqrt(var_j + eps), clip_obs) - frozen statistics.  Null: the row is taken as it is.
//   tower    h1 = tanh(W1 x + b1), h2 = tanh(W2 h1 + b2), out = W3 h2 + b3; W in nn.Linear's [out, in] layout, hidden width 64.
//            Every dot product is a float32 fmaf chain that starts from the bias.  Layer 1 runs over the columns in natural
//            order 0, 1, 2, ... (an odd D is padded with one zero operand: fmaf(0, 0, acc) leaves acc's bits alone, and the host
//            does the same).  Layers 2 and 3 run over the hidden units in the order KORD below.
//   noise    Philox(seed; row_offset + e, calls, TAG + column block b): the draw's four words give two Box-Muller pairs, the
//            columns 4b .. 4b + 3.  Uniforms are ((word >> 8) + 1) 2^-24 in (0, 1]: log is finite and |z| <= sqrt(48 ln 2) < 5.77.
//   outputs  action = fmaf(exp(log_std), z, mean) (mean when deterministic: z = 0), env_action = action clamped to [-1, 1],
//            logp = sum over columns, in column order, of ((-0.5 z z) - log_std) - log(2 pi) / 2, value.  logp and value may be
//            null; a null value skips the value tower.
//
// KORD is the order in which v_mfma_f32_32x32x2_f32 consumes a 32x32 accumulator tile as its next B operand with no lane
// movement.  With the batch row on the lane (column j = lane & 31) and the unit in the accumulator (row i), register r of lane
// half h = lane >> 5 holds unit 32 t + 8 (r >> 2) + 4 h + (r & 3) of tile t.  One MFMA takes one k per lane half and adds half
// 0's product first, so step (t, r) contributes unit 32 t + 8 (r >> 2) + (r & 3), then that unit + 4:
//   0 4 1 5 2 6 3 7 | 8 12 9 13 10 14 11 15 | 16 20 ... | 56 60 57 61 58 62 59 63
#pragma once
#include <stdint.h>
#include "xarm_core.h"
#include "xarm_norm_core.h"

namespace xpol {

constexpr int HID = 64;                      // hidden width (XARM_POLICY_HIDDEN)
constexpr int MAX_DIM = XARM_POLICY_MAX_DIM; // 96
constexpr int MAX_ACT = XARM_POLICY_MAX_ACT; // 16
constexpr int TILE = 32;                     // rows per wavefront
constexpr uint32_t PHILOX_TAG = 0x504F4C00u; // "POL\0"

// the k order of a 64-wide layer (layers 2 and 3)
constexpr int KORD[HID] = {0, 4, 1, 5, 2, 6, 3, 7, 8, 12, 9, 13, 10, 14, 11, 15, 16, 20, 17, 21, 18, 22, 19, 23, 24, 28, 25, 29, 26, 30, 27, 31,
                           32, 36, 33, 37, 34, 38, 35, 39, 40, 44, 41, 45, 42, 46, 43, 47, 48, 52, 49, 53, 50, 54, 51, 55, 56, 60, 57, 61, 58, 62, 59, 63};
// unit held by accumulator register r of lane half h in tile t
constexpr int unit_of(int t, int r, int h) { return 32 * t + 8 * (r >> 2) + 4 * h + (r & 3); }
constexpr bool kord_matches_mfma() {
    for (int t = 0; t < 2; t++)
        for (int r = 0; r < 16; r++)
            for (int h = 0; h < 2; h++)
                if (KORD[2 * (16 * t + r) + h] != unit_of(t, r, h)) return false;
    return true;
}
static_assert(kord_matches_mfma(), "KORD must be the accumulator order of v_mfma_f32_32x32x2_f32");

struct Tower {
    const float *W1, *b1, *W2, *b2, *W3, *b3;
};

struct Args {
    int64_t E, row_offset;
    int obs, goal, D, A;
    uint64_t seed;
    double clip_obs, eps;
    int deterministic;
    Tower pi, vf;
    const float *log_std;
    const double *stats;                 // nullable
    const int64_t *calls;                // read when not deterministic
    const float *x0, *x1, *x2;           // observation | achieved_goal | desired_goal (x1 / x2 unused when goal == 0)
    float *action, *env_action, *logp, *value;   // logp / value nullable
};

// null when the layout is usable, else what is wrong with it
inline const char *layout_error(const xarm_policy_layout *l) {
    if (!l) return "layout is NULL";
    if (l->num_envs < 0) return "num_envs must be >= 0";
    if (l->obs_dim < 1) return "obs_dim must be >= 1";
    if (l->goal_dim < 0) return "goal_dim must be >= 0";
    if (l->obs_dim > MAX_DIM || l->goal_dim > MAX_DIM || l->obs_dim + 2 * l->goal_dim > MAX_DIM)
        return "obs_dim + 2 goal_dim must be <= XARM_POLICY_MAX_DIM (96)";
    if (l->act_dim < 1 || l->act_dim > MAX_ACT) return "act_dim must lie in [1, XARM_POLICY_MAX_ACT (16)]";
    if (l->hidden != HID) return "hidden must be XARM_POLICY_HIDDEN (64)";
    if (l->row_offset < 0) return "row_offset must be >= 0";
    return nullptr;
}

inline const char *params_error(const xarm_policy_params *p, bool with_stats) {
    if (!p) return "params is NULL";
    if (!with_stats) return nullptr;
    if (!(p->eps > 0.0) || !(p->eps < 1e300)) return "eps must be finite and > 0";
    if (!(p->clip_obs > 0.0)) return "clip_obs must be > 0";
    return nullptr;
}

// the pointers a call with these arguments reads or writes; null when all are there
inline const char *pointer_error(const xarm_policy_layout *l, const xarm_policy_params *p, const xarm_policy_weights *w, const int64_t *calls,
                                 const float *obs, const float *ag, const float *dg, const float *action, const float *env_action,
                                 const float *value) {
    if (!w) return "weights is NULL";
    if (!w->pi_w1 || !w->pi_b1 || !w->pi_w2 || !w->pi_b2 || !w->pi_w3 || !w->pi_b3 || !w->log_std) return "NULL policy weight pointer";
    if (value && (!w->vf_w1 || !w->vf_b1 || !w->vf_w2 || !w->vf_b2 || !w->vf_w3 || !w->vf_b3)) return "NULL value weight pointer with out_value set";
    // b1, W2, b2 and W3 are read in 16-byte pieces
    if ((((uintptr_t)w->pi_b1 | (uintptr_t)w->pi_w2 | (uintptr_t)w->pi_b2 | (uintptr_t)w->pi_w3) & 15u) != 0 ||
        (value && (((uintptr_t)w->vf_b1 | (uintptr_t)w->vf_w2 | (uintptr_t)w->vf_b2 | (uintptr_t)w->vf_w3) & 15u) != 0))
        return "b1, W2, b2 and W3 must be 16-byte aligned";
    if (!p->deterministic && !calls) return "NULL calls with a stochastic call";
    if (!obs || (l->goal_dim > 0 && (!ag || !dg))) return "NULL observation pointer";
    if (!action || !env_action) return "NULL out_action / out_env_action";
    return nullptr;
}

inline void fill_args(Args &a, const xarm_policy_layout *l, const xarm_policy_params *p, const xarm_policy_weights *w) {
    a.E = l->num_envs; a.row_offset = l->row_offset; a.obs = l->obs_dim; a.goal = l->goal_dim; a.D = l->obs_dim + 2 * l->goal_dim;
    a.A = l->act_dim; a.seed = p->seed; a.clip_obs = p->clip_obs; a.eps = p->eps; a.deterministic = p->deterministic != 0;
    a.pi = Tower{w->pi_w1, w->pi_b1, w->pi_w2, w->pi_b2, w->pi_w3, w->pi_b3};
    a.vf = Tower{w->vf_w1, w->vf_b1, w->vf_w2, w->vf_b2, w->vf_w3, w->vf_b3};
    a.log_std = w->log_std;
}

// ---------------------------------------------------------------------------------------------- float32 elementary functions
// Coefficients: the single-precision Cephes library (S. Moshier, public domain).  Every step is spelled out, so that the host
// and the device run the same operations.
XARM_HD float f_from_bits(uint32_t u) { float f; __builtin_memcpy(&f, &u, 4); return f; }
XARM_HD uint32_t bits_of(float f) { uint32_t u; __builtin_memcpy(&u, &f, 4); return u; }
XARM_HD float fma32(float a, float b, float c) { return __builtin_fmaf(a, b, c); }

// e^x for x clamped to [-87, 88] (the result stays a normal float): n = round(x log2 e) by the 1.5 2^23 shift, r = x - n ln 2 in
// two parts, e^r = 1 + r + r^2 P(r) on |r| <= 0.347, scaled by 2^n through the exponent bits.  About 1 ulp.
XARM_HD float exp_f(float x) {
    x = x < -87.0f ? -87.0f : (x > 88.0f ? 88.0f : x);
    const float t = fma32(x, 1.44269504088896341f, 12582912.0f);
    const float nf = t - 12582912.0f;
    const int n = (int)(bits_of(t) & 0x7FFFFFu) - 0x400000;
    float r = fma32(nf, -0.693359375f, x);
    r = fma32(nf, 2.12194440e-4f, r);
    float p = 1.9875691500e-4f;
    p = fma32(p, r, 1.3981999507e-3f);
    p = fma32(p, r, 8.3334519073e-3f);
    p = fma32(p, r, 4.1665795894e-2f);
    p = fma32(p, r, 1.6666665459e-1f);
    p = fma32(p, r, 5.0000001201e-1f);
    const float rr = r * r;
    float y = fma32(p, rr, r);
    y = y + 1.0f;
    return y * f_from_bits((uint32_t)(n + 127) << 23);
}

// tanh: the odd polynomial x + x z P(z), z = x^2, below 0.625; above, 1 - 2 / (e^(2 |x|) + 1) with |x| clamped to 10 (tanh is 1 to
// float32 from 9.02 on) and the sign copied back
XARM_HD float tanh_f(float x) {
    const uint32_t b = bits_of(x);
    const float ax = f_from_bits(b & 0x7FFFFFFFu);
    if (ax < 0.625f) {
        const float z = x * x;
        float p = -5.70498872745e-3f;
        p = fma32(p, z, 2.06390887954e-2f);
        p = fma32(p, z, -5.37397155531e-2f);
        p = fma32(p, z, 1.33314422036e-1f);
        p = fma32(p, z, -3.33332819422e-1f);
        const float pz = p * z;
        return fma32(pz, x, x);
    }
    const float c = ax > 10.0f ? 10.0f : ax;
    const float e = exp_f(c + c);
    const float q = 2.0f / (e + 1.0f);
    const float r = 1.0f - q;
    return f_from_bits(bits_of(r) | (b & 0x80000000u));
}

// natural logarithm of a positive normal float: x = 2^e f with f in [sqrt(1/2), sqrt 2), log f = w - w^2 / 2 + w^3 P(w) with
// w = f - 1 (exact), plus e ln 2 in two parts
XARM_HD float log_f(float x) {
    const uint32_t b = bits_of(x);
    int e = (int)(b >> 23) - 127;
    float f = f_from_bits((b & 0x7FFFFFu) | 0x3F800000u);
    if (f > 1.41421356237f) { f = f * 0.5f; e = e + 1; }
    const float w = f - 1.0f;
    const float z = w * w;
    float p = 7.0376836292e-2f;
    p = fma32(p, w, -1.1514610310e-1f);
    p = fma32(p, w, 1.1676998740e-1f);
    p = fma32(p, w, -1.2420140846e-1f);
    p = fma32(p, w, 1.4249322787e-1f);
    p = fma32(p, w, -1.6668057665e-1f);
    p = fma32(p, w, 2.0000714765e-1f);
    p = fma32(p, w, -2.4999993993e-1f);
    p = fma32(p, w, 3.3333331174e-1f);
    const float wz = w * z;
    const float ef = (float)e;
    float y = p * wz;
    y = fma32(ef, -2.12194440e-4f, y);
    y = fma32(-0.5f, z, y);
    const float r = w + y;
    return fma32(ef, 0.693359375f, r);
}

// cosine and sine of 2 pi m / 2^24, m in [1, 2^24]: the nearest quarter turn is taken off in integers, the rest (at most an
// eighth of a turn, exact as a float) goes through the polynomials on [-pi / 4, pi / 4], and the quarter turns rotate the pair
XARM_HD void sincos_turn(uint32_t m, float &c, float &s) {
    const uint32_t q = (m + 0x200000u) >> 22;
    const int rem = (int)m - (int)(q << 22);
    const float fr = (float)rem * 5.9604644775390625e-8f;          // turns, exact
    const float th = fr * 6.28318530717958648f;
    const float z = th * th;
    float ps = -1.9515295891e-4f;
    ps = fma32(ps, z, 8.3321608736e-3f);
    ps = fma32(ps, z, -1.6666654611e-1f);
    const float psz = ps * z;
    const float sn = fma32(psz, th, th);
    float pc = 2.443315711809948e-5f;
    pc = fma32(pc, z, -1.388731625493765e-3f);
    pc = fma32(pc, z, 4.166664568298827e-2f);
    const float zz = z * z;
    float cs = fma32(-0.5f, z, 1.0f);
    cs = fma32(pc, zz, cs);
    switch (q & 3u) {
    case 0: c = cs; s = sn; break;
    case 1: c = -sn; s = cs; break;
    case 2: c = -cs; s = -sn; break;
    default: c = sn; s = -cs; break;
    }
}

// one Box-Muller pair from two Philox words
XARM_HD void box_muller(uint32_t w0, uint32_t w1, float &z0, float &z1) {
    const uint32_t m1 = (w0 >> 8) + 1u, m2 = (w1 >> 8) + 1u;
    const float u1 = (float)m1 * 5.9604644775390625e-8f;           // (0, 1], exact
    const float l = log_f(u1);
    const float r = __builtin_sqrtf(-2.0f * l);
    float c, s;
    sincos_turn(m2, c, s);
    z0 = r * c;
    z1 = r * s;
}

// the four standard normals of column block b (columns 4 b .. 4 b + 3) of global row `grow` at call number `calls`
XARM_HD void noise4(uint64_t seed, int64_t grow, int64_t calls, int b, float (&z)[4]) {
    uint32_t o[4];
    xk::philox(seed, (uint32_t)grow, (uint32_t)((uint64_t)grow >> 32), (uint32_t)calls,
               PHILOX_TAG + (uint32_t)b + ((uint32_t)((uint64_t)calls >> 32) << 2), o);
    box_muller(o[0], o[1], z[0], z[1]);
    box_muller(o[2], o[3], z[2], z[3]);
}

// ------------------------------------------------------------------------------------------------------------- the row's parts
// column j of row e as it enters the network (normalised with the frozen statistics when they are given)
XARM_HD float input_at(const Args &a, int64_t e, int j) {
    const float *p = a.x0;
    int w = a.obs, k = j;
    if (j >= a.obs + a.goal) { p = a.x2; w = a.goal; k = j - a.obs - a.goal; }
    else if (j >= a.obs) { p = a.x1; w = a.goal; k = j - a.obs; }
    const float x = p[e * w + k];
    if (a.stats == nullptr) return x;
    return xnorm::norm_value(x, a.stats[j], sqrt(a.stats[a.D + j] + a.eps), a.clip_obs);
}

// action, env_action and the log-probability term of one column
XARM_HD float finish_column(float mean, float log_std, float z, bool deterministic, float &action, float &env_action) {
    action = deterministic ? mean : fma32(exp_f(log_std), z, mean);
    env_action = action < -1.0f ? -1.0f : (action > 1.0f ? 1.0f : action);
    const float zz = z * z;
    float t = -0.5f * zz;
    t = t - log_std;
    return t - 0.918938533204672742f;
}

// ---- the layers' chains, NU units side by side (every unit's own chain is the one described at the top: from the bias, layer 1 over
// the columns in natural order with the zero operand behind an odd D, layers 2 and 3 in the order KORD).  W: the first unit's row;
// x / h: operand k at x[k * xs].  The host rows below run them with NU = 1, the A2C update (xarm_a2c_core.h) with a row's 16 units.
constexpr int kord(int s) { return unit_of(s >> 5, (s >> 1) & 15, s & 1); }   // KORD[s]
constexpr bool kord_is_the_table() {
    for (int s = 0; s < HID; s++)
        if (kord(s) != KORD[s]) return false;
    return true;
}
static_assert(kord_is_the_table(), "kord(s) must be KORD[s]");
template <int NU> XARM_HD void layer1_chains(const float *W, int D, const float *x, int xs, float (&acc)[NU]) {
    for (int k = 0; k < D; k++) {
        const float xk = x[k * xs];
#pragma unroll
        for (int u = 0; u < NU; u++) acc[u] = fma32(W[u * D + k], xk, acc[u]);
    }
    if (D & 1) {
#pragma unroll
        for (int u = 0; u < NU; u++) acc[u] = fma32(0.0f, 0.0f, acc[u]);
    }
}
template <int NU> XARM_HD void hidden_chains(const float *W, const float *h, int hs, float (&acc)[NU]) {
    for (int s = 0; s < HID; s++) {
        const int k = kord(s);
        const float hk = h[k * hs];
#pragma unroll
        for (int u = 0; u < NU; u++) acc[u] = fma32(W[u * HID + k], hk, acc[u]);
    }
}

#if !defined(__HIPCC__) || defined(XARM_HOST_BUILD)
// ---- the whole row as plain loops (the host build; the kernel holds the same chains in MFMA accumulators); h1 / h2 are kept
inline void tower_row_keep(const Tower &T, const float *x, int D, int nout, float *h1, float *h2, float *out) {
    for (int u = 0; u < HID; u++) {
        float acc[1] = {T.b1[u]};
        layer1_chains<1>(T.W1 + u * D, D, x, 1, acc);
        h1[u] = tanh_f(acc[0]);
    }
    for (int u = 0; u < HID; u++) {
        float acc[1] = {T.b2[u]};
        hidden_chains<1>(T.W2 + u * HID, h1, 1, acc);
        h2[u] = tanh_f(acc[0]);
    }
    for (int u = 0; u < nout; u++) {
        float acc[1] = {T.b3[u]};
        hidden_chains<1>(T.W3 + u * HID, h2, 1, acc);
        out[u] = acc[0];
    }
}
inline void tower_row(const Tower &T, const float *x, int D, int nout, float *out) {
    float h1[HID], h2[HID];
    tower_row_keep(T, x, D, nout, h1, h2, out);
}

inline void row(const Args &a, int64_t e) {
    float x[MAX_DIM], mean[MAX_ACT];
    for (int j = 0; j < a.D; j++) x[j] = input_at(a, e, j);
    tower_row(a.pi, x, a.D, a.A, mean);
    const int64_t calls = a.deterministic ? 0 : a.calls[0];
    float lp = 0.0f;
    for (int b = 0; 4 * b < a.A; b++) {
        float z[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        if (!a.deterministic) noise4(a.seed, a.row_offset + e, calls, b, z);
        for (int m = 0; m < 4 && 4 * b + m < a.A; m++) {
            const int c = 4 * b + m;
            const float t = finish_column(mean[c], a.log_std[c], z[m], a.deterministic != 0, a.action[e * a.A + c], a.env_action[e * a.A + c]);
            lp = c == 0 ? t : lp + t;
        }
    }
    if (a.logp) a.logp[e] = lp;
    if (a.value) {
        float v;
        tower_row(a.vf, x, a.D, 1, &v);
        a.value[e] = v;
    }
}
#endif

#if defined(__HIPCC__) && !defined(XARM_HOST_BUILD)
// k_policy_act (+ k_policy_tick behind a stochastic call) on `stream` (xarm_k_policy.hip); returns the launches' hipError_t
int launch_policy(const Args &a, int64_t *calls, void *stream);
#endif

}  // namespace xpol
