// xarm_sac_core.h - device-resident SAC update: one call is one gradient step of stable-baselines3's SAC.train() on a
// batch drawn from a replay buffer - the squashed-Gaussian actor on obs and next_obs, the entropy coefficient's step, the soft target,
// the step of both critics, the actor's step through the stepped critics, the Polyak step of the targets - stream-ordered on the
// module's own parameter tensors.  The kernels are in xarm_k_sac.hip; like xarm_a2c_core.h, whose host backward this reuses, it also
// compiles for the host (g++ -DXARM_HOST_BUILD -ffp-contract=off, tests/hostbuild_sac/) for the CPU tests.  Everything a ROW gives - a, logp, y, q
// and dq/da - is equal between the two builds bit for bit (the policy's chains and elementary functions, the backward's fmaf chains in
// the tile's order); the sums over rows are not (each build is repeatable): the device adds a workgroup's rows in float32 and the
// workgroups' partials in float64 in workgroup order, the host adds chunks of 64 rows in float32 and the chunks in float64.
//
//   towers    actor D -> 64 -> 64 -> 2A, outputs 0 .. A-1 the mean, A .. 2A-1 log_std; critics Dq = D + A -> 64 -> 64 -> 1 on obs | action
//   actor     ls = clamp(log_std, -20, 2), e = exp_f(ls), u = fmaf(e, z, mean), a = tanh_f(u), s = fmaf(-a, a, 1);
//             logp = sum_c ((-0.5 z z - ls) - log(2 pi) / 2) - sum_c log_f(s + 1e-6), each sum in column order
//   alpha     auto: exp_f(log_alpha) with log_alpha as it is at call start; else (float) ent_coef
//   target    y = fmaf(gamma (1 - done), min(q1_t, q2_t) - alpha logp', reward)
//   critics   delta = (q - y) use on q1 and q2 at obs | action; g = (float)(sum / n_use), n_use = max(sum use, 1); Adam; then
//             target = (1 - tau) target + tau critic with the stepped critic (nothing changes the critics again inside the step)
//   dq/da     the stepped critics at obs | a_pi: d3 = 1, d2 = (W3^T d3)(1 - h2^2), d1 = (W2^T d2)(1 - h1^2), dq/da_c = sum_i W1[i][D + c] d1_i
//   actor     the critic with the smaller q (q2 when q2 < q1, else q1); t = 2 a s / (s + 1e-6), g = dq/da s:
//             dmean_c = (alpha t - g) use; dlog_std_c = (alpha (t e z - 1) - g e z) use, 0 where log_std lies outside [-20, 2]
//   log_alpha g = (float)(-sum((logp_pi + target_entropy) use) / n_use) (auto only)
//   flat      the 19 trained tensors one after the other: actor's 6, q1's 6, q2's 6, log_alpha: P floats
//   noise     supplied, or Philox(seed; row, step at call start, TAG + 4 stream + column block), stream 0 = z_pi, 1 = z_next
//   Adam      xopt::adam (xarm_opt_core.h) with t = step + 1 for all three optimisers
//   finish    the call's last writes - log_alpha's step, its out_grad entry, the stats, step += 1 - are finish() below in both builds
#pragma once
#include <stdint.h>
#if !defined(__HIPCC__) || defined(XARM_HOST_BUILD)
#include <vector>
#endif
#include "xarm_a2c_core.h"

namespace xsac {

using xa2c::ROWS;
using xpol::fma32;
using xpol::HID;
using xpol::Tower;

constexpr int MAX_A = XARM_SAC_MAX_ACT;     // 8: the actor's 2 A outputs fill the tile's MAX_ACT delta columns
constexpr int NT = 19;                      // trained tensors: actor 0-5, q1 6-11, q2 12-17, log_alpha 18
constexpr int RED = 256;                    // threads per block of the apply kernels: one flat parameter each
constexpr int MAX_GROUPS = xa2c::MAX_GROUPS;
constexpr uint32_t PHILOX_TAG = 0x53414300u; // "SAC\0"
constexpr float LOG_STD_MIN = -20.0f, LOG_STD_MAX = 2.0f, SQUASH_EPS = 1e-6f;
constexpr int RS = 4, QS = 2, PS = 2;       // per-group scalars (double) of the rows kernel: use, logp_pi use, (logp_pi + target_entropy) use, 0;
                                            // of a critic's gradient kernel: (q - y)^2 use, 0; of the actor's: (alpha logp_pi - qmin) use, qmin use
static_assert(2 * MAX_A <= xpol::MAX_ACT, "the actor's outputs must fit the tile's delta columns");

struct Shape {
    int64_t B, P, Pa, Pq, tiles, pstride, row_offset;
    int D, A, Dq, G, NBq, NBp;
    int64_t off[NT + 1];            // where tensor i starts in the flat gradient
};

struct Hyper {
    xopt::Adam adam;
    float gamma, tau, one_m_tau, alpha_fixed, target_entropy;
    int auto_alpha, deterministic;
    uint64_t seed;
};

// byte offsets of the parts of the workspace (each 16-byte aligned)
struct Work {
    int64_t hdr, y, logp, z, xq, xpi, qpi, dqda, partial, scal_rows, scal_q, scal_p, total;
};

inline const char *layout_error(const xarm_sac_layout *l) {
    if (!l) return "layout is NULL";
    if (l->batch_size < 0) return "batch_size must be >= 0 (and < 2^31)";
    if (l->obs_dim < 1) return "obs_dim must be >= 1";
    if (l->act_dim < 1 || l->act_dim > MAX_A) return "act_dim must lie in [1, XARM_SAC_MAX_ACT (8)]";
    if (l->obs_dim > xpol::MAX_DIM || l->obs_dim + l->act_dim > xpol::MAX_DIM) return "obs_dim + act_dim must be <= XARM_POLICY_MAX_DIM (96)";
    if (l->hidden != HID) return "hidden must be XARM_POLICY_HIDDEN (64)";
    if (l->row_offset < 0) return "row_offset must be >= 0";
    return nullptr;
}

inline const char *params_error(const xarm_sac_params *p) {
    if (!p) return "params is NULL";
    if (!(p->gamma >= 0.0 && p->gamma <= 1.0)) return "gamma must lie in [0, 1]";
    if (const char *why = xopt::adam_error(p->lr, p->beta1, p->beta2, p->eps)) return why;
    if (!(p->tau >= 0.0 && p->tau <= 1.0)) return "tau must lie in [0, 1]";
    if (!(p->ent_coef >= 0.0) || !(p->ent_coef < 1e300)) return "ent_coef must be finite and >= 0";
    if (!(p->target_entropy > -1e300 && p->target_entropy < 1e300)) return "target_entropy must be finite";
    return nullptr;
}

// the 19 trained tensors of a weights struct in the flat order
inline void tensors_of(const xarm_sac_weights *w, float *(&t)[NT]) {
    for (int i = 0; i < 6; i++) {
        t[i] = const_cast<float *>(w->actor[i]);
        t[6 + i] = const_cast<float *>(w->q1[i]);
        t[12 + i] = const_cast<float *>(w->q2[i]);
    }
    t[18] = const_cast<float *>(w->log_alpha);
}

inline Tower tower_of(const float *const *p) { return Tower{p[0], p[1], p[2], p[3], p[4], p[5]}; }

// b1, W2, b2 and W3 of a tower 16-byte aligned, all six there
inline const char *tower_error(const float *const *p) {
    for (int i = 0; i < 6; i++)
        if (!p[i]) return "NULL weight pointer";
    if ((((uintptr_t)p[1] | (uintptr_t)p[2] | (uintptr_t)p[3] | (uintptr_t)p[4]) & 15u) != 0) return "b1, W2, b2 and W3 must be 16-byte aligned";
    return nullptr;
}

// the pointers xarm_sac_act reads or writes with batch_size > 0
inline const char *act_pointer_error(const xarm_sac_params *p, const xarm_sac_weights *w, const int64_t *calls, const float *obs, const float *action) {
    if (!w) return "weights is NULL";
    if (const char *why = tower_error(w->actor)) return why;
    if (!p->deterministic && !calls) return "NULL calls with a stochastic call";
    if (!obs) return "NULL observation pointer";
    if (!action) return "NULL out_action";
    return nullptr;
}

// the pointers xarm_sac_update reads or writes with batch_size > 0
inline const char *pointer_error(const xarm_sac_weights *w, const xarm_sac_weights *m, const xarm_sac_weights *v, const int64_t *step,
                                 const float *obs, const float *next_obs, const float *action, const float *reward, const float *done,
                                 const void *workspace) {
    if (!w) return "weights is NULL";
    if (!m || !v) return "exp_avg / exp_avg_sq is NULL";
    const float *const *towers[5] = {w->actor, w->q1, w->q2, w->q1_target, w->q2_target};
    for (int i = 0; i < 5; i++)
        if (const char *why = tower_error(towers[i])) return why;
    if (!w->log_alpha) return "NULL log_alpha";
    float *t[NT];
    tensors_of(m, t);
    for (int i = 0; i < NT; i++)
        if (!t[i]) return "NULL exp_avg pointer";
    tensors_of(v, t);
    for (int i = 0; i < NT; i++)
        if (!t[i]) return "NULL exp_avg_sq pointer";
    if (!step) return "step_i64 is NULL";
    if (!obs || !next_obs || !action || !reward || !done) return "NULL obs / next_obs / action / reward / done";
    if (!workspace) return "workspace is NULL";
    if (((uintptr_t)workspace & 15u) != 0) return "workspace must be 16-byte aligned";
    return nullptr;
}

inline void fill_shape(Shape &s, const xarm_sac_layout *l) {
    s.B = l->batch_size; s.D = l->obs_dim; s.A = l->act_dim; s.Dq = s.D + s.A; s.row_offset = l->row_offset;
    const int64_t na[6] = {HID * s.D, HID, HID * HID, HID, HID * 2 * s.A, 2 * s.A}, nq[6] = {HID * s.Dq, HID, HID * HID, HID, HID, 1};
    s.off[0] = 0;
    for (int i = 0; i < 6; i++) s.off[i + 1] = s.off[i] + na[i];
    for (int i = 6; i < 18; i++) s.off[i + 1] = s.off[i] + nq[(i - 6) % 6];
    s.off[NT] = s.off[18] + 1;
    s.Pa = s.off[6]; s.Pq = s.off[12] - s.off[6]; s.P = s.off[NT];
    s.tiles = (s.B + ROWS - 1) / ROWS;
    s.G = (int)(s.tiles < MAX_GROUPS ? s.tiles : MAX_GROUPS);
    s.pstride = ((s.Pa > s.Pq ? s.Pa : s.Pq) + 3) & ~(int64_t)3;      // a group's slice holds one tower's gradient
    s.NBq = (int)((2 * s.Pq + RED - 1) / RED);
    s.NBp = (int)((s.Pa + 1 + RED - 1) / RED);
}

inline void fill_hyper(Hyper &h, const xarm_sac_params *p) {
    xopt::fill_adam(h.adam, p->lr, p->beta1, p->beta2, p->eps);
    h.gamma = (float)p->gamma; h.tau = (float)p->tau; h.one_m_tau = (float)(1.0 - p->tau); h.alpha_fixed = (float)p->ent_coef;
    h.target_entropy = (float)p->target_entropy; h.auto_alpha = p->auto_ent_coef != 0; h.deterministic = p->deterministic != 0; h.seed = p->seed;
}

inline void fill_work(Work &k, const Shape &s) {
    int64_t at = 0;
    auto take = [&at](int64_t bytes) { const int64_t o = at; at += (bytes + 15) & ~(int64_t)15; return o; };
    k.hdr = take(16);                                   // Adam's two scalars of the step, alpha, 0
    k.y = take(s.B * 4);
    k.logp = take(s.B * 4);
    k.z = take(s.B * s.A * 4);
    k.xq = take(s.B * s.Dq * 4);
    k.xpi = take(s.B * s.Dq * 4);
    k.qpi = take(2 * s.B * 4);
    k.dqda = take(2 * s.B * s.A * 4);
    k.partial = take(2 * (int64_t)s.G * s.pstride * 4);
    k.scal_rows = take((int64_t)s.G * RS * 8);
    k.scal_q = take(2 * (int64_t)s.G * QS * 8);
    k.scal_p = take((int64_t)s.G * PS * 8);
    k.total = at;
}

// -------------------------------------------------------------------------------------------------- the row's and the parameter's parts
// the four standard normals of column block b (columns 4 b .. 4 b + 3) of row `row` at step counter `counter`, noise stream `stream`
XARM_HD void noise4(uint64_t seed, int64_t row, int64_t counter, int stream, int b, float (&z)[4]) {
    uint32_t o[4];
    xk::philox(seed, (uint32_t)row, (uint32_t)((uint64_t)row >> 32), (uint32_t)counter,
               PHILOX_TAG + (uint32_t)(4 * stream + b) + ((uint32_t)((uint64_t)counter >> 32) << 4), o);
    xpol::box_muller(o[0], o[1], z[0], z[1]);
    xpol::box_muller(o[2], o[3], z[2], z[3]);
}

XARM_HD float clamp_log_std(float ls) { return ls < LOG_STD_MIN ? LOG_STD_MIN : (ls > LOG_STD_MAX ? LOG_STD_MAX : ls); }

// the squashed Gaussian of one row: the actor tower's outputs at out[c * os] (mean_c, then log_std_c at (A + c) * os), the row's z;
// a[c] = tanh(u_c) (tanh(mean_c) when deterministic: z is not read); returns logp
XARM_HD float actor_head(int A, const float *out, int os, const float *z, bool deterministic, float (&a)[MAX_A]) {
    float lg = 0.0f, lq = 0.0f;
#pragma unroll
    for (int c = 0; c < MAX_A; c++) {
        a[c] = 0.0f;
        if (c < A) {
            const float mean = out[c * os], ls = clamp_log_std(out[(A + c) * os]);
            const float zc = deterministic ? 0.0f : z[c];
            const float u = deterministic ? mean : fma32(xpol::exp_f(ls), zc, mean);
            const float ac = xpol::tanh_f(u);
            const float zz = zc * zc;
            float t = -0.5f * zz;
            t = t - ls;
            t = t - xa2c::HALF_LOG_2PI;
            float s = fma32(-ac, ac, 1.0f);
            s = s + SQUASH_EPS;
            const float l = xpol::log_f(s);
            lg = c == 0 ? t : lg + t;
            lq = c == 0 ? l : lq + l;
            a[c] = ac;
        }
    }
    return lg - lq;
}

XARM_HD float alpha_of(const Hyper &h, const float *log_alpha) { return h.auto_alpha ? xpol::exp_f(log_alpha[0]) : h.alpha_fixed; }

XARM_HD float target_row(float gamma, float alpha, float reward, float done, float q1t, float q2t, float logp_next) {
    const float qm = q2t < q1t ? q2t : q1t;
    const float ent = alpha * logp_next;
    const float v = qm - ent;
    const float keep = 1.0f - done;
    return fma32(gamma * keep, v, reward);
}

// the actor's output deltas of one row: the tower's outputs at out[c * os] are replaced by d loss / d mean_c and d loss / d log_std_c
// (times use); dq[c] = d qmin / d a_c
XARM_HD void actor_deltas(int A, float *out, int os, const float *z, float alpha, const float *dq, float use) {
#pragma unroll
    for (int c = 0; c < MAX_A; c++) {
        if (c < A) {
            const float mean = out[c * os], raw = out[(A + c) * os];
            const bool outside = raw < LOG_STD_MIN || raw > LOG_STD_MAX;
            const float e = xpol::exp_f(clamp_log_std(raw));
            const float zc = z[c];
            const float u = fma32(e, zc, mean);
            const float a = xpol::tanh_f(u);
            const float s = fma32(-a, a, 1.0f);
            const float a2 = 2.0f * a;
            const float num = a2 * s;
            const float t = num / (s + SQUASH_EPS);
            const float g = dq[c] * s;
            const float at = alpha * t;
            const float du = at - g;
            const float ez = e * zc;
            const float tm = fma32(t, ez, -1.0f);
            const float l1 = alpha * tm;
            const float l2 = g * ez;
            const float dl = outside ? 0.0f : l1 - l2;
            out[c * os] = du * use;
            out[(A + c) * os] = dl * use;
        }
    }
}

XARM_HD float polyak(const Hyper &h, float target, float w) {
    const float keep = h.one_m_tau * target;
    const float in = h.tau * w;
    return keep + in;
}

// the call's last writes: log_alpha's Adam step (sc: Adam's two scalars of the step; w, m, v: log_alpha and its state), its entry of
// out_grad (nullable), the stats row (nullable) and the step count.  sent, closs, aloss, slp, sq: the sums over rows of
// (logp_pi + target_entropy) use, (q - y)^2 use of both critics, (alpha logp_pi - qmin) use, logp_pi use, qmin use
XARM_HD void finish(const Hyper &h, const float *sc, float alpha, double n_use, double sent, double closs, double aloss, double slp, double sq,
                    float *w, float *m, float *v, float *out_grad, float *out_stats, int64_t *step) {
    const float log_alpha = w[0];
    float gf = 0.0f;
    if (h.auto_alpha) {
        gf = (float)(-sent / n_use);
        float mn = m[0], vn = v[0], wn = log_alpha;
        xopt::adam(h.adam, sc, gf, mn, vn, wn);
        m[0] = mn;
        v[0] = vn;
        w[0] = wn;
    }
    if (out_grad != nullptr) out_grad[0] = gf;
    if (out_stats != nullptr) {
        float *o = out_stats;
        o[0] = (float)(0.5 * closs / n_use); o[1] = (float)(aloss / n_use);
        o[2] = h.auto_alpha ? (float)(-(double)log_alpha * sent / n_use) : 0.0f; o[3] = alpha;
        o[4] = (float)(slp / n_use); o[5] = (float)(sq / n_use); o[6] = (float)n_use; o[7] = 0.0f;
    }
    step[0] = step[0] + 1;
}

#if !defined(__HIPCC__) || defined(XARM_HOST_BUILD)
// ---- the host build: plain loops over the rows
inline void host_noise(const Hyper &h, const float *given, int64_t n, int64_t counter, int stream, int A, float (&z)[MAX_A]) {
    for (int b = 0; 4 * b < A; b++) {
        float q[4];
        if (given == nullptr) noise4(h.seed, n, counter, stream, b, q);
        for (int m = 0; m < 4 && 4 * b + m < A; m++) z[4 * b + m] = given != nullptr ? given[n * A + 4 * b + m] : q[m];
    }
}

// xarm_sac_act: the noise of xpol::noise4 (seed, row_offset + row, calls, column block)
inline void host_act(const Shape &s, const Hyper &h, const Tower &actor, int64_t *calls, const float *obs, float *out_action, float *out_logp) {
    const int64_t c0 = h.deterministic ? 0 : calls[0];
    for (int64_t n = 0; n < s.B; n++) {
        float out[2 * MAX_A], z[MAX_A] = {0.0f}, a[MAX_A];
        xpol::tower_row(actor, obs + n * s.D, s.D, 2 * s.A, out);
        if (!h.deterministic)
            for (int b = 0; 4 * b < s.A; b++) {
                float q[4];
                xpol::noise4(h.seed, s.row_offset + n, c0, b, q);
                for (int m = 0; m < 4 && 4 * b + m < s.A; m++) z[4 * b + m] = q[m];
            }
        const float lp = actor_head(s.A, out, 1, z, h.deterministic != 0, a);
        for (int c = 0; c < s.A; c++) out_action[n * s.A + c] = a[c];
        if (out_logp) out_logp[n] = lp;
    }
    if (!h.deterministic) calls[0] += 1;
}

// q and dq / d x_j, D0 <= j < D0 + nc, of one critic at row x [Dq]: the tile's chains (d3 = 1)
inline void host_dqda(const Tower &T, const float *x, int Dq, int D0, int nc, float &q, float *dq) {
    float h1[HID], h2[HID], d2[HID], d1[HID];
    xpol::tower_row_keep(T, x, Dq, 1, h1, h2, &q);
    for (int j = 0; j < HID; j++) {
        const float pre = fma32(T.W3[j], 1.0f, 0.0f);
        d2[j] = pre * fma32(-h2[j], h2[j], 1.0f);
    }
    for (int j = 0; j < HID; j++) {
        float pre = 0.0f;
        for (int k = 0; k < HID; k++) pre = fma32(T.W2[k * HID + j], d2[k], pre);
        d1[j] = pre * fma32(-h1[j], h1[j], 1.0f);
    }
    for (int c = 0; c < nc; c++) {
        float dx = 0.0f;
        for (int i = 0; i < HID; i++) dx = fma32(T.W1[i * Dq + D0 + c], d1[i], dx);
        dq[c] = dx;
    }
}

// a view of tensors t0 .. t0 + 5 of the flat order as xa2c::host_backward wants it
inline xa2c::Shape tower_shape(const Shape &s, int t0, int Din) {
    xa2c::Shape a = {};
    a.D = Din;
    for (int i = 0; i <= 6; i++) a.off[i] = s.off[t0 + i];
    return a;
}

// w: the 19 trained tensors; tq: the 12 target tensors (q1_target's 6, q2_target's 6); m / v: Adam's state of the 19
inline void host_update(const Shape &s, const Hyper &h, float *const *w, float *const *tq, float *const *m, float *const *v, int64_t *step,
                        const float *obs, const float *next_obs, const float *action, const float *reward, const float *done, const float *use,
                        const float *noise_pi, const float *noise_next, float *out_grad, float *out_dqda, float *out_target, float *out_stats) {
    const Tower actor = tower_of(w), q1 = tower_of(w + 6), q2 = tower_of(w + 12), q1t = tower_of(tq), q2t = tower_of(tq + 6);
    const int D = s.D, A = s.A, Dq = s.Dq;
    const int64_t B = s.B, t0 = step[0];
    const float alpha = alpha_of(h, w[18]);
    std::vector<float> y((size_t)B), lpv((size_t)B), zv((size_t)(B * A)), xq((size_t)(B * Dq)), xpi((size_t)(B * Dq)), g((size_t)s.P, 0.0f);
    std::vector<double> G((size_t)s.P);
    std::vector<float> chunk((size_t)s.P);
    double nuse = 0.0, slp = 0.0, sent = 0.0;
    // the rows: both actor passes, the target
    for (int64_t n = 0; n < B; n++) {
        float out[2 * MAX_A], z[MAX_A] = {0.0f}, a[MAX_A], xn[xpol::MAX_DIM], qa, qb;
        xpol::tower_row(actor, next_obs + n * D, D, 2 * A, out);
        host_noise(h, noise_next, n, t0, 1, A, z);
        const float lpn = actor_head(A, out, 1, z, false, a);
        for (int j = 0; j < D; j++) xn[j] = next_obs[n * D + j];
        for (int c = 0; c < A; c++) xn[D + c] = a[c];
        xpol::tower_row(q1t, xn, Dq, 1, &qa);
        xpol::tower_row(q2t, xn, Dq, 1, &qb);
        y[(size_t)n] = target_row(h.gamma, alpha, reward[n], done[n], qa, qb, lpn);
        xpol::tower_row(actor, obs + n * D, D, 2 * A, out);
        host_noise(h, noise_pi, n, t0, 0, A, z);
        const float lp = actor_head(A, out, 1, z, false, a);
        lpv[(size_t)n] = lp;
        for (int j = 0; j < D; j++) xq[(size_t)(n * Dq + j)] = xpi[(size_t)(n * Dq + j)] = obs[n * D + j];
        for (int c = 0; c < A; c++) {
            xq[(size_t)(n * Dq + D + c)] = action[n * A + c];
            xpi[(size_t)(n * Dq + D + c)] = a[c];
            zv[(size_t)(n * A + c)] = z[c];
        }
        const float u = use ? use[n] : 1.0f;
        nuse += (double)u;
        slp += (double)(lp * u);
        sent += (double)((lp + h.target_entropy) * u);
        if (out_target) out_target[n] = y[(size_t)n];
    }
    const double n_use = xopt::n_use(nuse);
    float sc[2];
    xopt::adam_scalars(h.adam, t0 + 1, sc);
    auto zero_sums = [&]() { for (int64_t p = 0; p < s.P; p++) { G[(size_t)p] = 0.0; chunk[(size_t)p] = 0.0f; } };
    auto flush = [&]() { for (int64_t p = 0; p < s.P; p++) { G[(size_t)p] += (double)chunk[(size_t)p]; chunk[(size_t)p] = 0.0f; } };
    auto mean_grad = [&](int64_t p0, int64_t p1) { for (int64_t p = p0; p < p1; p++) g[(size_t)p] = (float)(G[(size_t)p] / n_use); };
    auto apply = [&](int i0, int i1) {
        for (int i = i0; i < i1; i++)
            for (int64_t p = s.off[i]; p < s.off[i + 1]; p++) xopt::adam(h.adam, sc, g[(size_t)p], m[i][p - s.off[i]], v[i][p - s.off[i]], w[i][p - s.off[i]]);
    };
    // the critics
    zero_sums();
    double closs = 0.0;
    const xa2c::Shape sq1 = tower_shape(s, 6, Dq), sq2 = tower_shape(s, 12, Dq);
    for (int64_t n = 0; n < B; n++) {
        const float *x = &xq[(size_t)(n * Dq)], u = use ? use[n] : 1.0f;
        const Tower *T[2] = {&q1, &q2};
        for (int i = 0; i < 2; i++) {
            float h1[HID], h2[HID], q;
            xpol::tower_row_keep(*T[i], x, Dq, 1, h1, h2, &q);
            const float diff = q - y[(size_t)n], d3 = diff * u;
            xa2c::host_backward(i ? sq2 : sq1, chunk.data(), *T[i], 0, x, h1, h2, &d3, 1);
            closs += (double)(diff * diff * u);
        }
        if ((n + 1) % ROWS == 0 || n + 1 == B) flush();
    }
    mean_grad(s.off[6], s.off[18]);
    apply(6, 18);
    for (int i = 0; i < 12; i++)
        for (int64_t p = 0; p < s.off[7 + i] - s.off[6 + i]; p++) tq[i][p] = polyak(h, tq[i][p], w[6 + i][p]);
    // the actor through the stepped critics
    zero_sums();
    double aloss = 0.0, sq = 0.0;
    const xa2c::Shape sa = tower_shape(s, 0, D);
    for (int64_t n = 0; n < B; n++) {
        float qa, qb, da[MAX_A], db[MAX_A], h1[HID], h2[HID], out[2 * MAX_A];
        host_dqda(q1, &xpi[(size_t)(n * Dq)], Dq, D, A, qa, da);
        host_dqda(q2, &xpi[(size_t)(n * Dq)], Dq, D, A, qb, db);
        if (out_dqda)
            for (int c = 0; c < A; c++) { out_dqda[n * A + c] = da[c]; out_dqda[(B + n) * A + c] = db[c]; }
        const bool second = qb < qa;
        const float qm = second ? qb : qa, u = use ? use[n] : 1.0f;
        xpol::tower_row_keep(actor, obs + n * D, D, 2 * A, h1, h2, out);
        actor_deltas(A, out, 1, &zv[(size_t)(n * A)], alpha, second ? db : da, u);
        xa2c::host_backward(sa, chunk.data(), actor, 0, obs + n * D, h1, h2, out, 2 * A);
        const float ent = alpha * lpv[(size_t)n];
        aloss += (double)((ent - qm) * u);
        sq += (double)(qm * u);
        if ((n + 1) % ROWS == 0 || n + 1 == B) flush();
    }
    mean_grad(0, s.off[6]);
    apply(0, 6);
    if (out_grad)
        for (int64_t p = 0; p < s.off[18]; p++) out_grad[p] = g[(size_t)p];
    finish(h, sc, alpha, n_use, sent, closs, aloss, slp, sq, w[18], m[18], v[18], out_grad ? out_grad + s.off[18] : nullptr, out_stats, step);
}
#endif

#if defined(__HIPCC__) && !defined(XARM_HOST_BUILD)
struct Dev {
    Shape s;
    Hyper h;
    Tower actor, q1, q2, q1t, q2t;
    float *w[NT], *m[NT], *v[NT], *tq[12];
    int64_t *step, *calls;
    const float *obs, *next_obs, *action, *reward, *done, *use, *noise_pi, *noise_next;
    float *hdr, *y, *logp, *z, *xq, *xpi, *qpi, *dqda, *partial;
    double *scal_rows, *scal_q, *scal_p;
    float *out_grad, *out_dqda, *out_target, *out_stats, *out_action, *out_logp;
};
constexpr int LAUNCHES = 6;     // rows; critic gradient, critic apply + Polyak; action gradient; actor gradient, actor + log_alpha apply
// the six launches of one step on `stream` (xarm_k_sac.hip); returns the launches' hipError_t
int launch_update(const Dev &d, void *stream);
// k_sac_act (+ k_sac_tick behind a stochastic call)
int launch_act(const Dev &d, void *stream);
#endif

}  // namespace xsac
