// xarm_opt_core.h - what follows the gradient in every device-resident learner, stated once for both builds: the
// float64 sum of a parameter's partial slices, n_use, the Gaussian entropy, the clip coefficient of torch's clip_grad_norm_, the
// lookup of the tensor that holds a flat parameter, and the steps of torch's RMSprop and Adam.  The kernels of xarm_k_a2c.hip,
// xarm_k_ppo.hip, xarm_k_sac.hip and xarm_k_sacw.hip and the g++ host builds (tests/hostbuild_*) all call these functions; the units
// are built with -ffp-contract=off, so every operation below is performed as written and in this order in either build.
//
//   sum       (double) base[0] + (double) base[stride] + ... in index order
//   n_use     max(sum use, 1)
//   entropy   sum_c (log_std_c + 0.5 + log(2 pi) / 2), float64
//   clip      g *= min(1, max_grad_norm / (norm + 1e-6))
//   RMSprop   sq = alpha sq + (1 - alpha) g g; p = p - lr (g / (sqrt(sq) + eps))
//   Adam      step t: m = m + (1 - b1)(g - m); v = b2 v + (1 - b2) g g; p -= (lr / (1 - b1^t)) m / (sqrt(v) / sqrt(1 - b2^t) + eps);
//             the powers by repeated squaring in float64 (ipow)
#pragma once
#include <stdint.h>
#include "xarm_core.h"

namespace xopt {

// ------------------------------------------------------------------------------------------------------------------------ sums
XARM_HD double slice_sum(const float *base, int count, int64_t stride) {
    double sum = 0.0;
    for (int k = 0; k < count; k++) sum += (double)base[(int64_t)k * stride];
    return sum;
}

XARM_HD double n_use(double sum_use) { return sum_use > 1.0 ? sum_use : 1.0; }

XARM_HD double gaussian_entropy(const float *log_std, int A) {
    double ent = 0.0;
    for (int c = 0; c < A; c++) ent += (double)log_std[c] + 0.5 + 0.918938533204672742;
    return ent;
}

XARM_HD float clip_coef(float norm, float max_norm) {
    const float c = max_norm / (norm + 1e-6f);
    return c < 1.0f ? c : 1.0f;
}

// ------------------------------------------------------------------------------------------------------------------ flat order
// the tensor, of first .. first + count - 1, that holds flat position p (off[i]: where tensor i starts; p >= off[first])
XARM_HD int tensor_at(const int64_t *off, int first, int count, int64_t p) {
    int i = first;
    for (int k = 1; k < count; k++)
        if (p >= off[first + k]) i = first + k;
    return i;
}

// the same for a count known at compile time: an unrolled compare chain
template <int COUNT> XARM_HD int tensor_at(const int64_t *off, int first, int64_t p) {
    int i = first;
#pragma unroll
    for (int k = 1; k < COUNT; k++)
        if (p >= off[first + k]) i = first + k;
    return i;
}

// --------------------------------------------------------------------------------------------------------------------- RMSprop
struct RmsProp {
    float lr, alpha, one_m_alpha, eps;
};

XARM_HD void rmsprop(const RmsProp &h, float g, float &sq, float &p) {
    const float gg = g * g;
    const float s = h.alpha * sq + h.one_m_alpha * gg;
    const float avg = __builtin_sqrtf(s) + h.eps;
    sq = s;
    p = p - h.lr * (g / avg);
}

// ------------------------------------------------------------------------------------------------------------------------ Adam
struct Adam {
    float b1, one_m_b1, b2, one_m_b2, eps;
    double lr, beta1, beta2;
};

inline void fill_adam(Adam &a, double lr, double beta1, double beta2, double eps) {
    a.b1 = (float)beta1; a.one_m_b1 = (float)(1.0 - beta1); a.b2 = (float)beta2; a.one_m_b2 = (float)(1.0 - beta2);
    a.eps = (float)eps; a.lr = lr; a.beta1 = beta1; a.beta2 = beta2;
}

inline const char *adam_error(double lr, double beta1, double beta2, double eps) {
    if (!(lr >= 0.0) || !(lr < 1e300)) return "lr must be finite and >= 0";
    if (!(beta1 >= 0.0 && beta1 < 1.0) || !(beta2 >= 0.0 && beta2 < 1.0)) return "beta1 and beta2 must lie in [0, 1)";
    if (!(eps > 0.0) || !(eps < 1e300)) return "eps must be finite and > 0";
    return nullptr;
}

XARM_HD double ipow(double b, int64_t t) {
    double r = 1.0;
    while (t > 0) {
        if (t & 1) r = r * b;
        b = b * b;
        t >>= 1;
    }
    return r;
}

// the two float32 scalars of Adam's step t: lr / (1 - b1^t) and sqrt(1 - b2^t)
XARM_HD void adam_scalars(const Adam &h, int64_t t, float *out) {
    out[0] = (float)(h.lr / (1.0 - ipow(h.beta1, t)));
    out[1] = (float)__builtin_sqrt(1.0 - ipow(h.beta2, t));
}

XARM_HD void adam(const Adam &h, const float *sc, float g, float &m, float &v, float &p) {
    const float mn = m + h.one_m_b1 * (g - m);
    const float gg = g * g;
    const float vn = h.b2 * v + h.one_m_b2 * gg;
    const float denom = __builtin_sqrtf(vn) / sc[1] + h.eps;
    m = mn;
    v = vn;
    p = p - sc[0] * (mn / denom);
}

}  // namespace xopt
