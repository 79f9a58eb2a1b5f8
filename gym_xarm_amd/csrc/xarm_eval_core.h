// xarm_eval_core.h - device-resident policy evaluation: the episode accounting of stable-baselines3's
// `evaluate_policy` for a batch of envs, and the summary of its records.  One env's part of a step and one thread's part of the
// summary.  The kernels are in xarm_k_eval.hip; like the norm and replay cores this also compiles for the host (g++
// -DXARM_HOST_BUILD -ffp-contract=off, tests/hostbuild_eval/) for the CPU tests.  Every index is integer arithmetic, the float64
// sums run in one fixed order, and both builds are compiled with contraction off: the host build and the device agree bit for bit.
//
//   quotas    E = num_envs, N = n_eval_episodes, q, r = divmod(N, E).  Env i contributes its first target[i] = q + (i >= E - r)
//             episodes (= (N + i) / E, SB3's split); its records start at slot base[i] = q i + max(0, i - (E - r)), the exclusive
//             prefix of target in closed form.  Neither is stored.
//   cur_ret   double [E], cur_len int32 [E]: return and length of the running episode
//   count     int32 [E]: records env i has written, <= target[i]
//   remaining int32 [1]: N - records written
//   records   double [N, 3]: (return, length, success) of episode k of env i at slot base[i] + k - env-major, whatever the
//             order of arrival
//
// step (env i): cur_ret += c rew, cur_len += c with c = keep[i] != 0 (keep null: 1); on done, if count < target the record is
// written and count += 1, then cur_ret and cur_len are zeroed either way.
// summary: thread t of THREADS owns the slots t, t + THREADS, ...; a slot is written when its index inside its env is below
// that env's count.  Pass 1: per thread n, sum of returns, of lengths, of successes, min and max over its written slots in slot
// order; the partials are merged in thread order.  Pass 2: the squared deviations from the two means the same way.
// out = mean_reward, std_reward (population), mean_length, std_length, success_rate, min_reward, max_reward, n.
#pragma once
#include <stdint.h>
#include <math.h>
#include "../../include/xarm_hip.h"
#include "xarm_core.h"

namespace xeval {

constexpr int THREADS = 256;             // the summary's one workgroup, and the envs of one workgroup of the step

struct Layout { int32_t E, N, q, r; };

inline Layout make_layout(const xarm_eval_layout &l) {
    Layout L;
    L.E = l.num_envs; L.N = l.n_eval_episodes;
    L.q = L.E > 0 ? L.N / L.E : 0; L.r = L.E > 0 ? L.N % L.E : 0;
    return L;
}

// null when the layout is usable, else what is wrong with it
inline const char *layout_error(const xarm_eval_layout *l) {
    if (!l) return "layout is NULL";
    if (l->num_envs < 0) return "num_envs must be >= 0";
    if (l->n_eval_episodes < 1) return "n_eval_episodes must be >= 1";
    return nullptr;
}

XARM_HD int32_t target_of(const Layout &L, int32_t i) { return L.q + (i >= L.E - L.r ? 1 : 0); }
XARM_HD int32_t base_of(const Layout &L, int32_t i) { return L.q * i + (i > L.E - L.r ? i - (L.E - L.r) : 0); }   // < N: no overflow

// slot s < N -> its env and its index inside that env's slots
XARM_HD void slot_owner(const Layout &L, int32_t s, int32_t &env, int32_t &k) {
    const int32_t plain = L.E - L.r, b0 = L.q * plain;      // the first E - r envs hold q slots each, the others q + 1
    if (s < b0) { env = s / L.q; k = s - env * L.q; }        // s < b0 implies q >= 1
    else { const int32_t d = s - b0; env = plain + d / (L.q + 1); k = d - (env - plain) * (L.q + 1); }
}

struct StepArgs {
    Layout L;
    double *cur_ret;
    int32_t *cur_len, *count, *remaining;
    double *records;
    const float *rew;
    const uint8_t *done, *success, *keep;     // keep may be null
};

// env i's part of one step; returns 1 when it wrote a record.  The caller lowers `remaining` by the sum of the returns.
XARM_HD int eval_step_env(const StepArgs &a, int32_t i) {
    const bool c = a.keep == nullptr || a.keep[i] != 0;
    double ret = a.cur_ret[i];
    int32_t len = a.cur_len[i];
    if (c) { ret = ret + (double)a.rew[i]; len += 1; }
    int wrote = 0;
    if (a.done[i] != 0) {
        const int32_t n = a.count[i];
        if (n < target_of(a.L, i)) {
            double *rec = a.records + 3 * (int64_t)(base_of(a.L, i) + n);
            rec[0] = ret; rec[1] = (double)len; rec[2] = a.success[i] != 0 ? 1.0 : 0.0;
            a.count[i] = n + 1;
            wrote = 1;
        }
        ret = 0.0; len = 0;
    }
    a.cur_ret[i] = ret; a.cur_len[i] = len;
    return wrote;
}

struct SummaryArgs {
    Layout L;
    const int32_t *count;
    const double *records;
    double *out;                              // [8]
};

struct Part1 { int32_t n, succ; double sum_r, sum_l, mn, mx; };
struct Part2 { double sq_r, sq_l; };

XARM_HD bool slot_written(const SummaryArgs &a, int32_t s) {
    int32_t env, k;
    slot_owner(a.L, s, env, k);
    return k < a.count[env];
}

XARM_HD Part1 summary_part1(const SummaryArgs &a, int t) {
    Part1 p;
    p.n = 0; p.succ = 0; p.sum_r = 0.0; p.sum_l = 0.0; p.mn = INFINITY; p.mx = -INFINITY;
    for (int32_t s = t; s < a.L.N; s += THREADS) {
        if (!slot_written(a, s)) continue;
        const double *rec = a.records + 3 * (int64_t)s;
        const double r = rec[0];
        p.n += 1;
        p.succ += rec[2] != 0.0 ? 1 : 0;
        p.sum_r = p.sum_r + r;
        p.sum_l = p.sum_l + rec[1];
        p.mn = r < p.mn ? r : p.mn;
        p.mx = r > p.mx ? r : p.mx;
    }
    return p;
}

// the THREADS partials in thread order
XARM_HD Part1 summary_merge1(const Part1 *p) {
    Part1 m = p[0];
    for (int t = 1; t < THREADS; t++) {
        m.n += p[t].n; m.succ += p[t].succ;
        m.sum_r = m.sum_r + p[t].sum_r;
        m.sum_l = m.sum_l + p[t].sum_l;
        m.mn = p[t].mn < m.mn ? p[t].mn : m.mn;
        m.mx = p[t].mx > m.mx ? p[t].mx : m.mx;
    }
    return m;
}

XARM_HD Part2 summary_part2(const SummaryArgs &a, int t, double mean_r, double mean_l) {
    Part2 p;
    p.sq_r = 0.0; p.sq_l = 0.0;
    for (int32_t s = t; s < a.L.N; s += THREADS) {
        if (!slot_written(a, s)) continue;
        const double *rec = a.records + 3 * (int64_t)s;
        const double dr = rec[0] - mean_r, dl = rec[1] - mean_l;
        p.sq_r = p.sq_r + dr * dr;
        p.sq_l = p.sq_l + dl * dl;
    }
    return p;
}

XARM_HD Part2 summary_merge2(const Part2 *p) {
    Part2 m = p[0];
    for (int t = 1; t < THREADS; t++) {
        m.sq_r = m.sq_r + p[t].sq_r;
        m.sq_l = m.sq_l + p[t].sq_l;
    }
    return m;
}

// with no record every mean is 0 / 0 = NaN, as np.mean([]) gives, and so are min and max
XARM_HD void summary_write(const SummaryArgs &a, const Part1 &m, const Part2 &v) {
    const double n = (double)m.n;
    a.out[0] = m.sum_r / n;
    a.out[1] = sqrt(v.sq_r / n);
    a.out[2] = m.sum_l / n;
    a.out[3] = sqrt(v.sq_l / n);
    a.out[4] = (double)m.succ / n;
    a.out[5] = m.n > 0 ? m.mn : a.out[0];
    a.out[6] = m.n > 0 ? m.mx : a.out[0];
    a.out[7] = n;
}

#if defined(__HIPCC__) && !defined(XARM_HOST_BUILD)
// the launches on `stream` (xarm_k_eval.hip); return the launch's hipError_t
int launch_eval_begin(const StepArgs &a, void *stream);
int launch_eval_step(const StepArgs &a, void *stream);
int launch_eval_summary(const SummaryArgs &a, void *stream);
#endif

}  // namespace xeval
