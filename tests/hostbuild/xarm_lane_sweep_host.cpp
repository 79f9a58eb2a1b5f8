// Host (g++) instantiation of the one-env-per-lane PickAndPlace core alone (gym_xarm_amd/csrc/xarm_core.h: xk::env_step,
// xk::env_step_fast_range, xk::env_reset), for tests/test_lane_sweep_forms.py: the same translation unit is built with
// -DXK_SWEEP_V1 -DXK_TABLE_V1 (the sweep of xk::substep in its first form: one set of impulses, one loop with a test per
// arm-limit row, scalar table slots), with -DXK_SWEEP_FULL (the product form in the fast AND the full substep), as the product
// is (the product form in the fast substep alone) and with an odd -DXK_SWEEP_ITERS, and the builds are compared bit for bit.
// XARM_HOST_ANY_PER_ENV: the wave-level predicates follow the one env a call steps, so that an env with no arm joint inside a
// limit window runs the limit-free loop of the product as a device wavefront of such envs does.  Never loaded by the product package.
#define XARM_HOST_BUILD 1
#define XARM_HOST_ANY_PER_ENV 1
#include "../../gym_xarm_amd/csrc/xarm_core.h"
#include <string.h>

namespace {
template <typename T> struct HostLds {
    T *base;
    T &operator[](int i) const { return base[i]; }
};
template <typename T> void load(const double *row, xk::EnvState<T> &s) {
    for (int i = 0; i < 9; i++) { s.q[i] = (T)row[xk::S_Q + i]; s.qd[i] = (T)row[xk::S_QD + i]; }
    for (int i = 0; i < 3; i++) { s.bp[i] = (T)row[xk::S_BP + i]; s.bv[i] = (T)row[xk::S_BV + i]; s.bw[i] = (T)row[xk::S_BW + i]; s.goal[i] = (T)row[xk::S_GOAL + i]; }
    for (int i = 0; i < 4; i++) s.bq[i] = (T)row[xk::S_BQ + i];
    for (int i = 0; i < 8; i++) { s.lam_t[i] = (T)row[xk::S_LT + i]; s.lam_p[i] = (T)row[xk::S_LP + i]; }
    s.touch = (T)row[xk::S_TOUCH]; s.mug = (T)row[xk::S_MUG]; s.steps = (T)row[xk::S_STEPS]; s.episode = (T)row[xk::S_EPISODE];
}
template <typename T> void store(const xk::EnvState<T> &s, double *row) {
    for (int i = 0; i < 9; i++) { row[xk::S_Q + i] = s.q[i]; row[xk::S_QD + i] = s.qd[i]; }
    for (int i = 0; i < 3; i++) { row[xk::S_BP + i] = s.bp[i]; row[xk::S_BV + i] = s.bv[i]; row[xk::S_BW + i] = s.bw[i]; row[xk::S_GOAL + i] = s.goal[i]; }
    for (int i = 0; i < 4; i++) row[xk::S_BQ + i] = s.bq[i];
    for (int i = 0; i < 8; i++) { row[xk::S_LT + i] = s.lam_t[i]; row[xk::S_LP + i] = s.lam_p[i]; }
    row[xk::S_TOUCH] = s.touch; row[xk::S_MUG] = s.mug; row[xk::S_STEPS] = s.steps; row[xk::S_EPISODE] = s.episode;
}
// what a step returns beside the state: the observation, the reward and the two flags
constexpr int OUT_DIM = xk::OBS_DIM + 3;
template <typename T> void store_out(const T (&o)[xk::OBS_DIM], T r, bool d, bool su, double *row) {
    for (int i = 0; i < xk::OBS_DIM; i++) row[i] = o[i];
    row[xk::OBS_DIM] = r; row[xk::OBS_DIM + 1] = d ? 1.0 : 0.0; row[xk::OBS_DIM + 2] = su ? 1.0 : 0.0;
}
xk::EnvCfg mkcfg(uint64_t seed) {
    xk::EnvCfg c; memset(&c, 0, sizeof c); c.seed = seed;
    return c;
}
template <typename T> void lane_step(const xk::EnvCfg &cfg, int64_t E, double *state, const double *act, double *out) {
    for (int64_t e = 0; e < E; e++) {
        xk::EnvState<T> s; T lds[xk::LDS_FLOATS]; HostLds<T> L{lds};
        load(state + e * xk::STATE_DIM, s);
        T a[4], o[xk::OBS_DIM], r; bool d, su;
        for (int k = 0; k < 4; k++) a[k] = (T)act[e * 4 + k];
        xk::env_step<T>(cfg, s, a, o, r, d, su, L);
        store(s, state + e * xk::STATE_DIM);
        store_out(o, r, d, su, out + e * OUT_DIM);
    }
}
// the step as the staged pipeline runs it on an env that is never handed off: the fast ranges [0,5), [5,10), [10,15).
// ok[e] = 0: a pad row was active in one of them (the env is handed off; its state and out rows are left as they were)
template <typename T> void lane_step_fast3(const xk::EnvCfg &cfg, int64_t E, double *state, const double *act, double *out, int *ok) {
    static const int EDGE[4] = {0, 5, 10, xm::PNP_N_SUBSTEPS};
    for (int64_t e = 0; e < E; e++) {
        xk::EnvState<T> s; T lds[xk::LDS_FLOATS]; HostLds<T> L{lds};
        load(state + e * xk::STATE_DIM, s);
        T a[4], qt[9], o[xk::OBS_DIM], r = (T)0; bool d = false, su = false;
        for (int k = 0; k < 4; k++) a[k] = (T)act[e * 4 + k];
        bool fast = true;
        for (int g = 0; g < 3 && fast; g++) fast = xk::env_step_fast_range<T>(cfg, s, a, qt, EDGE[g], EDGE[g + 1], o, r, d, su, L);
        ok[e] = fast ? 1 : 0;
        if (!fast) continue;
        store(s, state + e * xk::STATE_DIM);
        store_out(o, r, d, su, out + e * OUT_DIM);
    }
}
template <typename T> void lane_reset(const xk::EnvCfg &cfg, int64_t E, double *state) {
    for (int64_t e = 0; e < E; e++) {
        xk::EnvState<T> s; T lds[xk::LDS_FLOATS]; HostLds<T> L{lds};
        load(state + e * xk::STATE_DIM, s);
        xk::env_reset<T>(cfg, e, s, L);
        store(s, state + e * xk::STATE_DIM);
    }
}
}  // namespace

extern "C" {
// which forms this build holds: sets of impulses in the sweep (1 = XK_SWEEP_V1, 2 = XK_SWEEP_FULL), whether XK_TABLE_V1 is
// set, and its sweep count
int xls_sets(void) {
#if defined(XK_SWEEP_V1)
    return 1;
#elif defined(XK_SWEEP_FULL)
    return 2;
#else
    return 0;   // the shipped mix: two sets in the fast substep, one in the full substep
#endif
}
int xls_table_v1(void) {
#ifdef XK_TABLE_V1
    return 1;
#else
    return 0;
#endif
}
int xls_sweeps(void) { return XK_SWEEP_ITERS; }
int xls_out_dim(void) { return OUT_DIM; }
// the arm joints' limits and the width of the window in which a limit row exists
void xls_limits(double *lower, double *upper, double *window) {
    for (int i = 0; i < 7; i++) { lower[i] = xm::LOWER[i]; upper[i] = xm::UPPER[i]; }
    *window = xm::LIMIT_WINDOW;
}
void xls_step(int f32, uint64_t seed, int64_t E, double *state, const double *act, double *out) {
    const xk::EnvCfg c = mkcfg(seed);
    if (f32) lane_step<float>(c, E, state, act, out); else lane_step<double>(c, E, state, act, out);
}
void xls_step_fast3(int f32, uint64_t seed, int64_t E, double *state, const double *act, double *out, int *ok) {
    const xk::EnvCfg c = mkcfg(seed);
    if (f32) lane_step_fast3<float>(c, E, state, act, out, ok); else lane_step_fast3<double>(c, E, state, act, out, ok);
}
void xls_reset(int f32, uint64_t seed, int64_t E, double *state) {
    const xk::EnvCfg c = mkcfg(seed);
    if (f32) lane_reset<float>(c, E, state); else lane_reset<double>(c, E, state);
}
}
