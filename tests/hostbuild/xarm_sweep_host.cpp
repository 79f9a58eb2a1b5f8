// Host (g++) instantiation of the cooperative PickAndPlace core alone (gym_xarm_amd/csrc/xarm_coop_core.h), for
// tests/test_sweep_forms.py: the same translation unit is built with and without -DXC_SWEEP_COPY (one set of impulse
// pairs with a copy per pair step / two sets, no copy) and with an odd -DXC_SWEEP_ITERS, and the builds are compared
// bit for bit.  Never loaded by the product package.
#define XARM_HOST_BUILD 1
#include "../../gym_xarm_amd/csrc/xarm_core.h"
#include "../../gym_xarm_amd/csrc/xarm_coop_core.h"
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
xk::EnvCfg mkcfg(uint64_t seed) {
    xk::EnvCfg c; memset(&c, 0, sizeof c); c.seed = seed;
    return c;
}
template <typename T> void coop_step(const xk::EnvCfg &cfg, int64_t E, double *state, const double *act) {
    for (int64_t e = 0; e < E; e++) {
        xk::EnvState<T> s; T lds[xk::LDS_FLOATS]; HostLds<T> L{lds};
        load(state + e * xk::STATE_DIM, s);
        T a[4], o[xk::OBS_DIM], r; bool d, su;
        for (int k = 0; k < 4; k++) a[k] = (T)act[e * 4 + k];
        xc::env_step<T>(xc::Grp(), cfg, s, a, o, r, d, su, L);
        store(s, state + e * xk::STATE_DIM);
    }
}
template <typename T> void coop_reset(const xk::EnvCfg &cfg, int64_t E, double *state) {
    for (int64_t e = 0; e < E; e++) {
        xk::EnvState<T> s; T lds[xk::LDS_FLOATS]; HostLds<T> L{lds};
        load(state + e * xk::STATE_DIM, s);
        xc::env_reset<T>(xc::Grp(), cfg, e, s, L);
        store(s, state + e * xk::STATE_DIM);
    }
}
}  // namespace

extern "C" {
// which form this build holds: 1 = one set and a copy (XC_SWEEP_COPY), 2 = two sets; and its sweep count
int xsw_sets(void) {
#ifdef XC_SWEEP_COPY
    return 1;
#else
    return 2;
#endif
}
int xsw_sweeps(void) { return XC_SWEEP_ITERS; }
void xsw_coop_step(int f32, uint64_t seed, int64_t E, double *state, const double *act) {
    const xk::EnvCfg c = mkcfg(seed);
    if (f32) coop_step<float>(c, E, state, act); else coop_step<double>(c, E, state, act);
}
void xsw_coop_reset(int f32, uint64_t seed, int64_t E, double *state) {
    const xk::EnvCfg c = mkcfg(seed);
    if (f32) coop_reset<float>(c, E, state); else coop_reset<double>(c, E, state);
}
}
