// Host (g++ -ffp-contract=off) instantiation of gym_xarm_amd/csrc/xarm_policy_core.h for the CPU-side tests ONLY (tests/test_policy_host.py,
// tests/test_policy_gpu.py, and policy_main.cpp for the sanitizer run).  Never loaded by the product package: gym_xarm_amd evaluates the
// policy through libxarm_hip.so (xarm_k_policy.hip).  The rows run here one after the other through xpol::row, which walks the
// same k-order table with fmaf that the kernel's MFMA chain follows, on NumPy / malloc'd memory; `calls` is advanced after a
// stochastic call as k_policy_tick does.
#define XARM_HOST_BUILD 1
#include "../../gym_xarm_amd/csrc/xarm_policy_core.h"

using namespace xpol;

extern "C" {

int ph_act(const xarm_policy_layout *l, const xarm_policy_params *p, const xarm_policy_weights *w, const double *stats, int64_t *calls,
           const float *obs, const float *ag, const float *dg, float *action, float *env_action, float *logp, float *value) {
    if (layout_error(l) || params_error(p, stats != nullptr) || !w) return -1;
    if (l->num_envs == 0) return 0;
    if (pointer_error(l, p, w, calls, obs, ag, dg, action, env_action, value)) return -1;
    Args a = {};
    fill_args(a, l, p, w);
    a.stats = stats; a.calls = calls; a.x0 = obs; a.x1 = ag; a.x2 = dg;
    a.action = action; a.env_action = env_action; a.logp = logp; a.value = value;
    for (int64_t e = 0; e < a.E; e++) row(a, e);
    if (!a.deterministic) calls[0] += 1;
    return 0;
}

// the elementary functions on arrays, and the k-order table (the tests state their accuracy)
void ph_tanh(const float *x, float *y, int64_t n) { for (int64_t i = 0; i < n; i++) y[i] = tanh_f(x[i]); }
void ph_exp(const float *x, float *y, int64_t n) { for (int64_t i = 0; i < n; i++) y[i] = exp_f(x[i]); }
void ph_log(const float *x, float *y, int64_t n) { for (int64_t i = 0; i < n; i++) y[i] = log_f(x[i]); }
void ph_sincos_turn(const uint32_t *m, float *c, float *s, int64_t n) { for (int64_t i = 0; i < n; i++) sincos_turn(m[i], c[i], s[i]); }
void ph_kord(int32_t *out) { for (int k = 0; k < HID; k++) out[k] = KORD[k]; }
uint32_t ph_philox_tag(void) { return PHILOX_TAG; }

}  // extern "C"
