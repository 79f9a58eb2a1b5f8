// Host (g++ -ffp-contract=off) instantiation of gym_xarm_amd/csrc/xarm_ppo_core.h for the CPU-side tests ONLY (tests/test_ppo_host.py,
// tests/test_ppo_gpu.py, and ppo_main.cpp for the sanitizer run).  Never loaded by the product package: gym_xarm_amd runs the update
// through libxarm_hip.so (xarm_k_ppo.hip).  ph_update validates exactly as xarm_ppo_update does and then runs xppo::host_update on
// NumPy / malloc'd memory; the workspace is not used by the host build (any non-null 16-byte aligned pointer passes).  Its one
// argument beyond the ABI's, out_old_logp [T, E] (may be NULL), returns the call-start log-probabilities in use.
#define XARM_HOST_BUILD 1
#include "../../gym_xarm_amd/csrc/xarm_ppo_core.h"

using namespace xppo;

extern "C" {

int64_t ph_workspace_bytes(const xarm_ppo_layout *l) {
    if (layout_error(l)) return -1;
    Shape s;
    Work k;
    fill_shape(s, l);
    fill_work(k, s);
    return k.total;
}

int64_t ph_param_count(const xarm_ppo_layout *l) {
    if (layout_error(l)) return -1;
    Shape s;
    fill_shape(s, l);
    return s.a.P;
}

// the launch geometry for this layout: tiles of a full minibatch, groups, rows per tile, the most groups, rows per minibatch,
// minibatches per epoch, optimiser steps, launches of one update
void ph_geometry(const xarm_ppo_layout *l, int64_t *out) {
    Shape s;
    fill_shape(s, l);
    out[0] = s.a.tiles; out[1] = s.a.G; out[2] = ROWS; out[3] = xa2c::MAX_GROUPS; out[4] = s.B; out[5] = s.M; out[6] = s.S; out[7] = 4 + 3 * s.S;
}

int ph_update(const xarm_ppo_layout *l, const xarm_ppo_params *p, const xarm_policy_weights *w, const xarm_policy_weights *m,
              const xarm_policy_weights *v, int64_t *step, const float *obs, const float *action, const float *reward, const float *done,
              const float *use, const float *last_obs, const float *old_logp, const int32_t *perm, void *workspace, float *out_adv,
              float *out_returns, float *out_grad, float *out_stats, float *out_old_logp) {
    if (layout_error(l) || params_error(p) || !w || !m || !v) return -1;
    if (l->num_envs == 0) return 0;
    if (pointer_error(l, w, m, v, step, obs, action, reward, done, last_obs, perm, workspace)) return -1;
    Shape s;
    Hyper h;
    fill_shape(s, l);
    fill_hyper(h, p);
    float *wt[NTENS], *mt[NTENS], *vt[NTENS];
    xa2c::tensors_of(w, wt);
    xa2c::tensors_of(m, mt);
    xa2c::tensors_of(v, vt);
    host_update(s, h, wt, mt, vt, step, obs, action, reward, done, use, last_obs, old_logp, perm, out_adv, out_returns, out_grad, out_stats,
                out_old_logp);
    return 0;
}

}  // extern "C"
