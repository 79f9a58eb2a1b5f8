// Host (g++ -ffp-contract=off) instantiation of gym_xarm_amd/csrc/xarm_ppo_core.h and xarm_ppow_core.h WITH xarm_ppo_options, for the
// CPU-side tests ONLY (tests/ppo_opt_host.py, tests/test_ppo_opt_host.py, tests/test_ppo_opt_gpu.py, and ppo_opt_main.cpp for the
// sanitizer run).  Never loaded by the product package.  poh_update / powh_update are tests/hostbuild_ppo's ph_update and
// tests/hostbuild_ppow's pwh_update with one more argument, the options (NULL = none), validated as xarm_ppo_update_opt /
// xarm_ppow_update_opt validate them.  max_steps >= 0 (tests only) ends the call after that many optimiser steps, as if the layout
// held no more: what a stopped call is compared with.
#define XARM_HOST_BUILD 1
#include "../../gym_xarm_amd/csrc/xarm_ppo_core.h"
#include "../../gym_xarm_amd/csrc/xarm_ppow_core.h"

extern "C" {

int poh_update(const xarm_ppo_layout *l, const xarm_ppo_params *p, const xarm_policy_weights *w, const xarm_policy_weights *m,
               const xarm_policy_weights *v, int64_t *step, const float *obs, const float *action, const float *reward, const float *done,
               const float *use, const float *last_obs, const float *old_logp, const int32_t *perm, void *workspace, float *out_adv,
               float *out_returns, float *out_grad, float *out_stats, const xarm_ppo_options *options, int64_t max_steps, float *out_old_logp) {
    using namespace xppo;
    if (layout_error(l) || params_error(p) || options_error(options) || !w || !m || !v) return -1;
    if (l->num_envs == 0) return 0;
    if (pointer_error(l, w, m, v, step, obs, action, reward, done, last_obs, perm, workspace)) return -1;
    Shape s;
    Hyper h;
    fill_shape(s, l);
    fill_hyper(h, p, options);
    if (max_steps >= 0 && max_steps < s.S) s.S = max_steps;
    float *wt[NTENS], *mt[NTENS], *vt[NTENS];
    xa2c::tensors_of(w, wt);
    xa2c::tensors_of(m, mt);
    xa2c::tensors_of(v, vt);
    host_update(s, h, wt, mt, vt, step, obs, action, reward, done, use, last_obs, old_logp, perm, out_adv, out_returns, out_grad, out_stats,
                out_old_logp);
    return 0;
}

int64_t powh_workspace_bytes(const xarm_ppow_layout *l) {
    if (xppow::layout_error(l)) return -1;
    xppow::Dev d = {};
    xppow::fill_shape(d, l);
    return xppow::fill_work(d, nullptr);
}

int powh_update(const xarm_ppow_layout *l, const xarm_ppo_params *p, const xarm_acw_weights *w, const xarm_acw_weights *m, const xarm_acw_weights *v,
                int64_t *step, const float *obs, const float *action, const float *reward, const float *done, const float *use, const float *last_obs,
                const float *old_logp, const int32_t *perm, void *workspace, float *out_adv, float *out_returns, float *out_grad, float *out_stats,
                const xarm_ppo_options *options, int64_t max_steps) {
    if (xppow::layout_error(l) || xppo::params_error(p) || xppo::options_error(options) || !w || !m || !v) return -1;
    if (l->num_envs == 0) return 0;
    if (xppow::pointer_error(l, w, m, v, step, obs, action, reward, done, last_obs, perm, workspace)) return -1;
    xppow::Dev d = {};
    xppow::fill_shape(d, l);
    xppo::fill_hyper(d.h, p, options);
    if (max_steps >= 0 && max_steps < d.p.S) d.p.S = max_steps;      // after fill_shape: the workspace below is carved for the whole layout
    xppow::tensors_of(d, w, d.w);
    xppow::tensors_of(d, m, d.m);
    xppow::tensors_of(d, v, d.v);
    xppow::fill_work(d, workspace);
    d.step = step;
    d.obs = obs; d.action = action; d.reward = reward; d.done = done; d.use = use; d.last_obs = last_obs; d.old_logp = old_logp; d.perm = perm;
    d.out_adv = out_adv; d.out_returns = out_returns; d.out_grad = out_grad; d.out_stats = out_stats;
    xppow::HostExec ex;
    xppow::run_update(d, ex);
    return 0;
}

}  // extern "C"
