// Host (g++ -ffp-contract=off) instantiation of gym_xarm_amd/csrc/xarm_acw_core.h and xarm_ppow_core.h for the CPU-side tests ONLY
// (tests/test_ppow_host.py, tests/test_ppow_gpu.py, tests/test_polw_gpu.py, and ppow_main.cpp for the sanitizer run).  Never loaded by the
// product package: gym_xarm_amd runs both calls through libxarm_hip.so (xarm_k_acw.hip, xarm_k_ppow.hip).  pwh_act / pwh_update validate
// exactly as xarm_acw_act / xarm_ppow_update do and then run the cores' own chains (xacw::run_act, xppow::run_update) with the host
// executors on NumPy / malloc'd memory; the workspaces are used as the device uses them.
#define XARM_HOST_BUILD 1
#include "../../gym_xarm_amd/csrc/xarm_acw_core.h"
#include "../../gym_xarm_amd/csrc/xarm_ppow_core.h"

extern "C" {

int64_t pwh_act_workspace_bytes(const xarm_acw_layout *l) {
    if (xacw::layout_error(l)) return -1;
    xacw::Dev d = {};
    xacw::fill_shape(d, l);
    return xacw::fill_work(d, nullptr);
}

int pwh_act(const xarm_acw_layout *l, const xarm_policy_params *p, const xarm_acw_weights *w, const double *stats, int64_t *calls, const float *obs,
            const float *ag, const float *dg, void *workspace, float *action, float *env_action, float *logp, float *value) {
    if (xacw::layout_error(l) || xpol::params_error(p, stats != nullptr) || !w) return -1;
    if (l->num_rows == 0) return 0;
    if (xacw::pointer_error(l, p, w, calls, obs, ag, dg, workspace, value)) return -1;
    xacw::Dev d = {};
    xacw::fill_dev(d, l, p, w, stats, calls, obs, ag, dg, workspace, action, env_action, logp, value);
    xacw::HostExec ex;
    xacw::run_act(d, ex);
    return 0;
}

int64_t pwh_workspace_bytes(const xarm_ppow_layout *l) {
    if (xppow::layout_error(l)) return -1;
    xppow::Dev d = {};
    xppow::fill_shape(d, l);
    return xppow::fill_work(d, nullptr);
}

// parameters, rows of a minibatch, minibatches, steps, call-start chunks, launches, row ranges, tensors, then the ranges' 17 row bounds,
// the NT + 1 offsets of the flat gradient, and where mean, value, adv, ret, old_logp start in the workspace (in floats)
void pwh_geometry(const xarm_ppow_layout *l, int64_t *out) {
    xppow::Dev d = {};
    xppow::fill_shape(d, l);
    float *base = (float *)(uintptr_t)4096;
    xppow::fill_work(d, base);
    out[0] = d.g.P; out[1] = d.g.B; out[2] = d.p.M; out[3] = d.p.S; out[4] = d.CN + d.CE; out[5] = xppow::launches(d.g.L, d.p.S, d.CN + d.CE);
    out[6] = d.g.S; out[7] = d.g.NT;
    for (int k = 0; k <= xsacw::MAX_SPLIT; k++) out[8 + k] = d.g.rows[k];
    for (int k = 0; k <= d.g.NT; k++) out[25 + k] = d.g.off[k];
    out[43] = d.mean - base; out[44] = d.value - base; out[45] = d.adv - base; out[46] = d.ret - base; out[47] = d.oldlp - base;
}

int pwh_update(const xarm_ppow_layout *l, const xarm_ppo_params *p, const xarm_acw_weights *w, const xarm_acw_weights *m, const xarm_acw_weights *v,
               int64_t *step, const float *obs, const float *action, const float *reward, const float *done, const float *use, const float *last_obs,
               const float *old_logp, const int32_t *perm, void *workspace, float *out_adv, float *out_returns, float *out_grad, float *out_stats) {
    if (xppow::layout_error(l) || xppo::params_error(p) || !w || !m || !v) return -1;
    if (l->num_envs == 0) return 0;
    if (xppow::pointer_error(l, w, m, v, step, obs, action, reward, done, last_obs, perm, workspace)) return -1;
    xppow::Dev d = {};
    xppow::fill_shape(d, l);
    xppo::fill_hyper(d.h, p);
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
