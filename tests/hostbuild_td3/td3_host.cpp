// Host (g++ -ffp-contract=off) instantiation of gym_xarm_amd/csrc/xarm_td3_core.h for the CPU-side tests ONLY (tests/test_td3_host.py,
// tests/test_td3_gpu.py, and td3_main.cpp for the sanitizer run).  Never loaded by the product package: gym_xarm_amd runs the update
// through libxarm_hip.so (xarm_k_td3.hip).  t3h_act / t3h_update validate exactly as xarm_td3_act / xarm_td3_update do and then run
// the core's own chain (xtd3::run_update / run_act) with xtd3::HostExec on NumPy / malloc'd memory; the workspace is used as the
// device uses it (t3h_workspace_bytes bytes, 16-byte aligned).
#define XARM_HOST_BUILD 1
#include "../../gym_xarm_amd/csrc/xarm_td3_core.h"

using namespace xtd3;

extern "C" {

int64_t t3h_workspace_bytes(const xarm_sacw_layout *l) {
    if (xsacw::layout_error(l)) return -1;
    Dev d = {};
    shape_of(d.s, l);
    return fill_work(d, nullptr);
}

int64_t t3h_param_count(const xarm_sacw_layout *l) {
    if (xsacw::layout_error(l)) return -1;
    Shape s;
    shape_of(s, l);
    return s.P;
}

// row ranges, actor parameters, parameters of one critic, launches of a step, launches of a deterministic act call, trained tensors,
// then the ranges' MAX_SPLIT + 1 row bounds
void t3h_geometry(const xarm_sacw_layout *l, int64_t *out) {
    Shape s;
    shape_of(s, l);
    out[0] = s.S; out[1] = s.Pa; out[2] = s.Pq; out[3] = launches(s.L); out[4] = act_launches(s.L, MODE_DET); out[5] = s.NT;
    for (int k = 0; k <= xsacw::MAX_SPLIT; k++) out[6 + k] = s.rows[k];
}

// where parts of the workspace start, in floats: the delay flag, next_obs | a' [B, D + A], obs | a_pi [B, D + A], y [B]
void t3h_work_offsets(const xarm_sacw_layout *l, int64_t *out) {
    Dev d = {};
    shape_of(d.s, l);
    float *base = (float *)(uintptr_t)4096;
    fill_work(d, base);
    out[0] = (float *)d.flag - base; out[1] = d.xn - base; out[2] = d.xpi - base; out[3] = d.y - base;
}

int t3h_act(const xarm_sacw_layout *l, const xarm_td3_params *p, const xarm_td3_weights *w, int64_t *calls, const float *obs, void *workspace,
            float *out_action) {
    if (xsacw::layout_error(l) || params_error(p) || !w) return -1;
    if (l->batch_size == 0) return 0;
    if (act_pointer_error(l, p, w, calls, obs, workspace, out_action)) return -1;
    Dev d = {};
    shape_of(d.s, l);
    fill_hyper(d.h, p);
    for (int i = 0; i < d.s.tp; i++) d.w[i] = const_cast<float *>(w->actor[i]);
    fill_work_act(d, workspace);
    d.calls = calls; d.obs = obs; d.out_action = out_action;
    HostExec ex;
    run_act(d, ex);
    return 0;
}

// returns the launches of the chain (> 0), or -1 where xarm_td3_update returns XARM_E_INVALID; 0 with batch_size 0
int t3h_update(const xarm_sacw_layout *l, const xarm_td3_params *p, const xarm_td3_weights *w, const xarm_td3_weights *m, const xarm_td3_weights *v,
               int64_t *step, const float *obs, const float *next_obs, const float *action, const float *reward, const float *done, const float *use,
               const float *noise_next, void *workspace, float *out_grad, float *out_target, float *out_q, float *out_dqda, float *out_stats) {
    if (xsacw::layout_error(l) || params_error(p) || !w || !m || !v) return -1;
    if (l->batch_size == 0) return 0;
    if (pointer_error(l, w, m, v, step, obs, next_obs, action, reward, done, workspace)) return -1;
    Dev d = {};
    shape_of(d.s, l);
    fill_hyper(d.h, p);
    tensors_of(d.s, w, d.w, d.tg);
    tensors_of(d.s, m, d.m, nullptr);
    tensors_of(d.s, v, d.v, nullptr);
    fill_work(d, workspace);
    d.step = step;
    d.obs = obs; d.next_obs = next_obs; d.action = action; d.reward = reward; d.done = done; d.use = use; d.noise_next = noise_next;
    d.out_grad = out_grad; d.out_target = out_target; d.out_q = out_q; d.out_dqda = out_dqda; d.out_stats = out_stats;
    HostExec ex;
    run_update(d, ex);
    return ex.count;
}

}  // extern "C"
