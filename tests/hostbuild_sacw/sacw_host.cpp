// Host (g++ -ffp-contract=off) instantiation of gym_xarm_amd/csrc/xarm_sacw_core.h for the CPU-side tests ONLY (tests/test_sacw_host.py,
// tests/test_sacw_gpu.py, and sacw_main.cpp for the sanitizer run).  Never loaded by the product package: gym_xarm_amd runs the update
// through libxarm_hip.so (xarm_k_sacw.hip).  swh_act / swh_update validate exactly as xarm_sacw_act / xarm_sacw_update do and then run
// the core's own chain (xsacw::run_update / run_act) with xsacw::HostExec on NumPy / malloc'd memory; the workspace is used as the
// device uses it (swh_workspace_bytes bytes, 16-byte aligned).
#define XARM_HOST_BUILD 1
#include "../../gym_xarm_amd/csrc/xarm_sacw_core.h"

using namespace xsacw;

extern "C" {

int64_t swh_workspace_bytes(const xarm_sacw_layout *l) {
    if (layout_error(l)) return -1;
    Dev d = {};
    fill_shape(d.s, l);
    return fill_work(d, nullptr);
}

int64_t swh_param_count(const xarm_sacw_layout *l) {
    if (layout_error(l)) return -1;
    Shape s;
    fill_shape(s, l);
    return s.P;
}

// the geometry for this layout: row ranges, the most ranges, rows per tile of a range, actor parameters, parameters of one critic, launches of
// a step, launches of an act call, trained tensors, then the ranges' MAX_SPLIT + 1 row bounds and the NT + 1 offsets of the flat gradient
void swh_geometry(const xarm_sacw_layout *l, int64_t *out) {
    Shape s;
    fill_shape(s, l);
    out[0] = s.S; out[1] = MAX_SPLIT; out[2] = SPLIT_ROWS; out[3] = s.Pa; out[4] = s.Pq; out[5] = launches(s.L); out[6] = act_launches(s.L); out[7] = s.NT;
    for (int k = 0; k <= MAX_SPLIT; k++) out[8 + k] = s.rows[k];
    for (int k = 0; k <= s.NT; k++) out[8 + MAX_SPLIT + 1 + k] = s.off[k];
}

// where the per-row parts of the workspace start, in floats: logp_pi [B], logp' [B], z_pi [B, A], obs | a_pi [B, D + A], next_obs | a' [B, D + A], y [B]
void swh_work_offsets(const xarm_sacw_layout *l, int64_t *out) {
    Dev d = {};
    fill_shape(d.s, l);
    float *base = (float *)(uintptr_t)4096;
    fill_work(d, base);
    out[0] = d.logp - base; out[1] = d.lpn - base; out[2] = d.z - base; out[3] = d.xpi - base; out[4] = d.xn - base; out[5] = d.y - base;
}

int swh_act(const xarm_sacw_layout *l, const xarm_sac_params *p, const xarm_sacw_weights *w, int64_t *calls, const float *obs, void *workspace,
            float *out_action, float *out_logp) {
    if (layout_error(l) || !p || !w) return -1;
    if (l->batch_size == 0) return 0;
    if (act_pointer_error(l, p, w, calls, obs, workspace, out_action)) return -1;
    Dev d = {};
    fill_shape(d.s, l);
    d.h.seed = p->seed;
    d.h.deterministic = p->deterministic != 0;
    for (int i = 0; i < d.s.tp; i++) d.w[i] = const_cast<float *>(w->actor[i]);
    fill_work_act(d, workspace);
    d.calls = calls; d.obs = obs; d.out_action = out_action; d.out_logp = out_logp;
    HostExec ex;
    run_act(d, ex);
    return 0;
}

int swh_update(const xarm_sacw_layout *l, const xarm_sac_params *p, const xarm_sacw_weights *w, const xarm_sacw_weights *m, const xarm_sacw_weights *v,
               int64_t *step, const float *obs, const float *next_obs, const float *action, const float *reward, const float *done, const float *use,
               const float *noise_pi, const float *noise_next, void *workspace, float *out_grad, float *out_dqda, float *out_target, float *out_stats,
               float *out_q) {
    if (layout_error(l) || xsac::params_error(p) || !w || !m || !v) return -1;
    if (l->batch_size == 0) return 0;
    if (pointer_error(l, w, m, v, step, obs, next_obs, action, reward, done, workspace)) return -1;
    Dev d = {};
    fill_shape(d.s, l);
    xsac::fill_hyper(d.h, p);
    tensors_of(d.s, w, d.w, d.tq);
    tensors_of(d.s, m, d.m, nullptr);
    tensors_of(d.s, v, d.v, nullptr);
    fill_work(d, workspace);
    d.step = step;
    d.obs = obs; d.next_obs = next_obs; d.action = action; d.reward = reward; d.done = done; d.use = use; d.noise_pi = noise_pi; d.noise_next = noise_next;
    d.out_grad = out_grad; d.out_dqda = out_dqda; d.out_target = out_target; d.out_stats = out_stats; d.out_q = out_q;
    HostExec ex;
    run_update(d, ex);
    return 0;
}

}  // extern "C"
