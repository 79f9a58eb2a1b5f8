// Host (g++ -ffp-contract=off) instantiation of gym_xarm_amd/csrc/xarm_sac_core.h for the CPU-side tests ONLY (tests/test_sac_host.py,
// tests/test_sac_gpu.py, and sac_main.cpp for the sanitizer run).  Never loaded by the product package: gym_xarm_amd runs the update
// through libxarm_hip.so (xarm_k_sac.hip).  sh_act / sh_update validate exactly as xarm_sac_act / xarm_sac_update do and then run
// xsac::host_act / xsac::host_update on NumPy / malloc'd memory; the workspace is not used by the host build (any non-null 16-byte
// aligned pointer passes).
#define XARM_HOST_BUILD 1
#include "../../gym_xarm_amd/csrc/xarm_sac_core.h"

using namespace xsac;

extern "C" {

int64_t sh_workspace_bytes(const xarm_sac_layout *l) {
    if (layout_error(l)) return -1;
    Shape s;
    Work k;
    fill_shape(s, l);
    fill_work(k, s);
    return k.total;
}

int64_t sh_param_count(const xarm_sac_layout *l) {
    if (layout_error(l)) return -1;
    Shape s;
    fill_shape(s, l);
    return s.P;
}

// the launch geometry for this layout: tiles, groups, rows per tile, the most groups, actor parameters, parameters of one critic, launches
void sh_geometry(const xarm_sac_layout *l, int64_t *out) {
    Shape s;
    fill_shape(s, l);
    out[0] = s.tiles; out[1] = s.G; out[2] = ROWS; out[3] = MAX_GROUPS; out[4] = s.Pa; out[5] = s.Pq; out[6] = 6;
}

int sh_act(const xarm_sac_layout *l, const xarm_sac_params *p, const xarm_sac_weights *w, int64_t *calls, const float *obs, float *out_action,
           float *out_logp) {
    if (layout_error(l) || !p || !w) return -1;
    if (l->batch_size == 0) return 0;
    if (act_pointer_error(p, w, calls, obs, out_action)) return -1;
    Shape s;
    Hyper h = {};
    fill_shape(s, l);
    h.seed = p->seed;
    h.deterministic = p->deterministic != 0;
    host_act(s, h, tower_of(w->actor), calls, obs, out_action, out_logp);
    return 0;
}

int sh_update(const xarm_sac_layout *l, const xarm_sac_params *p, const xarm_sac_weights *w, const xarm_sac_weights *m, const xarm_sac_weights *v,
              int64_t *step, const float *obs, const float *next_obs, const float *action, const float *reward, const float *done, const float *use,
              const float *noise_pi, const float *noise_next, void *workspace, float *out_grad, float *out_dqda, float *out_target, float *out_stats) {
    if (layout_error(l) || params_error(p) || !w || !m || !v) return -1;
    if (l->batch_size == 0) return 0;
    if (pointer_error(w, m, v, step, obs, next_obs, action, reward, done, workspace)) return -1;
    Shape s;
    Hyper h;
    fill_shape(s, l);
    fill_hyper(h, p);
    float *wt[NT], *mt[NT], *vt[NT], *tq[12];
    tensors_of(w, wt);
    tensors_of(m, mt);
    tensors_of(v, vt);
    for (int i = 0; i < 6; i++) {
        tq[i] = const_cast<float *>(w->q1_target[i]);
        tq[6 + i] = const_cast<float *>(w->q2_target[i]);
    }
    host_update(s, h, wt, tq, mt, vt, step, obs, next_obs, action, reward, done, use, noise_pi, noise_next, out_grad, out_dqda, out_target, out_stats);
    return 0;
}

}  // extern "C"
