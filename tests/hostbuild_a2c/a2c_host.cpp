// Host (g++ -ffp-contract=off) instantiation of gym_xarm_amd/csrc/xarm_a2c_core.h for the CPU-side tests ONLY (tests/test_a2c_host.py,
// tests/test_a2c_gpu.py, and a2c_main.cpp for the sanitizer run).  Never loaded by the product package: gym_xarm_amd runs the update
// through libxarm_hip.so (xarm_k_a2c.hip).  ah_update validates exactly as xarm_a2c_update does and then runs xa2c::host_update on
// NumPy / malloc'd memory; the workspace is not used by the host build (any non-null 16-byte aligned pointer passes).
#define XARM_HOST_BUILD 1
#include "../../gym_xarm_amd/csrc/xarm_a2c_core.h"

using namespace xa2c;

extern "C" {

int64_t ah_workspace_bytes(const xarm_a2c_layout *l) {
    if (layout_error(l)) return -1;
    Shape s;
    Work k;
    fill_shape(s, l);
    fill_work(k, s);
    return k.total;
}

int64_t ah_param_count(const xarm_a2c_layout *l) {
    if (layout_error(l)) return -1;
    Shape s;
    fill_shape(s, l);
    return s.P;
}

// the launch geometry of the gradient kernel for this layout: tiles, groups
void ah_geometry(const xarm_a2c_layout *l, int64_t *out) {
    Shape s;
    fill_shape(s, l);
    out[0] = s.tiles; out[1] = s.G; out[2] = ROWS; out[3] = MAX_GROUPS;
}

int ah_update(const xarm_a2c_layout *l, const xarm_a2c_params *p, const xarm_policy_weights *w, const xarm_policy_weights *sq, const float *obs,
              const float *action, const float *reward, const float *done, const float *use, const float *last_obs, void *workspace,
              float *out_returns, float *out_grad, float *out_stats) {
    if (layout_error(l) || params_error(p) || !w || !sq) return -1;
    if (l->num_envs == 0) return 0;
    if (pointer_error(l, w, sq, obs, action, reward, done, last_obs, workspace)) return -1;
    Shape s;
    Hyper h;
    fill_shape(s, l);
    fill_hyper(h, p);
    float *wt[NTENS], *st[NTENS];
    tensors_of(w, wt);
    tensors_of(sq, st);
    host_update(s, h, wt, st, obs, action, reward, done, use, last_obs, out_returns, out_grad, out_stats);
    return 0;
}

}  // extern "C"
