// Host (g++ -ffp-contract=off) instantiation of gym_xarm_amd/csrc/xarm_a2cw_core.h for the CPU-side tests ONLY (tests/test_a2cw_host.py,
// tests/test_a2cw_gpu.py, and a2cw_main.cpp for the sanitizer run).  Never loaded by the product package: gym_xarm_amd runs the call
// through libxarm_hip.so (xarm_k_a2cw.hip).  awh_update validates exactly as xarm_a2cw_update does and then runs the core's own chain
// (xa2cw::run_update) with the host executor on NumPy / malloc'd memory; the workspace is used as the device uses it.
#define XARM_HOST_BUILD 1
#include "../../gym_xarm_amd/csrc/xarm_a2cw_core.h"

// counts what the chain hands the executor: the launches of the device
struct CountExec : xa2cw::HostExec {
    int count = 0;
    void fwd(const xsacw::Fwd &f) { xa2cw::HostExec::fwd(f); count++; }
    void bd(const xsacw::Bd &f) { xa2cw::HostExec::bd(f); count++; }
    void wg(const xsacw::Wg &f) { xa2cw::HostExec::wg(f); count++; }
    void returns(const xa2cw::Dev &d) { xa2cw::HostExec::returns(d); count++; }
    void head(const xa2cw::Dev &d) { xa2cw::HostExec::head(d); count++; }
    void reduce(const xa2cw::Dev &d) { xa2cw::HostExec::reduce(d); count++; }
    void apply(const xa2cw::Dev &d) { xa2cw::HostExec::apply(d); count++; }
};

extern "C" {

int64_t awh_workspace_bytes(const xarm_a2cw_layout *l) {
    if (xa2cw::layout_error(l)) return -1;
    xa2cw::Dev d = {};
    xa2cw::fill_shape(d, l);
    return xa2cw::fill_work(d, nullptr);
}

// parameters, rows, head groups, the most head groups, launches, row ranges, tensors, parameter blocks, then the ranges' 17 row bounds, the
// NT + 1 offsets of the flat gradient, and where value, ret, mean, the hidden activations and grad start in the workspace (in floats)
void awh_geometry(const xarm_a2cw_layout *l, int64_t *out) {
    xa2cw::Dev d = {};
    xa2cw::fill_shape(d, l);
    float *base = (float *)(uintptr_t)4096;
    xa2cw::fill_work(d, base);
    out[0] = d.g.P; out[1] = d.N; out[2] = d.G; out[3] = xa2cw::HEAD_GROUPS; out[4] = xa2cw::launches(d.g.L); out[5] = d.g.S; out[6] = d.g.NT; out[7] = d.NB;
    for (int k = 0; k <= xsacw::MAX_SPLIT; k++) out[8 + k] = d.g.rows[k];
    for (int k = 0; k <= d.g.NT; k++) out[25 + k] = d.g.off[k];
    out[43] = d.value - base; out[44] = d.ret - base; out[45] = d.mean - base; out[46] = d.hid - base; out[47] = d.grad - base;
}

// returns 0, or -1 for a refused call; *launched (nullable): what the chain handed the executor
int awh_update(const xarm_a2cw_layout *l, const xarm_a2c_params *p, const xarm_acw_weights *w, const xarm_acw_weights *sq, const float *obs,
               const float *action, const float *reward, const float *done, const float *use, const float *last_obs, void *workspace,
               float *out_returns, float *out_grad, float *out_stats, int64_t *launched) {
    if (launched) *launched = 0;
    if (xa2cw::layout_error(l) || xa2c::params_error(p) || !w || !sq) return -1;
    if (l->num_envs == 0) return 0;
    if (xa2cw::pointer_error(l, w, sq, obs, action, reward, done, last_obs, workspace)) return -1;
    xa2cw::Dev d = {};
    xa2cw::fill_shape(d, l);
    xa2c::fill_hyper(d.h, p);
    xppow::tensors_of(d, w, d.w);
    xppow::tensors_of(d, sq, d.sq);
    xa2cw::fill_work(d, workspace);
    d.obs = obs; d.action = action; d.reward = reward; d.done = done; d.use = use; d.last_obs = last_obs;
    d.out_returns = out_returns; d.out_grad = out_grad; d.out_stats = out_stats;
    CountExec ex;
    xa2cw::run_update(d, ex);
    if (launched) *launched = ex.count;
    return 0;
}

}  // extern "C"
