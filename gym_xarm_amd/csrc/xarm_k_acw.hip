// xarm_k_acw.hip - the kernels of the wide device-resident MlpPolicy.  Core: xarm_acw_core.h, which states the chain of
// launches and the per-row formulas; the forward's GEMM kernel and its launcher are xarm_gemm_tile.h's, shared with the wide SAC unit.
// Built with -ffp-contract=off (build.py UNIT_FLAGS): every float32 operation is the one the host build performs.
//   k_acw_prep   one thread per (row, column): observation | achieved_goal | desired_goal, normalised when asked, into the workspace
//   k_sacw_fwd   L + 1 launches, one job per tower
//   k_acw_head   one thread per row: noise, action, env_action, logp, value
//   k_acw_tick   one thread: calls += 1 behind a stochastic call's head
#include <hip/hip_runtime.h>
#include "xarm_acw_core.h"
#include "xarm_gemm_tile.h"

namespace xacw {

constexpr int RED = xsacw::RED;

__global__ __launch_bounds__(RED) void k_acw_prep(Dev d) {
    const int64_t i = (int64_t)blockIdx.x * RED + threadIdx.x;
    const int D = d.a.D;
    if (i < d.s.B * D) prep_at(d, i / D, (int)(i % D));
}

__global__ __launch_bounds__(RED) void k_acw_head(Dev d) {
    const int64_t n = (int64_t)blockIdx.x * RED + threadIdx.x;
    if (n < d.s.B) head_row(d, n);
}

__global__ void k_acw_tick(int64_t *calls) {
    if (blockIdx.x == 0 && threadIdx.x == 0) calls[0] += 1;
}

struct DevExec : xsacw::GemmExec {
    void prep(const Dev &d) { k_acw_prep<<<dim3(blocks(d.s.B * d.a.D, RED)), dim3(RED), 0, st>>>(d); count++; }
    void head(const Dev &d) { k_acw_head<<<dim3(blocks(d.s.B, RED)), dim3(RED), 0, st>>>(d); count++; }
};

int launch_act(const Dev &d, int64_t *calls, void *stream) {
    DevExec ex = {{(hipStream_t)stream, 0}};
    run_act(d, ex);
    if (ex.count != act_launches(d.s.L)) return (int)hipErrorLaunchFailure;
    if (!d.a.deterministic) k_acw_tick<<<dim3(1), dim3(1), 0, ex.st>>>(calls);
    return (int)hipGetLastError();
}

}  // namespace xacw
