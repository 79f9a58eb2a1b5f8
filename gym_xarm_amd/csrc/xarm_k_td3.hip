// xarm_k_td3.hip - the kernels of the device-resident TD3 update.  Core: xarm_td3_core.h, which states the chain of
// launches and every formula; this file executes the jobs.  Built with -ffp-contract=off (build.py UNIT_FLAGS).
//
// The three GEMM kernels and the executor part that launches them are xarm_gemm_tile.h's, shared with the wide SAC, MlpPolicy, PPO and
// A2C units; the actor phase launches their gated instantiations with the delay flag as the gate.
//   k_td3_head / k_td3_api / k_td3_act   one thread per row.   k_td3_crit / k_td3_pi   ONE workgroup: thread t walks rows t, t + 256, ...
//                  and keeps float64 sums, added in thread order at the end.
//   k_td3_apply_critics / k_td3_apply_actor   one thread per parameter: the ranges' partials added in float64 in range order, / n_use,
//                  Adam (the actor's launch: and the Polyak step of all three targets).   k_td3_finish   one thread: stats, step.
// k_td3_api, k_td3_pi and k_td3_apply_actor start with the delay flag and return after one uniform read on a delayed call.
// No atomics anywhere: the same inputs give the same bits.
#include <hip/hip_runtime.h>
#include "xarm_td3_core.h"
#include "xarm_gemm_tile.h"

namespace xtd3 {

__global__ __launch_bounds__(RED) void k_td3_head(Dev d) {
    const int64_t n = (int64_t)blockIdx.x * RED + threadIdx.x, t0 = d.step[0];
    if (n == 0) head_first(d, t0);
    if (n < d.s.B) head_row(d, n, t0);
}

// the threads' sums first .. first + COUNT - 1 added in thread order to d.scal
template <int COUNT> __device__ __forceinline__ void store_sums(const Dev &d, const double *sums, int first) {
    __shared__ double red[COUNT][RED];
    const int t = threadIdx.x;
#pragma unroll
    for (int i = 0; i < COUNT; i++) red[i][t] = sums[first + i];
    __syncthreads();
    if (t < COUNT) {
        double tot = 0.0;
        for (int k = 0; k < RED; k++) tot += red[t][k];
        d.scal[first + t] = tot;
    }
}

__global__ __launch_bounds__(RED) void k_td3_crit(Dev d) {
    double sums[NSC] = {0.0, 0.0, 0.0, 0.0};
    for (int64_t n = threadIdx.x; n < d.s.B; n += RED) crit_row(d, n, sums);
    store_sums<3>(d, sums, 0);
}

__global__ __launch_bounds__(RED) void k_td3_apply_critics(Dev d) {
    const int64_t p = d.s.Pa + (int64_t)blockIdx.x * RED + threadIdx.x;
    if (p < d.s.P) apply_critic(d, p);
}

__global__ __launch_bounds__(RED) void k_td3_api(Dev d) {
    if (delayed(d)) return;
    const int64_t n = (int64_t)blockIdx.x * RED + threadIdx.x;
    if (n < d.s.B) api_row(d, n);
}

__global__ __launch_bounds__(RED) void k_td3_pi(Dev d) {
    if (delayed(d)) return;
    double sums[NSC] = {0.0, 0.0, 0.0, 0.0};
    for (int64_t n = threadIdx.x; n < d.s.B; n += RED) pi_row(d, n, sums);
    store_sums<1>(d, sums, 3);
}

__global__ __launch_bounds__(RED) void k_td3_apply_actor(Dev d) {
    if (delayed(d)) return;
    const int64_t p = (int64_t)blockIdx.x * RED + threadIdx.x;
    if (p < d.s.P) apply_actor(d, p);
}

__global__ void k_td3_finish(Dev d) {
    if (blockIdx.x == 0 && threadIdx.x == 0) finish(d);
}

__global__ __launch_bounds__(RED) void k_td3_act(Dev d) {
    const int64_t n = (int64_t)blockIdx.x * RED + threadIdx.x;
    if (n < d.s.B) act_row(d, n);
}

__global__ void k_td3_tick(int64_t *calls) {
    if (blockIdx.x == 0 && threadIdx.x == 0) calls[0] += 1;
}

struct DevExec : xsacw::GemmExec {
    void head(const Dev &d) { k_td3_head<<<dim3(blocks(d.s.B, RED)), dim3(RED), 0, st>>>(d); count++; }
    void crit(const Dev &d) { k_td3_crit<<<dim3(1), dim3(RED), 0, st>>>(d); count++; }
    void apply_critics(const Dev &d) { k_td3_apply_critics<<<dim3(blocks(2 * d.s.Pq, RED)), dim3(RED), 0, st>>>(d); count++; }
    void api(const Dev &d) { k_td3_api<<<dim3(blocks(d.s.B, RED)), dim3(RED), 0, st>>>(d); count++; }
    void pi(const Dev &d) { k_td3_pi<<<dim3(1), dim3(RED), 0, st>>>(d); count++; }
    void apply_actor(const Dev &d) { k_td3_apply_actor<<<dim3(blocks(d.s.P, RED)), dim3(RED), 0, st>>>(d); count++; }
    void finish(const Dev &d) { k_td3_finish<<<dim3(1), dim3(1), 0, st>>>(d); count++; }
    void act(const Dev &d) {
        k_td3_act<<<dim3(blocks(d.s.B, RED)), dim3(RED), 0, st>>>(d);
        count++;
        if (d.h.mode != MODE_DET) k_td3_tick<<<dim3(1), dim3(1), 0, st>>>(d.calls);
    }
};

int launch_update(const Dev &d, void *stream) {
    DevExec ex = {{(hipStream_t)stream, 0}};
    run_update(d, ex);
    if (ex.count != launches(d.s.L)) return (int)hipErrorLaunchFailure;
    return (int)hipGetLastError();
}

int launch_act(const Dev &d, void *stream) {
    DevExec ex = {{(hipStream_t)stream, 0}};
    run_act(d, ex);
    return (int)hipGetLastError();
}

}  // namespace xtd3
