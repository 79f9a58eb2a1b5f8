// xarm_k_sacw.hip - the kernels of the wide device-resident SAC update.  Core: xarm_sacw_core.h, which states the chain of
// launches, the jobs and every formula; this file executes the jobs.  Built with -ffp-contract=off (build.py UNIT_FLAGS).
//
// The three GEMM kernels (k_sacw_fwd, k_sacw_bd, k_sacw_wg) and the executor part that launches them are in xarm_gemm_tile.h, shared with
// the wide MlpPolicy unit (xarm_k_acw.hip).
//   k_sacw_head / k_sacw_act   one thread per row.   k_sacw_crit / k_sacw_pi   ONE workgroup: thread t walks rows t, t + 256, ... and
//                  keeps float64 sums, added in thread order at the end (a few floats per row: microseconds at 65 536 rows).
//   k_sacw_apply   one thread per parameter: the ranges' partials added in float64 in range order, / n_use, Adam (and Polyak);
//                  the actor's launch has one more thread for log_alpha, the stats and the step count.
// No atomics anywhere: the same inputs give the same bits.
#include <hip/hip_runtime.h>
#include "xarm_sacw_core.h"
#include "xarm_gemm_tile.h"

namespace xsacw {

// ------------------------------------------------------------------------------------------------------------ rows and parameters
__global__ __launch_bounds__(RED) void k_sacw_head(Dev d) {
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

__global__ __launch_bounds__(RED) void k_sacw_crit(Dev d) {
    double sums[NSC] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int64_t n = threadIdx.x; n < d.s.B; n += RED) crit_row(d, n, sums);
    store_sums<4>(d, sums, 0);
}

__global__ __launch_bounds__(RED) void k_sacw_pi(Dev d) {
    double sums[NSC] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int64_t n = threadIdx.x; n < d.s.B; n += RED) pi_row(d, n, sums);
    store_sums<2>(d, sums, 4);
}

__global__ __launch_bounds__(RED) void k_sacw_apply(Dev d, int64_t p0, int64_t count, int64_t pstride, int targets, int last) {
    const int64_t e = (int64_t)blockIdx.x * RED + threadIdx.x;
    if (e < count) apply_param(d, p0 + e, d.partial + e, pstride, targets != 0);
    else if (e == count && last) finish(d);
}

__global__ __launch_bounds__(RED) void k_sacw_act(Dev d) {
    const int64_t n = (int64_t)blockIdx.x * RED + threadIdx.x;
    if (n < d.s.B) act_row(d, n);
}

__global__ void k_sacw_tick(int64_t *calls) {
    if (blockIdx.x == 0 && threadIdx.x == 0) calls[0] += 1;
}

struct DevExec : GemmExec {
    void head(const Dev &d) { k_sacw_head<<<dim3(blocks(d.s.B, RED)), dim3(RED), 0, st>>>(d); count++; }
    void crit(const Dev &d) { k_sacw_crit<<<dim3(1), dim3(RED), 0, st>>>(d); count++; }
    void pi(const Dev &d) { k_sacw_pi<<<dim3(1), dim3(RED), 0, st>>>(d); count++; }
    void apply(const Dev &d, int64_t p0, int64_t n, int64_t pstride, bool targets, bool last) {
        k_sacw_apply<<<dim3(blocks(n + (last ? 1 : 0), RED)), dim3(RED), 0, st>>>(d, p0, n, pstride, targets ? 1 : 0, last ? 1 : 0);
        count++;
    }
    void act(const Dev &d) {
        k_sacw_act<<<dim3(blocks(d.s.B, RED)), dim3(RED), 0, st>>>(d);
        count++;
        if (!d.h.deterministic) k_sacw_tick<<<dim3(1), dim3(1), 0, st>>>(d.calls);
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

}  // namespace xsacw
