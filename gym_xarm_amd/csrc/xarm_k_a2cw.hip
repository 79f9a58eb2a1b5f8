// xarm_k_a2cw.hip - the kernels of the wide device-resident A2C update.  Core: xarm_a2cw_core.h, which states the chain of
// launches and every formula; the three GEMM kernels and their launcher are xarm_gemm_tile.h's, shared with the other wide units.
// Built with -ffp-contract=off (build.py UNIT_FLAGS): every float32 operation is the one the host build performs.
//   k_a2cw_returns   one thread per env: the n-step returns down its T rows from the bootstrap value
//   k_a2cw_head      G = min(HEAD_GROUPS, ceil(N / 256)) workgroups: thread t of group g walks rows 256 g + t, + 256 G, ... in float64; the
//                    group's 256 records are added in thread order into the group's slot
//   k_a2cw_reduce    one thread per parameter.  Every workgroup first adds the G slots in g order (thread k the scalar k: the same sums in
//                    every workgroup; workgroup 0 keeps them in the workspace and writes the stats row), then the ranges' partials in
//                    float64 in range order, / n_use, the entropy term, the float32 gradient; a block's sum of squares by the fixed tree
//   k_a2cw_apply     one thread per parameter: the norm from the blocks' sums in block order, the clip, RMSprop
// No atomics anywhere: the same inputs give the same bits.
#include <hip/hip_runtime.h>
#include "xarm_a2cw_core.h"
#include "xarm_gemm_tile.h"
#include "xarm_grad_tile.h"

namespace xa2cw {

__global__ __launch_bounds__(RED) void k_a2cw_returns(Dev d) {
    const int64_t e = (int64_t)blockIdx.x * RED + threadIdx.x;
    if (e < d.E) returns_env(d, e);
}

__global__ __launch_bounds__(RED) void k_a2cw_head(Dev d) {
    __shared__ double red[NSCAL][RED];
    const int t = threadIdx.x;
    double sums[NSCAL] = {};
    head_thread(d, blockIdx.x, t, sums);
#pragma unroll
    for (int k = 0; k < NSCAL; k++) red[k][t] = sums[k];
    __syncthreads();
    if (t < NSCAL) {
        double tot = 0.0;
        for (int k = 0; k < RED; k++) tot += red[t][k];
        d.rec[(int64_t)blockIdx.x * NSCAL + t] = tot;
    }
}

__global__ __launch_bounds__(RED) void k_a2cw_reduce(Dev d) {
    __shared__ double red[RED];
    __shared__ double scal[NSCAL];
    const int t = threadIdx.x;
    const int64_t p = (int64_t)blockIdx.x * RED + t;
    if (t < NSCAL) {
        const double tot = groups_sum(d, t);
        scal[t] = tot;
        if (blockIdx.x == 0) d.scal[t] = tot;
    }
    __syncthreads();
    double sq = 0.0;
    if (p < d.g.P) {
        const float gf = xppow::param_grad(d, scal, p);
        d.grad[p] = gf;
        if (d.out_grad != nullptr) d.out_grad[p] = gf;
        sq = (double)gf * (double)gf;
    }
    sq = xa2c::block_sum(red, sq);
    if (t == 0) {
        d.normpart[blockIdx.x] = sq;
        if (blockIdx.x == 0) finish_stats(d, scal);
    }
}

__global__ __launch_bounds__(RED) void k_a2cw_apply(Dev d) {
    const int64_t p = (int64_t)blockIdx.x * RED + threadIdx.x;
    float norm;
    const float coef = xppow::clip_of(d, d.NB, norm);
    if (p == 0 && d.out_stats != nullptr) d.out_stats[3] = norm;
    if (p < d.g.P) apply_param(d, p, coef);
}

struct DevExec : xsacw::GemmExec {
    void returns(const Dev &d) { k_a2cw_returns<<<dim3(blocks(d.E, RED)), dim3(RED), 0, st>>>(d); count++; }
    void head(const Dev &d) { k_a2cw_head<<<dim3((unsigned)d.G), dim3(RED), 0, st>>>(d); count++; }
    void reduce(const Dev &d) { k_a2cw_reduce<<<dim3((unsigned)d.NB), dim3(RED), 0, st>>>(d); count++; }
    void apply(const Dev &d) { k_a2cw_apply<<<dim3((unsigned)d.NB), dim3(RED), 0, st>>>(d); count++; }
};

int launch_update(const Dev &d, void *stream) {
    DevExec ex = {{(hipStream_t)stream, 0}};
    run_update(d, ex);
    if (ex.count != launches(d.g.L)) return (int)hipErrorLaunchFailure;
    return (int)hipGetLastError();
}

}  // namespace xa2cw
