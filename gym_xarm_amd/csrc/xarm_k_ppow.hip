// xarm_k_ppow.hip - the kernels of the wide device-resident PPO update.  Core: xarm_ppow_core.h, which states the chain of
// launches and every formula; the three GEMM kernels and their launcher are xarm_gemm_tile.h's, shared with the wide SAC unit.
// Built with -ffp-contract=off (build.py UNIT_FLAGS): every float32 operation is the one the host build performs.
//   k_ppow_gae       one thread per rollout row: old_logp (unless given); the threads of the first E rows: their env's GAE recursion
//   k_ppow_advstats  one workgroup per optimiser step: thread t walks positions t, t + 256, ... in float64; thread 0 adds the 256
//                    partials in t order
//   k_ppow_gather    one thread per (position, column) of the step's minibatch
//   k_ppow_head      ONE workgroup: thread t walks rows t, t + 256, ..., the 256 records are added in t order (instantiated with and
//                    without clip_range_vf: a branch in the row loop cost the call without the option 1.5 %)
//   k_ppow_reduce    one thread per parameter: the ranges' partials added in float64 in range order, / n_use, the entropy term, the float32
//                    gradient; a block's sum of squares by the fixed tree; block 0's thread 0: step, Adam's scalars, the stats row
//   k_ppow_apply     one thread per parameter: the norm from the blocks' sums in block order, the clip, Adam
// With target_kl on, the gather, head, reduce and apply of a stopped step return after one uniform read of the stop flag (the reduce
// writes the stopped stats row first), and so do the GEMM launches between them, through their header's gate (xarm_ppow_core.h).  The
// read sits in the KL = true instantiations, which only a call with target_kl launches: a call without it runs the kernels it always ran
// (the check ahead of every kernel cost a launch-bound update of 1 024-row minibatches 2 - 3 %).
// No atomics anywhere: the same inputs and perm give the same bits.
#include <hip/hip_runtime.h>
#include "xarm_ppow_core.h"
#include "xarm_gemm_tile.h"
#include "xarm_grad_tile.h"

namespace xppow {

__global__ __launch_bounds__(RED) void k_ppow_gae(Dev d) {
    const int64_t n = (int64_t)blockIdx.x * RED + threadIdx.x;
    if (n < d.p.a.N) gae_row(d, n);
}

// the 256 threads' values added in thread order by thread 0; every thread gets the sum
__device__ __forceinline__ double ordered_sum(double *red, double x) {
    __syncthreads();
    red[threadIdx.x] = x;
    __syncthreads();
    if (threadIdx.x == 0) {
        double tot = 0.0;
        for (int k = 0; k < RED; k++) tot += red[k];
        red[0] = tot;
    }
    __syncthreads();
    return red[0];
}

__global__ __launch_bounds__(RED) void k_ppow_advstats(Dev d) {
    __shared__ double red[RED];
    const int t = threadIdx.x;
    const int64_t st = blockIdx.x;
    double n, sa;
    adv_sums(d, st, t, n, sa);
    n = ordered_sum(red, n);
    sa = ordered_sum(red, sa);
    const double mu = mean_of(n, sa);
    const double sv = ordered_sum(red, adv_squares(d, st, t, mu));
    if (t == 0) xppo::finish_stats(d.musig + st * NMS, n, mu, sv, d.h.normalize);
}

template <bool KL> __global__ __launch_bounds__(RED) void k_ppow_gather(Dev d, int64_t st) {
    if (KL && xppo::stopped_before(d.h, d.stop, st)) return;
    const int W = gather_width(d);
    const int64_t i = (int64_t)blockIdx.x * RED + threadIdx.x;
    if (i < d.g.B * W) gather_at(d, st, i / W, (int)(i % W));
}

template <bool VCLIP, bool KL> __global__ __launch_bounds__(RED) void k_ppow_head(Dev d, int64_t st) {
    if (KL && xppo::stopped_before(d.h, d.stop, st)) return;
    __shared__ double red[NSCAL][RED];
    const int t = threadIdx.x;
    double sums[NSCAL] = {};
    for (int64_t i = t; i < d.g.B; i += RED) head_row<VCLIP>(d, i, sums);
#pragma unroll
    for (int k = 0; k < NSCAL; k++) red[k][t] = sums[k];
    __syncthreads();
    if (t < NSCAL) {
        double tot = 0.0;
        for (int k = 0; k < RED; k++) tot += red[t][k];
        d.scal[t] = tot;
    }
}

template <bool KL> __global__ __launch_bounds__(RED) void k_ppow_reduce(Dev d, int64_t st) {
    if (KL && xppo::stopped_before(d.h, d.stop, st)) {
        if (blockIdx.x == 0 && threadIdx.x == 0) skip_step(d, st);
        return;
    }
    __shared__ double red[RED];
    const int64_t p = (int64_t)blockIdx.x * RED + threadIdx.x;
    double sq = 0.0;
    if (p < d.g.P) {
        const float gf = param_grad(d, p);
        d.grad[p] = gf;
        if (st == 0 && d.out_grad != nullptr) d.out_grad[p] = gf;
        sq = (double)gf * (double)gf;
    }
    sq = xa2c::block_sum(red, sq);
    if (threadIdx.x == 0) {
        d.normpart[blockIdx.x] = sq;
        if (blockIdx.x == 0) finish_step(d, st);
    }
}

template <bool KL> __global__ __launch_bounds__(RED) void k_ppow_apply(Dev d, int64_t st) {
    if (KL && xppo::stopped_at(d.h, d.stop)) return;
    const int64_t p = (int64_t)blockIdx.x * RED + threadIdx.x;
    float norm;
    const float coef = clip_of(d, norm);
    if (p == 0 && d.out_stats != nullptr) d.out_stats[st * 8 + 3] = norm;
    if (p < d.g.P) apply_param(d, p, coef);
}

struct DevExec : xsacw::GemmExec {
    void gae(const Dev &d) { k_ppow_gae<<<dim3(blocks(d.p.a.N, RED)), dim3(RED), 0, st>>>(d); count++; }
    void advstats(const Dev &d) { k_ppow_advstats<<<dim3((unsigned)d.p.S), dim3(RED), 0, st>>>(d); count++; }
    static bool kl(const Dev &d) { return d.h.kl_limit > 0.0; }
    void gather(const Dev &d, int64_t s) {
        const dim3 grid(blocks(d.g.B * (d.g.D + d.g.A + (d.h.vclip > 0.0f ? 5 : 4)), RED));
        if (kl(d)) k_ppow_gather<true><<<grid, dim3(RED), 0, st>>>(d, s);
        else k_ppow_gather<false><<<grid, dim3(RED), 0, st>>>(d, s);
        count++;
    }
    void head(const Dev &d, int64_t s) {
        const bool vclip = d.h.vclip > 0.0f;
        if (kl(d)) {
            if (vclip) k_ppow_head<true, true><<<dim3(1), dim3(RED), 0, st>>>(d, s);
            else k_ppow_head<false, true><<<dim3(1), dim3(RED), 0, st>>>(d, s);
        } else {
            if (vclip) k_ppow_head<true, false><<<dim3(1), dim3(RED), 0, st>>>(d, s);
            else k_ppow_head<false, false><<<dim3(1), dim3(RED), 0, st>>>(d, s);
        }
        count++;
    }
    void reduce(const Dev &d, int64_t s) {
        const dim3 grid((unsigned)d.p.a.NB);
        if (kl(d)) k_ppow_reduce<true><<<grid, dim3(RED), 0, st>>>(d, s);
        else k_ppow_reduce<false><<<grid, dim3(RED), 0, st>>>(d, s);
        count++;
    }
    void apply(const Dev &d, int64_t s) {
        const dim3 grid((unsigned)d.p.a.NB);
        if (kl(d)) k_ppow_apply<true><<<grid, dim3(RED), 0, st>>>(d, s);
        else k_ppow_apply<false><<<grid, dim3(RED), 0, st>>>(d, s);
        count++;
    }
};

int launch_update(const Dev &d, void *stream) {
    DevExec ex = {{(hipStream_t)stream, 0}};
    run_update(d, ex);
    if ((int64_t)ex.count != launches(d.g.L, d.p.S, d.CN + d.CE)) return (int)hipErrorLaunchFailure;
    return (int)hipGetLastError();
}

}  // namespace xppow
