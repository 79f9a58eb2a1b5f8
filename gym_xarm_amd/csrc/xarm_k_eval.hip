// xarm_k_eval.hip - the kernels of the device-resident policy evaluation.  Core: xarm_eval_core.h.
// Built with -ffp-contract=off (build.py UNIT_FLAGS): every float64 operation is the IEEE one the host build performs.
//
//   k_eval_begin    grid-stride: zeroes cur_ret, cur_len, count and the records, remaining = N.
//   k_eval_step     one thread per env, 256 to a workgroup.  Each env's accounting touches its own words only; the records a
//                   wavefront wrote are counted by a 64-bit ballot and popcount and taken off `remaining` by lane 0 with one
//                   integer vector atomic per wavefront - an integer sum, so the order of the wavefronts cannot show.
//   k_eval_summary  one workgroup of 256: thread t's partials over the slots t, t + 256, ... go to LDS, every thread merges them
//                   in thread order (the same value in every thread), then the squared deviations the same way; thread 0 writes.
// No floating-point atomics, no allocation, no host read: all three can be captured in a graph.
#include <hip/hip_runtime.h>
#include "xarm_eval_core.h"

namespace xeval {

constexpr int WAVE = 64;

__global__ __launch_bounds__(THREADS) void k_eval_begin(StepArgs a) {
    const int64_t tid = (int64_t)blockIdx.x * THREADS + threadIdx.x, stride = (int64_t)gridDim.x * THREADS;
    for (int64_t i = tid; i < a.L.E; i += stride) {
        a.cur_ret[i] = 0.0; a.cur_len[i] = 0; a.count[i] = 0;
    }
    for (int64_t i = tid; i < 3 * (int64_t)a.L.N; i += stride) a.records[i] = 0.0;
    if (tid == 0) a.remaining[0] = a.L.N;
}

__global__ __launch_bounds__(THREADS) void k_eval_step(StepArgs a) {
    const int64_t i = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    const int wrote = i < a.L.E ? eval_step_env(a, (int32_t)i) : 0;
    const unsigned long long m = __ballot(wrote != 0);
    if ((threadIdx.x & (WAVE - 1)) == 0 && m != 0ull) atomicSub(a.remaining, __popcll(m));
}

__global__ __launch_bounds__(THREADS) void k_eval_summary(SummaryArgs a) {
    __shared__ Part1 p1[THREADS];
    __shared__ Part2 p2[THREADS];
    const int t = threadIdx.x;
    p1[t] = summary_part1(a, t);
    __syncthreads();
    const Part1 m = summary_merge1(p1);
    const double n = (double)m.n;
    p2[t] = summary_part2(a, t, m.sum_r / n, m.sum_l / n);
    __syncthreads();
    if (t == 0) summary_write(a, m, summary_merge2(p2));
}

static unsigned blocks_for(int64_t n, int64_t cap) {
    int64_t b = (n + THREADS - 1) / THREADS;
    if (b < 1) b = 1;
    return (unsigned)(b < cap ? b : cap);
}

int launch_eval_begin(const StepArgs &a, void *stream) {
    const int64_t n = 3 * (int64_t)a.L.N > a.L.E ? 3 * (int64_t)a.L.N : a.L.E;
    k_eval_begin<<<dim3(blocks_for(n, 1024)), dim3(THREADS), 0, (hipStream_t)stream>>>(a);
    return (int)hipGetLastError();
}

int launch_eval_step(const StepArgs &a, void *stream) {
    k_eval_step<<<dim3(blocks_for(a.L.E, (int64_t)1 << 30)), dim3(THREADS), 0, (hipStream_t)stream>>>(a);
    return (int)hipGetLastError();
}

int launch_eval_summary(const SummaryArgs &a, void *stream) {
    k_eval_summary<<<dim3(1), dim3(THREADS), 0, (hipStream_t)stream>>>(a);
    return (int)hipGetLastError();
}

}  // namespace xeval
