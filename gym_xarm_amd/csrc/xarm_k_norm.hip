// xarm_k_norm.hip - the kernels of the device-resident VecNormalize + episode monitor.  Core: xarm_norm_core.h.
// Built with -ffp-contract=off (build.py UNIT_FLAGS): every float64 operation is the IEEE one the host build performs.
//
// Three plain launches per call, stream order the only synchronisation between them:
//   k_norm_partial  one workgroup of 256 per chunk of 128 envs.  The chunk's rows are read the way they lie in memory - lane i
//                   at base + 4 i of each of the up to three row-major inputs - and staged in LDS as float32 [rows, D + 1] with
//                   the new return as the last column; (column, segment) pairs are then spread over the threads, consecutive
//                   threads on consecutive columns of one row (consecutive LDS banks).  Writes the chunk's (n, mean, M2) per
//                   column and its count of finished envs to the workspace.
//   k_norm_merge    one workgroup: thread j merges column j's partials in chunk order and updates the running statistics;
//                   then the exclusive prefix of the finished counts (integers: any order gives the same sums) and n.
//   k_norm_apply    one workgroup per chunk: sqrt(var + eps) per column once into LDS, the per-env scalars on the chunk's two
//                   wavefronts (the rank of a finished env is the chunk's prefix + the finished envs of the lower wavefront +
//                   the popcount of the 64-bit ballot below its lane), the [rows, D] normalisation on all four.
// With update == 0 the partial launch only counts finished envs and the merge launch only scans them (the observation-only
// call then runs k_norm_apply alone): the monitor still needs the prefix, and n cannot be advanced in the launch that reads it.
#include <hip/hip_runtime.h>
#include "xarm_norm_core.h"

namespace xnorm {

constexpr int WAVE = 64, THREADS = 256;

// the up to three inputs of chunk rows [r0, r0 + rows) -> tile[r * stride + col], coalesced on the global side
__device__ __forceinline__ void stage_part(float *tile, int stride, int col0, const float *src, int w, int64_t r0, int rows) {
    const float *base = src + r0 * w;
    for (int i = threadIdx.x; i < rows * w; i += THREADS) {
        const int r = i / w, k = i - r * w;
        tile[r * stride + col0 + k] = base[i];
    }
}

__global__ __launch_bounds__(THREADS) void k_norm_partial(Args a) {
    extern __shared__ double lds[];
    const Layout &L = a.L;
    const int nc = ncols(a), stride = nc;
    const int64_t c = blockIdx.x, r0 = c * CHUNK;
    const int rows = (int)(L.E - r0 < CHUNK ? L.E - r0 : CHUNK);
    const int tid = threadIdx.x;
    __shared__ int wfin[2];
    __shared__ int segn[NSEG];
    __shared__ uint8_t kf[CHUNK];
    // finished envs of the chunk: one ballot per wavefront of envs
    if (a.step && tid < CHUNK) {
        const bool d = tid < rows && a.done[r0 + tid] != 0;
        const unsigned long long m = __ballot(d);
        if ((tid & (WAVE - 1)) == 0) wfin[tid >> 6] = __popcll(m);
    }
    if (!a.update) {
        __syncthreads();
        if (tid == 0) a.fin[c] = a.step ? wfin[0] + wfin[1] : 0;
        return;
    }
    double *segv = lds;                          // [NSEG, nc]
    double *meanv = segv + NSEG * nc;            // [nc]
    float *tile = (float *)(meanv + nc);         // [CHUNK, nc]
    stage_part(tile, stride, 0, a.obs, L.obs, r0, rows);
    if (L.goal > 0) {
        stage_part(tile, stride, L.obs, a.ag, L.goal, r0, rows);
        stage_part(tile, stride, L.obs + L.goal, a.dg, L.goal, r0, rows);
    }
    if (tid < CHUNK) {
        kf[tid] = tid < rows && kept(a, r0 + tid) ? 1 : 0;      // rows past the batch are never kept
        if (a.step && tid < rows) tile[tid * stride + L.D] = ret_next(a.ret[r0 + tid], a.gamma, a.rew[r0 + tid]);
    }
    __syncthreads();
    for (int i = tid; i < NSEG * nc; i += THREADS) {
        const int s = i / nc, j = i - s * nc;
        segv[i] = seg_sum(tile, stride, j, kf, s * SEG, s * SEG + SEG);
        if (j == 0) segn[s] = seg_count(kf, s * SEG, s * SEG + SEG);
    }
    __syncthreads();
    int n = 0;
    for (int s = 0; s < NSEG; s++) n += segn[s];
    if (tid < nc) meanv[tid] = n > 0 ? seg_combine(segv + tid, nc) / (double)n : 0.0;
    __syncthreads();
    for (int i = tid; i < NSEG * nc; i += THREADS) {
        const int s = i / nc, j = i - s * nc;
        segv[i] = seg_sq(tile, stride, j, kf, s * SEG, s * SEG + SEG, meanv[j]);
    }
    __syncthreads();
    double *p = a.part + c * L.W;
    if (tid < nc) {
        p[1 + tid] = meanv[tid];
        p[1 + (L.D + 1) + tid] = seg_combine(segv + tid, nc);
    }
    if (tid == 0) {
        p[0] = (double)n;
        a.fin[c] = a.step ? wfin[0] + wfin[1] : 0;
    }
}

__global__ __launch_bounds__(THREADS) void k_norm_merge(Args a) {
    const Layout &L = a.L;
    const int tid = threadIdx.x, nc = ncols(a);
    __shared__ int64_t run[THREADS];
    if (a.update) {
        const double obs_count = a.stats[2 * L.D + 2], ret_count = a.stats[2 * L.D + 3];
        __syncthreads();                          // every thread holds the counts before thread 0 / D replaces them
        if (tid < nc) {
            const double count = tid < L.D ? obs_count : ret_count;
            const double n = merge_column(a, tid, count);
            if (n > 0.0 && tid == 0) a.stats[2 * L.D + 2] = obs_count + n;
            if (n > 0.0 && tid == L.D) a.stats[2 * L.D + 3] = ret_count + n;
        }
    }
    if (!a.step) return;
    // exclusive prefix of fin over chunks: thread t owns the chunks [t per, (t + 1) per)
    const int64_t per = (L.chunks + THREADS - 1) / THREADS;
    const int64_t lo = tid * per < L.chunks ? tid * per : L.chunks, hi = lo + per < L.chunks ? lo + per : L.chunks;
    int64_t s = 0;
    for (int64_t c = lo; c < hi; c++) s += a.fin[c];
    run[tid] = s;
    __syncthreads();
    int64_t before = 0;
    for (int t = 0; t < tid; t++) before += run[t];
    for (int64_t c = lo; c < hi; c++) {
        a.prefix[c] = before;
        before += a.fin[c];
    }
    if (tid == THREADS - 1) {                     // `before` is the call's total here
        const int64_t n = a.n[0];
        a.n_base[0] = n;
        a.n[0] = n + before;
    }
}

__device__ __forceinline__ void norm_part(const Args &a, const double *meanv, const double *denomv, int col0, const float *src, int w,
                                          int64_t r0, int rows) {
    const float *base = src + r0 * w;
    float *out = a.nobs + r0 * a.L.D;
    for (int i = threadIdx.x; i < rows * w; i += THREADS) {
        const int r = i / w, j = col0 + (i - r * w);
        out[r * a.L.D + j] = norm_value(base[i], meanv[j], denomv[j], a.clip_obs);
    }
}

__global__ __launch_bounds__(THREADS) void k_norm_apply(Args a) {
    extern __shared__ double lds[];
    const Layout &L = a.L;
    const int64_t c = blockIdx.x, r0 = c * CHUNK;
    const int rows = (int)(L.E - r0 < CHUNK ? L.E - r0 : CHUNK);
    const int tid = threadIdx.x, lane = tid & (WAVE - 1);
    double *meanv = lds, *denomv = lds + L.D;
    __shared__ int wfin[2];
    if (tid < L.D) {
        meanv[tid] = a.stats[tid];
        denomv[tid] = sqrt(a.stats[L.D + tid] + a.eps);
    }
    unsigned long long m = 0;
    if (a.step && tid < CHUNK) {                  // wavefront-uniform: the chunk's envs are wavefronts 0 and 1
        const bool d = tid < rows && a.done[r0 + tid] != 0;
        m = __ballot(d);
        if (lane == 0) wfin[tid >> 6] = __popcll(m);
    }
    __syncthreads();
    if (tid < rows) {
        if (a.step) {
            const int64_t rank = a.prefix[c] + (tid >= WAVE ? wfin[0] : 0) + __popcll(m & ((1ull << lane) - 1ull));
            apply_env(a, r0 + tid, rank, sqrt(a.stats[2 * L.D + 1] + a.eps));
        } else if (a.zero_ret) {
            a.ret[r0 + tid] = 0.0f;
        }
    }
    norm_part(a, meanv, denomv, 0, a.obs, L.obs, r0, rows);
    if (L.goal > 0) {
        norm_part(a, meanv, denomv, L.obs, a.ag, L.goal, r0, rows);
        norm_part(a, meanv, denomv, L.obs + L.goal, a.dg, L.goal, r0, rows);
    }
}

static size_t partial_lds(const Args &a) {
    const int nc = a.L.D + (a.step ? 1 : 0);
    return a.update ? sizeof(double) * (NSEG * nc + nc) + sizeof(float) * CHUNK * nc : 0;
}

int launch_norm(const Args &a, void *stream) {
    const hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)a.L.chunks), block(THREADS);
    if (a.update || a.step) {
        k_norm_partial<<<grid, block, partial_lds(a), s>>>(a);
        k_norm_merge<<<dim3(1), block, 0, s>>>(a);
    }
    k_norm_apply<<<grid, block, sizeof(double) * 2 * a.L.D, s>>>(a);
    return (int)hipGetLastError();
}

}  // namespace xnorm
