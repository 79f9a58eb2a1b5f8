// xarm_k_a2c.hip - the kernels of the device-resident A2C update.  Core: xarm_a2c_core.h.
// Built with -ffp-contract=off (build.py UNIT_FLAGS): every float32 operation is the one the host build performs.
//
// One update is six launches on the caller's stream:
//   k_policy_act    (xarm_k_policy.hip, deterministic) on last_obs: the bootstrap value
//   k_policy_act    on the T E rows of obs: mean and value of every row - the policy kernel's own bits
//   k_a2c_returns   one thread per env: the return recursion from the bootstrap value down
//   k_a2c_grad      grid (groups, 2 towers), 256 threads.  A workgroup walks the 64-row tiles g, g + groups, ... of ONE tower.  The tile
//                   body is xa2c::grad_tile (xarm_grad_tile.h, shared with the PPO update); A2CHead below supplies rows and deltas.  Per
//                   tile, in LDS and transposed ([unit][row], stride 65: a lane per row and a lane per unit both read without bank
//                   conflicts): the rows, h1 and h2 from the policy's chains (lane = row, wavefront w = units 16 w .. 16 w + 15, so
//                   the weights are wavefront-uniform loads), the output deltas, then d2 and d1 in place over h2 and h1 once the
//                   outer products that need h2 / h1 are taken.  The gradient lives in registers across the tiles: thread
//                   (ib, jb) = (t & 15, t >> 4) owns the entries (ib + 16 a, jb + 16 b) of dW2 and dW1, thread (t & 63, t >> 6)
//                   the entries of dW3.  At the end the workgroup stores its float32 sums to its own slice of the workspace,
//                   and the policy tower's workgroups their loss / n_use / log_std sums (float64, lanes added in lane order).
//   k_a2c_reduce    one thread per parameter: the slices added in float64 in group order, / n_use, the entropy term, the float32
//                   gradient; a block's sum of squares (a fixed tree) to normpart; block 0 writes the losses
//   k_a2c_apply     one thread per parameter: norm from normpart in block order, the clip, RMSprop
// No atomics anywhere: the same inputs give the same bits.
#include <hip/hip_runtime.h>
#include "xarm_grad_tile.h"

namespace xa2c {

__global__ __launch_bounds__(256) void k_a2c_returns(Dev d) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= d.s.E) return;
    float r = d.boot[e];
    for (int k = d.s.T - 1; k >= 0; k--) {
        const int64_t n = (int64_t)k * d.s.E + e;
        r = return_step(d.h.gamma, d.done[n], d.reward[n], r);
        d.ret[n] = r;
        if (d.out_returns != nullptr) d.out_returns[n] = r;
    }
}

// A2C's head: the deltas come from the call-start mean / value / returns, so they are written with the tile's load
struct A2CHead {
    static constexpr bool FROM_H2 = false;
    const Dev &d;
    bool is_pi;
    int64_t r0;
    float (&dls)[MAX_ACT];
    double &ploss, &vloss, &nuse;
    __device__ __forceinline__ int64_t row(int rr) const { const int64_t n = r0 + rr; return n < d.s.N ? n : -1; }
    __device__ __forceinline__ void deltas(int r, float *D3) {
        const int64_t n = r0 + r;
        if (n < d.s.N) {
            const float u = d.use != nullptr ? d.use[n] : 1.0f, v = d.value[n], rt = d.ret[n];
            if (is_pi) {
                const float adv = rt - v;
                const float lp = pi_deltas(d.s.A, d.mean + n * d.s.A, d.action + n * d.s.A, d.w[12], adv, u, D3, LS, dls);
                ploss += (double)(adv * lp * u);
                vloss += (double)((rt - v) * (rt - v) * u);
                nuse += (double)u;
            } else {
                D3[0] = value_delta(d.h.vf2, v, rt, u);
            }
        }
    }
};

// JW: columns of dW1 per thread; the tile holds 16 JW >= D columns
template <int JW> __global__ __launch_bounds__(THREADS) void k_a2c_grad(Dev d) {
    XARM_TILE_LDS(JW);
    const bool is_pi = blockIdx.y == 0;
    const Tower T = is_pi ? d.pi : d.vf;
    const int D = d.s.D, A = d.s.A, G = d.s.G, g = blockIdx.x, nout = is_pi ? A : 1;

    TileGrad<JW> acc;
    acc.zero();
    float dls[MAX_ACT];
#pragma unroll
    for (int c = 0; c < MAX_ACT; c++) dls[c] = 0.0f;
    double ploss = 0.0, vloss = 0.0, nuse = 0.0;
    A2CHead head = {d, is_pi, 0, dls, ploss, vloss, nuse};

    for (int64_t tile = g; tile < d.s.tiles; tile += G) {
        head.r0 = tile * ROWS;
        grad_tile<JW>(T, D, nout, d.obs, L, head, acc);
    }
    acc.store(d.partial + ((int64_t)blockIdx.y * G + g) * d.s.pstride, D, nout);

    if (is_pi) {    // the scalars: loss, value loss, use, the log_std terms
        static_assert(3 + MAX_ACT <= NSCAL, "a record holds the scalars");
        double sums[NSCAL] = {ploss, vloss, nuse};
#pragma unroll
        for (int c = 0; c < MAX_ACT; c++) sums[3 + c] = (double)dls[c];
        store_scalars<NSCAL>(H1t, sums, d.scal + (int64_t)g * NSCAL);
    }
}

__global__ __launch_bounds__(RED) void k_a2c_reduce(Dev d) {
    __shared__ double red[RED];
    const int G = d.s.G;
    const double n_use = reduce_block(d.s, d.partial, d.scal, NSCAL, d.h.ent_coef, d.grad, d.out_grad, red, d.normpart);
    if (blockIdx.x == 0 && threadIdx.x == 0 && d.out_stats != nullptr) {
        double ploss = 0.0, vloss = 0.0;
        for (int g = 0; g < G; g++) { ploss += d.scal[(int64_t)g * NSCAL]; vloss += d.scal[(int64_t)g * NSCAL + 1]; }
        const double ent = xopt::gaussian_entropy(d.w[12], d.s.A);
        d.out_stats[0] = (float)(-ploss / n_use); d.out_stats[1] = (float)(vloss / n_use); d.out_stats[2] = (float)ent;
        d.out_stats[4] = (float)n_use; d.out_stats[5] = d.out_stats[6] = d.out_stats[7] = 0.0f;
    }
}

__global__ __launch_bounds__(RED) void k_a2c_apply(Dev d) {
    const int64_t p = (int64_t)blockIdx.x * RED + threadIdx.x;
    float norm;
    const float coef = norm_and_clip(d.s, d.normpart, d.h.max_norm, norm);
    if (p == 0 && d.out_stats != nullptr) d.out_stats[3] = norm;
    if (p >= d.s.P) return;
    const int i = xopt::tensor_at<NTENS>(d.s.off, 0, p);
    const int64_t e = p - d.s.off[i];
    float sq = d.sq[i][e], w = d.w[i][e];
    xopt::rmsprop(d.h.rms, d.grad[p] * coef, sq, w);
    d.sq[i][e] = sq;
    d.w[i][e] = w;
}

int launch_update(const Dev &d, void *stream) {
    const hipStream_t s = (hipStream_t)stream;
    xpol::Args a = {};
    a.E = d.s.E; a.obs = d.s.D; a.D = d.s.D; a.A = d.s.A; a.deterministic = 1; a.pi = d.pi; a.vf = d.vf; a.log_std = d.w[12];
    a.x0 = d.last_obs; a.action = d.mean; a.env_action = d.env; a.value = d.boot;
    int le = xpol::launch_policy(a, nullptr, stream);
    if (le != 0) return le;
    a.E = d.s.N; a.x0 = d.obs; a.value = d.value;
    le = xpol::launch_policy(a, nullptr, stream);
    if (le != 0) return le;
    k_a2c_returns<<<dim3((unsigned)((d.s.E + 255) / 256)), dim3(256), 0, s>>>(d);
    const dim3 grid((unsigned)d.s.G, 2);
    XARM_TILE_LAUNCH(d.s.D, k_a2c_grad, grid, s, d);
    k_a2c_reduce<<<dim3((unsigned)d.s.NB), dim3(RED), 0, s>>>(d);
    k_a2c_apply<<<dim3((unsigned)d.s.NB), dim3(RED), 0, s>>>(d);
    return (int)hipGetLastError();
}

}  // namespace xa2c
