// xarm_k_ppo.hip - the kernels of the device-resident PPO update.  Core: xarm_ppo_core.h; the tile: xarm_grad_tile.h.
// Built with -ffp-contract=off (build.py UNIT_FLAGS): every float32 operation is the one the host build performs.
//
// One update of S = n_epochs M optimiser steps is 4 + 3 S launches on the caller's stream:
//   k_policy_act    (xarm_k_policy.hip, deterministic) on last_obs: v_T
//   k_policy_act    on the T E rows of obs: mean and value of every row under the weights at call start
//   k_ppo_gae       one thread per row: old_logp of the stored action (skipped when the caller hands one in); the threads of the first
//                   E rows: the GAE recursion of their env from k = T - 1 down
//   k_ppo_advstats  one workgroup per optimiser step: n, mu, sigma of that step's rows (perm is known and adv does not change during
//                   the call), float64, a thread's entries in position order and the threads by a fixed tree
//   per step s:
//   k_ppo_grad      grid (groups, 2 towers), 256 threads.  A workgroup walks the 64-position tiles g, g + groups, ... of the step's
//                   span of perm; the tile's rows are gathered through perm at the tile load (an entry outside [0, N) is an empty slot),
//                   h1 / h2 and the tower's outputs - mean or value under the weights of THIS step - come from the tile itself, the head
//                   (ratio, clip, deltas) runs on them and the backward is the shared tile's.  Partials and scalars per workgroup.
//   k_ppo_reduce    one thread per parameter: the slices added in float64 in group order, / n_use, the entropy term, the float32
//                   gradient; a block's sum of squares to normpart; block 0's thread 0 writes the step's stats row, advances `step`
//                   (every read of the old value - the previous step's k_ppo_apply - lies behind a kernel boundary) and Adam's scalars
//   k_ppo_apply     one thread per parameter: norm from normpart in block order, the clip, Adam
// With target_kl on (xarm_ppo_core.h, options) k_ppo_gae's first thread clears the stop flag, k_ppo_reduce's stats thread sets it, and
// a stopped step's three launches return after one uniform read of it (its reduce writes the stopped stats row first).
// No atomics anywhere: the same inputs and perm give the same bits.
#include <hip/hip_runtime.h>
#include "xarm_ppo_core.h"
#include "xarm_grad_tile.h"

namespace xppo {

using xa2c::LS;
using xa2c::THREADS;

__global__ __launch_bounds__(256) void k_ppo_gae(Dev d) {
    const xa2c::Shape &a = d.s.a;
    const int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (n >= a.N) return;
    if (n == 0 && d.h.kl_limit > 0.0) d.stop[0] = 0;
    if (d.old_logp == nullptr) {
        float nodls[MAX_ACT];
        d.oldlp[n] = xa2c::pi_row<false>(a.A, d.mean + n * a.A, 1, d.action + n * a.A, d.w[12], 0.0f, nullptr, 0, nodls);
    }
    if (n >= a.E) return;
    float nv = d.boot[n], na = 0.0f;
    for (int k = a.T - 1; k >= 0; k--) {
        const int64_t i = (int64_t)k * a.E + n;
        const float v = d.value[i];
        na = gae_step(d.h.gamma, d.h.gl, d.done[i], d.reward[i], v, nv, na);
        nv = v;
        const float rt = na + v;
        d.adv[i] = na;
        d.ret[i] = rt;
        if (d.out_adv != nullptr) d.out_adv[i] = na;
        if (d.out_returns != nullptr) d.out_returns[i] = rt;
    }
}

__global__ __launch_bounds__(RED) void k_ppo_advstats(Dev d) {
    __shared__ double red[RED];
    const int tid = threadIdx.x;
    const int64_t N = d.s.a.N;
    int64_t first, count;
    step_span(d.s, blockIdx.x, first, count);
    double n = 0.0, sa = 0.0, sv = 0.0;
    for (int64_t i = tid; i < count; i += RED) {
        const int64_t r = row_of(d.perm[first + i], N);
        if (r < 0) continue;
        const double u = d.use != nullptr ? (double)d.use[r] : 1.0;
        n += u;
        sa += (double)d.adv[r] * u;
    }
    n = xa2c::block_sum(red, n);
    sa = xa2c::block_sum(red, sa);
    const double mu = n > 0.0 ? sa / n : 0.0;
    for (int64_t i = tid; i < count; i += RED) {
        const int64_t r = row_of(d.perm[first + i], N);
        if (r < 0) continue;
        const double u = d.use != nullptr ? (double)d.use[r] : 1.0, dd = (double)d.adv[r] - mu;
        sv += dd * dd * u;
    }
    sv = xa2c::block_sum(red, sv);
    if (tid == 0) finish_stats(d.musig + (int64_t)blockIdx.x * NMS, n, mu, sv, d.h.normalize);
}

// PPO's head: mean / value of the slot come from this tile's h2 under the step's weights (D3 holds them when deltas() is called)
struct PpoHead {
    static constexpr bool FROM_H2 = true;
    const Dev &d;
    bool is_pi;
    const int *Rt;                      // LDS: the batch row of each tile slot, -1 for an empty one
    const double *ms;                   // the step's mu, sigma, normalise, n
    float (&dls)[MAX_ACT];
    double (&sums)[NSCAL];              // the group's record: 0 surrogate, 1 value loss, 2 use, 19 kl, 20 clipped (3..18: dls, at the end)
    __device__ __forceinline__ int64_t row(int rr) const { return Rt[rr]; }
    __device__ __forceinline__ void deltas(int r, float *D3) {
        const int64_t n = Rt[r];
        const int A = d.s.a.A;
        if (n < 0) {
#pragma unroll
            for (int c = 0; c < MAX_ACT; c++) D3[c * LS] = 0.0f;
            return;
        }
        const float u = d.use != nullptr ? d.use[n] : 1.0f;
        if (is_pi) {
            float nodls[MAX_ACT];
            const float *act = d.action + n * A;
            const float lp = xa2c::pi_row<false>(A, D3, LS, act, d.w[12], 0.0f, nullptr, 0, nodls);
            const float olp = d.old_logp != nullptr ? d.old_logp[n] : d.oldlp[n];
            const RowTerms t = surrogate(d.h, norm_adv(d.adv[n], ms), lp, olp, u);
            xa2c::pi_row<true>(A, D3, LS, act, d.w[12], t.q, D3, LS, dls);
            sums[0] += (double)t.surr; sums[19] += (double)t.kl; sums[20] += (double)t.clipped;
            sums[2] += (double)u;
        } else {
            const float v = D3[0], rt = d.ret[n];
            const ValueTerms vt = value_terms(d.h, v, d.h.vclip > 0.0f ? d.value[n] : v, rt, u);
            D3[0] = vt.dvalue;
            sums[1] += (double)vt.loss;
            sums[2] += (double)u;
        }
    }
};

// JW: columns of dW1 per thread; the tile holds 16 JW >= D columns
template <int JW> __global__ __launch_bounds__(THREADS) void k_ppo_grad(Dev d, int step) {
    if (stopped_before(d.h, d.stop, step)) return;
    XARM_TILE_LDS(JW);
    __shared__ int Rt[ROWS];
    const int t = threadIdx.x;
    const bool is_pi = blockIdx.y == 0;
    const Tower T = is_pi ? d.pi : d.vf;
    const xa2c::Shape &a = d.s.a;
    const int D = a.D, G = a.G, g = blockIdx.x, nout = is_pi ? a.A : 1;
    int64_t first, count;
    step_span(d.s, step, first, count);
    const int64_t tiles = (count + ROWS - 1) / ROWS;

    xa2c::TileGrad<JW> acc;
    acc.zero();
    float dls[MAX_ACT];
#pragma unroll
    for (int c = 0; c < MAX_ACT; c++) dls[c] = 0.0f;
    static_assert(3 + MAX_ACT <= 19 && 21 <= NSCAL, "a record holds the scalars");
    double sums[NSCAL] = {};
    PpoHead head = {d, is_pi, Rt, d.musig + (int64_t)step * NMS, dls, sums};

    for (int64_t tile = g; tile < tiles; tile += G) {
        if (t < ROWS) {     // the gather: the tile's slots through perm (the previous tile ended on a barrier)
            const int64_t pos = tile * ROWS + t;
            Rt[t] = pos < count ? (int)row_of(d.perm[first + pos], a.N) : -1;
        }
        __syncthreads();
        xa2c::grad_tile<JW>(T, D, nout, d.obs, L, head, acc);
    }
    acc.store(d.partial + ((int64_t)blockIdx.y * G + g) * a.pstride, D, nout);

    // the scalars (a workgroup without a tile stores zeros)
#pragma unroll
    for (int c = 0; c < MAX_ACT; c++) sums[3 + c] = (double)dls[c];
    xa2c::store_scalars<NSCAL>(H1t, sums, d.scal + ((int64_t)blockIdx.y * G + g) * NSCAL);
}

__global__ __launch_bounds__(RED) void k_ppo_reduce(Dev d, int step) {
    if (stopped_before(d.h, d.stop, step)) {
        if (blockIdx.x == 0 && threadIdx.x == 0 && d.out_stats != nullptr) stopped_row(d.out_stats + (int64_t)step * 8);
        return;
    }
    __shared__ double red[RED];
    const xa2c::Shape &a = d.s.a;
    const int G = a.G;
    const double n_use = xa2c::reduce_block(a, d.partial, d.scal, NSCAL, d.h.ent_coef, d.grad, step == 0 ? d.out_grad : nullptr, red, d.normpart);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        double surr = 0.0, vloss = 0.0, kl = 0.0, clipped = 0.0;
        if (d.out_stats != nullptr || d.h.kl_limit > 0.0)
            for (int g = 0; g < G; g++) {
                const double *pi = d.scal + (int64_t)g * NSCAL, *vf = d.scal + ((int64_t)G + g) * NSCAL;
                surr += pi[0]; kl += pi[19]; clipped += pi[20]; vloss += vf[1];
            }
        const bool trips = kl_trips(d.h, (float)(kl / n_use));
        if (trips) {
            d.stop[0] = step + 1;
        } else {
            const int64_t t = d.step[0] + 1;
            d.step[0] = t;
            xopt::adam_scalars(d.h.adam, t, d.adam);
        }
        if (d.out_stats != nullptr) {
            const double ent = xopt::gaussian_entropy(d.w[12], a.A);
            float *o = d.out_stats + (int64_t)step * 8;
            o[0] = (float)(-surr / n_use); o[1] = (float)(vloss / n_use); o[2] = (float)ent; o[4] = (float)n_use;
            o[5] = (float)(kl / n_use); o[6] = (float)(clipped / n_use); o[7] = trips ? 1.0f : 0.0f;
            if (trips) o[3] = 0.0f;
        }
    }
}

__global__ __launch_bounds__(RED) void k_ppo_apply(Dev d, int step) {
    if (stopped_at(d.h, d.stop)) return;
    const xa2c::Shape &a = d.s.a;
    const int64_t p = (int64_t)blockIdx.x * RED + threadIdx.x;
    float norm;
    const float coef = xa2c::norm_and_clip(a, d.normpart, d.h.max_norm, norm);
    if (p == 0 && d.out_stats != nullptr) d.out_stats[(int64_t)step * 8 + 3] = norm;
    if (p >= a.P) return;
    const int i = xopt::tensor_at<NTENS>(a.off, 0, p);
    const int64_t e = p - a.off[i];
    const float sc[2] = {d.adam[0], d.adam[1]};
    float m = d.m[i][e], v = d.v[i][e], w = d.w[i][e];
    xopt::adam(d.h.adam, sc, d.grad[p] * coef, m, v, w);
    d.m[i][e] = m;
    d.v[i][e] = v;
    d.w[i][e] = w;
}

int launch_update(const Dev &d, void *stream) {
    const hipStream_t s = (hipStream_t)stream;
    const xa2c::Shape &sh = d.s.a;
    xpol::Args a = {};
    a.E = sh.E; a.obs = sh.D; a.D = sh.D; a.A = sh.A; a.deterministic = 1; a.pi = d.pi; a.vf = d.vf; a.log_std = d.w[12];
    a.x0 = d.last_obs; a.action = d.mean; a.env_action = d.env; a.value = d.boot;
    int le = xpol::launch_policy(a, nullptr, stream);
    if (le != 0) return le;
    a.E = sh.N; a.x0 = d.obs; a.value = d.value;
    le = xpol::launch_policy(a, nullptr, stream);
    if (le != 0) return le;
    k_ppo_gae<<<dim3((unsigned)((sh.N + 255) / 256)), dim3(256), 0, s>>>(d);
    k_ppo_advstats<<<dim3((unsigned)d.s.S), dim3(RED), 0, s>>>(d);
    const dim3 grid((unsigned)sh.G, 2), rgrid((unsigned)sh.NB), rblock(RED);
    for (int st = 0; st < (int)d.s.S; st++) {
        XARM_TILE_LAUNCH(sh.D, k_ppo_grad, grid, s, d, st);
        k_ppo_reduce<<<rgrid, rblock, 0, s>>>(d, st);
        k_ppo_apply<<<rgrid, rblock, 0, s>>>(d, st);
    }
    return (int)hipGetLastError();
}

}  // namespace xppo
