// xarm_k_sac.hip - the kernels of the device-resident SAC update.  Core: xarm_sac_core.h; the tile: xarm_grad_tile.h.
// Built with -ffp-contract=off (build.py UNIT_FLAGS): every float32 operation is the one the host build performs.
//
// One step is six launches on the caller's stream:
//   k_sac_rows     grid (groups), 256 threads.  A workgroup walks the 64-row tiles g, g + groups, ...; per tile four forwards of the
//                  shared tile (lane = row, wavefront w = units 16 w .. 16 w + 15): the actor on next_obs, both target critics on
//                  next_obs | a', the actor on obs.  Wavefront 0 (lane = row) draws or reads z, finishes the squashed Gaussian and writes
//                  y, logp_pi, z_pi and the rows xq = obs | action and xpi = obs | a_pi; its lanes keep the float64 sums of use,
//                  logp_pi use and (logp_pi + target_entropy) use, added in lane order at the end.  Workgroup 0 also writes Adam's two
//                  scalars of the step and alpha.
//   k_sac_qgrad    grid (groups, 2 critics): the shared backward tile on xq with delta (q - y) use at the output
//   k_sac_qapply   one thread per critic parameter: the slices added in float64 in group order, / n_use, Adam, and the Polyak step of
//                  the matching target entry with the stepped value (nothing changes the critics again inside the step)
//   k_sac_dqda     grid (groups, 2 critics): the tile's forward and input gradient (no outer products) of the stepped critics over xpi:
//                  q_i and dq_i / da per row
//   k_sac_pgrad    grid (groups): the shared backward tile on obs, 2 A outputs; the head recomputes a from the tile's own mean / log_std
//                  and the step's z, picks the critic with the smaller q and writes the deltas of xsac::actor_deltas
//   k_sac_papply   one thread per actor parameter and one for log_alpha: reduce, Adam; the log_alpha thread also writes the stats and
//                  advances `step` - every other read of `step` lies in k_sac_rows, behind kernel boundaries
// xarm_sac_act is k_sac_act (one workgroup per 64-row tile: the actor's forward, the head) and, behind a stochastic call, k_sac_tick.
// No atomics anywhere: the same inputs give the same bits.
#include <hip/hip_runtime.h>
#include "xarm_sac_core.h"
#include "xarm_grad_tile.h"

namespace xsac {

using xa2c::LS;
using xa2c::THREADS;
using xa2c::store_scalars;
using xpol::MAX_ACT;

// rows r0 .. r0 + 63 of x [B, W] to Xt's columns 0 .. W - 1, zeros in the slots past B and in the columns W .. 16 JW - 1
template <int JW> __device__ __forceinline__ void load_rows(float *Xt, const float *x, int W, int64_t r0, int64_t B) {
    for (int idx = threadIdx.x; idx < 16 * JW * ROWS; idx += THREADS) {
        const int rr = idx / (16 * JW), j = idx - rr * (16 * JW);
        const int64_t n = r0 + rr;
        Xt[j * LS + rr] = (n < B && j < W) ? x[n * W + j] : 0.0f;
    }
}

// the z of row n: the supplied tensor, or Philox (stream 0: z_pi, 1: z_next)
__device__ __forceinline__ void row_noise(const Dev &d, const float *given, int64_t n, int64_t counter, int stream, float (&z)[MAX_A]) {
    const int A = d.s.A;
#pragma unroll
    for (int b = 0; b < MAX_A / 4; b++) {
        float q[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        if (given == nullptr && 4 * b < A) noise4(d.h.seed, n, counter, stream, b, q);
#pragma unroll
        for (int m = 0; m < 4; m++) {
            const int c = 4 * b + m;
            z[c] = 0.0f;
            if (c < A) z[c] = given != nullptr ? given[n * A + c] : q[m];
        }
    }
}

__device__ __forceinline__ double n_use_of(const Dev &d) {
    double nuse = 0.0;
    for (int g = 0; g < d.s.G; g++) nuse += d.scal_rows[(int64_t)g * RS];
    return xopt::n_use(nuse);
}

// ------------------------------------------------------------------------------------------------------------------------ rows
template <int JW> __global__ __launch_bounds__(THREADS) void k_sac_rows(Dev d) {
    XARM_TILE_LDS(JW);
    const int t = threadIdx.x, r = t & 63, wv = __builtin_amdgcn_readfirstlane(t >> 6);
    const int D = d.s.D, A = d.s.A, Dq = d.s.Dq, G = d.s.G, g = blockIdx.x;
    const int64_t B = d.s.B, t0 = d.step[0];
    const float alpha = alpha_of(d.h, d.w[18]);
    if (g == 0 && t == 0) {
        xopt::adam_scalars(d.h.adam, t0 + 1, d.hdr);
        d.hdr[2] = alpha;
        d.hdr[3] = 0.0f;
    }
    double sums[RS] = {0.0, 0.0, 0.0, 0.0};
    for (int64_t tile = g; tile < d.s.tiles; tile += G) {
        const int64_t r0 = tile * ROWS, n = r0 + r;
        const bool live = n < B;
        // the actor on next_obs; a' goes behind the row
        load_rows<JW>(Xt, d.next_obs, D, r0, B);
        __syncthreads();
        xa2c::tile_forward<true>(d.actor, D, 2 * A, L, r, wv);
        float lpn = 0.0f;
        if (wv == 0) {
            float z[MAX_A], a[MAX_A];
            row_noise(d, d.noise_next, live ? n : 0, t0, 1, z);
            lpn = actor_head(A, D3t + r, LS, z, false, a);
#pragma unroll
            for (int c = 0; c < MAX_A; c++)
                if (c < A) Xt[(D + c) * LS + r] = live ? a[c] : 0.0f;
        }
        __syncthreads();
        xa2c::tile_forward<true>(d.q1t, Dq, 1, L, r, wv);
        float qa = 0.0f;
        if (wv == 0) qa = D3t[r];
        xa2c::tile_forward<true>(d.q2t, Dq, 1, L, r, wv);
        if (wv == 0 && live) {
            const float y = target_row(d.h.gamma, alpha, d.reward[n], d.done[n], qa, D3t[r], lpn);
            d.y[n] = y;
            if (d.out_target != nullptr) d.out_target[n] = y;
        }
        __syncthreads();
        // the actor on obs; the load also writes xq = obs | action and the obs part of xpi
        for (int idx = t; idx < 16 * JW * ROWS; idx += THREADS) {
            const int rr = idx / (16 * JW), j = idx - rr * (16 * JW);
            const int64_t nn = r0 + rr;
            float x = 0.0f;
            if (nn < B && j < Dq) {
                x = j < D ? d.obs[nn * D + j] : d.action[nn * A + (j - D)];
                d.xq[nn * Dq + j] = x;
                if (j < D) d.xpi[nn * Dq + j] = x;
            }
            Xt[j * LS + rr] = j < D ? x : 0.0f;
        }
        __syncthreads();
        xa2c::tile_forward<true>(d.actor, D, 2 * A, L, r, wv);
        if (wv == 0 && live) {
            float z[MAX_A], a[MAX_A];
            row_noise(d, d.noise_pi, n, t0, 0, z);
            const float lp = actor_head(A, D3t + r, LS, z, false, a);
            d.logp[n] = lp;
#pragma unroll
            for (int c = 0; c < MAX_A; c++)
                if (c < A) { d.xpi[n * Dq + D + c] = a[c]; d.z[n * A + c] = z[c]; }
            const float u = d.use != nullptr ? d.use[n] : 1.0f;
            sums[0] += (double)u;
            sums[1] += (double)(lp * u);
            sums[2] += (double)((lp + d.h.target_entropy) * u);
        }
        __syncthreads();
    }
    store_scalars<RS>(H1t, sums, d.scal_rows + (int64_t)g * RS);
}

// ------------------------------------------------------------------------------------------------------------------- the critics
struct CriticHead {
    static constexpr bool FROM_H2 = true;
    const Dev &d;
    int64_t r0;
    double &loss;
    __device__ __forceinline__ int64_t row(int rr) const { const int64_t n = r0 + rr; return n < d.s.B ? n : -1; }
    __device__ __forceinline__ void deltas(int r, float *D3) {
        const int64_t n = r0 + r;
        if (n >= d.s.B) { D3[0] = 0.0f; return; }
        const float u = d.use != nullptr ? d.use[n] : 1.0f;
        const float diff = D3[0] - d.y[n];
        D3[0] = diff * u;
        loss += (double)(diff * diff * u);
    }
};

template <int JW> __global__ __launch_bounds__(THREADS) void k_sac_qgrad(Dev d) {
    XARM_TILE_LDS(JW);
    const int G = d.s.G, g = blockIdx.x;
    const Tower T = blockIdx.y == 0 ? d.q1 : d.q2;
    xa2c::TileGrad<JW> acc;
    acc.zero();
    double sums[QS] = {0.0, 0.0};
    CriticHead head = {d, 0, sums[0]};
    for (int64_t tile = g; tile < d.s.tiles; tile += G) {
        head.r0 = tile * ROWS;
        xa2c::grad_tile<JW>(T, d.s.Dq, 1, d.xq, L, head, acc);
    }
    acc.store(d.partial + ((int64_t)blockIdx.y * G + g) * d.s.pstride, d.s.Dq, 1);
    store_scalars<QS>(H1t, sums, d.scal_q + ((int64_t)blockIdx.y * G + g) * QS);
}

// one thread per parameter of q1 | q2
__global__ __launch_bounds__(RED) void k_sac_qapply(Dev d) {
    const Shape &s = d.s;
    const int64_t p = (int64_t)blockIdx.x * RED + threadIdx.x;
    if (p >= 2 * s.Pq) return;
    const double n_use = n_use_of(d);
    const int tower = p >= s.Pq ? 1 : 0;
    const int64_t local = p - tower * s.Pq;
    const float gf = (float)(xopt::slice_sum(d.partial + (int64_t)tower * s.G * s.pstride + local, s.G, s.pstride) / n_use);
    if (d.out_grad != nullptr) d.out_grad[s.Pa + p] = gf;
    const int i = xopt::tensor_at<6>(s.off, 6 + 6 * tower, s.Pa + p);
    const int64_t e = s.Pa + p - s.off[i];
    const float sc[2] = {d.hdr[0], d.hdr[1]};
    float m = d.m[i][e], v = d.v[i][e], w = d.w[i][e];
    xopt::adam(d.h.adam, sc, gf, m, v, w);
    d.m[i][e] = m;
    d.v[i][e] = v;
    d.w[i][e] = w;
    d.tq[i - 6][e] = polyak(d.h, d.tq[i - 6][e], w);
}

// the stepped critics at obs | a_pi: q and dq / da
struct ActionGradHead {
    static constexpr bool FROM_H2 = true, INPUT_GRAD = true, WEIGHT_GRAD = false;
    const Dev &d;
    int tower;
    int64_t r0;
    __device__ __forceinline__ int64_t row(int rr) const { const int64_t n = r0 + rr; return n < d.s.B ? n : -1; }
    __device__ __forceinline__ int col0() const { return d.s.D; }
    __device__ __forceinline__ int ncol() const { return d.s.A; }
    __device__ __forceinline__ void deltas(int r, float *D3) {
        const int64_t n = r0 + r;
        if (n >= d.s.B) { D3[0] = 0.0f; return; }
        d.qpi[tower * d.s.B + n] = D3[0];
        D3[0] = 1.0f;
    }
    __device__ __forceinline__ void input_grad(int r, int c, float dx) {
        const int64_t n = r0 + r;
        if (n >= d.s.B) return;
        const int64_t at = ((int64_t)tower * d.s.B + n) * d.s.A + c;
        d.dqda[at] = dx;
        if (d.out_dqda != nullptr) d.out_dqda[at] = dx;
    }
};

template <int JW> __global__ __launch_bounds__(THREADS) void k_sac_dqda(Dev d) {
    XARM_TILE_LDS(JW);
    const int G = d.s.G, g = blockIdx.x;
    const Tower T = blockIdx.y == 0 ? d.q1 : d.q2;
    xa2c::TileGrad<JW> unused;
    ActionGradHead head = {d, (int)blockIdx.y, 0};
    for (int64_t tile = g; tile < d.s.tiles; tile += G) {
        head.r0 = tile * ROWS;
        xa2c::grad_tile<JW>(T, d.s.Dq, 1, d.xpi, L, head, unused);
    }
}

// --------------------------------------------------------------------------------------------------------------------- the actor
struct ActorHead {
    static constexpr bool FROM_H2 = true;
    const Dev &d;
    int64_t r0;
    float alpha;
    double (&sums)[PS];
    __device__ __forceinline__ int64_t row(int rr) const { const int64_t n = r0 + rr; return n < d.s.B ? n : -1; }
    __device__ __forceinline__ void deltas(int r, float *D3) {
        const int64_t n = r0 + r, B = d.s.B;
        const int A = d.s.A;
        if (n >= B) {
#pragma unroll
            for (int c = 0; c < MAX_ACT; c++) D3[c * LS] = 0.0f;
            return;
        }
        const float u = d.use != nullptr ? d.use[n] : 1.0f;
        const float qa = d.qpi[n], qb = d.qpi[B + n];
        const bool second = qb < qa;
        const float qm = second ? qb : qa;
        actor_deltas(A, D3, LS, d.z + n * A, alpha, d.dqda + ((second ? B : 0) + n) * A, u);
        const float ent = alpha * d.logp[n];
        sums[0] += (double)((ent - qm) * u);
        sums[1] += (double)(qm * u);
    }
};

template <int JW> __global__ __launch_bounds__(THREADS) void k_sac_pgrad(Dev d) {
    XARM_TILE_LDS(JW);
    const int G = d.s.G, g = blockIdx.x;
    xa2c::TileGrad<JW> acc;
    acc.zero();
    double sums[PS] = {0.0, 0.0};
    ActorHead head = {d, 0, d.hdr[2], sums};
    for (int64_t tile = g; tile < d.s.tiles; tile += G) {
        head.r0 = tile * ROWS;
        xa2c::grad_tile<JW>(d.actor, d.s.D, 2 * d.s.A, d.obs, L, head, acc);
    }
    acc.store(d.partial + (int64_t)g * d.s.pstride, d.s.D, 2 * d.s.A);
    store_scalars<PS>(H1t, sums, d.scal_p + (int64_t)g * PS);
}

// one thread per actor parameter; thread Pa: log_alpha, the stats and the step count
__global__ __launch_bounds__(RED) void k_sac_papply(Dev d) {
    const Shape &s = d.s;
    const int64_t p = (int64_t)blockIdx.x * RED + threadIdx.x;
    if (p > s.Pa) return;
    const int G = s.G;
    const double n_use = n_use_of(d);
    const float sc[2] = {d.hdr[0], d.hdr[1]};
    if (p < s.Pa) {
        const float gf = (float)(xopt::slice_sum(d.partial + p, G, s.pstride) / n_use);
        if (d.out_grad != nullptr) d.out_grad[p] = gf;
        const int i = xopt::tensor_at<6>(s.off, 0, p);
        const int64_t e = p - s.off[i];
        float m = d.m[i][e], v = d.v[i][e], w = d.w[i][e];
        xopt::adam(d.h.adam, sc, gf, m, v, w);
        d.m[i][e] = m;
        d.v[i][e] = v;
        d.w[i][e] = w;
        return;
    }
    double slp = 0.0, sent = 0.0, closs = 0.0, aloss = 0.0, sq = 0.0;
    for (int g = 0; g < G; g++) {
        slp += d.scal_rows[(int64_t)g * RS + 1];
        sent += d.scal_rows[(int64_t)g * RS + 2];
        closs += d.scal_q[(int64_t)g * QS] + d.scal_q[((int64_t)G + g) * QS];
        aloss += d.scal_p[(int64_t)g * PS];
        sq += d.scal_p[(int64_t)g * PS + 1];
    }
    finish(d.h, sc, d.hdr[2], n_use, sent, closs, aloss, slp, sq, d.w[18], d.m[18], d.v[18],
           d.out_grad != nullptr ? d.out_grad + s.off[18] : nullptr, d.out_stats, d.step);
}

// ---------------------------------------------------------------------------------------------------------------------- the act call
template <int JW> __global__ __launch_bounds__(THREADS) void k_sac_act(Dev d) {
    XARM_TILE_LDS(JW);
    const int t = threadIdx.x, r = t & 63, wv = __builtin_amdgcn_readfirstlane(t >> 6), A = d.s.A;
    const int64_t r0 = (int64_t)blockIdx.x * ROWS, n = r0 + r;
    load_rows<JW>(Xt, d.obs, d.s.D, r0, d.s.B);
    __syncthreads();
    xa2c::tile_forward<true>(d.actor, d.s.D, 2 * A, L, r, wv);
    if (wv != 0 || n >= d.s.B) return;
    float z[MAX_A], a[MAX_A];
    const bool det = d.h.deterministic != 0;
    const int64_t calls = det ? 0 : d.calls[0];
#pragma unroll
    for (int b = 0; b < MAX_A / 4; b++) {
        float q[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        if (!det && 4 * b < A) xpol::noise4(d.h.seed, d.s.row_offset + n, calls, b, q);
#pragma unroll
        for (int m = 0; m < 4; m++) z[4 * b + m] = q[m];
    }
    const float lp = actor_head(A, D3t + r, LS, z, det, a);
#pragma unroll
    for (int c = 0; c < MAX_A; c++)
        if (c < A) d.out_action[n * A + c] = a[c];
    if (d.out_logp != nullptr) d.out_logp[n] = lp;
}

__global__ void k_sac_tick(int64_t *calls) {
    if (blockIdx.x == 0 && threadIdx.x == 0) calls[0] += 1;
}

int launch_update(const Dev &d, void *stream) {
    const hipStream_t s = (hipStream_t)stream;
    const Shape &sh = d.s;
    const dim3 one((unsigned)sh.G), two((unsigned)sh.G, 2);
    XARM_TILE_LAUNCH(sh.Dq, k_sac_rows, one, s, d);
    XARM_TILE_LAUNCH(sh.Dq, k_sac_qgrad, two, s, d);
    k_sac_qapply<<<dim3((unsigned)sh.NBq), dim3(RED), 0, s>>>(d);
    XARM_TILE_LAUNCH(sh.Dq, k_sac_dqda, two, s, d);
    XARM_TILE_LAUNCH(sh.D, k_sac_pgrad, one, s, d);
    k_sac_papply<<<dim3((unsigned)sh.NBp), dim3(RED), 0, s>>>(d);
    return (int)hipGetLastError();
}

int launch_act(const Dev &d, void *stream) {
    const hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)d.s.tiles);
    XARM_TILE_LAUNCH(d.s.D, k_sac_act, grid, s, d);
    if (!d.h.deterministic) k_sac_tick<<<dim3(1), dim3(1), 0, s>>>(d.calls);
    return (int)hipGetLastError();
}

}  // namespace xsac
