// xarm_grad_tile.h - one 64-row tile of the two-tower backward, shared by the gradient kernels of the A2C update (xarm_k_a2c.hip,
// DESIGN.md 21), of the PPO update (xarm_k_ppo.hip) and of the SAC update (xarm_k_sac.hip).  Device code
// only; the units are built with -ffp-contract=off.  Next to the tile, what those kernels share around it: the tile's LDS declaration
// (XARM_TILE_LDS), the launch of the instantiation that fits a width (XARM_TILE_LAUNCH), a workgroup's scalar record (store_scalars),
// the block tree (block_sum) and the reduce / apply bodies of the A2C and PPO updates (reduce_block, norm_and_clip).
//
// A workgroup of 256 threads works on ONE tower.  Per tile, in LDS and transposed ([unit][row], stride 65: a lane per row and a lane
// per unit both read without bank conflicts): the rows, h1 and h2 from the policy's chains (lane = row, wavefront w = units
// 16 w .. 16 w + 15, so the weights are wavefront-uniform loads), the output deltas, then d2 and d1 in place over h2 and h1 once the
// outer products that need h2 / h1 are taken.  The gradient lives in registers across the tiles (TileGrad): thread
// (ib, jb) = (t & 15, t >> 4) owns the entries (ib + 16 a, jb + 16 b) of dW2 and dW1, thread (t & 63, t >> 6) the entries of dW3.
//
// What differs between the algorithms is the Head:
//   int64_t row(int rr)               the batch row in tile slot rr, or -1 for an empty slot (its row enters as zeros)
//   void deltas(int r, float *D3)     called by lane r of wavefront 0: writes the output deltas of slot r to D3[c * LS], c < nout (they are
//                                     zero when it is called; an empty slot leaves them so)
//   FROM_H2                           false: the deltas need nothing of this tile's forward and are written with its load.
//                                     true: the tower's outputs W3 h2 + b3 (the policy's chain, order KORD) are put to D3[c * LS] first and
//                                     deltas() replaces them - a head that needs mean / value under the CURRENT weights.
// Two optional traits, which a head that does not name them leaves off (A2C's and PPO's do not: their instantiations are the
// operations above and nothing else):
//   INPUT_GRAD = true                 behind d1 the tile also forms the gradient at the tower's input, dx_j = sum_i W1[i][j] d1_i (i
//                                     ascending, fmaf from 0), for the columns col0() <= j < col0() + ncol(): lane r of wavefront w calls
//                                     void input_grad(int r, int c, float dx) for slot r and c = w, w + 4, ... (c counted from col0())
//   WEIGHT_GRAD = false               the outer products (dW3, dW2, dW1 and the bias sums) are skipped and G is not touched: a pass that
//                                     wants the tower's outputs and its input gradient only
#pragma once
#include <hip/hip_runtime.h>
#include "xarm_a2c_core.h"

namespace xa2c {

constexpr int THREADS = 256, LS = ROWS + 1, UPW = 16;     // LDS row stride; units per wavefront in the lane = row stages
static_assert(ROWS == 64 && THREADS == 4 * ROWS && UPW * (THREADS / 64) == HID, "four wavefronts: 64 rows x 16 units each");

template <class H, class = void> struct head_input_grad { static constexpr bool value = false; };
template <class H> struct head_input_grad<H, decltype((void)H::INPUT_GRAD)> { static constexpr bool value = H::INPUT_GRAD; };
template <class H, class = void> struct head_weight_grad { static constexpr bool value = true; };
template <class H> struct head_weight_grad<H, decltype((void)H::WEIGHT_GRAD)> { static constexpr bool value = H::WEIGHT_GRAD; };

struct TileLds {
    float *Xt, *H1t, *H2t, *D3t;       // [16 JW][LS], [HID][LS], [HID][LS], [MAX_ACT][LS]
};

// a tile kernel's LDS: the four arrays and L, their TileLds.  JW: 16 JW >= D columns in the tile
#define XARM_TILE_LDS(JW)                                                                   \
    __shared__ __attribute__((aligned(16))) float Xt[16 * JW * xa2c::LS];                   \
    __shared__ __attribute__((aligned(16))) float H1t[xpol::HID * xa2c::LS];                \
    __shared__ __attribute__((aligned(16))) float H2t[xpol::HID * xa2c::LS];                \
    __shared__ __attribute__((aligned(16))) float D3t[xpol::MAX_ACT * xa2c::LS];            \
    const xa2c::TileLds L = {Xt, H1t, H2t, D3t}

// launch the instantiation of a tile kernel that holds W columns: KERNEL<JW><<<GRID, THREADS, 0, STREAM>>>(arguments)
#define XARM_TILE_LAUNCH(W, KERNEL, GRID, STREAM, ...)                                                          \
    do {                                                                                                        \
        if ((W) <= 16) KERNEL<1><<<GRID, dim3(xa2c::THREADS), 0, STREAM>>>(__VA_ARGS__);                        \
        else if ((W) <= 32) KERNEL<2><<<GRID, dim3(xa2c::THREADS), 0, STREAM>>>(__VA_ARGS__);                   \
        else if ((W) <= 64) KERNEL<4><<<GRID, dim3(xa2c::THREADS), 0, STREAM>>>(__VA_ARGS__);                   \
        else KERNEL<6><<<GRID, dim3(xa2c::THREADS), 0, STREAM>>>(__VA_ARGS__);                                  \
    } while (0)

// the lanes of wavefront 0 hold NS float64 sums each; slot k of this workgroup's record <- the lanes added in lane order.  lds: h1's tile
template <int NS> __device__ __forceinline__ void store_scalars(float *lds, const double (&sums)[NS], double *record) {
    const int t = threadIdx.x;
    double *sc = (double *)lds;
    static_assert(NS * 64 * sizeof(double) <= HID * LS * sizeof(float), "the scalars fit h1's tile");
    __syncthreads();
    if (t < 64) {
#pragma unroll
        for (int i = 0; i < NS; i++) sc[i * 64 + t] = sums[i];
    }
    __syncthreads();
    if (t < NS) {
        double sum = 0.0;
        for (int l = 0; l < 64; l++) sum += sc[t * 64 + l];
        record[t] = sum;
    }
}

// ---- behind the gradient kernel, one thread per flat parameter in blocks of RED: what k_a2c_reduce / k_a2c_apply and k_ppo_reduce /
// k_ppo_apply share.  scal: the policy tower's group records, nscal doubles each (slot 2: sum use, slots 3 + c: log_std_c's sums)

// a block's sum of one double per thread: a fixed tree; every thread gets the sum
__device__ __forceinline__ double block_sum(double *red, double x) {
    const int tid = threadIdx.x;
    __syncthreads();
    red[tid] = x;
    __syncthreads();
    for (int s = RED / 2; s > 0; s >>= 1) {
        if (tid < s) red[tid] += red[tid + s];
        __syncthreads();
    }
    return red[0];
}

__device__ __forceinline__ double groups_n_use(const Shape &s, const double *scal, int nscal) {
    double nuse = 0.0;
    for (int g = 0; g < s.G; g++) nuse += scal[(int64_t)g * nscal + 2];
    return xopt::n_use(nuse);
}

// the gradient of flat parameter p: its groups' sums added in float64 in group order, / n_use, the entropy term on log_std
__device__ __forceinline__ float param_grad(const Shape &s, const float *partial, const double *scal, int nscal, double n_use, double ent_coef, int64_t p) {
    const bool ls = p >= s.off[12];
    double sum = 0.0;
    if (ls) {
        const int c = (int)(p - s.off[12]);
        for (int g = 0; g < s.G; g++) sum += scal[(int64_t)g * nscal + 3 + c];
    } else {
        const int tower = p >= s.off[6] ? 1 : 0;
        sum = xopt::slice_sum(partial + (int64_t)tower * s.G * s.pstride + (p - (tower ? s.off[6] : 0)), s.G, s.pstride);
    }
    double v = sum / n_use;
    if (ls) v -= ent_coef;
    return (float)v;
}

// the reduce kernel's body: grad (and out_grad, nullable) of the block's parameters, the block's sum of squares to normpart; returns n_use
__device__ __forceinline__ double reduce_block(const Shape &s, const float *partial, const double *scal, int nscal, double ent_coef, float *grad,
                                               float *out_grad, double *red, double *normpart) {
    const int64_t p = (int64_t)blockIdx.x * RED + threadIdx.x;
    const double n_use = groups_n_use(s, scal, nscal);
    double sq = 0.0;
    if (p < s.P) {
        const float gf = param_grad(s, partial, scal, nscal, n_use, ent_coef, p);
        grad[p] = gf;
        if (out_grad != nullptr) out_grad[p] = gf;
        sq = (double)gf * (double)gf;
    }
    sq = block_sum(red, sq);
    if (threadIdx.x == 0) normpart[blockIdx.x] = sq;
    return n_use;
}

// the apply kernel's head: the norm from normpart in block order; returns the clip coefficient
__device__ __forceinline__ float norm_and_clip(const Shape &s, const double *normpart, float max_norm, float &norm) {
    double sum2 = 0.0;
    for (int b = 0; b < s.NB; b++) sum2 += normpart[b];
    norm = (float)__builtin_sqrt(sum2);
    return xopt::clip_coef(norm, max_norm);
}

// JW: columns of dW1 per thread; the tile holds 16 JW >= D columns
template <int JW> struct TileGrad {
    float g1[4][JW], gb1[4], g2[4][4], gb2[4], g3[4], gb3[4];

    __device__ __forceinline__ void zero() {
#pragma unroll
        for (int a = 0; a < 4; a++) {
            gb1[a] = gb2[a] = g3[a] = gb3[a] = 0.0f;
#pragma unroll
            for (int b = 0; b < 4; b++) g2[a][b] = 0.0f;
#pragma unroll
            for (int m = 0; m < JW; m++) g1[a][m] = 0.0f;
        }
    }

    // the workgroup's slice: one tower's tensors in the flat order
    __device__ __forceinline__ void store(float *slice, int D, int nout) const {
        const int t = threadIdx.x, r = t & 63, wv = __builtin_amdgcn_readfirstlane(t >> 6), ib = t & 15, jb = t >> 4;
        float *sW1 = slice, *sb1 = sW1 + HID * D, *sW2 = sb1 + HID, *sb2 = sW2 + HID * HID, *sW3 = sb2 + HID, *sb3 = sW3 + nout * HID;
#pragma unroll
        for (int a = 0; a < 4; a++) {
            const int i = ib + 16 * a;
#pragma unroll
            for (int m = 0; m < JW; m++)
                if (jb + 16 * m < D) sW1[i * D + jb + 16 * m] = g1[a][m];
#pragma unroll
            for (int b = 0; b < 4; b++) sW2[i * HID + jb + 16 * b] = g2[a][b];
            if (jb == 0) { sb1[i] = gb1[a]; sb2[i] = gb2[a]; }
            const int c = 4 * wv + a;
            if (c < nout) {
                sW3[c * HID + r] = g3[a];
                if (r == 0) sb3[c] = gb3[a];
            }
        }
    }
};

// the forward of one tile from the rows in Xt: h1 and h2 by the policy's chains (lane = row, wavefront w = units 16 w .. 16 w + 15) and,
// with OUTPUTS, the tower's outputs W3 h2 + b3 in D3t[c * LS + row], c < nout.  r, wv: the thread's lane and (wavefront-uniform)
// wavefront.  Starts behind a barrier on Xt, ends on a barrier.
template <bool OUTPUTS>
__device__ __forceinline__ void tile_forward(const Tower &T, int D, int nout, const TileLds &L, int r, int wv) {
    float *const Xt = L.Xt, *const H1t = L.H1t, *const H2t = L.H2t, *const D3t = L.D3t;
    const int u0 = UPW * wv;
    {   // h1
        float acc[UPW];
#pragma unroll
        for (int u = 0; u < UPW; u++) acc[u] = T.b1[u0 + u];
        xpol::layer1_chains<UPW>(T.W1 + u0 * D, D, Xt + r, LS, acc);
#pragma unroll
        for (int u = 0; u < UPW; u++) H1t[(u0 + u) * LS + r] = xpol::tanh_f(acc[u]);
    }
    __syncthreads();
    {   // h2
        float acc[UPW];
#pragma unroll
        for (int u = 0; u < UPW; u++) acc[u] = T.b2[u0 + u];
        xpol::hidden_chains<UPW>(T.W2 + u0 * HID, H1t + r, LS, acc);
#pragma unroll
        for (int u = 0; u < UPW; u++) H2t[(u0 + u) * LS + r] = xpol::tanh_f(acc[u]);
    }
    __syncthreads();

    if constexpr (OUTPUTS) {
        // the outputs: wavefront w takes outputs 4 w .. 4 w + 3 (rows of W3 past nout do not exist and are not read)
#pragma unroll
        for (int a = 0; a < 4; a++) {
            const int c = 4 * wv + a;
            if (c < nout) {
                float acc[1] = {T.b3[c]};
                xpol::hidden_chains<1>(T.W3 + c * HID, H2t + r, LS, acc);
                D3t[c * LS + r] = acc[0];
            }
        }
        __syncthreads();
    }
}

// one tile; ends on a barrier, so the caller may rewrite what row() reads and call it again
template <int JW, class Head>
__device__ __forceinline__ void grad_tile(const Tower &T, int D, int nout, const float *obs, const TileLds &L, Head &head, TileGrad<JW> &G) {
    float *const Xt = L.Xt, *const H1t = L.H1t, *const H2t = L.H2t, *const D3t = L.D3t;
    const int t = threadIdx.x, r = t & 63, wv = __builtin_amdgcn_readfirstlane(t >> 6), u0 = UPW * wv, ib = t & 15, jb = t >> 4;

    // the tile's rows (zeros in empty slots and past column D) and the deltas at the outputs (wavefront 0: lane = row)
    for (int idx = t; idx < 16 * JW * ROWS; idx += THREADS) {
        const int rr = idx / (16 * JW), j = idx - rr * (16 * JW);
        const int64_t n = head.row(rr);
        Xt[j * LS + rr] = (n >= 0 && j < D) ? obs[n * D + j] : 0.0f;
    }
    if (wv == 0) {
#pragma unroll
        for (int c = 0; c < MAX_ACT; c++) D3t[c * LS + r] = 0.0f;
        if constexpr (!Head::FROM_H2) head.deltas(r, D3t + r);
    }
    __syncthreads();

    tile_forward<Head::FROM_H2>(T, D, nout, L, r, wv);

    if constexpr (Head::FROM_H2) {
        if (wv == 0) head.deltas(r, D3t + r);
        __syncthreads();
    }

    constexpr bool WG = head_weight_grad<Head>::value;
    if constexpr (WG) {
        // dW3, db3: thread (unit r, outputs 4 wv .. 4 wv + 3)
        if (4 * wv < nout) {
            for (int rr = 0; rr < ROWS; rr++) {
                const float hv = H2t[r * LS + rr];
#pragma unroll
                for (int a = 0; a < 4; a++) {
                    const float dv = D3t[(4 * wv + a) * LS + rr];
                    G.g3[a] = fma32(dv, hv, G.g3[a]);
                    G.gb3[a] += dv;
                }
            }
        }
        __syncthreads();
    }
    {   // d2 over h2
        float pre[UPW];
#pragma unroll
        for (int u = 0; u < UPW; u++) pre[u] = 0.0f;
        for (int c = 0; c < nout; c++) {
            const float dv = D3t[c * LS + r];
#pragma unroll
            for (int u = 0; u < UPW; u++) pre[u] = fma32(T.W3[c * HID + u0 + u], dv, pre[u]);
        }
#pragma unroll
        for (int u = 0; u < UPW; u++) {
            const float hv = H2t[(u0 + u) * LS + r];
            H2t[(u0 + u) * LS + r] = pre[u] * fma32(-hv, hv, 1.0f);
        }
    }
    __syncthreads();

    if constexpr (WG) {
        // dW2, db2: thread (ib, jb) owns (ib + 16 a, jb + 16 b)
        for (int rr = 0; rr < ROWS; rr++) {
            float dv[4], hv[4];
#pragma unroll
            for (int a = 0; a < 4; a++) { dv[a] = H2t[(ib + 16 * a) * LS + rr]; hv[a] = H1t[(jb + 16 * a) * LS + rr]; }
#pragma unroll
            for (int a = 0; a < 4; a++) {
                G.gb2[a] += dv[a];
#pragma unroll
                for (int b = 0; b < 4; b++) G.g2[a][b] = fma32(dv[a], hv[b], G.g2[a][b]);
            }
        }
        __syncthreads();
    }
    {   // d1 over h1
        float pre[UPW];
#pragma unroll
        for (int u = 0; u < UPW; u++) pre[u] = 0.0f;
        for (int k = 0; k < HID; k++) {
            const float dv = H2t[k * LS + r];
#pragma unroll
            for (int u = 0; u < UPW; u++) pre[u] = fma32(T.W2[k * HID + u0 + u], dv, pre[u]);
        }
#pragma unroll
        for (int u = 0; u < UPW; u++) {
            const float hv = H1t[(u0 + u) * LS + r];
            H1t[(u0 + u) * LS + r] = pre[u] * fma32(-hv, hv, 1.0f);
        }
    }
    __syncthreads();

    if constexpr (head_input_grad<Head>::value) {
        // dx over the head's columns: lane = row, wavefront wv the columns wv, wv + 4, ... (W1's column is a wavefront-uniform load)
        const int c0 = head.col0(), nc = head.ncol();
        for (int c = wv; c < nc; c += THREADS / 64) {
            float dx = 0.0f;
            for (int i = 0; i < HID; i++) dx = fma32(T.W1[i * D + c0 + c], H1t[i * LS + r], dx);
            head.input_grad(r, c, dx);
        }
    }
    if constexpr (WG) {
        // dW1, db1: thread (ib, jb) owns (ib + 16 a, jb + 16 m)
        for (int rr = 0; rr < ROWS; rr++) {
            float dv[4], xv[JW];
#pragma unroll
            for (int a = 0; a < 4; a++) dv[a] = H1t[(ib + 16 * a) * LS + rr];
#pragma unroll
            for (int m = 0; m < JW; m++) xv[m] = Xt[(jb + 16 * m) * LS + rr];
#pragma unroll
            for (int a = 0; a < 4; a++) {
                G.gb1[a] += dv[a];
#pragma unroll
                for (int m = 0; m < JW; m++) G.g1[a][m] = fma32(dv[a], xv[m], G.g1[a][m]);
            }
        }
    }
    __syncthreads();
}

}  // namespace xa2c
