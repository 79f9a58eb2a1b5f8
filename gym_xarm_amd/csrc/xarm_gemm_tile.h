// xarm_gemm_tile.h - the three f32 MFMA GEMM kernels of the wide learners and the executor part that launches them.
// Device-only; included by xarm_k_sacw.hip, xarm_k_acw.hip, xarm_k_ppow.hip and xarm_k_a2cw.hip, each of which gets its own (internal) copy of
// the kernels it launches.
// The jobs (Fwd, Bd, Wg), the passes that fill them and the host build's loops over the same jobs are in xarm_sacw_core.h.
//
// A kernel runs one wavefront per workgroup on one 32 x 32 accumulator tile of v_mfma_f32_32x32x2_f32: the A operand's lane l & 31 is the
// tile's row, the B operand's lane l & 31 its column, lane half l >> 5 the k of the pair (half 0's product is added first), and register
// r of lane half h holds tile row 8 (r >> 2) + 4 h + (r & 3) of column l & 31.  The operands come straight from memory (L2: a layer's
// weights and one [256, 256] activation are 256 KB each); nothing is staged in LDS, so a tile's chain is the k order alone.
//   k_sacw_fwd     grid (row tiles, unit blocks, jobs).  A = x (row n), B = W (unit u): acc starts at b[u], the epilogue applies the
//                  activation and stores along u.  With K a multiple of 8 and 16-byte aligned operands both halves read the same 32 bytes
//                  of a row and pick their k of each pair; otherwise (the input layer) one guarded scalar load per operand and step.
//   k_sacw_bd      grid (row tiles, column blocks, jobs).  A = d (row n), B = W[k][c0 + i] (coalesced along i); epilogue pre * act'(h).
//   k_sacw_wg      grid (input blocks, unit blocks, jobs x row ranges).  A = d^T (unit j), B = x (input i; i = K is the bias column of
//                  ones), both coalesced; k runs over the range's rows.  A range's tile goes to the range's partial gradient.
// Each kernel has a GATED instantiation that starts with its header's gate (xarm_sacw_core.h Gate); the executor launches it only for a
// header whose gate is set - the wide PPO update with target_kl on.  Every other launch runs the instantiation without the read.
#pragma once
#include <hip/hip_runtime.h>
#include "xarm_sacw_core.h"

namespace xsacw {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ f32x16 mfma(float a, float b, f32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0); }
__device__ __forceinline__ int tile_row(int r, int h) { return 8 * (r >> 2) + 4 * h + (r & 3); }

// acc += A[row a][k] B[row b][k] over k < K, both operands K-contiguous rows (null: zeros)
__device__ __forceinline__ f32x16 dot_rows(const float *ar, const float *br, int K, int vec, int h, f32x16 acc) {
    if (vec) {
        for (int k0 = 0; k0 < K; k0 += 8) {
            f32x4 a0 = {0.0f, 0.0f, 0.0f, 0.0f}, a1 = a0, b0 = a0, b1 = a0;
            if (ar != nullptr) { a0 = *(const f32x4 *)(ar + k0); a1 = *(const f32x4 *)(ar + k0 + 4); }
            if (br != nullptr) { b0 = *(const f32x4 *)(br + k0); b1 = *(const f32x4 *)(br + k0 + 4); }
            acc = mfma(h ? a0[1] : a0[0], h ? b0[1] : b0[0], acc);
            acc = mfma(h ? a0[3] : a0[2], h ? b0[3] : b0[2], acc);
            acc = mfma(h ? a1[1] : a1[0], h ? b1[1] : b1[0], acc);
            acc = mfma(h ? a1[3] : a1[2], h ? b1[3] : b1[2], acc);
        }
    } else {
        for (int k0 = 0; k0 < K; k0 += 2) {
            const int k = k0 + h;
            const float av = (ar != nullptr && k < K) ? ar[k] : 0.0f;
            const float bv = (br != nullptr && k < K) ? br[k] : 0.0f;
            acc = mfma(av, bv, acc);
        }
    }
    return acc;
}

template <bool GATED> static __global__ __launch_bounds__(64) void k_sacw_fwd(Fwd f) {
    if (GATED && gate_shut(f.gate)) return;
    const FwdJob &a = f.j[blockIdx.z];
    if ((int)blockIdx.y * TILE >= a.N) return;
    const int lane = threadIdx.x, c = lane & 31, h = lane >> 5;
    const int u = blockIdx.y * TILE + c;
    const int64_t r0 = (int64_t)blockIdx.x * TILE, n = r0 + c;
    const bool ul = u < a.N;
    const float bias = ul ? a.b[u] : 0.0f;
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; r++) acc[r] = bias;
    acc = dot_rows(n < f.B ? a.x + n * a.K : nullptr, ul ? a.W + (int64_t)u * a.K : nullptr, a.K, a.vec, h, acc);
    if (!ul) return;
#pragma unroll
    for (int r = 0; r < 16; r++) {
        const int64_t nn = r0 + tile_row(r, h);
        if (nn < f.B) a.out[nn * a.N + u] = act_f(a.act, acc[r]);
    }
}

template <bool GATED> static __global__ __launch_bounds__(64) void k_sacw_bd(Bd f) {
    if (GATED && gate_shut(f.gate)) return;
    const BdJob &a = f.j[blockIdx.z];
    if ((int)blockIdx.y * TILE >= a.N) return;
    const int lane = threadIdx.x, c = lane & 31, h = lane >> 5;
    const int i = blockIdx.y * TILE + c;
    const int64_t r0 = (int64_t)blockIdx.x * TILE, n = r0 + c;
    const bool il = i < a.N, nl = n < f.B;
    const float *dr = a.d + (nl ? n : 0) * a.K, *wc = a.W + a.c0 + (il ? i : 0);
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; r++) acc[r] = 0.0f;
    if (a.vec) {
        for (int k0 = 0; k0 < a.K; k0 += 8) {
            f32x4 d0 = {0.0f, 0.0f, 0.0f, 0.0f}, d1 = d0;
            if (nl) { d0 = *(const f32x4 *)(dr + k0); d1 = *(const f32x4 *)(dr + k0 + 4); }
            float w[4];
#pragma unroll
            for (int m = 0; m < 4; m++) w[m] = il ? wc[(int64_t)(k0 + 2 * m + h) * a.ldw] : 0.0f;
            acc = mfma(h ? d0[1] : d0[0], w[0], acc);
            acc = mfma(h ? d0[3] : d0[2], w[1], acc);
            acc = mfma(h ? d1[1] : d1[0], w[2], acc);
            acc = mfma(h ? d1[3] : d1[2], w[3], acc);
        }
    } else {
        for (int k0 = 0; k0 < a.K; k0 += 2) {
            const int k = k0 + h;
            const bool kl = k < a.K;
            const float dv = (nl && kl) ? dr[k] : 0.0f;
            const float wv = (il && kl) ? wc[(int64_t)k * a.ldw] : 0.0f;
            acc = mfma(dv, wv, acc);
        }
    }
    if (!il) return;
#pragma unroll
    for (int r = 0; r < 16; r++) {
        const int64_t nn = r0 + tile_row(r, h);
        if (nn < f.B) {
            const float o = delta_f(a.mode, acc[r], a.mode == ACT_NONE ? 0.0f : a.h[nn * a.N + i]);
            a.out[nn * a.N + i] = o;
            if (a.out2 != nullptr) a.out2[nn * a.N + i] = o;
        }
    }
}

template <bool GATED> static __global__ __launch_bounds__(64) void k_sacw_wg(Wg f) {
    if (GATED && gate_shut(f.gate)) return;
    const int jn = blockIdx.z / f.S, sp = blockIdx.z - jn * f.S;
    const WgJob &a = f.j[jn];
    if ((int)blockIdx.x * TILE > a.K || (int)blockIdx.y * TILE >= a.N) return;
    const int lane = threadIdx.x, c = lane & 31, h = lane >> 5;
    const int j = blockIdx.y * TILE + c, i = blockIdx.x * TILE + c;     // j: the A operand's unit, i: the B operand's input
    const bool jl = j < a.N, il = i < a.K, one = i == a.K;
    const int64_t n0 = f.rows[sp], n1 = f.rows[sp + 1];
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; r++) acc[r] = 0.0f;
    for (int64_t nb = n0; nb < n1; nb += 8) {
        float dv[4], xv[4];
#pragma unroll
        for (int m = 0; m < 4; m++) {
            const int64_t n = nb + 2 * m + h;
            const bool nl = n < n1;
            dv[m] = (nl && jl) ? a.d[n * a.N + j] : 0.0f;
            xv[m] = nl ? (il ? a.x[n * a.K + i] : (one ? 1.0f : 0.0f)) : 0.0f;
        }
#pragma unroll
        for (int m = 0; m < 4; m++) {
            if (nb + 2 * m >= n1) break;                   // uniform: whole steps past the range are not issued
            acc = mfma(dv[m], xv[m], acc);
        }
    }
    if (!il && !one) return;
    float *part = f.partial + (int64_t)sp * f.pstride;
#pragma unroll
    for (int r = 0; r < 16; r++) {
        const int jj = blockIdx.y * TILE + tile_row(r, h);
        if (jj < a.N) {
            if (il) part[a.poff + (int64_t)jj * a.K + i] = acc[r];
            else part[a.boff + jj] = acc[r];
        }
    }
}

// the GEMM part of a device executor: what fwd_pass, bd_pass and wg_pass call; `count` is the launches so far
struct GemmExec {
    hipStream_t st;
    int count;
    static unsigned blocks(int64_t n, int per) { return (unsigned)((n + per - 1) / per); }
    void fwd(const Fwd &f) {
        const dim3 grid(blocks(f.B, TILE), blocks(f.maxN, TILE), f.nj);
        if (f.gate.stop != nullptr) k_sacw_fwd<true><<<grid, dim3(64), 0, st>>>(f);
        else k_sacw_fwd<false><<<grid, dim3(64), 0, st>>>(f);
        count++;
    }
    void bd(const Bd &f) {
        const dim3 grid(blocks(f.B, TILE), blocks(f.maxN, TILE), f.nj);
        if (f.gate.stop != nullptr) k_sacw_bd<true><<<grid, dim3(64), 0, st>>>(f);
        else k_sacw_bd<false><<<grid, dim3(64), 0, st>>>(f);
        count++;
    }
    void wg(const Wg &f) {
        const dim3 grid(blocks(f.maxK + 1, TILE), blocks(f.maxN, TILE), f.nj * f.S);
        if (f.gate.stop != nullptr) k_sacw_wg<true><<<grid, dim3(64), 0, st>>>(f);
        else k_sacw_wg<false><<<grid, dim3(64), 0, st>>>(f);
        count++;
    }
};

}  // namespace xsacw
