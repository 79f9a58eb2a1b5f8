// xarm_k_policy.hip - the kernel of the device-resident MlpPolicy.  Core: xarm_policy_core.h.
// Built with -ffp-contract=off (build.py UNIT_FLAGS): every float32 operation is the one the host build performs.
//
//   k_policy_act   one wavefront per tile of 32 rows, four wavefronts per workgroup.  The products run on
//                  v_mfma_f32_32x32x2_f32 with the weights as the A operand and the batch as the B operand: lane l serves batch
//                  row l & 31, the layer's units are the rows of the accumulator tile, and one instruction adds the products of
//                  two k, lane half 0's first - bit for bit fmaf(a1, b1, fmaf(a0, b0, c)).  Layer 1 feeds column 2 s + (l >> 5) at
//                  step s.  A hidden layer's two accumulator tiles, after the tanh on the VALU, ARE the next layer's B operands:
//                  register r of tile t at step 16 t + r, which is the k order xpol::KORD.  The weights are read through L2 (at
//                  most 84 KB, shared by every wavefront of the grid): lane (i, h) loads the 16-byte pieces [8 q + 4 h, + 4) of
//                  row i of W, one piece per four steps.  Rows past the batch in the last tile are computed on zeros and never
//                  stored.  The mean's 16 columns lie in registers 0-7 of the two lane halves (half h: column blocks h and h + 2);
//                  each half draws and finishes its own blocks, and half 0 adds the log-probability terms in column order after
//                  one exchange with lane + 32.
//   k_policy_tick  one thread, behind a stochastic k_policy_act on the same stream: calls += 1.
#include <hip/hip_runtime.h>
#include "xarm_policy_core.h"

namespace xpol {

constexpr int WAVE = 64, WAVES = 4, THREADS = WAVE * WAVES;
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ f32x16 mfma(float a, float b, f32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0); }

// accumulator tile t of a layer with n units, filled with the bias: register r of lane half h is unit unit_of(t, r, h)
__device__ __forceinline__ f32x16 bias_tile(const float *b, int t, int h, int n) {
    f32x16 c;
#pragma unroll
    for (int g = 0; g < 4; g++) {
        const int u0 = unit_of(t, 4 * g, h);
        if (n == HID) {
            const f32x4 v = *(const f32x4 *)(b + u0);
            c[4 * g] = v[0]; c[4 * g + 1] = v[1]; c[4 * g + 2] = v[2]; c[4 * g + 3] = v[3];
        } else {
#pragma unroll
            for (int m = 0; m < 4; m++) c[4 * g + m] = u0 + m < n ? b[u0 + m] : 0.0f;
        }
    }
    return c;
}

__device__ __forceinline__ void tanh_tile(f32x16 &c) {
#pragma unroll
    for (int r = 0; r < 16; r++) c[r] = tanh_f(c[r]);
}

// one output tile of a 64-wide layer: c += W[row, KORD] . (x0 | x1), W's row `row` (null: a zero row beyond the layer's units)
__device__ __forceinline__ f32x16 hidden_tile(const float *wrow, int h, const f32x16 &x0, const f32x16 &x1, f32x16 c) {
#pragma unroll
    for (int q = 0; q < 8; q++) {
        f32x4 w = {0.0f, 0.0f, 0.0f, 0.0f};
        if (wrow != nullptr) w = *(const f32x4 *)(wrow + 8 * q + 4 * h);
#pragma unroll
        for (int m = 0; m < 4; m++) c = mfma(w[m], q < 4 ? x0[4 * q + m] : x1[4 * (q - 4) + m], c);
    }
    return c;
}

// layers 2 and 3 of one tower from the layer-1 accumulators (already through the tanh); returns the output tile
__device__ __forceinline__ f32x16 tower_tail(const Tower &T, int nout, int i, int h, const f32x16 &a0, const f32x16 &a1) {
    f32x16 c0 = hidden_tile(T.W2 + i * HID, h, a0, a1, bias_tile(T.b2, 0, h, HID));
    f32x16 c1 = hidden_tile(T.W2 + (32 + i) * HID, h, a0, a1, bias_tile(T.b2, 1, h, HID));
    tanh_tile(c0);
    tanh_tile(c1);
    return hidden_tile(i < nout ? T.W3 + i * HID : nullptr, h, c0, c1, bias_tile(T.b3, 0, h, nout));
}

__global__ __launch_bounds__(THREADS) void k_policy_act(Args a) {
    const int lane = threadIdx.x & (WAVE - 1), i = lane & 31, h = lane >> 5;
    const int64_t r0 = ((int64_t)blockIdx.x * WAVES + (threadIdx.x >> 6)) * TILE;
    if (r0 >= a.E) return;                                 // wavefront-uniform
    const int64_t e = r0 + i;
    const bool live = e < a.E, with_value = a.value != nullptr;
    const int64_t el = live ? e : a.E - 1;                 // the row whose memory a dead lane may touch
    const int D = a.D;

    // layer 1, both towers: column 2 s + h of the row against column 2 s + h of W1's rows i and 32 + i
    f32x16 p0 = bias_tile(a.pi.b1, 0, h, HID), p1 = bias_tile(a.pi.b1, 1, h, HID), v0, v1;
    if (with_value) { v0 = bias_tile(a.vf.b1, 0, h, HID); v1 = bias_tile(a.vf.b1, 1, h, HID); }
    for (int s0 = 0; 2 * s0 < D; s0 += 4) {
        float x[4], wp0[4], wp1[4], wv0[4], wv1[4];
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const int c = 2 * (s0 + u) + h, cc = c < D ? c : D - 1;
            const bool in = c < D;
            const float xv = input_at(a, el, cc);
            x[u] = in && live ? xv : 0.0f;
            const float w0 = a.pi.W1[i * D + cc], w1 = a.pi.W1[(32 + i) * D + cc];
            wp0[u] = in ? w0 : 0.0f; wp1[u] = in ? w1 : 0.0f;
            if (with_value) {
                const float y0 = a.vf.W1[i * D + cc], y1 = a.vf.W1[(32 + i) * D + cc];
                wv0[u] = in ? y0 : 0.0f; wv1[u] = in ? y1 : 0.0f;
            }
        }
#pragma unroll
        for (int u = 0; u < 4; u++) {
            if (2 * (s0 + u) >= D) break;                  // uniform: whole steps of padding are not issued
            p0 = mfma(wp0[u], x[u], p0);
            p1 = mfma(wp1[u], x[u], p1);
            if (with_value) { v0 = mfma(wv0[u], x[u], v0); v1 = mfma(wv1[u], x[u], v1); }
        }
    }

    tanh_tile(p0);
    tanh_tile(p1);
    const f32x16 mean = tower_tail(a.pi, a.A, i, h, p0, p1);

    // columns: half h holds blocks h (registers 0-3) and h + 2 (registers 4-7)
    const int64_t calls = a.deterministic ? 0 : a.calls[0];
    float term[8];
#pragma unroll
    for (int g = 0; g < 2; g++) {
        const int b = 2 * g + h;
        float z[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        if (!a.deterministic && 4 * b < a.A) noise4(a.seed, a.row_offset + e, calls, b, z);
#pragma unroll
        for (int m = 0; m < 4; m++) {
            const int c = 4 * b + m;
            term[4 * g + m] = 0.0f;
            if (c < a.A) {
                float act, env;
                term[4 * g + m] = finish_column(mean[4 * g + m], a.log_std[c], z[m], a.deterministic != 0, act, env);
                if (live) {
                    a.action[e * a.A + c] = act;
                    a.env_action[e * a.A + c] = env;
                }
            }
        }
    }
    if (a.logp != nullptr) {
        float other[8];
#pragma unroll
        for (int k = 0; k < 8; k++) other[k] = __shfl(term[k], lane ^ 32, WAVE);
        float lp = term[0];                                // column 0: half 0, register 0
#pragma unroll
        for (int c = 1; c < MAX_ACT; c++) {
            const int b = c >> 2, m = c & 3;
            const float t = (b & 1) ? other[4 * (b >> 1) + m] : term[4 * (b >> 1) + m];
            if (c < a.A) lp = lp + t;
        }
        if (live && h == 0) a.logp[e] = lp;
    }

    if (with_value) {
        tanh_tile(v0);
        tanh_tile(v1);
        const f32x16 val = tower_tail(a.vf, 1, i, h, v0, v1);
        if (live && h == 0) a.value[e] = val[0];
    }
}

__global__ void k_policy_tick(int64_t *calls) {
    if (blockIdx.x == 0 && threadIdx.x == 0) calls[0] += 1;
}

int launch_policy(const Args &a, int64_t *calls, void *stream) {
    const hipStream_t s = (hipStream_t)stream;
    const int64_t tiles = (a.E + TILE - 1) / TILE;
    k_policy_act<<<dim3((unsigned)((tiles + WAVES - 1) / WAVES)), dim3(THREADS), 0, s>>>(a);
    if (!a.deterministic) k_policy_tick<<<dim3(1), dim3(1), 0, s>>>(calls);
    return (int)hipGetLastError();
}

}  // namespace xpol
