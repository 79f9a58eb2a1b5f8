// xarm_cubes_dev.h - device-only parts of the two-arm cube scenes' kernels (core: xarm_stack_core.h), templated on the scene
// description Sc: state load / store, observation, reward, and the class-order kernels' bodies.  xarm_k_stack.hip (xs::Tower3)
// and xarm_k_rearrange.hip (xra::Rearrange4) build their __global__ kernels from these: two translation units, so the two big
// kernels compile in parallel.
// The init / step / reset kernels themselves are written out in each unit, in the same words but for the scene alias and the
// LDS accessor: as one more inlined function between the __global__ entry and lane_step / lane_reset, their bodies are compiled
// to other code - the loads of the by-value KParams fields land elsewhere and the whole 30 000-instruction kernel is scheduled
// anew (profiles/r09a_cubes_one_core.txt); spelled in the kernel, the assembly is what it was before the two cores were one.
#pragma once
#include "xarm_dev.h"

namespace xd {

template <typename Sc> __device__ __forceinline__ void cubes_load(const KParams &P, int64_t e, int arm, xs::Lane<float, Sc> &L) {
    const float *S = P.state + e;
    const int64_t n = P.stride;
#pragma unroll
    for (int i = 0; i < 9; i++) {
        L.q[i] = S[(Sc::K_Q + 9 * arm + i) * n]; L.qd[i] = S[(Sc::K_QD + 9 * arm + i) * n]; L.qt[i] = S[(Sc::K_QT + 9 * arm + i) * n];
    }
#pragma unroll
    for (int o = 0; o < Sc::NOBJ; o++) {
#pragma unroll
        for (int k = 0; k < 3; k++) {
            L.bp[o][k] = S[(Sc::K_BP + 3 * o + k) * n]; L.bv[o][k] = S[(Sc::K_BV + 3 * o + k) * n];
            L.bw[o][k] = S[(Sc::K_BW + 3 * o + k) * n]; L.goal[o][k] = S[(Sc::K_GOAL + 3 * o + k) * n];
        }
#pragma unroll
        for (int k = 0; k < 4; k++) L.bq[o][k] = S[(Sc::K_BQ + 4 * o + k) * n];
#pragma unroll
        for (int k = 0; k < 8; k++) L.lam_t[o][k] = S[(Sc::K_LT + 8 * o + k) * n];
    }
#pragma unroll
    for (int k = 0; k < 4; k++) L.lam_p[k] = S[(Sc::K_LP + 4 * arm + k) * n];
    L.steps = S[Sc::K_STEPS * n]; L.episode = S[Sc::K_EPISODE * n];
    L.cls = 0;
}

template <typename Sc> __device__ __forceinline__ void cubes_store(const KParams &P, int64_t e, int arm, const xs::Lane<float, Sc> &L) {
    float *S = P.state + e;
    const int64_t n = P.stride;
#pragma unroll
    for (int i = 0; i < 9; i++) {
        S[(Sc::K_Q + 9 * arm + i) * n] = L.q[i]; S[(Sc::K_QD + 9 * arm + i) * n] = L.qd[i]; S[(Sc::K_QT + 9 * arm + i) * n] = L.qt[i];
    }
#pragma unroll
    for (int k = 0; k < 4; k++) S[(Sc::K_LP + 4 * arm + k) * n] = L.lam_p[k];
    if (arm == 0) { // shared fields are bit-identical in both lanes
#pragma unroll
        for (int o = 0; o < Sc::NOBJ; o++) {
#pragma unroll
            for (int k = 0; k < 3; k++) {
                S[(Sc::K_BP + 3 * o + k) * n] = L.bp[o][k]; S[(Sc::K_BV + 3 * o + k) * n] = L.bv[o][k];
                S[(Sc::K_BW + 3 * o + k) * n] = L.bw[o][k]; S[(Sc::K_GOAL + 3 * o + k) * n] = L.goal[o][k];
            }
#pragma unroll
            for (int k = 0; k < 4; k++) S[(Sc::K_BQ + 4 * o + k) * n] = L.bq[o][k];
#pragma unroll
            for (int k = 0; k < 8; k++) S[(Sc::K_LT + 8 * o + k) * n] = L.lam_t[o][k];
        }
        S[Sc::K_STEPS * n] = L.steps; S[Sc::K_EPISODE * n] = L.episode;
    }
}

// observation (_get_obs :190-199): cube pos 3N, quat 4N, v 3N, w 3N, then per arm hand COM pos 3, vel 3, finger q, qd
template <typename Sc>
__device__ __forceinline__ void cubes_write_obs(const xs::Lane<float, Sc> &L, int64_t e, int arm, float *obs_out, float *ag_out, float *dg_out) {
    float o8[8];
    xs::arm_obs(L, arm, o8);
    float *o = obs_out + e * Sc::OBS_DIM;
#pragma unroll
    for (int k = 0; k < 8; k++) o[Sc::O_ARM + 8 * arm + k] = o8[k];
    if (arm == 0) {
#pragma unroll
        for (int ob = 0; ob < Sc::NOBJ; ob++) {
#pragma unroll
            for (int k = 0; k < 3; k++) {
                o[Sc::O_BP + 3 * ob + k] = L.bp[ob][k]; o[Sc::O_BV + 3 * ob + k] = L.bv[ob][k]; o[Sc::O_BW + 3 * ob + k] = L.bw[ob][k];
                if (ag_out) { ag_out[e * Sc::GOAL_DIM + 3 * ob + k] = L.bp[ob][k]; dg_out[e * Sc::GOAL_DIM + 3 * ob + k] = L.goal[ob][k]; }
            }
#pragma unroll
            for (int k = 0; k < 4; k++) o[Sc::O_BQ + 4 * ob + k] = L.bq[ob][k];
        }
    }
}

// class-homogeneous wavefronts (xarm_stack_core.h class_layout): histogram of the per-env class keys, then every env takes
// the next slot of its class; order[slot] = env is the order the step kernel visits the envs in.  The arrival order inside a
// class comes from an atomic counter and differs from run to run - it decides which wavefront an env shares, never its
// result (an env is bitwise independent of its neighbours).  h: NCLS ints of shared memory.
template <int NCLS> __device__ __forceinline__ void class_hist(const uint8_t *__restrict__ key, int64_t n, int *__restrict__ hist, int *h) {
    for (int c = threadIdx.x; c < NCLS; c += blockDim.x) h[c] = 0;
    __syncthreads();
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e < n) atomicAdd(&h[key[e] & (NCLS - 1)], 1);
    __syncthreads();
    for (int c = threadIdx.x; c < NCLS; c += blockDim.x)
        if (h[c]) atomicAdd(&hist[c], h[c]);
}

// Y, cnt, base: shared memory
template <int NCLS>
__device__ __forceinline__ void class_place(const uint8_t *__restrict__ key, int64_t n, const int *__restrict__ hist, int *__restrict__ cursor,
                                            int *__restrict__ order, int group, xs::ClassLayoutN<NCLS> &Y, int *cnt, int *base) {
    for (int c = threadIdx.x; c < NCLS; c += blockDim.x) { cnt[c] = 0; base[c] = 0; }
    if (threadIdx.x == 0) {
        int hh[NCLS];
        for (int c = 0; c < NCLS; c++) hh[c] = hist[c];
        xs::class_layout(hh, group, Y);
    }
    __syncthreads();
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int c = e < n ? (int)(key[e] & (NCLS - 1)) : 0;
    // arrival number inside the class: rank inside the block (LDS counter), one global atomic per block and class -
    // thousands of class-0 envs on one global counter cost 90 us per call
    const int local = e < n ? atomicAdd(&cnt[c], 1) : 0;
    __syncthreads();
    for (int k = threadIdx.x; k < NCLS; k += blockDim.x)
        if (cnt[k]) base[k] = atomicAdd(&cursor[k], cnt[k]);
    __syncthreads();
    if (e >= n) return;
    const int slot = xs::class_slot(Y, c, base[c] + local);
    if (slot >= 0 && slot < n) order[slot] = (int)e;   // always true for a histogram of these keys; never write outside
}

// compute_reward (:124-129) over n rows of 3N
template <typename Sc>
__device__ __forceinline__ void cubes_compute_reward(int reward_type, const float *__restrict__ ag, const float *__restrict__ g, int64_t n, float *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float d2 = 0.f;
#pragma unroll
    for (int k = 0; k < Sc::GOAL_DIM; k++) { const float d = ag[i * Sc::GOAL_DIM + k] - g[i * Sc::GOAL_DIM + k]; d2 += d * d; }
    const float d = sqrtf(d2);
    out[i] = reward_type == 0 ? (d > (float)Sc::DISTANCE_THRESHOLD ? -1.f : 0.f) : -d;
}

} // namespace xd
