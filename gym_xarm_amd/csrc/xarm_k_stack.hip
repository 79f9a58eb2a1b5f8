// xarm_k_stack.hip - XarmPDStackTower-v0 (two arms, three cubes, one tower goal; scene: xs::Tower3 in xarm_stack_core.h).
// Part of libxarm_hip.so (gfx950); shared declarations: xarm_dev.h, shared kernel parts: xarm_cubes_dev.h, C ABI: xarm_hip.hip.
#include "xarm_cubes_dev.h"

namespace xd {

// --------------------------------------------------------------------- LDS: a private copy of every column per lane
// 603 LDS floats per lane = 151 KB per wavefront: one wavefront per CU, which is this scene's BASELINE size
// (8192 envs per GPU = 256 wavefronts)
using Sc = xs::Tower3;

__global__ __launch_bounds__(WG) void k_st_init(KParams P) {
    const int64_t t = (int64_t)blockIdx.x * WG + threadIdx.x, e = t >> 1;
    const int arm = (int)(t & 1);
    if (e >= P.num_envs) return;
    xs::Lane<float, Sc> L;
    xs::lane_init<float>(P.cfg, e, L);
    cubes_store(P, e, arm, L);
}

__global__ void k_class_hist(const uint8_t *__restrict__ key, int64_t n, int *__restrict__ hist) {
    __shared__ int h[Sc::NCLS];
    class_hist<Sc::NCLS>(key, n, hist, h);
}

__global__ void k_class_place(const uint8_t *__restrict__ key, int64_t n, const int *__restrict__ hist, int *__restrict__ cursor,
                              int *__restrict__ order, int group) {
    __shared__ xs::ClassLayoutN<Sc::NCLS> Y;
    __shared__ int cnt[Sc::NCLS], base[Sc::NCLS];
    class_place<Sc::NCLS>(key, n, hist, cursor, order, group, Y, cnt, base);
}

__global__ __launch_bounds__(WG) void k_st_step(KParams P, const float *__restrict__ actions, float *__restrict__ obs_out,
                                                float *__restrict__ ag_out, float *__restrict__ dg_out,
                                                float *__restrict__ rew_out, uint8_t *__restrict__ done_out,
                                                uint8_t *__restrict__ succ_out, float *__restrict__ term_obs,
                                                int *__restrict__ done_list, int *__restrict__ done_count,
                                                const int *__restrict__ order, uint8_t *__restrict__ key) {
    __shared__ float smem[Sc::LDS_FLOATS * WG];
    const int64_t t = (int64_t)blockIdx.x * WG + threadIdx.x, slot = t >> 1;
    const int arm = (int)(t & 1);
    if (slot >= P.num_envs) return;
    const int64_t e_in = order ? (int64_t)order[slot] : slot;
    DevLds lds{smem + threadIdx.x};
    xs::Lane<float, Sc> L;
    cubes_load(P, e_in, arm, L);
    const float4 a4 = reinterpret_cast<const float4 *>(actions)[e_in * 2 + arm];
    const float act[4] = {a4.x, a4.y, a4.z, a4.w};
    float reward;
    bool done, success;
    xs::lane_step<float, DevLds, DppXchg>(P.cfg, L, arm, act, reward, done, success, lds, DppXchg());
    const int64_t e = late_index(e_in);
    cubes_store(P, e, arm, L);
    cubes_write_obs(L, e, arm, obs_out, ag_out, dg_out);
    if (done && P.auto_reset && term_obs) cubes_write_obs(L, e, arm, term_obs, nullptr, nullptr);
    if (arm == 0) {
        if (key) key[e] = (uint8_t)L.cls;
        rew_out[e] = reward;
        done_out[e] = done ? 1 : 0;
        succ_out[e] = success ? 1 : 0;
        if (done && P.auto_reset) {
            const int pos = atomicAdd(done_count, 1);
            done_list[pos] = (int)e;
        }
    }
}

__global__ __launch_bounds__(WG) void k_st_reset(KParams P, const int *__restrict__ list, const int *__restrict__ count,
                                                 float *__restrict__ obs_out, float *__restrict__ ag_out, float *__restrict__ dg_out,
                                                 uint8_t *__restrict__ key) {
    __shared__ float smem[Sc::LDS_FLOATS * WG];
    const int64_t t = (int64_t)blockIdx.x * WG + threadIdx.x, i = t >> 1;
    const int arm = (int)(t & 1);
    const int64_t n = count ? (int64_t)*count : P.num_envs;
    if (i >= n) return;
    const int64_t e_in = list ? (int64_t)list[i] : i;
    DevLds lds{smem + threadIdx.x};
    xs::Lane<float, Sc> L;
    cubes_load(P, e_in, arm, L);
    xs::lane_reset<float, DevLds, DppXchg>(P.cfg, e_in, L, arm, lds, DppXchg());
    const int64_t e = late_index(e_in);
    cubes_store(P, e, arm, L);
    if (key && arm == 0) key[e] = (uint8_t)L.cls;
    if (obs_out) cubes_write_obs(L, e, arm, obs_out, ag_out, dg_out);
}

__global__ void k_st_compute_reward(int reward_type, const float *__restrict__ ag, const float *__restrict__ g, int64_t n, float *__restrict__ out) {
    cubes_compute_reward<Sc>(reward_type, ag, g, n, out);
}

} // namespace xd
