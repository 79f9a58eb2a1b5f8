// xarm_k_rearrange.hip - XarmRearrange-v0 (two arms, four cubes, a goal per cube; scene: xra::Rearrange4 in xarm_rearrange_core.h).
// Part of libxarm_hip.so (gfx950); shared declarations: xarm_dev.h, shared kernel parts: xarm_cubes_dev.h, C ABI: xarm_hip.hip.
#include "xarm_cubes_dev.h"

namespace xd {

// --------------------------------------------------------------------- LDS: one copy of the object columns per env
// The core addresses 929 floats per lane (Rearrange4::LDS_FLOATS).  The first 117 (the arm's S | T | A_hh columns) are the lane's own,
// at stride WG; the other 812 (16 table slots, 6 cube/cube pairs, the clipping scratch) hold the same numbers in both lanes of an
// env - each lane computes the object rows redundantly and bit-identically, in lockstep - and are ONE copy per env at stride
// WG / 2: same-address reads broadcast, the two lanes' writes carry the same value.  117 x 64 + 812 x 32 floats = 130.75 KiB per
// wavefront of 32 envs (929 x 64 = 232 KiB would not fit a CU's 160 KiB).
struct RaLds {
    float *arm;   // + lane, column stride WG
    float *obj;   // + lane / 2, column stride WG / 2
    __device__ __forceinline__ float &operator[](int i) const { return i < xk::LDS_TBL ? arm[i * WG] : obj[(i - xk::LDS_TBL) * (WG / 2)]; }
};
constexpr int RA_LDS_FLOATS = xk::LDS_TBL * WG + xra::Rearrange4::LDS_SHARED * (WG / 2);
static_assert(RA_LDS_FLOATS * 4 <= 160 * 1024, "one wavefront must fit a CU's LDS");
__device__ __forceinline__ RaLds ra_lds(float *smem) { return RaLds{smem + threadIdx.x, smem + xk::LDS_TBL * WG + (threadIdx.x >> 1)}; }

using Sc = xra::Rearrange4;

__global__ __launch_bounds__(WG) void k_ra_init(KParams P) {
    const int64_t t = (int64_t)blockIdx.x * WG + threadIdx.x, e = t >> 1;
    const int arm = (int)(t & 1);
    if (e >= P.num_envs) return;
    xs::Lane<float, Sc> L;
    xs::lane_init<float>(P.cfg, e, L);
    cubes_store(P, e, arm, L);
}

__global__ void k_ra_class_hist(const uint8_t *__restrict__ key, int64_t n, int *__restrict__ hist) {
    __shared__ int h[Sc::NCLS];
    class_hist<Sc::NCLS>(key, n, hist, h);
}

__global__ void k_ra_class_place(const uint8_t *__restrict__ key, int64_t n, const int *__restrict__ hist, int *__restrict__ cursor,
                                 int *__restrict__ order, int group) {
    __shared__ xs::ClassLayoutN<Sc::NCLS> Y;
    __shared__ int cnt[Sc::NCLS], base[Sc::NCLS];
    class_place<Sc::NCLS>(key, n, hist, cursor, order, group, Y, cnt, base);
}

__global__ __launch_bounds__(WG) void k_ra_step(KParams P, const float *__restrict__ actions, float *__restrict__ obs_out,
                                                float *__restrict__ ag_out, float *__restrict__ dg_out,
                                                float *__restrict__ rew_out, uint8_t *__restrict__ done_out,
                                                uint8_t *__restrict__ succ_out, float *__restrict__ term_obs,
                                                int *__restrict__ done_list, int *__restrict__ done_count,
                                                const int *__restrict__ order, uint8_t *__restrict__ key) {
    __shared__ float smem[RA_LDS_FLOATS];
    const int64_t t = (int64_t)blockIdx.x * WG + threadIdx.x, slot = t >> 1;
    const int arm = (int)(t & 1);
    if (slot >= P.num_envs) return;
    const int64_t e_in = order ? (int64_t)order[slot] : slot;
    const RaLds lds = ra_lds(smem);
    xs::Lane<float, Sc> L;
    cubes_load(P, e_in, arm, L);
    const float4 a4 = reinterpret_cast<const float4 *>(actions)[e_in * 2 + arm];
    const float act[4] = {a4.x, a4.y, a4.z, a4.w};
    float reward;
    bool done, success;
    xs::lane_step<float, RaLds, DppXchg>(P.cfg, L, arm, act, reward, done, success, lds, DppXchg());
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

__global__ __launch_bounds__(WG) void k_ra_reset(KParams P, const int *__restrict__ list, const int *__restrict__ count,
                                                 float *__restrict__ obs_out, float *__restrict__ ag_out, float *__restrict__ dg_out,
                                                 uint8_t *__restrict__ key) {
    __shared__ float smem[RA_LDS_FLOATS];
    const int64_t t = (int64_t)blockIdx.x * WG + threadIdx.x, i = t >> 1;
    const int arm = (int)(t & 1);
    const int64_t n = count ? (int64_t)*count : P.num_envs;
    if (i >= n) return;
    const int64_t e_in = list ? (int64_t)list[i] : i;
    const RaLds lds = ra_lds(smem);
    xs::Lane<float, Sc> L;
    cubes_load(P, e_in, arm, L);
    xs::lane_reset<float, RaLds, DppXchg>(P.cfg, e_in, L, arm, lds, DppXchg());
    const int64_t e = late_index(e_in);
    cubes_store(P, e, arm, L);
    if (key && arm == 0) key[e] = (uint8_t)L.cls;
    if (obs_out) cubes_write_obs(L, e, arm, obs_out, ag_out, dg_out);
}

__global__ void k_ra_compute_reward(int reward_type, const float *__restrict__ ag, const float *__restrict__ g, int64_t n, float *__restrict__ out) {
    cubes_compute_reward<Sc>(reward_type, ag, g, n, out);
}

} // namespace xd
