// xarm_k_her.hip - the replay kernels of the device-resident HER buffer.  Core: xarm_her_core.h.
//
// One wavefront per env (k_her_add) or per output row (k_her_sample), four of them to a workgroup.  A record is 31 (Reach) to
// 151 floats, so the 64 lanes of a wavefront move it in one to three fully coalesced passes over consecutive floats, on the
// [E, dim] / [batch, dim] side as well as on the ring side; a 16-lane row per env would save idle lanes on Reach's record only
// and cannot take the pick through readfirstlane.  The close-out walk of a finished env strides the same 64 lanes over the
// episode's entries (at most `horizon` of them).  k_her_sample computes the pick in every lane - it depends on the row alone -
// and passes it through readfirstlane, so the record addresses are scalar and the copy loops carry one vector offset.
// The clock {t, sample_calls} is read by every wavefront of the two kernels and advanced by k_her_tick, a single thread
// launched behind them on the same stream: stream order is the only synchronisation, nothing is allocated, no workspace,
// no host read - all three launches can be captured in a graph, whose replays then advance the clock themselves.
#include <hip/hip_runtime.h>
#include "xarm_her_core.h"

namespace xher {

constexpr int WAVE = 64, WAVES_PER_BLOCK = 4;

__device__ __forceinline__ int64_t uniform64(int64_t x) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)x);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)((uint64_t)x >> 32));
    return (int64_t)(((uint64_t)hi << 32) | lo);
}

__global__ __launch_bounds__(WAVE * WAVES_PER_BLOCK) void k_her_add(AddArgs a) {
    const int lane = threadIdx.x & (WAVE - 1);
    const int64_t e = (int64_t)blockIdx.x * WAVES_PER_BLOCK + (threadIdx.x >> 6);
    if (e >= a.L.E) return;                                  // wavefront-uniform
    her_add_env(a, a.clock[0], e, lane, WAVE);
}

__global__ __launch_bounds__(WAVE * WAVES_PER_BLOCK) void k_her_sample(SampleArgs a) {
    const int lane = threadIdx.x & (WAVE - 1);
    const int64_t b = (int64_t)blockIdx.x * WAVES_PER_BLOCK + (threadIdx.x >> 6);
    if (b >= a.batch) return;                                // wavefront-uniform
    Pick p = her_pick(a.L, a.ep_end, a.ep_first, a.clock[0], a.clock[1], a.seed, a.strategy, b);
    p.slot = uniform64(p.slot); p.env = uniform64(p.env); p.t_abs = uniform64(p.t_abs); p.t_goal = uniform64(p.t_goal);
    p.ok = __builtin_amdgcn_readfirstlane(p.ok);
    const int failed = her_write_row(a, p, b, lane, WAVE);
    if (failed && lane == 0) atomicAdd((unsigned long long *)a.fail_count, 1ull);
}

__global__ void k_her_tick(int64_t *clock, int which) {
    if (blockIdx.x == 0 && threadIdx.x == 0) clock[which] += 1;
}

static unsigned blocks_for(int64_t groups) { return (unsigned)((groups + WAVES_PER_BLOCK - 1) / WAVES_PER_BLOCK); }

int launch_her_add(const AddArgs &a, int64_t *clock, void *stream) {
    k_her_add<<<dim3(blocks_for(a.L.E)), dim3(WAVE * WAVES_PER_BLOCK), 0, (hipStream_t)stream>>>(a);
    k_her_tick<<<dim3(1), dim3(1), 0, (hipStream_t)stream>>>(clock, 0);
    return (int)hipGetLastError();
}

int launch_her_sample(const SampleArgs &a, int64_t *clock, void *stream) {
    k_her_sample<<<dim3(blocks_for(a.batch)), dim3(WAVE * WAVES_PER_BLOCK), 0, (hipStream_t)stream>>>(a);
    k_her_tick<<<dim3(1), dim3(1), 0, (hipStream_t)stream>>>(clock, 1);
    return (int)hipGetLastError();
}

}  // namespace xher
