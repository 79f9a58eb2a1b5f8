// xarm_k_replay.hip - the kernels of the device-resident uniform replay buffer.  Core: xarm_replay_core.h.
//
// One wavefront per env (k_replay_add) or per output row (k_replay_sample), four of them to a workgroup, as in xarm_k_her.hip: a
// record is 69 (Handover NoGoal: 2 x 29 + 8 + 3) to a few hundred floats, which the 64 lanes move in coalesced passes over
// consecutive floats on both sides.  k_replay_sample computes the pick in every lane - it depends on the row alone - and passes it
// through readfirstlane, so the record address is scalar and the copy loops carry one vector offset.  The sampled row is written
// as the learners take it: both observation rows concatenated and (with `stats`) normalised, done as float32 with the time-limit
// truncations taken out, use = 1 - so nothing stands between this launch and the learner's first one.
// The clock {t, sample_calls} is read by every wavefront of the two kernels and advanced by k_replay_tick, a single thread
// launched behind them on the same stream: stream order is the only synchronisation, nothing is allocated, no workspace, no
// atomics, no host read - all launches can be captured in a graph, whose replays then advance the clock themselves.
#include <hip/hip_runtime.h>
#include "xarm_replay_core.h"

namespace xrep {

constexpr int WAVE = 64, WAVES_PER_BLOCK = 4;

__device__ __forceinline__ int64_t uniform64(int64_t x) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)x);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)((uint64_t)x >> 32));
    return (int64_t)(((uint64_t)hi << 32) | lo);
}

__global__ __launch_bounds__(WAVE * WAVES_PER_BLOCK) void k_replay_add(AddArgs a) {
    const int lane = threadIdx.x & (WAVE - 1);
    const int64_t e = (int64_t)blockIdx.x * WAVES_PER_BLOCK + (threadIdx.x >> 6);
    if (e >= a.L.E) return;                                  // wavefront-uniform
    replay_add_env(a, a.clock[0], e, lane, WAVE);
}

__global__ __launch_bounds__(WAVE * WAVES_PER_BLOCK) void k_replay_sample(SampleArgs a) {
    const int lane = threadIdx.x & (WAVE - 1);
    const int64_t b = (int64_t)blockIdx.x * WAVES_PER_BLOCK + (threadIdx.x >> 6);
    if (b >= a.batch) return;                                // wavefront-uniform
    Pick p = replay_pick(a.L, a.clock[0], a.clock[1], a.seed, b);
    p.slot = uniform64(p.slot); p.env = uniform64(p.env); p.t_abs = uniform64(p.t_abs);
    p.ok = __builtin_amdgcn_readfirstlane(p.ok);
    replay_write_row(a, p, b, lane, WAVE);
}

__global__ void k_replay_tick(int64_t *clock, int which) {
    if (blockIdx.x == 0 && threadIdx.x == 0) clock[which] += 1;
}

static unsigned blocks_for(int64_t groups) { return (unsigned)((groups + WAVES_PER_BLOCK - 1) / WAVES_PER_BLOCK); }

int launch_replay_add(const AddArgs &a, int64_t *clock, void *stream) {
    k_replay_add<<<dim3(blocks_for(a.L.E)), dim3(WAVE * WAVES_PER_BLOCK), 0, (hipStream_t)stream>>>(a);
    k_replay_tick<<<dim3(1), dim3(1), 0, (hipStream_t)stream>>>(clock, 0);
    return (int)hipGetLastError();
}

int launch_replay_sample(const SampleArgs &a, int64_t *clock, void *stream) {
    k_replay_sample<<<dim3(blocks_for(a.batch)), dim3(WAVE * WAVES_PER_BLOCK), 0, (hipStream_t)stream>>>(a);
    k_replay_tick<<<dim3(1), dim3(1), 0, (hipStream_t)stream>>>(clock, 1);
    return (int)hipGetLastError();
}

}  // namespace xrep
