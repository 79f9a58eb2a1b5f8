// xarm_k_rollout.hip - the device shuffle of the PPO update.  Core: xarm_rollout_core.h.
//
// Bandwidth-trivial: 256-thread workgroups, one int32 per thread, consecutive threads on consecutive addresses, blockIdx.y is the
// epoch.  Every thread reads the device counter `calls`, and k_rollout_tick - one thread, launched behind the fill on the same
// stream - advances it, so the replays of a captured graph draw a fresh shuffle each.  Stream order is the only synchronisation;
// nothing is allocated, there is no workspace, no host read and no atomic: the same inputs give the same bits.
#include <hip/hip_runtime.h>
#include "xarm_rollout_core.h"

namespace xroll {

__global__ __launch_bounds__(THREADS) void k_perm_fill(int32_t *perm, int64_t N, int bits, uint64_t seed, const int64_t *calls) {
    const int64_t i = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    if (i >= N) return;
    const uint32_t ep = blockIdx.y;
    perm[(int64_t)ep * N + i] = perm_entry(i, N, bits, seed, ep, calls[0]);
}

__global__ void k_rollout_tick(int64_t *calls) {
    if (blockIdx.x == 0 && threadIdx.x == 0) calls[0] += 1;
}

static unsigned blocks_for(int64_t n) { return (unsigned)((n + THREADS - 1) / THREADS); }

int launch_perm_fill(int32_t *perm, int32_t n_epochs, int64_t N, uint64_t seed, int64_t *calls, void *stream) {
    k_perm_fill<<<dim3(blocks_for(N), (unsigned)n_epochs), dim3(THREADS), 0, (hipStream_t)stream>>>(perm, N, perm_bits(N), seed, calls);
    k_rollout_tick<<<dim3(1), dim3(1), 0, (hipStream_t)stream>>>(calls);
    return (int)hipGetLastError();
}

}  // namespace xroll
