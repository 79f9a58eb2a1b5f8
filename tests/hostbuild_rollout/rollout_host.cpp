// Host (g++) instantiation of gym_xarm_amd/csrc/xarm_rollout_core.h for the CPU-side tests ONLY (tests/test_rollout_host.py,
// tests/test_rollout_gpu.py).  Never loaded by the product package: gym_xarm_amd shuffles through libxarm_hip.so
// (xarm_k_rollout.hip).  The kernel's per-entry code runs here in index order, and the counter is advanced after the call as the tick
// launch does.
#define XARM_HOST_BUILD 1
#include "../../gym_xarm_amd/csrc/xarm_rollout_core.h"

using namespace xroll;

extern "C" {

int rh_perm_bits(int64_t N) { return perm_error(1, N) ? -1 : perm_bits(N); }

int rh_perm_fill(int32_t *perm, int32_t n_epochs, int64_t N, uint64_t seed, int64_t *calls) {
    if (perm_error(n_epochs, N)) return -1;
    if (N == 0) return 0;
    if (!perm || !calls) return -1;
    const int bits = perm_bits(N);
    for (int32_t ep = 0; ep < n_epochs; ep++)
        for (int64_t i = 0; i < N; i++) perm[(int64_t)ep * N + i] = perm_entry(i, N, bits, seed, (uint32_t)ep, calls[0]);
    calls[0] += 1;
    return 0;
}

}  // extern "C"
