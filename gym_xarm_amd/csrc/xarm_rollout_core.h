// xarm_rollout_core.h - a device shuffle for the PPO update's minibatch order: one entry of one permutation.  The kernel
// is in xarm_k_rollout.hip; like the HER and normaliser cores this also compiles for the host (g++ -DXARM_HOST_BUILD,
// tests/hostbuild_rollout/) and that build is the checker: the shuffle is integer arithmetic, so the host build and the device agree
// bit for bit.  No atomics.
//
// perm_entry: entry i of epoch ep of the shuffle drawn at counter value `calls` - a keyed bijection of [0, 2^b), b = max(8,
//   ceil(log2 N)), walked until it lands below N (cycle walking: the restriction of a permutation of the domain to [0, N) is a
//   permutation of [0, N), and the walk from i < N returns below N before it returns to i).  The bijection is an alternating
//   unbalanced Feistel network of PERM_ROUNDS rounds over the low lb = b / 2 and the high hb = b - lb bits: an even round x-ors
//   into the low half a word of Philox(seed; high half, round | epoch << 8, calls) masked to lb bits, an odd round x-ors into the
//   high half a word keyed by the low half.  Any round function gives a bijection; Philox makes the eight rounds' functions
//   independent across rounds, epochs and calls.  The floor of 8 bits keeps the halves at four bits or more: on a domain of 8 or
//   16 values the network's permutations are visibly non-uniform (tests/test_rollout_host.py, the uniformity test).
#pragma once
#include <stdint.h>
#include "../../include/xarm_hip.h"
#include "xarm_core.h"

namespace xroll {

constexpr uint32_t PERM_TAG = 0x5045524Du;   // c3 of every draw: keeps the stream apart from the envs', the replay's and the policy's
constexpr int PERM_ROUNDS = 8;
constexpr int PERM_MIN_BITS = 8;
constexpr int THREADS = 256;                 // the fill kernel's workgroup

// null when the call is usable, else what is wrong with it
inline const char *perm_error(int32_t n_epochs, int64_t N) {
    if (N < 0 || N >= ((int64_t)1 << 31)) return "N must lie in [0, 2^31)";
    if (n_epochs < 1 || n_epochs > 255) return "n_epochs must lie in [1, 255]";
    return nullptr;
}

inline int perm_bits(int64_t N) {   // max(PERM_MIN_BITS, ceil(log2 N)), N < 2^31
    int b = PERM_MIN_BITS;
    while (((int64_t)1 << b) < N) b++;
    return b;
}

XARM_HD uint32_t perm_encipher(uint32_t x, int bits, uint64_t seed, uint32_t epoch, int64_t calls) {
    const int lb = bits >> 1, hb = bits - lb;
    const uint32_t lmask = (1u << lb) - 1u, hmask = (1u << hb) - 1u;
    uint32_t lo = x & lmask, hi = x >> lb;
    const uint32_t c2 = (uint32_t)calls, c3 = PERM_TAG + (uint32_t)((uint64_t)calls >> 32);
    for (int r = 0; r < PERM_ROUNDS; r++) {
        uint32_t o[4];
        const uint32_t c1 = (uint32_t)r | (epoch << 8);
        if ((r & 1) == 0) {
            xk::philox(seed, hi, c1, c2, c3, o);
            lo ^= o[0] & lmask;
        } else {
            xk::philox(seed, lo, c1, c2, c3, o);
            hi ^= o[0] & hmask;
        }
    }
    return (hi << lb) | lo;
}

XARM_HD int32_t perm_entry(int64_t i, int64_t N, int bits, uint64_t seed, uint32_t epoch, int64_t calls) {
    if (N <= 1) return 0;
    uint32_t x = (uint32_t)i;
    do {
        x = perm_encipher(x, bits, seed, epoch, calls);
    } while ((int64_t)x >= N);
    return (int32_t)x;
}

#if defined(__HIPCC__) && !defined(XARM_HOST_BUILD)
// k_perm_fill + k_rollout_tick on `stream` (xarm_k_rollout.hip); returns the launches' hipError_t
int launch_perm_fill(int32_t *perm, int32_t n_epochs, int64_t N, uint64_t seed, int64_t *calls, void *stream);
#endif

}  // namespace xroll
