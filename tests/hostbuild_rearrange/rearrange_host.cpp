// Host (g++) instantiation of the cube core (gym_xarm_amd/csrc/xarm_stack_core.h) for the scene xra::Rearrange4
// (xarm_rearrange_core.h), for the CPU-side tests ONLY (tests/rearrange_host.py).  It lives under tests/ and is never loaded by the
// product package.  The lane-pair runner is tests/hostbuild/cube_pair_host.h, shared with StackTower's host build.
#define XARM_HOST_BUILD 1
#include "../../gym_xarm_amd/csrc/xarm_rearrange_core.h"
#include "../hostbuild/cube_pair_host.h"

using Sc = xra::Rearrange4;

extern "C" {
int ra_dims(int32_t *d) { d[0] = Sc::STATE_DIM; d[1] = Sc::OBS_DIM; d[2] = Sc::GOAL_DIM; d[3] = Sc::LDS_FLOATS; d[4] = Sc::NCLS; return 0; }
void ra_init(int f32, uint64_t seed, int64_t off, int rt, int64_t E, double *state) {
    auto c = cubes::cfg(seed, off, rt);
    if (f32) cubes::init<float, Sc>(c, E, state); else cubes::init<double, Sc>(c, E, state);
}
// key (optional): the row-set class of each env's last substep
void ra_step(int f32, uint64_t seed, int64_t off, int rt, int64_t E, double *state, const double *act, double *obs, double *ag, double *dg,
             double *rew, uint8_t *done, uint8_t *succ, uint8_t *key) {
    auto c = cubes::cfg(seed, off, rt);
    if (f32) cubes::run<float, Sc>(0, c, E, state, act, 0, obs, ag, dg, rew, done, succ, key); else cubes::run<double, Sc>(0, c, E, state, act, 0, obs, ag, dg, rew, done, succ, key);
}
void ra_reset(int f32, uint64_t seed, int64_t off, int rt, int64_t E, double *state, const uint8_t *mask, double *obs, double *ag, double *dg, uint8_t *key) {
    auto c = cubes::cfg(seed, off, rt);
    if (f32) cubes::run<float, Sc>(1, c, E, state, 0, mask, obs, ag, dg, 0, 0, 0, key); else cubes::run<double, Sc>(1, c, E, state, 0, mask, obs, ag, dg, 0, 0, 0, key);
}
// tests only: one bare tick (15 substeps towards the stored motor targets) of every row - the reset's tick without its draws
void ra_tick(int f32, int64_t E, double *state, uint8_t *key) {
    auto c = cubes::cfg(0, 0, 0);
    if (f32) cubes::run<float, Sc>(2, c, E, state, 0, 0, 0, 0, 0, 0, 0, 0, key); else cubes::run<double, Sc>(2, c, E, state, 0, 0, 0, 0, 0, 0, 0, 0, key);
}
// tests only: the 16 arm entries of the observation (xs::arm_obs of both arms) of every row, float64
void ra_arm_obs(int64_t E, const double *state, double *out) {
    for (int64_t e = 0; e < E; e++)
        for (int a = 0; a < 2; a++) {
            xs::Lane<double, Sc> L; double o8[8];
            cubes::load(state + e * Sc::STATE_DIM, a, L);
            xs::arm_obs(L, a, o8);
            for (int k = 0; k < 8; k++) out[e * 16 + 8 * a + k] = o8[k];
        }
}
// the kernel's reward arithmetic (k_ra_compute_reward) over n rows of 12, in float32
void ra_compute_reward(int rt, const float *ag, const float *g, int64_t n, float *out) {
    for (int64_t i = 0; i < n; i++) {
        float d2 = 0.f;
        for (int k = 0; k < 12; k++) { const float d = ag[i * 12 + k] - g[i * 12 + k]; d2 += d * d; }
        const float d = sqrtf(d2);
        out[i] = rt == 0 ? (d > (float)xm::RA_DISTANCE_THRESHOLD ? -1.f : 0.f) : -d;
    }
}
int ra_class_order(const uint8_t *key, int64_t n, int group, int32_t *order) { return cubes::class_order<Sc>(key, n, group, order); }
}
