// Host (g++) instantiation of gym_xarm_amd/csrc/xarm_replay_core.h for the CPU-side replay tests ONLY (tests/test_replay_host.py,
// tests/test_replay_gpu.py).  Never loaded by the product package: gym_xarm_amd replays through libxarm_hip.so (xarm_k_replay.hip).
// The kernels' per-env and per-row code runs here as lane 0 of a one-lane group, and the clock is advanced after each call as
// k_replay_tick does.  Built with -ffp-contract=off, as the device unit is.
#define XARM_HOST_BUILD 1
#include "../../gym_xarm_amd/csrc/xarm_replay_core.h"

using namespace xrep;

extern "C" {

int rh_record_floats(const xarm_replay_layout *l) { return layout_error(l) ? -1 : make_layout(*l).R; }

int rh_add(const xarm_replay_layout *l, float *ring, int64_t *clock, const float *obs, const float *ag, const float *dg, const float *next_obs,
           const float *next_ag, const float *act, const float *rew, const uint8_t *done, const uint8_t *timeout) {
    if (layout_error(l)) return -1;
    AddArgs a;
    a.L = make_layout(*l);
    a.ring = ring; a.clock = clock; a.obs = obs; a.ag = ag; a.dg = dg; a.next_obs = next_obs; a.next_ag = next_ag; a.act = act; a.rew = rew;
    a.done = done; a.timeout = timeout;
    for (int64_t e = 0; e < a.L.E; e++) replay_add_env(a, clock[0], e, 0, 1);
    clock[0] += 1;
    return 0;
}

int rh_sample(const xarm_replay_layout *l, const float *ring, int64_t *clock, uint64_t seed, int32_t batch, int32_t handle_timeout,
              const double *stats, double clip_obs, double eps, float *obs, float *next_obs, float *act, float *rew, float *done, float *use,
              int64_t *env, int64_t *time) {
    if (layout_error(l) || batch < 0) return -1;
    SampleArgs a;
    a.L = make_layout(*l);
    a.ring = ring; a.clock = clock; a.seed = seed; a.batch = batch; a.handle_timeout = handle_timeout != 0;
    a.stats = stats; a.clip_obs = clip_obs; a.eps = eps;
    a.obs = obs; a.next_obs = next_obs; a.act = act; a.rew = rew; a.done = done; a.use = use; a.env = env; a.time = time;
    if (batch == 0 || a.L.E == 0) return 0;
    for (int64_t b = 0; b < batch; b++) replay_write_row(a, replay_pick(a.L, clock[0], clock[1], seed, b), b, 0, 1);
    clock[1] += 1;
    return 0;
}

}  // extern "C"
