// Host (g++) instantiation of gym_xarm_amd/csrc/xarm_her_core.h for the CPU-side replay tests ONLY (tests/test_her_device_host.py,
// tests/test_her_device_gpu.py).  Never loaded by the product package: gym_xarm_amd replays through libxarm_hip.so (xarm_k_her.hip).
// The kernels' per-env and per-row code runs here as lane 0 of a one-lane group, and the clock is advanced after each call as
// k_her_tick does.
#define XARM_HOST_BUILD 1
#include "../../gym_xarm_amd/csrc/xarm_her_core.h"

using namespace xher;

extern "C" {

int hh_record_floats(const xarm_her_layout *l) { return layout_error(l) ? -1 : make_layout(*l).R; }
int hh_max_tries(void) { return XARM_HER_MAX_TRIES; }

int hh_add(const xarm_her_layout *l, float *ring, int64_t *ep_end, int64_t *ep_first, int64_t *ep_start, int64_t *clock, const float *obs,
           const float *next_obs, const float *ag, const float *next_ag, const float *dg, const float *act, const float *rew,
           const uint8_t *done) {
    if (layout_error(l)) return -1;
    AddArgs a;
    a.L = make_layout(*l);
    a.ring = ring; a.ep_end = ep_end; a.ep_first = ep_first; a.ep_start = ep_start; a.clock = clock;
    a.obs = obs; a.next_obs = next_obs; a.ag = ag; a.next_ag = next_ag; a.dg = dg; a.act = act; a.rew = rew; a.done = done;
    for (int64_t e = 0; e < a.L.E; e++) her_add_env(a, clock[0], e, 0, 1);
    clock[0] += 1;
    return 0;
}

int hh_sample(const xarm_her_layout *l, const float *ring, const int64_t *ep_end, const int64_t *ep_first, int64_t *clock, uint64_t seed,
              int32_t strategy, int32_t batch, int32_t n_her, float *obs, float *next_obs, float *ag, float *next_ag, float *goal,
              float *act, float *rew, uint8_t *done, int64_t *env, int64_t *time, int64_t *goal_time, uint8_t *ok, int64_t *fail_count) {
    if (layout_error(l) || batch < 0 || n_her < 0 || n_her > batch || strategy < 0 || strategy > 2) return -1;
    SampleArgs a;
    a.L = make_layout(*l);
    a.ring = ring; a.ep_end = ep_end; a.ep_first = ep_first; a.clock = clock; a.seed = seed;
    a.strategy = strategy; a.batch = batch; a.n_her = n_her;
    a.obs = obs; a.next_obs = next_obs; a.ag = ag; a.next_ag = next_ag; a.goal = goal; a.act = act; a.rew = rew;
    a.done = done; a.ok = ok; a.env = env; a.time = time; a.goal_time = goal_time; a.fail_count = fail_count;
    if (batch == 0 || a.L.E == 0) return 0;
    for (int64_t b = 0; b < batch; b++) {
        const Pick p = her_pick(a.L, ep_end, ep_first, clock[0], clock[1], seed, strategy, b);
        *fail_count += her_write_row(a, p, b, 0, 1);
    }
    clock[1] += 1;
    return 0;
}

}  // extern "C"
