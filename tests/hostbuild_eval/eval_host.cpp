// Host (g++) instantiation of gym_xarm_amd/csrc/xarm_eval_core.h for the CPU-side evaluation tests ONLY (tests/test_eval_host.py,
// tests/test_eval_gpu.py).  Never loaded by the product package: gym_xarm_amd evaluates through libxarm_hip.so (xarm_k_eval.hip).
// The step kernel's per-env code runs here env by env and `remaining` is lowered by the sum of its returns, as the ballots do; the
// summary's THREADS partials are computed thread by thread and merged by the same functions.  Built with -ffp-contract=off, as the
// device unit is.
#define XARM_HOST_BUILD 1
#include "../../gym_xarm_amd/csrc/xarm_eval_core.h"

using namespace xeval;

extern "C" {

int eh_begin(const xarm_eval_layout *l, double *cur_ret, int32_t *cur_len, int32_t *count, int32_t *remaining, double *records) {
    if (layout_error(l)) return -1;
    for (int32_t i = 0; i < l->num_envs; i++) { cur_ret[i] = 0.0; cur_len[i] = 0; count[i] = 0; }
    for (int64_t i = 0; i < 3 * (int64_t)l->n_eval_episodes; i++) records[i] = 0.0;
    remaining[0] = l->n_eval_episodes;
    return 0;
}

int eh_step(const xarm_eval_layout *l, double *cur_ret, int32_t *cur_len, int32_t *count, int32_t *remaining, double *records,
            const float *rew, const uint8_t *done, const uint8_t *success, const uint8_t *keep) {
    if (layout_error(l)) return -1;
    StepArgs a;
    a.L = make_layout(*l);
    a.cur_ret = cur_ret; a.cur_len = cur_len; a.count = count; a.remaining = remaining; a.records = records;
    a.rew = rew; a.done = done; a.success = success; a.keep = keep;
    int wrote = 0;
    for (int32_t i = 0; i < a.L.E; i++) wrote += eval_step_env(a, i);
    remaining[0] -= wrote;
    return 0;
}

int eh_summary(const xarm_eval_layout *l, const int32_t *count, const double *records, double *out) {
    if (layout_error(l)) return -1;
    if (l->num_envs == 0) return 0;
    SummaryArgs a;
    a.L = make_layout(*l);
    a.count = count; a.records = records; a.out = out;
    static Part1 p1[THREADS];
    static Part2 p2[THREADS];
    for (int t = 0; t < THREADS; t++) p1[t] = summary_part1(a, t);
    const Part1 m = summary_merge1(p1);
    const double n = (double)m.n;
    for (int t = 0; t < THREADS; t++) p2[t] = summary_part2(a, t, m.sum_r / n, m.sum_l / n);
    summary_write(a, m, summary_merge2(p2));
    return 0;
}

// the closed forms, for the tests of the quotas
int eh_target(const xarm_eval_layout *l, int32_t i) { return target_of(make_layout(*l), i); }
int eh_base(const xarm_eval_layout *l, int32_t i) { return base_of(make_layout(*l), i); }

}  // extern "C"
