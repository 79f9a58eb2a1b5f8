// Test-side helpers of the host (g++) builds: the LDS accessor, the lane-pair emulation (the two lanes of an environment run
// as two host threads, the lane-pair exchange is a slot + spin barrier) and the runner of the two-arm cube scenes, templated
// on the scene description (xs::Tower3, xra::Rearrange4; core: gym_xarm_amd/csrc/xarm_stack_core.h).  Included by
// tests/hostbuild/xarm_host.cpp and tests/hostbuild_rearrange/rearrange_host.cpp after XARM_HOST_BUILD is defined.
// Rebuild checks: tests/rearrange_host.py lists this header; the check of libxarm_host.so (tests/conftest.py, a fixed list)
// does not see it - after an edit here, touch xarm_host.cpp or delete tests/hostbuild/libxarm_host.so.
#pragma once
#include "../../gym_xarm_amd/csrc/xarm_stack_core.h"
#include <atomic>
#include <pthread.h>
#include <sched.h>
#include <string.h>

namespace {
template <typename T> struct HostLds {
    T *base;
    T &operator[](int i) const { return base[i]; }
};
// two-party sense-reversing spin barrier: the lane pair exchanges thousands of values per tick, and a futex-based
// pthread barrier made the emulation ~50x slower than the arithmetic it synchronises
struct SpinBarrier {
    std::atomic<int> count{0}, gen{0};
    void wait() {
        const int g = gen.load(std::memory_order_acquire);
        if (count.fetch_add(1, std::memory_order_acq_rel) + 1 == 2) {
            count.store(0, std::memory_order_relaxed);
            gen.store(g + 1, std::memory_order_release);
        } else {
            int spins = 0;
            while (gen.load(std::memory_order_acquire) == g)
                if (++spins > 4096) { sched_yield(); spins = 0; }
        }
    }
};
struct PairShared { SpinBarrier bar; double slot[2]; };
struct PairXchg {
    PairShared *sh; int arm;
    template <typename T> T get(int src, T v) const {
        sh->slot[arm] = (double)v;
        sh->bar.wait();
        T r = (T)sh->slot[src];
        sh->bar.wait();
        return r;
    }
    template <typename T> T from0(T v) const { return get(0, v); }
    template <typename T> T from1(T v) const { return get(1, v); }
    template <typename T> T partner(T v) const { return get(1 - arm, v); }
};

// ---- the cube scenes: rows are float64 state rows [E, Sc::STATE_DIM]; each lane keeps its own copy of the object columns
// (Rearrange's device kernels share them between the two lanes of an env: they hold the same numbers)
namespace cubes {
template <typename T, typename Sc> void load(const double *r, int arm, xs::Lane<T, Sc> &L) {
    for (int i = 0; i < 9; i++) { L.q[i] = (T)r[Sc::K_Q + 9 * arm + i]; L.qd[i] = (T)r[Sc::K_QD + 9 * arm + i]; L.qt[i] = (T)r[Sc::K_QT + 9 * arm + i]; }
    for (int o = 0; o < Sc::NOBJ; o++) {
        for (int k = 0; k < 3; k++) { L.bp[o][k] = (T)r[Sc::K_BP + 3 * o + k]; L.bv[o][k] = (T)r[Sc::K_BV + 3 * o + k]; L.bw[o][k] = (T)r[Sc::K_BW + 3 * o + k]; L.goal[o][k] = (T)r[Sc::K_GOAL + 3 * o + k]; }
        for (int k = 0; k < 4; k++) L.bq[o][k] = (T)r[Sc::K_BQ + 4 * o + k];
        for (int k = 0; k < 8; k++) L.lam_t[o][k] = (T)r[Sc::K_LT + 8 * o + k];
    }
    for (int k = 0; k < 4; k++) L.lam_p[k] = (T)r[Sc::K_LP + 4 * arm + k];
    L.steps = (T)r[Sc::K_STEPS]; L.episode = (T)r[Sc::K_EPISODE];
    L.cls = 0;
}
template <typename T, typename Sc> void store(const xs::Lane<T, Sc> &L, int arm, double *r) {
    for (int i = 0; i < 9; i++) { r[Sc::K_Q + 9 * arm + i] = L.q[i]; r[Sc::K_QD + 9 * arm + i] = L.qd[i]; r[Sc::K_QT + 9 * arm + i] = L.qt[i]; }
    for (int k = 0; k < 4; k++) r[Sc::K_LP + 4 * arm + k] = L.lam_p[k];
    if (arm == 0) {
        for (int o = 0; o < Sc::NOBJ; o++) {
            for (int k = 0; k < 3; k++) { r[Sc::K_BP + 3 * o + k] = L.bp[o][k]; r[Sc::K_BV + 3 * o + k] = L.bv[o][k]; r[Sc::K_BW + 3 * o + k] = L.bw[o][k]; r[Sc::K_GOAL + 3 * o + k] = L.goal[o][k]; }
            for (int k = 0; k < 4; k++) r[Sc::K_BQ + 4 * o + k] = L.bq[o][k];
            for (int k = 0; k < 8; k++) r[Sc::K_LT + 8 * o + k] = L.lam_t[o][k];
        }
        r[Sc::K_STEPS] = L.steps; r[Sc::K_EPISODE] = L.episode;
    }
}
inline xk::EnvCfg cfg(uint64_t seed, int64_t off, int rt) { xk::EnvCfg c; memset(&c, 0, sizeof c); c.seed = seed; c.env_id_offset = off; c.reward_type = rt; return c; }
template <typename T, typename Sc> void init(const xk::EnvCfg &c, int64_t E, double *state) {
    for (int64_t e = 0; e < E; e++) for (int a = 1; a >= 0; a--) { xs::Lane<T, Sc> L; xs::lane_init<T>(c, e, L); store(L, a, state + e * Sc::STATE_DIM); }
}
// mode 0: step, 1: reset of the envs with mask[e] != 0 (all without a mask), 2 (tests only): one bare xs::tick of every env,
// which writes state and key and no other output; key (optional): the row-set class of the last substep
struct Job {
    int mode; xk::EnvCfg cfg; int64_t E; double *state; const double *act; const uint8_t *mask;
    double *obs, *ag, *dg, *rew; uint8_t *done, *succ, *key; PairShared *sh; int arm;
};
template <typename T, typename Sc> void *thread(void *p) {
    Job &J = *(Job *)p;
    PairXchg x{J.sh, J.arm};
    for (int64_t e = 0; e < J.E; e++) {
        if (J.mode == 1 && J.mask && !J.mask[e]) continue;
        xs::Lane<T, Sc> L; T lds[Sc::LDS_FLOATS]; HostLds<T> hl{lds};
        load(J.state + e * Sc::STATE_DIM, J.arm, L);
        T r = 0; bool d = false, su = false;
        if (J.mode == 0) {
            T a[4]; for (int k = 0; k < 4; k++) a[k] = (T)J.act[e * 8 + 4 * J.arm + k];
            xs::lane_step<T>(J.cfg, L, J.arm, a, r, d, su, hl, x);
        } else if (J.mode == 1) xs::lane_reset<T>(J.cfg, e, L, J.arm, hl, x);
        else {
            xs::tick<T>(L, hl, J.arm, x);
            J.sh->bar.wait();
            store(L, J.arm, J.state + e * Sc::STATE_DIM);
            if (J.arm == 0 && J.key) J.key[e] = (uint8_t)L.cls;
            J.sh->bar.wait();
            continue;
        }
        T o8[8];
        xs::arm_obs(L, J.arm, o8);
        J.sh->bar.wait();
        store(L, J.arm, J.state + e * Sc::STATE_DIM);
        double *o = J.obs + e * Sc::OBS_DIM;
        for (int k = 0; k < 8; k++) o[Sc::O_ARM + 8 * J.arm + k] = o8[k];
        if (J.arm == 0) {
            for (int ob = 0; ob < Sc::NOBJ; ob++) {
                for (int k = 0; k < 3; k++) {
                    o[Sc::O_BP + 3 * ob + k] = L.bp[ob][k]; o[Sc::O_BV + 3 * ob + k] = L.bv[ob][k]; o[Sc::O_BW + 3 * ob + k] = L.bw[ob][k];
                    J.ag[e * Sc::GOAL_DIM + 3 * ob + k] = L.bp[ob][k]; J.dg[e * Sc::GOAL_DIM + 3 * ob + k] = L.goal[ob][k];
                }
                for (int k = 0; k < 4; k++) o[Sc::O_BQ + 4 * ob + k] = L.bq[ob][k];
            }
            if (J.mode == 0) { J.rew[e] = r; J.done[e] = d; J.succ[e] = su; }
            if (J.key) J.key[e] = (uint8_t)L.cls;
        }
        J.sh->bar.wait();
    }
    return 0;
}
template <typename T, typename Sc> void run(int mode, const xk::EnvCfg &cfg, int64_t E, double *state, const double *act, const uint8_t *mask,
                                            double *obs, double *ag, double *dg, double *rew, uint8_t *done, uint8_t *succ, uint8_t *key) {
    PairShared sh;
    Job j[2];
    pthread_t th[2];
    for (int a = 0; a < 2; a++) { j[a] = Job{mode, cfg, E, state, act, mask, obs, ag, dg, rew, done, succ, key, &sh, a}; pthread_create(&th[a], 0, thread<T, Sc>, &j[a]); }
    for (int a = 0; a < 2; a++) pthread_join(th[a], 0);
}
// class-homogeneous visiting order (xs::class_layout / class_slot as the class-order kernels run them, with the envs arriving in
// index order): order[slot] = env; 1 when the classes are wavefront-aligned, 0 when not, -1 on an invalid permutation
template <typename Sc> int class_order(const uint8_t *key, int64_t n, int group, int32_t *order) {
    int hist[Sc::NCLS] = {0}, cursor[Sc::NCLS] = {0};
    xs::ClassLayoutN<Sc::NCLS> Y;
    for (int64_t e = 0; e < n; e++) hist[key[e] & (Sc::NCLS - 1)]++;
    xs::class_layout(hist, group, Y);
    for (int64_t e = 0; e < n; e++) order[e] = -1;
    for (int64_t e = 0; e < n; e++) {
        const int c = key[e] & (Sc::NCLS - 1);
        const int slot = xs::class_slot(Y, c, cursor[c]++);
        if (slot < 0 || slot >= n || order[slot] != -1) return -1;
        order[slot] = (int32_t)e;
    }
    return Y.aligned ? 1 : 0;
}
}
}
