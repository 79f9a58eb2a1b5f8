// Stand-alone driver of the host build of csrc/xarm_norm_core.h for the sanitizer run of tests/test_norm_host.py
// (g++ -fsanitize=address,undefined; run directly, never loaded into python).  It plays the scripted stream of the CPU tests -
// a reset, then 30 steps with env e finishing every (3, 4, 5, 5, 2, 4, 1)[e % 7] calls and a keep mask that drops every fifth
// row on every third call - on exactly sized heap arrays, for every batch size and row width the tests use plus an
// update-off pass, and checks the counters the script fixes.  Exit status 0 and "norm_main ok" when nothing was flagged.
#include <cstdio>
#include <cstdlib>
#include "norm_host.cpp"

static uint32_t lcg(uint32_t &s) { s = s * 1664525u + 1013904223u; return s; }
static float uni(uint32_t &s) { return ((float)(lcg(s) >> 8) / 8388608.0f - 1.0f) * 4.0f; }   // [-4, 4)

static int run_case(int E, int od, int gd, int update) {
    static const int lens[7] = {3, 4, 5, 5, 2, 4, 1};
    const int D = od + 2 * gd, cap = E;                    // the smallest capacity the calls accept: the ring wraps
    xarm_norm_layout l = {E, od, gd, cap};
    xarm_norm_params p = {10.0, 10.0, 1e-8, 0.99f, 0.0f, update};
    const int64_t wb = nh_work_bytes(&l);
    if (wb <= 0) return 1;
    std::vector<double> stats(2 * D + 4, 0.0);
    for (int j = 0; j < D; j++) stats[D + j] = 1.0;
    stats[2 * D + 1] = 1.0; stats[2 * D + 2] = stats[2 * D + 3] = 1e-4;
    std::vector<float> ret(E, 0.f), ep_ret(E, 0.f), ep_len(E, 0.f), ring((size_t)cap * 3, 0.f), obs((size_t)E * od),
        ag((size_t)E * gd + 1), dg((size_t)E * gd + 1), rew(E), nobs((size_t)E * D), nrew(E);
    std::vector<uint8_t> done(E), keep(E), work((size_t)wb, 0xFF);
    int64_t n = 0, expect_n = 0;
    uint32_t s = 12345u + (uint32_t)E * 31u + (uint32_t)D;
    const float *agp = gd ? ag.data() : nullptr, *dgp = gd ? dg.data() : nullptr;
    for (auto &x : obs) x = uni(s);
    for (auto &x : ag) x = uni(s);
    for (auto &x : dg) x = uni(s);
    if (nh_obs(&l, &p, stats.data(), ret.data(), work.data(), obs.data(), agp, dgp, 1, nobs.data()) != 0) return 2;
    for (int t = 1; t <= 30; t++) {
        for (auto &x : obs) x = uni(s);
        for (auto &x : ag) x = uni(s);
        for (auto &x : dg) x = uni(s);
        for (int e = 0; e < E; e++) {
            rew[e] = uni(s);
            done[e] = t % lens[e % 7] == 0;
            keep[e] = e % 5 != 4;
            expect_n += done[e];
        }
        p.t_seconds = (float)t;
        std::fill(work.begin(), work.end(), 0xFF);
        if (nh_step(&l, &p, stats.data(), ret.data(), ep_ret.data(), ep_len.data(), ring.data(), &n, work.data(), obs.data(), agp, dgp,
                    rew.data(), done.data(), t % 3 == 2 ? keep.data() : nullptr, nobs.data(), nrew.data()) != 0) return 3;
        for (size_t i = 0; i < nobs.size(); i++)
            if (!(nobs[i] >= -10.0f && nobs[i] <= 10.0f)) return 4;
        for (int e = 0; e < E; e++)
            if (!(nrew[e] >= -10.0f && nrew[e] <= 10.0f)) return 5;
    }
    if (n != expect_n) return 6;
    const double count = stats[2 * D + 2];
    if (update ? !(count > 1.0) : count != 1e-4) return 7;
    return 0;
}

int main() {
    static const int Es[] = {1, 127, 128, 129, 1000}, widths[][2] = {{8, 3}, {24, 3}, {29, 0}, {68, 12}};
    for (int E : Es)
        for (auto &w : widths)
            for (int update = 1; update >= 0; update--) {
                const int rc = run_case(E, w[0], w[1], update);
                if (rc) {
                    printf("norm_main FAILED: E %d widths %d %d update %d -> %d\n", E, w[0], w[1], update, rc);
                    return 1;
                }
            }
    printf("norm_main ok\n");
    return 0;
}
