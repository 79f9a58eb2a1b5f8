// Stand-alone driver of the host build of csrc/xarm_policy_core.h for the sanitizer run of tests/test_policy_host.py
// (g++ -fsanitize=address,undefined; run directly, never loaded into python).  Every batch size and row width of the CPU tests,
// act_dim 1, 4, 8 and 16, with and without frozen statistics, stochastic and deterministic, with and without logp / value, on
// exactly sized heap arrays (so that a read or write one element past a row, a weight matrix or an output is flagged).  Checks
// that every output element was written, that env_action is the clamp of action and that `calls` counted the stochastic calls.
// Exit status 0 and "policy_main ok" when nothing was flagged.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "policy_host.cpp"

static uint32_t lcg(uint32_t &s) { s = s * 1664525u + 1013904223u; return s; }
static float uni(uint32_t &s, float lo, float hi) { return lo + (hi - lo) * ((float)(lcg(s) >> 8) / 16777216.0f); }

// 16-byte aligned, exactly sized
struct Buf {
    float *p; size_t n;
    explicit Buf(size_t n_) : p(nullptr), n(n_) { if (posix_memalign((void **)&p, 16, (n ? n : 1) * sizeof(float))) abort(); }
    ~Buf() { free(p); }
    void fill(uint32_t &s, float lo, float hi) { for (size_t i = 0; i < n; i++) p[i] = uni(s, lo, hi); }
    void nan() { for (size_t i = 0; i < n; i++) p[i] = NAN; }
};

static int run_case(int E, int od, int gd, int A, int with_stats, int det, int with_opt) {
    const int D = od + 2 * gd;
    xarm_policy_layout l = {E, od, gd, A, 64, 1000};
    xarm_policy_params p = {7u, 10.0, 1e-8, det};
    uint32_t s = 999u + (uint32_t)E * 13u + (uint32_t)D * 7u + (uint32_t)A;
    const float k1 = 1.0f / std::sqrt((float)D);
    Buf pw1((size_t)64 * D), pb1(64), pw2(64 * 64), pb2(64), pw3((size_t)A * 64), pb3(A), vw1((size_t)64 * D), vb1(64), vw2(64 * 64), vb2(64),
        vw3(64), vb3(1), ls(A), obs((size_t)E * od), ag((size_t)E * gd), dg((size_t)E * gd), act((size_t)E * A), env((size_t)E * A), lp(E), val(E);
    pw1.fill(s, -k1, k1); pb1.fill(s, -k1, k1); vw1.fill(s, -k1, k1); vb1.fill(s, -k1, k1);
    for (Buf *b : {&pw2, &pb2, &pw3, &pb3, &vw2, &vb2, &vw3, &vb3}) b->fill(s, -0.125f, 0.125f);
    ls.fill(s, -2.0f, 0.5f);
    obs.fill(s, -10.f, 10.f); ag.fill(s, -10.f, 10.f); dg.fill(s, -10.f, 10.f);
    std::vector<double> stats(2 * D + 4, 0.0);
    for (int j = 0; j < D; j++) { stats[j] = uni(s, -1.f, 1.f); stats[D + j] = uni(s, 0.5f, 2.f); }
    xarm_policy_weights w = {pw1.p, pb1.p, pw2.p, pb2.p, pw3.p, pb3.p, vw1.p, vb1.p, vw2.p, vb2.p, vw3.p, vb3.p, ls.p};
    int64_t calls = 0;
    for (int k = 0; k < 2; k++) {
        act.nan(); env.nan(); lp.nan(); val.nan();
        if (ph_act(&l, &p, &w, with_stats ? stats.data() : nullptr, &calls, obs.p, gd ? ag.p : nullptr, gd ? dg.p : nullptr, act.p, env.p,
                   with_opt ? lp.p : nullptr, with_opt ? val.p : nullptr) != 0) return 1;
        for (size_t i = 0; i < act.n; i++) {
            if (!std::isfinite(act.p[i])) return 2;
            const float c = act.p[i] < -1.f ? -1.f : (act.p[i] > 1.f ? 1.f : act.p[i]);
            if (env.p[i] != c) return 3;
        }
        for (int e = 0; e < E; e++)
            if (with_opt ? !(std::isfinite(lp.p[e]) && std::isfinite(val.p[e])) : !(std::isnan(lp.p[e]) && std::isnan(val.p[e]))) return 4;
    }
    if (calls != (det ? 0 : 2)) return 5;
    return 0;
}

int main() {
    static const int Es[] = {1, 31, 32, 33, 63, 64, 65, 1000}, widths[][2] = {{8, 3}, {24, 3}, {29, 0}, {68, 12}, {96, 0}}, As[] = {1, 4, 8, 16};
    for (int E : Es)
        for (auto &wd : widths)
            for (int A : As)
                for (int m = 0; m < 8; m++) {
                    if (E != 1 && E != 33 && m != 0 && m != 7) continue;                // every mode at two sizes, two modes at the others
                    if (E == 1000 && (wd[0] != 68 || A != 8)) continue;                 // the large batch at one width
                    const int rc = run_case(E, wd[0], wd[1], A, m & 1, (m >> 1) & 1, (m >> 2) & 1 ? 0 : 1);
                    if (rc) {
                        printf("policy_main FAILED: E %d widths %d %d act %d mode %d -> %d\n", E, wd[0], wd[1], A, m, rc);
                        return 1;
                    }
                }
    printf("policy_main ok\n");
    return 0;
}
