// Stand-alone driver of the host build of csrc/xarm_acw_core.h and csrc/xarm_ppow_core.h for the sanitizer run of tests/test_ppow_host.py
// (g++ -fsanitize=address,undefined; run directly, never loaded into python).  One update and one act call at (29, 1, 192, 3, tanh), 5 x 13
// rows, two epochs of two minibatches (33 + 32) with a use mask, out-of-range perm entries and every optional output, then the same
// update with old_logp supplied, on exactly sized heap arrays (so that a read or write one element past a row, a tensor, perm, the
// workspace or an output is flagged).  Checks that every requested output element was written, that parameters and Adam's state stay
// finite and that `step` advanced by the number of optimiser steps.  Exit status 0 and "ppow_main ok" when nothing was flagged.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "ppow_host.cpp"

static uint32_t lcg(uint32_t &s) { s = s * 1664525u + 1013904223u; return s; }
static float uni(uint32_t &s, float lo, float hi) { return lo + (hi - lo) * ((float)(lcg(s) >> 8) / 16777216.0f); }

// 16-byte aligned, exactly sized
struct Buf {
    float *p; size_t n;
    explicit Buf(size_t n_) : p(nullptr), n(n_) { if (posix_memalign((void **)&p, 16, (n ? n : 1) * sizeof(float))) abort(); memset(p, 0, (n ? n : 1) * sizeof(float)); }
    ~Buf() { free(p); }
    void fill(uint32_t &s, float lo, float hi) { for (size_t i = 0; i < n; i++) p[i] = uni(s, lo, hi); }
    void nan() { for (size_t i = 0; i < n; i++) p[i] = NAN; }
    bool finite() const { for (size_t i = 0; i < n; i++) if (!std::isfinite(p[i])) return false; return true; }
};

int main() {
    const int T = 5, E = 13, D = 29, A = 1, H = 192, L = 3, epochs = 2, batch = 33;
    const size_t N = (size_t)T * E;
    xarm_ppow_layout l = {E, T, D, A, H, L, XARM_SACW_TANH, epochs, batch};
    xarm_ppo_params p = {0.99, 0.95, 0.2, 3e-4, 0.9, 0.999, 1e-5, 0.5, 0.01, 0.5, 1};
    uint32_t s = 4242u;
    int64_t geo[48];
    pwh_geometry(&l, geo);
    const int64_t P = geo[0], S = geo[3], NT = geo[7];
    if (S != 4 || NT != 17) { printf("unexpected geometry\n"); return 1; }
    std::vector<Buf *> w, m, v;
    xarm_acw_weights ws = {}, ms = {}, vs = {};
    for (int i = 0; i < NT; i++) {
        const size_t n = (size_t)(geo[25 + i + 1] - geo[25 + i]);
        w.push_back(new Buf(n)); m.push_back(new Buf(n)); v.push_back(new Buf(n));
        w[i]->fill(s, i == NT - 1 ? -1.2f : -0.08f, i == NT - 1 ? -0.3f : 0.08f);
        m[i]->fill(s, -0.01f, 0.01f);
        v[i]->fill(s, 0.0f, 0.01f);
        const float **slot[3] = {i == NT - 1 ? &ws.log_std : (i < 8 ? &ws.pi[i] : &ws.vf[i - 8]), i == NT - 1 ? &ms.log_std : (i < 8 ? &ms.pi[i] : &ms.vf[i - 8]),
                                 i == NT - 1 ? &vs.log_std : (i < 8 ? &vs.pi[i] : &vs.vf[i - 8])};
        *slot[0] = w[i]->p; *slot[1] = m[i]->p; *slot[2] = v[i]->p;
    }
    Buf obs(N * D), act(N * A), rew(N), done(N), use(N), last((size_t)E * D), olp(N), adv(N), ret(N), grad((size_t)P), stats((size_t)S * 8);
    Buf work((size_t)pwh_workspace_bytes(&l) / 4);
    obs.fill(s, -2.5f, 2.5f); act.fill(s, -1.f, 1.f); rew.fill(s, -1.f, 1.f); last.fill(s, -2.5f, 2.5f); olp.fill(s, -3.f, 0.f);
    for (size_t i = 0; i < N; i++) { done.p[i] = (lcg(s) >> 8) % 5 == 0 ? 1.0f : 0.0f; use.p[i] = (lcg(s) >> 8) % 10 == 0 ? 0.0f : 1.0f; }
    int32_t *perm = (int32_t *)malloc(sizeof(int32_t) * epochs * N);
    if (!perm) abort();
    for (int ep = 0; ep < epochs; ep++)
        for (size_t i = 0; i < N; i++) {
            int32_t r = (int32_t)((i * 7 + 3 * ep + 1) % N);
            if (ep == 1 && i % 7 == 0) r = (i % 14 == 0) ? -1 : (int32_t)N;
            perm[ep * N + i] = r;
        }
    int64_t step = 0;
    for (int pass = 0; pass < 2; pass++) {
        adv.nan(); ret.nan(); grad.nan(); stats.nan();
        if (pwh_update(&l, &p, &ws, &ms, &vs, &step, obs.p, act.p, rew.p, done.p, use.p, last.p, pass ? olp.p : nullptr, perm, work.p, adv.p, ret.p, grad.p,
                       stats.p) != 0) { printf("update refused\n"); return 1; }
        if (!adv.finite() || !ret.finite() || !grad.finite() || !stats.finite() || step != (pass + 1) * S) { printf("update pass %d: unwritten output or step\n", pass); return 1; }
        for (int i = 0; i < NT; i++)
            if (!w[i]->finite() || !m[i]->finite() || !v[i]->finite()) { printf("non-finite state\n"); return 1; }
    }
    // the act call on the same weights: 13 rows as three parts (obs 23 + 2 x 3), normalised, stochastic
    xarm_acw_layout al = {E, D - 6, 3, A, H, L, XARM_SACW_TANH, 5};
    xarm_policy_params pp = {9, 10.0, 1e-8, 0};
    Buf o0((size_t)E * (D - 6)), o1((size_t)E * 3), o2((size_t)E * 3), aw((size_t)pwh_act_workspace_bytes(&al) / 4), oa((size_t)E * A), oe((size_t)E * A), ol(E), ov(E);
    o0.fill(s, -2.f, 2.f); o1.fill(s, -2.f, 2.f); o2.fill(s, -2.f, 2.f);
    std::vector<double> st((size_t)2 * D + 4);
    for (int j = 0; j < D; j++) { st[j] = uni(s, -0.5f, 0.5f); st[D + j] = uni(s, 0.5f, 2.0f); }
    int64_t calls = 0;
    oa.nan(); oe.nan(); ol.nan(); ov.nan();
    if (pwh_act(&al, &pp, &ws, st.data(), &calls, o0.p, o1.p, o2.p, aw.p, oa.p, oe.p, ol.p, ov.p) != 0) { printf("act refused\n"); return 1; }
    if (!oa.finite() || !oe.finite() || !ol.finite() || !ov.finite() || calls != 1) { printf("act: unwritten output or calls\n"); return 1; }
    if (pwh_act(&al, &pp, &ws, nullptr, &calls, o0.p, o1.p, o2.p, aw.p, nullptr, oe.p, nullptr, nullptr) != 0 || calls != 2) { printf("act with null outputs refused\n"); return 1; }
    free(perm);
    for (int i = 0; i < NT; i++) { delete w[i]; delete m[i]; delete v[i]; }
    printf("ppow_main ok\n");
    return 0;
}
