// Stand-alone driver of the host build of csrc/xarm_ppo_core.h for the sanitizer run of tests/test_ppo_host.py
// (g++ -fsanitize=address,undefined; run directly, never loaded into python).  Updates on fixed inputs over the row counts, widths and
// batch sizes of the CPU tests, with and without a use mask, a supplied old_logp, out-of-range perm entries and the optional outputs,
// on exactly sized heap arrays (so that a read or write one element past a row, a tensor, perm or an output is flagged).  Checks that
// every requested output element was written, that parameters and Adam's state stay finite, that `step` advanced by the number of
// optimiser steps and that the all-masked batch leaves the parameters alone.
// Exit status 0 and "ppo_main ok" when nothing was flagged.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "ppo_host.cpp"

static uint32_t lcg(uint32_t &s) { s = s * 1664525u + 1013904223u; return s; }
static float uni(uint32_t &s, float lo, float hi) { return lo + (hi - lo) * ((float)(lcg(s) >> 8) / 16777216.0f); }

// 16-byte aligned, exactly sized
struct Buf {
    float *p; size_t n;
    explicit Buf(size_t n_) : p(nullptr), n(n_) { if (posix_memalign((void **)&p, 16, (n ? n : 1) * sizeof(float))) abort(); }
    ~Buf() { free(p); }
    void fill(uint32_t &s, float lo, float hi) { for (size_t i = 0; i < n; i++) p[i] = uni(s, lo, hi); }
    void nan() { for (size_t i = 0; i < n; i++) p[i] = NAN; }
    bool finite() const { for (size_t i = 0; i < n; i++) if (!std::isfinite(p[i])) return false; return true; }
};

static int run_case(int T, int E, int D, int A, int batch, int masked, int with_out) {
    const size_t N = (size_t)T * E;
    const int epochs = 2;
    xarm_ppo_layout l = {E, T, D, A, 64, epochs, batch};
    xarm_ppo_params p = {0.99, 0.95, 0.2, 3e-4, 0.9, 0.999, 1e-5, 0.5, 0.01, 0.5, with_out};
    uint32_t s = 977u + (uint32_t)N * 13u + (uint32_t)D * 7u + (uint32_t)A + (uint32_t)batch;
    const float k1 = 1.0f / std::sqrt((float)D);
    const size_t n[13] = {(size_t)64 * D, 64, 4096, 64, (size_t)64 * A, (size_t)A, (size_t)64 * D, 64, 4096, 64, 64, 1, (size_t)A};
    std::vector<Buf *> w, m, v;
    for (int i = 0; i < 13; i++) {
        w.push_back(new Buf(n[i])); m.push_back(new Buf(n[i])); v.push_back(new Buf(n[i]));
        const float k = (i % 6) < 2 && i < 12 ? k1 : 0.125f;
        w[i]->fill(s, i == 12 ? -2.0f : -k, i == 12 ? 0.5f : k);
        m[i]->fill(s, -0.01f, 0.01f);
        v[i]->fill(s, 0.0f, 0.01f);
    }
    Buf obs(N * D), act(N * A), rew(N), done(N), use(N), last((size_t)E * D), olp(N), adv(N), ret(N), work(4);
    int64_t geo[8];
    ph_geometry(&l, geo);
    const int64_t P = ph_param_count(&l), S = geo[6];
    Buf grad((size_t)P), stats((size_t)S * 8);
    obs.fill(s, -3.f, 3.f); act.fill(s, -2.f, 2.f); rew.fill(s, -1.f, 1.f); last.fill(s, -3.f, 3.f); olp.fill(s, -12.f, -2.f);
    for (size_t i = 0; i < N; i++) { done.p[i] = (lcg(s) >> 8) % 5 == 0 ? 1.0f : 0.0f; use.p[i] = masked == 2 ? 0.0f : ((lcg(s) >> 8) % 10 == 0 ? 0.0f : 1.0f); }
    // exactly sized perm: a rotation per epoch, every seventh entry of the second epoch out of range
    int32_t *perm = (int32_t *)malloc(sizeof(int32_t) * epochs * N);
    if (!perm) abort();
    for (int ep = 0; ep < epochs; ep++)
        for (size_t i = 0; i < N; i++) {
            int32_t r = (int32_t)((i * 7 + 3 * ep + 1) % N);
            if (N % 7 == 0) r = (int32_t)((i + ep) % N);
            if (ep == 1 && i % 7 == 0) r = (i % 14 == 0) ? -1 : (int32_t)N;
            perm[ep * N + i] = r;
        }
    xarm_policy_weights ws = {w[0]->p, w[1]->p, w[2]->p, w[3]->p, w[4]->p, w[5]->p, w[6]->p, w[7]->p, w[8]->p, w[9]->p, w[10]->p, w[11]->p, w[12]->p};
    xarm_policy_weights ms = {m[0]->p, m[1]->p, m[2]->p, m[3]->p, m[4]->p, m[5]->p, m[6]->p, m[7]->p, m[8]->p, m[9]->p, m[10]->p, m[11]->p, m[12]->p};
    xarm_policy_weights vs = {v[0]->p, v[1]->p, v[2]->p, v[3]->p, v[4]->p, v[5]->p, v[6]->p, v[7]->p, v[8]->p, v[9]->p, v[10]->p, v[11]->p, v[12]->p};
    std::vector<std::vector<float>> before;
    for (int i = 0; i < 13; i++) before.emplace_back(w[i]->p, w[i]->p + n[i]);
    if (masked == 2)
        for (int i = 0; i < 13; i++) { memset(m[i]->p, 0, n[i] * sizeof(float)); memset(v[i]->p, 0, n[i] * sizeof(float)); }
    int64_t *step = (int64_t *)malloc(sizeof(int64_t));
    if (!step) abort();
    step[0] = 5;
    int rc = 0;
    if (ph_workspace_bytes(&l) <= 0) rc = 6;
    for (int k = 0; k < 2 && !rc; k++) {
        adv.nan(); ret.nan(); grad.nan(); stats.nan();
        if (ph_update(&l, &p, &ws, &ms, &vs, step, obs.p, act.p, rew.p, done.p, masked ? use.p : nullptr, last.p, k ? olp.p : nullptr, perm, work.p,
                      with_out ? adv.p : nullptr, with_out ? ret.p : nullptr, with_out ? grad.p : nullptr, with_out ? stats.p : nullptr, nullptr) != 0) { rc = 1; break; }
        if (with_out && !(adv.finite() && ret.finite() && grad.finite() && stats.finite())) rc = 2;
        if (!with_out && !(std::isnan(adv.p[0]) && std::isnan(ret.p[0]) && std::isnan(grad.p[0]) && std::isnan(stats.p[0]))) rc = 3;
        if (step[0] != 5 + (k + 1) * S) rc = 7;
        for (int i = 0; i < 13 && !rc; i++) {
            if (!(w[i]->finite() && m[i]->finite() && v[i]->finite())) rc = 4;
            // an all-masked batch from zero state with no entropy term on this tensor: nothing moves
            if (masked == 2 && i < 12 && memcmp(w[i]->p, before[i].data(), n[i] * sizeof(float)) != 0) rc = 5;
        }
    }
    for (int i = 0; i < 13; i++) { delete w[i]; delete m[i]; delete v[i]; }
    free(perm);
    free(step);
    return rc;
}

int main() {
    static const int shapes[][2] = {{1, 1}, {1, 33}, {5, 13}, {3, 64}}, widths[][2] = {{14, 4}, {29, 1}, {30, 4}, {96, 16}, {1, 1}};
    static const int batches[] = {1 << 20, 64, 20};
    static const int modes[][2] = {{0, 1}, {1, 0}, {2, 1}};        // (masked, with_out)
    for (auto &sh : shapes)
        for (auto &wd : widths)
            for (int batch : batches)
                for (auto &md : modes) {
                    // the minibatch sizes at the shapes they split, at three widths, with a mask and every output
                    if (batch != batches[0] && (sh[0] * sh[1] < 65 || wd[0] == 96 || wd[0] == 1 || md[0] != 1)) continue;
                    const int rc = run_case(sh[0], sh[1], wd[0], wd[1], batch, md[0], batch != batches[0] ? 1 : md[1]);
                    if (rc) {
                        printf("ppo_main FAILED: T %d E %d D %d A %d batch %d masked %d out %d -> %d\n", sh[0], sh[1], wd[0], wd[1], batch, md[0], md[1], rc);
                        return 1;
                    }
                }
    xarm_ppo_layout zero = {0, 5, 14, 4, 64, 2, 64};
    xarm_ppo_params p = {0.99, 0.95, 0.2, 3e-4, 0.9, 0.999, 1e-5, 0.5, 0.0, 0.5, 1};
    xarm_policy_weights none = {};
    if (ph_update(&zero, &p, &none, &none, &none, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                  nullptr, nullptr, nullptr) != 0) {
        printf("ppo_main FAILED: num_envs 0 is a no-op\n");
        return 1;
    }
    printf("ppo_main ok\n");
    return 0;
}
