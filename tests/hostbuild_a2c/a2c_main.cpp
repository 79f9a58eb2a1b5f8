// Stand-alone driver of the host build of csrc/xarm_a2c_core.h for the sanitizer run of tests/test_a2c_host.py
// (g++ -fsanitize=address,undefined; run directly, never loaded into python).  Updates on fixed inputs over the row counts and
// widths of the CPU tests, with and without a use mask and the optional outputs, on exactly sized heap arrays (so that a read or
// write one element past a row, a tensor or an output is flagged).  Checks that every requested output element was written, that
// parameters and square_avg stay finite and that the all-masked batch leaves the parameters alone.
// Exit status 0 and "a2c_main ok" when nothing was flagged.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "a2c_host.cpp"

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

static int run_case(int T, int E, int D, int A, int masked, int with_out) {
    const size_t N = (size_t)T * E;
    xarm_a2c_layout l = {E, T, D, A, 64};
    xarm_a2c_params p = {0.99, 7e-4, 0.99, 1e-5, 0.5, 0.01, 0.5};
    uint32_t s = 4242u + (uint32_t)N * 13u + (uint32_t)D * 7u + (uint32_t)A;
    const float k1 = 1.0f / std::sqrt((float)D);
    const size_t n[13] = {(size_t)64 * D, 64, 4096, 64, (size_t)64 * A, (size_t)A, (size_t)64 * D, 64, 4096, 64, 64, 1, (size_t)A};
    std::vector<Buf *> w, q;
    for (int i = 0; i < 13; i++) {
        w.push_back(new Buf(n[i])); q.push_back(new Buf(n[i]));
        const float k = (i % 6) < 2 && i < 12 ? k1 : 0.125f;
        w[i]->fill(s, i == 12 ? -2.0f : -k, i == 12 ? 0.5f : k);
        q[i]->fill(s, 0.0f, 0.01f);
    }
    Buf obs(N * D), act(N * A), rew(N), done(N), use(N), last((size_t)E * D), ret(N), stats(8), work(4);
    const int64_t P = ah_param_count(&l);
    Buf grad((size_t)P);
    obs.fill(s, -3.f, 3.f); act.fill(s, -2.f, 2.f); rew.fill(s, -1.f, 1.f); last.fill(s, -3.f, 3.f);
    for (size_t i = 0; i < N; i++) { done.p[i] = (lcg(s) >> 8) % 5 == 0 ? 1.0f : 0.0f; use.p[i] = masked == 2 ? 0.0f : ((lcg(s) >> 8) % 10 == 0 ? 0.0f : 1.0f); }
    xarm_policy_weights ws = {w[0]->p, w[1]->p, w[2]->p, w[3]->p, w[4]->p, w[5]->p, w[6]->p, w[7]->p, w[8]->p, w[9]->p, w[10]->p, w[11]->p, w[12]->p};
    xarm_policy_weights qs = {q[0]->p, q[1]->p, q[2]->p, q[3]->p, q[4]->p, q[5]->p, q[6]->p, q[7]->p, q[8]->p, q[9]->p, q[10]->p, q[11]->p, q[12]->p};
    std::vector<std::vector<float>> before;
    for (int i = 0; i < 13; i++) before.emplace_back(w[i]->p, w[i]->p + n[i]);
    int rc = 0;
    if (ah_workspace_bytes(&l) <= 0) rc = 6;
    for (int k = 0; k < 2 && !rc; k++) {
        ret.nan(); grad.nan(); stats.nan();
        if (ah_update(&l, &p, &ws, &qs, obs.p, act.p, rew.p, done.p, masked ? use.p : nullptr, last.p, work.p, with_out ? ret.p : nullptr,
                      with_out ? grad.p : nullptr, with_out ? stats.p : nullptr) != 0) { rc = 1; break; }
        if (with_out && !(ret.finite() && grad.finite() && stats.finite())) rc = 2;
        if (!with_out && !(std::isnan(ret.p[0]) && std::isnan(grad.p[0]) && std::isnan(stats.p[0]))) rc = 3;
        for (int i = 0; i < 13 && !rc; i++) {
            if (!(w[i]->finite() && q[i]->finite())) rc = 4;
            // an all-masked batch with no entropy term on this tensor: nothing moves
            if (masked == 2 && i < 12 && memcmp(w[i]->p, before[i].data(), n[i] * sizeof(float)) != 0) rc = 5;
        }
    }
    for (int i = 0; i < 13; i++) { delete w[i]; delete q[i]; }
    return rc;
}

int main() {
    static const int shapes[][2] = {{1, 1}, {1, 31}, {5, 13}, {5, 200}, {3, 64}}, widths[][2] = {{14, 4}, {29, 1}, {30, 4}, {96, 16}, {1, 1}};
    for (auto &sh : shapes)
        for (auto &wd : widths)
            for (int masked = 0; masked < 3; masked++)
                for (int with_out = 0; with_out < 2; with_out++) {
                    if (sh[1] == 200 && (wd[0] != 30 || masked == 2)) continue;           // the large batch at one width
                    const int rc = run_case(sh[0], sh[1], wd[0], wd[1], masked, with_out);
                    if (rc) {
                        printf("a2c_main FAILED: T %d E %d D %d A %d masked %d out %d -> %d\n", sh[0], sh[1], wd[0], wd[1], masked, with_out, rc);
                        return 1;
                    }
                }
    xarm_a2c_layout zero = {0, 5, 14, 4, 64};
    xarm_a2c_params p = {0.99, 7e-4, 0.99, 1e-5, 0.5, 0.0, 0.5};
    xarm_policy_weights none = {};
    if (ah_update(&zero, &p, &none, &none, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) != 0) {
        printf("a2c_main FAILED: num_envs 0 is a no-op\n");
        return 1;
    }
    printf("a2c_main ok\n");
    return 0;
}
