// Stand-alone driver of the host build of csrc/xarm_a2cw_core.h for the sanitizer run of tests/test_a2cw_host.py (g++
// -fsanitize=address,undefined; run directly, never loaded into python).  Two updates at (29, 1, 192, 3, tanh), 5 x 13 rows, with a use mask
// and every optional output, then one without the mask and without outputs, on exactly sized heap arrays (so that a read or write one
// element past a row, a tensor, the workspace or an output is flagged).  Checks that every requested output element was written, that
// parameters and square_avg stay finite and that the chain ran 3 L + 7 launches.  Exit status 0 and "a2cw_main ok" when nothing was flagged.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "a2cw_host.cpp"

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
    const int T = 5, E = 13, D = 29, A = 1, H = 192, L = 3;
    const size_t N = (size_t)T * E;
    xarm_a2cw_layout l = {E, T, D, A, H, L, XARM_SACW_TANH};
    xarm_a2c_params p = {0.95, 1e-3, 0.99, 1e-5, 0.5, 0.01, 0.5};
    uint32_t s = 2626u;
    int64_t geo[48];
    awh_geometry(&l, geo);
    const int64_t P = geo[0], NT = geo[6];
    if (geo[1] != (int64_t)N || geo[2] != 1 || NT != 17 || geo[4] != 16) { printf("unexpected geometry\n"); return 1; }
    std::vector<Buf *> w, q;
    xarm_acw_weights ws = {}, qs = {};
    for (int i = 0; i < NT; i++) {
        const size_t n = (size_t)(geo[25 + i + 1] - geo[25 + i]);
        w.push_back(new Buf(n)); q.push_back(new Buf(n));
        w[i]->fill(s, i == NT - 1 ? -1.2f : -0.08f, i == NT - 1 ? -0.3f : 0.08f);
        q[i]->fill(s, 0.0f, 0.01f);
        const float **slot[2] = {i == NT - 1 ? &ws.log_std : (i < 8 ? &ws.pi[i] : &ws.vf[i - 8]), i == NT - 1 ? &qs.log_std : (i < 8 ? &qs.pi[i] : &qs.vf[i - 8])};
        *slot[0] = w[i]->p; *slot[1] = q[i]->p;
    }
    Buf obs(N * D), act(N * A), rew(N), done(N), use(N), last((size_t)E * D), ret(N), grad((size_t)P), stats(8);
    Buf work((size_t)awh_workspace_bytes(&l) / 4);
    obs.fill(s, -2.5f, 2.5f); act.fill(s, -1.f, 1.f); rew.fill(s, -1.f, 1.f); last.fill(s, -2.5f, 2.5f);
    for (size_t i = 0; i < N; i++) { done.p[i] = (lcg(s) >> 8) % 5 == 0 ? 1.0f : 0.0f; use.p[i] = (lcg(s) >> 8) % 10 == 0 ? 0.0f : 1.0f; }
    for (int pass = 0; pass < 3; pass++) {
        const bool bare = pass == 2;
        int64_t launched = -1;
        ret.nan(); grad.nan(); stats.nan();
        if (awh_update(&l, &p, &ws, &qs, obs.p, act.p, rew.p, done.p, bare ? nullptr : use.p, last.p, work.p, bare ? nullptr : ret.p, bare ? nullptr : grad.p,
                       bare ? nullptr : stats.p, &launched) != 0) { printf("update refused\n"); return 1; }
        if (launched != 3 * L + 7) { printf("update pass %d: %lld launches\n", pass, (long long)launched); return 1; }
        if (!bare && (!ret.finite() || !grad.finite() || !stats.finite())) { printf("update pass %d: unwritten output\n", pass); return 1; }
        for (int i = 0; i < NT; i++)
            if (!w[i]->finite() || !q[i]->finite()) { printf("non-finite state\n"); return 1; }
    }
    for (int i = 0; i < NT; i++) { delete w[i]; delete q[i]; }
    printf("a2cw_main ok\n");
    return 0;
}
