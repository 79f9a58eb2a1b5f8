// Stand-alone driver of tests/hostbuild_ppo_opt for the sanitizer run of tests/test_ppo_opt_host.py (g++ -fsanitize=address,undefined;
// run directly, never loaded into python).  The options path of both cores - clip_range_vf, target_kl, both, and options that never
// act - over the two row shapes of the tests (5 x 13 rows in minibatches of 20 over 3 epochs, 3 x 40 in minibatches of 32 over 2), the
// fused tile's core at 64-64 tanh and the wide core at [64, 64] tanh and [256, 256, 256] ReLU, with a use mask, on exactly sized heap
// arrays (so that a read or write one element past a row, a tensor, perm, the workspace or an output is flagged).  Checks that every
// stats row was written, that column 7 is zeros then ones, that `step` advanced by the number of zeros, that a call with target_kl at
// lr 1e-2 stops before its end and that parameters and Adam's state stay finite.  Exit status 0 and "ppo_opt_main ok" when nothing
// was flagged.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "ppo_opt_host.cpp"

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

struct Rows {
    int T, E, D, A, batch, epochs;
};

// stats: column 7 is zeros then ones; returns the number of zeros, -1 when a row is unwritten or out of order
static int64_t applied_of(const Buf &stats, int64_t S) {
    if (!stats.finite()) return -1;
    int64_t zeros = 0;
    bool stopped = false;
    for (int64_t s = 0; s < S; s++) {
        const float f = stats.p[s * 8 + 7];
        if (f == 1.0f) stopped = true;
        else if (f != 0.0f || stopped) return -1;
        else zeros++;
    }
    return zeros;
}

// hidden 0: the fused tile's core; otherwise the wide core at `hidden` x `layers`
static int run_case(const Rows &r, int hidden, int layers, int act) {
    const size_t N = (size_t)r.T * r.E;
    const int D = r.D, A = r.A;
    xarm_ppo_params p = {0.99, 0.95, 0.2, 1e-2, 0.9, 0.999, 1e-5, 0.5, 0.01, 0.5, 1};
    uint32_t s = 31u + (uint32_t)N * 13u + (uint32_t)D * 7u + (uint32_t)hidden;
    std::vector<size_t> n;
    const int H = hidden ? hidden : 64, L = hidden ? layers : 2;
    for (int t = 0; t < 2; t++)
        for (int k = 0; k <= L; k++) {
            const size_t nin = k == 0 ? (size_t)D : (size_t)H, nout = k == L ? (t == 0 ? (size_t)A : 1) : (size_t)H;
            n.push_back(nout * nin); n.push_back(nout);
        }
    n.push_back((size_t)A);
    const int NT = (int)n.size(), tp = 2 * (L + 1);
    std::vector<Buf *> w, m, v;
    for (int i = 0; i < NT; i++) {
        w.push_back(new Buf(n[i])); m.push_back(new Buf(n[i])); v.push_back(new Buf(n[i]));
        w[i]->fill(s, i == NT - 1 ? -1.2f : -0.1f, i == NT - 1 ? -0.3f : 0.1f);
    }
    xarm_policy_weights pw[3] = {};
    xarm_acw_weights aw[3] = {};
    std::vector<Buf *> *st[3] = {&w, &m, &v};
    for (int k = 0; k < 3; k++) {
        const float **flat = (const float **)&pw[k];
        for (int i = 0; i < NT; i++) {
            if (!hidden) flat[i] = (*st[k])[i]->p;
            else if (i == NT - 1) aw[k].log_std = (*st[k])[i]->p;
            else (i < tp ? aw[k].pi[i] : aw[k].vf[i - tp]) = (*st[k])[i]->p;
        }
    }
    size_t P = 0;
    for (size_t x : n) P += x;
    const size_t B = (size_t)r.batch < N ? (size_t)r.batch : N;
    const int64_t S = (int64_t)r.epochs * (int64_t)((N + B - 1) / B);
    xarm_ppo_layout pl = {r.E, r.T, D, A, 64, r.epochs, r.batch};
    xarm_ppow_layout wl = {r.E, r.T, D, A, H, L, act, r.epochs, r.batch};
    Buf obs(N * D), actn(N * A), rew(N), done(N), use(N), last((size_t)r.E * D), adv(N), ret(N), grad(P), stats((size_t)S * 8);
    Buf work(hidden ? (size_t)powh_workspace_bytes(&wl) / 4 : 4);
    obs.fill(s, -2.5f, 2.5f); actn.fill(s, -1.f, 1.f); rew.fill(s, -1.f, 1.f); last.fill(s, -2.5f, 2.5f);
    for (size_t i = 0; i < N; i++) { done.p[i] = (lcg(s) >> 8) % 5 == 0 ? 1.0f : 0.0f; use.p[i] = (lcg(s) >> 8) % 10 == 0 ? 0.0f : 1.0f; }
    int32_t *perm = (int32_t *)malloc(sizeof(int32_t) * r.epochs * N);
    int64_t *step = (int64_t *)malloc(sizeof(int64_t));
    if (!perm || !step) abort();
    for (int ep = 0; ep < r.epochs; ep++)
        for (size_t i = 0; i < N; i++) perm[ep * N + i] = (int32_t)((i * 7 + 3 * ep + 1) % N);
    step[0] = 0;
    const xarm_ppo_options opts[4] = {{0.05, 0.0}, {0.0, 1e-4}, {0.05, 1e-4}, {1e30, 1e30}};
    int rc = 0;
    int64_t total = 0;
    for (int k = 0; k < 4 && !rc; k++) {
        adv.nan(); ret.nan(); grad.nan(); stats.nan();
        const int e = hidden ? powh_update(&wl, &p, &aw[0], &aw[1], &aw[2], step, obs.p, actn.p, rew.p, done.p, use.p, last.p, nullptr, perm, work.p, adv.p,
                                           ret.p, grad.p, stats.p, &opts[k], -1)
                             : poh_update(&pl, &p, &pw[0], &pw[1], &pw[2], step, obs.p, actn.p, rew.p, done.p, use.p, last.p, nullptr, perm, work.p, adv.p,
                                          ret.p, grad.p, stats.p, &opts[k], -1, nullptr);
        if (e != 0) { rc = 1; break; }
        const int64_t applied = applied_of(stats, S);
        if (applied < 0 || !adv.finite() || !ret.finite() || !grad.finite()) rc = 2;
        else if (opts[k].target_kl == 1e-4 && !(applied >= 1 && applied < S)) rc = 3;      // step 0 has approx_kl 0; an Adam step of 1e-2 moves it past 1.5e-4
        else if (opts[k].target_kl == 0.0 && applied != S) rc = 4;
        total += applied > 0 ? applied : 0;
        if (!rc && step[0] != total) rc = 5;
        for (int i = 0; i < NT && !rc; i++)
            if (!(w[i]->finite() && m[i]->finite() && v[i]->finite())) rc = 6;
        if (rc) printf("options %d (%g, %g): applied %lld of %lld, step %lld\n", k, opts[k].clip_range_vf, opts[k].target_kl, (long long)applied, (long long)S,
                       (long long)step[0]);
    }
    for (int i = 0; i < NT; i++) { delete w[i]; delete m[i]; delete v[i]; }
    free(perm);
    free(step);
    return rc;
}

int main() {
    static const Rows rows[2] = {{5, 13, 14, 4, 20, 3}, {3, 40, 30, 4, 32, 2}};
    static const int arch[3][3] = {{0, 0, 0}, {64, 2, XARM_SACW_TANH}, {256, 3, XARM_SACW_RELU}};
    for (const Rows &r : rows)
        for (auto &a : arch) {
            const int rc = run_case(r, a[0], a[1], a[2]);
            if (rc) {
                printf("ppo_opt_main FAILED: T %d E %d D %d A %d batch %d hidden %d x %d -> %d\n", r.T, r.E, r.D, r.A, r.batch, a[0], a[1], rc);
                return 1;
            }
        }
    const xarm_ppo_options bad = {-1.0, 0.0};
    xarm_ppo_layout pl = {13, 5, 14, 4, 64, 3, 20};
    xarm_ppo_params p = {0.99, 0.95, 0.2, 3e-4, 0.9, 0.999, 1e-5, 0.5, 0.0, 0.5, 1};
    xarm_policy_weights none = {};
    if (poh_update(&pl, &p, &none, &none, &none, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                   nullptr, &bad, -1, nullptr) != -1) {
        printf("ppo_opt_main FAILED: a negative option is refused\n");
        return 1;
    }
    printf("ppo_opt_main ok\n");
    return 0;
}
