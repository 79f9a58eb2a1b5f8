// Stand-alone driver of the host build of csrc/xarm_sac_core.h for the sanitizer run of tests/test_sac_host.py
// (g++ -fsanitize=address,undefined; run directly, never loaded into python).  Steps and act calls on fixed inputs over the row counts
// and widths of the CPU tests, with and without a use mask, supplied and Philox noise, a fixed and a trained entropy coefficient and
// the optional outputs, on exactly sized heap arrays (so that a read or write one element past a row, a tensor or an output is
// flagged).  Checks that every requested output element was written, that parameters, targets and Adam's state stay finite, that
// `step` and `calls` advanced and that the all-masked batch from zero state leaves the trained parameters alone.
// Exit status 0 and "sac_main ok" when nothing was flagged.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "sac_host.cpp"

static uint32_t lcg(uint32_t &s) { s = s * 1664525u + 1013904223u; return s; }
static float uni(uint32_t &s, float lo, float hi) { return lo + (hi - lo) * ((float)(lcg(s) >> 8) / 16777216.0f); }

// 16-byte aligned, exactly sized
struct Buf {
    float *p; size_t n;
    explicit Buf(size_t n_) : p(nullptr), n(n_) { if (posix_memalign((void **)&p, 16, (n ? n : 1) * sizeof(float))) abort(); }
    ~Buf() { free(p); }
    void fill(uint32_t &s, float lo, float hi) { for (size_t i = 0; i < n; i++) p[i] = uni(s, lo, hi); }
    void nan() { for (size_t i = 0; i < n; i++) p[i] = NAN; }
    void zero() { for (size_t i = 0; i < n; i++) p[i] = 0.0f; }
    bool finite() const { for (size_t i = 0; i < n; i++) if (!std::isfinite(p[i])) return false; return true; }
};

// mode: 0 no mask, Philox noise, every output; 1 mask, supplied noise, no output, fixed alpha; 2 all masked from zero state
static int run_case(int B, int D, int A, int mode) {
    const int Dq = D + A;
    xarm_sac_layout l = {B, D, A, 64, 7};
    xarm_sac_params p = {11u, 0.95, 1e-3, 0.005, 0.2, -(double)A, 0.9, 0.999, 1e-8, mode != 1, 0};
    uint32_t s = 4177u + (uint32_t)B * 13u + (uint32_t)D * 7u + (uint32_t)A + (uint32_t)mode;
    const size_t na[6] = {(size_t)64 * D, 64, 4096, 64, (size_t)128 * A, (size_t)2 * A}, nq[6] = {(size_t)64 * Dq, 64, 4096, 64, 64, 1};
    std::vector<Buf *> w, m, v;
    std::vector<size_t> n;
    for (int i = 0; i < 31; i++) {
        const size_t k = i < 6 ? na[i] : (i < 30 ? nq[(i - 6) % 6] : 1);
        n.push_back(k);
        w.push_back(new Buf(k)); m.push_back(new Buf(k)); v.push_back(new Buf(k));
        const float r = (i % 6) < 2 && i < 30 ? 1.0f / std::sqrt((float)(i < 6 ? D : Dq)) : 0.125f;
        w[i]->fill(s, -r, r);
        if (mode == 2) { m[i]->zero(); v[i]->zero(); } else { m[i]->fill(s, -0.01f, 0.01f); v[i]->fill(s, 0.0f, 0.01f); }
    }
    auto pack = [](std::vector<Buf *> &x) {
        xarm_sac_weights ws;
        for (int i = 0; i < 6; i++) { ws.actor[i] = x[i]->p; ws.q1[i] = x[6 + i]->p; ws.q2[i] = x[12 + i]->p; ws.q1_target[i] = x[18 + i]->p; ws.q2_target[i] = x[24 + i]->p; }
        ws.log_alpha = x[30]->p;
        return ws;
    };
    xarm_sac_weights ws = pack(w), ms = pack(m), vs = pack(v);
    Buf obs((size_t)B * D), nobs((size_t)B * D), act((size_t)B * A), rew(B), done(B), use(B), zp((size_t)B * A), zn((size_t)B * A), work(4);
    const int64_t P = sh_param_count(&l);
    Buf grad((size_t)P), dqda((size_t)2 * B * A), target(B), stats(8), oa((size_t)B * A), ol(B);
    obs.fill(s, -3.f, 3.f); nobs.fill(s, -3.f, 3.f); act.fill(s, -1.f, 1.f); rew.fill(s, -1.f, 1.f); zp.fill(s, -2.f, 2.f); zn.fill(s, -2.f, 2.f);
    for (int i = 0; i < B; i++) { done.p[i] = (lcg(s) >> 8) % 5 == 0 ? 1.0f : 0.0f; use.p[i] = mode == 2 ? 0.0f : ((lcg(s) >> 8) % 10 == 0 ? 0.0f : 1.0f); }
    std::vector<std::vector<float>> before;
    for (int i = 0; i < 31; i++) before.emplace_back(w[i]->p, w[i]->p + n[i]);
    int64_t *step = (int64_t *)malloc(sizeof(int64_t)), *calls = (int64_t *)malloc(sizeof(int64_t));
    if (!step || !calls) abort();
    step[0] = 5; calls[0] = 3;
    const bool out = mode != 1;
    int rc = 0;
    if (sh_workspace_bytes(&l) <= 0) rc = 6;
    for (int k = 0; k < 2 && !rc; k++) {
        grad.nan(); dqda.nan(); target.nan(); stats.nan();
        if (sh_update(&l, &p, &ws, &ms, &vs, step, obs.p, nobs.p, act.p, rew.p, done.p, mode ? use.p : nullptr, mode == 1 ? zp.p : nullptr,
                      mode == 1 ? zn.p : nullptr, work.p, out ? grad.p : nullptr, out ? dqda.p : nullptr, out ? target.p : nullptr,
                      out ? stats.p : nullptr) != 0) { rc = 1; break; }
        if (out && !(grad.finite() && dqda.finite() && target.finite() && stats.finite())) rc = 2;
        if (!out && !(std::isnan(grad.p[0]) && std::isnan(dqda.p[0]) && std::isnan(target.p[0]) && std::isnan(stats.p[0]))) rc = 3;
        if (step[0] != 5 + (k + 1)) rc = 7;
        for (int i = 0; i < 31 && !rc; i++) {
            if (!w[i]->finite() || (i < 18 || i == 30 ? !(m[i]->finite() && v[i]->finite()) : false)) rc = 4;
            // an all-masked batch from zero state: Adam's step on a zero gradient is p - x * (0 / eps) = p for every trained tensor
            if (mode == 2 && (i < 18 || i == 30) && memcmp(w[i]->p, before[i].data(), n[i] * sizeof(float)) != 0) rc = 5;
        }
    }
    for (int det = 0; det < 2 && !rc; det++) {
        oa.nan(); ol.nan();
        xarm_sac_params pa = p;
        pa.deterministic = det;
        if (sh_act(&l, &pa, &ws, calls, obs.p, oa.p, det ? nullptr : ol.p) != 0) { rc = 8; break; }
        if (!oa.finite() || (!det && !ol.finite()) || calls[0] != 4) rc = 9;
        for (size_t i = 0; i < oa.n; i++) if (!(std::fabs(oa.p[i]) <= 1.0f)) rc = 10;
    }
    for (int i = 0; i < 31; i++) { delete w[i]; delete m[i]; delete v[i]; }
    free(step);
    free(calls);
    return rc;
}

int main() {
    static const int rows[] = {1, 31, 33, 64, 65, 200}, widths[][2] = {{14, 4}, {30, 4}, {29, 1}, {88, 8}, {1, 1}};
    for (int B : rows)
        for (auto &wd : widths)
            for (int mode = 0; mode < 3; mode++) {
                if (B == 200 && wd[0] == 88 && mode == 2) continue;
                const int rc = run_case(B, wd[0], wd[1], mode);
                if (rc) {
                    printf("sac_main FAILED: B %d D %d A %d mode %d -> %d\n", B, wd[0], wd[1], mode, rc);
                    return 1;
                }
            }
    xarm_sac_layout zero = {0, 14, 4, 64, 0};
    xarm_sac_params p = {0u, 0.95, 1e-3, 0.005, 0.2, -4.0, 0.9, 0.999, 1e-8, 1, 0};
    xarm_sac_weights none = {};
    if (sh_update(&zero, &p, &none, &none, &none, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                  nullptr, nullptr) != 0 || sh_act(&zero, &p, &none, nullptr, nullptr, nullptr, nullptr) != 0) {
        printf("sac_main FAILED: batch_size 0 is a no-op\n");
        return 1;
    }
    printf("sac_main ok\n");
    return 0;
}
