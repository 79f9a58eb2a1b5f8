// Stand-alone driver of the host build of csrc/xarm_td3_core.h for the sanitizer run of tests/test_td3_host.py
// (g++ -fsanitize=address,undefined; run directly, never loaded into python).  Steps and act calls on fixed inputs over the shapes and
// row counts of the CPU tests, with and without a use mask, given and Philox noise, policy_delay 1 and 2 and the optional outputs, on
// exactly sized heap arrays - the workspace included - so that a read or write one element past a row, a tensor, an output or a part
// of the workspace's end is flagged.  Checks that every requested output element was written, that parameters, targets and Adam's
// state stay finite, that `step` and `calls` advanced, that the chain ran launches(n_hidden) jobs, that a delayed call leaves the
// actor and every target alone and that the all-masked batch from zero state leaves the trained parameters alone.  Exit status 0 and
// "td3_main ok" when nothing was flagged.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "td3_host.cpp"

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

// mode: 0 no mask, Philox noise, every output, policy_delay 1; 1 mask, given noise, no output, policy_delay 2; 2 all masked from zero state
static int run_case(int B, int D, int A, int H, int L, int act, int mode) {
    xarm_sacw_layout l = {B, D, A, H, L, act, 7};
    xarm_td3_params p = {11u, 0.95, 1e-3, 0.005, 0.9, 0.999, 1e-8, 0.2, 0.5, 0.1, mode == 1 ? 2 : 1, 0};
    uint32_t s = 4177u + (uint32_t)B * 13u + (uint32_t)D * 7u + (uint32_t)A + (uint32_t)mode + (uint32_t)H;
    Shape sh;
    shape_of(sh, &l);
    const int tp = sh.tp, nt = 6 * tp;
    std::vector<Buf *> w, m, v;
    std::vector<size_t> n;
    for (int i = 0; i < nt; i++) {
        const int t = (i / tp) % 3 == 0 ? i % tp : tp + i % tp;          // the size of trained tensor i % tp of the actor or of a critic
        const size_t k = (size_t)(sh.off[t + 1] - sh.off[t]);
        n.push_back(k);
        w.push_back(new Buf(k)); m.push_back(new Buf(k)); v.push_back(new Buf(k));
        const float r = 1.0f / std::sqrt((float)((i % tp) < 2 ? ((i / tp) % 3 == 0 ? D : D + A) : H));
        w[i]->fill(s, -r, r);
        if (mode == 2) { m[i]->zero(); v[i]->zero(); } else { m[i]->fill(s, -0.01f, 0.01f); v[i]->fill(s, 0.0f, 0.01f); }
    }
    auto pack = [tp](std::vector<Buf *> &x) {
        xarm_td3_weights ws = {};
        for (int i = 0; i < tp; i++) {
            ws.actor[i] = x[i]->p; ws.q1[i] = x[tp + i]->p; ws.q2[i] = x[2 * tp + i]->p;
            ws.actor_target[i] = x[3 * tp + i]->p; ws.q1_target[i] = x[4 * tp + i]->p; ws.q2_target[i] = x[5 * tp + i]->p;
        }
        return ws;
    };
    xarm_td3_weights ws = pack(w), ms = pack(m), vs = pack(v);
    const int64_t wbytes = t3h_workspace_bytes(&l), P = t3h_param_count(&l);
    if (wbytes <= 0 || P != sh.P) return 6;
    Buf obs((size_t)B * D), nobs((size_t)B * D), actn((size_t)B * A), rew(B), done(B), use(B), zn((size_t)B * A), work((size_t)wbytes / 4);
    Buf grad((size_t)P), dqda((size_t)B * A), target(B), stats(8), q((size_t)2 * B), oa((size_t)B * A);
    obs.fill(s, -3.f, 3.f); nobs.fill(s, -3.f, 3.f); actn.fill(s, -1.f, 1.f); rew.fill(s, -1.f, 1.f); zn.fill(s, -2.f, 2.f);
    for (int i = 0; i < B; i++) { done.p[i] = (lcg(s) >> 8) % 5 == 0 ? 1.0f : 0.0f; use.p[i] = mode == 2 ? 0.0f : ((lcg(s) >> 8) % 10 == 0 ? 0.0f : 1.0f); }
    int64_t *step = (int64_t *)malloc(sizeof(int64_t)), *calls = (int64_t *)malloc(sizeof(int64_t));
    if (!step || !calls) abort();
    step[0] = 4; calls[0] = 3;
    const bool out = mode != 1;
    int rc = 0;
    for (int k = 0; k < 2 && !rc; k++) {
        std::vector<std::vector<float>> before;
        for (int i = 0; i < nt; i++) before.emplace_back(w[i]->p, w[i]->p + n[i]);
        grad.nan(); dqda.nan(); target.nan(); q.nan(); work.nan(); stats.zero();
        const bool steps = (step[0] + 1) % p.policy_delay == 0;
        const int got = t3h_update(&l, &p, &ws, &ms, &vs, step, obs.p, nobs.p, actn.p, rew.p, done.p, mode ? use.p : nullptr, mode == 1 ? zn.p : nullptr,
                                   work.p, out ? grad.p : nullptr, out ? target.p : nullptr, out ? q.p : nullptr, out ? dqda.p : nullptr,
                                   out ? stats.p : nullptr);
        if (got != launches(L)) { rc = 1; break; }
        if (out && !(grad.finite() && dqda.finite() && target.finite() && stats.finite() && q.finite())) rc = 2;
        if (!out && !(std::isnan(grad.p[0]) && std::isnan(dqda.p[0]) && std::isnan(target.p[0]) && std::isnan(q.p[0]))) rc = 3;
        if (out && stats.p[5] != (steps ? 1.0f : 0.0f)) rc = 11;
        if (step[0] != 4 + (k + 1)) rc = 7;
        for (int i = 0; i < nt && !rc; i++) {
            const bool is_trained = i < 3 * tp, same = memcmp(w[i]->p, before[i].data(), n[i] * sizeof(float)) == 0;
            if (!w[i]->finite() || (is_trained ? !(m[i]->finite() && v[i]->finite()) : false)) rc = 4;
            // an all-masked batch from zero state: Adam's step on a zero gradient is p - x * (0 / eps) = p for every trained tensor
            if (mode == 2 && is_trained && !same) rc = 5;
            // a delayed call leaves the actor and every target alone
            if (!steps && (i < tp || i >= 3 * tp) && !same) rc = 12;
        }
    }
    for (int am = 0; am < 3 && !rc; am++) {
        oa.nan(); work.nan();
        xarm_td3_params pa = p;
        pa.mode = am;
        const int64_t c0 = calls[0];
        if (t3h_act(&l, &pa, &ws, calls, obs.p, work.p, oa.p) != 0) { rc = 8; break; }
        if (!oa.finite() || calls[0] != c0 + (am ? 1 : 0)) rc = 9;
        for (size_t i = 0; i < oa.n; i++) if (!(std::fabs(oa.p[i]) <= 1.0f)) rc = 10;
    }
    for (int i = 0; i < nt; i++) { delete w[i]; delete m[i]; delete v[i]; }
    free(step);
    free(calls);
    return rc;
}

int main() {
    static const int shapes[][5] = {{14, 4, 128, 2, 1}, {30, 4, 256, 3, 1}, {29, 1, 192, 3, 0}, {88, 8, 256, 2, 0}, {14, 4, 64, 2, 0}};
    static const int rows[] = {1, 63, 65, 200};
    for (auto &sh : shapes)
        for (int B : rows)
            for (int mode = 0; mode < 3; mode++) {
                if (sh[2] == 256 && (B == 63 || (B > 65 && (mode != 0 || sh[0] != 30)))) continue;   // the wide shapes: fewer, for the run's length
                const int rc = run_case(B, sh[0], sh[1], sh[2], sh[3], sh[4], mode);
                if (rc) {
                    printf("td3_main FAILED: B %d D %d A %d H %d L %d act %d mode %d -> %d\n", B, sh[0], sh[1], sh[2], sh[3], sh[4], mode, rc);
                    return 1;
                }
            }
    if (run_case(64 * xsacw::MAX_SPLIT + 1, 14, 4, 64, 2, 1, 1)) { printf("td3_main FAILED: every row range\n"); return 1; }
    xarm_sacw_layout zero = {0, 14, 4, 256, 3, 1, 0};
    xarm_td3_params p = {0u, 0.95, 1e-3, 0.005, 0.9, 0.999, 1e-8, 0.2, 0.5, 0.1, 2, 0};
    xarm_td3_weights none = {};
    if (t3h_update(&zero, &p, &none, &none, &none, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                   nullptr, nullptr) != 0 || t3h_act(&zero, &p, &none, nullptr, nullptr, nullptr, nullptr) != 0) {
        printf("td3_main FAILED: batch_size 0 is a no-op\n");
        return 1;
    }
    printf("td3_main ok\n");
    return 0;
}
