// Host (g++ -ffp-contract=off) instantiation of gym_xarm_amd/csrc/xarm_norm_core.h for the CPU-side tests ONLY (tests/test_norm_host.py,
// tests/test_norm_gpu.py, and norm_main.cpp for the sanitizer run).  Never loaded by the product package: gym_xarm_amd normalises
// through libxarm_hip.so (xarm_k_norm.hip).  The three launches run here one after the other, each workgroup's threads as plain
// loops over the same (column, segment) items and the same per-env functions, on NumPy / malloc'd memory.
#define XARM_HOST_BUILD 1
#include <vector>
#include "../../gym_xarm_amd/csrc/xarm_norm_core.h"

using namespace xnorm;

static void run_partial(const Args &a) {
    const Layout &L = a.L;
    const int nc = ncols(a);
    std::vector<float> tile((size_t)CHUNK * nc);
    std::vector<double> segv((size_t)NSEG * nc), meanv(nc);
    uint8_t kf[CHUNK];
    for (int64_t c = 0; c < L.chunks; c++) {
        const int64_t r0 = c * CHUNK;
        const int rows = (int)(L.E - r0 < CHUNK ? L.E - r0 : CHUNK);
        int64_t fin = 0;
        if (a.step)
            for (int r = 0; r < rows; r++) fin += a.done[r0 + r] != 0;
        a.fin[c] = fin;
        if (!a.update) continue;
        for (int r = 0; r < CHUNK; r++) {
            kf[r] = r < rows && kept(a, r0 + r) ? 1 : 0;
            if (r >= rows) continue;
            for (int j = 0; j < L.D; j++) tile[r * nc + j] = obs_at(a, r0 + r, j);
            if (a.step) tile[r * nc + L.D] = ret_next(a.ret[r0 + r], a.gamma, a.rew[r0 + r]);
        }
        int n = 0;
        for (int s = 0; s < NSEG; s++) n += seg_count(kf, s * SEG, s * SEG + SEG);
        for (int i = 0; i < NSEG * nc; i++) segv[i] = seg_sum(tile.data(), nc, i % nc, kf, (i / nc) * SEG, (i / nc) * SEG + SEG);
        for (int j = 0; j < nc; j++) meanv[j] = n > 0 ? seg_combine(segv.data() + j, nc) / (double)n : 0.0;
        for (int i = 0; i < NSEG * nc; i++) segv[i] = seg_sq(tile.data(), nc, i % nc, kf, (i / nc) * SEG, (i / nc) * SEG + SEG, meanv[i % nc]);
        double *p = a.part + c * L.W;
        p[0] = (double)n;
        for (int j = 0; j < nc; j++) {
            p[1 + j] = meanv[j];
            p[1 + (L.D + 1) + j] = seg_combine(segv.data() + j, nc);
        }
    }
}

static void run_merge(const Args &a) {
    const Layout &L = a.L;
    if (a.update) {
        const double obs_count = a.stats[2 * L.D + 2], ret_count = a.stats[2 * L.D + 3];
        for (int j = 0; j < ncols(a); j++) {
            const double n = merge_column(a, j, j < L.D ? obs_count : ret_count);
            if (n > 0.0 && j == 0) a.stats[2 * L.D + 2] = obs_count + n;
            if (n > 0.0 && j == L.D) a.stats[2 * L.D + 3] = ret_count + n;
        }
    }
    if (!a.step) return;
    int64_t before = 0;
    for (int64_t c = 0; c < L.chunks; c++) {
        a.prefix[c] = before;
        before += a.fin[c];
    }
    a.n_base[0] = a.n[0];
    a.n[0] += before;
}

static void run_apply(const Args &a) {
    const Layout &L = a.L;
    std::vector<double> denomv(L.D);
    for (int j = 0; j < L.D; j++) denomv[j] = sqrt(a.stats[L.D + j] + a.eps);
    for (int64_t c = 0; c < L.chunks; c++) {
        const int64_t r0 = c * CHUNK;
        const int rows = (int)(L.E - r0 < CHUNK ? L.E - r0 : CHUNK);
        int64_t rank = a.step ? a.prefix[c] : 0;
        for (int r = 0; r < rows; r++) {
            const int64_t e = r0 + r;
            if (a.step) {
                apply_env(a, e, rank, sqrt(a.stats[2 * L.D + 1] + a.eps));
                rank += a.done[e] != 0 ? 1 : 0;         // env order: the next finished env of the call takes the next row
            } else if (a.zero_ret) {
                a.ret[e] = 0.0f;
            }
            for (int j = 0; j < L.D; j++) a.nobs[e * L.D + j] = norm_value(obs_at(a, e, j), a.stats[j], denomv[j], a.clip_obs);
        }
    }
}

static int run(Args &a, const xarm_norm_layout *l, const xarm_norm_params *p, void *work) {
    if (layout_error(l) || params_error(p)) return -1;
    a.L = make_layout(*l);
    if (a.L.E == 0) return 0;
    a.clip_obs = p->clip_obs; a.clip_rew = p->clip_reward; a.eps = p->eps; a.gamma = p->gamma; a.t_seconds = p->t_seconds;
    a.update = p->update != 0;
    carve_work(a, work);
    if (a.update || a.step) {
        run_partial(a);
        run_merge(a);
    }
    run_apply(a);
    return 0;
}

extern "C" {

int64_t nh_work_bytes(const xarm_norm_layout *l) { return layout_error(l) ? -1 : work_bytes(make_layout(*l)); }
int nh_chunk(void) { return CHUNK; }

int nh_obs(const xarm_norm_layout *l, const xarm_norm_params *p, double *stats, float *ret, void *work, const float *obs, const float *ag,
           const float *dg, int32_t zero_ret, float *out_nobs) {
    Args a = {};
    a.step = 0; a.zero_ret = zero_ret != 0;
    a.stats = stats; a.ret = ret; a.obs = obs; a.ag = ag; a.dg = dg; a.nobs = out_nobs;
    return run(a, l, p, work);
}

int nh_step(const xarm_norm_layout *l, const xarm_norm_params *p, double *stats, float *ret, float *ep_ret, float *ep_len, float *ring,
            int64_t *n, void *work, const float *obs, const float *ag, const float *dg, const float *rew, const uint8_t *done,
            const uint8_t *keep, float *out_nobs, float *out_nrew) {
    Args a = {};
    a.step = 1;
    a.stats = stats; a.ret = ret; a.ep_ret = ep_ret; a.ep_len = ep_len; a.ring = ring; a.n = n;
    a.obs = obs; a.ag = ag; a.dg = dg; a.rew = rew; a.done = done; a.keep = keep; a.nobs = out_nobs; a.nrew = out_nrew;
    return run(a, l, p, work);
}

}  // extern "C"
