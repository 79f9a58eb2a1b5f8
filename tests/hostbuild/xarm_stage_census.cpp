// Reset census per hand-off stage of the staged PickAndPlace step (DESIGN.md 4b "Resets per hand-off stage"), on the host, float32
// cooperative core with the XC_ROW_CENSUS counting hook (as xarm_row_census.cpp): the resets of list B - episodes that ended in a step
// that carried pad rows - split by the stage of the step's FIRST pad-carrying substep, which is the stage whose hand-off steps the env
// on the device:  B0 substeps 0-4, B1 substeps 5-9, B2 substeps 10-14;  list A: the step carried no pad row.
// Per class, per env and for the union of 4 consecutive events of the class (one device wavefront): how many of a reset's 90 substeps
// carry pad rows, and a MODELLED length of the reset from that.  E envs under random actions with auto-reset, episode phases spread as
// bench.py spreads them.  Built and run by tools/row_census.py --stages; a stand-alone program.
//   xarm_stage_census [envs, default 256] [steps, default 150]
#define XARM_HOST_BUILD 1
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
namespace census { void record(bool pad, bool la, const bool *padw, int np, const bool *law, int nla); }
#define XC_ROW_CENSUS(pad, la, padw, law) census::record(pad, la, padw, NP, law, NLA);
#include "../../gym_xarm_amd/csrc/xarm_core.h"
#include "../../gym_xarm_amd/csrc/xarm_coop_core.h"

namespace census {
// one mask per substep: bits 0-3 live pads
std::vector<uint8_t> *sink = nullptr;
void record(bool pad, bool, const bool *padw, int np, const bool *, int) {
    uint8_t m = 0;
    for (int p = 0; p < np; p++) if (pad && padw[p]) m |= (uint8_t)(1u << p);
    if (sink) sink->push_back(m);
}
}  // namespace census

namespace {
template <typename T> struct HostLds { T *base; T &operator[](int i) const { return base[i]; } };
uint64_t rng_state = 1234;
double uni() {   // splitmix64 -> uniform [-1, 1)
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; z ^= z >> 31;
    return (double)(z >> 11) / 4503599627370496.0 - 1.0;
}
typedef std::vector<uint8_t> Event;   // the pad masks of the substeps of one reset (90) or one step (15)

// THE MODEL (profiles/r07a_pnp_pad_setup.txt): a pad substep of the cooperative core is about 14.7 k instructions, a pad-free one 9.4 k,
// a lone wavefront retires one instruction per 4.35 cycles at 2.4 GHz: 90 pad substeps = 2.40 ms, what k_reset_coop of list B takes
const double K_PAD = 14.7e3, K_FREE = 9.4e3, CPI = 4.35, MHZ = 2400.0;
double model_us(long pad, long all) { return ((double)pad * K_PAD + (double)(all - pad) * K_FREE) * CPI / MHZ; }

// the union of up to 4 consecutive events: the row set a wavefront of 4 such envs runs
std::vector<Event> unions4(const std::vector<Event> &ev) {
    std::vector<Event> out;
    for (size_t i = 0; i < ev.size(); i += 4) {
        Event u = ev[i];
        for (size_t j = i + 1; j < i + 4 && j < ev.size(); j++)
            for (size_t k = 0; k < u.size(); k++) u[k] |= ev[j][k];
        out.push_back(u);
    }
    return out;
}
// returns the modelled length of the slowest event (0: none)
double table_row(const char *name, const std::vector<Event> &ev) {
    long n = 0, pad_sum = 0, pad_max = 0, ge45 = 0, ge80 = 0, four = 0;
    double us_sum = 0, us_max = 0;
    for (const Event &e : ev) {
        long p = 0;
        for (uint8_t m : e) { p += m != 0; four += m == 15; }
        n++; pad_sum += p;
        if (p > pad_max) pad_max = p;
        ge45 += p >= 45; ge80 += p >= 80;
        const double us = model_us(p, (long)e.size());
        us_sum += us;
        if (us > us_max) us_max = us;
    }
    if (!n) { printf("| %s | 0 | | | | | | | |\n", name); return 0; }
    printf("| %s | %ld | %.1f | %ld | %ld | %ld | %.0f | %.0f | %.0f |\n", name, n, (double)pad_sum / n, pad_max, ge45, ge80,
           pad_sum ? 100.0 * four / pad_sum : 0.0, us_sum / n, us_max);
    return us_max;
}
}  // namespace

int main(int argc, char **argv) {
    typedef float T;
    const int E = argc > 1 ? atoi(argv[1]) : 256, STEPS = argc > 2 ? atoi(argv[2]) : 150;
    static_assert(xm::PNP_N_SUBSTEPS == 15, "three stages of five substeps");
    xk::EnvCfg cfg; memset(&cfg, 0, sizeof cfg);
    std::vector<xk::EnvState<T>> st(E);
    T lds[xk::LDS_FLOATS]; HostLds<T> L{lds};
    for (int e = 0; e < E; e++) {
        xk::env_init<T>(cfg, e, st[e]);
        xc::env_reset<T>(xc::Grp(), cfg, e, st[e], L);
        st[e].steps = (T)((int64_t)e * 7919 % xm::PNP_MAX_EPISODE_STEPS);   // bench.py --episode-phase desync
    }
    std::vector<Event> cls[4];   // A, B0, B1, B2
    long resets = 0, handed[3] = {0, 0, 0}, steps_all = 0;
    for (int s = 0; s < STEPS; s++)
        for (int e = 0; e < E; e++) {
            T a[4], o[xk::OBS_DIM], r; bool d, su;
            for (int k = 0; k < 4; k++) a[k] = (T)uni();
            Event ev;
            census::sink = &ev;
            xc::env_step<T>(xc::Grp(), cfg, st[e], a, o, r, d, su, L);
            steps_all++;
            int first = -1;
            for (size_t k = 0; k < ev.size() && first < 0; k++) if (ev[k]) first = (int)k;
            const int c = first < 0 ? 0 : 1 + first / 5;
            if (c) handed[c - 1]++;
            if (d) {
                Event rv;
                census::sink = &rv;
                xc::env_reset<T>(xc::Grp(), cfg, e, st[e], L);
                cls[c].push_back(rv);
                resets++;
            }
            census::sink = nullptr;
        }
    printf("stage census: %d envs, %d steps, float32 host cooperative core, random actions, auto-reset, desynchronised phases\n", E, STEPS);
    printf("%ld env steps; first pad-carrying substep in 0-4: %ld, 5-9: %ld, 10-14: %ld\n", steps_all, handed[0], handed[1], handed[2]);
    printf("resets: %ld = A %zu + B0 %zu + B1 %zu + B2 %zu\n", resets, cls[0].size(), cls[1].size(), cls[2].size(), cls[3].size());
    printf("MODEL of a reset's length: pad substeps x %.1f k + pad-free substeps x %.1f k instructions, %.2f cycles per instruction at %.1f GHz "
           "(constants from profiles/r07a_pnp_pad_setup.txt; 90 pad substeps = %.0f us, none = %.0f us)\n",
           K_PAD / 1e3, K_FREE / 1e3, CPI, MHZ / 1e3, model_us(90, 90), model_us(0, 90));
    printf("| resets | n | pad substeps per reset: mean | max | resets with >= 45 | >= 80 | all four pads live (%% of pad substeps) | modelled us: mean | max |\n");
    printf("|---|---|---|---|---|---|---|---|---|\n");
    static const char *names[4] = {"A", "B0", "B1", "B2"};
    double slow[4] = {0, 0, 0, 0};
    for (int c = 0; c < 4; c++) {
        char nm[64];
        snprintf(nm, sizeof nm, "%s, per env", names[c]);
        table_row(nm, cls[c]);
        snprintf(nm, sizeof nm, "%s, union of 4", names[c]);
        slow[c] = table_row(nm, unions4(cls[c]));
    }
    // what the decision rule of DESIGN.md 4b compares: the slowest wavefront of each stage's reset
    printf("slowest union of 4, modelled us: B0 %.0f, B1 %.0f (B0 - B1 = %.0f; its hand-off ends 83 us after hand-off 0), "
           "B2 %.0f (B0 - B2 = %.0f; its hand-off ends 184 us after hand-off 0)\n",
           slow[1], slow[2], slow[1] - slow[2], slow[3], slow[1] - slow[3]);
    return 0;
}
