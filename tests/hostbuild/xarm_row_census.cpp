// Row-set census of the cooperative PickAndPlace core (gym_xarm_amd/csrc/xarm_coop_core.h) on the host, float32:
// which row sets - finger-pad rows (slot 2), arm-limit rows (slot 3) - the substeps of a reset and of a pad-touching
// step carry, and how many pads / arm-limit rows are live in them, per env and for the union of 4 envs (one device
// wavefront).  E envs under random actions with auto-reset, episode phases spread as bench.py spreads them.
// Built and run by tools/row_census.py; a stand-alone program, never loaded by the product package or the tests.
//   xarm_row_census [envs, default 256] [steps, default 150]
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
// one mask per substep: bits 0-3 live pads, bits 4-10 live arm-limit rows
std::vector<uint16_t> *sink = nullptr;
void record(bool pad, bool la, const bool *padw, int np, const bool *law, int nla) {
    uint16_t m = 0;
    for (int p = 0; p < np; p++) if (pad && padw[p]) m |= (uint16_t)(1u << p);
    for (int i = 0; i < nla; i++) if (la && law[i]) m |= (uint16_t)(16u << i);
    if (sink) sink->push_back(m);
}
}  // namespace census

namespace {
template <typename T> struct HostLds { T *base; T &operator[](int i) const { return base[i]; } };
int popc(unsigned x) { int n = 0; for (; x; x &= x - 1) n++; return n; }
uint64_t rng_state = 1234;
double uni() {   // splitmix64 -> uniform [-1, 1)
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; z ^= z >> 31;
    return (double)(z >> 11) / 4503599627370496.0 - 1.0;
}
typedef std::vector<uint16_t> Event;   // the masks of the substeps of one reset (90) or one step (15)
struct Tally {
    long n = 0, sub = 0, none = 0, pad_only = 0, la_only = 0, both = 0, any_both = 0, any_pad = 0;
    long pads[5] = {0, 0, 0, 0, 0}, laws[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    double max_both = 0, max_pad = 0;
    void add(const Event &e) {
        long b = 0, p = 0;
        for (uint16_t m : e) {
            const int np = popc(m & 15u), nl = popc(m >> 4);
            sub++;
            if (np && nl) both++; else if (np) pad_only++; else if (nl) la_only++; else none++;
            if (np) { pads[np]++; p++; }
            if (np && nl) b++;
            if (np) laws[nl]++;
        }
        n++;
        any_both += b > 0; any_pad += p > 0;
        if ((double)b / e.size() > max_both) max_both = (double)b / e.size();
        if ((double)p / e.size() > max_pad) max_pad = (double)p / e.size();
    }
    void print(const char *name) const {
        if (!n) { printf("| %s | 0 | | | | | | | | |\n", name); return; }
        const double s = 100.0 / sub, pd = pad_only + both ? 100.0 / (pad_only + both) : 0.0;
        printf("| %s | %ld | %.1f | %.1f | %.1f | %.1f | %.0f / %.0f | %.0f / %.0f | %.0f / %.0f / %.0f / %.0f | %.0f / %.0f / %.0f / %.0f |\n", name, n,
               none * s, pad_only * s, la_only * s, both * s, 100.0 * any_pad / n, 100.0 * any_both / n, 100 * max_pad, 100 * max_both,
               pads[1] * pd, pads[2] * pd, pads[3] * pd, pads[4] * pd, laws[0] * pd, laws[1] * pd, laws[2] * pd,
               (laws[3] + laws[4] + laws[5] + laws[6] + laws[7]) * pd);
    }
};
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
void table_row(const char *name, const std::vector<Event> &ev) {
    Tally t; for (const Event &e : ev) t.add(e);
    t.print(name);
}
}  // namespace

int main(int argc, char **argv) {
    typedef float T;
    const int E = argc > 1 ? atoi(argv[1]) : 256, STEPS = argc > 2 ? atoi(argv[2]) : 150;
    xk::EnvCfg cfg; memset(&cfg, 0, sizeof cfg);
    std::vector<xk::EnvState<T>> st(E);
    T lds[xk::LDS_FLOATS]; HostLds<T> L{lds};
    for (int e = 0; e < E; e++) {
        xk::env_init<T>(cfg, e, st[e]);
        xc::env_reset<T>(xc::Grp(), cfg, e, st[e], L);
        st[e].steps = (T)((int64_t)e * 7919 % xm::PNP_MAX_EPISODE_STEPS);   // bench.py --episode-phase desync
    }
    std::vector<Event> step_pad, reset_a, reset_b;
    long steps_all = 0;
    for (int s = 0; s < STEPS; s++)
        for (int e = 0; e < E; e++) {
            T a[4], o[xk::OBS_DIM], r; bool d, su;
            for (int k = 0; k < 4; k++) a[k] = (T)uni();
            Event ev;
            census::sink = &ev;
            xc::env_step<T>(xc::Grp(), cfg, st[e], a, o, r, d, su, L);
            steps_all++;
            bool pad = false;
            for (uint16_t m : ev) pad = pad || (m & 15u);
            if (pad) step_pad.push_back(ev);
            if (d) {
                // list B of the device: the episode ended in a step that carried pad rows (a hand-off); list A: the others
                Event rv;
                census::sink = &rv;
                xc::env_reset<T>(xc::Grp(), cfg, e, st[e], L);
                (pad ? reset_b : reset_a).push_back(rv);
            }
            census::sink = nullptr;
        }
    printf("row-set census: %d envs, %d steps, float32 host cooperative core, random actions, auto-reset, desynchronised phases\n", E, STEPS);
    printf("%ld env steps, %zu of them pad-touching (%.1f %%); %zu resets: %zu after a pad-free step (list A), %zu after a pad-touching step (list B)\n",
           steps_all, step_pad.size(), 100.0 * step_pad.size() / steps_all, reset_a.size() + reset_b.size(), reset_a.size(), reset_b.size());
    printf("| events | n | %% substeps no extra rows | pad only | arm-limit only | pad + arm-limit | %% events with a pad / a pad + arm-limit substep | max %% of an event's substeps pad / pad + arm-limit | live pads 1 / 2 / 3 / 4 (%% of pad substeps) | live arm-limit rows 0 / 1 / 2 / 3+ (%% of pad substeps) |\n");
    printf("|---|---|---|---|---|---|---|---|---|---|\n");
    table_row("reset, list A, per env", reset_a);
    table_row("reset, list A, union of 4", unions4(reset_a));
    table_row("reset, list B, per env", reset_b);
    table_row("reset, list B, union of 4", unions4(reset_b));
    table_row("pad-touching step, per env", step_pad);
    table_row("pad-touching step, union of 4", unions4(step_pad));
    return 0;
}
