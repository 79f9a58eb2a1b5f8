"""Per-launch timeline of the staged PickAndPlace step from a rocprofv3 --kernel-trace run of bench.py.

  python tools/probes/pnp_stage_timeline.py <rocprofv3 output dir> <fast stages per call> [calls to average, default 10]

A call starts at every n-th launch of the fast kernel (k_step_fast_stage; n = 1 for the unstaged pipeline, XARM_PNP_STAGES=1).  Every kernel of the
library that starts before the next call's first fast launch belongs to it.  Printed: start and end of each launch relative
to the call's first launch, the median over the last calls of the trace (keyed by kernel name and its ordinal within the
call), then the span of the call and when its last reset launch began."""
import csv
import glob
import re
import statistics
import sys


def short(name):
    m = re.search(r"(k_[a-z_0-9]+)", name)
    return m.group(1) if m else None


def main():
    path = glob.glob(sys.argv[1] + "/**/*kernel_trace.csv", recursive=True)[0]
    nst = int(sys.argv[2])
    ncall = int(sys.argv[3]) if len(sys.argv) > 3 else 10
    rows = []
    for r in csv.DictReader(open(path)):
        n = short(r["Kernel_Name"])
        if n and (n.startswith("k_step") or n.startswith("k_reset")):
            rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), n, r.get("Grid_Size_X", r.get("Grid_Size", "?"))))
    rows.sort()
    fast = [i for i, r in enumerate(rows) if r[2] == "k_step_fast_stage"]
    heads = fast[::nst]
    heads = heads[-(ncall + 1):]           # the last one only closes the call before it
    per_key, order, spans, last_reset = {}, [], [], []
    for a, b in zip(heads[:-1], heads[1:]):
        t0, seen = rows[a][0], {}
        for s, e, n, g in rows[a:b]:
            k = (n, seen.get(n, 0))
            seen[n] = k[1] + 1
            if k not in per_key:
                per_key[k] = []
                order.append(k)
            per_key[k].append(((s - t0) / 1e3, (e - t0) / 1e3, g))
        spans.append((max(r[1] for r in rows[a:b]) - t0) / 1e3)
        rs = [r for r in rows[a:b] if r[2].startswith("k_reset")]
        # the reset the call waits for: the one that ends last
        last_reset.append((max(rs, key=lambda r: r[1])[0] - t0) / 1e3 if rs else float("nan"))
    print("%-28s %3s %10s %10s %10s %8s  (median of %d calls, us from the call's first launch)" % ("kernel", "#", "start", "end", "dur", "grid", len(spans)))
    order.sort(key=lambda k: statistics.median(x[0] for x in per_key[k]))
    for k in order:
        v = per_key[k]
        s, e = statistics.median(x[0] for x in v), statistics.median(x[1] for x in v)
        d = statistics.median(x[1] - x[0] for x in v)
        print("%-28s %3d %10.1f %10.1f %10.1f %8s" % (k[0], k[1], s, e, d, v[-1][2]))
    print("call span: median %.1f us (min %.1f, max %.1f); the reset that ends last starts at %.1f us" % (
        statistics.median(spans), min(spans), max(spans), statistics.median(last_reset)))


if __name__ == "__main__":
    main()
