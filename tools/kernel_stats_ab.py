"""dev helper: two rocprofv3 `--kernel-trace --stats` kernel_stats.csv files (before, after) of the same benchmark command ->
time per network forward of every kernel, side by side.  The number of forwards of a run is the call count of the read-out kernel.
    python tools/kernel_stats_ab.py before_kernel_stats.csv after_kernel_stats.csv [min_us]
"""
import csv
import re
import sys


def load(path):
    rows = {}
    for r in csv.DictReader(open(path)):
        name = re.sub(r"\(.*", "", r["Name"]).replace("void dsg::", "")
        rows[name] = (int(r["Calls"]), float(r["TotalDurationNs"]))
    fwd = max(c for n, (c, _) in rows.items() if n.startswith("fused_readout96_kernel"))
    return rows, fwd


a, fa = load(sys.argv[1])
b, fb = load(sys.argv[2])
min_us = float(sys.argv[3]) if len(sys.argv) > 3 else 1.0
print(f"forwards: before {fa}, after {fb}")
print(f"{'kernel':58s} {'calls/fwd':>9s} {'before us/fwd':>13s} {'calls/fwd':>9s} {'after us/fwd':>13s}")
ta = tb = 0.0
for name in sorted(set(a) | set(b), key=lambda n: -(a.get(n, (0, 0.0))[1] / fa + b.get(n, (0, 0.0))[1] / fb)):
    ca, na = a.get(name, (0, 0.0))
    cb, nb = b.get(name, (0, 0.0))
    ua, ub = na / fa / 1e3, nb / fb / 1e3
    ta += ua
    tb += ub
    if max(ua, ub) >= min_us:
        print(f"{name[:58]:58s} {ca / fa:9.2f} {ua:13.1f} {cb / fb:9.2f} {ub:13.1f}")
print(f"{'all kernels':58s} {'':9s} {ta:13.1f} {'':9s} {tb:13.1f}")
