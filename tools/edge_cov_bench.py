"""The posterior covariance of the edge coefficients at the headline size: bnr_chains_cov over 8 chains (n = 500, V = 100, R = 7; q = 5050 edge
columns) with a 20 000-row window each, all q columns and a 256-column subset, each timed between two bnr_device_synchronize calls (median of
--reps calls after --warm warm-up calls), and the host fallback api._host_edge_cov on the same tables, once.

The chains are not sampled: every chain's gamma rows are loaded from one seeded matrix of normal draws (column scales 1e-3 .. 1e1), since the
time of the call depends on the shapes alone -- this keeps the traced run (below) free of the sweep's launches and the host within memory.

Kernel times come from a run of their own under the profiler (section 4 of the measuring notes):
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o cov -- python tools/edge_cov_bench.py --trace --reps 3
makes --reps calls of each shape and nothing else; the timing run then takes --kernel-stats DIR, reads the *kernel_stats.csv there and reports
k_cov's time per call and its share of the 78.6 TFLOP/s f64 matrix peak, counting S ncols (ncols + 1) flops.  Writes --out (default
profiles/edge_cov_headline.txt)."""
import argparse
import csv
import glob
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import bnr_amd
from bnr_amd import _capi, api

ap = argparse.ArgumentParser()
ap.add_argument("--out", default="profiles/edge_cov_headline.txt")
ap.add_argument("--nsamp", type=int, default=20000)
ap.add_argument("--chains", type=int, default=8)
ap.add_argument("--V", type=int, default=100)
ap.add_argument("--subset", type=int, default=256)
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--warm", type=int, default=2)
ap.add_argument("--trace", action="store_true", help="the run under the profiler: --reps calls of each shape, nothing else, no file written")
ap.add_argument("--kernel-stats", default=None, help="directory of a --trace run's rocprofv3 output")
ap.add_argument("--trace-reps", type=int, default=3, help="the --reps of the --trace run behind --kernel-stats")
ap.add_argument("--no-host", action="store_true", help="skip the host fallback")
a = ap.parse_args()

PEAK = 78.6e12
n, V, R, nsamp, K = 500, a.V, 7, a.nsamp, a.chains
q, tot = V * (V + 1) // 2, nsamp + 1
S = K * nsamp
X, y, _ = bnr_amd.make_synthetic(n, V, R, seed=20240501)
chains = [bnr_amd.Chain(X, y, R, tot, 4242, 1)]
chains += [bnr_amd.Chain.like(chains[0], 4242, c) for c in range(2, K + 1)]
rng = np.random.default_rng(20240917)
gamma = np.empty((tot, q, 1), order="F")
scale = np.logspace(-3, 1, q)
for e in range(q):                                        # (column by column: no second copy of the matrix)
    gamma[:, e, 0] = rng.standard_normal(tot) * scale[e]
table = dict(tau2=np.ones((tot, 1, 1), order="F"), gamma=gamma)
for ch in chains:
    ch.load(table)
cols = np.sort(rng.choice(q, size=min(a.subset, q), replace=False))
dev = 0
calls = {"all": lambda: _capi.pooled_cov(chains, 2, nsamp), "subset": lambda: _capi.pooled_cov(chains, 2, nsamp, cols)}


def once(f):
    _capi.device_synchronize(dev)
    t = time.perf_counter()
    f()
    _capi.device_synchronize(dev)
    return time.perf_counter() - t


def close():
    for ch in chains:
        ch.close()


if a.trace:
    for _ in range(a.reps):
        for f in calls.values():
            f()
    close()
    sys.exit(0)

for f in calls.values():
    for _ in range(a.warm):
        f()
ts = {k: [] for k in calls}
for _ in range(a.reps):
    for k, f in calls.items():
        ts[k].append(once(f))
med = {k: float(np.median(v)) for k, v in ts.items()}
ncol = {"all": q, "subset": cols.size}
flops = {k: float(S) * m * (m + 1) for k, m in ncol.items()}
lines = ["edge_cov_headline: n %d V %d R %d (q = %d edge columns), %d chains, window rows 2..%d of each (nsamp %d, S = %d pooled draws); gamma rows loaded "
         "from seeded normal draws, not sampled (the call's time depends on the shapes alone)" % (n, V, R, q, K, tot, nsamp, S)]
for k, label in (("all", "bnr_chains_cov, all %d columns" % q), ("subset", "bnr_chains_cov, %d columns" % cols.size)):
    lines.append("%-40s whole call, median of %d: %9.1f ms (best %9.1f, worst %9.1f); S ncols (ncols + 1) = %.3g flops"
                 % (label, a.reps, 1e3 * med[k], 1e3 * min(ts[k]), 1e3 * max(ts[k]), flops[k]))
if a.kernel_stats:
    files = sorted(glob.glob(os.path.join(a.kernel_stats, "**", "*kernel_stats.csv"), recursive=True))
    if not files:
        raise SystemExit("no *kernel_stats.csv under %s" % a.kernel_stats)
    tot_ns = {}
    for row in csv.DictReader(open(files[0])):
        tot_ns[row["Name"]] = tot_ns.get(row["Name"], 0.0) + float(row["TotalDurationNs"])
    calls_of = {}
    for row in csv.DictReader(open(files[0])):
        calls_of[row["Name"]] = calls_of.get(row["Name"], 0) + int(row["Calls"])
    nlaunch = lambda key: sum(v for kk, v in calls_of.items() if key in kk) // a.trace_reps
    pick = lambda key: sum(v for kk, v in tot_ns.items() if key in kk) / a.trace_reps * 1e-9
    kc = {"all": pick("k_cov<4>") + pick("k_covILi4E"), "subset": pick("k_cov<2>") + pick("k_covILi2E")}
    rest = {kk: pick(kk) for kk in ("k_cov_finish", "k_summary", "k_fetch_cols")}
    lines.append("kernel times (rocprofv3 --kernel-trace --stats, a run of its own: %d calls of each shape, per call):" % a.trace_reps)
    for k, name in (("all", "k_cov<4>"), ("subset", "k_cov<2>")):
        if kc[k] > 0:
            lines.append("  %-10s (%s, %d launches per call): %9.2f ms = %6.2f TFLOP/s = %5.1f %% of the %.1f TFLOP/s f64 matrix peak"
                         % (name, "all columns" if k == "all" else "%d columns" % cols.size, nlaunch(name), 1e3 * kc[k],
                            flops[k] / kc[k] * 1e-12, 100 * flops[k] / kc[k] / PEAK, PEAK * 1e-12))
    lines.append("  both shapes together, per call of each: k_cov_finish %.2f ms, k_summary (the centres) %.2f ms, k_fetch_cols (their staging) %.2f ms"
                 % tuple(1e3 * rest[kk] for kk in ("k_cov_finish", "k_summary", "k_fetch_cols")))
else:
    lines.append("kernel times: not measured in this run (no --kernel-stats)")
got = _capi.pooled_cov(chains, 2, nsamp, cols)
close()
if not a.no_host:
    print("\n".join(lines), flush=True)
    tables = [table] * K
    t = time.perf_counter()
    sub = api._host_edge_cov(tables, 1, nsamp, cols)
    th_sub = time.perf_counter() - t
    print("host subset done in %.1f s" % th_sub, flush=True)
    t = time.perf_counter()
    full = api._host_edge_cov(tables, 1, nsamp)
    th = time.perf_counter() - t
    d = np.sqrt(np.diag(sub.cov))
    err = float(np.max(np.abs(got[1] - sub.cov) / np.outer(d, d)))
    threads = os.environ.get("OMP_NUM_THREADS", "?")
    lines.append("host fallback api._host_edge_cov (numpy, OMP_NUM_THREADS=%s) on the same tables: all columns %.1f s = %.0f x the device call; %d columns %.2f s "
                 "= %.0f x" % (threads, th, th / med["all"], cols.size, th_sub, th_sub / med["subset"]))
    lines.append("device against host on the %d columns: max |difference| / (sd_a sd_b) = %.2e; mean bit for bit: %s"
                 % (cols.size, err, np.array_equal(got[0], sub.mean)))
    del full
print("\n".join(lines))
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "w") as f:
    f.write("\n".join(lines) + "\n")
