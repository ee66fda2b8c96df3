"""Marginal PSIS-LOO at the headline size: bnr_chains_marginal_loo over 8 chains (n = 500, V = 100, R = 7; q = 5050) with a 20 000-row window
each and 2 000 draws per chain (thin 10), in three runs that each write their own section (--out):

  (default)   the whole call between two bnr_device_synchronize calls, median of --reps after --warm warm-up calls, and the host restatement
              api._host_marginal_loglik on the same tables with the threads the environment gives it (OMP_NUM_THREADS) -- on --host-draws draws
              per chain, since all of them would take it many minutes: its time per draw times the draws of the device call is what the
              device call is compared with.  The chains are not sampled: tau2, mu, u, lambda and S of every row are loaded from seeded draws,
              since the time of the call depends on the shapes alone.
  --trace     --reps calls and nothing else, to be run under the profiler:
                  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o mloo -- python tools/marginal_loo_bench.py --trace --reps 2
              a later default run takes --kernel-stats DIR and reports the four kernels' times per call and k_mloo_gram's share of the 78.6
              TFLOP/s f64 matrix peak, counting the MFMAs it issues: 2 q 32^2 nt (nt + 1) / 2 flops per draw, nt = ceil(n / 32).
  --fit       a real fit at the headline shape (8 chains, --fit-burn burn-in rows, nsamp sampled rows): n_high_k, median and maximum k-hat of
              LOO and of MarginalLOO over chain 1's window and over the pooled windows."""
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
ap.add_argument("--out", default="profiles/marginal_loo_headline.txt")
ap.add_argument("--nsamp", type=int, default=20000)
ap.add_argument("--draws", type=int, default=2000, help="draws per chain (thin = ceil(nsamp / draws))")
ap.add_argument("--chains", type=int, default=8)
ap.add_argument("--n", type=int, default=500)
ap.add_argument("--V", type=int, default=100)
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--warm", type=int, default=2)
ap.add_argument("--host-draws", type=int, default=4, help="draws per chain of the host restatement")
ap.add_argument("--batch", type=int, default=0, help='option "mloo_batch_draws" (0: automatic)')
ap.add_argument("--trace", action="store_true")
ap.add_argument("--kernel-stats", default=None)
ap.add_argument("--trace-reps", type=int, default=2)
ap.add_argument("--fit", action="store_true")
ap.add_argument("--fit-burn", type=int, default=10000)
a = ap.parse_args()

PEAK = 78.6e12
_capi.mloo_set_option("mloo_batch_draws", a.batch)
n, V, R, nsamp, K = a.n, a.V, 7, a.nsamp, a.chains
q = V * (V + 1) // 2
thin = api._marginal_loo_thin(nsamp, a.draws)
nd = -(-nsamp // thin)
D = K * nd
X, y, _ = bnr_amd.make_synthetic(n, V, R, seed=20240501)
lines = []


def stats(k):
    return "n_high_k %d of %d, median k-hat %.2f, max %.2f" % (int(np.sum(k > 0.7)), k.size, float(np.median(k)), float(np.max(k)))


if a.fit:
    for pool in (False, True):
        t = time.perf_counter()
        res = bnr_amd.Fit(X, y, R, nburn=a.fit_burn, nsamples=nsamp, num_chains=K, seed=4242, x_transform=False, suppress_timer=True, filename=None,
                          return_state=False, loo=True, marginal_loo=True, marginal_loo_draws=a.draws, pool_chains=pool)
        lo, ml = res.loo, res.marginal_loo
        lines.append("real fit (n %d V %d R %d, %d chains, burn-in %d, nsamp %d, max R-hat gamma %.2f), %s, %.0f s:"
                     % (n, V, R, K, a.fit_burn, nsamp, float(np.max(res.rhatgamma)), "pooled windows of all chains" if pool else "chain 1's window",
                        time.perf_counter() - t))
        lines.append("  LOO         (%6d draws): %s, elpd_loo %.1f, p_loo %.1f" % (nsamp * res.stat_chains, stats(lo["pareto_k"]), lo["elpd_loo"], lo["p_loo"]))
        lines.append("  MarginalLOO (%6d draws): %s, elpd_loo %.1f, p_loo %.1f, rmse_loo %.3f, r2_loo %.3f, n_bad %d"
                     % (ml["draws"], stats(ml["pareto_k"]), ml["elpd_loo"], ml["p_loo"], ml["rmse_loo"], ml["r2_loo"], ml["n_bad"]))
        print("\n".join(lines[-3:]), flush=True)
else:
    tot = nsamp + 1
    chains = [bnr_amd.Chain(X, y, R, tot, 4242, 1)]
    chains += [bnr_amd.Chain.like(chains[0], 4242, c) for c in range(2, K + 1)]
    rng = np.random.default_rng(20241020)
    S = np.empty((tot, q, 1), order="F")
    for e in range(q):                                    # (column by column: no second copy of the matrix)
        S[:, e, 0] = rng.standard_exponential(tot)
    table = dict(tau2=np.asfortranarray(rng.standard_exponential((tot, 1, 1)) + 0.5), mu=np.asfortranarray(rng.standard_normal((tot, 1, 1))),
                 u=np.asfortranarray(rng.standard_normal((tot, R, V)) * 0.3), lam=np.asfortranarray(rng.integers(-1, 2, size=(tot, R, 1)).astype(np.float64)),
                 S=S)
    for ch in chains:
        ch.load(table)
    call = lambda: _capi.chains_marginal_loo(chains, 2, nsamp, thin)
    if a.trace:
        for _ in range(a.reps):
            call()
        for ch in chains:
            ch.close()
        sys.exit(0)
    for _ in range(a.warm):
        call()
    ts = []
    for _ in range(a.reps):
        _capi.device_synchronize(0)
        t = time.perf_counter()
        out = call()
        _capi.device_synchronize(0)
        ts.append(time.perf_counter() - t)
    med = float(np.median(ts))
    nt = -(-n // 32)
    gflop = 2.0 * q * 32 * 32 * nt * (nt + 1) / 2 * D
    lines.append("marginal_loo_headline: n %d V %d R %d (q = %d), %d chains, window rows 2..%d of each (nsamp %d), thin %d: %d draws per chain, D = %d; tau2, mu, u, "
                 "lambda, S loaded from seeded draws, not sampled (the call's time depends on the shapes alone); n_bad %d" % (n, V, R, q, K, tot, nsamp, thin, nd, D, out[6]))
    lines.append("bnr_chains_marginal_loo, whole call (kernels, the copies of the n x D matrices, bnr_psis_weights, the host sums), median of %d: %.1f ms (best %.1f, "
                 "worst %.1f)" % (a.reps, 1e3 * med, 1e3 * min(ts), 1e3 * max(ts)))
    if a.kernel_stats:
        files = sorted(glob.glob(os.path.join(a.kernel_stats, "**", "*kernel_stats.csv"), recursive=True))
        if not files:
            raise SystemExit("no *kernel_stats.csv under %s" % a.kernel_stats)
        tot_ns, ncall = {}, {}
        for row in csv.DictReader(open(files[0])):
            tot_ns[row["Name"]] = tot_ns.get(row["Name"], 0.0) + float(row["TotalDurationNs"])
            ncall[row["Name"]] = ncall.get(row["Name"], 0) + int(row["Calls"])
        pick = lambda key: sum(v for kk, v in tot_ns.items() if key in kk) / a.trace_reps * 1e-9
        cnt = lambda key: sum(v for kk, v in ncall.items() if key in kk) // a.trace_reps
        lines.append("kernel times (rocprofv3 --kernel-trace --stats, a run of its own: %d calls, per call):" % a.trace_reps)
        for name in ("k_mloo_w", "k_mloo_rhs", "k_mloo_gram", "k_mloo_factor", "k_psis_w"):
            lines.append("  %-14s %4d launches, %9.2f ms" % (name, cnt(name), 1e3 * pick(name)))
        tg = pick("k_mloo_gram")
        if tg > 0:
            lines.append("  k_mloo_gram: %.3g flops issued as MFMAs per call = %.2f TFLOP/s = %.1f %% of the %.1f TFLOP/s f64 matrix peak"
                         % (gflop, gflop / tg * 1e-12, 100 * gflop / tg / PEAK, PEAK * 1e-12))
    else:
        lines.append("kernel times: not measured in this run (no --kernel-stats)")
    print("\n".join(lines), flush=True)
    hthin = -(-nsamp // a.host_draws)
    hnd = -(-nsamp // hthin)
    dev = _capi.chains_marginal_loo(chains, 2, nsamp, hthin, loglik=True)
    for ch in chains:
        ch.close()
    Xd = np.asarray(X, dtype=np.float64)
    t = time.perf_counter()
    h = api._host_marginal_loglik([table] * K, Xd, y, 1, nsamp, hthin)
    th = time.perf_counter() - t
    per = th / (K * hnd)
    lines.append("host restatement api._host_marginal_loglik (numpy, OMP_NUM_THREADS=%s) on the same tables, %d draws per chain (%d in all): %.2f s = %.3f s per draw; "
                 "the %d draws of the device call at that rate: %.0f s = %.0f x the device call" % (os.environ.get("OMP_NUM_THREADS", "?"), hnd, K * hnd, th, per, D, per * D, per * D / med))
    lines.append("device against host on those %d draws: max |loglik difference| %.2e, max relative logml difference %.2e"
                 % (K * hnd, float(np.max(np.abs(dev[5] - h[0]))), float(np.max(np.abs(dev[4] - h[3]) / np.abs(h[3])))))
    print("\n".join(lines[-2:]), flush=True)
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "w") as f:
    f.write("\n".join(lines) + "\n")
