"""The marginal LOO predictive checks at the headline size: bnr_chains_marginal_loo_predict over 8 chains (n = 500, V = 100, R = 7; q = 5050) with
a 20 000-row window each and 2 000 draws per chain (thin 10), in three runs that each write their own section of --out (the first writes the
file, the others append):

  (default)   the whole call between two bnr_device_synchronize calls, median of --reps after --warm warm-up calls, beside
              bnr_chains_marginal_loo (device_marginal_loo's call) on the same chains in the same process.  The chains are not sampled: tau2, mu, u,
              lambda and S of every row are loaded from seeded draws, since the time of the call depends on the shapes alone.
  --trace     --trace-reps calls and nothing else, to be run under the profiler:
                  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o mcheck -- python tools/marginal_loo_predict_bench.py --trace
              a later default run takes --kernel-stats DIR and reports the kernels' times per call.
  --fit       a real fit at the headline shape (8 chains, --fit-burn burn-in rows, nsamp sampled rows) with loo_predict and marginal_loo_predict:
              ks, coverage and n_high_k of LOOPredict and of MarginalLOOPredict over chain 1's window.
No time is gated: the file records what was measured."""
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
ap.add_argument("--out", default="profiles/marginal_loo_predict_headline.txt")
ap.add_argument("--nsamp", type=int, default=20000)
ap.add_argument("--draws", type=int, default=2000, help="draws per chain (thin = ceil(nsamp / draws))")
ap.add_argument("--chains", type=int, default=8)
ap.add_argument("--n", type=int, default=500)
ap.add_argument("--V", type=int, default=100)
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--warm", type=int, default=2)
ap.add_argument("--batch", type=int, default=0, help='option "mcheck_batch_draws" (0: automatic)')
ap.add_argument("--trace", action="store_true")
ap.add_argument("--kernel-stats", default=None)
ap.add_argument("--trace-reps", type=int, default=2)
ap.add_argument("--fit", action="store_true")
ap.add_argument("--fit-burn", type=int, default=10000)
a = ap.parse_args()

_capi.mcheck_set_option("mcheck_batch_draws", a.batch)
n, V, R, nsamp, K = a.n, a.V, 7, a.nsamp, a.chains
q = V * (V + 1) // 2
thin = api._marginal_loo_thin(nsamp, a.draws)
nd = -(-nsamp // thin)
D = K * nd
X, y, _ = bnr_amd.make_synthetic(n, V, R, seed=20240501)
p_lo, p_hi = api._loo_interval_probs(95)
lines = []

if a.fit:
    t = time.perf_counter()
    res = bnr_amd.Fit(X, y, R, nburn=a.fit_burn, nsamples=nsamp, num_chains=K, seed=4242, x_transform=False, suppress_timer=True, filename=None,
                      return_state=False, loo_predict=True, marginal_loo_predict=True, marginal_loo_draws=a.draws)
    c, m = res.loo_predictive, res.marginal_loo_predictive
    lines.append("real fit (n %d V %d R %d, %d chains, burn-in %d, nsamp %d, max R-hat gamma %.2f), chain 1's window, %.0f s:"
                 % (n, V, R, K, a.fit_burn, nsamp, float(np.max(res.rhatgamma)), time.perf_counter() - t))
    for name, r in (("LOOPredict", c), ("MarginalLOOPredict", m)):
        lines.append("  %-18s (%6d draws): n_high_k %3d of %d, median k-hat %.2f; ks %.3f, coverage of the %g %% interval %.3f, rmse_loo %.3f, r2_loo %.3f"
                     % (name, r.draws, r.n_high_k, r.pareto_k.size, float(np.median(r.pareto_k)), r.ks, r.interval, r.coverage, r.rmse_loo, r.r2_loo))
    lines.append("  n_bad %d; mean width of the interval: conditional %.3f, marginal %.3f; mean loo_sd: conditional %.3f, marginal %.3f"
                 % (m.n_bad, float(np.mean(c.loo_upper - c.loo_lower)), float(np.mean(m.loo_upper - m.loo_lower)), float(np.mean(c.loo_sd)),
                    float(np.mean(m.loo_sd))))
    print("\n".join(lines), flush=True)
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
    check = lambda: _capi.chains_marginal_loo_predict(chains, 2, nsamp, thin, None, p_lo, p_hi)
    loo = lambda: _capi.chains_marginal_loo(chains, 2, nsamp, thin)
    if a.trace:
        for _ in range(a.trace_reps):
            check()
        for ch in chains:
            ch.close()
        sys.exit(0)

    def timed(call):
        for _ in range(a.warm):
            call()
        ts = []
        for _ in range(a.reps):
            _capi.device_synchronize(0)
            t = time.perf_counter()
            out = call()
            _capi.device_synchronize(0)
            ts.append(time.perf_counter() - t)
        return out, ts

    out, tc = timed(check)
    ref, tl = timed(loo)
    lines.append("marginal_loo_predict_headline: n %d V %d R %d (q = %d), %d chains, window rows 2..%d of each (nsamp %d), thin %d: %d draws per chain, D = %d; "
                 "tau2, mu, u, lambda, S loaded from seeded draws, not sampled (the call's time depends on the shapes alone); n_bad %d"
                 % (n, V, R, q, K, tot, nsamp, thin, nd, D, out[5]))
    lines.append("bnr_chains_marginal_loo_predict, whole call (the marginal kernels, the copy of loglik, bnr_psis_weights, the upload of the weights, the three "
                 "mixture kernels, five n-vectors back), median of %d: %.1f ms (best %.1f, worst %.1f)" % (a.reps, 1e3 * float(np.median(tc)), 1e3 * min(tc), 1e3 * max(tc)))
    lines.append("bnr_chains_marginal_loo on the same chains, same process (loglik, resid and var copied to the host, loo_mean and loo_sd in a host loop), "
                 "median of %d: %.1f ms (best %.1f, worst %.1f)" % (a.reps, 1e3 * float(np.median(tl)), 1e3 * min(tl), 1e3 * max(tl)))
    lines.append("elpd_loo and pareto_k of the two calls equal bit for bit: %s; largest |loo_mean difference| %.2e, largest relative loo_sd difference %.2e"
                 % (bool(np.array_equal(out[0], ref[0]) and np.array_equal(out[1], ref[1])), float(np.max(np.abs(out[2][0] - ref[2]))),
                    float(np.max(np.abs(out[2][1] - ref[3]) / ref[3]))))
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
        for name in ("k_mloo_w", "k_mloo_rhs", "k_mloo_gram", "k_mloo_factor", "k_psis_w", "k_mcheck_stage", "k_mcheck_moments", "k_mcheck_quantile"):
            lines.append("  %-18s %4d launches, %9.2f ms" % (name, cnt(name), 1e3 * pick(name)))
    else:
        lines.append("kernel times: not measured in this run (no --kernel-stats)")
    print("\n".join(lines), flush=True)
    for ch in chains:
        ch.close()
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "a" if a.fit else "w") as f:
    f.write(("\n" if a.fit else "") + "\n".join(lines) + "\n")
