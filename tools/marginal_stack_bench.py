"""Chain stacking on the marginal PSIS-LOO at the headline size: bnr_chains_marginal_stack over 8 chains (n = 500, V = 100, R = 7; q = 5050) with
2 000 draws per chain, in three runs that each write their own section of --out (the first writes the file, the others append):

  (default)   the whole call between two bnr_device_synchronize calls, median of --reps after --warm warm-up calls; beside it, on the same chains
              in the same process, bnr_chains_marginal_loo_predict (the one-pass call the new one extends by K - 1 PSIS set-ups, a host repack
              and one staging kernel) and device_marginal_loo(per_chain=True) + stacking_weights (the route to the same weights by hand: K + 1
              passes; --route-reps calls).  The chains are not sampled: tau2, mu, u, lambda and S of every row are loaded from seeded draws,
              different ones per chain, since the time of the call depends on the shapes alone.
  --trace     --trace-reps calls and nothing else, to be run under the profiler:
                  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o mstack -- python tools/marginal_stack_bench.py --trace
              a later default run takes --kernel-stats DIR and reports the kernels' times per call.
  --fit       a real fit at the headline shape (8 chains, --fit-burn burn-in rows, --fit-nsamp sampled rows) with stack_chains, marginal_stack,
              marginal_loo_predict (pooled) and marginal_predict of --fresh fresh rows from the same truth: both weight vectors, n_high_k per
              chain under both, elpd_stack against elpd_uniform, ks and coverage of the stacked LOO predictive beside the pooled one, and the
              held-out elpd under the uniform, conditional and marginal weights.
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
ap.add_argument("--out", default="profiles/marginal_stack_headline.txt")
ap.add_argument("--nsamp", type=int, default=2000)
ap.add_argument("--draws", type=int, default=2000, help="draws per chain (thin = ceil(nsamp / draws))")
ap.add_argument("--chains", type=int, default=8)
ap.add_argument("--n", type=int, default=500)
ap.add_argument("--V", type=int, default=100)
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--warm", type=int, default=1)
ap.add_argument("--route-reps", type=int, default=3)
ap.add_argument("--batch", type=int, default=0, help='option "mstack_batch_draws" (0: automatic)')
ap.add_argument("--trace", action="store_true")
ap.add_argument("--kernel-stats", default=None)
ap.add_argument("--trace-reps", type=int, default=2)
ap.add_argument("--fit", action="store_true")
ap.add_argument("--fit-burn", type=int, default=10000)
ap.add_argument("--fit-nsamp", type=int, default=20000)
ap.add_argument("--fresh", type=int, default=400)
a = ap.parse_args()

_capi.mstack_set_option("mstack_batch_draws", a.batch)
n, V, R, K = a.n, a.V, 7, a.chains
q = V * (V + 1) // 2
X, y, truth = bnr_amd.make_synthetic(n, V, R, seed=20240501)
p_lo, p_hi = api._loo_interval_probs(95)
lines = []
fmt = lambda v: "[" + " ".join("%.6g" % x for x in v) + "]"

if a.fit:
    nsamp = a.fit_nsamp
    rng = np.random.default_rng(20241021)
    Xf = np.asfortranarray((rng.random((a.fresh, q)) < 0.5) * np.abs(rng.standard_normal((a.fresh, q))))    # make_synthetic's rows, the same truth
    yf = 10.0 + Xf @ truth["B"] + rng.standard_normal(a.fresh)
    t = time.perf_counter()
    res = bnr_amd.Fit(X, y, R, nburn=a.fit_burn, nsamples=nsamp, num_chains=K, seed=4242, x_transform=False, suppress_timer=True, filename=None,
                      return_state=False, stack_chains=True, marginal_stack=True, marginal_loo_predict=True, pool_chains=True, marginal_loo_draws=a.draws,
                      predict_X=Xf, predict_y=yf, marginal_predict=True, marginal_predict_draws=a.draws)
    c, m, pooled = res.stacking, res.marginal_stacking, res.marginal_loo_predictive
    lines.append("real fit (n %d V %d R %d, %d chains, burn-in %d, nsamp %d, max R-hat gamma %.2f), every chain's window, %d draws per chain for the "
                 "marginal calls, %.0f s:" % (n, V, R, K, a.fit_burn, nsamp, float(np.max(res.rhatgamma)), m.draws // K, time.perf_counter() - t))
    for name, r in (("conditional (Stacking)", c), ("marginal (MarginalStack)", m)):
        lines.append("  %-25s weights %s" % (name, fmt(r.weights)))
        lines.append("  %-25s n_high_k per chain (of %d) %s; elpd per chain %s" % ("", r.pareto_k.shape[1], list(map(int, r.n_high_k)), fmt(r.elpd_chain)))
        lines.append("  %-25s elpd_stack %.2f (se %.2f) against elpd_uniform %.2f over %d rows; gap %.3g after %d solver updates"
                     % ("", r.elpd_stack, r.se, r.elpd_uniform, r.n_used, r.gap, r.iterations))
    lines.append("  stacked LOO predictive (marginal weights): ks %.3f, coverage of the %g %% interval %.3f, rmse_loo %.3f, r2_loo %.3f, n_bad %d"
                 % (m.ks, m.interval, m.coverage, m.rmse_loo, m.r2_loo, m.n_bad))
    lines.append("  pooled MarginalLOOPredict (%d draws): ks %.3f, coverage %.3f, rmse_loo %.3f, r2_loo %.3f, n_high_k %d"
                 % (pooled.draws, pooled.ks, pooled.coverage, pooled.rmse_loo, pooled.r2_loo, pooled.n_high_k))
    held = [("uniform (pooled)", res.marginal_prediction), ("conditional weights", c.marginal_prediction), ("marginal weights", m.marginal_prediction)]
    lines.append("  held-out elpd of device_marginal_predict on %d fresh rows from the same truth: %s"
                 % (a.fresh, "; ".join("%s %.2f" % (name, float(np.sum(p.lpd))) for name, p in held)))
    print("\n".join(lines), flush=True)
else:
    nsamp = a.nsamp
    thin = api._marginal_loo_thin(nsamp, a.draws)
    nd = -(-nsamp // thin)
    D = K * nd
    tot = nsamp + 1
    chains = [bnr_amd.Chain(X, y, R, tot, 4242, 1)]
    chains += [bnr_amd.Chain.like(chains[0], 4242, c) for c in range(2, K + 1)]
    for k, ch in enumerate(chains):
        rng = np.random.default_rng([20241021, k])
        S = np.empty((tot, q, 1), order="F")
        for e in range(q):                                    # (column by column: no second copy of the matrix)
            S[:, e, 0] = rng.standard_exponential(tot)
        ch.load(dict(tau2=np.asfortranarray(rng.standard_exponential((tot, 1, 1)) + 0.5), mu=np.asfortranarray(rng.standard_normal((tot, 1, 1))),
                     u=np.asfortranarray(rng.standard_normal((tot, R, V)) * 0.3),
                     lam=np.asfortranarray(rng.integers(-1, 2, size=(tot, R, 1)).astype(np.float64)), S=S))
    stack = lambda: _capi.chains_marginal_stack(chains, 2, nsamp, thin, None, None, 100000, 1e-9, p_lo, p_hi)
    check = lambda: _capi.chains_marginal_loo_predict(chains, 2, nsamp, thin, None, p_lo, p_hi)

    def route():
        r = api.device_marginal_loo(chains, 1, nsamp, thin, per_chain=True)
        return r, api.stacking_weights(r["elpd_chain"].T)

    if a.trace:
        for _ in range(a.trace_reps):
            stack()
        for ch in chains:
            ch.close()
        sys.exit(0)

    def timed(call, warm, reps):
        for _ in range(warm):
            call()
        ts = []
        for _ in range(reps):
            _capi.device_synchronize(0)
            t = time.perf_counter()
            out = call()
            _capi.device_synchronize(0)
            ts.append(time.perf_counter() - t)
        return out, ts

    out, ts = timed(stack, a.warm, a.reps)
    ref, tc = timed(check, a.warm, a.reps)
    (rt, sw), tr = timed(route, 0, a.route_reps)
    ms = lambda v: "%.1f ms (best %.1f, worst %.1f)" % (1e3 * float(np.median(v)), 1e3 * min(v), 1e3 * max(v))
    lines.append("marginal_stack_headline: n %d V %d R %d (q = %d), %d chains, window rows 2..%d of each (nsamp %d), thin %d: %d draws per chain, D = %d; "
                 "tau2, mu, u, lambda, S loaded from seeded draws (per chain), not sampled (the call's time depends on the shapes alone); n_bad %d"
                 % (n, V, R, q, K, tot, nsamp, thin, nd, D, out[8]))
    lines.append("bnr_chains_marginal_stack, whole call (the marginal kernels once over all chains, the copy of loglik, the repack, %d bnr_psis_weights, the "
                 "solver, the upload of the weights, the staging kernel and the two row kernels, five n-vectors back), median of %d: %s"
                 % (K, a.reps, ms(ts)))
    lines.append("bnr_chains_marginal_loo_predict on the same chains, same process (one pass, one PSIS over all D draws), median of %d: %s" % (a.reps, ms(tc)))
    lines.append("device_marginal_loo(per_chain=True) + stacking_weights on the same chains, same process (%d passes), median of %d: %s"
                 % (K + 1, a.route_reps, ms(tr)))
    lines.append("weights %s, gap %.3g after %d solver updates; equal to the by-hand route's bit for bit: weights %s, elpd_chain %s, pareto_k_chain %s"
                 % (fmt(out[0]), out[4], out[5], bool(np.array_equal(out[0], sw["weights"])), bool(np.array_equal(out[1], rt["elpd_chain"])),
                    bool(np.array_equal(out[2], rt["pareto_k_chain"]))))
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
        for name in ("k_mloo_w", "k_mloo_rhs", "k_mloo_gram", "k_mloo_factor", "k_psis_w", "k_mstack_stage", "k_mcheck_moments", "k_mcheck_quantile"):
            lines.append("  %-18s %4d launches, %9.2f ms" % (name, cnt(name), 1e3 * pick(name)))
    else:
        lines.append("kernel times: not measured in this run (no --kernel-stats)")
    print("\n".join(lines), flush=True)
    for ch in chains:
        ch.close()
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "a" if a.fit else "w") as f:
    f.write(("\n" if a.fit else "") + "\n".join(lines) + "\n")
