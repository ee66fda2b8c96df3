"""The Rao-Blackwellised covariance of the edge coefficients at the headline size: bnr_chains_marginal_edge_cov over 8 chains (n = 500, V = 100,
R = 7; q = 5050) with a 20 000-row window each and 2 000 draws per chain (thin 10), for all q columns and for one node's V edges, in three runs
that each write their own section (--out):

  (default)   the whole call between two bnr_device_synchronize calls, median of --reps after --warm warm-up calls, for both column sets, beside
              bnr_chains_marginal_edges on the same chains, and the host restatement api._host_marginal_edge_cov on the same tables (--host-draws
              draws per chain; its time per draw times the draws of the device call is what the device call is compared with).  The chains are
              not sampled: tau2, mu, u, lambda and S of every row are loaded from seeded draws, since the time depends on the shapes alone.
  --trace     --reps calls over all q columns and nothing else, to be run under the profiler:
                  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o mcov -- python tools/marginal_edge_cov_bench.py --trace --reps 1
              a later default run takes --kernel-stats DIR and reports the kernels' times per call and k_mcov_gram's share of the 78.6 TFLOP/s
              f64 matrix peak, counting the MFMAs it issues: per tile pair of 128 x 128 entries 2 * 128 * 128 flops for every staged row (the
              within Gram: D rows-rounded-up-to-16 rows; the between Gram: D rows rounded up to 16 per chain).
  --fit       a real fit at the headline shape (8 chains, --fit-burn burn-in rows, nsamp sampled rows) and, for every node's total effect (the
              sum of the V edges that touch the node): its sd from EdgeCov (bnr_chains_cov over the gamma draws of every row of the window) against
              its sd from MarginalEdgeCov (the draws used), and rb_share of the edges."""
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
ap.add_argument("--out", default="profiles/marginal_edge_cov_headline.txt")
ap.add_argument("--nsamp", type=int, default=20000)
ap.add_argument("--draws", type=int, default=2000, help="draws per chain (thin = ceil(nsamp / draws))")
ap.add_argument("--chains", type=int, default=8)
ap.add_argument("--n", type=int, default=500)
ap.add_argument("--V", type=int, default=100)
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--warm", type=int, default=1)
ap.add_argument("--host-draws", type=int, default=4, help="draws per chain of the host restatement")
ap.add_argument("--batch", type=int, default=0, help='option "mcov_batch_draws" (0: automatic)')
ap.add_argument("--trace", action="store_true")
ap.add_argument("--kernel-stats", default=None)
ap.add_argument("--trace-reps", type=int, default=1)
ap.add_argument("--fit", action="store_true")
ap.add_argument("--fit-burn", type=int, default=10000)
a = ap.parse_args()

PEAK = 78.6e12
_capi.mcov_set_option("mcov_batch_draws", a.batch)
n, V, R, nsamp, K = a.n, a.V, 7, a.nsamp, a.chains
q = V * (V + 1) // 2
thin = api._marginal_loo_thin(nsamp, a.draws)
nd = -(-nsamp // thin)
D = K * nd
X, y, _ = bnr_amd.make_synthetic(n, V, R, seed=20240501)
n1, n2 = api._edge_nodes(V, np.arange(q))
node_cols = np.flatnonzero((n1 == 1) | (n2 == 1)).astype(np.int32)        # the V edges of node 1
lines = []

if a.fit:
    keep = []
    t = time.perf_counter()
    res = bnr_amd.generate_samples(X, y, R, nburn=a.fit_burn, nsamp=nsamp, maxburn=a.fit_burn, num_chains=K, seed=4242, x_transform=False,
                                   suppress_timer=True, return_state=False, _keep=keep)
    chains = [keep[0].chains[c] for c in keep[0].ids]
    lines.append("real fit (n %d V %d R %d, %d chains, burn-in %d, nsamp %d, max R-hat gamma %.2f), %.0f s; every chain's window, EdgeCov over every row, "
                 "MarginalEdgeCov over every %d-th: %d draws per chain" % (n, V, R, K, a.fit_burn, nsamp, float(np.max(res.rhatgamma)), time.perf_counter() - t, thin, nd))
    ec = api.device_edge_cov(chains, a.fit_burn, nsamp)
    mc = api.device_marginal_edge_cov(chains, a.fit_burn, nsamp, thin)
    Cn = np.zeros((V, q))
    for k in range(1, V + 1):
        Cn[k - 1, (n1 == k) | (n2 == k)] = 1.0
    sd_e, sd_m = ec.contrast(Cn)["sd"], mc.contrast(Cn)["sd"]
    wi = np.sqrt(np.einsum("ia,ab,ib->i", Cn, mc.within, Cn))
    share = mc.rb_share
    ratio = sd_e / sd_m
    lines.append("  n_bad %d; rb_share = diag(within) / diag(cov) per edge: median %.3f (min %.3f, max %.3f); smallest diag(within) %.3g"
                 % (mc.n_bad, np.nanmedian(share), np.nanmin(share), np.nanmax(share), float(np.min(np.diag(mc.within)))))
    lines.append("  total effect of every node (the sum of its %d edges), sd from EdgeCov / sd from MarginalEdgeCov: median %.3f (min %.3f, max %.3f); sd from "
                 "MarginalEdgeCov: median %.4g; the share of its variance that is `within`: median %.3f (min %.3f, max %.3f)"
                 % (V, np.median(ratio), ratio.min(), ratio.max(), np.median(sd_m), np.median((wi / sd_m) ** 2), ((wi / sd_m) ** 2).min(), ((wi / sd_m) ** 2).max()))
    lines.append("  largest |mean difference| between the two records in posterior sds: %.3f; largest |corr difference| over all pairs: %.3f"
                 % (float(np.max(np.abs(ec.mean - mc.mean) / mc.sd)), float(np.nanmax(np.abs(ec.corr - mc.corr)))))
    print("\n".join(lines), flush=True)
    keep[0].close()
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
    call_all = lambda: _capi.chains_marginal_edge_cov(chains, 2, nsamp, thin)
    call_node = lambda: _capi.chains_marginal_edge_cov(chains, 2, nsamp, thin, node_cols)
    if a.trace:
        for _ in range(a.reps):
            call_all()
        for ch in chains:
            ch.close()
        sys.exit(0)

    def timed(fn, reps=a.reps):
        for _ in range(a.warm):
            fn()
        ts = []
        for _ in range(reps):
            _capi.device_synchronize(0)
            t = time.perf_counter()
            out = fn()
            _capi.device_synchronize(0)
            ts.append(time.perf_counter() - t)
        return ts, out

    ts, out = timed(call_all)
    med = float(np.median(ts))
    tn, outn = timed(call_node)
    te, _ = timed(lambda: _capi.chains_marginal_edges(chains, 2, nsamp, thin))
    rs = -(-n // 16) * 16
    ntp = (lambda nt: nt * (nt + 1) // 2)(-(-q // 128))
    flops = 2.0 * 128 * 128 * ntp * (D * rs + K * (-(-nd // 16) * 16))
    lines.append("marginal_edge_cov_headline: n %d V %d R %d (q = %d), %d chains, window rows 2..%d of each (nsamp %d), thin %d: %d draws per chain, D = %d; tau2, mu, "
                 "u, lambda, S loaded from seeded draws, not sampled (the call's time depends on the shapes alone); n_bad %d" % (n, V, R, q, K, tot, nsamp, thin, nd, D, out[5]))
    lines.append("bnr_chains_marginal_edge_cov, all %d columns, whole call (the marginal kernels, k_mcov_*, k_medge_summary, the copies of mean, cov, within), median "
                 "of %d: %.1f ms (best %.1f, worst %.1f)" % (q, a.reps, 1e3 * med, 1e3 * min(ts), 1e3 * max(ts)))
    lines.append("bnr_chains_marginal_edge_cov, the %d edges of node 1, median of %d: %.1f ms (best %.1f, worst %.1f); its entries equal the all-column call's bit for "
                 "bit: %s" % (node_cols.size, a.reps, 1e3 * float(np.median(tn)), 1e3 * min(tn), 1e3 * max(tn),
                              bool(np.array_equal(outn[1], out[1][np.ix_(node_cols, node_cols)]) and np.array_equal(outn[2], out[2][np.ix_(node_cols, node_cols)]))))
    lines.append("bnr_chains_marginal_edges on the same chains, same commit, median of %d: %.1f ms (best %.1f, worst %.1f)"
                 % (a.reps, 1e3 * float(np.median(te)), 1e3 * min(te), 1e3 * max(te)))
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
        lines.append("kernel times, all %d columns (rocprofv3 --kernel-trace --stats, a run of its own: %d calls, per call):" % (q, a.trace_reps))
        for name in ("k_mloo_w", "k_mloo_rhs", "k_mloo_gram", "k_mloo_factor", "k_mcov_proj", "k_mcov_gram", "k_medge_summary", "k_mcov_center", "k_mcov_finish"):
            lines.append("  %-16s %5d launches, %9.2f ms" % (name, cnt(name), 1e3 * pick(name)))
        tg = pick("k_mcov_gram")
        if tg > 0:
            lines.append("  k_mcov_gram: %.3g flops issued as MFMAs per call = %.2f TFLOP/s = %.1f %% of the %.1f TFLOP/s f64 matrix peak"
                         % (flops, flops / tg * 1e-12, 100 * flops / tg / PEAK, PEAK * 1e-12))
    else:
        lines.append("kernel times: not measured in this run (no --kernel-stats)")
    print("\n".join(lines), flush=True)
    hthin = -(-nsamp // a.host_draws)
    hnd = -(-nsamp // hthin)
    dev = _capi.chains_marginal_edge_cov(chains, 2, nsamp, hthin)
    for ch in chains:
        ch.close()
    Xd = np.asarray(X, dtype=np.float64)
    t = time.perf_counter()
    h = api._host_marginal_edge_cov([table] * K, Xd, y, 1, nsamp, hthin)
    th = time.perf_counter() - t
    per = th / (K * hnd)
    lines.append("host restatement api._host_marginal_edge_cov (numpy, OMP_NUM_THREADS=%s) on the same tables, %d draws per chain (%d in all): %.2f s = %.3f s per "
                 "draw; the %d draws of the device call at that rate: %.0f s = %.0f x the device call"
                 % (os.environ.get("OMP_NUM_THREADS", "?"), hnd, K * hnd, th, per, D, per * D, per * D / med))
    lines.append("device against host on those %d draws: max |cov difference| %.2e, max |within difference| %.2e (largest |cov| %.2e)"
                 % (K * hnd, float(np.max(np.abs(dev[1] - h.cov))), float(np.max(np.abs(dev[2] - h.within))), float(np.max(np.abs(h.cov)))))
    print("\n".join(lines[-2:]), flush=True)
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "w") as f:
    f.write("\n".join(lines) + "\n")
