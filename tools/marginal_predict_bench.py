"""Rao-Blackwellised prediction of new rows at the headline size: bnr_chains_marginal_predict over 8 chains (n = 500, V = 100, R = 7; q = 5050)
with a 20 000-row window each, 2 000 draws per chain (thin 10) and 500 held-out rows from synthetic.py, in three runs that each write their own
section (--out):

  (default)   the whole call between two bnr_device_synchronize calls, median of --reps after --warm warm-up calls, beside
              bnr_chains_marginal_edges on the same chains, and the host restatement api._host_marginal_predict's terms on the same tables
              (--host-draws draws in all; its time per draw times the draws of the device call is what the device call is compared with).  The
              chains are not sampled: tau2, mu, u, lambda and S of every row are loaded from seeded draws, since the time depends on the shapes
              alone.
  --trace     --reps calls and nothing else, to be run under the profiler:
                  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o mpred -- python tools/marginal_predict_bench.py --trace --reps 2
              a later default run takes --kernel-stats DIR and reports the kernels' times per call and k_mpred_cross's share of the 78.6 TFLOP/s
              f64 matrix peak, counting the MFMAs it issues: per draw 2 * np * 32 ceil(m / 32) * 32 ceil(q / 32) flops, np = 32 ceil(n / 32).
  --fit       a real fit at the headline shape (8 chains, --fit-burn burn-in rows, nsamp sampled rows) and, over every chain's window (the draws
              device_predict_pooled pools, thinned alike): per held-out row the share var_within / sd^2 and the batch-means variance (30 batches
              per chain set) of the posterior mean from the draws mu + x* . gamma against that of their conditional means; and the batch-means
              variance of the held-out elpd, log-mean-exp over the gamma draws against the mixture's."""
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
ap.add_argument("--out", default="profiles/marginal_predict_headline.txt")
ap.add_argument("--nsamp", type=int, default=20000)
ap.add_argument("--draws", type=int, default=2000, help="draws per chain (thin = ceil(nsamp / draws))")
ap.add_argument("--chains", type=int, default=8)
ap.add_argument("--n", type=int, default=500)
ap.add_argument("--V", type=int, default=100)
ap.add_argument("--m", type=int, default=500, help="held-out rows")
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--warm", type=int, default=2)
ap.add_argument("--host-draws", type=int, default=32, help="draws of the host restatement, in all")
ap.add_argument("--batch", type=int, default=0, help='option "mpred_batch_draws" (0: automatic)')
ap.add_argument("--block", type=int, default=0, help='option "mpred_block_rows" (0: automatic)')
ap.add_argument("--trace", action="store_true")
ap.add_argument("--kernel-stats", default=None)
ap.add_argument("--trace-reps", type=int, default=2)
ap.add_argument("--fit", action="store_true")
ap.add_argument("--fit-burn", type=int, default=10000)
a = ap.parse_args()

PEAK = 78.6e12
_capi.mpred_set_option("mpred_batch_draws", a.batch)
_capi.mpred_set_option("mpred_block_rows", a.block)
n, V, R, nsamp, K, m = a.n, a.V, 7, a.nsamp, a.chains, a.m
q = V * (V + 1) // 2
thin = api._marginal_loo_thin(nsamp, a.draws)
nd = -(-nsamp // thin)
D = K * nd
Xall, yall, _ = bnr_amd.make_synthetic(n + m, V, R, seed=20240501)      # one data set: the first n rows train, the last m are held out
Xall, yall = np.asarray(Xall, dtype=np.float64), np.asarray(yall, dtype=np.float64).reshape(-1)
X, y, Xn, yn = Xall[:n], yall[:n], Xall[n:], yall[n:]
lines = []

if a.fit:
    keep = []
    t = time.perf_counter()
    res = bnr_amd.generate_samples(X, y, R, nburn=a.fit_burn, nsamp=nsamp, maxburn=a.fit_burn, num_chains=K, seed=4242, x_transform=False,
                                   suppress_timer=True, return_state=False, _keep=keep)
    chains = [keep[0].chains[c] for c in keep[0].ids]
    lines.append("real fit (n %d V %d R %d, %d chains, burn-in %d, nsamp %d, max R-hat gamma %.2f), %.0f s; every chain's window, every %d-th row: %d draws "
                 "per chain, %d held-out rows" % (n, V, R, K, a.fit_burn, nsamp, float(np.max(res.rhatgamma)), time.perf_counter() - t, thin, nd, m))
    mp_ = api.device_marginal_predict(chains, a.fit_burn, nsamp, Xn, yn, thin, per_draw=True)
    pooled = api.device_predict_pooled(chains, a.fit_burn, nsamp, Xn, yn)
    eta, t2 = np.empty((D, m)), np.empty(D)
    step = 1000 // thin * thin or thin
    for k, ch in enumerate(chains):                                         # mu + x* . gamma of the rows used, a block of rows at a time
        for r0 in range(0, nsamp, step):
            tab = ch.fetch(a.fit_burn + 1 + r0, a.fit_burn + min(r0 + step, nsamp))
            g, mu = tab["gamma"][::thin, :, 0], tab["mu"][::thin, 0, 0]
            lo = k * nd + r0 // thin
            eta[lo:lo + g.shape[0]] = mu[:, None] + g @ Xn.T
            t2[lo:lo + g.shape[0]] = tab["tau2"][::thin, 0, 0]
    nb = 30
    use = nd // nb * nb
    per = use // nb

    def batches(x):
        """(nb, K per, ...): batch b holds draws b per .. (b + 1) per - 1 of every chain"""
        x = x.reshape((K, nd) + x.shape[1:])[:, :use].reshape((K, nb, per) + x.shape[1:])
        return np.moveaxis(x, 0, 1).reshape((nb, K * per) + x.shape[3:])

    bm = lambda x: batches(x).mean(axis=1).var(axis=0, ddof=1)
    ratio = bm(eta) / bm(mp_.mean)

    def lme(l):
        mx = l.max(axis=1, keepdims=True)
        return (mx + np.log(np.mean(np.exp(l - mx), axis=1, keepdims=True)))[:, 0]

    ldraw = -0.5 * (np.log(2 * np.pi) + np.log(t2))[:, None] - 0.5 * (yn[None, :] - eta) ** 2 / t2[:, None]
    vo = mp_.var + t2[:, None]
    lmix = -0.5 * (np.log(2 * np.pi) + np.log(vo)) - 0.5 * (yn[None, :] - mp_.mean) ** 2 / vo
    e_draw, e_mix = lme(batches(ldraw)).sum(axis=1), lme(batches(lmix)).sum(axis=1)
    share = mp_.rb_share
    lines.append("  n_bad %d; var_within / sd^2 per held-out row: median %.3f (min %.3f, max %.3f)" % (mp_.n_bad, np.median(share), share.min(), share.max()))
    lines.append("  batch-means variance of the posterior mean of a row (%d batches of %d draws from each of %d chains), mu + x* . gamma / conditional means: "
                 "median ratio %.2f (min %.2f, max %.2f), ratio > 1 on %d of %d rows" % (nb, per, K, np.median(ratio), ratio.min(), ratio.max(), int(np.sum(ratio > 1)), m))
    lines.append("  held-out elpd (%d rows): device_predict_pooled %.2f (all %d rows of every window), the mixture %.2f (%d draws); batch-means variance over the %d "
                 "batches: log-mean-exp over the gamma draws %.3f, the mixture %.3f, ratio %.2f; batch elpd: draws %.2f .. %.2f, mixture %.2f .. %.2f"
                 % (m, pooled.elpd, nsamp, mp_.elpd, D, nb, e_draw.var(ddof=1), e_mix.var(ddof=1), e_draw.var(ddof=1) / e_mix.var(ddof=1), e_draw.min(), e_draw.max(),
                    e_mix.min(), e_mix.max()))
    lines.append("  largest |Rao-Blackwellised mean - mean of the draws| in posterior sds of the row: %.3f; rmse against y*: draws %.4f, mixture %.4f"
                 % (float(np.max(np.abs(mp_.estimate - eta.mean(axis=0)) / eta.std(axis=0))), float(np.sqrt(np.mean((eta.mean(axis=0) - yn) ** 2))),
                    float(np.sqrt(np.mean((mp_.estimate - yn) ** 2)))))
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
    call = lambda: _capi.chains_marginal_predict(chains, 2, nsamp, Xn, yn, thin)
    if a.trace:
        for _ in range(a.reps):
            call()
        for ch in chains:
            ch.close()
        sys.exit(0)

    def timed(fn):
        for _ in range(a.warm):
            fn()
        ts = []
        for _ in range(a.reps):
            _capi.device_synchronize(0)
            t = time.perf_counter()
            out = fn()
            _capi.device_synchronize(0)
            ts.append(time.perf_counter() - t)
        return ts, out

    ts, out = timed(call)
    med = float(np.median(ts))
    te, _ = timed(lambda: _capi.chains_marginal_edges(chains, 2, nsamp, thin))
    r32 = lambda v: -(-v // 32) * 32
    flops = 2.0 * r32(n) * r32(m) * r32(q) * D
    lines.append("marginal_predict_headline: n %d V %d R %d (q = %d), %d held-out rows, %d chains, window rows 2..%d of each (nsamp %d), thin %d: %d draws per chain, "
                 "D = %d; tau2, mu, u, lambda, S loaded from seeded draws, not sampled (the call's time depends on the shapes alone); n_bad %d"
                 % (n, V, R, q, m, K, tot, nsamp, thin, nd, D, out[3]))
    lines.append("bnr_chains_marginal_predict, whole call (the marginal kernels, k_mpred_rhs / cross / proj, two k_medge_summary, k_mpred_score, the copies), "
                 "median of %d: %.1f ms (best %.1f, worst %.1f)" % (a.reps, 1e3 * med, 1e3 * min(ts), 1e3 * max(ts)))
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
        lines.append("kernel times (rocprofv3 --kernel-trace --stats, a run of its own: %d calls, per call):" % a.trace_reps)
        for name in ("k_mloo_w", "k_mloo_rhs", "k_mloo_gram", "k_mloo_factor", "k_mpred_rhs", "k_mpred_cross", "k_mpred_proj", "k_medge_summary", "k_mpred_score"):
            lines.append("  %-16s %4d launches, %9.2f ms" % (name, cnt(name), 1e3 * pick(name)))
        tp = pick("k_mpred_cross")
        if tp > 0:
            lines.append("  k_mpred_cross: %.3g flops issued as MFMAs per call = %.2f TFLOP/s = %.1f %% of the %.1f TFLOP/s f64 matrix peak"
                         % (flops, flops / tp * 1e-12, 100 * flops / tp / PEAK, PEAK * 1e-12))
    else:
        lines.append("kernel times: not measured in this run (no --kernel-stats)")
    print("\n".join(lines), flush=True)
    hper = max(1, a.host_draws // K)
    hthin = -(-nsamp // hper)
    hnd = -(-nsamp // hthin)
    dev = _capi.chains_marginal_predict(chains, 2, nsamp, Xn, yn, hthin, per_draw=True)
    for ch in chains:
        ch.close()
    t = time.perf_counter()
    hm, hv, _hb = api._host_predict_terms(X, y, Xn, *api._host_marginal_draws([table] * K, 1, nsamp, hthin))
    th = time.perf_counter() - t
    per = th / (K * hnd)
    lines.append("host restatement api._host_predict_terms (numpy, OMP_NUM_THREADS=%s) on the same tables, %d draws per chain (%d in all): %.2f s = %.3f s per draw; "
                 "the %d draws of the device call at that rate: %.0f s = %.0f x the device call" % (os.environ.get("OMP_NUM_THREADS", "?"), hnd, K * hnd, th, per, D, per * D, per * D / med))
    lines.append("device against host on those %d draws: max |mean difference| %.2e, max |var difference| %.2e"
                 % (K * hnd, float(np.max(np.abs(dev[1] - hm))), float(np.max(np.abs(dev[2] - hv)))))
    print("\n".join(lines[-2:]), flush=True)
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "w") as f:
    f.write("\n".join(lines) + "\n")
