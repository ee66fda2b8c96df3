"""Rao-Blackwellised edge summaries at the headline size: bnr_chains_marginal_edges over 8 chains (n = 500, V = 100, R = 7; q = 5050) with a
20 000-row window each and 2 000 draws per chain (thin 10), in three runs that each write their own section (--out):

  (default)   the whole call between two bnr_device_synchronize calls, median of --reps after --warm warm-up calls, beside
              bnr_chains_marginal_loo on the same chains, and the host restatement api._host_marginal_gamma on the same tables (--host-draws
              draws per chain; its time per draw times the draws of the device call is what the device call is compared with).  The chains are
              not sampled: tau2, mu, u, lambda and S of every row are loaded from seeded draws, since the time depends on the shapes alone.
  --trace     --reps calls and nothing else, to be run under the profiler:
                  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o medge -- python tools/marginal_edges_bench.py --trace --reps 2
              a later default run takes --kernel-stats DIR and reports the kernels' times per call and k_medge_proj's share of the 78.6 TFLOP/s
              f64 matrix peak, counting the MFMAs it issues: per draw and block of 128 edges 2 * 128 * 16 * kk(rt) flops for every 16-row tile
              rt of L^-1, kk(rt) = the first multiple of 32 that is >= 16 (rt + 1).
  --fit       a real fit at the headline shape (8 chains, --fit-burn burn-in rows, nsamp sampled rows) and, per edge over chain 1's window: the
              share var_within / sd^2, the batch-means variance (30 batches) of the posterior mean from the gamma draws of the rows used
              against that of their conditional means m, and the edges whose counted sign probability is exactly 0 or 1 with the mixture's lfsr."""
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
ap.add_argument("--out", default="profiles/marginal_edges_headline.txt")
ap.add_argument("--nsamp", type=int, default=20000)
ap.add_argument("--draws", type=int, default=2000, help="draws per chain (thin = ceil(nsamp / draws))")
ap.add_argument("--chains", type=int, default=8)
ap.add_argument("--n", type=int, default=500)
ap.add_argument("--V", type=int, default=100)
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--warm", type=int, default=2)
ap.add_argument("--host-draws", type=int, default=4, help="draws per chain of the host restatement")
ap.add_argument("--batch", type=int, default=0, help='option "medge_batch_draws" (0: automatic)')
ap.add_argument("--trace", action="store_true")
ap.add_argument("--kernel-stats", default=None)
ap.add_argument("--trace-reps", type=int, default=2)
ap.add_argument("--fit", action="store_true")
ap.add_argument("--fit-burn", type=int, default=10000)
a = ap.parse_args()

PEAK = 78.6e12
_capi.medge_set_option("medge_batch_draws", a.batch)
n, V, R, nsamp, K = a.n, a.V, 7, a.nsamp, a.chains
q = V * (V + 1) // 2
thin = api._marginal_loo_thin(nsamp, a.draws)
nd = -(-nsamp // thin)
D = K * nd
X, y, _ = bnr_amd.make_synthetic(n, V, R, seed=20240501)
lines = []

if a.fit:
    keep = []
    t = time.perf_counter()
    res = bnr_amd.generate_samples(X, y, R, nburn=a.fit_burn, nsamp=nsamp, maxburn=a.fit_burn, num_chains=K, seed=4242, x_transform=False,
                                   suppress_timer=True, return_state=False, _keep=keep)
    ch = keep[0].chains[1]
    lines.append("real fit (n %d V %d R %d, %d chains, burn-in %d, nsamp %d, max R-hat gamma %.2f), %.0f s; chain 1's window, every %d-th row: %d draws"
                 % (n, V, R, K, a.fit_burn, nsamp, float(np.max(res.rhatgamma)), time.perf_counter() - t, thin, nd))
    me = api.device_marginal_edges([ch], a.fit_burn, nsamp, thin, per_draw=True)
    g = np.empty((nd, q))
    step = 1000 // thin * thin or thin
    for r0 in range(0, nsamp, step):                                       # the gamma draws of the rows used, a block of rows at a time
        tab = ch.fetch(a.fit_burn + 1 + r0, a.fit_burn + min(r0 + step, nsamp))
        rows = tab["gamma"][::thin, :, 0]
        g[r0 // thin:r0 // thin + rows.shape[0]] = rows
    nb = 30
    use = nd // nb * nb
    bm = lambda x: x[:use].reshape(nb, use // nb, -1).mean(axis=1).var(axis=0, ddof=1)
    ratio = bm(g) / bm(me.m)
    share = me.rb_share
    counted = np.minimum((g > 0).mean(axis=0), (g < 0).mean(axis=0))
    hard = counted == 0
    lines.append("  n_bad %d; var_within / sd^2 per edge: median %.3f (min %.3f, max %.3f)" % (me.n_bad, np.median(share), share.min(), share.max()))
    lines.append("  batch-means variance of the posterior mean (%d batches of %d draws), gamma draws / conditional means: median ratio %.2f (min %.2f, max %.2f), "
                 "ratio > 1 on %d of %d edges" % (nb, use // nb, np.median(ratio), ratio.min(), ratio.max(), int(np.sum(ratio > 1)), q))
    lines.append("  edges whose counted sign probability is exactly 0 or 1: %d of %d; the mixture's lfsr on them: min %.3g, median %.3g, max %.3g"
                 % (int(hard.sum()), q, *((me.lfsr[hard].min(), np.median(me.lfsr[hard]), me.lfsr[hard].max()) if hard.any() else (np.nan,) * 3)))
    lines.append("  largest |Rao-Blackwellised mean - mean of the draws| in posterior sds: %.3f" % float(np.max(np.abs(me.estimate - g.mean(axis=0)) / g.std(axis=0))))
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
    call = lambda: _capi.chains_marginal_edges(chains, 2, nsamp, thin)
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
    tl, _ = timed(lambda: _capi.chains_marginal_loo(chains, 2, nsamp, thin))
    nrt = -(-n // 16)
    flops = 2.0 * 128 * 16 * sum(-(-16 * (rt + 1) // 32) * 32 for rt in range(nrt)) * (-(-q // 128)) * D
    lines.append("marginal_edges_headline: n %d V %d R %d (q = %d), %d chains, window rows 2..%d of each (nsamp %d), thin %d: %d draws per chain, D = %d; tau2, mu, u, "
                 "lambda, S loaded from seeded draws, not sampled (the call's time depends on the shapes alone); n_bad %d" % (n, V, R, q, K, tot, nsamp, thin, nd, D, out[3]))
    lines.append("bnr_chains_marginal_edges, whole call (the marginal kernels, k_medge_proj, k_medge_summary, the copies), median of %d: %.1f ms (best %.1f, worst %.1f)"
                 % (a.reps, 1e3 * med, 1e3 * min(ts), 1e3 * max(ts)))
    lines.append("bnr_chains_marginal_loo on the same chains, same commit, median of %d: %.1f ms (best %.1f, worst %.1f)"
                 % (a.reps, 1e3 * float(np.median(tl)), 1e3 * min(tl), 1e3 * max(tl)))
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
        for name in ("k_mloo_w", "k_mloo_rhs", "k_mloo_gram", "k_mloo_factor", "k_medge_proj", "k_medge_summary"):
            lines.append("  %-16s %4d launches, %9.2f ms" % (name, cnt(name), 1e3 * pick(name)))
        tp = pick("k_medge_proj")
        if tp > 0:
            lines.append("  k_medge_proj: %.3g flops issued as MFMAs per call = %.2f TFLOP/s = %.1f %% of the %.1f TFLOP/s f64 matrix peak"
                         % (flops, flops / tp * 1e-12, 100 * flops / tp / PEAK, PEAK * 1e-12))
    else:
        lines.append("kernel times: not measured in this run (no --kernel-stats)")
    print("\n".join(lines), flush=True)
    hthin = -(-nsamp // a.host_draws)
    hnd = -(-nsamp // hthin)
    dev = _capi.chains_marginal_edges(chains, 2, nsamp, hthin, per_draw=True)
    for ch in chains:
        ch.close()
    Xd = np.asarray(X, dtype=np.float64)
    t = time.perf_counter()
    hm, hv, _hb = api._host_marginal_gamma([table] * K, Xd, y, 1, nsamp, hthin)
    th = time.perf_counter() - t
    per = th / (K * hnd)
    lines.append("host restatement api._host_marginal_gamma (numpy, OMP_NUM_THREADS=%s) on the same tables, %d draws per chain (%d in all): %.2f s = %.3f s per draw; "
                 "the %d draws of the device call at that rate: %.0f s = %.0f x the device call" % (os.environ.get("OMP_NUM_THREADS", "?"), hnd, K * hnd, th, per, D, per * D, per * D / med))
    lines.append("device against host on those %d draws: max |m difference| %.2e, max |v difference| %.2e"
                 % (K * hnd, float(np.max(np.abs(dev[1] - hm))), float(np.max(np.abs(dev[2] - hv)))))
    print("\n".join(lines[-2:]), flush=True)
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "w") as f:
    f.write("\n".join(lines) + "\n")
