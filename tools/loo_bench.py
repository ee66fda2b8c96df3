"""PSIS-LOO at the headline size: bnr_chain_loo on chain 1 of an 8-chain group (n = 500, V = 100, R = 7) over a 20 000-row window, timed
with the call's own device synchronise (median of 5 after one warm-up), next to bnr_chain_loglik_stats (the same k_predict, with
k_pred_loglik instead of k_psis) on the same window; the host fallback (LOO on the fetched table) on the same window.  --no-host skips the
host fallback (for a rocprofv3 --kernel-trace --stats run).  Writes --out (default profiles/loo_headline.txt)."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import bnr_amd
from bnr_amd.api import Results, _tail_length

ap = argparse.ArgumentParser()
ap.add_argument("--out", default="profiles/loo_headline.txt")
ap.add_argument("--nsamp", type=int, default=20000)
ap.add_argument("--no-host", action="store_true")
a = ap.parse_args()

n, V, R, nsamp = 500, 100, 7, a.nsamp
q, tot = V * (V + 1) // 2, nsamp + 1
X, y, _ = bnr_amd.make_synthetic(n, V, R, seed=20240501)
chains = [bnr_amd.Chain(X, y, R, tot, 4242, 1)]
chains += [bnr_amd.Chain.like(chains[0], 4242, c) for c in range(2, 9)]
grp = bnr_amd.Group(chains)
for ch in chains:
    ch.init_prior()
t0 = time.perf_counter()
grp.run(2, tot, tot)
lines = ["loo_headline: n %d V %d R %d (q %d), chain 1 of an 8-chain group, window rows 2..%d (nsamp %d, tail length M = %d); sampling took %.1f s"
         % (n, V, R, q, tot, nsamp, _tail_length(nsamp, 1.0), time.perf_counter() - t0)]
ch1 = chains[0]


def timed(f, reps=5):
    f()
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        f()
        ts.append(time.perf_counter() - t)
    return float(np.median(ts)), float(np.min(ts))


ll_med, ll_best = timed(lambda: ch1.loglik_stats(2, nsamp))
loo_med, loo_best = timed(lambda: ch1.loo(2, nsamp))
lines.append("bnr_chain_loglik_stats n %d: median %8.3f ms (best %8.3f)" % (n, 1e3 * ll_med, 1e3 * ll_best))
lines.append("bnr_chain_loo          n %d: median %8.3f ms (best %8.3f); the PSIS adds %.3f ms (medians)" % (n, 1e3 * loo_med, 1e3 * loo_best,
                                                                                                           1e3 * (loo_med - ll_med)))
lpd, elpd, k = ch1.loo(2, nsamp)
lines.append("result: elpd_loo %.3f, p_loo %.3f, max k-hat %.3f, rows with k-hat > 0.7: %d" % (elpd.sum(), (lpd - elpd).sum(), k.max(), int((k > 0.7).sum())))
if not a.no_host:
    t = time.perf_counter()
    st = ch1.fetch(1, tot)
    tf = time.perf_counter() - t
    res = Results(st, None, None, 1, nsamp)
    t = time.perf_counter()
    host = bnr_amd.LOO(res, X, y, x_transform=False)
    th = time.perf_counter() - t
    worst = float(np.max(np.abs(host["elpd_loo_i"] - elpd) / np.abs(host["elpd_loo_i"])))
    lines.append("host fallback (LOO on the fetched table, numpy on %s threads): %.3f s, plus %.3f s to fetch the table; device call %.3f ms = %.0fx faster "
                 "than the host computation alone; worst relative difference of elpd_loo_i %.1e, of k-hat %.1e"
                 % (os.environ.get("OMP_NUM_THREADS", "?"), th, tf, 1e3 * loo_med, th / loo_med, worst, float(np.max(np.abs(host["pareto_k"] - k)))))
grp.close()
for ch in chains:
    ch.close()
print("\n".join(lines))
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "w") as f:
    f.write("\n".join(lines) + "\n")
