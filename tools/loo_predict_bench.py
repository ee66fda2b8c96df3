"""LOO predictive checks at the headline size: an 8-chain group (n = 500, V = 100, R = 7), every chain's 20 000-row window.  Timed with the
call's own device synchronise (median of 5 after one warm-up), for the pooled group (S = 160 000) and for chain 1 alone (S = 20 000):
  - bnr_chains_loo (k_predict + k_psis): the baseline.  --old-only times only the entry points the parent commit has too (bnr_chains_loo,
    bnr_chains_loglik_stats, bnr_chains_predict), for a run on the parent's library in the same visit (BNR_HIP_LIB selects the library);
  - bnr_chains_loo_predict with only lpd / elpd_loo / k-hat (k_psis_w), with the moments (k_loo_moments), and with everything (k_loo_quantile);
  - the host fallback (_host_loo_predict over the fetched gamma / mu / tau2 columns, --host-rows training rows of it extrapolated to n),
    with the fetch, for chain 1 and -- with --host-pooled -- the pooled window.
Per-kernel times come from a rocprofv3 --kernel-trace --stats run of this script with --no-host (k_psis_w, k_loo_moments, k_loo_quantile).
Writes --out (default profiles/loo_predict_headline.txt)."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import bnr_amd
from bnr_amd import _capi, api
from bnr_amd.api import _summary_ranks

ap = argparse.ArgumentParser()
ap.add_argument("--out", default="profiles/loo_predict_headline.txt")
ap.add_argument("--nsamp", type=int, default=20000)
ap.add_argument("--chains", type=int, default=8)
ap.add_argument("--no-host", action="store_true")
ap.add_argument("--host-pooled", action="store_true")
ap.add_argument("--host-rows", type=int, default=50)
ap.add_argument("--old-only", action="store_true")
ap.add_argument("--label", default="this")
a = ap.parse_args()

n, V, R, nsamp, nch = 500, 100, 7, a.nsamp, a.chains
q, tot = V * (V + 1) // 2, nsamp + 1
X, y, _ = bnr_amd.make_synthetic(n, V, R, seed=20240501)
chains = [bnr_amd.Chain(X, y, R, tot, 4242, 1)]
chains += [bnr_amd.Chain.like(chains[0], 4242, c) for c in range(2, nch + 1)]
grp = bnr_amd.Group(chains)
for ch in chains:
    ch.init_prior()
t0 = time.perf_counter()
grp.run(2, tot, tot)
lines = ["loo_predict_headline (%s): n %d V %d R %d (q %d), %d-chain group, window rows 2..%d of every chain (nsamp %d); sampling took %.1f s"
         % (a.label, n, V, R, q, nch, tot, nsamp, time.perf_counter() - t0)]


def timed(f, reps=5):
    f()
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        f()
        ts.append(time.perf_counter() - t)
    return float(np.median(ts)), float(np.min(ts))


Xn, yn, _ = bnr_amd.make_synthetic(500, V, R, seed=507)
for cs, name in ((chains, "%d chains pooled" % nch), (chains[:1], "chain 1 alone")):
    S = len(cs) * nsamp
    old = timed(lambda: _capi.pooled_loo(cs, 2, nsamp))
    lines.append("%-7s %s, S = %6d: bnr_chains_loo                          median %9.3f ms (best %9.3f)" % (a.label, name, S, 1e3 * old[0], 1e3 * old[1]))
    ll = timed(lambda: _capi.pooled_loglik_stats(cs, 2, nsamp, pit=True))
    lines.append("%-7s %s, S = %6d: bnr_chains_loglik_stats with PIT        median %9.3f ms (best %9.3f)" % (a.label, name, S, 1e3 * ll[0], 1e3 * ll[1]))
    pr = timed(lambda: _capi.pooled_predict(cs, Xn, 2, nsamp, *_summary_ranks(S, 95), y=yn))
    lines.append("%-7s %s, S = %6d: bnr_chains_predict m 500 (with y)       median %9.3f ms (best %9.3f)" % (a.label, name, S, 1e3 * pr[0], 1e3 * pr[1]))
    if a.old_only:
        continue
    w = timed(lambda: _capi.pooled_loo_predict(cs, 2, nsamp, fields=("lpd", "elpd_loo", "pareto_k")))
    mo = timed(lambda: _capi.pooled_loo_predict(cs, 2, nsamp, fields=("lpd", "elpd_loo", "pareto_k", "loo_mean", "loo_sd", "loo_pit")))
    full = timed(lambda: _capi.pooled_loo_predict(cs, 2, nsamp))
    lines.append("%-7s %s, S = %6d: bnr_chains_loo_predict, weights only    median %9.3f ms (best %9.3f) = %.2f x bnr_chains_loo"
                 % (a.label, name, S, 1e3 * w[0], 1e3 * w[1], w[0] / old[0]))
    lines.append("%-7s %s, S = %6d: bnr_chains_loo_predict, + moments       median %9.3f ms (best %9.3f); k_loo_moments adds %.3f ms"
                 % (a.label, name, S, 1e3 * mo[0], 1e3 * mo[1], 1e3 * (mo[0] - w[0])))
    lines.append("%-7s %s, S = %6d: bnr_chains_loo_predict, everything      median %9.3f ms (best %9.3f) = %.2f x bnr_chains_loo; the bounds (2 x 40 bisection "
                 "passes per row) add %.3f ms" % (a.label, name, S, 1e3 * full[0], 1e3 * full[1], full[0] / old[0], 1e3 * (full[0] - mo[0])))
    if not a.no_host and (len(cs) == 1 or a.host_pooled):
        t = time.perf_counter()
        tables = []
        for ch in cs:                                    # only the columns the restatement reads cross PCIe
            st = {k: np.zeros((tot,) + _capi.table_shapes(V, R)[k], order="F") for k in ("tau2", "gamma", "mu")}
            ptrs = [_capi._ptr(st.get(k)) for k in _capi.TABLE_COLUMNS]
            _capi.check(ch.L.bnr_chain_fetch(ch.h, 1, tot, tot, 0, *ptrs))
            tables.append(st)
        tf = time.perf_counter() - t
        hr = min(a.host_rows, n)
        t = time.perf_counter()
        hp = api._host_loo_predict(tables, X[:hr], y[:hr], 1, nsamp, 95)
        th = (time.perf_counter() - t) * n / hr
        dev = _capi.pooled_loo_predict(cs, 2, nsamp)
        lines.append("%-7s %s: host fallback (_host_loo_predict, numpy / scipy on %s threads; %d rows timed, scaled to %d): %.1f s, plus %.2f s to fetch gamma, "
                     "mu, tau2 of %d chain(s); device call %.1f ms = %.0fx faster than the host computation with its fetch"
                     % (a.label, name, os.environ.get("OMP_NUM_THREADS", "?"), hr, n, th, tf, len(cs), 1e3 * full[0], (th + tf) / full[0]))
        lines.append("%-7s %s: device against host on those rows: max gaps loo_mean %.3g, loo_sd %.3g, loo_pit %.3g, loo_lower %.3g, loo_upper %.3g, elpd_loo %.3g"
                     % (a.label, name, np.max(np.abs(dev[3][:hr] - hp.loo_mean)), np.max(np.abs(dev[4][:hr] - hp.loo_sd)), np.max(np.abs(dev[5][:hr] - hp.loo_pit)),
                        np.max(np.abs(dev[6][:hr] - hp.loo_lower)), np.max(np.abs(dev[7][:hr] - hp.loo_upper)), np.max(np.abs(dev[1][:hr] - hp.elpd_loo_i))))
    if len(cs) > 1:
        lp = api.device_loo_predict(cs, y, 1, nsamp, 95)
        lines.append("%-7s %s: coverage %.3f, KS %.3f, rmse_loo %.4f, r2_loo %.4f, n_high_k %d of %d (threshold %.2f)"
                     % (a.label, name, lp.coverage, lp.ks, lp.rmse_loo, lp.r2_loo, lp.n_high_k, n, lp.khat_threshold))
grp.close()
for ch in chains:
    ch.close()
print("\n".join(lines))
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "w") as f:
    f.write("\n".join(lines) + "\n")
