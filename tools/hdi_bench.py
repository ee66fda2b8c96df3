"""The highest-density intervals at the headline size: bnr_chains_hdi over an 8-chain group (n = 500, V = 100, R = 7; q + V = 5150 parameters)
with a 20 000-row window per chain and three levels, timed with the call's own device synchronise (median of 3 after one warm-up); beside it
bnr_chains_rank_diag with rhat_bulk alone (one k_rank and one k_acov at one lag per block of columns) on the same windows.  The host fallback
(api._host_hdi on the fetched windows) is timed on the first --host-cols gamma columns and scaled to q + V columns (its cost is per column).
--no-host skips it (for a rocprofv3 --kernel-trace --stats run, which gives k_hdi's and k_rank's time per launch on the same blocks).
Writes --out (default profiles/hdi_headline.txt)."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import bnr_amd
from bnr_amd import _capi, api

ap = argparse.ArgumentParser()
ap.add_argument("--out", default="profiles/hdi_headline.txt")
ap.add_argument("--nsamp", type=int, default=20000)
ap.add_argument("--chains", type=int, default=8)
ap.add_argument("--host-cols", type=int, default=32)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--no-host", action="store_true")
a = ap.parse_args()

n, V, R, nsamp = 500, 100, 7, a.nsamp
LEVELS = (0.5, 0.9, 0.95)
q, tot = V * (V + 1) // 2, nsamp + 1
X, y, _ = bnr_amd.make_synthetic(n, V, R, seed=20240501)
chains = [bnr_amd.Chain(X, y, R, tot, 4242, 1)]
chains += [bnr_amd.Chain.like(chains[0], 4242, c) for c in range(2, a.chains + 1)]
grp = bnr_amd.Group(chains) if len(chains) > 1 else None
for ch in chains:
    ch.init_prior()
t0 = time.perf_counter()
(grp or chains[0]).run(2, tot, tot)
S = len(chains) * nsamp
lines = ["hdi_headline: n %d V %d R %d (q + V = %d parameters), %d chains, window rows 2..%d of each (nsamp %d, S = %d pooled draws per parameter), levels %s; "
         "sampling took %.1f s" % (n, V, R, q + V, len(chains), tot, nsamp, S, LEVELS, time.perf_counter() - t0)]


def timed(f, reps=a.reps):
    f()
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        f()
        ts.append(time.perf_counter() - t)
    return float(np.median(ts)), float(np.min(ts))


hdi_med, hdi_best = timed(lambda: _capi.pooled_hdi(chains, 2, nsamp, LEVELS))
sg_med, sg_best = timed(lambda: _capi.pooled_hdi(chains, 2, nsamp, (), fields=("median", "p_pos", "p_neg")))
rk_med, rk_best = timed(lambda: _capi.pooled_rank_diag(chains, 2, nsamp, 250, fields=("rhat_bulk",)))
lines.append("bnr_chains_hdi, three levels, all five outputs:        median %9.1f ms (best %9.1f)" % (1e3 * hdi_med, 1e3 * hdi_best))
lines.append("bnr_chains_hdi, no level (median, p_pos, p_neg only):  median %9.1f ms (best %9.1f)" % (1e3 * sg_med, 1e3 * sg_best))
lines.append("bnr_chains_rank_diag, rhat_bulk only (for comparison): median %9.1f ms (best %9.1f)" % (1e3 * rk_med, 1e3 * rk_best))
es = api.device_edge_selection(chains, 1, nsamp, 0.95, 0.05)
_mean, lo, up, _pxi = _capi.pooled_summary(chains, 2, nsamp, *api._summary_ranks(S, 95))
et_excl = (lo > 0) | (up < 0)
lines.append("result at hdi_prob 0.95, fdr 0.05: %d of %d edges selected (expected false sign rate %.4f); the 95 %% HDI excludes zero for %d edges, the equal-tailed "
             "95 %% interval for %d (%d edges differ); mean HDI width %.4f against %.4f equal-tailed"
             % (es.n_selected, q, es.expected_fsr, int(es.hdi_excludes_zero.sum()), int(et_excl.sum()), int((et_excl != es.hdi_excludes_zero).sum()),
                float(np.mean(es.hdi_upper - es.hdi_lower)), float(np.mean(up - lo))))
if not a.no_host:
    hc = min(a.host_cols, q)
    wins, tf = [], 0.0
    for ch in chains:
        t = time.perf_counter()
        st = ch.fetch(1, tot)
        tf += time.perf_counter() - t
        wins.append(np.ascontiguousarray(st["gamma"][1:, :hc, 0]))
        del st
    dev = _capi.pooled_hdi(chains, 2, nsamp, LEVELS)
    t = time.perf_counter()
    host = api._host_hdi(np.concatenate(wins, axis=0).T, LEVELS)
    th = time.perf_counter() - t
    scaled = th * (q + V) / hc
    same = all(np.array_equal(host[f], np.asarray(d)[..., :hc], equal_nan=True) for f, d in zip(_capi.HDI_FIELDS, dev))
    lines.append("host fallback (_host_hdi, numpy on %s threads): %.2f s for the first %d gamma columns = %.0f s scaled to %d columns (not run in full), plus "
                 "%.1f s (measured) to fetch the %d tables; device call %.1f ms = %.0fx faster than the scaled host computation alone"
                 % (os.environ.get("OMP_NUM_THREADS", "?"), th, hc, scaled, q + V, tf, len(chains), 1e3 * hdi_med, scaled / hdi_med))
    lines.append("device and host agree bit for bit on those columns: %s" % same)
if grp:
    grp.close()
for ch in chains:
    ch.close()
print("\n".join(lines))
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "w") as f:
    f.write("\n".join(lines) + "\n")
