"""The rank-normalised diagnostics at the headline size: bnr_chains_rank_diag over an 8-chain group (n = 500, V = 100, R = 7; q + V = 5150
parameters) with a 20 000-row window per chain and max_lag 250, timed with the call's own device synchronise (median of 3 after one warm-up),
with all six outputs and with rhat_bulk / rhat_tail only.  The host fallback (api._host_rank_diagnostics on the fetched tables) is timed on the
first --host-cols gamma columns of the same windows and scaled to q + V columns (its cost is per column); the time to fetch the eight tables is
measured in full.  --no-host skips it (for a rocprofv3 --kernel-trace --stats run).  Writes --out (default profiles/rank_diag_headline.txt)."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import bnr_amd
from bnr_amd import _capi, api

ap = argparse.ArgumentParser()
ap.add_argument("--out", default="profiles/rank_diag_headline.txt")
ap.add_argument("--nsamp", type=int, default=20000)
ap.add_argument("--max-lag", type=int, default=250)
ap.add_argument("--chains", type=int, default=8)
ap.add_argument("--host-cols", type=int, default=32)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--no-host", action="store_true")
a = ap.parse_args()

n, V, R, nsamp, L = 500, 100, 7, a.nsamp, a.max_lag
q, tot = V * (V + 1) // 2, nsamp + 1
X, y, _ = bnr_amd.make_synthetic(n, V, R, seed=20240501)
chains = [bnr_amd.Chain(X, y, R, tot, 4242, 1)]
chains += [bnr_amd.Chain.like(chains[0], 4242, c) for c in range(2, a.chains + 1)]
grp = bnr_amd.Group(chains) if len(chains) > 1 else None
for ch in chains:
    ch.init_prior()
t0 = time.perf_counter()
(grp or chains[0]).run(2, tot, tot)
lines = ["rank_diag_headline: n %d V %d R %d (q + V = %d parameters), %d chains, window rows 2..%d of each (nsamp %d, S' = %d ranked draws per parameter), "
         "max_lag %d; sampling took %.1f s" % (n, V, R, q + V, len(chains), tot, nsamp, 2 * len(chains) * (nsamp // 2), L, time.perf_counter() - t0)]


def timed(f, reps=a.reps):
    f()
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        f()
        ts.append(time.perf_counter() - t)
    return float(np.median(ts)), float(np.min(ts))


all_med, all_best = timed(lambda: _capi.pooled_rank_diag(chains, 2, nsamp, L))
rh_med, rh_best = timed(lambda: _capi.pooled_rank_diag(chains, 2, nsamp, L, fields=("rhat_bulk", "rhat_tail")))
lines.append("bnr_chains_rank_diag, all six outputs:          median %9.1f ms (best %9.1f)" % (1e3 * all_med, 1e3 * all_best))
lines.append("bnr_chains_rank_diag, rhat_bulk / rhat_tail only: median %9.1f ms (best %9.1f)" % (1e3 * rh_med, 1e3 * rh_best))
d = api.device_rank_diagnostics(chains, 1, nsamp, L)
rg, rx = _capi.rhat(chains, len(chains), None, 1, nsamp)
lines.append("result: max rhat gamma %.3f (classic split-R-hat %.3f), max rhat xi %.3f (classic %.3f; NaN: %d constant xi columns), min ess_bulk gamma %.0f, "
             "min ess_tail gamma %.0f of %d draws" % (np.nanmax(d.rhat_gamma), rg.max(), np.nanmax(d.rhat_xi), rx.max(), int(np.isnan(d.rhat_xi).sum()),
                                                     np.nanmin(d.ess_bulk_gamma), np.nanmin(d.ess_tail_gamma), d.draws))
if not a.no_host:
    hc = min(a.host_cols, q)
    sub, tf = [], 0.0
    for ch in chains:
        t = time.perf_counter()
        st = ch.fetch(1, tot)
        tf += time.perf_counter() - t
        sub.append(dict(gamma=np.asfortranarray(st["gamma"][:, :hc]), xi=np.zeros((tot, 0, 1), order="F")))
        del st
    t = time.perf_counter()
    host = api._host_rank_diagnostics(sub, 1, nsamp, L)
    th = time.perf_counter() - t
    scaled = th * (q + V) / hc
    gap = {f: float(np.nanmax(np.abs(getattr(host, f + "_gamma") - getattr(d, f + "_gamma")[:hc]) / np.abs(getattr(host, f + "_gamma"))))
           for f in ("rhat_bulk", "rhat_tail", "ess_bulk", "ess_tail", "ess_mean", "mcse_mean")}
    lines.append("host fallback (_host_rank_diagnostics, numpy on %s threads): %.2f s for the first %d gamma columns = %.0f s scaled to %d columns (not run in full), "
                 "plus %.1f s (measured) to fetch the %d tables; device call %.1f ms = %.0fx faster than the scaled host computation alone"
                 % (os.environ.get("OMP_NUM_THREADS", "?"), th, hc, scaled, q + V, tf, len(chains), 1e3 * all_med, scaled / all_med))
    lines.append("largest relative difference device / host on those columns: " + ", ".join("%s %.1e" % kv for kv in gap.items()))
if grp:
    grp.close()
for ch in chains:
    ch.close()
print("\n".join(lines))
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "w") as f:
    f.write("\n".join(lines) + "\n")
