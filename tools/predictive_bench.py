"""Pooled prediction at the headline size: an 8-chain group (n = 500, V = 100, R = 7), every chain's 20 000-row window pooled (S = 160 000
draws), m = 16 and m = 500 new rows.  Timed with the call's own device synchronise (median of 5 after one warm-up):
  - bnr_chain_predict on chain 1 (this build), and 8 x that figure: the same k_predict work the pooled call does;
  - bnr_chains_predict without the extras, and with the predictive bounds and the PIT (k_pred_pit, k_pred_noise, a second k_summary);
  - the host fallback (_host_pooled_predict on the fetched gamma / mu / tau2 / xi columns) for m = 500.
The noise pass's achieved bytes/s is 16 m S bytes (E read and written once) over the kernel's time, which comes from a
rocprofv3 --kernel-trace --stats run of this script with --no-host (kernel names k_pred_noise, k_pred_pit, k_summary, k_predict).
--parent-file: the output of tools/predict_bench.py run on the parent commit in the same visit; its single-chain medians are quoted x 8.
Writes --out (default profiles/predictive_headline.txt)."""
import argparse
import ctypes as C
import os
import re
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import bnr_amd
from bnr_amd import _capi, api
from bnr_amd.api import _summary_ranks

ap = argparse.ArgumentParser()
ap.add_argument("--out", default="profiles/predictive_headline.txt")
ap.add_argument("--nsamp", type=int, default=20000)
ap.add_argument("--chains", type=int, default=8)
ap.add_argument("--no-host", action="store_true")
ap.add_argument("--parent-file", default=None)
a = ap.parse_args()

n, V, R, nsamp, nch = 500, 100, 7, a.nsamp, a.chains
q, tot = V * (V + 1) // 2, nsamp + 1
S = nch * nsamp
X, y, _ = bnr_amd.make_synthetic(n, V, R, seed=20240501)
chains = [bnr_amd.Chain(X, y, R, tot, 4242, 1)]
chains += [bnr_amd.Chain.like(chains[0], 4242, c) for c in range(2, nch + 1)]
grp = bnr_amd.Group(chains)
for ch in chains:
    ch.init_prior()
t0 = time.perf_counter()
grp.run(2, tot, tot)
lines = ["predictive_headline: n %d V %d R %d (q %d), %d-chain group, window rows 2..%d of every chain (nsamp %d, S = %d pooled draws); sampling took %.1f s"
         % (n, V, R, q, nch, tot, nsamp, S, time.perf_counter() - t0)]
ch1 = chains[0]
k1 = _summary_ranks(nsamp, 95)
kS = _summary_ranks(S, 95)


def timed(f, reps=5):
    f()
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        f()
        ts.append(time.perf_counter() - t)
    return float(np.median(ts)), float(np.min(ts))


parent = {}
if a.parent_file and os.path.exists(a.parent_file):
    for ln in open(a.parent_file):
        mm = re.match(r"bnr_chain_predict m\s+(\d+) \(with y\): median\s+([0-9.]+) ms", ln)
        if mm:
            parent[int(mm.group(1))] = float(mm.group(2))

for m in (16, 500):
    Xn, yn, _ = bnr_amd.make_synthetic(m, V, R, seed=7 + m)
    one = timed(lambda: ch1.predict(Xn, 2, nsamp, *k1, y=yn))
    plain = timed(lambda: _capi.pooled_predict(chains, Xn, 2, nsamp, *kS, y=yn))
    full = timed(lambda: _capi.pooled_predict(chains, Xn, 2, nsamp, *kS, y=yn, pred_seed=4242, pit=True))
    lines.append("m %4d  bnr_chain_predict (chain 1, with y): median %8.3f ms (best %8.3f); x %d = %8.3f ms%s"
                 % (m, 1e3 * one[0], 1e3 * one[1], nch, 1e3 * nch * one[0],
                    ("; parent commit, same visit: %8.3f ms, x %d = %8.3f ms" % (parent[m], nch, nch * parent[m])) if m in parent else ""))
    lines.append("m %4d  bnr_chains_predict, %d chains pooled (with y): median %8.3f ms (best %8.3f) = %.2f x the %d single-chain calls"
                 % (m, nch, 1e3 * plain[0], 1e3 * plain[1], plain[0] / (nch * one[0]), nch))
    lines.append("m %4d  bnr_chains_predict + predictive bounds + PIT:  median %8.3f ms (best %8.3f); the extras add %8.3f ms; noise pass traffic %.3g bytes"
                 % (m, 1e3 * full[0], 1e3 * full[1], 1e3 * (full[0] - plain[0]), 16.0 * m * S))
med, best = timed(lambda: _capi.pooled_loglik_stats(chains, 2, nsamp, pit=True))
lines.append("bnr_chains_loglik_stats n %d with PIT: median %8.3f ms (best %8.3f)" % (n, 1e3 * med, 1e3 * best))
med, best = timed(lambda: _capi.pooled_summary(chains, 2, nsamp, *kS), reps=3)
lines.append("bnr_chains_summary (q + V = %d columns x S, staged in blocks of ~1 GiB): median %8.3f ms (best %8.3f)" % (q + V, 1e3 * med, 1e3 * best))
if not a.no_host:
    t = time.perf_counter()
    tables = []
    for ch in chains:                                    # only the columns the restatement reads cross PCIe
        st = {k: np.zeros((tot,) + _capi.table_shapes(V, R)[k], order="F") for k in ("tau2", "xi", "gamma", "mu")}
        ptrs = [_capi._ptr(st.get(k)) for k in _capi.TABLE_COLUMNS]
        _capi.check(ch.L.bnr_chain_fetch(ch.h, 1, tot, tot, 0, *ptrs))
        tables.append(st)
    tf = time.perf_counter() - t
    Xn, yn, _ = bnr_amd.make_synthetic(500, V, R, seed=7 + 500)
    t = time.perf_counter()
    hp = api._host_pooled_predict(tables, Xn, yn, 1, nsamp, pred_seed=4242)
    th = time.perf_counter() - t
    dev = _capi.pooled_predict(chains, Xn, 2, nsamp, *kS, y=yn, pred_seed=4242, pit=True)
    full = timed(lambda: _capi.pooled_predict(chains, Xn, 2, nsamp, *kS, y=yn, pred_seed=4242, pit=True))[0]
    lines.append("host fallback m 500 (_host_pooled_predict with bounds and PIT, numpy on %s threads): %.2f s, plus %.2f s to fetch gamma, mu, tau2, xi of %d chains; "
                 "device call %.3f ms = %.0fx faster than the host computation alone"
                 % (os.environ.get("OMP_NUM_THREADS", "?"), th, tf, nch, 1e3 * full, th / full))
    lines.append("device against host at m 500: max |pred_lower| gap %.3g, max |pred_upper| gap %.3g, max |pit| gap %.3g, max |estimate| gap %.3g"
                 % (np.max(np.abs(dev[5] - hp.pred_lower_bound)), np.max(np.abs(dev[6] - hp.pred_upper_bound)), np.max(np.abs(dev[7] - hp.pit)),
                    np.max(np.abs(dev[0] - hp.estimate))))
grp.close()
for ch in chains:
    ch.close()
print("\n".join(lines))
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "w") as f:
    f.write("\n".join(lines) + "\n")
