"""Chain stacking at the headline size: bnr_chains_wsummary beside the unchanged bnr_chains_summary over an 8-chain group (n = 500, V = 100,
R = 7; q + V = 5150 parameters) with a 20 000-row window per chain, each timed between two bnr_device_synchronize calls (median of --reps calls
after --warm warm-up calls, the two interleaved in one session), and bnr_chains_stack (one PSIS-LOO pass per chain, then the weight solver
on the host).  Writes --out (default profiles/stacking_headline.txt)."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import bnr_amd
from bnr_amd import _capi, api

ap = argparse.ArgumentParser()
ap.add_argument("--out", default="profiles/stacking_headline.txt")
ap.add_argument("--nsamp", type=int, default=20000)
ap.add_argument("--chains", type=int, default=8)
ap.add_argument("--reps", type=int, default=11)
ap.add_argument("--warm", type=int, default=2)
a = ap.parse_args()

n, V, R, nsamp = 500, 100, 7, a.nsamp
q, tot = V * (V + 1) // 2, nsamp + 1
X, y, _ = bnr_amd.make_synthetic(n, V, R, seed=20240501)
chains = [bnr_amd.Chain(X, y, R, tot, 4242, 1)]
chains += [bnr_amd.Chain.like(chains[0], 4242, c) for c in range(2, a.chains + 1)]
grp = bnr_amd.Group(chains) if len(chains) > 1 else None
for ch in chains:
    ch.init_prior()
t0 = time.perf_counter()
(grp or chains[0]).run(2, tot, tot)
K = len(chains)
S = K * nsamp
lines = ["stacking_headline: n %d V %d R %d (q + V = %d parameters), %d chains, window rows 2..%d of each (nsamp %d, S = %d pooled draws per parameter); "
         "sampling took %.1f s" % (n, V, R, q + V, K, tot, nsamp, S, time.perf_counter() - t0)]
k_lo, k_hi = api._summary_ranks(S, 95)
dev = 0


def once(f):
    _capi.device_synchronize(dev)
    t = time.perf_counter()
    f()
    _capi.device_synchronize(dev)
    return time.perf_counter() - t


st = api.device_stack_chains(chains, 1, nsamp)
w = st.weights
calls = dict(summary=lambda: _capi.pooled_summary(chains, 2, nsamp, k_lo, k_hi),
             wsummary=lambda: _capi.stacked_summary(chains, w, 2, nsamp, k_lo, k_hi),
             wsummary_uniform=lambda: _capi.stacked_summary(chains, np.full(K, 1.0 / K), 2, nsamp, k_lo, k_hi),
             stack=lambda: _capi.chains_stack(chains, 2, nsamp))
for f in calls.values():
    for _ in range(a.warm):
        f()
ts = {k: [] for k in calls}
for _ in range(a.reps):                                  # interleaved: every call sees the same session
    for k, f in calls.items():
        ts[k].append(once(f))
med = {k: float(np.median(v)) for k, v in ts.items()}
for k, label in (("summary", "bnr_chains_summary (k_summary, unchanged)"), ("wsummary", "bnr_chains_wsummary, stacking weights"),
                 ("wsummary_uniform", "bnr_chains_wsummary, weights 1/K"), ("stack", "bnr_chains_stack (%d PSIS-LOO passes + solver)" % K)):
    lines.append("%-50s median of %d: %9.1f ms (best %9.1f, worst %9.1f)" % (label, a.reps, 1e3 * med[k], 1e3 * min(ts[k]), 1e3 * max(ts[k])))
lines.append("ratio bnr_chains_wsummary / bnr_chains_summary: %.2f (weights 1/K: %.2f)" % (med["wsummary"] / med["summary"], med["wsummary_uniform"] / med["summary"]))
lines.append("stacking weights %s; %d updates, gap %.3g; elpd_stack %.2f against elpd_uniform %.2f and per chain %s; rows with k-hat above %.2f per chain: %s"
             % (np.array2string(w, precision=4), st.iterations, st.gap, st.elpd_stack, st.elpd_uniform, np.array2string(st.elpd_chain, precision=1),
                st.khat_threshold, st.n_high_k.tolist()))
pooled = _capi.pooled_summary(chains, 2, nsamp, k_lo, k_hi)
uni = _capi.stacked_summary(chains, np.full(K, 1.0 / K), 2, nsamp, k_lo, k_hi)
if K & (K - 1) == 0:
    lines.append("weights 1/K give bnr_chains_summary's order statistics bit for bit: %s"
                 % (np.array_equal(pooled[1], uni[1], equal_nan=True) and np.array_equal(pooled[2], uni[2], equal_nan=True)))
if grp:
    grp.close()
for ch in chains:
    ch.close()
print("\n".join(lines))
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "w") as f:
    f.write("\n".join(lines) + "\n")
