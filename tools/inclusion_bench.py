"""The joint posterior of the node indicators at the headline size: bnr_chains_inclusion over an 8-chain group (n = 500, V = 100, R = 7; two
pattern words) with a 20 000-row window per chain (S = 160 000 pooled draws), timed with the call's own device synchronise (median of 3
after one warm-up): all six outputs, prob + joint only (k_incl_pack and k_incl_joint), the top sets only (k_incl_pack and k_incl_group) and
prob alone (k_incl_pack).  The host fallback (api._host_node_sets on the fetched tables) is timed in two parts, the fetch and the compute,
and must agree with the device exactly.  --no-host skips it (for a rocprofv3 --kernel-trace --stats run, which gives each kernel's time per
launch).  Writes --out (default profiles/inclusion_headline.txt)."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import bnr_amd
from bnr_amd import _capi, api

ap = argparse.ArgumentParser()
ap.add_argument("--out", default="profiles/inclusion_headline.txt")
ap.add_argument("--nsamp", type=int, default=20000)
ap.add_argument("--chains", type=int, default=8)
ap.add_argument("--ntop", type=int, default=10)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--no-host", action="store_true")
a = ap.parse_args()

n, V, R, nsamp, ntop = 500, 100, 7, a.nsamp, a.ntop
tot = nsamp + 1
X, y, _ = bnr_amd.make_synthetic(n, V, R, seed=20240501)
chains = [bnr_amd.Chain(X, y, R, tot, 4242, 1)]
chains += [bnr_amd.Chain.like(chains[0], 4242, c) for c in range(2, a.chains + 1)]
grp = bnr_amd.Group(chains) if len(chains) > 1 else None
for ch in chains:
    ch.init_prior()
t0 = time.perf_counter()
(grp or chains[0]).run(2, tot, tot)
S = len(chains) * nsamp
lines = ["inclusion_headline: n %d V %d R %d (W = %d pattern words), %d chains, window rows 2..%d of each (nsamp %d, S = %d pooled draws), ntop %d; "
         "sampling took %.1f s" % (n, V, R, (V + 63) // 64, len(chains), tot, nsamp, S, ntop, time.perf_counter() - t0)]


def timed(f, reps=a.reps):
    f()
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        f()
        ts.append(time.perf_counter() - t)
    return float(np.median(ts)), float(np.min(ts))


cases = (("all six outputs", _capi.INCL_FIELDS), ("prob + joint only", ("prob", "joint")), ("top sets only", ("top_sets", "top_count")), ("prob only", ("prob",)))
for name, fields in cases:
    med, best = timed(lambda: _capi.pooled_inclusion(chains, 2, nsamp, 0, ntop, fields=fields))
    lines.append("bnr_chains_inclusion, xi, %-18s median %9.2f ms (best %9.2f)" % (name + ":", 1e3 * med, 1e3 * best))
    if fields is _capi.INCL_FIELDS:
        all_med = med
med, best = timed(lambda: _capi.pooled_inclusion(chains, 2, nsamp, 1, ntop))
lines.append("bnr_chains_inclusion, lambda, all six outputs:     median %9.2f ms (best %9.2f)" % (1e3 * med, 1e3 * best))
dev_med, dev_best = timed(lambda: api.device_node_sets(chains, 1, nsamp, ntop))
dev = api.device_node_sets(chains, 1, nsamp, ntop)
lines.append("device_node_sets (both calls and the Python around them): median %9.2f ms (best %9.2f)" % (1e3 * dev_med, 1e3 * dev_best))
lines.append("result: %d distinct node sets among %d draws; mean size %.2f of %d nodes (mode %d); MAP model has %d nodes and share %.5f; %d nodes in the median "
             "model; mean active dimensions %.3f of %d; largest off-diagonal co-inclusion %.4f"
             % (dev.n_distinct, S, dev.size_mean, V, dev.size_mode, dev.map_model.size, dev.top_prob[0], dev.median_model.size, dev.dim_mean, R,
                float((dev.co_inclusion - np.diag(np.diag(dev.co_inclusion))).max())))
if not a.no_host:
    t = time.perf_counter()
    tabs = [ch.fetch(1, tot) for ch in chains]
    tf = time.perf_counter() - t
    t = time.perf_counter()
    host = api._host_node_sets(tabs, 1, nsamp, ntop)
    th = time.perf_counter() - t
    same = all(np.array_equal(getattr(host, f), getattr(dev, f)) for f in ("prob_nodes", "co_inclusion", "size_pmf", "top_prob", "prob_active", "dim_pmf"))
    same = same and host.n_distinct == dev.n_distinct and [s.tolist() for s in host.top_sets] == [s.tolist() for s in dev.top_sets]
    lines.append("host fallback (_host_node_sets, numpy): %.2f s to fetch the %d tables + %.2f s to compute; device_node_sets %.1f ms = %.0fx faster than "
                 "fetch + compute, %.0fx than the compute alone" % (tf, len(chains), th, 1e3 * dev_med, (tf + th) / dev_med, th / dev_med))
    lines.append("device and host agree exactly: %s" % same)
    assert same
if grp:
    grp.close()
for ch in chains:
    ch.close()
print("\n".join(lines))
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "w") as f:
    f.write("\n".join(lines) + "\n")
