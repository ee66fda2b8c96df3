"""Posterior prediction at the headline size: bnr_chain_predict on chain 1 of an 8-chain group (n = 500, V = 100, R = 7) over a 20 000-row
window, m = 16 and m = 500 new rows, timed with the call's own device synchronise (median of 5 after one warm-up); bnr_chain_loglik_stats of
the 500 training rows; the host fallback (Predict on the fetched table) on the same window.  Achieved flop/s and bytes/s are computed from
the shapes (2 m q nsamp flop; the nsamp x q gamma window + m x q X + m x nsamp E bytes).  --no-host skips the host fallback (for a
rocprofv3 --kernel-trace --stats run).  Writes --out (default profiles/predict_headline.txt)."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import bnr_amd
from bnr_amd.api import Results, _summary_ranks

ap = argparse.ArgumentParser()
ap.add_argument("--out", default="profiles/predict_headline.txt")
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
lines = ["predict_headline: n %d V %d R %d (q %d), chain 1 of an 8-chain group, window rows 2..%d (nsamp %d); sampling took %.1f s"
         % (n, V, R, q, tot, nsamp, time.perf_counter() - t0)]
ch1 = chains[0]
k_lo, k_hi = _summary_ranks(nsamp, 95)


def timed(f, reps=5):
    f()
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        f()
        ts.append(time.perf_counter() - t)
    return float(np.median(ts)), float(np.min(ts))


for m in (16, 500):
    Xn, yn, _ = bnr_amd.make_synthetic(m, V, R, seed=7 + m)
    med, best = timed(lambda: ch1.predict(Xn, 2, nsamp, k_lo, k_hi, y=yn))
    flop, byt = 2.0 * m * q * nsamp, 8.0 * (nsamp * q + m * q + m * nsamp)
    lines.append("bnr_chain_predict m %4d (with y): median %8.3f ms (best %8.3f)  %7.2f TFLOP/s  %6.2f TB/s  (flop %.3g, bytes %.3g)"
                 % (m, 1e3 * med, 1e3 * best, flop / med / 1e12, byt / med / 1e12, flop, byt))
med, best = timed(lambda: ch1.loglik_stats(2, nsamp))
lines.append("bnr_chain_loglik_stats n %d: median %8.3f ms (best %8.3f)  %7.2f TFLOP/s" % (n, 1e3 * med, 1e3 * best, 2.0 * n * q * nsamp / med / 1e12))
if not a.no_host:
    t = time.perf_counter()
    st = ch1.fetch(1, tot)
    tf = time.perf_counter() - t
    res = Results(st, None, None, 1, nsamp)
    Xn, yn, _ = bnr_amd.make_synthetic(500, V, R, seed=7 + 500)
    t = time.perf_counter()
    bnr_amd.Predict(res, Xn, yn, x_transform=False)
    th = time.perf_counter() - t
    dev = timed(lambda: ch1.predict(Xn, 2, nsamp, k_lo, k_hi, y=yn))[0]
    lines.append("host fallback m 500 (Predict on the fetched table, numpy on %s threads): %.3f s, plus %.3f s to fetch the table; device call %.3f ms = %.0fx faster than the host computation alone"
                 % (os.environ.get("OMP_NUM_THREADS", "?"), th, tf, 1e3 * dev, th / dev))
grp.close()
for ch in chains:
    ch.close()
print("\n".join(lines))
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "w") as f:
    f.write("\n".join(lines) + "\n")
