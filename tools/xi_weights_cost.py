"""What the model option xi_weights = reference costs per sweep (GPU): a lockstep group of C chains at a shape, every member in one mode,
graph-replayed sweeps timed by wall clock around the (synchronous) run call, the two modes interleaved A B A B ... so that drift hits both.

    python tools/xi_weights_cost.py [--sweeps 200] [--reps 5]
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np                                   # noqa: E402
import bnr_amd                                       # noqa: E402

SHAPES = [(500, 100, 7, 8, "headline (BASELINE configs[2]: 8 chains)"), (500, 100, 7, 1, "headline shape, one chain"),
          (500, 300, 10, 8, "BASELINE configs[4]: 8 chains"), (500, 300, 10, 1, "configs[4] shape, one chain")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sweeps", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    tot = a.sweeps + 1
    print("%-42s %12s %12s %10s   %s" % ("shape", "log us/sw", "ref us/sw", "delta us", "nan_w per sweep (ref, all chains)"), flush=True)
    for n, V, R, C, label in SHAPES:
        X, y, _ = bnr_amd.make_synthetic(n, V, R, seed=20240501)
        runs = {}
        for mode in ("log", "reference"):
            chains = [bnr_amd.Chain(X, y, R, tot, 20240501, 1, xi_weights=mode)]
            chains += [bnr_amd.Chain.like(chains[0], 20240501, c, tot) for c in range(2, C + 1)]
            for ch in chains:
                ch.init_prior()
            r = bnr_amd.Group(chains) if C > 1 else chains[0]
            r.prepare()
            r.run(2, tot, tot)                                   # warm-up: first run call of the lazily built paths
            runs[mode] = (chains, r, [])
        for _ in range(a.reps):
            for mode in ("log", "reference"):
                chains, r, ts = runs[mode]
                t0 = time.perf_counter()
                r.run(2, tot, tot)
                ts.append((time.perf_counter() - t0) / a.sweeps * 1e6)
        nan_w = sum(ch.counters()["nan_w"] for ch in runs["reference"][0]) / float((a.reps + 1) * a.sweeps)
        ml, mr = np.median(runs["log"][2]), np.median(runs["reference"][2])
        print("%-42s %12.1f %12.1f %+10.2f   %.0f   (log %s | ref %s)" % (label, ml, mr, mr - ml, nan_w,
              " ".join("%.1f" % t for t in runs["log"][2]), " ".join("%.1f" % t for t in runs["reference"][2])), flush=True)
        for mode in runs:
            chains, r, _ = runs[mode]
            if C > 1:
                r.close()
            for ch in chains:
                ch.close()


if __name__ == "__main__":
    main()
