"""Diagnostic (-DBNR_STAMPS build): the gaps between the kernels of the sweep's critical chain, next to the bytes the kernel in front of each gap stored.
Per boundary: the time from the latest exit of any workgroup of a kernel to the first entry of the next one (s_memrealtime, 100 MHz, one clock for all XCDs),
median and quartiles over the sweeps sampled, and the median time of the kernel in front from its first entry to its last exit.  The stamps keep one sweep (atomicMax), so every sample is the second sweep of a two-sweep run call, whose
Gram follows the first sweep's back-projection under graph replay.  Back-projection -> next Gram is not stamped (the earlier sweep's words are overwritten): it is
derived as the wall time per sweep of one long run minus the stamped span Gram entry .. back-projection exit.
Usage: stamps_boundaries.py <chains> [samples] [n V R] [option=value ...]"""
import sys, os, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, bnr_amd
args = [a for a in sys.argv[1:] if "=" not in a]
opts = [a for a in sys.argv[1:] if "=" in a]
nb = int(args[0]) if args else 1
ns = int(args[1]) if len(args) > 1 else 200
n, V, R = (int(args[2]), int(args[3]), int(args[4])) if len(args) >= 5 else (500, 100, 7)
X, y, _ = bnr_amd.make_synthetic(n, V, R, seed=20240501)
tot = 2 * ns + 12 + 400
chains = [bnr_amd.Chain(X, y, R, tot, 20240501, 1)]
chains += [bnr_amd.Chain.like(chains[0], 20240501, c, tot) for c in range(2, nb + 1)]
for ch in chains: ch.init_prior()
r = bnr_amd.Group(chains) if nb > 1 else chains[0]
for kv in opts:
    k, v = kv.split("="); r.set_option(k, int(v))
r.run(2, 11, 11)
n_pad = (n + 63) // 64 * 64
nbk, ntile = n_pad // 32, n_pad // 64
ntl = ntile * (ntile + 1) // 2
plan = (bnr_amd._capi.C.c_int32 * 4)()
bnr_amd._capi.check(bnr_amd._capi.lib().bnr_host_gram_plan(n, V, 256, plan))
ksplit = plan[0]
KIND = {"gram": 0, "solve_w": 1, "solve_a4": 2, "backproj": 3, "psum": 4}      # (psum: the back-projection's sums as a launch of their own, split_sums)


def sample():
    d = np.stack([ch.debug_read(4096).astype(np.int64) for ch in chains])
    ev = {}
    for name, k in KIND.items():
        w = d[:, 4000 + 4 * k: 4000 + 4 * k + 3]
        ev[name] = (w[:, 0].min() if w[:, 0].max() else w[:, 1].min(), w[:, 2].max())
    for p in range(nbk):
        w = d[:, 8 * p: 8 * p + 8]
        ev["chol %d" % p] = (w[:, 1].min(), max(w[:, 5].max(), w[:, 7].max()))
    return ev


order = ["gram"] + ["chol %d" % p for p in range(nbk)] + ["solve_w"]
pairs = list(zip(order[:-1], order[1:])) + [("solve_a4", "backproj")]
gaps = {pr: [] for pr in pairs}
dur = {a: [] for a, _ in pairs}                                  # the kernel in front of the gap: first entry to last exit
span = []
for i in range(ns):
    f = 12 + 2 * i
    r.run(f, f + 1, f + 1)
    ev = sample()
    for a, b in pairs:
        gaps[(a, b)].append((ev[b][0] - ev[a][1]) / 100.0)
        dur[a].append((ev[a][1] - ev[a][0]) / 100.0)
    span.append((max(ev["backproj"][1], ev["psum"][1]) - ev["gram"][0]) / 100.0)
f = 12 + 2 * ns
bnr_amd.device_synchronize(0)
t0 = time.perf_counter()
r.run(f, f + 399, f + 399)
bnr_amd.device_synchronize(0)
per = 1e6 * (time.perf_counter() - t0) / 400


def stored(name):
    """bytes one chain's kernel leaves behind (8-byte elements, 32 x 32 blocks of 8 KiB)"""
    if name == "gram":
        return ksplit * ntl * 64 * 64 * 8
    if name == "solve_a4":
        return 2 * n_pad * 8
    p = int(name.split()[1])
    npanel = nbk - p                                            # the swept blocks of column p below and on the diagonal...
    if p == 0:
        return ntl * 64 * 64 * 8 + (n_pad * n_pad // 2) * 8     # E's lower tiles and Y = I (block upper triangle)
    m = nbk - (p + 1)
    return (npanel + m * (m + 1) // 2 + m * p) * 8192           # panel column + trailing blocks + identity rows of the trailing columns


print("%d chain(s), n=%d V=%d R=%d, K split %d: %d sweeps sampled; gap = next kernel's first entry - this kernel's last exit, us" % (nb, n, V, R, ksplit, ns))
print("  %-22s %9s %9s %9s %12s %14s" % ("boundary", "median", "q25", "q75", "stored MB", "kernel in front"))
for a, b in pairs:
    g = np.array(gaps[(a, b)])
    print("  %-22s %9.2f %9.2f %9.2f %12.2f %14.2f" % (a + " -> " + b, np.median(g), np.percentile(g, 25), np.percentile(g, 75), nb * stored(a) / 1e6, np.median(dur[a])))
steps = np.array([np.median(gaps[pr]) for pr in pairs[2:nbk]])
print("  sum of the gaps chol 1 -> ... -> chol %d: %.2f us; mean %.2f; sum of those steps' kernels (first entry to last exit): %.2f us"
      % (nbk - 1, steps.sum(), steps.mean(), sum(np.median(dur["chol %d" % p]) for p in range(1, nbk - 1))))
print("  stamped span Gram entry .. back-projection exit: median %.2f us; wall time per sweep over 400 sweeps: %.2f us; back-projection -> next Gram (derived): %.2f us"
      % (np.median(span), per, per - np.median(span)))
if nb > 1: r.close()
for ch in chains: ch.close()
