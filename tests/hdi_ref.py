"""Independent yardsticks of the highest-density interval of a sample, shared by tests/test_hdi_host.py and tests/test_hdi_gpu.py.

hdi(): a transcription of ArviZ's `_hdi` (arviz/stats/stats.py; the unimodal branch) and, equally, of R's HDInterval::hdi.default: a sorted
copy, interval_idx_inc = int(floor(prob n)), n_intervals = n - interval_idx_inc, the widths of the n_intervals windows, the FIRST minimum.
no_shorter_window(): the brute-force statement of what that means -- no window of w + 1 consecutive order statistics is shorter, and none
of equal width starts earlier.  arviz itself is compared where it can be imported."""
import numpy as np


def hdi(ary, hdi_prob):
    ary = np.asarray(ary, dtype=np.float64).flatten()
    n = len(ary)
    ary = np.sort(ary)
    interval_idx_inc = int(np.floor(hdi_prob * n))
    n_intervals = n - interval_idx_inc
    interval_width = np.subtract(ary[interval_idx_inc:], ary[:n_intervals], dtype=np.float64)
    if len(interval_width) == 0:
        raise ValueError("Too few elements for interval calculation.")
    min_idx = np.argmin(interval_width)
    hdi_min = ary[min_idx]
    hdi_max = ary[min_idx + interval_idx_inc]
    return hdi_min, hdi_max


def no_shorter_window(ary, hdi_prob, lower, upper):
    """True when [lower, upper] is a window of w + 1 consecutive order statistics of `ary`, w = floor(hdi_prob n), no other such window is
    shorter and no window of the same width starts at a smaller order statistic (plain Python loop: for small samples)"""
    xs = sorted(float(v) for v in np.asarray(ary, dtype=np.float64).flatten())
    n = len(xs)
    w = int(np.floor(hdi_prob * n))
    best = None
    for j in range(n - w):
        d = xs[j + w] - xs[j]
        if best is None or d < best[0]:
            best = (d, j)
    return best is not None and xs[best[1]] == lower and xs[best[1] + w] == upper


def arviz_hdi(ary, hdi_prob):
    """arviz.hdi of the sample, or None where arviz is not installed"""
    try:
        import arviz
    except Exception:                                  # not installed here, or not importable with this numpy
        return None
    lo, hi = arviz.hdi(np.asarray(ary, dtype=np.float64), hdi_prob=hdi_prob)
    return float(lo), float(hi)
