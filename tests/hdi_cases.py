"""What tests/test_hdi_host.py and tests/test_hdi_gpu.py share: the levels, the rows of the kernel's direct test and the comparison of bits."""
import numpy as np

import diag_ref as dr

LEVELS = (0.5, 0.9, 0.95)
FIELDS = ("lower", "upper", "median", "p_pos", "p_neg")
ROW_LENGTHS = (1, 2, 3, 63, 64, 65, 255, 256, 257, 1280, 4097)


def rows(S, seed=7):
    """the eight rows of test_rank_diag_gpu._rows: normal, constant, 0/1, clipped normal (ties at both ends), denormals, +-Inf, two ramps"""
    rng = np.random.default_rng([seed, S])
    x = rng.standard_normal(S)
    i = np.arange(S, dtype=np.float64)
    return np.stack([x, np.full(S, -1.5), (rng.random(S) < 0.3).astype(np.float64), np.clip(rng.standard_normal(S), -1.2, 1.2),
                     dr.special_column("denormal", S, 0, rng), dr.special_column("inf_both", S, 0, rng), -2.0 + 3.5 * i / S, 5.0 - 0.25 * i])


def long_row():
    return np.clip(np.random.default_rng(70001).standard_normal((1, 70001)), -1.2, 1.2)


def same_bits(a, b):
    """equal shapes, NaN in the same places, and the same 64 bits everywhere else"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    if a.shape != b.shape or not np.array_equal(np.isnan(a), np.isnan(b)):
        return False
    ok = ~np.isnan(a)
    return np.array_equal(a[ok].view(np.uint64), b[ok].view(np.uint64))
