"""The posterior covariance of ABI 17 by its definition, in Python integers and fractions.Fraction: no rounding anywhere.

For K chains of nsamp draws of m columns (x[k][s][a], any numbers that Fraction takes exactly -- every float64 is one):
  centre      c_a = sum_{k, s} x_ksa / (K nsamp)                 (no weights: the pooled mean)
              c_a = sum_k w_k (sum_s x_ksa / nsamp)              (chain weights w)
  per chain   G_k[a][b] = sum_s (x_ksa - c_a) (x_ksb - c_b)
  cov[a][b]   = sum_k G_k[a][b] / (K nsamp - 1)                  (no weights: numpy's cov)
              = sum_k w_k G_k[a][b] / nsamp                      (weights: the covariance of the mixture sum_k w_k P_k)
The cases of the GPU test are built here too: integer draws whose centre is an integer, so that float64 is exact as well."""
from fractions import Fraction

import numpy as np


def exact(x, weights=None):
    """(centres [m], per-chain sums [K][m][m], cov [m][m]) as Fractions, for x of shape (K, nsamp, m)"""
    x = np.asarray(x, dtype=np.float64)
    K, ns, m = x.shape
    num = lambda v: int(v) if float(v).is_integer() else Fraction(float(v))        # (whole numbers stay Python integers: the same values, faster)
    whole = lambda f: int(f) if f.denominator == 1 else f
    col = [[[num(x[k, s, a]) for s in range(ns)] for a in range(m)] for k in range(K)]
    w = None if weights is None else [Fraction(float(v)) for v in weights]
    c = []
    for a in range(m):
        if w is None:
            c.append(Fraction(sum(sum(col[k][a]) for k in range(K))) / (K * ns))
        else:
            c.append(sum((w[k] * (Fraction(sum(col[k][a])) / ns) for k in range(K)), Fraction(0)))
    dev = [[[v - whole(c[a]) for v in col[k][a]] for a in range(m)] for k in range(K)]
    G = [[[None] * m for _ in range(m)] for _ in range(K)]
    for k in range(K):
        for a in range(m):
            for b in range(a, m):
                G[k][a][b] = G[k][b][a] = Fraction(sum(p * q for p, q in zip(dev[k][a], dev[k][b])))
    if w is None:
        cov = [[sum((G[k][a][b] for k in range(K)), Fraction(0)) / (K * ns - 1) for b in range(m)] for a in range(m)]
    else:
        cov = [[sum((w[k] * G[k][a][b] for k in range(K)), Fraction(0)) / ns for b in range(m)] for a in range(m)]
    return c, G, cov


def as_float(rows):
    """a list (of lists) of Fractions rounded once to float64"""
    return np.array([[float(v) for v in r] for r in rows]) if isinstance(rows[0], list) else np.array([float(v) for v in rows])


# the shapes of the issue: every side of the 16-column MFMA tile, the K tail of the 16-draw step, one to three chains
MS = (1, 15, 16, 17, 33)
NSAMPS = (2, 3, 5, 63, 64, 65)
KS = (1, 2, 3)
DYADIC = {2: ((0.5, 0.5), (1.0, 0.0)), 3: ((0.5, 0.25, 0.25), (0.0, 1.0, 0.0))}


def integer_case(K, nsamp, m, weights=None, seed=0):
    """x (K, nsamp, m): integer draws |x| <= 2^10 whose centre is an integer.  No weights: the second half of the pooled draws mirrors the
    first about an integer per column (an odd count keeps one draw at that integer).  Weights (nsamp even): every chain mirrors its own first
    half about the same integer, so every chain's mean -- and any weighted mean -- is that integer."""
    rng = np.random.default_rng([17, K, nsamp, m, seed])
    mid = rng.integers(-400, 401, size=m)
    if weights is None:
        S = K * nsamp
        half = rng.integers(-600, 601, size=(S // 2, m))
        parts = [mid + half, mid - half[::-1]] + ([mid[None, :]] if S % 2 else [])
        flat = np.concatenate(parts, axis=0)
        flat = flat[rng.permutation(S)]
        return flat.reshape(K, nsamp, m).astype(np.float64)
    assert nsamp % 2 == 0
    half = rng.integers(-600, 601, size=(K, nsamp // 2, m))
    x = np.concatenate([mid + half, mid - half], axis=1)
    for k in range(K):
        x[k] = x[k][rng.permutation(nsamp)]
    return x.astype(np.float64)


def integer_cases():
    """(K, nsamp, m, weights or None) of the exact-input tests: every shape without weights, and the dyadic weight sets at the power-of-two windows"""
    out = [(K, ns, m, None) for K in KS for ns in NSAMPS for m in MS if K * ns >= 2]
    out += [(K, ns, m, w) for K in (2, 3) for w in DYADIC[K] for ns in (2, 64) for m in MS]
    return out
