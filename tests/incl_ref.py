"""The joint summary of an S x B matrix of 0/1 indicators (ABI 15) by brute force, in plain Python integers and collections.Counter over tuples:
independent of numpy's unique and packbits, which the package's restatement api._host_inclusion uses.  Also the case matrices that
tests/test_inclusion_host.py and tests/test_inclusion_gpu.py share, and the comparison of two results.  numpy only builds the matrices."""
import collections
import functools

import numpy as np

FIELDS = ("prob", "joint", "size_pmf", "n_distinct", "top_sets", "top_count")
S_GRID = (1, 2, 63, 64, 65, 257, 4097)
B_GRID = (1, 16, 63, 64, 65, 130)
NTOPS = (1, 4, 256)
MASK = (1 << 64) - 1


def brute(z, ntop):
    """dict of FIELDS, every number from integer counts: draws, indicator columns and patterns as Python ints"""
    rows = ["".join("1" if v != 0 else "0" for v in r) for r in np.asarray(z).tolist()]          # a draw as a string of B digits, indicator 0 first
    S, B = len(rows), len(rows[0])
    W = (B + 63) // 64
    cols = [int("".join(c)[::-1], 2) for c in zip(*rows)]                             # indicator k over the draws as one integer, draw 0 the lowest bit
    marg = [bin(c).count("1") for c in cols]
    joint = [[bin(cols[k] & cols[l]).count("1") for l in range(B)] for k in range(B)]
    sizes = collections.Counter(r.count("1") for r in rows)
    pats = collections.Counter(int(r[::-1], 2) for r in rows)                         # P = sum_k z_k 2^k
    ranked = sorted(pats.items(), key=lambda pc: (-pc[1], pc[0]))[:ntop]              # count descending, then the pattern as an integer
    top_sets = [[(p >> (64 * w)) & MASK for w in range(W)] for p, _ in ranked] + [[0] * W] * (ntop - len(ranked))
    top_count = [c for _, c in ranked] + [0] * (ntop - len(ranked))
    return dict(prob=np.array([m / S for m in marg]), joint=np.array(joint, dtype=np.int64).reshape(B, B) / float(S),
                size_pmf=np.array([sizes.get(m, 0) / S for m in range(B + 1)]), n_distinct=len(pats),
                top_sets=np.array(top_sets, dtype=np.uint64).reshape(ntop, W), top_count=np.array(top_count, dtype=np.int64))


def same(got, want, what, fields=FIELDS):
    """every field of `got` (a dict or the tuple of FIELDS) that `fields` names has the bits of `want`'s"""
    got = dict(zip(FIELDS, got)) if not isinstance(got, dict) else got
    for f in fields:
        g, w = got[f], want[f]
        if f == "n_distinct":
            assert int(g) == int(w), (what, f, g, w)
            continue
        g, w = np.asarray(g), np.asarray(w)
        assert g.shape == w.shape and g.dtype == w.dtype, (what, f, g.shape, w.shape, g.dtype, w.dtype)
        assert np.array_equal(g.view(np.uint64) if g.dtype == np.float64 else g, w.view(np.uint64) if w.dtype == np.float64 else w), (what, f)


# ------------------------------------------------------------------------------------------------------------------ the case matrices
def bernoulli(S, B, seed=0):
    """z_sk ~ Bernoulli(p_k), p_k spread over (0.02, 0.98)"""
    rng = np.random.default_rng([15, S, B, seed])
    p = 0.02 + 0.96 * (np.arange(B) + 0.5) / B
    return (rng.random((S, B)) < p).astype(np.uint8)


def five_rows(S, B):
    """only 5 distinct rows (fewer where 2^B or S is smaller), dealt round-robin and then shuffled: their counts are equal or differ by one, so
    the order among equal counts is decided by the tie rule"""
    rng = np.random.default_rng([16, S, B])
    base = np.unique((rng.random((5, B)) < 0.5).astype(np.uint8), axis=0)
    z = base[np.arange(S) % base.shape[0]]
    return z[rng.permutation(S)]


def one_bit(S, B, k):
    """rows that differ only in indicator k: a fixed random row, indicator k set in every third draw"""
    rng = np.random.default_rng([17, S, B, k])
    z = np.tile((rng.random(B) < 0.5).astype(np.uint8), (S, 1))
    z[:, k] = np.arange(S) % 3 == 0
    return z


def families(S, B):
    return (("bernoulli", bernoulli(S, B)), ("five rows", five_rows(S, B)), ("highest bit", one_bit(S, B, B - 1)), ("lowest bit", one_bit(S, B, 0)))


def long_matrix():
    """S = 70 001 draws of B = 3 indicators: indices past 16 bits, runs of thousands"""
    return bernoulli(70001, 3, seed=1)


@functools.lru_cache(maxsize=None)
def grid_cases():
    """((name, S, B), z) over the whole grid, built once"""
    return tuple(((name, S, B), z) for S in S_GRID for B in B_GRID for name, z in families(S, B))
