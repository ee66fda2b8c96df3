"""Inputs that reach the edges of the radix sort behind k_rank, k_hdi and k_incl_group (bnr_sort_build_keys / bnr_sort_passes), of k_rank's
tie-run sweep and of k_hdi's searches, shared by tests/test_sort_edges_host.py and tests/test_sort_edges_gpu.py.

Rows are built from the bytes of the sort key.  For a finite double bnr_key_of is bits | 2^63 (positive) or ~bits (negative), so bytes 0-6 of
the key are those of the bit image and the top byte takes all 256 values on finite doubles.  Every key row is checked on the way out: no NaN,
and exactly the promised set of key bytes is not constant (computed as bnr_sort_build_keys does, -0 folded onto +0) -- that set is the set of
passes that run.  Everything is generated from fixed seeds, once (functools.lru_cache), and handed out read-only."""
import functools

import numpy as np

import hdi_cases as hc

U = np.uint64
TOP = U(1) << U(63)
KEY_LENGTHS = (255, 256, 257, 513, 1025)
TIE_LENGTHS = (257, 513, 1025, 1280, 4097)
SKIP_PATTERNS = ((0, 2), (0, 7), (3, 5), (1, 6), (0, 3, 7), (0, 1, 2, 3, 5, 6, 7))
SINGLETON_BYTES = (0, 3, 7)
SINGLETON_LENGTHS = (257, 1025)
LEVELS = hc.LEVELS
INCL_NTOPS = (1, 4, 256)


# ------------------------------------------------------------------------------------------------------------------ the key image
def key_of(x):
    """bnr_key_of of a NaN-free array behind the fold of bnr_sort_build_keys (-0 -> +0)"""
    x = np.ascontiguousarray(x, dtype=np.float64)
    assert not np.isnan(x).any()
    u = np.where(x == 0.0, 0.0, x).view(U)
    return np.where(u & TOP != 0, ~u, u | TOP)


def double_of(k):
    """bnr_double_of"""
    k = np.ascontiguousarray(k, dtype=U)
    return np.where(k & TOP != 0, k & ~TOP, ~k).view(np.float64)


def live_bytes(x):
    """the bytes of the row's keys that are not the same in every key: the passes that run"""
    k = key_of(x)
    return tuple(b for b in range(8) if np.unique((k >> U(8 * b)) & U(255)).size > 1)


def keys_from_digits(live, digits):
    """keys whose byte b is digits[b] for b in `live` and constant elsewhere.  Byte 7 not live: the positive doubles 0x3FF0... | d << 8 b (base
    0x3F00... where byte 6 is live).  Byte 7 live: (d << 56) | 0x0010..., decoded by bnr_double_of -- negative doubles for d < 128."""
    n = len(next(iter(digits.values())))
    if 7 in live:
        k = np.full(n, 0 if 6 in live else 0x0010 << 48, dtype=U)
    else:
        k = np.full(n, (0x3F00 if 6 in live else 0x3FF0) << 48, dtype=U) | TOP
    for b in live:
        d = np.asarray(digits[b], dtype=U)
        k = k | (d << U(8 * b))
    if 6 in live and 7 in live:                                         # exponent 0x7FF (Inf, NaN) and the two zeros: move byte 6 away
        x = double_of(k)
        bad = ~np.isfinite(x) | (x == 0.0)
        k = np.where(bad, (k & ~(U(0xFF) << U(48))) | (U(0x80) << U(48)), k)
    return k


def _checked(x, live):
    x = np.ascontiguousarray(x, dtype=np.float64)
    assert not np.isnan(x).any() and np.isfinite(x).all()
    assert live_bytes(x) == tuple(live), (live_bytes(x), live)
    return x


def _orders(x, rng):
    """the row shuffled, ascending and descending"""
    s = np.sort(x)
    return (("shuffled", x[rng.permutation(x.size)]), ("ascending", s), ("descending", s[::-1].copy()))


def _uneven_digits(S, b, rng):
    """S digits: every one of the 256 values where S >= 256 (the first S of them below), the heavy one -- 0 for even b, 255 for odd -- more than
    256 times where S > 512 (in a presorted row it then fills a whole tile, all four waves), half of the rest exactly once"""
    if S <= 256:
        return np.arange(S) if b % 2 == 0 else 255 - np.arange(S)
    heavy = 0 if b % 2 == 0 else 255
    d = list(range(256))
    rest = S - 256
    take = min(rest, 299) if rest > 256 else rest // 2
    d += [heavy] * take
    d += list(rng.choice(np.arange(1, 255, 2), size=rest - take))       # odd values only: the even ones 2 .. 254 stay singletons
    return np.array(d)


def _add(out, name, x, live):
    x = _checked(x, live)
    out.append((name, x))
    out.append((name + " negated", _checked(-x, live)))                 # the complement of every key byte


@functools.lru_cache(maxsize=None)
def key_rows():
    """[(name, row)] of the three key families"""
    out = []
    for S in KEY_LENGTHS:
        for b in range(8):
            rng = np.random.default_rng([101, S, b])
            x = double_of(keys_from_digits((b,), {b: _uneven_digits(S, b, rng)}))
            if S >= 256:
                assert np.unique((key_of(x) >> U(8 * b)) & U(255)).size == 256
            for o, r in _orders(x, rng):
                _add(out, "one live byte %d, S=%d, %s" % (b, S, o), r, (b,))
        for live in SKIP_PATTERNS:
            rng = np.random.default_rng([102, S] + list(live))
            x = double_of(keys_from_digits(live, {b: rng.integers(0, 256, size=S) for b in live}))
            for o, r in _orders(x, rng):
                _add(out, "live bytes %s, S=%d, %s" % ("".join(map(str, live)), S, o), r, live)
    for S in SINGLETON_LENGTHS:
        for b in SINGLETON_BYTES:
            rng = np.random.default_rng([103, S, b])
            x = double_of(keys_from_digits((b,), {b: _uneven_digits(S, b, rng)}))
            x = x[rng.permutation(S)]
            dig = (key_of(x) >> U(8 * b)) & U(255)
            vals, cnt = np.unique(dig, return_counts=True)
            single = vals[cnt == 1]
            at = int(np.flatnonzero(dig == single[single.size // 2])[0])
            for pos in (0, 63, 64, 255, 256, S - 1):
                r = x.copy()
                r[[pos, at]] = r[[at, pos]]
                d2 = (key_of(r) >> U(8 * b)) & U(255)
                assert np.count_nonzero(d2 == d2[pos]) == 1
                _add(out, "singleton digit of byte %d at %d, S=%d" % (b, pos, S), r, (b,))
    return tuple((n, _ro(r)) for n, r in out)


def _ro(a):
    a = np.ascontiguousarray(a)
    a.setflags(write=False)
    return a


# ------------------------------------------------------------------------------------------------------------------ tie runs
STAIRCASE = (1, 1, 62, 1, 63, 64, 65, 1, 190, 256, 257, 1, 511, 1, 512, 513, 1, 255, 1, 1024)
CARRY = (255, 1, 800, 1, 1)


def _runs(pattern, S, fill):
    """run lengths that sum to S: `pattern`, cut at S; what is left goes to runs of `fill` (0: one last run)"""
    runs, left = [], S
    for r in pattern:
        if left == 0:
            break
        runs.append(min(r, left))
        left -= runs[-1]
    while left > 0:
        runs.append(left if fill == 0 else min(fill, left))
        left -= runs[-1]
    return runs


def row_of_runs(runs, rng):
    """small integers -- run k of the sorted row holds k - (number of runs) // 2, so negatives, a zero and positives --, positions shuffled"""
    v = np.repeat(np.arange(len(runs), dtype=np.float64) - len(runs) // 2, runs)
    return v[rng.permutation(v.size)]


def run_heads(x):
    """the sorted positions at which a run begins"""
    s = np.sort(np.asarray(x) + 0.0)
    return np.flatnonzero(np.append(True, s[1:] != s[:-1]))


@functools.lru_cache(maxsize=None)
def tie_rows():
    """[(name, row)] of the four tie-run families"""
    out = []
    for S in TIE_LENGTHS:
        rng = np.random.default_rng([104, S])
        out.append(("staircase S=%d" % S, row_of_runs(_runs(STAIRCASE, S, 0), rng)))
        runs = _runs(CARRY, S, 1)
        x = row_of_runs(runs, rng)
        heads = run_heads(x)
        assert heads[1] == 255 and heads[2] == 256 and (S <= 1056 or (heads[3] == 1056 and not np.any((heads > 256) & (heads < 1056))))
        out.append(("carry through headless tiles S=%d" % S, x))
        i = np.arange(S, dtype=np.float64) - S // 2
        first2, last2 = i.copy(), i.copy()
        first2[1], last2[-2] = first2[0], last2[-1]
        out.append(("distinct but the first two S=%d" % S, first2[rng.permutation(S)]))
        out.append(("distinct but the last two S=%d" % S, last2[rng.permutation(S)]))
    for S in (257, 513, 1025):
        rng = np.random.default_rng([105, S])
        body = _runs((100, 156, 256, 512), S - 1, 0)
        x = row_of_runs(body + [1], rng)
        assert run_heads(x)[-1] == S - 1 and (S - 1) % 256 == 0
        out.append(("last head on a tile's first lane S=%d" % S, x))
        x = row_of_runs([1, 255, S - 256], rng)
        assert run_heads(x)[-1] == 256
        out.append(("last run long, from a tile's first lane to n, S=%d" % S, x))
        out.append(("last run long, from mid-tile to n, S=%d" % S, row_of_runs([1, 99, S - 100], rng)))
    return tuple((n, _ro(r)) for n, r in out)


# ------------------------------------------------------------------------------------------------------------------ HDI rows
PLANTED = ((300, 100), (256, 255), (512, 1), (511, 256, 1))
PLANTED_LENGTHS = (1025, 1280)
PLANTED_LONG = (4097, 0.9, ((300, 100), (256, 255)))                    # (S, level, starts): the level 0.9 has more than 256 windows from S = 2561 on


def planted_row(S, prob, starts, rng):
    """integer draws whose windows of w = floor(prob S) + 1 order statistics have their smallest width exactly at the start indices `starts`:
    d_j = D + o_j with o_j = 0 there and 1 + j % 3 elsewhere, made by the gaps g_j = 10 (j < w) and g_(j+w) = 10 + o_(j+1) - o_j"""
    w = int(np.floor(prob * S))
    m = S - w
    assert w >= m - 1 and max(starts) < m
    o = 1 + np.arange(m) % 3
    o[list(starts)] = 0
    g = np.full(S - 1, 10, dtype=np.int64)
    g[w:w + m - 1] = 10 + np.diff(o)
    xs = np.concatenate([[0], np.cumsum(g)]).astype(np.float64)
    xs -= xs[S // 3]                                                    # a zero, negatives and positives
    d = xs[w:] - xs[:m]
    assert sorted(np.flatnonzero(d == d.min())) == sorted(starts)
    assert min(starts) % 256 > min(j % 256 for j in starts if j != min(starts))      # the first minimum is not the lowest thread's
    return xs[rng.permutation(S)]


def w_levels(S):
    """levels whose window lengths floor(prob S) are 0, 1, S - 2 and S - 1: bnr_hdi accepts every level in (0, 1) and caps w at S - 1, so 0 is
    the smallest window length it takes and S - 1 the largest"""
    pr = (0.5 / S, 1.5 / S, (S - 1.5) / S, (S - 0.5) / S)
    assert [int(np.floor(p * S)) for p in pr] == [0, 1, S - 2, S - 1] and all(0.0 < p < 1.0 for p in pr)
    return pr


def zero_block_row(n, first, last, rng):
    """sorted: `first` negatives, then a block of mixed -0 / +0 up to sorted position `last` (inclusive), then positives"""
    neg = -np.arange(first, 0, -1, dtype=np.float64)
    zeros = np.where(np.arange(last - first + 1) % 2 == 0, -0.0, 0.0)
    pos = np.arange(1, n - last, dtype=np.float64)
    x = np.concatenate([neg, zeros, pos])
    assert x.size == n
    return x[rng.permutation(n)]


@functools.lru_cache(maxsize=None)
def hdi_rows():
    """[(name, row, levels)] of the three HDI families"""
    out = []
    for S in PLANTED_LENGTHS:
        for starts in PLANTED:
            rng = np.random.default_rng([106, S] + list(starts))
            out.append(("minimal width planted at %s, S=%d" % (starts, S), planted_row(S, 0.5, starts, rng), LEVELS))
    S, prob, pairs = PLANTED_LONG
    for starts in pairs:
        rng = np.random.default_rng([106, S] + list(starts))
        out.append(("minimal width planted at %s for the level %g, S=%d" % (starts, prob, S), planted_row(S, prob, starts, rng), LEVELS))
    for S in (257, 1025):
        rng = np.random.default_rng([107, S])
        out.append(("the ends of w, normal draws, S=%d" % S, rng.standard_normal(S), w_levels(S)))
        out.append(("the ends of w, integer draws with ties, S=%d" % S, rng.integers(-40, 41, size=S).astype(np.float64), w_levels(S)))
    for n in (257, 513):
        rng = np.random.default_rng([108, n])
        i = np.arange(1, n + 1, dtype=np.float64)
        out.append(("all negative, n=%d" % n, -i[rng.permutation(n)], LEVELS))
        out.append(("all positive, n=%d" % n, i[rng.permutation(n)], LEVELS))
        out.append(("all +-0, n=%d" % n, np.where(rng.random(n) < 0.5, -0.0, 0.0), LEVELS))
        edges = sorted({0, 1, 255, 256, n - 1})
        for first in edges:
            for last in edges:
                if first <= last:
                    out.append(("zeros at sorted %d..%d, n=%d" % (first, last, n), zero_block_row(n, first, last, rng), LEVELS))
    return tuple((n, _ro(r), lv) for n, r, lv in out)


def by_length(rows):
    """{S: (names, matrix of the rows of length S)}: one device call per length"""
    groups = {}
    for name, r in rows:
        groups.setdefault(r.size, []).append((name, r))
    return {S: ([n for n, _ in g], _ro(np.stack([r for _, r in g]))) for S, g in sorted(groups.items())}


@functools.lru_cache(maxsize=None)
def rank_matrices():
    """the key and tie families by row length"""
    return by_length(key_rows() + tie_rows())


@functools.lru_cache(maxsize=None)
def hdi_matrices():
    """[(levels, names, matrix)]: the key and tie families at LEVELS by row length, the HDI families by (levels, row length)"""
    out = [(LEVELS, names, M) for names, M in rank_matrices().values()]
    groups = {}
    for name, r, lv in hdi_rows():
        groups.setdefault((lv, r.size), []).append((name, r))
    out += [(lv, [n for n, _ in g], _ro(np.stack([r for _, r in g]))) for (lv, _), g in groups.items()]
    return tuple(out)


# ------------------------------------------------------------------------------------------------------------------ inclusion matrices
def bits_of(words, B):
    """the S x B byte matrix of patterns given as S x W uint64 words (bit k % 64 of word k // 64 is indicator k)"""
    words = np.ascontiguousarray(words, dtype="<u8")
    return np.unpackbits(words.view(np.uint8), axis=1, bitorder="little")[:, :B].copy()


def _random_words(rng, shape):
    return rng.integers(0, 2 ** 63, size=shape, dtype=np.uint64) * U(2) + rng.integers(0, 2, size=shape, dtype=np.uint64)


def _mask(B, W):
    m = np.full(W, ~U(0), dtype=U)
    if B % 64:
        m[W - 1] = (U(1) << U(B % 64)) - U(1)
    return m


@functools.lru_cache(maxsize=None)
def inclusion_cases():
    """[(name, S x B uint8 matrix)] of the inclusion families"""
    out = []
    for B in (64, 65, 128, 130):
        W = (B + 63) // 64
        for wd in range(W):
            for byte in (0, 3, 7):
                if wd * 64 + byte * 8 >= B:
                    continue                                            # the byte lies past the last indicator
                for S in (257, 1025):
                    rng = np.random.default_rng([109, B, wd, byte, S])
                    words = np.tile(_random_words(rng, W) & _mask(B, W), (S, 1))
                    words[:, wd] &= ~(U(0xFF) << U(8 * byte))
                    words[:, wd] |= rng.integers(0, 256, size=S, dtype=np.uint64) << U(8 * byte)
                    words &= _mask(B, W)
                    out.append(("one byte differs: B=%d word %d byte %d S=%d" % (B, wd, byte, S), bits_of(words, B)))
    for B in (16, 64, 130):
        W = (B + 63) // 64
        for S in (257, 1025):
            rng = np.random.default_rng([110, B, S])
            where = rng.choice(B, size=11, replace=False)               # the 11 bits of the draw's label, scattered over the words
            label = rng.permutation(2048)[:S]
            z = np.tile((rng.random(B) < 0.5).astype(np.uint8), (S, 1))
            for i, k in enumerate(where):
                z[:, k] = (label >> i) & 1
            assert np.unique(z, axis=0).shape[0] == S
            out.append(("every draw distinct: B=%d S=%d" % (B, S), z))
    counts = (300, 299, 256, 255, 2, 1, 1)
    for B in (64, 130):
        W = (B + 63) // 64
        rng = np.random.default_rng([111, B])
        pats = _random_words(rng, (len(counts), W)) & _mask(B, W)
        pats[6] = pats[5]                                               # the two patterns of count 1 differ in their top word alone, the
        pats[6, W - 1] ^= U(2)                                          # two of 300 and 299 in word 0 alone
        pats[1] = pats[0]
        pats[1, 0] ^= U(1) << U(40)
        assert np.unique(pats, axis=0).shape[0] == len(counts)
        words = np.repeat(pats, counts, axis=0)[rng.permutation(sum(counts))]
        out.append(("counts %s: B=%d" % (counts, B), bits_of(words, B)))
    return tuple((n, _ro(z)) for n, z in out)


# ------------------------------------------------------------------------------------------------------------------ the chain path
CHAIN_WINDOWS = ((38, 601, 150), (3, 101, 25))                          # (first_row, nsamp, max_lag), with 3 chains pooled and with 1
CHAIN_SETS = 4                                                          # sets of tables: 4 x 136 gamma columns hold all 521 key and tie rows
CHAIN_ROWS = 3 * 640
MODERATE_TOP = np.concatenate([np.arange(0x21, 0x5F), np.arange(0xA1, 0xDF)]).astype(U)


def moderate(x):
    """the row with the top byte of every key mapped, in order, onto the 124 values that keep |x| inside 2^-495 .. 2^497: the chains' moments
    (k_acov's sums of squares, behind ess_mean and mcse_mean) overflow on draws near 1e300, and whether an overflowed sum ends as Inf or NaN
    depends on the order of its terms, which is not what these rows are about.  The live bytes stay what they were.  Only the tables of the
    rank diagnostics hold these; the order statistics and the HDIs are taken of the full-range rows."""
    k = key_of(x)
    top = MODERATE_TOP[((k >> U(56)) * U(MODERATE_TOP.size) // U(256)).astype(np.int64)]
    y = double_of((k & ~(U(0xFF) << U(56))) | (top << U(56)))
    assert live_bytes(y) == live_bytes(x) and np.all(np.abs(y) < 2.0 ** 497) and np.all(np.abs(y) > 2.0 ** -496)
    return y


def _is_wide(r):
    nz = np.abs(r[r != 0.0])
    return nz.size > 0 and (nz.max() >= 2.0 ** 497 or nz.min() <= 2.0 ** -496)


def ranked_rows(first, nsamp):
    """the 0-based table rows of one chain that k_rank ranks in the window: both halves, without the middle row of an odd window"""
    h = nsamp // 2
    return np.concatenate([np.arange(first - 1, first - 1 + h), np.arange(first - 1 + nsamp - h, first - 1 + nsamp)])


def placed_column(pattern, fill, nch, first, nsamp, rng):
    """3 x 640 draws whose ranked draws -- the split halves of the window in the first `nch` chains -- are exactly the tie runs of `pattern`
    (sorting forgets where a draw came from, so only this multiset matters); every other entry is a large value of its own"""
    rows = ranked_rows(first, nsamp)
    col = 1e6 + np.arange(CHAIN_ROWS, dtype=np.float64)
    at = np.concatenate([c * 640 + rows for c in range(nch)])
    col[at] = row_of_runs(_runs(pattern, at.size, fill), rng)
    return col


@functools.lru_cache(maxsize=None)
def chain_columns():
    """the CHAIN_SETS x 136 = 544 (name, 3 x 640 draws, the same for the rank diagnostics) that become gamma columns: every key and tie row,
    repeated or cut to 3 x 640 draws (521); the staircase and the headless-tile runs placed for each of the four (window, chains) cases (8);
    15 rows of the HDI families to fill up.  A row of the full exponent range goes to the rank diagnostics as moderate() makes it."""
    cols = [(n, np.resize(r, CHAIN_ROWS)) for n, r in key_rows() + tie_rows()]
    for first, nsamp, _lag in CHAIN_WINDOWS:
        for nch in (3, 1):
            rng = np.random.default_rng([112, first, nsamp, nch])
            what = "placed for %d chain(s), window (%d, %d)" % (nch, first, nsamp)
            cols.append(("staircase " + what, placed_column(STAIRCASE, 0, nch, first, nsamp, rng)))
            cols.append(("carry through headless tiles " + what, placed_column(CARRY, 1, nch, first, nsamp, rng)))
    cols += [(n, np.resize(r, CHAIN_ROWS)) for n, r, lv in hdi_rows() if lv == LEVELS][:CHAIN_SETS * 136 - len(cols)]
    assert len(cols) == CHAIN_SETS * 136
    return tuple((n, _ro(c), _ro(moderate(c)) if _is_wide(c) else _ro(c)) for n, c in cols)


@functools.lru_cache(maxsize=None)
def chain_tables(k, moderated=False):
    """set k of rank_diag_cases.tables() -- three chains of 640 rows, V = 16, R = 2 -- with gamma column j holding chain_columns()[136 k + j],
    dealt to the chains in blocks of 640; the xi columns stay the crafted ones"""
    import diag_ref as dr
    import rank_diag_cases as rc
    cols = chain_columns()[dr.Q * k:dr.Q * (k + 1)]
    assert dr.Q == 136 and len(cols) == dr.Q
    tabs = []
    for c, t in enumerate(rc.tables()):
        t = dict(t)
        g = np.empty((dr.TOT, dr.Q, 1), order="F")
        for j, col in enumerate(cols):
            g[:, j, 0] = col[2 if moderated else 1][c * dr.TOT:(c + 1) * dr.TOT]
        t["gamma"] = g
        tabs.append(t)
    return tuple(tabs)


def chain_names(k):
    return [c[0] for c in chain_columns()[136 * k:136 * (k + 1)]]
