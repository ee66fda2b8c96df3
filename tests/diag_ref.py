"""Long-double references, a-priori rounding bounds and float64 emulations for the convergence-diagnostic kernels, numpy only:
k_rhat_stats (the split-Rhat message), k_acov (the effective-sample-size message), k_summary (column mean and two order statistics),
and the crafted tables the host test and the GPU test feed them.

u = 2^-53, gamma_k = k u / (1 - k u) (linalg_ref.gamma_m): k successive float64 roundings change a value by at most gamma_k relatively.
The library is built with -ffp-contract=off, so every product and sum below is one rounding; a contracted form rounds less and stays inside.
All bounds assume that no intermediate overflows or underflows, which holds for every family of FAMILIES (products down to 1e-24 and up to
1e300, sums up to 320 x 1e300); the column mean of k_summary alone is also fed denormals and carries the absolute term 2^-1074 for them.

Every reference is evaluated in np.longdouble (64-bit significand on x86: eps = 2^-63); its own error is added to the bound it comes with
("slop"), and tests/test_diag_ref_host.py checks against fractions.Fraction that it is far inside that bound.
"""
import numpy as np

from linalg_ref import LD, U, gamma_m, ratio      # noqa: F401  (ratio is re-exported for the tests)

EPS_LD = float(np.finfo(LD).eps)
TINY = 2.0 ** -1074                                # spacing of the denormals: a quotient that underflows is off by at most half of it
NT = 256                                           # threads of k_acov / k_summary: the stride of their partial sums and of the lag loop


def mean_roundings(n):
    """roundings on any term of the mean of n values as k_acov / k_summary add them: thread t adds x[t], x[t + 256], ... (ceil(n / 256) - 1
    additions), the tree over the 256 partial sums has 8 levels, and one division"""
    return -(-n // NT) + 8


def up(x):
    """a float64 bound computed in floating point, nudged up past its own rounding"""
    return np.asarray(x, dtype=np.float64) * (1 + 1e-12)


# ------------------------------------------------------------------------------------------------------------ split statistics (k_rhat_stats)
def halves(par):
    """the two halves split-Rhat uses of a window par (nsamp x np): rows [0, h) and [nsamp - h, nsamp), h = nsamp // 2 (convergence.jl with the
    oracle's reading of copyto_split!: an odd window drops its middle row)"""
    nsamp = par.shape[0]
    h = nsamp // 2
    return h, (par[:h], par[nsamp - h:])


def split_stats_ref(par):
    """The k_rhat_stats message [mean0 | var0 | mean1 | var1] x np of a window par (nsamp x np float64) in long double, and its bound.

    Kernel order: s = x_0 + x_1 + ... serially (h - 1 additions), m^ = s / h: every x_i meets at most h roundings, so
        |m^ - m| <= db := gamma_h mean|x|.
    Second pass: d_i = fl(x_i - m^), fl(d_i d_i), serial sum (h - 1 additions), division by h - 1: at most 2 + 1 + (h - 1) + 1 = h + 3 roundings
    on a term, so v^ = (1 + theta) sum (x_i - m^)^2 / (h - 1), |theta| <= gamma_(h+3).  With m^ = m + delta the cross term vanishes
    (sum (x_i - m) = 0) and sum (x_i - m^)^2 = sum (x_i - m)^2 + h delta^2 exactly, so
        |v^ - v| <= gamma_(h+3) (v + h db^2 / (h - 1)) + h db^2 / (h - 1).
    Returns (ref, bound): (4, np) long double and (4, np) float64."""
    h, hs = halves(par)
    ref, bnd = [], []
    for x in hs:
        xl = x.astype(LD)
        mu = xl.sum(axis=0) / h
        c = xl - mu
        var = (c * c).sum(axis=0) / (h - 1)
        am = np.abs(x).sum(axis=0) / h
        db = gamma_m(h) * am
        dl = (h + 2) * EPS_LD * am                                          # the long-double mean's own error
        e2 = h * db * db / (h - 1)
        v64 = var.astype(np.float64)
        ref += [mu, var]
        bnd += [up(db + dl), up(gamma_m(h + 3) * (v64 + e2) + e2 + 2 * (h + 4) * EPS_LD * v64 + h * dl * dl / (h - 1))]
    return np.stack(ref), np.stack(bnd)


def emu_split_stats(par, ddof=1, second_start=None):
    """k_rhat_stats in float64 numpy, in the kernel's order.  Mutations: ddof=0 divides the variance by h; second_start=h starts the second half
    at row h (wrong for an odd window)."""
    nsamp = par.shape[0]
    h = nsamp // 2
    s1 = nsamp - h if second_start is None else second_start
    out = []
    for x in (par[:h], par[s1:s1 + h]):
        s = np.zeros(par.shape[1])
        for i in range(h):
            s = s + x[i]
        m = s / h
        v = np.zeros(par.shape[1])
        for i in range(h):
            d = x[i] - m
            v = v + d * d
        out += [m, v / (h - ddof)]
    return np.stack(out)


# ------------------------------------------------------------------------------------------------------------ autocovariances (k_acov)
def acov_ref(par, L):
    """The k_acov message [half][2 + L][np] = mean, var (1 / (h - 1)), acov_0 .. acov_(L-1) (1 / h) of a window, in long double, and its bound.

    Mean: mean_roundings(h) roundings on a term, |m^ - m| <= db := gamma_(ceil(h/256)+8) mean|x|.
    Lag t, n = h - t products: c^_i = fl(x_i - m^), fl(c^_i c^_(i+t)), serial sum (n - 1 additions), one division: at most n + 3 roundings, so
    a^_t = (1 + theta) sum_i (x_i - m^)(x_(i+t) - m^) / h with |theta| <= gamma_(n+3).  With c_i = x_i - m exact and m^ = m + delta,
        (x_i - m^)(x_(i+t) - m^) = c_i c_(i+t) - delta (c_i + c_(i+t)) + delta^2,
    so the bound has three terms,
        h |a^_t - a_t| <= gamma_(n+3) P' + db |sum_i (c_i + c_(i+t))| + n db^2,
    the rounding term on the products as the kernel sees them, P' = sum |c_i||c_(i+t)| + db sum (|c_i| + |c_(i+t)|) + n db^2, the first-order term
    in delta, and delta^2 n.  The variance is lag 0 with the divisor h - 1.
    Returns (ref, bound): (2, 2 + L, np) long double and float64."""
    h, hs = halves(par)
    npar = par.shape[1]
    ref = np.zeros((2, 2 + L, npar), dtype=LD)
    bnd = np.zeros((2, 2 + L, npar))
    for k, x in enumerate(hs):
        xl = x.astype(LD)
        mu = xl.sum(axis=0) / h
        c = xl - mu
        ca = np.abs(c).astype(np.float64)
        am = np.abs(x).sum(axis=0) / h
        db = gamma_m(mean_roundings(h)) * am
        dl = (h + 2) * EPS_LD * am
        ref[k, 0] = mu
        bnd[k, 0] = up(db + dl)
        for t in range(L):
            n = h - t
            a, b = c[:n], c[t:t + n]
            A = (a * b).sum(axis=0)
            P = (ca[:n] * ca[t:t + n]).sum(axis=0)
            S1 = (ca[:n] + ca[t:t + n]).sum(axis=0)
            B1 = np.abs((a + b).sum(axis=0)).astype(np.float64)
            err = gamma_m(n + 3) * (P + db * S1 + n * db * db) + db * B1 + n * db * db
            slop = 2 * (n + 4) * EPS_LD * P + dl * (B1 + 2 * n * dl) + n * dl * dl
            ref[k, 2 + t] = A / h
            bnd[k, 2 + t] = up((err + slop) / h)
            if t == 0:
                ref[k, 1] = A / (h - 1)
                bnd[k, 1] = up((err + slop) / (h - 1))
    return ref, bnd


def emu_mean(x):
    """the column means of x (n x np) as k_acov / k_summary add them: 256 thread-strided partial sums, an 8-level tree, one division"""
    n = x.shape[0]
    red = np.zeros((NT, x.shape[1]))
    for i0 in range(0, n, NT):
        blk = x[i0:i0 + NT]
        red[:blk.shape[0]] = red[:blk.shape[0]] + blk
    w = NT // 2
    while w > 0:
        red[:w] = red[:w] + red[w:2 * w]
        w //= 2
    return red[0] / n


def emu_acov(par, L, drop_last=False, alias_256=False):
    """k_acov in float64 numpy, in the kernel's order.  Mutations: drop_last leaves out the last product of every lag's sum; alias_256 computes
    lag t + 256 from the data of lag t (a lag loop that forgets its stride)."""
    h, hs = halves(par)
    out = np.zeros((2, 2 + L, par.shape[1]))
    for k, x in enumerate(hs):
        with np.errstate(all="ignore"):
            m = emu_mean(x)
            c = x - m
            out[k, 0] = m
            for t in range(L):
                td = t % NT if alias_256 else t
                n = h - td - (1 if drop_last else 0)
                s = np.zeros(par.shape[1])
                for i in range(n):
                    s = s + c[i] * c[i + td]
                out[k, 2 + t] = s / h
                if t == 0:
                    out[k, 1] = s / (h - 1)
    return out


# ------------------------------------------------------------------------------------------------------------ k_summary
def col_mean_ref(cols):
    """Column means of cols (S x np) in long double with the bound of k_summary's order: mean_roundings(S) roundings on a term, so
    |m^ - m| <= gamma_(ceil(S/256)+8) mean|x|, plus 2^-1074 for a quotient in the denormal range (sums of denormals are exact).
    A column that holds an Inf or a NaN has no bound: its mean is Inf / NaN exactly where numpy's float64 mean is.
    Returns (ref long double, bound float64, special float64, finite bool): `finite` marks the columns without Inf / NaN, on which ref and
    bound hold; `special` is numpy's mean on the others."""
    S = cols.shape[0]
    finite = np.isfinite(cols).all(axis=0)
    safe = np.where(finite[None, :], cols, 0.0)
    mu = safe.astype(LD).sum(axis=0) / S
    am = np.abs(safe).sum(axis=0) / S
    bound = up(gamma_m(mean_roundings(S)) * am + (S + 2) * EPS_LD * am + TINY)
    with np.errstate(all="ignore"):
        special = np.where(finite, 0.0, cols.mean(axis=0))
    return mu, bound, special, finite


def check_col_mean(dev, cols):
    """largest error / bound of the device's column means over the all-finite columns; asserts the Inf / NaN ones are what numpy's are"""
    mu, bound, special, finite = col_mean_ref(cols)
    dev = np.asarray(dev, dtype=np.float64)
    for p in np.flatnonzero(~finite):
        assert (np.isnan(dev[p]) and np.isnan(special[p])) or dev[p] == special[p], (p, dev[p], special[p])
    err = np.abs(np.where(finite, dev, 0.0).astype(LD) - mu).astype(np.float64)
    return ratio(err[finite], bound[finite])


def order_stat_ref(cols, k):
    """The k-th smallest (1-based) of every column of cols (S x np) under the reference's order (Julia's isless, which sort uses): numbers by
    value, every NaN after every number whatever its sign or payload.  NaN where the rank falls among the NaNs."""
    S, npar = cols.shape
    assert 1 <= k <= S
    out = np.full(npar, np.nan)
    for p in range(npar):
        x = cols[:, p]
        nums = np.sort(x[~np.isnan(x)])
        if k <= nums.size:
            out[p] = nums[k - 1]
    return out


def order_stat_match(dev, ref):
    """per column: equal as numbers (so -0 == +0: the reference's sort leaves their order open) where the reference is a number, a NaN where it is one"""
    dev, ref = np.asarray(dev), np.asarray(ref)
    return np.where(np.isnan(ref), np.isnan(dev), dev == ref)


def emu_order_stat(cols, k, nan_by_bits=False):
    """k_summary's selection restated: the k-th smallest of the order-preserving 64-bit keys, mapped back.  A NaN maps to the top key; the
    mutation nan_by_bits orders NaNs by their bit image like everything else, so that sign-bit NaNs come first."""
    c = np.ascontiguousarray(cols.T)                                   # (np, S)
    bits = c.view(np.uint64)
    top = np.uint64(1) << np.uint64(63)
    key = np.where(bits & top != 0, ~bits, bits | top)
    if not nan_by_bits:
        key = np.where(np.isnan(c), ~np.uint64(0), key)
    kk = np.sort(key, axis=1)[:, k - 1]
    back = np.where(kk & top != 0, kk & ~top, ~kk)
    return np.ascontiguousarray(back).view(np.float64)


# ------------------------------------------------------------------------------------------------------------ crafted columns and tables
NAN_POS = np.array([0x7FF8000000000000], dtype=np.uint64).view(np.float64)[0]          # np.nan
NAN_NEG = np.array([0xFFF8000000000000], dtype=np.uint64).view(np.float64)[0]          # -np.nan, and what x86 makes of inf - inf and 0 / 0
NAN_PAY_POS = np.array([0x7FF0000000000001], dtype=np.uint64).view(np.float64)[0]      # the smallest payload: one bit above +Inf
NAN_PAY_NEG = np.array([0xFFF8000000000ABC], dtype=np.uint64).view(np.float64)[0]

FAMILIES = ("normal", "ar1", "big_mean", "tiny", "alt", "ramp", "const0", "const1", "const025")
WELL_SCALED = ("normal", "ar1", "ramp")            # mean and spread of one order of magnitude: the families ess_from_stats is compared on
CONSTANT = ("const0", "const1", "const025")


def family_column(name, tot, rng):
    """one column of `tot` rows of the family `name`"""
    i = np.arange(tot, dtype=np.float64)
    if name == "normal":
        return rng.standard_normal(tot)
    if name == "ar1":
        e = rng.standard_normal(tot)
        x = np.empty(tot)
        x[0] = e[0] / np.sqrt(1 - 0.95 ** 2)
        for j in range(1, tot):
            x[j] = 0.95 * x[j - 1] + e[j]
        return x
    if name == "big_mean":
        return 1e8 + rng.standard_normal(tot)
    if name == "tiny":
        return 1e-8 + 1e-12 * rng.standard_normal(tot)
    if name == "alt":
        return np.where(i % 2 == 0, 1e150, -1e150)
    if name == "ramp":
        return -2.0 + (3.0 + rng.random()) * i / tot
    if name in CONSTANT:
        return np.full(tot, {"const0": 0.0, "const1": 1.0, "const025": 0.25}[name])
    raise KeyError(name)


def family_of(j):
    return FAMILIES[j % len(FAMILIES)]


def xi_column(v, tot, chain, rng):
    """0/1 patterns for the xi columns: 0 constant 1 in every chain; 1 constant 0 in chain 0 and constant 1 in every other; then an alternation, a
    period of 3, a step in the middle, and Bernoulli draws of rising probability"""
    i = np.arange(tot)
    if v == 0:
        return np.ones(tot)
    if v == 1:
        return np.full(tot, 0.0 if chain == 0 else 1.0)
    if v == 2:
        return (i % 2).astype(np.float64)
    if v == 3:
        return (i % 3 == 0).astype(np.float64)
    if v == 4:
        return (i >= tot // 2).astype(np.float64)
    return (rng.random(tot) < 0.05 + 0.9 * (v - 5) / 10.0).astype(np.float64)


def new_table(tot, V, R):
    """a zero table in the reference's layout (bnr_amd.new_table without the dead columns; restated so that this module needs numpy only)"""
    q = V * (V + 1) // 2
    sh = dict(tau2=(1, 1), u=(R, V), xi=(V, 1), gamma=(q, 1), S=(q, 1), theta=(1, 1), Delta=(1, 1), M=(R, R), mu=(1, 1), lam=(R, 1), pi=(R, 3))
    return {k: np.zeros((tot,) + s, dtype=np.float64, order="F") for k, s in sh.items()}


def crafted_table(tot, V, R, chain, seed=20260):
    """gamma column j holds family j % 9 (a fresh draw per column and chain), the xi columns the 0/1 patterns; everything else stays 0"""
    t = new_table(tot, V, R)
    q = V * (V + 1) // 2
    for j in range(q):
        t["gamma"][:, j, 0] = family_column(family_of(j), tot, np.random.default_rng([seed, chain, j]))
    for v in range(V):
        t["xi"][:, v, 0] = xi_column(v, tot, chain, np.random.default_rng([seed, chain, 1000 + v]))
    return t


SPECIALS = ("all_equal", "ties", "denormal", "inf_both", "inf_pos", "inf_neg", "nan_pos", "nan_neg", "nan_pay_pos", "nan_pay_neg", "nan_three",
            "nan_all_neg")
NAN_THREE_ROWS = (40, 300, 630)                   # 0-based rows of the three NaNs: all inside rows 38 .. 638


def special_column(name, tot, chain, rng):
    """the columns only k_summary is fed (the split statistics have no meaning on them)"""
    x = rng.standard_normal(tot)
    if name == "all_equal":
        return np.full(tot, -1.5)
    if name == "ties":
        return np.clip(x, -1.2, 1.2)                                   # about 11 % of the rows tie at either end: the blocks straddle ranks 1, 2, the 95 % ranks, S - 1, S
    if name == "denormal":
        k = rng.integers(-1000, 1001, size=tot).astype(np.float64)    # +-k 2^-1074, some +-0 among them
        d = k * TINY
        d[::37] = -0.0
        return d
    if name.startswith("inf"):
        sel = rng.permutation(tot)
        if name != "inf_neg":
            x[sel[:tot // 60 + 1]] = np.inf
        if name != "inf_pos":
            x[sel[-(tot // 60 + 1):]] = -np.inf
        return x
    if name == "nan_three":
        if chain == 0:
            x[[r % tot for r in NAN_THREE_ROWS]] = (NAN_NEG, NAN_POS, NAN_PAY_NEG)
        return x
    if name == "nan_all_neg":
        return np.full(tot, NAN_NEG)
    kind = dict(nan_pos=NAN_POS, nan_neg=NAN_NEG, nan_pay_pos=NAN_PAY_POS, nan_pay_neg=NAN_PAY_NEG)[name]
    x[rng.random(tot) < 0.08] = kind
    x[(7 * (chain + 1)) % tot] = kind                                  # at least one, whatever the draw
    return x


def summary_table(tot, V, R, chain, seed=20260):
    """crafted_table with the first len(SPECIALS) gamma columns past the first round of families replaced by the special columns"""
    t = crafted_table(tot, V, R, chain, seed)
    for s, name in enumerate(SPECIALS):
        t["gamma"][:, special_index(name), 0] = special_column(name, tot, chain, np.random.default_rng([seed, chain, 2000 + s]))
    return t


def special_index(name):
    return len(FAMILIES) + SPECIALS.index(name)


def window(t, first_row, nsamp):
    """the parameter columns [gamma(q) | xi(V)] of rows first_row .. first_row + nsamp - 1 (1-based) of a table: nsamp x (q + V)"""
    r = slice(first_row - 1, first_row - 1 + nsamp)
    return np.concatenate([t["gamma"][r, :, 0], t["xi"][r, :, 0]], axis=1)


def summary_ranks(S):
    """the rank pairs the tests ask of a window of S draws: both ends in either order, one in from the ends, the 95 % ranks the reference reads
    (round half to even of 0.025 S and 0.975 S), and S - 3 with S - 2 (a number and a NaN on the column with three NaNs); only pairs inside 1 .. S"""
    pairs = [(1, S), (S, 1), (2, S - 1), (int(round(S * 0.025)), int(round(S * 0.975))), (S - 3, S - 2)]
    out = []
    for a, b in pairs:
        if 1 <= a <= S and 1 <= b <= S and (a, b) not in out:
            out.append((a, b))
    return out


# ------------------------------------------------------------------------------------------------------------ the cases both test modules run
N, V, R, TOT = 8, 16, 2, 640                       # q = 136, q + V = 152 parameter columns: two 128-thread blocks of k_rhat_stats, ragged 32-column tiles
Q = V * (V + 1) // 2
RHAT_WINDOWS = ((1, 4), (1, 5), (3, 101), (38, 601), (1, 640))                                   # (first_row, nsamp)
ESS_CASES = ((1, 8, 2), (1, 9, 4), (38, 601, 300), (1, 640, 320), (1, 640, 257))                 # (first_row, nsamp, max_lag)
SUMMARY_WINDOWS = ((7, 1), (3, 33), (100, 257), (38, 601))                                       # (first_row, nsamp)
