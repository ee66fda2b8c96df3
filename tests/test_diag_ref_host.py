"""CPU tests of tests/diag_ref.py: the long-double references of the diagnostic kernels agree with an exact fractions.Fraction evaluation to 1 %
of their bounds on small cases; the float64 emulation of each kernel's summation order stays inside the bounds on every crafted family and every
window the GPU test uses (so a correct kernel passes before GPU time is spent); and each planted mutation of an emulation breaks a bound or an
exact comparison on at least one family (so the inputs are strong enough to see it)."""
from fractions import Fraction

import numpy as np
import pytest

import diag_ref as dr


def frac(x):
    return Fraction(*np.longdouble(x).as_integer_ratio())


@pytest.fixture(scope="module")
def table():
    return dr.crafted_table(dr.TOT, dr.V, dr.R, chain=0)


@pytest.fixture(scope="module")
def stable():
    return [dr.summary_table(dr.TOT, dr.V, dr.R, chain=c) for c in (0, 1)]


def _gamma_cols(name):
    return [j for j in range(dr.Q) if dr.family_of(j) == name]


# ------------------------------------------------------------------------------------------------------------------ exactness of the references
def _small():
    """11 rows of V = 4 (10 gamma columns: every family once, the first twice; 4 xi patterns)"""
    return dr.crafted_table(11, 4, 1, chain=0)


def _exact_half(x):
    h = len(x)
    xs = [Fraction(float(v)) for v in x]
    mu = sum(xs) / h
    c = [v - mu for v in xs]
    return mu, c


@pytest.mark.parametrize("first,nsamp", [(1, 4), (2, 9), (1, 10), (1, 11)])
def test_split_stats_reference_is_exact(first, nsamp):
    par = dr.window(_small(), first, nsamp)
    ref, bnd = dr.split_stats_ref(par)
    h = nsamp // 2
    for p in range(par.shape[1]):
        for k, x in enumerate((par[:h, p], par[nsamp - h:, p])):
            mu, c = _exact_half(x)
            var = sum(v * v for v in c) / (h - 1)
            assert abs(frac(ref[2 * k, p]) - mu) <= Fraction(bnd[2 * k, p]) / 100, (p, k)
            assert abs(frac(ref[2 * k + 1, p]) - var) <= Fraction(bnd[2 * k + 1, p]) / 100, (p, k)
    # and the bounds are of float64 size: a relative 1e-3 error of a non-constant column's variance is far outside
    live = ref[1].astype(np.float64) > 0
    assert live.sum() >= 6 and np.all(bnd[1][live] <= 1e-6 * ref[1].astype(np.float64)[live])


@pytest.mark.parametrize("first,nsamp,L", [(1, 8, 2), (2, 9, 4), (1, 11, 5)])
def test_acov_reference_is_exact(first, nsamp, L):
    par = dr.window(_small(), first, nsamp)
    ref, bnd = dr.acov_ref(par, L)
    h = nsamp // 2
    for p in range(par.shape[1]):
        for k, x in enumerate((par[:h, p], par[nsamp - h:, p])):
            mu, c = _exact_half(x)
            assert abs(frac(ref[k, 0, p]) - mu) <= Fraction(bnd[k, 0, p]) / 100, (p, k)
            for t in range(L):
                a = sum(c[i] * c[i + t] for i in range(h - t))
                assert abs(frac(ref[k, 2 + t, p]) - a / h) <= Fraction(bnd[k, 2 + t, p]) / 100, (p, k, t)
                if t == 0:
                    assert abs(frac(ref[k, 1, p]) - a / (h - 1)) <= Fraction(bnd[k, 1, p]) / 100, (p, k)


def test_column_mean_and_order_statistic_references_are_exact():
    t = dr.summary_table(40, 8, 1, chain=0)
    cols = dr.window(t, 3, 33)
    mu, bnd, special, finite = dr.col_mean_ref(cols)
    for p in np.flatnonzero(finite):
        exact = sum(Fraction(float(v)) for v in cols[:, p]) / cols.shape[0]
        assert abs(frac(mu[p]) - exact) <= Fraction(bnd[p]) / 100, p
    assert sorted(np.flatnonzero(~finite)) == sorted(dr.special_index(n) for n in dr.SPECIALS if n.startswith(("inf", "nan")))
    for p in np.flatnonzero(~finite):                                  # any NaN, or Inf of both signs: NaN; else the Inf that is there
        x = cols[:, p]
        if np.isnan(x).any() or ((x == np.inf).any() and (x == -np.inf).any()):
            assert np.isnan(special[p]), p
        else:
            assert special[p] == (np.inf if (x == np.inf).any() else -np.inf), p
    # the order: a plain Python sort with the reference's key (numbers by value, any NaN last)
    for k in (1, 2, 17, 32, 33):
        ref = dr.order_stat_ref(cols, k)
        for p in range(cols.shape[1]):
            want = sorted(cols[:, p].tolist(), key=lambda v: (v != v, 0.0 if v != v else v))[k - 1]
            assert (want != want and np.isnan(ref[p])) or ref[p] == want, (k, p)


def test_nan_kinds_are_what_they_claim():
    bits = lambda v: int(np.array([v]).view(np.uint64)[0])
    assert bits(dr.NAN_POS) >> 63 == 0 and bits(dr.NAN_PAY_POS) >> 63 == 0 and bits(dr.NAN_NEG) >> 63 == 1 and bits(dr.NAN_PAY_NEG) >> 63 == 1
    assert all(np.isnan(v) for v in (dr.NAN_POS, dr.NAN_NEG, dr.NAN_PAY_POS, dr.NAN_PAY_NEG))
    t = dr.summary_table(dr.TOT, dr.V, dr.R, chain=0)                 # the tables keep the bit images
    col = t["gamma"][:, dr.special_index("nan_three"), 0]
    assert [bits(col[r]) for r in dr.NAN_THREE_ROWS] == [bits(dr.NAN_NEG), bits(dr.NAN_POS), bits(dr.NAN_PAY_NEG)] and np.isnan(col).sum() == 3
    w = dr.window(t, 38, 601)[:, dr.special_index("nan_three")]
    assert np.isnan(w).sum() == 3
    assert not np.isnan(dr.order_stat_ref(w[:, None], 601 - 3)[0]) and np.isnan(dr.order_stat_ref(w[:, None], 601 - 2)[0])


# ------------------------------------------------------------------------------------------------------------------ emulations inside the bounds
def test_split_stats_emulation_stays_inside_the_bound(table):
    worst = 0.0
    for first, nsamp in dr.RHAT_WINDOWS:
        par = dr.window(table, first, nsamp)
        ref, bnd = dr.split_stats_ref(par)
        emu = dr.emu_split_stats(par)
        r = dr.ratio(np.abs(emu.astype(dr.LD) - ref).astype(np.float64), bnd)
        worst = max(worst, r)
        assert r <= 1, (first, nsamp, r)
        for name in dr.CONSTANT:
            assert np.all(emu[1::2][:, _gamma_cols(name)] == 0), name
    print("split statistics, emulation: worst error / bound %.3g" % worst)


def test_acov_emulation_stays_inside_the_bound(table):
    worst = 0.0
    for first, nsamp, L in dr.ESS_CASES:
        par = dr.window(table, first, nsamp)
        ref, bnd = dr.acov_ref(par, L)
        emu = dr.emu_acov(par, L)
        r = dr.ratio(np.abs(emu.astype(dr.LD) - ref).astype(np.float64), bnd)
        worst = max(worst, r)
        assert r <= 1, (first, nsamp, L, r)
    print("autocovariance message, emulation: worst error / bound %.3g" % worst)


def test_summary_emulation_stays_inside_the_bound(stable):
    worst = 0.0
    for first, nsamp in dr.SUMMARY_WINDOWS:
        one = dr.window(stable[0], first, nsamp)
        for cols in (one, np.concatenate([one, dr.window(stable[1], first, nsamp)], axis=0)):
            with np.errstate(all="ignore"):
                worst = max(worst, dr.check_col_mean(dr.emu_mean(cols), cols))
            for k_lo, k_hi in dr.summary_ranks(cols.shape[0]):
                for k in (k_lo, k_hi):
                    assert np.all(dr.order_stat_match(dr.emu_order_stat(cols, k), dr.order_stat_ref(cols, k))), (first, nsamp, k)
    assert worst <= 1, worst
    print("column mean, emulation: worst error / bound %.3g" % worst)


# ------------------------------------------------------------------------------------------------------------------ mutations break them
def _families_hit(err, bnd, cols_axis_len):
    """names of the gamma families with an entry outside its bound (err, bnd: (..., np))"""
    bad = (err > bnd).reshape(-1, cols_axis_len).any(axis=0)
    return sorted({dr.family_of(j) for j in np.flatnonzero(bad[:dr.Q])}), bool(bad[dr.Q:].any())


def test_split_stats_mutations_violate_the_bound(table):
    # the variance divided by h
    first, nsamp = 38, 601
    par = dr.window(table, first, nsamp)
    ref, bnd = dr.split_stats_ref(par)
    err = np.abs(dr.emu_split_stats(par, ddof=0).astype(dr.LD) - ref).astype(np.float64)
    fam, xi = _families_hit(err, bnd, par.shape[1])
    assert set(fam) == set(dr.FAMILIES) - set(dr.CONSTANT) and xi, fam             # every non-constant family sees it (a constant one has no variance)
    assert np.all(err[0::2] <= bnd[0::2])                                         # ... in the variances only
    # the second half from row h, odd windows
    for first, nsamp in [w for w in dr.RHAT_WINDOWS if w[1] % 2]:
        par = dr.window(table, first, nsamp)
        ref, bnd = dr.split_stats_ref(par)
        err = np.abs(dr.emu_split_stats(par, second_start=nsamp // 2).astype(dr.LD) - ref).astype(np.float64)
        fam, xi = _families_hit(err, bnd, par.shape[1])
        assert {"normal", "ar1", "big_mean", "tiny", "ramp"} <= set(fam) and xi, (nsamp, fam)    # (the +-1e150 alternation looks the same one row on)
        assert np.all(err[:2] <= bnd[:2])                                         # the first half is untouched
    # and the same slip is invisible on an even window: that is why the odd ones are in the list
    par = dr.window(table, 1, 640)
    assert np.array_equal(dr.emu_split_stats(par, second_start=320), dr.emu_split_stats(par))


def test_acov_mutations_violate_the_bound(table):
    first, nsamp, L = 1, 640, 257
    par = dr.window(table, first, nsamp)
    ref, bnd = dr.acov_ref(par, L)
    # the last product of every lag's sum dropped
    err = np.abs(dr.emu_acov(par, L, drop_last=True).astype(dr.LD) - ref).astype(np.float64)
    fam, xi = _families_hit(err, bnd, par.shape[1])
    assert set(fam) == set(dr.FAMILIES) - set(dr.CONSTANT) and xi, fam
    # lag 256 computed from the data of lag 0: only a case with max_lag > 256 can see it
    err = np.abs(dr.emu_acov(par, L, alias_256=True).astype(dr.LD) - ref).astype(np.float64)
    assert np.all(err[:, :2 + 256] <= bnd[:, :2 + 256])
    fam, xi = _families_hit(err[:, 2 + 256:], bnd[:, 2 + 256:], par.shape[1])
    assert set(fam) == set(dr.FAMILIES) - set(dr.CONSTANT) and xi, fam
    assert sum(1 for c in dr.ESS_CASES if c[2] > dr.NT) >= 2
    # the largest lag the entry point admits with an odd window: one product, the last row of each half
    par = dr.window(table, 1, 9)
    ref, bnd = dr.acov_ref(par, 4)
    err = np.abs(dr.emu_acov(par, 4, drop_last=True).astype(dr.LD) - ref).astype(np.float64)
    assert np.any(err[:, 2 + 3] > bnd[:, 2 + 3])


def test_order_statistic_mutations_are_seen(stable):
    first, nsamp = 38, 601
    cols = dr.window(stable[0], first, nsamp)
    S = nsamp
    for k, dk in ((2, -1), (2, 1), (S - 1, 1), (S - 1, -1), (15, 1), (586, -1)):
        ok = dr.order_stat_match(dr.emu_order_stat(cols, k + dk), dr.order_stat_ref(cols, k))
        fam = {dr.family_of(j) for j in np.flatnonzero(~ok[:dr.Q]) if j < len(dr.FAMILIES)}
        assert {"normal", "ar1", "big_mean", "tiny", "ramp"} <= fam, (k, dk, fam)
        assert ok[dr.special_index("all_equal")] and ok[dr.special_index("ties")]   # inside a block of ties the neighbour is the same number
    # with the three NaNs: one rank too high at S - 3 reads a NaN, one too low at S - 2 a number
    p = dr.special_index("nan_three")
    assert not dr.order_stat_match(dr.emu_order_stat(cols, S - 2), dr.order_stat_ref(cols, S - 3))[p]
    assert not dr.order_stat_match(dr.emu_order_stat(cols, S - 3), dr.order_stat_ref(cols, S - 2))[p]
    # NaNs ordered by their bit image: the sign-bit ones come first
    for k_lo, k_hi in dr.summary_ranks(S):
        bad_lo = ~dr.order_stat_match(dr.emu_order_stat(cols, k_lo, nan_by_bits=True), dr.order_stat_ref(cols, k_lo))
        bad_hi = ~dr.order_stat_match(dr.emu_order_stat(cols, k_hi, nan_by_bits=True), dr.order_stat_ref(cols, k_hi))
        hit = {n for n in dr.SPECIALS if bad_lo[dr.special_index(n)] or bad_hi[dr.special_index(n)]}
        assert hit <= {"nan_neg", "nan_pay_neg", "nan_three"}, hit                 # nothing but the sign-bit NaNs differs ...
        assert {"nan_neg", "nan_pay_neg"} <= hit, (k_lo, k_hi, hit)               # ... and those do at every rank pair asked
        assert not bad_lo[:len(dr.FAMILIES)].any() and not bad_hi[:len(dr.FAMILIES)].any()
    bad = ~dr.order_stat_match(dr.emu_order_stat(cols, 1, nan_by_bits=True), dr.order_stat_ref(cols, 1))
    assert bad[dr.special_index("nan_three")]                                       # rank 1 of the column with three NaNs is a NaN under that order
