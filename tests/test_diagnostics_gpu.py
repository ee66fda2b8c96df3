"""GPU tests of the convergence-diagnostic kernels against the long-double references and a-priori bounds of tests/diag_ref.py (run with -m gpu
on an MI355X): k_rhat_stats, k_acov, k_summary and the transposes k_load_cols / k_fetch_cols that feed them.

No sampling: crafted tables (diag_ref.crafted_table / summary_table) are loaded with Chain.load into chains of n = 8, V = 16, R = 2 (q = 136,
q + V = 152 parameter columns: two 128-thread blocks of k_rhat_stats, a ragged last 32-column tile of gamma and of xi) with 640-row tables.
Every tolerance is derived in diag_ref.py; the largest error / bound ratio of each kernel is printed (pytest -s).
A window of 1 row admits only the rank pair (1, 1) and a pooled one of 2 rows no (S - 3, S - 2): diag_ref.summary_ranks keeps the pairs inside
1 .. S, and the refusal of every other rank is tested on its own."""
import numpy as np
import pytest

import bnr_amd
import diag_ref as dr
from bnr_amd import _capi
from oracle import bnr_oracle as bo

pytestmark = pytest.mark.gpu
WORST = {}


def _note(what, r):
    WORST[what] = max(WORST.get(what, 0.0), r)
    assert r <= 1.0, (what, r)


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    print("\ndiagnostic kernels, largest error/bound:", {k: "%.3g" % v for k, v in sorted(WORST.items())})


@pytest.fixture(scope="module")
def chains(gpu):
    """three chains of one fit (never run: every test loads the table it needs)"""
    X, y, _ = bnr_amd.make_synthetic(dr.N, dr.V, dr.R, seed=3)
    cs = [bnr_amd.Chain(X, y, dr.R, dr.TOT, 99, 1, device=gpu)]
    cs += [bnr_amd.Chain.like(cs[0], 99, c) for c in (2, 3)]
    yield cs
    for c in cs:
        c.close()


@pytest.fixture(scope="module")
def tables():
    return [dr.crafted_table(dr.TOT, dr.V, dr.R, chain=c) for c in range(3)]


@pytest.fixture(scope="module")
def stables():
    return [dr.summary_table(dr.TOT, dr.V, dr.R, chain=c) for c in range(2)]


def _gamma_cols(names):
    return [j for j in range(dr.Q) if dr.family_of(j) in names]


def _err(dev, ref):
    return np.abs(np.asarray(dev, dtype=dr.LD) - ref).astype(np.float64)


# ------------------------------------------------------------------------------------------------------------------ k_rhat_stats / bnr_rhat
def test_rhat_stats_within_the_bound(chains, tables):
    ch, t = chains[0], tables[0]
    ch.load(t)
    const = _gamma_cols(dr.CONSTANT)
    for first, nsamp in dr.RHAT_WINDOWS:
        msg = ch.rhat_stats(first, nsamp).reshape(4, dr.Q + dr.V)
        ref, bnd = dr.split_stats_ref(dr.window(t, first, nsamp))
        r = dr.ratio(_err(msg, ref), bnd)
        print("rhat_stats first_row %d nsamp %d: error / bound %.3g" % (first, nsamp, r))
        _note("rhat_stats", r)
        assert np.all(msg[1::2][:, const] == 0.0), (first, nsamp)                      # constant columns: variance exactly 0 ...
        assert np.array_equal(msg[0::2][:, const], ref[0::2][:, const].astype(np.float64))     # ... around the exact mean
        assert np.all(msg[1::2][:, dr.Q] == 0.0) and np.all(msg[0::2][:, dr.Q] == 1.0)         # the xi column of ones


def test_rhat_over_three_crafted_chains_equals_the_oracle(chains, tables):
    for ch, t in zip(chains, tables):
        ch.load(t)
    for burn, nsamp in ((37, 601), (0, 640)):
        rg, rx = _capi.rhat(chains, 3, None, burn, nsamp)
        gam = np.stack([t["gamma"][burn:burn + nsamp, :, 0] for t in tables], axis=2)
        xi = np.stack([t["xi"][burn:burn + nsamp, :, 0] for t in tables], axis=2)
        want_g, want_x = bo.rhat(gam), bo.rhat(xi)
        assert np.allclose(rg, want_g, rtol=1e-10) and np.allclose(rx, want_x, rtol=1e-10), (burn, nsamp)
        assert not np.isnan(rg).any() and not np.isnan(rx).any()
        assert rx[0] == 1.0 and rx[1] == np.inf, (rx[0], rx[1])                       # constant 1 everywhere; 0 in one chain and 1 in the others
        assert np.all(rg[_gamma_cols(dr.CONSTANT)] == 1.0)
        assert np.all(np.isfinite(rg))
        if nsamp == 640:
            assert rx[4] == np.inf                                                     # the step in the middle: every half constant, the halves apart


# ------------------------------------------------------------------------------------------------------------------ k_acov
def test_ess_stats_within_the_bound(chains, tables):
    ch, t = chains[0], tables[0]
    ch.load(t)
    npar = dr.Q + dr.V
    well = _gamma_cols(dr.WELL_SCALED) + [dr.Q + v for v in range(2, dr.V)]
    const = _gamma_cols(dr.CONSTANT) + [dr.Q, dr.Q + 1]
    for first, nsamp, L in dr.ESS_CASES:
        msg = ch.ess_stats(first, nsamp, L)
        ref, bnd = dr.acov_ref(dr.window(t, first, nsamp), L)
        dev = msg.reshape(2, 2 + L, npar)
        r = dr.ratio(_err(dev, ref), bnd)
        print("ess_stats first_row %d nsamp %d max_lag %d: error / bound %.3g" % (first, nsamp, L, r))
        _note("ess_stats", r)
        ess_dev = _capi.ess_from_stats(msg[None, :], nsamp, L)
        ess_ref = _capi.ess_from_stats(ref.astype(np.float64).reshape(1, -1), nsamp, L)
        assert np.all(np.isnan(ess_dev[const])), (first, nsamp, L)
        live = [p for p in well if not np.isnan(ess_ref[p])]                          # (a 0/1 column can be constant over every half)
        assert set(_gamma_cols(dr.WELL_SCALED)) <= set(live)
        assert np.array_equal(np.isnan(ess_dev[well]), np.isnan(ess_ref[well]))
        assert np.allclose(ess_dev[live], ess_ref[live], rtol=1e-9, atol=0), (first, nsamp, L)


# ------------------------------------------------------------------------------------------------------------------ k_summary
def _check_summary(got, cols, k_lo, k_hi, what):
    mean, lo, hi, pxi = got
    g, x = cols[:, :dr.Q], cols[:, dr.Q:]
    for name, dev, k in (("lower", lo, k_lo), ("upper", hi, k_hi)):
        ref = dr.order_stat_ref(g, k)
        ok = dr.order_stat_match(dev, ref)
        assert np.all(ok), (what, name, k, [(int(j), dev[j], ref[j]) for j in np.flatnonzero(~ok)])
    _note("summary mean", dr.check_col_mean(mean, g))
    assert np.array_equal(pxi, x.sum(axis=0) / x.shape[0]), what                       # sums of 0/1 are exact, so is the one division


@pytest.mark.parametrize("first,nsamp", dr.SUMMARY_WINDOWS)
def test_summary_one_chain_and_pooled(chains, stables, first, nsamp):
    for ch, t in zip(chains, stables):
        ch.load(t)
    one = dr.window(stables[0], first, nsamp)
    both = np.concatenate([one, dr.window(stables[1], first, nsamp)], axis=0)
    for k_lo, k_hi in dr.summary_ranks(nsamp):
        _check_summary(chains[0].summary(first, nsamp, k_lo, k_hi), one, k_lo, k_hi, ("one", first, nsamp))
    for k_lo, k_hi in dr.summary_ranks(2 * nsamp):
        _check_summary(_capi.pooled_summary(chains[:2], first, nsamp, k_lo, k_hi), both, k_lo, k_hi, ("pooled", first, nsamp))
    if nsamp == 601:
        # the column with three NaNs (a sign-bit one among them): rank S - 3 is a number, rank S - 2 is not, and rank 1 is the minimum
        p = dr.special_index("nan_three")
        _m, lo, hi, _x = chains[0].summary(first, nsamp, nsamp - 3, nsamp - 2)
        assert lo[p] == np.nanmax(one[:, p]) and np.isnan(hi[p])
        _m, lo, hi, _x = chains[0].summary(first, nsamp, 1, nsamp)
        assert lo[p] == np.nanmin(one[:, p]) and np.isnan(hi[p])
        # and what Summary() prints is the same from either source, which is what the key order has to guarantee
        k_lo, k_hi = bnr_amd.api._summary_ranks(nsamp, 95)
        gs = np.sort(one[:, :dr.Q], axis=0)
        _m, lo, hi, _x = chains[0].summary(first, nsamp, k_lo, k_hi)
        assert np.array_equal(lo, gs[k_lo - 1], equal_nan=True) and np.array_equal(hi, gs[k_hi - 1], equal_nan=True)


# ------------------------------------------------------------------------------------------------------------------ k_load_cols / k_fetch_cols
def _coded_table(sign):
    """every element of every column holds (column, element, row) as an integer below 2^53, with `sign`"""
    t = bnr_amd.new_table(dr.TOT, dr.V, dr.R, dead=False)
    rows = np.arange(1, dr.TOT + 1, dtype=np.float64)
    for c, k in enumerate(_capi.TABLE_COLUMNS):
        a = t[k]
        ne = a.shape[1] * a.shape[2]
        el = np.arange(ne, dtype=np.float64).reshape(a.shape[2], a.shape[1]).T           # element index in memory order (d1 fastest)
        a[:] = sign * ((c + 1) * 2.0 ** 32 + el[None, :, :] * 4096.0 + rows[:, None, None])
    return t


def _bits_equal(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


def test_transposes_round_trip_bitwise(chains):
    ch = chains[2]
    back, new = _coded_table(-1.0), _coded_table(1.0)
    assert len({v for k in _capi.TABLE_COLUMNS for v in new[k].ravel().tolist()}) == sum(new[k].size for k in _capi.TABLE_COLUMNS)   # all distinct
    for first, last in ((1, 640), (2, 34), (33, 64), (600, 640)):
        ch.load(back)
        ch.load(new, first, last)
        full = ch.fetch()
        part = ch.fetch(first, last)
        for k in _capi.TABLE_COLUMNS:
            assert _bits_equal(full[k][first - 1:last], new[k][first - 1:last]), (k, first, last)
            assert _bits_equal(full[k][:first - 1], back[k][:first - 1]) and _bits_equal(full[k][last:], back[k][last:]), (k, first, last)
            assert part[k].shape[0] == last - first + 1 and _bits_equal(part[k], new[k][first - 1:last]), (k, first, last)
    # NaN payloads, signed zeros, denormals and Inf travel unchanged too
    odd = np.array([dr.NAN_POS, dr.NAN_NEG, dr.NAN_PAY_POS, dr.NAN_PAY_NEG, -0.0, 0.0, dr.TINY, -dr.TINY, np.inf, -np.inf, 1.7976931348623157e308])
    t = _coded_table(1.0)
    t["gamma"][:, :, 0] = odd[(np.arange(dr.TOT)[:, None] + np.arange(dr.Q)[None, :]) % odd.size]
    ch.load(t)
    assert _bits_equal(ch.fetch(5, 637)["gamma"], t["gamma"][4:637])


# ------------------------------------------------------------------------------------------------------------------ refusals
def test_refusals_stay_errors(chains, tables):
    ch = chains[0]
    ch.load(tables[0])
    with pytest.raises(bnr_amd.BnrError):
        ch.rhat_stats(1, 3)
    for first, nsamp, L in ((1, 7, 2), (1, 640, 1), (1, 640, 321), (1, 9, 5), (1, 601, 301)):
        with pytest.raises(bnr_amd.BnrError):
            ch.ess_stats(first, nsamp, L)
    for k_lo, k_hi in ((0, 5), (5, 0), (1, 34), (34, 1), (-1, 2)):
        with pytest.raises(bnr_amd.BnrError):
            ch.summary(3, 33, k_lo, k_hi)
    with pytest.raises(bnr_amd.BnrError):
        _capi.pooled_summary(chains[:2], 3, 33, 1, 67)
    assert ch.summary(3, 33, 1, 33)[1].shape == (dr.Q,) and _capi.pooled_summary(chains[:2], 3, 33, 1, 66)[1].shape == (dr.Q,)
