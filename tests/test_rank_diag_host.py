"""CPU tests of the rank-normalised convergence diagnostics (ABI 12): Phi^-1 (bnr_host_ndtri, AS 241) against scipy, the numpy restatement
api._host_rank_diagnostics against the independent transcription of `posterior` in tests/rank_diag_ref.py, the indicator identity behind
ess_tail, monotone invariance, and the ABI.  No GPU.

Phi^-1: the largest relative difference between bnr_host_ndtri and scipy.special.ndtri over the grid below was measured here as 1.03e-15
(at S = 160 000, in the branch r <= 5; both claim about 1e-16, scipy's is Cephes); the test allows 4 x that, the project's habit for such gaps.

Restatement against transcription: xi_1 is degenerate (constant inside every split chain, not overall) in every window, xi_4 in the window
(1, 640) whose halves fall on the two sides of its step; there only rhat >= 1e6 or +Inf is asserted.  In the other windows xi_4 is an ordinary
column (a step inside one half) or a constant, and is compared like the rest."""
import ctypes as C
import re

import numpy as np
import pytest
from scipy.special import ndtri

import bnr_amd
import diag_ref as dr
import rank_diag_cases as rc
import rank_diag_ref as rr
from bnr_amd import _capi, api

NDTRI_GAP = 1.03e-15                                   # measured (see the module docstring)


def test_ndtri_against_scipy():
    worst = 0.0
    for S in (2, 16, 1280, 160000):
        r = np.arange(1.0, S + 0.25, 0.5)
        p = (r - 0.375) / (S + 0.25)
        a, b = _capi.host_ndtri(p), ndtri(p)
        assert np.array_equal(a == 0.0, b == 0.0)
        nz = b != 0.0
        worst = max(worst, float(np.max(np.abs(a[nz] - b[nz]) / np.abs(b[nz]))))
    for p in (1e-300, 1e-17, 1.0 - 2.0 ** -53):
        a, b = float(_capi.host_ndtri(p)), float(ndtri(p))
        worst = max(worst, abs(a - b) / abs(b))
    print("bnr_host_ndtri against scipy.special.ndtri: largest relative difference %.3g" % worst)
    assert worst <= 4 * NDTRI_GAP, worst


def test_ndtri_centre_antisymmetry_and_ends():
    f = _capi.host_ndtri
    assert float(f(0.5)) == 0.0
    rng = np.random.default_rng(5)
    p = np.concatenate([rng.random(2000) * 0.5, 2.0 ** -np.arange(1, 60), [1e-300, 0.075, 0.0749999, 0.425 + 0.5, 3.7e-12]])
    p = p[(p > 0) & (p < 1)]
    exact = (1.0 - (1.0 - p)) == p                     # 1 - p is exact
    assert exact.sum() > 1000
    assert np.array_equal(f(p[exact]), -f(1.0 - p[exact]))
    assert float(f(0.0)) == -np.inf and float(f(1.0)) == np.inf and np.isnan(float(f(np.nan)))


@pytest.mark.parametrize("first,nsamp,lag", rc.WINDOWS)
def test_restatement_against_the_transcription(first, nsamp, lag):
    wins = rc.windows_of(rc.tables(), first, nsamp)
    want = rr.diagnostics_all(wins, lag)
    got = rc.host(3, first, nsamp, lag)
    gaps = rc.compare(got, want, wins, (first, nsamp, lag))
    print("restatement against transcription, window", (first, nsamp, lag), {k: "%.2g" % v for k, v in gaps.items()})
    deg = rc.degenerate(wins)
    assert deg[rc.XI1] and (deg[rc.XI4] == (nsamp == 640))
    const = [j for j in range(dr.Q) if dr.family_of(j) in dr.CONSTANT] + [dr.Q]          # the constant families and xi_0: NaN throughout
    for f in rc.FIELDS:
        assert np.isnan(got[f][const]).all(), f
    alt = [j for j in range(dr.Q) if dr.family_of(j) == "alt"] + [dr.Q + 2]              # alt and xi_2 fold to a constant
    assert np.isnan(got["rhat_tail"][alt]).all() and np.isnan(got["ess_tail"][alt]).all()
    assert not np.isnan(got["rhat"][alt]).any()                                            # fmax: the bulk R-hat survives
    if nsamp >= 101:
        assert np.isnan(got["ess_tail"][dr.Q + 5:]).sum() > (dr.V - 5) // 2              # most Bernoulli xi columns


def test_one_table_and_the_results_path():
    t = rc.tables()[0]
    d = api._host_rank_diagnostics([t], 37, 601)
    assert (d.chains, d.draws, d.max_lag) == (1, 600, 150) and d.rhat_gamma.shape == (dr.Q,) and d.ess_tail_xi.shape == (dr.V,)
    want = rr.diagnostics_all([dr.window(t, 38, 601)], 150)
    rc.compare(rc.as_dict(d), want, [dr.window(t, 38, 601)], "one table")
    res = bnr_amd.Results(t, None, None, 37, 601)
    assert res.rank_diag is None
    assert np.array_equal(bnr_amd.RankDiagnose(res).full("ess_bulk"), d.full("ess_bulk"), equal_nan=True)
    with pytest.raises(ValueError):
        bnr_amd.RankDiagnose(bnr_amd.Results(None, None, None, 37, 601))
    for bad in ((0, 7, None), (0, 640, 1), (0, 640, 321)):
        with pytest.raises(ValueError):
            api._host_rank_diagnostics([t], *bad)


def test_indicator_identity():
    """I(x <= x_(k)), k = floor((S' - 1) prob) + 1, is `posterior`'s I(x <= quantile(x, prob, type 7)) on every non-constant column"""
    for first, nsamp, _lag in rc.WINDOWS:
        X = rr.split_draws(rc.windows_of(rc.tables(), first, nsamp))
        flat = X.reshape(-1, X.shape[2])
        n = flat.shape[0]
        for p in range(flat.shape[1]):
            x = flat[:, p]
            if np.all(x == x[0]):
                continue
            xs = np.sort(x)
            for prob in (0.05, 0.95):
                k = int(np.floor((n - 1) * prob)) + 1
                assert np.array_equal(x <= xs[k - 1], x <= np.quantile(x, prob)), (first, nsamp, p, prob)


def test_monotone_invariance_is_bitwise():
    tabs = [dict(t) for t in rc.tables()]
    for t in tabs:
        t["gamma"] = t["gamma"].copy()
        t["gamma"][:, 9, 0] = t["gamma"][:, 0, 0] ** 3                # column 9 (a second "normal") becomes the cube of column 0
    d = api._host_rank_diagnostics(tabs, 37, 601, 150)
    for f in ("rhat_bulk", "ess_bulk", "ess_tail"):
        v = getattr(d, f + "_gamma")
        assert v[0] == v[9] and not np.isnan(v[0]), f
    assert d.ess_mean_gamma[0] != d.ess_mean_gamma[9]


def test_abi_12_and_its_exports():
    src = open(bnr_amd.LIB.replace("bayesiannetworkregression.jl_amd/libbnr_hip.so", "include/bnr_hip.h")).read()
    ver = int(re.search(r"#define BNR_ABI_VERSION (\d+)", src).group(1))
    L = bnr_amd.lib()
    assert ver >= 12 and L.bnr_abi_version() == ver
    raw = C.CDLL(bnr_amd.LIB)
    for name in ("bnr_chain_rank_diag", "bnr_chains_rank_diag", "bnr_rank_normalize", "bnr_host_ndtri"):
        assert hasattr(raw, name) and name in bnr_amd.EXPORTS, name


def test_fit_refuses_rank_diagnostics_it_cannot_compute_before_sampling():
    X, y, _ = bnr_amd.make_synthetic(8, 4, 2, seed=1)
    with pytest.raises(ValueError):                    # 6 samples: nsamp < 8, refused before any chain is created
        bnr_amd.generate_samples(X, y, 2, nburn=4, nsamp=6, x_transform=False, rank_diagnostics=True, suppress_timer=True)
