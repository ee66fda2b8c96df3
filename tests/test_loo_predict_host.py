"""CPU tests of the LOO predictive checks (ABI 11, an addition to the reference): the weights restatement against _psis_row / _psis_host, the
tail under ties, the closed forms of the mixture predictive (moments, PIT, bounds), both quantile solvers, the totals, the argument checks that
run before any GPU call, the ABI version and the exports, the Julia shim's new names, the place of the new kernels in the code object, and a
statistical sanity check of "leaving one row out" on the golden fixture with the CPU oracle's trace."""
import math
import os
import re

import numpy as np
import pytest

import bnr_amd
import code_objects as co
from bnr_amd import _capi, api
from bnr_amd.api import (_host_eta, _host_loo_predict, _loo_bracket_c, _loo_predict_rows, _loo_predictive, _mixture_cdf, _mixture_quantile, _psis_host,
                         _psis_row, _psis_weights_host, _psis_weights_row, _tail_length)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Z975 = 1.959963984540054          # the 0.975 quantile of N(0, 1)


def loglik_rows(seed, S=600):
    rng = np.random.default_rng(seed)
    rows = [-0.5 * (rng.standard_normal(S) * sc) ** 2 - 1.0 for sc in (0.3, 1.0, 3.0, 10.0)]
    for k in (0.3, 0.8, 1.3):
        u = rng.random(S)
        rows.append(-np.log(((1 - u) ** (-k) - 1) / k))
    rows.append(np.round(rng.standard_normal(S), 1))                   # many ties, at the cutoff too
    return np.array(rows)


def test_weights_agree_with_psis_row():
    for seed, r_eff in ((1, None), (2, 0.4), (3, np.linspace(0.3, 2.0, 8))):
        ll = loglik_rows(seed)
        lw, e, k = _psis_weights_host(ll, r_eff)
        lpd, he, hk = _psis_host(ll, r_eff)
        assert np.allclose(np.exp(lw).sum(axis=1), 1.0, rtol=0, atol=1e-13)
        assert np.all(lw <= 0)
        from_w = np.array([api._logsumexp(lw[i] + ll[i]) for i in range(ll.shape[0])])
        assert np.all(np.abs(from_w - he) <= 1e-12 * np.abs(he)) and np.all(np.abs(e - he) <= 1e-12 * np.abs(he))
        assert np.array_equal(k, hk)                                   # the same fit on the same tail in the same order: to the bit
        assert np.all(np.isfinite(k[:7]))
    # _psis_host itself did not move: its rows are _psis_row's, bit for bit
    ll = loglik_rows(4)
    out = _psis_host(ll)
    for i in range(ll.shape[0]):
        assert (out[0][i], out[1][i], out[2][i]) == _psis_row(ll[i], _tail_length(ll.shape[1], 1.0))


def test_no_smoothing_gives_the_truncated_raw_ratios():
    rng = np.random.default_rng(5)
    # M = ceil(0.2 S) < 5 (S <= 20): no fit; the weights are the raw ratios exp(-l), normalised
    for S in (1, 7, 20):
        ll = rng.standard_normal(S)
        assert _tail_length(S, 1.0) < 5
        _lpd, e, k, lw = _psis_weights_row(ll, _tail_length(S, 1.0))
        raw = np.exp(-ll - np.max(-ll))
        assert math.isinf(k) and np.allclose(np.exp(lw), raw / raw.sum(), rtol=1e-14, atol=0)
    # a constant tail (the M largest ratios tied): no fit either
    S = 100
    ll = np.concatenate([np.full(40, -3.0), rng.standard_normal(60) + 2.0])
    M = _tail_length(S, 1.0)
    assert M == 20
    _lpd, e, k, lw = _psis_weights_row(ll, M)
    raw = np.exp(-ll - np.max(-ll))
    assert math.isinf(k) and np.allclose(np.exp(lw), raw / raw.sum(), rtol=1e-14, atol=0)
    # a constant row: every weight the same number, 1 / S up to the rounding of exp(-log S), and elpd = lpd = l
    for S in (8, 100, 1000):
        _lpd, e, k, lw = _psis_weights_row(np.full(S, -2.0), _tail_length(S, 1.0))
        w = np.exp(lw)
        assert np.all(w == w[0]) and abs(w[0] * S - 1.0) <= 4 * np.finfo(float).eps and math.isinf(k)
        assert abs(e + 2.0) < 1e-14 and abs(_lpd + 2.0) < 1e-14


def test_ties_at_the_cutoff_take_the_largest_draw_indices():
    """S = 100, M = 20: 17 distinct large ratios and 30 draws tied at the cutoff value -- the tail is the 17 and, of the tied ones, the 3 with
    the largest draw index (fewer than the M / 4 entries below the fit's x*, which has to be positive); position j of (lw, s) gets the j-th quantile, so the smoothed weights of the tied tail draws increase with s"""
    rng = np.random.default_rng(6)
    S, M = 100, 20
    ll = rng.standard_normal(S) + 3.0
    big = rng.choice(S, 17, replace=False)
    ll[big] = -5.0 - np.arange(17) * 0.1                               # the 17 smallest l: the 17 largest ratios
    rest = np.setdiff1d(np.arange(S), big)
    tied = np.sort(rng.choice(rest, 30, replace=False))
    ll[tied] = -1.0                                                    # next: 30 tied
    assert np.all(ll[np.setdiff1d(rest, tied)] > -1.0)
    _lpd, e, k, lw = _psis_weights_row(ll, M)
    raw = -ll - np.max(-ll)
    raw_n = raw - api._logsumexp(raw)
    changed = np.flatnonzero(np.abs((lw - lw[tied[0]]) - (raw_n - raw_n[tied[0]])) > 1e-12)   # draws whose weight moved against a tied non-tail draw
    want = np.sort(np.concatenate([big, tied[-3:]]))
    top = int(np.argmax(raw))                                          # (the largest ratio's smoothed weight is truncated at 0: its raw value)
    assert math.isfinite(k) and np.array_equal(np.union1d(changed, [top]), want), (changed, want)
    assert np.all(np.diff(lw[tied[-3:]]) > 0) and np.all(lw[tied[:-3]] == lw[tied[0]])
    # ... and this is the M largest in (lw, s)
    order = sorted(range(S), key=lambda s: (raw[s], s))
    assert np.array_equal(np.sort(order[S - M:]), want)


def test_nan_row_gives_nan_outputs():
    rng = np.random.default_rng(7)
    ll = rng.standard_normal((3, 200))
    ll[1, 17] = np.nan
    lw, e, k = _psis_weights_host(ll)
    assert np.all(np.isnan(lw[1])) and np.isnan(e[1]) and np.isinf(k[1])
    assert np.all(np.isfinite(lw[[0, 2]])) and np.all(np.isfinite(e[[0, 2]]))
    eta = rng.standard_normal((3, 200))
    tau2 = rng.random(200) + 0.5
    mean, sd, pit, lo, hi, _w = _loo_predict_rows(eta, tau2, np.zeros(3), lw, 0.025, 0.975)
    for a in (mean, sd, pit, lo, hi):
        assert np.isnan(a[1]) and np.all(np.isfinite(a[[0, 2]]))
    lp = _loo_predictive(np.zeros(3), np.zeros(3), e, k, mean, sd, pit, lo, hi, 95, 200)
    assert math.isfinite(lp.rmse_loo) and math.isfinite(lp.coverage)          # totals over the finite rows


@pytest.mark.parametrize("solver", ["brentq", "bisect"])
def test_closed_forms_of_the_predictive(solver):
    if solver == "brentq":
        pytest.importorskip("scipy.optimize")
    S = 50
    eta0, t0 = 1.25, 2.5
    eta = np.full((2, S), eta0)
    tau2 = np.full(S, t0)
    lwn = np.full((2, S), -math.log(S))
    y = np.array([0.3, 4.0])
    mean, sd, pit, lo, hi, width = _loo_predict_rows(eta, tau2, y, lwn, 0.025, 0.975, solver)
    s0 = math.sqrt(t0)
    assert np.allclose(mean, eta0, rtol=1e-14) and np.allclose(sd, s0, rtol=1e-12)
    assert np.allclose(pit, [0.5 * math.erfc(-(v - eta0) / s0 / math.sqrt(2)) for v in y], rtol=1e-13)
    tol = width[0] * 2.0 ** -40                                        # the solver's tolerance: 2^-40 of the bracket
    assert width[0] == pytest.approx(2 * _loo_bracket_c(0.025, 0.975) * s0)
    assert np.all(np.abs(lo - (eta0 - Z975 * s0)) <= tol + 1e-13) and np.all(np.abs(hi - (eta0 + Z975 * s0)) <= tol + 1e-13)
    # a two-component mixture: F at the returned bound is p, within the slope of F times the solver's tolerance
    rng = np.random.default_rng(8)
    eta2 = np.array([np.where(np.arange(S) % 2 == 0, -2.0, 3.0)])
    tau22 = np.where(np.arange(S) % 2 == 0, 0.5, 1.5)
    w = rng.random(S) + 0.1
    lw2 = np.log(w / w.sum())[None, :]
    _m, _s, _p, lo2, hi2, width2 = _loo_predict_rows(eta2, tau22, np.zeros(1), lw2, 0.05, 0.9, solver)
    resid = 0.3990 * width2[0] * 2.0 ** -40 / math.sqrt(0.5) + 1e-15
    wn, sd2 = np.exp(lw2[0]), np.sqrt(tau22)
    assert abs(_mixture_cdf(lo2[0], wn, eta2[0], sd2) - 0.05) <= resid and abs(_mixture_cdf(hi2[0], wn, eta2[0], sd2) - 0.9) <= resid
    assert lo2[0] < hi2[0]
    # the mixture moments against their closed form
    m_want = float(np.sum(wn * eta2[0]))
    assert _m[0] == pytest.approx(m_want, rel=1e-13) and _s[0] == pytest.approx(math.sqrt(float(np.sum(wn * (tau22 + eta2[0] ** 2))) - m_want ** 2), rel=1e-12)


def test_both_solvers_agree():
    pytest.importorskip("scipy.optimize")
    rng = np.random.default_rng(9)
    S = 300
    eta, sd = rng.standard_normal(S) * 2, np.sqrt(rng.random(S) + 0.2)
    w = rng.random(S) ** 4
    w /= w.sum()
    c = _loo_bracket_c(0.1, 0.9)
    for p in (0.1, 0.5, 0.9):
        a, width = _mixture_quantile(p, w, eta, sd, c, "brentq")
        b, _ = _mixture_quantile(p, w, eta, sd, c, "bisect")
        assert abs(a - b) <= width * 2.0 ** -40
    for p_lo, p_hi in ((0.025, 0.975), (1e-6, 0.5), (0.4, 0.999999), (0.25, 0.75)):
        c = _loo_bracket_c(p_lo, p_hi)
        assert 0.5 * math.erfc(c / math.sqrt(2)) < min(p_lo, 1 - p_hi) / 2 and (c == 1.0 or 0.5 * math.erfc((c - 0.5) / math.sqrt(2)) >= min(p_lo, 1 - p_hi) / 2)


def test_totals_against_numpy():
    rng = np.random.default_rng(10)
    n = 40
    y = rng.standard_normal(n) * 3
    mean = y + rng.standard_normal(n)
    sd = rng.random(n) + 1
    pit = rng.random(n)
    lo, hi = mean - 1.0, mean + 1.0
    k = rng.random(n)
    mean[3] = np.nan                                                   # a refused row: left out of every total
    lp = _loo_predictive(y, np.zeros(n), np.zeros(n), k, mean, sd, pit, lo, hi, 90, 1000)
    ok = np.arange(n) != 3
    r = (y - mean)[ok]
    assert lp.rmse_loo == pytest.approx(math.sqrt(np.mean(r ** 2)), rel=1e-14)
    assert lp.r2_loo == pytest.approx(1 - np.var(r) / np.var(y[ok]), rel=1e-14)
    assert lp.coverage == pytest.approx(np.mean(np.abs(r) <= 1.0), rel=1e-14)
    u = np.sort(pit[ok])
    m = u.size
    ks = max(max((i + 1) / m - u[i], u[i] - i / m) for i in range(m))
    assert lp.ks == pytest.approx(ks, rel=1e-14)
    assert lp.interval == 90 and lp.draws == 1000 and lp.khat_threshold == pytest.approx(min(1 - 1 / 3.0, 0.7)) and lp.n_high_k == int(np.sum(k > lp.khat_threshold))
    assert api._ks_uniform(np.array([0.5])) == 0.5 and api._ks_uniform((np.arange(100) + 0.5) / 100) == pytest.approx(0.005)


def test_abi_version_and_exports():
    hdr = open(os.path.join(ROOT, "include", "bnr_hip.h")).read()
    ver = int(re.search(r"#define BNR_ABI_VERSION (\d+)", hdr).group(1))
    L = bnr_amd.lib()
    assert ver >= 11 and L.bnr_abi_version() == ver
    for name in ("bnr_chain_loo_predict", "bnr_chains_loo_predict", "bnr_psis_weights"):
        assert name in _capi.EXPORTS and getattr(L, name) is not None and name in hdr
    for name in ("LOOPredict", "LOOPredictive", "psis_weights", "device_loo_predict"):
        assert hasattr(bnr_amd, name)
    assert hasattr(_capi.Chain, "loo_predict") and hasattr(_capi, "pooled_loo_predict") and hasattr(_capi, "psis_weights_raw")


def test_refusals_before_any_gpu_call():
    ll = np.zeros((2, 50))
    for p_lo, p_hi in ((0.5, 0.5), (0.6, 0.4), (0.0, 0.9), (0.1, 1.0), (-0.1, 0.5), (float("nan"), 0.5)):
        with pytest.raises(ValueError):
            _capi.loo_probs(p_lo, p_hi)
        with pytest.raises(ValueError):
            _capi.pooled_loo_predict([], 1, 10, None, p_lo, p_hi)
    for interval in (0, 100, 150, -5):
        with pytest.raises(ValueError):
            api._loo_interval_probs(interval)
    assert api._loo_interval_probs(95) == pytest.approx((0.025, 0.975))
    with pytest.raises(ValueError):
        _capi.pooled_loo_predict([], 1, 10)                            # no chain
    with pytest.raises(ValueError):
        _capi.psis_weights_raw(np.zeros(5))
    with pytest.raises(ValueError):
        _capi.psis_weights_raw(ll, [1.0, -1.0])
    with pytest.raises(ValueError):
        _psis_weights_host(np.zeros(5))
    # the library's own checks that precede the first HIP call: NULL arguments, shapes, r_eff, a tail past the limit
    L = bnr_amd.lib()
    out = np.empty((2, 50))
    assert L.bnr_psis_weights(0, 2, 50, None, None, _capi._ptr(out), None, None) == _capi.BNR_ERR_BAD_ARG
    assert L.bnr_psis_weights(0, 2, 50, _capi._ptr(ll), None, None, None, None) == _capi.BNR_ERR_BAD_ARG
    assert L.bnr_psis_weights(0, 0, 50, _capi._ptr(ll), None, _capi._ptr(out), None, None) == _capi.BNR_ERR_BAD_ARG
    assert L.bnr_psis_weights(0, 2, 50, _capi._ptr(ll), _capi._ptr(np.array([1.0, np.inf])), _capi._ptr(out), None, None) == _capi.BNR_ERR_BAD_ARG
    S = 50000
    big = np.zeros((1, S))
    r_bad = np.array([S * 9.0 / 8193.0 ** 2 * 0.999])                  # M = 8193 (or 8194) > BNR_PSIS_MAX_TAIL
    assert _tail_length(S, r_bad[0]) > 8192
    assert L.bnr_psis_weights(0, 1, S, _capi._ptr(big), _capi._ptr(r_bad), _capi._ptr(np.empty((1, S))), None, None) == _capi.BNR_ERR_BAD_ARG
    assert b"8192" in L.bnr_last_error()
    assert L.bnr_chain_loo_predict(None, 1, 10, None, 0.025, 0.975, *([None] * 8)) == _capi.BNR_ERR_BAD_ARG
    assert L.bnr_chains_loo_predict(None, 1, 1, 10, None, 0.025, 0.975, *([None] * 8)) == _capi.BNR_ERR_BAD_ARG
    # Fit refuses a bad interval before it samples (refused before any chain is created)
    X, y, _ = bnr_amd.make_synthetic(20, 5, 2, seed=3)
    with pytest.raises(ValueError):
        bnr_amd.Fit(X, y, 2, nburn=10, nsamples=10, x_transform=False, filename=None, loo_predict=True, predict_interval=100)
    with pytest.raises(ValueError):
        bnr_amd.LOOPredict(api.Results(None, None, None, 0, 10))


def test_julia_shim_has_the_new_names():
    src = open(os.path.join(ROOT, "julia", "BNRHip.jl")).read()
    for name in ("bnr_chain_loo_predict", "bnr_chains_loo_predict", "bnr_psis_weights", "loo_predict"):
        assert name in src, name
    assert re.search(r"ccall\(\(:bnr_chains_loo_predict", src) and re.search(r"ccall\(\(:bnr_psis_weights", src)


def test_loo_predict_kernels_sit_outside_the_code_object_of_the_sweep(tmp_path):
    """the kernels of ABI 11 are compiled in csrc/bnr_analysis.hip: all five are in the analysis code object and none in the sweep's"""
    assert os.path.exists(co.LIB), "libbnr_hip.so has not been built"         # (a failed build is a failure here, not a skip)
    if not co.have_tools():
        pytest.skip("no ROCm LLVM tools here")
    names = ("k_psis_w", "k_loo_moments", "k_loo_quantile", "k_inv_sd")
    sweep, analysis = co.sweep_and_analysis(tmp_path)
    new = [k for k in analysis if k.startswith(names)]
    assert len(new) == 5 and set(new) <= co.ANALYSIS, sorted(analysis)
    assert not [k for k in sweep if k.startswith(names)]


def test_leaving_one_row_out_on_the_golden_fixture():
    """tests/golden/test1_xy.npz (n = 70, V = 19) with the CPU oracle's trace, a 400-row table, window 101 .. 400.  Leaving a row out can only
    widen its predictive and, for most rows, moves the mean away from the row's own response: the mean loo_sd is not below the mean in-sample
    predictive sd, and |y - loo_mean| >= |y - in-sample mean| for at least 75 % of the rows (observed with the host restatement alone on this
    fixture: 66 of 70 = 94.3 %; mean loo_sd 3.67 against 2.49 in sample).  The threshold leaves room for the rows whose PSIS estimate is
    itself noisy -- with q = 190 > n most rows have a k-hat above the threshold here, which is the point of reporting n_high_k."""
    from oracle import bnr_oracle as bo
    d = np.load(os.path.join(ROOT, "tests", "golden", "test1_xy.npz"))
    X, y = d["X"], d["y"]
    o = bo.Oracle(X, y, 5, 400, 20240501, chain=1, pdf_mode=1)
    o.init_prior()
    o.run(2, 400, 400)
    nb, ns = 100, 300
    lp = _host_loo_predict([o.t], X, y, nb, ns, 95, False)
    eta = _host_eta(o.t, X, nb, ns)
    tau2 = o.t["tau2"][nb:nb + ns, 0, 0]
    ins_mean = eta.mean(axis=1)
    ins_sd = np.sqrt(np.mean(tau2[None, :] + eta ** 2, axis=1) - ins_mean ** 2)
    share = float(np.mean(np.abs(y - lp.loo_mean) >= np.abs(y - ins_mean)))
    print("mean loo_sd %.4f, in-sample %.4f; share of rows with |y - loo_mean| >= |y - mean|: %.4f; n_high_k %d of %d"
          % (lp.loo_sd.mean(), ins_sd.mean(), share, lp.n_high_k, y.size))
    assert np.all(np.isfinite(lp.loo_mean)) and np.all(np.isfinite(lp.loo_sd)) and np.all(lp.loo_lower < lp.loo_upper)
    assert lp.loo_sd.mean() >= ins_sd.mean()
    assert share >= 0.75
    assert np.all((lp.loo_pit >= 0) & (lp.loo_pit <= 1)) and 0 <= lp.coverage <= 1 and lp.draws == ns
    # the fallback of LOOPredict over a fetched table is this restatement; a fit's own object is returned as it is
    res = api.Results(o.t, None, None, nb, ns)
    again = bnr_amd.LOOPredict(res, X, y, x_transform=False)
    assert np.array_equal(again.loo_mean, lp.loo_mean) and np.array_equal(again.loo_upper, lp.loo_upper) and again.ks == lp.ks
    res.loo_predictive = lp
    assert bnr_amd.LOOPredict(res) is lp and bnr_amd.LOOPredict(res, interval=95) is lp
