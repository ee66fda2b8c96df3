"""CPU tests of tests/pred_ref.py, the reference of the prediction, WAIC and PSIS-LOO kernels.

The new operations (erfc, log1p, expm1) and the long-double generalized Pareto fit are held against mpmath at 40 digits, which fixes
ERFC_REF_ULPS.  Then the float64 host restatements of api.py (_host_eta, _host_pointwise, _host_pit, _psis_host, _psis_weights_host,
_loo_predict_rows: another summation order, glibc's libm) stand in for the device at every input of tests/test_pred_exact_gpu.py (the rows of 2^21 + 513 draws included): they
lie inside every bound (the worst error / bound per stage is printed, pytest -s), the LOO moments also inside the sharper bound of their own
sums over the weights given (check_loo_sums), the reference's selection is the stable argsort's, the
skip cap and the non-vacuity rule hold, and two planted errors of the reference (a tail length off by one, the prior adjustment of k
dropped) make the same arithmetic fail.  The restatements do not calibrate a bound."""
import warnings

import mpmath
import numpy as np
import pytest

import bnr_amd
import pred_ref as pr
import sweep_ref as sr
from bnr_amd import _capi, api
from pred_ref import VE, LD, U

mpmath.mp.dps = 40
WORST = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    print("\nhost restatements, largest error/bound:", {k: "%.3g" % v for k, v in sorted(WORST.items())})


def _note(stage, r, what):
    print("ratio %-26s %.3e  %s" % (stage, r, what))
    WORST[stage] = max(WORST.get(stage, 0.0), r)
    assert r < 1.0, (stage, r, what)


def _mpf(x):
    x = LD(x)
    hi = float(x)
    return mpmath.mpf(hi) + mpmath.mpf(float(x - LD(hi)))


def _ulps(got, want):
    """|got - want| in units of u |want| (got a long double, want an mpf)"""
    return float(abs(_mpf(got) - want) / (mpmath.mpf(U) * abs(want))) if want != 0 else float(abs(_mpf(got)))


# ------------------------------------------------------------------------------------------------------------------ against 40 digits
def test_erfc_log1p_expm1_against_mpmath():
    rng = np.random.default_rng(3)
    grid = np.r_[np.linspace(-9.5, 26.5, 1441), rng.uniform(-1, 6.5, 600), [1e-300, -1e-300, 1e-8, 0.5 - 1e-9, 0.4769362762044699, 5.656854249492381, 1.5]]
    ald = np.asarray(grid, dtype=LD) * (1 + LD(2) ** -55)                            # long doubles between two doubles
    got, got64 = pr.erfc_ld(ald), pr._erfc64(grid)
    worst, worst64 = 0.0, 0.0
    for a, g, g64 in zip(ald, got, got64):
        worst = max(worst, _ulps(g, mpmath.erfc(_mpf(a))))
        worst64 = max(worst64, _ulps(g64, mpmath.erfc(mpmath.mpf(float(a)))) if abs(float(a)) <= 5.7 else 0.0)
    print("erfc_ld: %.4f ulp; scipy's erfc up to |z| = 8: %.2f ulp" % (worst, worst64))
    assert worst <= pr.ERFC_REF_ULPS
    assert np.all(np.abs(got64 - sr.f64(got)) <= (64 + 2 * grid * grid) * U * got64 + pr.DENORM * 2.0 ** 52)  # the cross-check; scipy rounds a^2
    assert float(pr.erfc_ld(LD(-12))) == 2.0 and 0 < float(pr.erfc_ld(LD(26.0))) < 1e-290
    for a in np.r_[-0.999, -0.5, -1e-5, -1e-300, 0.0, 1e-300, 1e-9, 0.3, 1.0, 50.0, 1e10]:
        x = VE(LD(float(a)) * (1 + LD(2) ** -60))
        assert _ulps(pr.vlog1p(x).v, mpmath.log1p(_mpf(x.v))) <= 1 / 256 if a != 0 else pr.vlog1p(x).v == 0
    for a in np.r_[-700.0, -40.0, -1.0, -1e-5, -1e-300, 1e-300, 1e-9, 0.3, 1.0, 50.0, 700.0]:
        x = VE(LD(float(a)) * (1 + LD(2) ** -60))
        assert _ulps(pr.vexpm1(x).v, mpmath.expm1(_mpf(x.v))) <= 1 / 256
    # the derivatives of the error model
    a = VE(LD(0.25), 1e-12)
    assert pr.vlog1p(a).e == pytest.approx(1e-12 / 1.25 + sr.LIBM_ULPS * U * np.log1p(0.25), rel=1e-12)
    assert pr.vexpm1(a).e == pytest.approx(1e-12 * np.exp(0.25) + sr.LIBM_ULPS * U * np.expm1(0.25), rel=1e-12)
    assert pr.verfc(a).e == pytest.approx(1e-12 * 2 / np.sqrt(np.pi) * np.exp(-0.0625) + (pr.ERFC_REF_ULPS + pr.ERFC_ULPS) * U * float(pr._erfc64(0.25)), rel=1e-12)


def _mp_gpdfit(x):
    """gpdfit.R at 40 digits: (k after the prior adjustment, sigma)"""
    N = len(x)
    mg = 30 + int(mpmath.floor(mpmath.sqrt(N)))
    xs = x[int(mpmath.floor(N / mpmath.mpf(4) + mpmath.mpf(1) / 2)) - 1]
    th = [1 / x[-1] + (1 - mpmath.sqrt(mpmath.mpf(mg) / (j - mpmath.mpf(1) / 2))) / 3 / xs for j in range(1, mg + 1)]
    kk = [sum(mpmath.log1p(-t * v) for v in x) / N for t in th]
    lt = [N * (mpmath.log(-t / k) - k - 1) for t, k in zip(th, kk)]
    mx = max(lt)
    w = [mpmath.exp(v - mx) for v in lt]
    that = sum(t * v for t, v in zip(th, w)) / sum(w)
    k = sum(mpmath.log1p(-that * v) for v in x) / N
    return k * N / (N + 10) + mpmath.mpf(5) / (N + 10), -k / that


@pytest.mark.parametrize("M", [5, 64, 1200])
def test_long_double_gpdfit_against_mpmath(M):
    rng = np.random.default_rng(M)
    x = np.sort(((1 - rng.random(M)) ** -0.45 - 1) / 0.45)
    kh, sigma, _k0 = pr.gpdfit(VE(np.asarray(x, dtype=LD)))
    wk, ws = _mp_gpdfit([mpmath.mpf(float(v)) for v in x])
    # the reference's own rounding is 1/2048 of the device's bound: within 1/100 of it
    assert abs(_mpf(kh.v) - wk) <= mpmath.mpf(float(kh.e)) / 100, (float(kh.v), float(wk), kh.e)
    assert abs(_mpf(sigma.v) - ws) <= mpmath.mpf(float(sigma.e)) / 100
    assert pr.nonvacuous(kh) and pr.nonvacuous(sigma)
    hk, hs = api._gpdfit(x)
    _note("gpdfit khat", pr.err_ratio(hk, kh), "M=%d" % M)
    _note("gpdfit sigma", pr.err_ratio(hs, sigma), "M=%d" % M)


# ------------------------------------------------------------------------------------------------------------------ k_predict
def test_host_eta_is_exact_on_the_exact_tables():
    tabs = {V: [pr.table(V, pr.PREDICT_TOT, V + c, pr.CHAIN_OFFSET * c) for c in range(3 if V == 5 else 1)] for V in pr.PREDICT_V}
    for V, m, nsamp, first, _blk, nc in pr.PREDICT_CASES:
        X = pr.predict_X(V, m)
        g, mu, _t = pr.window(tabs[V][:nc], first, nsamp)
        E = pr.exact_eta(X, g, mu)
        host = np.concatenate([api._host_eta(t, X, first - 1, nsamp) for t in tabs[V][:nc]], axis=1)
        assert np.array_equal(host, E), (V, m, nsamp)
        assert np.all(np.abs(pr.exact_mean(E) - E.mean(axis=1)) <= 4 * U * np.abs(E).max(axis=1))
        # index-coded: another draw, another column offset or a shifted row of X is another eta
        if nsamp > 1:
            assert not np.array_equal(E[:, 0], E[:, 1])


def test_host_eta_within_the_bound_on_real_values():
    t, X = pr.real_case()
    g, mu, _ = pr.window([t], 1, 300)
    ref = pr.eta(X, g, mu)
    assert np.all(pr.nonvacuous(ref))
    _note("eta", pr.err_ratio(api._host_eta(t, X, 0, 300), ref), "V=12 normal")


# ------------------------------------------------------------------------------------------------------------------ k_pred_loglik, k_pred_pit
def test_host_pointwise_and_pit_within_the_bounds():
    for name, t, X, y, Ss, ill in pr.loglik_inputs():
        for S in Ss:
            g, mu, tau2 = pr.window([t], 2, S)
            E = pr.exact_eta(X, g, mu)
            L = pr.ell(y, VE(np.asarray(E, dtype=LD)), tau2)
            rl, rp = pr.lpd_pwaic(L)
            rt = pr.pit(y, VE(np.asarray(E, dtype=LD)), tau2)
            with np.errstate(invalid="ignore", divide="ignore"), warnings.catch_warnings():
                warnings.simplefilter("ignore")                                      # (one draw: numpy warns of the ddof-1 variance)
                lpd, pw = api._host_pointwise(t, X, y, 1, S)
            skipped = pr.check_pointwise(name, rl, rp, rt, lpd, pw, api._host_pit(E, tau2, y), S, ill, _note)
            assert skipped <= pr.SKIP_FRACTION * len(y), (name, S, skipped)
            if name == "all l equal":
                assert np.ptp(sr.f64(L.v)) == 0.0
            if name.startswith("tau2"):
                assert S < 255 or np.max(np.ptp(sr.f64(L.v), axis=1)) > 745                      # an exp of the log-mean-exp underflows
            if ill:
                assert 1e-7 < np.ptp(sr.f64(L.v)) < 1e-5 and abs(sr.f64(L.v)[0, 0]) > 1e3


# ------------------------------------------------------------------------------------------------------------------ PSIS on crafted rows
def _host_psis(ll, Ms, weights):
    out = [api._psis_weights_row(ll[i].copy(), M) if weights else api._psis_row(ll[i].copy(), M) + (None,) for i, M in enumerate(Ms)]
    lpd, elpd, khat = (np.array([o[j] for o in out]) for j in range(3))
    return lpd, elpd, khat, (np.array([o[3] for o in out]) if weights else None)


@pytest.mark.parametrize("weights", [False, True])
def test_host_psis_within_the_bounds(weights):
    for name, ll, Ms in pr.psis_cases(big=True):
        with np.errstate(all="ignore"):
            skipped = pr.run_psis_case(name, ll, Ms, _host_psis(ll, Ms, weights), weights, _note)
        assert skipped <= pr.SKIP_FRACTION * len(Ms), (name, skipped)
        for M in Ms:                                                                # every tail length can be asked for through r_eff
            assert M == pr.tail_length(ll.shape[1]) or pr.r_eff_for(ll.shape[1], M) > 0


def test_selection_is_the_stable_argsort():
    for name, ll, Ms in pr.psis_cases(big=True):
        S = ll.shape[1]
        for i, M in enumerate(Ms):
            if M < 5:
                continue
            lw = (-ll[i]) - np.max(-ll[i])
            assert np.array_equal(pr.psis_ref(name, i, ll[i], M)["tail"], np.argsort(lw, kind="stable")[S - M:]), (name, i)
    # the big row: the tied draws that join the reference's tail are those of the largest index, s_c on the boundaries of the index digits
    name, ll, Ms = pr.psis_cases(big=True)[-1]
    for i, (t, sc) in enumerate(((3, 2 ** 21), (6, 2 ** 11), (10, 2 ** 10 - 1))):
        assert Ms[i] == pr.BIG_ABOVE + t
        tail = pr.psis_ref(name, i, ll[i], Ms[i])["tail"]
        tied = np.sort(tail[ll[i][tail] == ll[i][pr.BIG_TIED[0]]])
        assert tied.size == t and tied[0] == sc and np.array_equal(tied, pr.BIG_TIED[-t:])


def test_crafted_rows_hit_the_digits_they_are_built_for():
    key = lambda v: np.where(v < 0, ~v.view(np.uint64), v.view(np.uint64) | np.uint64(1 << 63))
    name, ll, Ms = pr.psis_cases(big=False)[2]
    M, S = Ms[0], ll.shape[1]
    for i in (0, 1):                                                                # keys around the cutoff agree above the lowest 9 bits
        lw = (-ll[i]) - np.max(-ll[i])
        k = np.sort(key(lw))
        near = k[S - M - 8:S - M + 6]
        assert np.unique(near >> np.uint64(9)).size <= 2 and np.unique(near).size == near.size
    lw = (-ll[2]) - np.max(-ll[2])                                                  # every decade of the top digit's range
    top = np.unique(key(lw[lw < 0]) >> np.uint64(53))
    assert top.size > 200
    for i, want_join in ((4, None), (5, 0), (6, 5), (7, 2)):                        # all / none / some / rounded
        lw = (-ll[i]) - np.max(-ll[i])
        srt = np.sort(lw)
        kc = srt[S - M - 1]
        join = int(np.sum(srt[S - M:] == kc))
        assert (join == want_join) if want_join is not None else (join == 0 and np.sum(srt[S - M:] == srt[S - M]) == 12), (i, join)
    lw = (-ll[3]) - np.max(-ll[3])                                                  # more ties than M
    assert np.sum(lw == 0) > M


# ------------------------------------------------------------------------------------------------------------------ the chain path
@pytest.mark.parametrize("nc", [1, 3])
def test_host_loo_predict_within_the_bounds(nc):
    X, y, tabs = pr.loo_inputs(nc)
    p_lo, p_hi = api._loo_interval_probs(95)
    c = api._loo_bracket_c(p_lo, p_hi)
    g, mu, tau2 = pr.window(tabs, pr.LOO_FIRST, pr.LOO_S)
    refs = pr.loo_reference(X, y, g, mu, tau2, p_lo, p_hi, c)
    E = pr.exact_eta(X, g, mu)
    ll = np.concatenate([api._host_loglik(t, X, y, pr.LOO_FIRST - 1, pr.LOO_S) for t in tabs], axis=1)
    lpd = api._psis_host(ll)[0]
    lwn, e, k = api._psis_weights_host(ll)
    mean, sd, pit, lo, hi, width = api._loo_predict_rows(E, tau2, y, lwn, p_lo, p_hi, solver="bisect")
    assert np.allclose(width, [d["width"] for d in refs], rtol=1e-14)
    skipped = pr.check_loo("%d chains" % nc, refs, (lpd, e, k, mean, sd, pit, lo, hi), p_lo, p_hi, _note)
    assert skipped <= pr.SKIP_FRACTION * len(y), skipped
    pr.check_loo_sums("%d chains" % nc, E, tau2, y, lwn, mean, sd, pit, _note)
    # the weights themselves, against the reference's, on the decided rows
    for i, d in enumerate(refs):
        if d["decided"] and d["fit_decided"]:
            _note("loo weights", pr.err_ratio(lwn[i], d["lw"]), "row %d" % i)


# ------------------------------------------------------------------------------------------------------------------ planted errors
def test_a_wrong_reference_fails_the_same_arithmetic():
    name, ll, Ms = pr.psis_cases(big=False)[1]                                      # crafted_rows, S = 400
    for i in (0, 3, 4, 5):
        M = Ms[i]
        lpd, elpd, k, lwn = api._psis_weights_row(ll[i].copy(), M)
        good = pr.psis(ll[i], M)
        assert pr.err_ratio(k, good["khat"]) < 1 and pr.err_ratio(elpd, good["elpd"]) < 1
        off = pr.psis(ll[i], M + 1)                                                 # the tail length off by one
        assert pr.err_ratio(k, off["khat"]) > 1e3 and pr.err_ratio(elpd, off["elpd"]) > 1e3 and pr.err_ratio(lwn, off["lw"]) > 1e3
        assert pr.err_ratio(k, good["k0"]) > 1e3                                    # the prior adjustment (k M + 5) / (M + 10) dropped
