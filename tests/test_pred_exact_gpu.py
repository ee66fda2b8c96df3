"""GPU tests of the prediction, WAIC and PSIS-LOO kernels (k_predict<1|2>, k_pred_loglik, k_pred_pit, k_psis<0|1>, k_psis_w<0|1>, k_inv_sd,
k_loo_moments, k_loo_quantile) against the extended-precision reference of tests/pred_ref.py (run with -m gpu on an MI355X): every output
lies within the a-priori bound of the device's float64 error; where eta is exactly representable it is the exact value bit for bit.
The inputs and the assertions are those that tests/test_pred_ref_host.py runs on the CPU with the float64 host restatements in the
device's place.  Every `ratio <stage> <error / bound>` is printed (pytest -s) and must be below 1; the worst per stage is reported at the end.

  the device's libm   a one-draw window exposes erfc (the PIT at tau2 = 1) and log (lpd at y = eta): their error against the long-double
                      reference stays within ERFC_ULPS and LIBM_ULPS, the budgets of the bounds
  k_predict           crafted tables (gamma and mu index-coded, X = k / 16: every partial sum is a double) at the edges of the tiling:
                      rows 1 .. 65, windows 1 .. 257, q = 3 .. 496 = 31 x 16, a first row other than 1, every predict_block_rows, three
                      chains pooled at unaligned column offsets; one-row windows and the order statistics give eta itself, the mean is the
                      exact mean to an ulp; then normal X and gamma against the bound gamma_(q16 + 2) sum |x| |gamma|
  k_pred_loglik, k_pred_pit   on the exact tables, 1 .. 513 draws, tau2 over six decades (an l spread far above 745: the exp underflows), a
                      row of equal l, and a row of nearly equal l of size 1e3 (ill-conditioned on purpose: the bound alone is asserted)
  PSIS on crafted rows   keys that differ in the lowest digit of the radix select, keys in every bin of the top digit, ties at the cutoff
                      (more than the tail, all / none / some of them in the tail, made by rounding), 2^21 + 513 draws with the tied draws on
                      both sides of every digit of the draw-index select, tail lengths 4 .. 257, 255 .. 257 draws
  the chain path      one chain and three pooled: lpd, elpd, k-hat, the LOO mean, sd and PIT against bounds built on the reference's own
                      weights, and again against the sums over the device's own weights; the quantiles by the residual of the reference's
                      mixture CDF

Measured on an MI355X: the device's erfc 1.76 ulp at most, its log 0.36 ulp; largest error / bound: eta 0.017 (order statistic 0.011, mean
0.00044; mean over the device's own eta 0.020), lpd 0.12, pwaic 0.065, pit 0.071; rows: k-hat 0.115, elpd 0.017, weights 0.45 (outside the
tail 0.35), sum of weights 0.030; chain path: l 0.25, lpd 0.060, elpd 0.012, k-hat 0.090, loo_mean 0.00058, loo_sd 0.00029, loo_pit 0.0023 (over
the device's own weights 0.051, 0.084, 0.060), loo_lower 0.38, loo_upper 0.077; no row skipped.  The ratios below 1e-3 are sums of many
independently rounded terms under a worst-case bound, which is why those stages have the second, sharper check (pred_ref's docstring)."""
import numpy as np
import pytest

import bnr_amd
import pred_ref as pr
from bnr_amd import _capi, api
from pred_ref import LD, U, VE

pytestmark = pytest.mark.gpu
WORST, LIBM = {}, {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    print("\nprediction and PSIS kernels, largest error/bound:", {k: "%.3g" % v for k, v in sorted(WORST.items())})
    print("device libm, largest error in ulps:", {k: "%.3g" % v for k, v in sorted(LIBM.items())})


def _note(stage, r, what):
    print("ratio %-26s %.3e  %s" % (stage, r, what))
    WORST[stage] = max(WORST.get(stage, 0.0), r)
    assert r < 1.0, (stage, r, what)


@pytest.fixture(scope="module")
def chains(gpu):
    """{V: the chains of that size}: three at V = 5 (the training rows of the chain path, tables of 520 rows), one elsewhere"""
    out = {}
    for V, q in pr.PREDICT_V.items():
        X, y = pr.loo_training() if V == 5 else (pr.exact_X(4, q, V), np.arange(4.0))
        first = bnr_amd.Chain(np.asfortranarray(X), y, 1, pr.LOGLIK_TOT if V == 5 else pr.PREDICT_TOT, 500 + V, 1, device=gpu)
        out[V] = [first] + [bnr_amd.Chain.like(first, 500 + V, c + 1) for c in range(1, 3 if V == 5 else 1)]
        for ch in out[V]:
            ch.init_prior()
    yield out
    for cs in out.values():
        for ch in cs:
            ch.close()


def _load(cs, tabs):
    for ch, t in zip(cs, tabs):
        ch.load(t)


# ------------------------------------------------------------------------------------------------------------------ the device's libm
def test_device_erfc_and_log_within_their_budgets(chains):
    ch = chains[5][0]
    t = pr.table(5, pr.LOGLIK_TOT, 55)
    taus = 10.0 ** np.r_[np.arange(-300.0, 301.0, 15.0), [-0.3, 0.2, 0.001]]
    t["mu"][:, 0, 0] = 0.0
    t["tau2"][0, 0, 0] = 1.0
    t["tau2"][1:1 + taus.size, 0, 0] = taus
    ch.load(t)
    # the arguments at which Phi is smallest in the later cases (the log-likelihood rows: far below the last normal double; the chain path)
    _n, lt, lX, ly, _S, _i = pr.loglik_inputs()[0]
    g, mu, tau2 = pr.window([lt], 2, 513)
    zl = np.min((ly[:, None] - pr.exact_eta(lX, g, mu)) / np.sqrt(tau2))
    X, y, tabs = pr.loo_inputs(1)
    g, mu, tau2 = pr.window(tabs, pr.LOO_FIRST, pr.LOO_S)
    zc = np.min((y[:, None] - pr.exact_eta(X, g, mu)) / np.sqrt(tau2))
    z = np.r_[np.linspace(-8, 8, 49), [-37.5, -37.0, -30.1, -12.3, -5.5, 1 / 3, 0.674489750196082, -0.674489750196082, np.pi, -np.e], zl, zc]
    assert 55 <= z.size <= 70
    pit = _capi.pooled_predict([ch], np.zeros((z.size, 15)), 1, 1, 1, 1, y=z, pit=True)[7]
    arg = -z / 1.41421356237309504880                                               # the device's own float64 argument
    ref = pr.erfc_ld(np.asarray(arg, dtype=LD)) / 2
    err = np.abs(pr.f64(np.asarray(pit, dtype=LD) - ref))
    normal = pr.f64(ref) >= pr.TINY
    ulps = err[normal] / (U * pr.f64(ref)[normal])
    print("erfc: %.3f ulp at most (z = %.4g); below the normal range %.3g at most" % (ulps.max(), z[normal][np.argmax(ulps)], err[~normal].max(initial=0.0)))
    LIBM["erfc"] = float(ulps.max())
    assert np.all(ulps <= pr.ERFC_ULPS), ulps.max()
    assert np.all(err[~normal] <= 2.0 ** -1022 * pr.ERFC_ULPS * U + pr.DENORM)
    # log: lpd of one draw at y = eta is -(log 2 pi + log tau2) / 2, one rounded sum on top of the device's log
    c64 = 1.8378770664093454836
    worst = 0.0
    for j, tau in enumerate(taus):
        lpd = ch.predict(np.zeros((1, 15)), 2 + j, 1, 1, 1, y=[0.0])[3]
        want = LD(c64) + np.log(LD(tau))
        e = float(abs(LD(-2.0 * lpd[0]) - want)) - U * abs(float(want))             # less the rounding of the sum
        lg = abs(float(np.log(LD(tau))))
        assert e <= pr.LIBM_ULPS * U * lg, (tau, e, lg)
        if lg > 0:                                                                  # (tau2 = 1: the log is 0 and must be exact)
            worst = max(worst, e / (U * lg))
    print("log: %.3f ulp at most" % worst)
    LIBM["log"] = worst


# ------------------------------------------------------------------------------------------------------------------ k_predict, exact
def _predict(cs, X, first, nsamp, k_lo, k_hi):
    if len(cs) == 1:
        return cs[0].predict(X, first, nsamp, k_lo, k_hi)[:3]
    return _capi.pooled_predict(cs, X, first, nsamp, k_lo, k_hi)[:3]


def test_predict_is_exact_on_exactly_representable_tables(chains):
    tabs = {V: [pr.table(V, pr.LOGLIK_TOT if V == 5 else pr.PREDICT_TOT, V + c, pr.CHAIN_OFFSET * c) for c in range(len(chains[V]))] for V in chains}
    for V in chains:
        _load(chains[V], tabs[V])
    seen = {k: set() for k in ("m", "nsamp", "V", "blk")}
    for V, m, nsamp, first, blk, nc in pr.PREDICT_CASES:
        what = "V=%d m=%d nsamp=%d first=%d block=%d chains=%d" % (V, m, nsamp, first, blk, nc)
        cs = chains[V][:nc]
        X = pr.predict_X(V, m)
        g, mu, _t = pr.window(tabs[V][:nc], first, nsamp)
        E = pr.exact_eta(X, g, mu)
        S = nc * nsamp
        srt, em = np.sort(E, axis=1), pr.exact_mean(E)
        cs[0].set_option("predict_block_rows", blk)
        try:
            for k_lo, k_hi in pr.order_ranks(S):
                mean, lo, hi = _predict(cs, X, first, nsamp, k_lo, k_hi)
                assert np.array_equal(lo, srt[:, k_lo - 1]) and np.array_equal(hi, srt[:, k_hi - 1]), (what, k_lo, k_hi)
                assert np.all(np.abs(mean - em) <= np.spacing(np.abs(em))), (what, np.max(np.abs(mean - em)))
            if nc == 1:                                                             # one-row windows: that draw's eta
                for s in sorted({0, 1, 15, 16, 31, 32, nsamp - 1}):
                    if s < nsamp:
                        m1, l1, h1 = _predict(cs, X, first + s, 1, 1, 1)
                        assert np.array_equal(m1, E[:, s]) and np.array_equal(l1, m1) and np.array_equal(h1, m1), (what, s)
        finally:
            cs[0].set_option("predict_block_rows", 0)
        for k, v in zip(("m", "nsamp", "V", "blk"), (m, nsamp, V, blk)):
            seen[k].add(v)
    assert seen == dict(m={1, 16, 17, 31, 32, 33, 65}, nsamp={1, 15, 16, 17, 31, 32, 33, 127, 128, 129, 257}, V=set(pr.PREDICT_V), blk={0, 1, 32})


def test_predict_on_real_values_within_the_bound(gpu):
    t, X = pr.real_case()
    Xt, yt, _ = bnr_amd.make_synthetic(6, 12, 1, seed=3)
    ch = bnr_amd.Chain(Xt, yt, 1, 300, 77, 1, device=gpu)
    ch.init_prior()
    ch.load(t)
    g, mu, _ = pr.window([t], 1, 300)
    ref = pr.eta(X, g, mu)
    assert np.all(pr.nonvacuous(ref))
    Edev = np.empty(ref.v.shape)
    for s in range(300):                                                            # one-row windows: the device's own eta of every draw
        m1, l1, h1 = ch.predict(X, 1 + s, 1, 1, 1)[:3]
        assert np.array_equal(m1, l1) and np.array_equal(m1, h1)
        Edev[:, s] = m1
    _note("eta", pr.err_ratio(Edev, ref), "V=12 normal, every draw")
    # the whole window: the order statistics are those of the device's own eta, bit for bit; the mean is its strided sum and one quotient --
    # a bound of a few ulps of sum |eta| / S.  Against the reference's eta the same outputs only have the worst-case sum of the errors of
    # 300 etas as their bound, some 1000 times the rounding of the sum itself
    srt = np.sort(Edev, axis=1)
    sharp = pr.vsum(VE(np.asarray(Edev, dtype=LD))) / 300.0
    bound = VE(np.sort(ref.v, axis=1), np.max(ref.e, axis=1, keepdims=True) * np.ones(ref.e.shape))
    rmean = pr.vsum(ref) / 300.0
    for k_lo, k_hi in pr.order_ranks(300):
        mean, lo, hi = ch.predict(X, 1, 300, k_lo, k_hi)[:3]
        assert np.array_equal(lo, srt[:, k_lo - 1]) and np.array_equal(hi, srt[:, k_hi - 1]), (k_lo, k_hi)
        _note("eta mean over the device's eta", pr.err_ratio(mean, sharp), "V=12 normal")
        _note("eta order statistic", max(pr.err_ratio(lo, bound[:, k_lo - 1]), pr.err_ratio(hi, bound[:, k_hi - 1])), "ranks %d, %d" % (k_lo, k_hi))
        _note("eta mean", pr.err_ratio(mean, rmean), "V=12 normal")
    ch.close()


# ------------------------------------------------------------------------------------------------------------------ k_pred_loglik, k_pred_pit
def test_loglik_and_pit_within_the_bounds(chains):
    ch = chains[5][0]
    for name, t, X, y, Ss, ill in pr.loglik_inputs():
        ch.load(t)
        for S in Ss:
            g, mu, tau2 = pr.window([t], 2, S)
            E = VE(np.asarray(pr.exact_eta(X, g, mu), dtype=LD))
            L = pr.ell(y, E, tau2)
            rl, rp = pr.lpd_pwaic(L)
            out = _capi.pooled_predict([ch], X, 2, S, 1, S, y=y, pit=True)
            skipped = pr.check_pointwise(name, rl, rp, pr.pit(y, E, tau2), out[3], out[4], out[7], S, ill, _note)
            assert skipped <= pr.SKIP_FRACTION * len(y), (name, S, skipped)
            if S == 1:
                _note("lpd of one draw = l", pr.err_ratio(out[3], L[:, 0]), name)


# ------------------------------------------------------------------------------------------------------------------ PSIS on crafted rows
@pytest.mark.parametrize("case", range(len(pr.PSIS_NAMES)), ids=pr.PSIS_NAMES)
def test_psis_on_crafted_rows_within_the_bounds(gpu, case):
    name, ll, Ms = pr.psis_cases(big=True)[case]                                    # (built at the first use, not at collection)
    S = ll.shape[1]
    r = None if all(M == pr.tail_length(S) for M in Ms) else [1.0 if M == pr.tail_length(S) else pr.r_eff_for(S, M) for M in Ms]
    lpd, elpd, k = _capi.psis_loo_raw(ll, r, gpu)
    skipped = pr.run_psis_case(name, ll, Ms, (lpd, elpd, k, None), False, _note)
    lw, ew, kw = _capi.psis_weights_raw(ll, r, gpu)
    skipped = max(skipped, pr.run_psis_case(name, ll, Ms, (None, ew, kw, lw), True, _note))
    assert skipped <= pr.SKIP_FRACTION * len(Ms), (name, skipped)


# ------------------------------------------------------------------------------------------------------------------ the chain path
@pytest.mark.parametrize("nc", [1, 3])
def test_loo_predict_of_chains_within_the_bounds(chains, nc):
    X, y, tabs = pr.loo_inputs(nc)
    cs = chains[5][:nc]
    _load(cs, tabs)
    p_lo, p_hi = api._loo_interval_probs(95)
    g, mu, tau2 = pr.window(tabs, pr.LOO_FIRST, pr.LOO_S)
    refs = pr.loo_reference(X, y, g, mu, tau2, p_lo, p_hi, api._loo_bracket_c(p_lo, p_hi))
    fields = _capi.pooled_loo_predict(cs, pr.LOO_FIRST, pr.LOO_S, None, p_lo, p_hi)
    skipped = pr.check_loo("%d chains" % nc, refs, fields, p_lo, p_hi, _note)
    assert skipped <= pr.SKIP_FRACTION * len(y), skipped
    # k_loo_moments alone.  A one-draw window with y gives lpd = l, the device's own l of every draw; k_psis_w<0> on it is k_psis_w<1>'s code
    # behind pass 1, so its output is the weights k_loo_moments read: elpd and k-hat bit for bit, and the moments within the bound of their
    # own sums (check_loo above bounds them by the whole error of the weights, some 1000 times wider)
    E = pr.exact_eta(X, g, mu)
    Ldev = np.column_stack([ch.predict(X, pr.LOO_FIRST + s, 1, 1, 1, y=y)[3] for ch in cs for s in range(pr.LOO_S)])
    _note("l of every draw", pr.err_ratio(Ldev, pr.ell(y, VE(np.asarray(E, dtype=LD)), tau2)), "%d chains" % nc)
    lwd, ed, kd = _capi.psis_weights_raw(Ldev, None, 0)
    assert np.array_equal(ed, fields[1]) and np.array_equal(kd, fields[2])
    pr.check_loo_sums("%d chains" % nc, E, tau2, y, lwd, fields[3], fields[4], fields[5], _note)
    # k_psis<1>: the same reference (a row from eta has no exact ties)
    lpd, elpd, k = _capi.pooled_loo(cs, pr.LOO_FIRST, pr.LOO_S)
    for i, d in enumerate(refs):
        rat, _skip, bad = pr.check_psis(d, elpd[i], k[i], None, lpd[i])
        assert not bad, (i, bad)
        for stage, r in rat.items():
            _note("k_psis " + stage, r, "%d chains row %d" % (nc, i))
    # lpd is bit for bit loglik_stats's
    ls = _capi.pooled_loglik_stats(cs, pr.LOO_FIRST, pr.LOO_S)[0]
    assert np.array_equal(fields[0], ls) and np.array_equal(lpd, ls)
    if nc == 1:
        one = cs[0].loo_predict(pr.LOO_FIRST, pr.LOO_S, None, p_lo, p_hi)
        assert all(np.array_equal(u, v) for u, v in zip(one, fields))
        assert np.array_equal(cs[0].loo(pr.LOO_FIRST, pr.LOO_S)[1], elpd)
