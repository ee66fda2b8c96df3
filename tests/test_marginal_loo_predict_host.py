"""CPU tests of the marginal LOO predictive checks (include/bnr_mcheck.h, libbnr_mcheck.so): the numpy restatement api._host_weighted_mixture
against the mpmath reference within the derived bound (tests/mcheck_ref.py), the closed forms, the refit fact that motivates the feature on a
seeded CPU fit, what the library exports and which kernels its code object holds, the ctypes signatures, the refusals and the Fit plumbing with
the device call stubbed.  No GPU."""
import ctypes as C
import dataclasses
import inspect
import math
import os
import re
import subprocess
import types

import numpy as np
import pytest

import bnr_amd
import code_objects as co
import mcheck_ref as cr
from bnr_amd import _capi, api
from oracle import bnr_oracle as bo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("mean", "sd", "pit", "lower", "upper")


def _strip_comments(src):
    return re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", src, flags=re.S))


def _host(c, rows, p_lo, p_hi, with_y=True, solver=None):
    out = api._host_weighted_mixture(c["mean"][:rows], c["var"][:rows], c["logw"][:rows], c["y"][:rows] if with_y else None, p_lo, p_hi, solver)
    return dict(zip(FIELDS, out[:5]))


# ------------------------------------------------------------------------------------------ the numpy restatement within the bound
@pytest.mark.parametrize("pattern", cr.PATTERNS)
@pytest.mark.parametrize("D", (1, 2, 63, 64, 65, 257))
@pytest.mark.parametrize("rows", (1, 3))
def test_host_restatement_meets_the_bound(rows, D, pattern):
    p_lo, p_hi = api._loo_interval_probs(95)
    c = cr.case(D, pattern)
    got = _host(c, rows, p_lo, p_hi)
    worst = cr.check_case(D, pattern, rows, got, p_lo, p_hi)
    if D in (2, 65):                                                     # the library's own bisection instead of brentq, and the form without y
        cr.check_case(D, pattern, rows, _host(c, rows, p_lo, p_hi, solver="bisect"), p_lo, p_hi)
        noy = _host(c, rows, p_lo, p_hi, with_y=False)
        assert np.isnan(noy["pit"]).all()
        cr.check_case(D, pattern, rows, noy, p_lo, p_hi, with_y=False)
    print("rows=%d D=%d %s: worst error / bound %s" % (rows, D, pattern, {k: "%.3g" % v for k, v in worst.items()}))


def test_bracket_constant_is_the_librarys():
    for interval in (50, 90, 95, 99):
        p_lo, p_hi = api._loo_interval_probs(interval)
        assert cr.bracket_c(p_lo, p_hi) == api._loo_bracket_c(p_lo, p_hi)


def test_nan_rules_of_the_restatement():
    c = cr.case(65, "random")
    base = _host(c, 3, 0.025, 0.975)
    for what in ("var_nan", "var_neg", "mean_nan", "lw_inf", "lw_ninf", "lw_nan"):
        m, v, lw = c["mean"][:3].copy(), c["var"][:3].copy(), c["logw"][:3].copy()
        {"var_nan": v, "var_neg": v, "mean_nan": m, "lw_inf": lw, "lw_ninf": lw, "lw_nan": lw}[what][1, 7] = \
            {"var_nan": np.nan, "var_neg": -1.0, "mean_nan": np.nan, "lw_inf": np.inf, "lw_ninf": -np.inf, "lw_nan": np.nan}[what]
        got = dict(zip(FIELDS, api._host_weighted_mixture(m, v, lw, c["y"][:3], 0.025, 0.975)[:5]))
        for k in FIELDS:
            assert math.isnan(got[k][1]) and np.array_equal(got[k][[0, 2]], base[k][[0, 2]]), (what, k)
    y = c["y"][:3].copy()
    y[2] = np.nan                                                        # a NaN y: mean, sd and pit (formed through y) are NaN, the bounds are not
    got = dict(zip(FIELDS, api._host_weighted_mixture(c["mean"][:3], c["var"][:3], c["logw"][:3], y, 0.025, 0.975)[:5]))
    assert all(math.isnan(got[k][2]) for k in ("mean", "sd", "pit")) and got["lower"][2] == base["lower"][2] and got["upper"][2] == base["upper"][2]
    assert all(np.array_equal(got[k][:2], base[k][:2]) for k in FIELDS)


# ------------------------------------------------------------------------------------------ closed forms
def test_closed_forms():
    rng = np.random.default_rng(187)
    m, v, y = rng.normal(size=(4, 1)) * 3, rng.exponential(size=(4, 1)) + 0.1, rng.normal(size=4) * 2
    lw = np.zeros((4, 1))
    import mpmath as mp
    for interval in (95, 50):
        p_lo, p_hi = api._loo_interval_probs(interval)
        mean, sd, pit, lo, hi, width = api._host_weighted_mixture(m, v, lw, y, p_lo, p_hi)
        with mp.workdps(30):
            zp = float(mp.sqrt(2) * mp.erfinv(2 * mp.mpf(p_hi) - 1))
        s = np.sqrt(v[:, 0])
        assert np.all(np.abs(mean - m[:, 0]) <= 9 * cr.U * (np.abs(y - m[:, 0]) + np.abs(y)))       # D = 1: mean = y - (y - m)
        e2 = v[:, 0] + m[:, 0] ** 2                                                                   # sd^2 = (var + m^2) - mean^2: four roundings of size e2
        assert np.all(np.abs(sd - s) <= 4 * cr.U * e2 / (2 * s) + 2 * np.spacing(s))
        ref = np.array([0.5 * math.erfc(-(y[i] - m[i, 0]) / s[i] / math.sqrt(2)) for i in range(4)])
        assert np.all(np.abs(pit - ref) <= 16 * cr.U * ref)
        h = width * 2.0 ** -40
        assert np.all(np.abs(lo - (m[:, 0] - zp * s)) <= h + 8 * cr.U * (np.abs(m[:, 0]) + zp * s))
        assert np.all(np.abs(hi - (m[:, 0] + zp * s)) <= h + 8 * cr.U * (np.abs(m[:, 0]) + zp * s))
    assert np.array_equal(api._host_weighted_mixture(m, v, lw, None, 0.25, 0.75)[0], m[:, 0])        # without y the mean is sum w m = m
    # uniform weights: the mean of _host_mixture_summary (draws x columns, its own summation order) to the sum bound of both
    for D in (2, 65, 257):
        c = cr.case(D, "uniform")
        mine = api._host_weighted_mixture(c["mean"], c["var"], c["logw"], None, 0.025, 0.975)[0]
        theirs = api._host_mixture_summary(c["mean"].T, c["var"].T, 1)["mean"]
        b = cr.numpy_bounds(c["mean"], c["var"], c["logw"])["tol_mean"]
        assert np.all(np.abs(mine - theirs) <= 2 * cr.GATE * b), D
    # one point mass: the bracket has no width, every statistic is the point's
    one = api._host_weighted_mixture(np.full((1, 5), 1.5), np.zeros((1, 5)), np.full((1, 5), math.log(0.2)), None, 0.025, 0.975)
    assert one[3][0] == 1.5 and one[4][0] == 1.5 and abs(one[0][0] - 1.5) <= 4e-16 and one[1][0] <= 1e-7


# ------------------------------------------------------------------------------------------ the refit fact
def _oracle_table(X, y, seed):
    o = bo.Oracle(X, y, 3, 3000, seed, chain=1, pdf_mode=1)
    o.init_prior()
    o.run(2, 3000, 3000)
    return o.t


def _refit_predictive(X, y, i, seed):
    """(mean, sd, pit) of the true leave-one-out predictive of row i: the fit without the row, then the mixture of N(mean_s, var_s + tau2_s) of
    the left-out row over the refit's 1500 draws (api._host_predict_terms), uniform weights"""
    Xa, ya = np.delete(X, i, axis=0), np.delete(y, i)
    t2, mu, S, W = api._host_marginal_draws([_oracle_table(Xa, ya, seed)], 1500, 1500, 1)
    mean, var, nb = api._host_predict_terms(Xa, ya, X[i:i + 1], t2, mu, S, W)
    assert nb == 0
    mean, vo = mean[:, 0], var[:, 0] + t2
    mm = float(mean.mean())
    return mm, math.sqrt(float(np.mean(vo + mean * mean)) - mm * mm), float(np.mean(0.5 * api._erfc(-((y[i] - mean) / np.sqrt(vo)) / math.sqrt(2.0))))


def test_marginal_checks_match_a_refit_where_the_conditional_ones_do_not():
    """the seeded CPU fit of the issue: n = 60, V = 10, R = 3, rows 1500 .. 2999 (0-based) of 3000; rows 0, 6, .., 54 are refitted twice (seeds
    4242 and 99).  The tolerance comes from the reference alone: g = the largest gap between the two refits, for the mean in units of the row's
    LOO sd and for the pit; the PSIS estimate adds its own Monte Carlo error to a refit's, hence 3 g.  Measured here: marginal against refit
    0.043 sd at most (g = 0.044), pit 0.004 (g = 0.023); squared mean gaps 0.0067 (marginal) against 1.34 (conditional)."""
    X, y, _ = bnr_amd.make_synthetic(60, 10, 3, seed=7)
    X, y = np.asarray(X, dtype=np.float64), np.asarray(y, dtype=np.float64)
    t = _oracle_table(X, y, 4242)
    marg = api._host_marginal_loo_predict([t], X, y, 1500, 1500)
    cond = api._host_loo_predict([t], X, y, 1500, 1500)
    assert marg.n_bad == 0 and marg.draws == 1500 and marg.thin == 1 and marg.chains == 1
    rows = list(range(0, 60, 6))
    A = np.array([_refit_predictive(X, y, i, 4242) for i in rows])
    B = np.array([_refit_predictive(X, y, i, 99) for i in rows])
    sd = marg.loo_sd[rows]
    g_mean = float(np.max(np.abs(A[:, 0] - B[:, 0]) / sd))
    g_pit = float(np.max(np.abs(A[:, 2] - B[:, 2])))
    gap_m = np.abs(marg.loo_mean[rows] - A[:, 0])
    gap_c = np.abs(cond.loo_mean[rows] - A[:, 0])
    gap_p = np.abs(marg.loo_pit[rows] - A[:, 2])
    ok = marg.pareto_k[rows] <= 0.7
    print("rows %s\nmarginal k-hat %s\n|marginal - refit A| mean %s (in LOO sd: %s)\n|conditional - refit A| mean %s\n|refit A - refit B| mean, largest in LOO sd: g = %.4f"
          "\n|marginal - refit A| pit %s; |refit A - refit B| pit, largest: g = %.4f\nsum of squared mean gaps: marginal %.4g, conditional %.4g"
          % (rows, np.round(marg.pareto_k[rows], 2), np.round(gap_m, 4), np.round(gap_m / sd, 4), np.round(gap_c, 4), g_mean, np.round(gap_p, 4), g_pit,
             float(np.sum(gap_m ** 2)), float(np.sum(gap_c ** 2))))
    assert ok.any()
    assert np.all(gap_m[ok] / sd[ok] <= 3 * g_mean), float(np.max(gap_m[ok] / sd[ok]))
    assert np.all(gap_p[ok] <= 3 * g_pit), float(np.max(gap_p[ok]))
    assert float(np.sum(gap_m ** 2)) < 0.25 * float(np.sum(gap_c ** 2))


# ------------------------------------------------------------------------------------------ the library
def test_mcheck_library_exports_exactly_what_its_header_declares():
    hdr = _strip_comments(open(os.path.join(ROOT, "include", "bnr_mcheck.h")).read())
    declared = set(re.findall(r"\b(bnr_[a-zA-Z0-9_]+)\s*\(", hdr))
    assert declared == set(_capi.MCHECK_EXPORTS) and len(declared) == 4
    assert declared == {"bnr_mcheck_abi_version", "bnr_mcheck_set_option", "bnr_weighted_mixture", "bnr_chains_marginal_loo_predict"}
    assert os.path.exists(bnr_amd.MCHECK_LIB), "libbnr_mcheck.so has not been built"
    syms = subprocess.run(["nm", "-D", "--defined-only", bnr_amd.MCHECK_LIB], check=True, stdout=subprocess.PIPE, text=True).stdout
    defined = {line.split()[-1] for line in syms.splitlines() if line.strip()}
    assert defined == declared, defined ^ declared                               # no kernel handle, host stub or template instance is exported
    L = _capi.mcheck_lib()
    assert L.bnr_mcheck_abi_version() == int(re.search(r"#define BNR_MCHECK_ABI_VERSION (\d+)", hdr).group(1)) == 1
    for name in ("MarginalLOOPredict", "MarginalLOOPredictive", "weighted_mixture", "device_marginal_loo_predict", "mcheck_lib", "MCHECK_LIB"):
        assert hasattr(bnr_amd, name), name
    needed = subprocess.run(["readelf", "-d", bnr_amd.MCHECK_LIB], check=True, stdout=subprocess.PIPE, text=True).stdout
    assert "libbnr_hip.so" in needed and "$ORIGIN" in needed
    assert "libbnr_mloo" not in needed and "libbnr_medge" not in needed and "libbnr_mpred" not in needed


def test_mcheck_code_object_holds_the_four_kernels_and_its_own(tmp_path, monkeypatch):
    if not (co.have_tools() and os.path.exists(bnr_amd.MCHECK_LIB)):
        pytest.skip("no ROCm LLVM tools / no built library here")
    monkeypatch.setattr(co, "LIB", bnr_amd.MCHECK_LIB)
    cos = co.code_objects(tmp_path)
    assert len(cos) == 1
    own = co.declared_kernels("bnr_mcheck_kernels.h")
    assert own == {"k_mcheck_stage", "k_mcheck_moments", "k_mcheck_quantile"}
    four = co.declared_kernels("bnr_mloo_kernels.h")
    assert four == {"k_mloo_w", "k_mloo_rhs", "k_mloo_gram", "k_mloo_factor"}
    assert set(cos[0]) == own | four, set(cos[0]) ^ (own | four)
    assert not (own | four) & {re.sub(r"<.*", "", k) for k in co.SWEEP | co.ANALYSIS}


def test_ctypes_signatures():
    L = _capi.mcheck_lib()
    dp = C.c_void_p
    assert L.bnr_weighted_mixture.argtypes == [C.c_int32] * 3 + [dp] * 4 + [C.c_double] * 2 + [dp] * 5 and L.bnr_weighted_mixture.restype is C.c_int
    f = L.bnr_chains_marginal_loo_predict
    assert f.argtypes == [C.POINTER(C.c_void_p)] + [C.c_int32] * 4 + [dp] + [C.c_double] * 2 + [dp] * 9 + [C.POINTER(C.c_int32)] and f.restype is C.c_int
    assert L.bnr_mcheck_set_option.argtypes == [C.c_char_p, C.c_int64] and L.bnr_mcheck_abi_version.argtypes == []
    hdr = _strip_comments(open(os.path.join(ROOT, "include", "bnr_mcheck.h")).read())
    for name, sig in _capi._MCHECK_SIGS.items():                                 # one ctypes argument per parameter of the header
        params = re.search(r"\b%s\s*\((.*?)\)\s*;" % name, hdr, flags=re.S).group(1).strip()
        assert len(sig[1]) == (0 if params == "void" else params.count(",") + 1), name


# ------------------------------------------------------------------------------------------ refusals
def test_refusals(monkeypatch):
    L = _capi.mcheck_lib()
    a = np.ones(8)
    p = _capi._ptr(a)
    err = lambda: _capi.lib().bnr_last_error()

    def raw(rows=2, D=2, mean=p, var=p, lw=p, y=p, p_lo=0.025, p_hi=0.975, om=p, sd=None, pit=None, lo=None, hi=None):
        return L.bnr_weighted_mixture(0, rows, D, mean, var, lw, y, p_lo, p_hi, om, sd, pit, lo, hi)

    for kw, word in ((dict(mean=None), b"NULL"), (dict(var=None), b"NULL"), (dict(lw=None), b"NULL"), (dict(om=None), b"at least one"),
                     (dict(rows=0), b"rows >= 1"), (dict(D=0), b"rows >= 1"), (dict(rows=1 << 16, D=1 << 15), b"2^31"), (dict(rows=46341, D=46341), b"2^31"),
                     (dict(y=None, pit=p), b"pit needs y"), (dict(lo=p, p_lo=0.0), b"p_lo"), (dict(hi=p, p_lo=0.6, p_hi=0.5), b"p_lo"),
                     (dict(lo=p, p_hi=1.0), b"p_lo"), (dict(lo=p, p_lo=float("nan")), b"p_lo")):
        assert raw(**kw) == _capi.BNR_ERR_BAD_ARG and word in err(), kw
    h = (C.c_void_p * 1)(None)

    def chain(ch=h, K=1, first=1, ns=1, thin=1, p_lo=0.025, p_hi=0.975, el=p, kh=p, mean=None, lo=None):
        return L.bnr_chains_marginal_loo_predict(ch, K, first, ns, thin, None, p_lo, p_hi, el, kh, mean, None, None, lo, None, None, None, None)

    assert chain(ch=None) == 1 and b"NULL argument" in err()                       # bnr_chains_marginal_loo's refusals, in its order
    assert chain(el=None) == 1 and b"NULL argument" in err()
    assert chain(K=0) == 1 and b"nchains" in err()
    assert chain(thin=0) == 1 and b"thin" in err()
    assert chain(lo=p, p_lo=0.7, p_hi=0.3) == 1 and b"p_lo" in err()
    assert chain(p_lo=0.7, p_hi=0.3) == 1 and b"NULL chain" in err()              # p is read only where a bound is asked for
    assert chain() == 1 and b"NULL chain" in err()
    M = _capi.mloo_lib()
    assert M.bnr_chains_marginal_loo(h, 1, 1, 1, 1, None, p, p, None, None, None, None, None) == 1 and b"NULL chain" in err()
    assert L.bnr_mcheck_set_option(b"no_such", 1) == 1 and L.bnr_mcheck_set_option(b"mcheck_batch_draws", -1) == 1 and L.bnr_mcheck_set_option(None, 1) == 1
    assert L.bnr_mcheck_set_option(b"mloo_batch_draws", 1) == 1                    # (the other library's option)
    assert L.bnr_mcheck_set_option(b"mcheck_batch_draws", 0) == 0
    m = np.ones((3, 4))
    for args in ((np.ones(4), np.ones(4), np.ones(4)), (m, np.ones((3, 5)), m), (m, m, np.ones((4, 3))), (np.ones((0, 4)), np.ones((0, 4)), np.ones((0, 4)))):
        with pytest.raises(ValueError):
            bnr_amd.weighted_mixture(*args)
    with pytest.raises(ValueError):
        bnr_amd.weighted_mixture(m, m, m, y=np.ones(4))
    with pytest.raises(ValueError):
        bnr_amd.weighted_mixture(m, m, m, interval=100)
    with pytest.raises(ValueError):
        _capi.weighted_mixture_raw(m, m, m, fields=("pit",))                        # pit only with y
    with pytest.raises(ValueError):
        _capi.weighted_mixture_raw(m, m, m, fields=("median",))
    big = np.lib.stride_tricks.as_strided(np.ones(1), shape=(46341, 46341), strides=(0, 0))     # (a view of one double: refused before any copy)
    with pytest.raises(ValueError, match="2\\^31"):
        _capi.weighted_mixture_raw(big, big, big)
    with pytest.raises(ValueError, match="2048"):
        api._fit_requests(np.zeros(2049), 2, X_new=_capi.XInput(np.zeros((2049, 3))), nsamp=10, x_transform=False, marginal_loo_predict=True)
    fake = types.SimpleNamespace(n=2049, q=3, h=None)
    monkeypatch.setattr(_capi, "_pooled", lambda chains: (fake, (None, 1)))
    with pytest.raises(ValueError, match="2048"):
        _capi.chains_marginal_loo_predict([fake], 1, 10)
    monkeypatch.undo()
    res = api.Results(None, np.zeros(1), np.zeros(1), 0, 1)
    with pytest.raises(ValueError):
        api.MarginalLOOPredict(res)


# ------------------------------------------------------------------------------------------ Fit
def test_fit_plumbing_with_the_device_call_stubbed(monkeypatch):
    y = np.zeros(5)
    assert api._fit_requests(y, 2).marginal_loo_predict is None
    assert api._fit_requests(y, 2, marginal_loo_predict=True).marginal_loo_predict == (2000, 95)
    assert api._fit_requests(y, 2, marginal_loo_predict=True, marginal_loo_draws=7, predict_interval=50).marginal_loo_predict == (7, 50)
    for bad in (0, 1.5, -3, True):
        with pytest.raises(ValueError):
            api._fit_requests(y, 2, marginal_loo_predict=True, marginal_loo_draws=bad)
    with pytest.raises(ValueError):
        api._fit_requests(y, 2, marginal_loo_predict=True, predict_interval=100)
    for fn in (bnr_amd.Fit, bnr_amd.generate_samples, bnr_amd.generate_samples_dbl, api._fit_requests):
        par = inspect.signature(fn).parameters
        assert par["marginal_loo_predict"].default is False and list(par)[-1] == "marginal_loo_predict", fn   # added after the existing keywords
    monkeypatch.setattr(api, "_rank_world", lambda: (0, 2))                         # chains spread over two ranks: refused before any sampling
    with pytest.raises(ValueError, match="marginal_loo_predict"):
        api._fit_requests(y, 2, marginal_loo_predict=True)
    with pytest.raises(ValueError, match="marginal_loo_predict"):
        bnr_amd.Fit(np.zeros((5, 3)), y, 2, x_transform=False, marginal_loo_predict=True, filename=None)
    monkeypatch.undo()

    calls, loo_calls = [], []

    def stub(chains, nburn, nsamp, thin=1, interval=95, r_eff=None):
        calls.append((list(chains), nburn, nsamp, thin, interval, r_eff))
        return types.SimpleNamespace(stub=len(calls), interval=interval)

    def loo_stub(chains, nburn, nsamp, thin=1, r_eff=None, per_chain=False):
        loo_calls.append((list(chains), nburn, nsamp, thin, r_eff))
        return {"loo": len(loo_calls)}

    monkeypatch.setattr(api, "device_marginal_loo_predict", stub)
    monkeypatch.setattr(api, "device_marginal_loo", loo_stub)
    c1, c2 = types.SimpleNamespace(name=1), types.SimpleNamespace(name=2)
    cs = types.SimpleNamespace(chains={1: c1, 2: c2}, ids=[1, 2])
    base = dict(return_state=False)
    new = lambda: api.Results(None, np.zeros(1), np.zeros(1), 30, 45)
    res = api._finish(cs, new(), api._fit_requests(y, 2, marginal_loo_predict=True, marginal_loo_draws=20, **base), 1)
    assert res.marginal_loo_predictive.stub == 1 and calls[-1] == ([c1], 30, 45, 3, 95, None) and res.stat_chains == 1     # chain 1, thin = ceil(45 / 20)
    assert res.marginal_loo is None and not loo_calls
    res = api._finish(cs, new(), api._fit_requests(y, 2, marginal_loo_predict=True, pool_chains=True, loo_r_eff=0.5, predict_interval=50, **base), 1)
    assert res.marginal_loo_predictive.stub == 2 and calls[-1] == ([c1, c2], 30, 45, 1, 50, 0.5) and res.stat_chains == 2
    assert api.MarginalLOOPredict(res) is res.marginal_loo_predictive and api.MarginalLOOPredict(res, interval=50) is res.marginal_loo_predictive
    # marginal_loo beside it still makes its own call
    res = api._finish(cs, new(), api._fit_requests(y, 2, marginal_loo_predict=True, marginal_loo=True, marginal_loo_draws=9, **base), 1)
    assert res.marginal_loo == {"loo": 1} and loo_calls[-1] == ([c1], 30, 45, 5, None) and calls[-1] == ([c1], 30, 45, 5, 95, None)
    # stack_chains: the stacking record gets no new attribute and is not read
    stack = types.SimpleNamespace(weights=np.array([0.25, 0.75]), summary=None, prediction=None, edge_cov=None, marginal_edges=None)
    monkeypatch.setattr(api, "device_stack_chains", lambda chains, nb, ns, r_eff: stack)
    before = dict(vars(stack))
    n_calls = len(calls)
    res = api._finish(cs, new(), api._fit_requests(y, 2, marginal_loo_predict=True, stack_chains=True, **base), 1)
    assert len(calls) == n_calls + 1 and calls[-1][0] == [c1] and res.stacking is stack and set(vars(stack)) == set(before)
    assert all(vars(stack)[k] is before[k] for k in before)
    # without the flag: no call, and the Results field for field what it was
    n_calls = len(calls)
    plain = api._finish(cs, new(), api._fit_requests(y, 2, stack_chains=True, **base), 1)
    with_flag = api._finish(cs, new(), api._fit_requests(y, 2, stack_chains=True, marginal_loo_predict=True, **base), 1)
    assert len(calls) == n_calls + 1 and plain.marginal_loo_predictive is None
    for f in api.Results.__dataclass_fields__:
        if f not in ("marginal_loo_predictive", "stat_chains"):
            a, b = getattr(plain, f), getattr(with_flag, f)
            assert (a is b) or np.array_equal(a, b), f
    bare = api._finish(cs, new(), api._fit_requests(y, 2, **base), 1)
    assert bare == api.Results(None, bare.rhatxi, bare.rhatgamma, 30, 45) and bare.marginal_loo_predictive is None and bare.stat_chains is None
    names = [f.name for f in dataclasses.fields(api.Results)]
    assert names[-1] == "marginal_loo_predictive" and {f.name: f.default for f in dataclasses.fields(api.Results)}["marginal_loo_predictive"] is None
    lp = [f.name for f in dataclasses.fields(api.LOOPredictive)]
    assert [f.name for f in dataclasses.fields(api.MarginalLOOPredictive)] == lp + ["thin", "chains", "n_bad", "logml", "loo"]


def test_accessor_falls_back_to_the_state_table():
    V, R, n = 2, 2, 6
    q = V * (V + 1) // 2
    rng = np.random.default_rng(188)
    X, y = rng.normal(size=(n, q)), rng.normal(size=n)
    t = _capi.new_table(4, V, R, dead=False)
    t["u"][:] = rng.normal(size=(4, R, V)) * 0.7
    t["lam"][:, :, 0] = rng.integers(-1, 2, size=(4, R))
    t["tau2"][:, 0, 0] = rng.exponential(size=4) + 0.05
    t["mu"][:, 0, 0] = rng.normal(size=4)
    t["S"][:, :, 0] = rng.exponential(size=(4, q))
    res = api.Results(t, np.zeros(1), np.zeros(1), 1, 3)
    got = api.MarginalLOOPredict(res, X, y, x_transform=False)
    X = api._dense_rows(api._new_rows(X, False, q, y))                            # (the accessor's own copy of X: the same bits in the same layout)
    ref = api._host_marginal_loo_predict([t], X, y, 1, 3)
    assert got.draws == 3 and got.thin == 1 and got.chains == 1 and got.n_bad == 0 and got.interval == 95 and got.logml.shape == (3,)
    for f in ("loo_mean", "loo_sd", "loo_pit", "loo_lower", "loo_upper", "elpd_loo_i", "pareto_k", "lpd_i"):
        assert np.array_equal(getattr(got, f), getattr(ref, f)), f
    # the pieces by hand: the marginal terms, the PSIS weights, the mixture
    ll, rs, vr, ml, _nb = api._host_marginal_loglik([t], X, y, 1, 3, 1)
    lw, e, k = api._psis_weights_host(ll)
    mean, sd, pit, lo, hi, _w = api._host_weighted_mixture(y[:, None] - rs, vr, lw, y, 0.025, 0.975)
    assert np.array_equal(got.loo_mean, mean) and np.array_equal(got.loo_pit, pit) and np.array_equal(got.loo_upper, hi) and np.array_equal(got.pareto_k, k)
    assert np.all(lo < mean) and np.all(mean < hi) and np.all((pit > 0) & (pit < 1)) and np.all(sd > 0)
    # loo: MarginalLOO's dict from the same arrays; the totals by _loo_predictive's rules
    mloo = api._host_marginal_loo([t], X, y, 1, 3)
    assert set(got.loo) == set(mloo) and np.array_equal(got.loo["elpd_loo_i"], mloo["elpd_loo_i"]) and got.loo["elpd_loo"] == mloo["elpd_loo"]
    assert np.allclose(got.loo["loo_mean"], mloo["loo_mean"], rtol=1e-13, atol=1e-14) and got.loo["draws"] == 3
    assert got.coverage == float(np.mean((y >= lo) & (y <= hi))) and got.ks == api._ks_uniform(pit)
    assert got.rmse_loo == float(math.sqrt(np.mean((y - mean) ** 2)))
    wide = api.MarginalLOOPredict(res, X, y, x_transform=False, interval=50)
    assert wide.interval == 50 and np.all(wide.loo_lower > got.loo_lower) and np.all(wide.loo_upper < got.loo_upper)
    assert np.array_equal(wide.loo_pit, got.loo_pit)
