"""CPU tests of the pooled-chain statistics, the predictive interval of a new observation and the PIT (additions to the reference): the ABI
and the exports, the host mirror of the predictive noise, the host restatements against closed forms, the pooling identity, and the argument
checks that need no GPU.

Closed forms.  Tables with gamma = 0, mu_s ~ N(a, b^2) i.i.d. and tau2 = c^2 make every eta_is = mu_s, and a new observation
y~_is = mu_s + c z_is ~ N(a, b^2 + c^2) i.i.d. over the S pooled draws of a row.  The k-th of S order statistics of such a sample estimates the
quantile x_p, p = k / S, with standard error SE = sqrt(p (1 - p) / S) / f(x_p) (f the density); the tests allow 5 SE (about 6e-7 per quantile
under the null).  The PIT of y = a is the mean over s of Phi((a - mu_s) / c) = Phi(-(b / c) Z): mean 1/2, variance
arcsin(k^2 / (1 + k^2)) / (2 pi) with k = b / c (E Phi(k Z)^2 = 1/4 + arcsin(k^2 / (1 + k^2)) / (2 pi)); the test allows 3 sqrt(Var / S)."""
import ctypes as C
import dataclasses
import math
import os
import re

import numpy as np
import pytest
from scipy import stats

import bnr_amd
from bnr_amd import _capi, api
from bnr_amd.api import Results

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("bnr_chains_summary", "bnr_chains_predict", "bnr_chains_predict_from_matrices", "bnr_chains_loglik_stats", "bnr_chains_loo",
               "bnr_host_pred_noise")
A, B, CC = 3.0, 0.8, 1.3          # mu_s ~ N(A, B^2), tau2 = CC^2


def test_abi_and_exports():
    hdr = open(os.path.join(ROOT, "include", "bnr_hip.h"), encoding="utf-8").read()
    v = int(re.search(r"#define BNR_ABI_VERSION (\d+)", hdr).group(1))
    assert v >= 10 and _capi.lib().bnr_abi_version() == v
    jl = open(os.path.join(ROOT, "julia", "BNRHip.jl"), encoding="utf-8").read()
    for sym in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % sym, hdr), sym
        assert sym in bnr_amd.EXPORTS and hasattr(_capi.lib(), sym), sym
        assert re.search(r"ccall\(\(:%s, LIB\)" % sym, jl), sym
    for fn in ("pooled_summary_stats", "pooled_predict_stats", "pooled_loglik_stats", "pooled_loo_stats"):
        assert re.search(r"^function %s\(" % fn, jl, flags=re.M), fn


def test_noise_mirror_equals_host_normal_and_is_standard_normal():
    L = _capi.lib()
    seed, s0, ns, i0, ni = 0x1234567890ABCDEF, 7, 11, 3, 5
    z = _capi.host_pred_noise(seed, s0, ns, i0, ni)
    assert z.shape == (ni, ns)
    for i in range(ni):
        for s in range(ns):
            assert z[i, s] == L.bnr_host_normal(C.c_uint64(seed), s0 + s, 40, i0 + i, 0), (i, s)
    # rows and draws are different counters: the block is not symmetric, and another seed gives another block
    assert not np.array_equal(_capi.host_pred_noise(seed, 3, 5, 3, 5), _capi.host_pred_noise(seed, 3, 5, 3, 5).T)
    assert not np.array_equal(z, _capi.host_pred_noise(seed + 1, s0, ns, i0, ni))
    big = _capi.host_pred_noise(2024, 0, 1000, 0, 100).reshape(-1)
    assert big.size == 100000
    p = stats.kstest(big, "norm").pvalue
    print("KS p of 1e5 noise values against N(0, 1): %.4f" % p)
    assert p > 1e-3, p


def hand_tables(nchains=3, rows=4000, V=4, seed=11):
    """tables whose gamma is identically 0: eta_s = mu_s ~ N(A, B^2), tau2 = CC^2"""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(nchains):
        st = _capi.new_table(rows, V, 2)
        st["mu"][:, 0, 0] = A + B * rng.standard_normal(rows)
        st["tau2"][:, 0, 0] = CC * CC
        out.append(st)
    return out, V * (V + 1) // 2


def test_closed_form_predictive_quantiles():
    tables, q = hand_tables()
    S = 3 * 4000
    X = np.random.default_rng(5).standard_normal((8, q))
    sd = math.sqrt(B * B + CC * CC)
    for interval in (90, 95):
        p = api._host_pooled_predict(tables, X, None, 0, 4000, interval=interval, pred_seed=99)
        assert p.draws == S and p.pit is None and p.lpd is None
        k_lo, k_hi = api._summary_ranks(S, interval)
        for k, got in ((k_lo, p.pred_lower_bound), (k_hi, p.pred_upper_bound)):
            pr = k / S
            xp = stats.norm.ppf(pr, loc=A, scale=sd)
            se = math.sqrt(pr * (1 - pr) / S) / stats.norm.pdf(xp, loc=A, scale=sd)
            print("interval %d rank %d: quantile %.5f, worst deviation %.2f SE" % (interval, k, xp, np.max(np.abs(got - xp)) / se))
            assert np.all(np.abs(got - xp) <= 5 * se), (interval, k, np.max(np.abs(got - xp)) / se)
        # eta itself is mu_s for every row: its order statistics are those of the pooled mu
        mu = np.sort(np.concatenate([t["mu"][:, 0, 0] for t in tables]))
        assert np.all(p.lower_bound == mu[k_lo - 1]) and np.all(p.upper_bound == mu[k_hi - 1])
        # the predictive interval contains the credible interval of the mean
        assert np.all(p.pred_lower_bound < p.lower_bound) and np.all(p.pred_upper_bound > p.upper_bound)


def test_closed_form_pit():
    tables, q = hand_tables()
    S = 3 * 4000
    rng = np.random.default_rng(6)
    m = 2000
    X = rng.standard_normal((m, q))
    y = A + math.sqrt(B * B + CC * CC) * rng.standard_normal(m)
    pit = api._host_pooled_predict(tables, X, y, 0, 4000, pred_seed=1).pit
    assert pit.shape == (m,) and np.all((pit > 0) & (pit < 1))
    pv = stats.kstest(pit, "uniform").pvalue
    print("KS p of %d PITs against U(0, 1): %.4f" % (m, pv))
    assert pv > 1e-3, pv
    k = B / CC
    var_phi = math.asin(k * k / (1 + k * k)) / (2 * math.pi)
    mid = api._host_pooled_predict(tables, X[:3], np.full(3, A), 0, 4000, pred_seed=1).pit
    print("PIT of y = a: %.6f, allowed %.6f" % (mid[0], 3 * math.sqrt(var_phi / S)))
    assert np.all(np.abs(mid - 0.5) <= 3 * math.sqrt(var_phi / S)), mid
    # the pointwise restatement of the training rows carries the same PIT
    assert np.array_equal(api._host_pooled_pointwise(tables, X, y, 0, 4000)[2], pit)


def random_tables(nchains, rows, V, seed):
    rng = np.random.default_rng(seed)
    q = V * (V + 1) // 2
    out = []
    for _ in range(nchains):
        st = _capi.new_table(rows, V, 2)
        st["gamma"][:, :, 0] = 0.3 * rng.standard_normal((rows, q))
        st["xi"][:, :, 0] = rng.random((rows, V)) < 0.4
        st["mu"][:, 0, 0] = 1.0 + rng.standard_normal(rows)
        st["tau2"][:, 0, 0] = 0.5 + rng.random(rows)
        out.append(st)
    return out, q


def test_pooling_identity():
    nb, ns, V = 7, 120, 5
    tables, q = random_tables(3, nb + ns, V, seed=21)
    rng = np.random.default_rng(22)
    X = rng.standard_normal((9, q))
    y = 1.0 + rng.standard_normal(9)
    # the row-concatenated table of the three windows, built here
    cat = {k: np.asfortranarray(np.concatenate([t[k][nb:nb + ns] for t in tables], axis=0)) for k in tables[0]}
    S = 3 * ns
    res = Results(cat, np.ones(V), np.ones(q), 0, S)
    single = bnr_amd.Predict(res, X, y, interval=90, x_transform=False)
    pooled = api._host_pooled_predict(tables, X, y, nb, ns, interval=90)
    for f in ("estimate", "lower_bound", "upper_bound", "lpd"):
        assert np.array_equal(getattr(single, f), getattr(pooled, f)), f
    assert pooled.elpd == single.elpd and pooled.draws == S and pooled.pred_lower_bound is None and pooled.pit is None
    w1, w2 = bnr_amd.WAIC(res, X, y, x_transform=False), api._host_pooled_waic(tables, X, y, nb, ns)
    l1, l2 = bnr_amd.LOO(res, X, y, x_transform=False), api._host_pooled_loo(tables, X, y, nb, ns)
    for a, b in ((w1, w2), (l1, l2)):
        assert a.keys() == b.keys()
        for k in a:
            assert np.array_equal(a[k], b[k]), k
    assert l2["khat_threshold"] == min(1 - 1 / math.log10(S), 0.7)
    sm = api._host_pooled_summary(tables, nb, ns, 90)
    g = cat["gamma"][:, :, 0]
    lw, hi = api._summary_ranks(S, 90)
    assert np.array_equal(sm["estimate"], g.mean(axis=0)) and np.array_equal(sm["probability"], cat["xi"][:, :, 0].mean(axis=0))
    assert np.array_equal(sm["lower_bound"], np.sort(g, axis=0)[lw - 1]) and np.array_equal(sm["upper_bound"], np.sort(g, axis=0)[hi - 1])
    # the predictive draws of the pooled tables are those of the concatenated table: draw c nsamp + s is chain c's s-th window row
    pp = api._host_pooled_predict(tables, X, y, nb, ns, interval=90, pred_seed=5)
    eta = api._host_eta(cat, X, 0, S)
    yt = np.sort(eta + np.sqrt(cat["tau2"][:, 0, 0])[None, :] * _capi.host_pred_noise(5, 0, S, 0, 9), axis=1)
    assert np.array_equal(pp.pred_lower_bound, yt[:, lw - 1]) and np.array_equal(pp.pred_upper_bound, yt[:, hi - 1])
    assert np.array_equal(pp.pit, api._host_pit(eta, cat["tau2"][:, 0, 0], y))
    # one table: today's host results, exactly
    one = Results(tables[0], np.ones(V), np.ones(q), nb, ns)
    s1 = bnr_amd.Predict(one, X, y, interval=90, x_transform=False)
    p1 = api._host_pooled_predict(tables[:1], X, y, nb, ns, interval=90)
    for f in ("estimate", "lower_bound", "upper_bound", "lpd"):
        assert np.array_equal(getattr(s1, f), getattr(p1, f)), f
    for a, b in ((bnr_amd.WAIC(one, X, y, x_transform=False), api._host_pooled_waic(tables[:1], X, y, nb, ns)),
                 (bnr_amd.LOO(one, X, y, x_transform=False), api._host_pooled_loo(tables[:1], X, y, nb, ns))):
        for k in a:
            assert np.array_equal(a[k], b[k]), k
    # Predict(results) hands the new fields of a carried prediction through
    carried = dataclasses.replace(one, prediction=pp)
    back = bnr_amd.Predict(carried, interval=90)
    assert np.array_equal(back.pred_lower_bound, pp.pred_lower_bound) and np.array_equal(back.pit, pp.pit) and back.draws == S


def test_null_chains_and_nchains_below_one_are_bad_arguments():
    L = _capi.lib()
    d = [np.zeros(8) for _ in range(8)]
    p = [_capi._ptr(a) for a in d]
    one_null = (C.c_void_p * 1)(None)
    X = np.zeros((2, 10), order="F")
    mats = (C.c_void_p * 2)(None, None)
    for arr, n in ((None, 1), (one_null, 0), (one_null, -3), (one_null, 1)):       # NULL array; nchains < 1; a NULL member
        assert L.bnr_chains_summary(arr, n, 1, 4, 1, 4, *p[:4]) == _capi.BNR_ERR_BAD_ARG
        assert L.bnr_chains_predict(arr, n, 1, 4, 2, _capi._ptr(X), 0, None, 1, 4, *p[:3], None, None, 7, None, None, None) == _capi.BNR_ERR_BAD_ARG
        assert L.bnr_chains_predict_from_matrices(arr, n, 1, 4, 2, mats, 0, None, 1, 4, *p[:3], None, None, 7, None, None, None) == _capi.BNR_ERR_BAD_ARG
        assert L.bnr_chains_loglik_stats(arr, n, 1, 4, p[0], p[1], None) == _capi.BNR_ERR_BAD_ARG
        assert L.bnr_chains_loo(arr, n, 1, 4, None, p[0], p[1], p[2]) == _capi.BNR_ERR_BAD_ARG
    assert L.bnr_chains_summary(one_null, 0, 1, 4, 1, 4, *p[:4]) == _capi.BNR_ERR_BAD_ARG and b"nchains" in L.bnr_last_error()
    # only one of pred_lower / pred_upper, and a PIT without y: refused before the chains are looked at
    assert L.bnr_chains_predict(one_null, 1, 1, 4, 2, _capi._ptr(X), 0, None, 1, 4, *p[:3], None, None, 7, p[3], None, None) == _capi.BNR_ERR_BAD_ARG
    assert L.bnr_chains_predict(one_null, 1, 1, 4, 2, _capi._ptr(X), 0, None, 1, 4, *p[:3], None, None, 7, None, None, p[3]) == _capi.BNR_ERR_BAD_ARG
    with pytest.raises(ValueError, match="at least one chain"):
        _capi.pooled_summary([], 1, 4, 1, 4)
    with pytest.raises(ValueError, match="at least one chain"):
        bnr_amd.device_predict_pooled([], 0, 4, X)


def test_fit_refuses_bad_pooled_requests_before_sampling(monkeypatch):
    Xt, yt, _ = bnr_amd.make_synthetic(8, 4, 2, seed=1)
    kw = dict(nburn=2, x_transform=False, suppress_timer=True)
    with pytest.raises(ValueError, match="predict_observation needs predict_X"):
        bnr_amd.Fit(Xt, yt, 2, nsamples=2, filename=None, predict_observation=True, **kw)
    with pytest.raises(ValueError, match="predict_observation needs predict_X"):
        bnr_amd.generate_samples(Xt, yt, 2, nsamp=2, predict_observation=True, **kw)
    with pytest.raises(ValueError, match="predict_observation needs predict_X"):
        bnr_amd.generate_samples_dbl(Xt, yt, 2, mingen=4, maxgen=8, x_transform=False, suppress_timer=True, predict_observation=True)

    class TwoRanks:                                     # what api._dist() hands out under an initialised two-rank process group
        @staticmethod
        def get_rank():
            return 0

        @staticmethod
        def get_world_size():
            return 2

        @staticmethod
        def broadcast(*a, **k):
            raise AssertionError("pool_chains must be refused before anything is exchanged")

        broadcast_object_list = all_gather = broadcast

    monkeypatch.setattr(api, "_dist", lambda: TwoRanks)
    with pytest.raises(ValueError, match="pool_chains"):
        bnr_amd.Fit(Xt, yt, 2, nsamples=2, filename=None, pool_chains=True, seed=3, **kw)
    with pytest.raises(ValueError, match="pool_chains"):
        bnr_amd.generate_samples(Xt, yt, 2, nsamp=2, pool_chains=True, seed=3, **kw)
    with pytest.raises(ValueError, match="pool_chains"):
        bnr_amd.generate_samples_dbl(Xt, yt, 2, mingen=4, maxgen=8, x_transform=False, suppress_timer=True, pool_chains=True, seed=3)


def test_new_keywords_default_to_off():
    import inspect
    for fn in (bnr_amd.Fit, bnr_amd.generate_samples, bnr_amd.generate_samples_dbl):
        p = inspect.signature(fn).parameters
        assert p["pool_chains"].default is False and p["predict_observation"].default is False and p["pred_seed"].default is None
    f = {x.name: x.default for x in dataclasses.fields(bnr_amd.BNRPrediction)}
    assert f["pred_lower_bound"] is None and f["pred_upper_bound"] is None and f["pit"] is None and f["draws"] is None
    assert {x.name: x.default for x in dataclasses.fields(Results)}["stat_chains"] is None
