"""CPU tests of Predict / WAIC (posterior prediction, an addition to the reference): the host path against closed forms, the argument
checks that run before any GPU call, and the Julia shim's prediction ccalls."""
import math
import os
import re

import numpy as np
import pytest

import bnr_amd
from bnr_amd import _capi
from bnr_amd.api import Results

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def hand_state(V=4, nburn=5, nsamp=40, seed=3):
    """a table whose gamma is identically 0: eta_s = mu_s for every row, known mu_s and tau2_s"""
    rng = np.random.default_rng(seed)
    q, tot = V * (V + 1) // 2, nburn + nsamp
    st = _capi.new_table(tot, V, 2)
    st["mu"][:, 0, 0] = 3.0 + rng.standard_normal(tot)
    st["tau2"][:, 0, 0] = 0.5 + rng.random(tot)
    return Results(st, np.ones(V), np.ones(q), nburn, nsamp), q


def test_closed_form_with_zero_gamma():
    res, q = hand_state()
    nb, ns = res.burn_in, res.sampled
    mu = res.state["mu"][nb:nb + ns, 0, 0]
    tau2 = res.state["tau2"][nb:nb + ns, 0, 0]
    rng = np.random.default_rng(5)
    X = rng.standard_normal((7, q))
    y = rng.standard_normal(7) + 3.0
    p = bnr_amd.Predict(res, X, y, interval=90, x_transform=False)
    k_lo, k_hi = int(round(ns * 0.05)), int(round(ns * 0.95))
    srt = np.sort(mu)
    assert p.ci_level == 90
    assert np.allclose(p.estimate, mu.mean(), rtol=0, atol=1e-14)
    assert np.all(p.lower_bound == srt[k_lo - 1]) and np.all(p.upper_bound == srt[k_hi - 1])
    for i in range(7):
        ell = [-0.5 * math.log(2 * math.pi * t) - (y[i] - m) ** 2 / (2 * t) for m, t in zip(mu, tau2)]
        ref = math.log(sum(math.exp(v) for v in ell) / ns)
        assert p.lpd[i] == pytest.approx(ref, rel=1e-12)
    assert p.elpd == pytest.approx(sum(p.lpd), rel=1e-15)
    w = bnr_amd.WAIC(res, X, y, x_transform=False)
    assert w["waic"] == pytest.approx(-2 * (np.sum(w["lpd_i"]) - np.sum(w["p_waic_i"])), rel=1e-14)
    assert w["p_waic"] >= 0 and np.all(w["p_waic_i"] >= 0)
    assert np.allclose(w["lpd_i"], p.lpd, rtol=1e-14, atol=0)
    e = w["lpd_i"] - w["p_waic_i"]
    assert w["se"] == pytest.approx(math.sqrt(len(e) * np.var(e)), rel=1e-14)


def test_input_formats_agree_on_the_host():
    res, q = hand_state(V=4)
    res.state["gamma"][:, :, 0] = np.random.default_rng(2).standard_normal((res.state["gamma"].shape[0], q))
    Xb = np.random.default_rng(4).random((6, q)) < 0.5
    mats = [bnr_amd.create_lower_tri(Xb[i], 4) for i in range(6)]
    a = bnr_amd.Predict(res, Xb.astype(float), x_transform=False)
    b = bnr_amd.Predict(res, mats, x_transform=True)
    assert np.array_equal(a.estimate, b.estimate) and np.array_equal(a.upper_bound, b.upper_bound)
    assert a.lpd is None and a.elpd is None
    r = bnr_amd.Predict(res, Xb.astype(float), x_transform=False, digits=2)
    assert np.array_equal(r.estimate, np.round(a.estimate, 2))


def test_argument_errors():
    res, q = hand_state()
    X = np.zeros((3, q))
    with pytest.raises(ValueError, match="edge columns"):
        bnr_amd.Predict(res, np.zeros((3, 15)), x_transform=False)           # V = 5 against the fit's V = 4
    with pytest.raises(ValueError, match="one entry per new row"):
        bnr_amd.Predict(res, X, np.zeros(4), x_transform=False)
    with pytest.raises(IndexError):
        bnr_amd.Predict(res, X, interval=99, x_transform=False)              # round(40 * 0.005) = 0
    bare = Results(None, res.rhatxi, res.rhatgamma, res.burn_in, res.sampled)
    with pytest.raises(ValueError, match="return_state=True"):
        bnr_amd.Predict(bare, X, x_transform=False)
    with pytest.raises(ValueError, match="predict_X"):
        bnr_amd.Predict(bare)
    with pytest.raises(ValueError, match="waic=True"):
        bnr_amd.WAIC(bare)
    # the low-level call checks q and y before it reaches the library (no handle, no GPU here)
    ch = _capi.Chain.__new__(_capi.Chain)
    ch.n, ch.q, ch.V, ch.R, ch.h, ch.L = 10, q, 4, 2, None, None
    with pytest.raises(ValueError):
        ch.predict(np.zeros((3, 15)), 1, 10, 1, 10)
    with pytest.raises(ValueError):
        ch.predict(X, 1, 10, 1, 10, y=np.zeros(2))
    # Fit refuses bad prediction inputs before it creates a chain
    Xt, yt, _ = bnr_amd.make_synthetic(8, 4, 2, seed=1)
    with pytest.raises(ValueError, match="edge columns"):
        bnr_amd.Fit(Xt, yt, 2, nburn=2, nsamples=2, x_transform=False, filename=None, suppress_timer=True, predict_X=np.zeros((2, 15)))
    with pytest.raises(ValueError, match="one entry per new row"):
        bnr_amd.Fit(Xt, yt, 2, nburn=2, nsamples=2, x_transform=False, filename=None, suppress_timer=True, predict_X=Xt[:2], predict_y=[1.0])
    with pytest.raises(ValueError, match="predict_y needs predict_X"):
        bnr_amd.generate_samples(Xt, yt, 2, nburn=2, nsamp=2, x_transform=False, suppress_timer=True, predict_y=[1.0])


def test_julia_shim_predicts_through_the_new_symbols():
    src = open(os.path.join(ROOT, "julia", "BNRHip.jl"), encoding="utf-8").read()
    for fn in ("predict_stats", "loglik_stats"):
        assert re.search(r"^function %s\(" % fn, src, flags=re.M), fn
    for sym in ("bnr_chain_predict", "bnr_chain_predict_from_matrices", "bnr_chain_loglik_stats"):
        assert re.search(r"ccall\(\(:%s, LIB\)" % sym, src), sym
        assert sym in bnr_amd.EXPORTS
    hdr = open(os.path.join(ROOT, "include", "bnr_hip.h"), encoding="utf-8").read()
    v = int(re.search(r"#define BNR_ABI_VERSION (\d+)", hdr).group(1))
    assert v >= 8 and _capi.lib().bnr_abi_version() == v
