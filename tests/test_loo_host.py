"""CPU tests of PSIS-LOO (an addition to the reference): the product's numpy restatement against a loop-by-loop transcription of loo 2.x
(gpdfit, lx, qgpd, psis_smooth_tail, do_psis_i) kept here, recovery of a known generalized Pareto shape, the edge cases, the totals, the
argument checks that run before any GPU call, the ABI version, the Julia shim's ccall and the place of k_psis in the code object."""
import math
import os
import re

import numpy as np
import pytest

import bnr_amd
import code_objects as co
from bnr_amd import _capi
from bnr_amd.api import Results, _gpdfit, _loo_from_pointwise, _psis_host, _tail_length

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = np.finfo(np.float64).eps


# ---------------------------------------------------------------- loo 2.x, transcribed statement by statement (scalar loops, no vector ops)
def ref_lx(a, x):
    a = [-t for t in a]
    out = []
    for ai in a:
        k = sum(np.log1p(ai * xi) for xi in x) / len(x)
        out.append(np.log(ai / k) - k - 1)
    return out


def ref_gpdfit(x):
    with np.errstate(all="ignore"):                    # R's arithmetic: x / 0 is inf, log of a negative is NaN
        return _ref_gpdfit([np.float64(v) for v in x])


def _ref_gpdfit(x):
    N = len(x)
    prior = 3.0
    M = 30 + math.floor(math.sqrt(N))
    xstar = x[math.floor(N / 4 + 0.5) - 1]
    theta = [1 / x[N - 1] + (1 - np.sqrt(M / (j - 0.5))) / prior / xstar for j in range(1, M + 1)]
    l_theta = [N * v for v in ref_lx(theta, x)]
    imax = max(range(M), key=lambda j: (l_theta[j], -j))
    lse = l_theta[imax] + np.log1p(sum(np.exp(l_theta[j] - l_theta[imax]) for j in range(M) if j != imax))
    w_theta = [np.exp(v - lse) for v in l_theta]
    theta_hat = sum(t * w for t, w in zip(theta, w_theta))
    k = sum(np.log1p(-theta_hat * xi) for xi in x) / N
    sigma = -k / theta_hat
    a = 10
    k = k * N / (N + a) + a * 0.5 / (N + a)
    if np.isnan(k):
        k = np.inf
    return k, sigma


def ref_qgpd(p, k, sigma):
    if np.isnan(sigma) or sigma <= 0:
        return [np.nan] * len(p)
    return [sigma * np.expm1(-k * np.log1p(-pi)) / k for pi in p]


def ref_psis_smooth_tail(x, cutoff):
    n = len(x)
    exp_cutoff = math.exp(cutoff)
    k, sigma = ref_gpdfit([math.exp(v) - exp_cutoff for v in x])
    if np.isfinite(k):
        p = [(j - 0.5) / n for j in range(1, n + 1)]
        return [np.log(q + exp_cutoff) for q in ref_qgpd(p, k, sigma)], k
    return list(x), k


def ref_do_psis_i(log_ratios, tail_len):
    S = len(log_ratios)
    mx = max(log_ratios)
    lw = [r - mx for r in log_ratios]
    khat = np.inf
    if tail_len >= 5:
        ix = sorted(range(S), key=lambda s: lw[s])
        tail_ids = ix[S - tail_len:]
        lw_tail = [lw[s] for s in tail_ids]
        if not abs(max(lw_tail) - min(lw_tail)) < EPS / 100:
            smoothed, khat = ref_psis_smooth_tail(lw_tail, lw[ix[S - tail_len - 1]])
            for s, v in zip(tail_ids, smoothed):
                lw[s] = v
    lw = [0.0 if v > 0 else v for v in lw]
    return lw, khat


def ref_lse(v):
    m = max(v)
    return m + math.log(sum(math.exp(t - m) for t in v))


def ref_loo_row(ll, r_eff=1.0):
    S = len(ll)
    M = math.ceil(min(0.2 * S, 3 * math.sqrt(S / r_eff)))
    lw, k = ref_do_psis_i([-v for v in ll], M)
    lpd = ref_lse(ll) - math.log(S)
    elpd = ref_lse([a + b for a, b in zip(lw, ll)]) - ref_lse(lw)
    return lpd, elpd, k


def gpd_draws(rng, k, sigma, n):
    u = rng.random(n)
    return sigma * ((1 - u) ** (-k) - 1) / k


def loglik_rows(seed):
    """varied rows: normal log densities of several spreads, heavy tails (log of GPD draws as ratios), skewed and short ones"""
    rng = np.random.default_rng(seed)
    rows = []
    for S, scale in ((400, 0.3), (400, 3.0), (1000, 1.0), (150, 10.0)):
        rows.append(-0.5 * (rng.standard_normal(S) * scale) ** 2 - 1.0)
    for k in (0.3, 0.8, 1.3):
        rows.append(-np.log(gpd_draws(rng, k, 1.0, 600)))
    rows.append(np.log(rng.random(300)) * 5)
    rows.append(rng.standard_normal(60))
    return rows


# ---------------------------------------------------------------- the product against the transcription
@pytest.mark.parametrize("seed", [1, 2])
def test_numpy_psis_matches_the_loop_transcription(seed):
    for ll in loglik_rows(seed):
        for r_eff in (1.0, 0.37):
            lpd, elpd, k = _psis_host(ll[None, :], r_eff)
            rl, re_, rk = ref_loo_row(list(ll), r_eff)
            assert lpd[0] == pytest.approx(rl, rel=1e-12, abs=1e-12)
            assert elpd[0] == pytest.approx(re_, rel=1e-12, abs=1e-12), (ll.size, r_eff)
            if math.isinf(rk):
                assert k[0] == rk
            else:
                assert k[0] == pytest.approx(rk, rel=1e-12, abs=1e-12)


def test_gpdfit_matches_the_transcription():
    rng = np.random.default_rng(3)
    for k in (-0.2, 0.3, 0.7, 1.5):
        x = np.sort(gpd_draws(rng, k, 1.5, 300)) if k > 0 else np.sort(rng.random(300))
        got, gs = _gpdfit(x)
        want, ws = ref_gpdfit(list(x))
        assert got == pytest.approx(want, rel=1e-12, abs=1e-13) and gs == pytest.approx(ws, rel=1e-12)


@pytest.mark.parametrize("k", [0.2, 0.5, 0.9])
def test_gpd_shape_is_recovered(k):
    x = np.sort(gpd_draws(np.random.default_rng(11), k, 2.0, 100000))
    khat, sigma = _gpdfit(x)
    assert abs(khat - k) < 0.03, (k, khat)
    assert abs(sigma - 2.0) < 0.1, sigma


# ---------------------------------------------------------------- edge cases
def test_constant_loglik():
    ll = np.full((3, 500), -1.25)
    lpd, elpd, k = _psis_host(ll)
    assert np.all(lpd == -1.25) and np.all(np.abs(elpd - lpd) < 1e-15) and np.all(np.isinf(k))
    d = _loo_from_pointwise(lpd, elpd, k, 500)
    assert np.all(np.abs(d["p_loo_i"]) < 1e-15)


def test_short_windows_use_plain_importance_sampling():
    rng = np.random.default_rng(4)
    for S in (2, 7, 20):                               # M = ceil(0.2 S) < 5
        assert _tail_length(S, 1.0) < 5
        ll = rng.standard_normal(S)
        lpd, elpd, k = _psis_host(ll[None, :])
        lw = -ll - np.max(-ll)                         # raw weights: 1 / p(y | theta_s), truncated at their max (no-op)
        want = math.log(np.sum(np.exp(lw + ll))) - math.log(np.sum(np.exp(lw)))
        assert math.isinf(k[0]) and elpd[0] == pytest.approx(want, rel=1e-13)
        assert elpd[0] == pytest.approx(-math.log(np.mean(np.exp(-ll))), rel=1e-12)   # the harmonic mean of p(y | theta_s)
    assert _tail_length(21, 1.0) == 5


def test_one_draw():
    lpd, elpd, k = _psis_host(np.array([[-3.5], [2.0]]))
    assert np.array_equal(elpd, [-3.5, 2.0]) and np.array_equal(lpd, [-3.5, 2.0]) and np.all(np.isinf(k))
    d = _loo_from_pointwise(lpd, elpd, k, 1)
    assert d["khat_threshold"] == -math.inf and d["n_high_k"] == 2


def test_ties_at_the_cutoff():
    rng = np.random.default_rng(5)
    base = rng.standard_normal(400)
    ll = np.concatenate([base, np.full(60, np.sort(base)[20])])          # 60 copies of a value near the cutoff of the smallest l
    rng.shuffle(ll)
    lpd, elpd, k = _psis_host(ll[None, :])
    rl, re_, rk = ref_loo_row(list(ll))
    assert elpd[0] == pytest.approx(re_, rel=1e-12) and k[0] == pytest.approx(rk, rel=1e-12)
    # which of the tied draws lands in the tail does not matter: any permutation gives the same numbers
    lpd2, elpd2, k2 = _psis_host(ll[::-1][None, :])
    assert elpd2[0] == pytest.approx(elpd[0], rel=1e-13) and k2[0] == pytest.approx(k[0], rel=1e-13)


def test_constant_tail_is_not_smoothed():
    ll = np.concatenate([np.full(100, -5.0), np.linspace(-1.0, 0.0, 400)])   # the 100 smallest l (largest ratios) are equal
    lpd, elpd, k = _psis_host(ll[None, :])
    assert _tail_length(500, 1.0) == 68 and math.isinf(k[0])
    lw = 5.0 - ll - 10.0
    assert elpd[0] == pytest.approx(math.log(np.sum(np.exp(lw + ll))) - math.log(np.sum(np.exp(lw))), rel=1e-13)


def test_non_finite_row():
    ll = np.random.default_rng(6).standard_normal((2, 100))
    ll[1, 17] = np.nan
    lpd, elpd, k = _psis_host(ll)
    assert np.isfinite(elpd[0]) and math.isnan(elpd[1]) and math.isinf(k[1])


def test_totals_threshold_and_high_k_count():
    lpd = np.array([-1.0, -2.0, -1.5, -0.5])
    e = np.array([-1.1, -2.5, -1.6, -0.5])
    k = np.array([0.1, 0.75, np.inf, 0.69])
    d = _loo_from_pointwise(lpd, e, k, 1000)
    assert d["elpd_loo"] == pytest.approx(-5.7, abs=1e-14) and d["looic"] == pytest.approx(11.4, abs=1e-13)
    assert d["p_loo"] == pytest.approx(0.1 + 0.5 + 0.1 + 0.0, abs=1e-14)
    assert np.allclose(d["p_loo_i"], [0.1, 0.5, 0.1, 0.0], atol=1e-15)
    assert d["se"] == pytest.approx(math.sqrt(4 * np.var(e)), rel=1e-14)
    assert d["khat_threshold"] == pytest.approx(1 - 1 / 3, rel=1e-15) and d["n_high_k"] == 3    # min(1 - 1/log10(1000), 0.7)
    assert _loo_from_pointwise(lpd, e, k, 10 ** 8)["khat_threshold"] == 0.7
    assert _loo_from_pointwise(lpd, e, k, 10 ** 8)["n_high_k"] == 2


# ---------------------------------------------------------------- LOO through Results, argument checks
def hand_results(V=4, nburn=5, nsamp=300, seed=3):
    rng = np.random.default_rng(seed)
    q, tot = V * (V + 1) // 2, nburn + nsamp
    st = _capi.new_table(tot, V, 2)
    st["mu"][:, 0, 0] = 3.0 + 0.3 * rng.standard_normal(tot)
    st["tau2"][:, 0, 0] = 0.5 + rng.random(tot)
    st["gamma"][:, :, 0] = 0.1 * rng.standard_normal((tot, q))
    return Results(st, np.ones(V), np.ones(q), nburn, nsamp), q


def test_loo_on_a_fetched_table_matches_the_transcription():
    res, q = hand_results()
    rng = np.random.default_rng(8)
    X = rng.standard_normal((9, q))
    y = 3.0 + rng.standard_normal(9)
    d = bnr_amd.LOO(res, X, y, x_transform=False)
    st, nb, ns = res.state, res.burn_in, res.sampled
    eta = st["mu"][nb:nb + ns, 0, 0][None, :] + X @ st["gamma"][nb:nb + ns, :, 0].T
    tau2 = st["tau2"][nb:nb + ns, 0, 0]
    for i in range(9):
        ll = [-0.5 * math.log(2 * math.pi * t) - (y[i] - m) ** 2 / (2 * t) for m, t in zip(eta[i], tau2)]
        rl, re_, rk = ref_loo_row(ll)
        assert d["lpd_i"][i] == pytest.approx(rl, rel=1e-12) and d["elpd_loo_i"][i] == pytest.approx(re_, rel=1e-12)
        assert d["pareto_k"][i] == pytest.approx(rk, rel=1e-9, abs=1e-9)
    w = bnr_amd.WAIC(res, X, y, x_transform=False)
    assert np.allclose(d["lpd_i"], w["lpd_i"], rtol=1e-14, atol=0)
    assert d["looic"] == pytest.approx(-2 * d["elpd_loo"], rel=1e-15) and d["p_loo"] == pytest.approx(np.sum(d["p_loo_i"]), rel=1e-13)
    # a per-row r_eff changes the tail lengths (and so the numbers) only where it should
    d2 = bnr_amd.LOO(res, X, y, x_transform=False, r_eff=np.full(9, 1.0))
    assert np.array_equal(d2["elpd_loo_i"], d["elpd_loo_i"])
    d3 = bnr_amd.LOO(res, X, y, x_transform=False, r_eff=0.2)
    assert not np.array_equal(d3["pareto_k"], d["pareto_k"])


def test_loo_argument_errors():
    res, q = hand_results()
    X, y = np.zeros((3, q)), np.zeros(3)
    bare = Results(None, res.rhatxi, res.rhatgamma, res.burn_in, res.sampled)
    with pytest.raises(ValueError, match="loo=True"):
        bnr_amd.LOO(bare)
    with pytest.raises(ValueError, match="loo=True"):
        bnr_amd.LOO(res)                                                       # state but no X, y
    with pytest.raises(ValueError, match="edge columns"):
        bnr_amd.LOO(res, np.zeros((3, 15)), y, x_transform=False)
    with pytest.raises(ValueError, match="one entry per new row"):
        bnr_amd.LOO(res, X, np.zeros(4), x_transform=False)
    for bad in (0.0, -1.0, np.inf, np.nan, np.ones(4), [1.0, 0.0, 1.0]):
        with pytest.raises(ValueError, match="r_eff"):
            bnr_amd.LOO(res, X, y, x_transform=False, r_eff=bad)
    with pytest.raises(ValueError, match="m x S"):
        bnr_amd.psis_loo(np.zeros(5))
    with pytest.raises(ValueError, match="r_eff"):
        bnr_amd.psis_loo(np.zeros((2, 5)), r_eff=[1.0])
    # the low-level call checks r_eff before it reaches the library (no handle, no GPU here)
    ch = _capi.Chain.__new__(_capi.Chain)
    ch.n, ch.q, ch.V, ch.R, ch.h, ch.L = 10, q, 4, 2, None, None
    with pytest.raises(ValueError, match="r_eff"):
        ch.loo(1, 10, r_eff=np.ones(3))
    # Fit refuses a bad loo_r_eff before it creates a chain
    Xt, yt, _ = bnr_amd.make_synthetic(8, 4, 2, seed=1)
    with pytest.raises(ValueError, match="r_eff"):
        bnr_amd.Fit(Xt, yt, 2, nburn=2, nsamples=2, x_transform=False, filename=None, suppress_timer=True, loo=True, loo_r_eff=-1.0)
    with pytest.raises(ValueError, match="r_eff"):
        bnr_amd.generate_samples_dbl(Xt, yt, 2, mingen=4, maxgen=8, x_transform=False, suppress_timer=True, loo=True, loo_r_eff=np.ones(3))


def test_library_refuses_bad_psis_arguments_before_touching_a_device():
    """bnr_psis_loo checks its arguments (NULLs, sizes, r_eff, the tail limit) before any HIP call"""
    L = _capi.lib()
    ll = np.zeros((2, 50))
    out = [np.empty(2) for _ in range(3)]
    p = [_capi._ptr(o) for o in out]
    assert L.bnr_psis_loo(0, 2, 50, None, None, p[0], p[1], p[2]) == _capi.BNR_ERR_BAD_ARG
    assert L.bnr_psis_loo(0, 0, 50, _capi._ptr(ll), None, p[0], p[1], p[2]) == _capi.BNR_ERR_BAD_ARG
    assert L.bnr_psis_loo(0, 2, 0, _capi._ptr(ll), None, p[0], p[1], p[2]) == _capi.BNR_ERR_BAD_ARG
    assert L.bnr_psis_loo(0, 2, 50, _capi._ptr(ll), _capi._ptr(np.array([1.0, -2.0])), p[0], p[1], p[2]) == _capi.BNR_ERR_BAD_ARG
    assert "r_eff" in L.bnr_last_error().decode()
    big = np.zeros((1, 50000))
    r = np.array([0.001])                                                       # M = ceil(min(10000, 3 sqrt(5e7))) = 10000 > 8192
    assert L.bnr_psis_loo(0, 1, 50000, _capi._ptr(big), _capi._ptr(r), p[0], p[1], p[2]) == _capi.BNR_ERR_BAD_ARG
    assert "8192" in L.bnr_last_error().decode()


# ---------------------------------------------------------------- ABI, shim, code object
def test_abi_version_and_exports():
    hdr = open(os.path.join(ROOT, "include", "bnr_hip.h"), encoding="utf-8").read()
    v = int(re.search(r"#define BNR_ABI_VERSION (\d+)", hdr).group(1))
    assert v >= 9 and _capi.lib().bnr_abi_version() == v
    for sym in ("bnr_chain_loo", "bnr_psis_loo"):
        assert sym in bnr_amd.EXPORTS and re.search(r"\bint %s\(" % sym, hdr)


def test_julia_shim_computes_loo_through_the_new_symbol():
    src = open(os.path.join(ROOT, "julia", "BNRHip.jl"), encoding="utf-8").read()
    assert re.search(r"^function loo_stats\(ch::Chain, nburn, nsamp; r_eff=nothing\)", src, flags=re.M)
    assert re.search(r"ccall\(\(:bnr_chain_loo, LIB\)", src)


def test_psis_kernels_sit_outside_the_code_object_of_the_sweep(tmp_path):
    """k_psis is compiled in csrc/bnr_analysis.hip: both of its instantiations are in the analysis code object and not in the sweep's"""
    assert co.have_tools() and os.path.exists(co.LIB)
    sweep, analysis = co.sweep_and_analysis(tmp_path)
    psis = [k for k in analysis if k.startswith("k_psis<")]
    assert len(psis) == 2 and set(psis) <= co.ANALYSIS, sorted(analysis)
    assert not [k for k in sweep if k.startswith("k_psis")]
