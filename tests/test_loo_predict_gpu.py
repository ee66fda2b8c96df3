"""GPU tests of the LOO predictive checks (ABI 11; run with -m gpu on an MI355X): bnr_chains_loo_predict / bnr_chain_loo_predict against the host
restatement over the fetched tables of a 3-chain lockstep group and of a lone chain, consistency with bnr_chains_loo and
bnr_chains_loglik_stats on the same window, the bitwise equalities (block sizes, repeated calls, one chain through the pooled entry point, the
outputs requested), no side effects on any member, bnr_psis_weights on crafted matrices, Fit(..., loo_predict=True), the 8-chain headline group.

Bounds.  lpd, elpd_loo, k-hat: test_loo_gpu.close's.  For the rest the device is compared with the HOST restatement (never with itself); a bound
is an eta part, derived, plus 4 x the gap measured on these fixtures (the rule of test_pooled_gpu.py for K_Z and the PIT), the measured values
below and in DESIGN.md section 8.  With B_is = test_predict_gpu.eta_bound and r_is = |y_i - eta_is|:
  log weights  |lw_dev - lw_host| <= 4 max_s(r_is B_is / tau2_s) + 4 KLW_MEASURED: l_is moves by r B / tau2 with eta, and lw_is = -l_is - max_s(-l_is)
               - log Z_i carries the moves of three such terms (4 covers them); the measured part is the different order of the sums of the fit
               and the normaliser, in log units.
  loo_mean     <= max_s B_is + 4 KMEAN_MEASURED max_s |eta_is|                 (a weighted mean of eta; the measured part is relative to the row's largest |eta|)
  loo_sd       <= 4 KSD_MEASURED loo_sd + (max_s B_is) (1 + 2 max_s |eta_is| / loo_sd)   (d sd = d(second moment) / (2 sd), the second moment moves by 2 |eta| B)
  loo_pit      <= 0.3990 max_s B_is / min_s sqrt(tau2_s) + 4 KPIT_MEASURED     (the slope of Phi is at most 1 / sqrt(2 pi) = 0.3990)
  bounds       by residual: with the host's F and weights |F_i(t_dev) - p| <= 0.3990 width_i 2^-40 / min_s sqrt(tau2_s) + the PIT bound above,
               width_i the starting bracket; and |t_dev - t_host| <= 2 width_i 2^-40 + that residual / F_i'(t_host).
Measured on the fixtures of this file (MI355X): K_LW 5.26e-13 (1.23e-12 on the crafted rows with the longest tail), K_MEAN 2.16e-13, K_SD 5.02e-13,
K_PIT 1.06e-13 -- all in the window 1..400, which holds the first sweeps after the prior draw; 2.6e-15 .. 4.8e-14 in the other windows.  The
bounds' residual reached 0.023 of its allowance, |t_dev - t_host| 0.021 of its.  The tests print the gaps on every run."""
import dataclasses
import math

import numpy as np
import pytest

import bnr_amd
from bnr_amd import _capi, api
from bnr_amd.api import _host_eta, _host_loglik, _host_loo_predict, _loo_bracket_c, _loo_predict_rows, _mixture_cdf, _psis_host, _psis_weights_host
from test_loo_gpu import close as loo_close, crafted_rows
from test_predict_gpu import eta_bound

pytestmark = pytest.mark.gpu
SEED = 4717
KLW_MEASURED = 5.3e-13            # largest |lw_dev - lw_host| (log units) of bnr_psis_weights on the host's own l of the trio (measured 5.26e-13)
KLW_CRAFTED_MEASURED = 1.3e-12    # the same on the crafted rows below, tails up to M = 8192 (measured 1.23e-12 at M = 8192, 5.58e-13 at S = 20 000)
KMEAN_MEASURED = 2.2e-13          # largest |loo_mean_dev - loo_mean_host| / max_s |eta_is| (measured 2.16e-13, window 1..400 of the trio)
KSD_MEASURED = 5.1e-13            # largest |loo_sd_dev - loo_sd_host| / loo_sd_host (measured 5.02e-13, the same window)
KPIT_MEASURED = 1.1e-13           # largest |loo_pit_dev - loo_pit_host| (measured 1.06e-13, the same window)
NB, NS = 100, 300
P_LO, P_HI = 0.025, 0.975
T40 = 2.0 ** -40


@pytest.fixture(scope="module")
def trio(gpu):
    """a 3-chain lockstep group, n = 60, V = 12, R = 3, 400-row tables, and one lone chain of the same model"""
    X, y, _ = bnr_amd.make_synthetic(60, 12, 3, seed=SEED)
    chains = [bnr_amd.Chain(X, y, 3, 400, SEED, 1, device=gpu)]
    chains += [bnr_amd.Chain.like(chains[0], SEED, c) for c in (2, 3)]
    grp = bnr_amd.Group(chains)
    for ch in chains:
        ch.init_prior()
    grp.run(2, 400, 400)
    lone = bnr_amd.Chain(X, y, 3, 400, SEED + 1, 1, device=gpu)
    lone.init_prior()
    lone.run(2, 400, 400)
    yield chains, X, y, [ch.fetch() for ch in chains], lone, lone.fetch()
    grp.close()
    for ch in chains + [lone]:
        ch.close()


def host_side(tables, X, y, nb, ns, r_eff, p_lo=P_LO, p_hi=P_HI):
    eta = np.concatenate([_host_eta(t, X, nb, ns) for t in tables], axis=1)
    B = np.concatenate([eta_bound(t, X, nb, ns) for t in tables], axis=1)
    tau2 = np.concatenate([t["tau2"][nb:nb + ns, 0, 0] for t in tables])
    ll = np.concatenate([_host_loglik(t, X, y, nb, ns) for t in tables], axis=1)
    lwn, e, k = _psis_weights_host(ll, r_eff)
    rows = _loo_predict_rows(eta, tau2, y, lwn, p_lo, p_hi)
    return eta, B, tau2, ll, lwn, (_psis_host(ll, r_eff)[0], e, k), rows


def check_against_host(dev, tables, X, y, nb, ns, r_eff, label, p_lo=P_LO, p_hi=P_HI):
    lpd, e, k, mean, sd, pit, lo, hi = dev
    eta, B, tau2, ll, lwn, host3, (hm, hs, hp, hlo, hhi, width) = host_side(tables, X, y, nb, ns, r_eff, p_lo, p_hi)
    loo_close((lpd, e, k), host3)
    Bm, amax, smin = B.max(axis=1), np.abs(eta).max(axis=1), np.sqrt(tau2).min()
    g_mean, g_sd, g_pit = np.abs(mean - hm) / amax, np.abs(sd - hs) / hs, np.abs(pit - hp)
    print("%s: measured K_MEAN %.3g, K_SD %.3g, K_PIT %.3g (eta parts up to %.3g, %.3g, %.3g)"
          % (label, g_mean.max(), g_sd.max(), g_pit.max(), Bm.max(), (Bm * (1 + 2 * amax / hs)).max(), 0.3990 * Bm.max() / smin))
    pit_bound = 0.3990 * Bm / smin + 4 * KPIT_MEASURED
    assert np.all(np.abs(mean - hm) <= Bm + 4 * KMEAN_MEASURED * amax), g_mean.max()
    assert np.all(np.abs(sd - hs) <= 4 * KSD_MEASURED * hs + Bm * (1 + 2 * amax / hs)), g_sd.max()
    assert np.all(g_pit <= pit_bound), g_pit.max()
    assert np.all((pit >= 0) & (pit <= 1)) and np.all(lo < hi) and np.all(sd > 0)
    # the bounds, by residual with the host's F and weights
    sdv = np.sqrt(tau2)
    worst_r = worst_t = 0.0
    for i in range(len(y)):
        w = np.exp(lwn[i])
        resid = 0.3990 * width[i] * T40 / smin + pit_bound[i]
        for t_dev, t_host, p in ((lo[i], hlo[i], p_lo), (hi[i], hhi[i], p_hi)):
            r = abs(_mixture_cdf(t_dev, w, eta[i], sdv) - p)
            z = (t_host - eta[i]) / sdv
            slope = float(np.sum(w * np.exp(-0.5 * z * z) / (math.sqrt(2 * math.pi) * sdv)))
            worst_r, worst_t = max(worst_r, r / resid), max(worst_t, abs(t_dev - t_host) / (2 * width[i] * T40 + resid / slope))
            assert r <= resid, (i, p, r, resid)
            assert abs(t_dev - t_host) <= 2 * width[i] * T40 + resid / slope, (i, p, t_dev, t_host)
    print("%s: bounds: worst residual / bound %.3g, worst |t_dev - t_host| / bound %.3g" % (label, worst_r, worst_t))


def test_pooled_and_lone_loo_predict_match_the_host(trio):
    chains, X, y, tables, lone, lone_table = trio
    for nb, ns, r_eff in ((NB, NS, None), (0, 400, 0.5), (150, 250, np.linspace(0.3, 2.0, 60))):
        dev = _capi.pooled_loo_predict(chains, nb + 1, ns, r_eff, P_LO, P_HI)
        check_against_host(dev, tables, X, y, nb, ns, r_eff, "3 chains, window %d+%d" % (nb, ns))
        one = lone.loo_predict(nb + 1, ns, r_eff, P_LO, P_HI)
        check_against_host(one, [lone_table], X, y, nb, ns, r_eff, "lone chain, window %d+%d" % (nb, ns))
    lp = api.device_loo_predict(chains, y, NB, NS, 95)
    host = _host_loo_predict(tables, X, y, NB, NS, 95)
    assert lp.draws == host.draws == 3 * NS and lp.n_high_k == host.n_high_k and lp.khat_threshold == host.khat_threshold
    assert lp.coverage == host.coverage and lp.rmse_loo == pytest.approx(host.rmse_loo, rel=1e-9) and lp.r2_loo == pytest.approx(host.r2_loo, rel=1e-9)
    assert lp.ks == pytest.approx(host.ks, abs=1e-9)


def test_weights_of_the_hosts_own_loglik_measure_klw(trio, gpu):
    """bnr_psis_weights on the host's l of the trio: no eta part, the gap is the arithmetic of the PSIS alone -> KLW_MEASURED"""
    chains, X, y, tables, _lone, _lt = trio
    worst = 0.0
    for nb, ns, r_eff in ((NB, NS, None), (0, 400, 0.5)):
        ll = np.concatenate([_host_loglik(t, X, y, nb, ns) for t in tables], axis=1)
        lw, e, k = _capi.psis_weights_raw(ll, r_eff, gpu)
        hlw, he, hk = _psis_weights_host(ll, r_eff)
        loo_close((_psis_host(ll, r_eff)[0], e, k), (_psis_host(ll, r_eff)[0], he, hk))
        worst = max(worst, float(np.max(np.abs(lw - hlw))))
        assert np.allclose(np.exp(lw).sum(axis=1), 1.0, rtol=0, atol=1e-12)
    print("K_LW: largest |lw_dev - lw_host| over the trio's own l: %.3g" % worst)
    assert worst <= 4 * KLW_MEASURED, worst


def test_consistent_with_the_old_path(trio):
    chains, _X, _y, _t, lone, _lt = trio
    for nb, ns, r_eff in ((NB, NS, None), (0, 400, 0.5)):
        new = _capi.pooled_loo_predict(chains, nb + 1, ns, r_eff)
        old = _capi.pooled_loo(chains, nb + 1, ns, r_eff)
        loo_close(new[:3], old)
        assert np.array_equal(new[0], _capi.pooled_loglik_stats(chains, nb + 1, ns)[0])          # lpd bit for bit
        assert np.array_equal(new[0], old[0])
        one = lone.loo_predict(nb + 1, ns, r_eff)
        loo_close(one[:3], lone.loo(nb + 1, ns, r_eff))
        assert np.array_equal(one[0], lone.loglik_stats(nb + 1, ns)[0])


def test_bitwise_stability(trio):
    chains, _X, _y, _t, lone, _lt = trio
    base = _capi.pooled_loo_predict(chains, 51, 333, 0.7, 0.05, 0.9)
    base1 = lone.loo_predict(51, 333, 0.7, 0.05, 0.9)
    try:
        for rows in (64, 20, 8, 1, 0):
            chains[0].set_option("predict_block_rows", rows)
            lone.set_option("predict_block_rows", rows)
            for u, v in zip(base, _capi.pooled_loo_predict(chains, 51, 333, 0.7, 0.05, 0.9)):
                assert np.array_equal(u, v), rows
            for u, v in zip(base1, lone.loo_predict(51, 333, 0.7, 0.05, 0.9)):
                assert np.array_equal(u, v), rows
    finally:
        chains[0].set_option("predict_block_rows", 0)
        lone.set_option("predict_block_rows", 0)
    for u, v in zip(base, _capi.pooled_loo_predict(chains, 51, 333, 0.7, 0.05, 0.9)):          # a repeated call
        assert np.array_equal(u, v)
    for ch in (lone, chains[1]):                                                               # one chain through the pooled entry point
        for u, v in zip(ch.loo_predict(51, 333, 0.7, 0.05, 0.9), _capi.pooled_loo_predict([ch], 51, 333, 0.7, 0.05, 0.9)):
            assert np.array_equal(u, v)
    # the outputs requested do not change the others: only the first three (still through the weights kernel), only one bound
    few = _capi.pooled_loo_predict(chains, 51, 333, 0.7, 0.05, 0.9, fields=("lpd", "elpd_loo", "pareto_k"))
    assert all(a is None for a in few[3:]) and all(np.array_equal(u, v) for u, v in zip(few[:3], base[:3]))
    up = _capi.pooled_loo_predict(chains, 51, 333, 0.7, 0.05, 0.9, fields=("loo_upper", "loo_sd"))
    assert np.array_equal(up[7], base[7]) and np.array_equal(up[4], base[4]) and up[6] is None and up[0] is None
    # the bounds move with their probabilities, and only they
    other = _capi.pooled_loo_predict(chains, 51, 333, 0.7, 0.1, 0.9)
    assert np.all(other[6] > base[6]) and np.array_equal(other[7], base[7]) and all(np.array_equal(u, v) for u, v in zip(other[:6], base[:6]))


def test_input_formats_give_bitwise_equal_results(gpu):
    """a 0/1 model matrix as float64, uint8, bool and as adjacency matrices: the formats the pooled tests cover"""
    rng = np.random.default_rng(SEED + 2)
    n, V = 40, 12
    Xb = rng.random((n, 78)) < 0.5
    y = rng.standard_normal(n)
    outs = []
    for Xin, xt in ((Xb.astype(np.float64), False), (Xb.astype(np.uint8), False), (Xb, False),
                    ([bnr_amd.create_lower_tri(Xb[i], V) for i in range(n)], True)):
        chains = [bnr_amd.Chain(_capi.XInput(Xin, xt), y, 3, 120, SEED, 1, device=gpu)]
        chains.append(bnr_amd.Chain.like(chains[0], SEED, 2))
        grp = bnr_amd.Group(chains)
        for ch in chains:
            ch.init_prior()
        grp.run(2, 120, 120)
        outs.append(_capi.pooled_loo_predict(chains, 21, 100))
        grp.close()
        for ch in chains:
            ch.close()
    for other in outs[1:]:
        for u, v in zip(outs[0], other):
            assert np.array_equal(u, v)


def test_no_side_effects_on_any_member(gpu):
    X, y, _ = bnr_amd.make_synthetic(60, 12, 3, seed=SEED + 3)
    k, tot = 40, 80
    groups = []
    for _ in range(2):
        chains = [bnr_amd.Chain(X, y, 3, tot, SEED, 1, device=gpu)]
        chains += [bnr_amd.Chain.like(chains[0], SEED, c) for c in (2, 3)]
        grp = bnr_amd.Group(chains)
        for ch in chains:
            ch.init_prior()
        grp.run(2, tot, k)
        groups.append((grp, chains))
    (ga, a), (gb, b) = groups
    before = [(ch.fetch(), ch.iter, ch.counters()) for ch in a]
    _capi.pooled_loo_predict(a, 2, k - 1)
    _capi.pooled_loo_predict(a, 1, k, 0.5, 0.1, 0.8)
    a[1].loo_predict(1, k)
    for ch, (t0, it0, c0) in zip(a, before):
        t1 = ch.fetch()
        for col in t0:
            assert np.array_equal(t0[col], t1[col]), col
        assert ch.iter == it0 and ch.counters() == c0
    ga.run(k + 1, tot, tot)
    gb.run(k + 1, tot, tot)
    for ca, cb in zip(a, b):
        ta, tb = ca.fetch(), cb.fetch()
        for col in ta:
            assert np.array_equal(ta[col], tb[col]), col
        assert ca.counters() == cb.counters() and ca.iter == cb.iter
    for grp, chains in groups:
        grp.close()
        for ch in chains:
            ch.close()


def refused(call):
    with pytest.raises(bnr_amd.BnrError) as e:
        call()
    assert e.value.code == _capi.BNR_ERR_BAD_ARG, e.value
    return str(e.value)


def test_refusals(trio, gpu):
    chains, X, y, _t, lone, _lt = trio
    assert "twice" in refused(lambda: _capi.pooled_loo_predict([chains[0], chains[1], chains[0]], NB + 1, NS))
    for first, ns in ((0, 10), (350, 60), (1, 0)):
        refused(lambda: _capi.pooled_loo_predict(chains, first, ns))
        refused(lambda: lone.loo_predict(first, ns))
    out = [np.empty(60) for _ in range(8)]
    ptrs = [_capi._ptr(o) for o in out]
    arr = (_capi.C.c_void_p * 3)(*[ch.h for ch in chains])
    L = chains[0].L
    for p_lo, p_hi in ((0.5, 0.5), (0.6, 0.4), (0.0, 0.9), (0.1, 1.0)):                       # (the Python wrapper refuses these itself)
        assert L.bnr_chains_loo_predict(arr, 3, NB + 1, NS, None, p_lo, p_hi, *ptrs) == _capi.BNR_ERR_BAD_ARG
        assert L.bnr_chain_loo_predict(lone.h, NB + 1, NS, None, p_lo, p_hi, *ptrs) == _capi.BNR_ERR_BAD_ARG
        assert L.bnr_chains_loo_predict(arr, 3, NB + 1, NS, None, p_lo, p_hi, *(ptrs[:6] + [None, None])) == _capi.BNR_OK   # no bound requested: not read
    assert L.bnr_chains_loo_predict(arr, 3, NB + 1, NS, _capi._ptr(np.full(60, -1.0)), P_LO, P_HI, *ptrs) == _capi.BNR_ERR_BAD_ARG
    X2, y2, _ = bnr_amd.make_synthetic(60, 10, 3, seed=SEED + 5)
    other = bnr_amd.Chain(X2, y2, 3, 400, SEED, 1, device=gpu)
    busy = bnr_amd.Chain.like(chains[0], SEED, 8, 400)
    try:
        for ch in (other, busy):
            ch.init_prior()
        busy.run(2, 400, 20)
        assert "equal n, V, R" in refused(lambda: _capi.pooled_loo_predict([chains[0], other], NB + 1, NS))
        busy.run_async(21, 400, 24)
        try:
            for cs in ([chains[0], busy], [busy, chains[0]]):
                assert "pending" in refused(lambda: _capi.pooled_loo_predict(cs, 2, 10))
            assert "pending" in refused(lambda: busy.loo_predict(2, 10))
        finally:
            busy.sync()
        _capi.pooled_loo_predict([chains[0], busy], 2, 20)
    finally:
        other.close()
        busy.close()


def weights_close(ll, r_eff, gpu):
    lw, e, k = _capi.psis_weights_raw(ll, r_eff, gpu)
    hlw, he, hk = _psis_weights_host(ll, r_eff)
    lpd = _psis_host(ll, r_eff)[0]
    loo_close((lpd, e, k), (lpd, he, hk))
    fin = np.isfinite(hlw)
    assert np.array_equal(fin, np.isfinite(lw))
    gap = float(np.max(np.abs(lw[fin] - hlw[fin]))) if fin.any() else 0.0
    return lw, e, k, gap


@pytest.mark.parametrize("S", [1, 7, 20, 21, 24, 25, 400, 20000])
def test_psis_weights_on_crafted_rows(gpu, S):
    """test_loo_gpu's crafted rows against the host restatement: 4 x the gap measured on these rows (KLW_CRAFTED_MEASURED); rows without a fit
    (M < 5) to 4 KLW_MEASURED."""
    rng = np.random.default_rng(S)
    ll = crafted_rows(S, rng)
    lw, e, k, gap = weights_close(ll, None, gpu)
    hlw = _psis_weights_host(ll)[0]
    print("S = %d: largest |lw_dev - lw_host| %.3g" % (S, gap))
    assert np.all(np.abs(lw - hlw) <= 4 * KLW_CRAFTED_MEASURED)
    assert np.allclose(np.exp(lw).sum(axis=1), 1.0, rtol=0, atol=1e-11)
    w = np.exp(lw[1])                                                              # the constant row: one number, 1 / S
    assert np.all(w == w[0]) and abs(w[0] * S - 1.0) <= 8 * np.finfo(float).eps
    if S <= 20:                                                                    # M < 5: the raw ratios, no fit
        raw = -ll - np.max(-ll, axis=1, keepdims=True)
        assert np.all(np.isinf(k)) and np.all(np.abs(lw - (raw - np.log(np.sum(np.exp(raw), axis=1, keepdims=True)))) <= 4 * KLW_MEASURED)
    d = bnr_amd.psis_weights(ll, device=gpu)
    assert np.array_equal(d["log_weights"], lw) and np.array_equal(d["pareto_k"], k)
    again = _capi.psis_weights_raw(ll, None, gpu)
    assert all(np.array_equal(u, v) for u, v in zip(again, (lw, e, k)))


def test_psis_weights_ties_nan_row_and_tail_limit(gpu):
    rng = np.random.default_rng(6)
    # the crafted ties of the host test: 17 large ratios, 30 tied at the cutoff, M = 20 -> the 3 tied draws of the largest index join the tail
    S = 100
    ll = rng.standard_normal(S) + 3.0
    big = rng.choice(S, 17, replace=False)
    ll[big] = -5.0 - np.arange(17) * 0.1
    tied = np.sort(rng.choice(np.setdiff1d(np.arange(S), big), 30, replace=False))
    ll[tied] = -1.0
    bad = rng.standard_normal(S)
    bad[12] = np.nan
    m = np.array([ll, bad, np.round(rng.standard_normal(S), 1)])
    lw, e, k, gap = weights_close(m, None, gpu)
    hlw = _psis_weights_host(m)[0]
    assert np.all(np.abs(lw[[0, 2]] - hlw[[0, 2]]) <= 4 * KLW_CRAFTED_MEASURED)
    assert np.all(np.diff(lw[0][tied[-3:]]) > 0) and np.all(lw[0][tied[:-3]] == lw[0][tied[0]]) and lw[0][tied[-3]] > lw[0][tied[0]]
    assert np.all(np.isnan(lw[1])) and np.isnan(e[1]) and np.isinf(k[1])
    # tails at and one past the supported length
    S = 50000
    ll = np.array([-0.5 * rng.standard_normal(S) ** 2, -np.log(((1 - rng.random(S)) ** -0.6 - 1) / 0.6)])
    r_ok = S * 9.0 / 8192.0 ** 2 * 1.0001
    assert api._tail_length(S, r_ok) == 8192
    lw, e, k, gap = weights_close(ll, r_ok, gpu)
    hlw = _psis_weights_host(ll, r_ok)[0]
    print("M = 8192: largest |lw_dev - lw_host| %.3g" % gap)
    assert np.all(np.abs(lw - hlw) <= 4 * KLW_CRAFTED_MEASURED)
    r_bad = S * 9.0 / 8193.0 ** 2 * 0.999
    assert "8192" in refused(lambda: _capi.psis_weights_raw(ll, [1.0, r_bad], gpu))


def test_fit_carries_the_loo_predictive(gpu, monkeypatch):
    X, y, _ = bnr_amd.make_synthetic(50, 10, 3, seed=SEED + 7)
    kw = dict(nburn=100, nsamples=200, x_transform=False, num_chains=3, seed=99, suppress_timer=True, filename=None, device=gpu)
    res = bnr_amd.Fit(X, y, 3, return_state=False, pool_chains=True, loo_predict=True, predict_interval=90, loo_r_eff=0.8, **kw)
    lp = res.loo_predictive
    assert lp is not None and bnr_amd.LOOPredict(res) is lp and res.state is None and res.stat_chains == 3 and lp.draws == 600 and lp.interval == 90
    assert res.loo is not None and np.array_equal(res.loo["elpd_loo_i"], lp.elpd_loo_i) and np.array_equal(res.loo["pareto_k"], lp.pareto_k)
    assert res.loo["n_high_k"] == lp.n_high_k
    # the same fit with the tables: the host restatement over the fetched tables of ALL chains
    keep = []
    again = bnr_amd.generate_samples(X, y, 3, nburn=100, nsamp=200, maxburn=300, psrf_cutoff=1.01, x_transform=False, num_chains=3, seed=99,
                                     suppress_timer=True, device=gpu, return_state=True, pool_chains=True, loo_predict=True, predict_interval=90,
                                     loo_r_eff=0.8, _keep=keep)
    cs = keep[0]
    try:
        for f in dataclasses.fields(lp):
            u, v = getattr(lp, f.name), getattr(again.loo_predictive, f.name)
            assert np.array_equal(u, v, equal_nan=True) if isinstance(u, np.ndarray) else (u == v or (u != u and v != v)), f.name
        tables = [cs.chains[c].fetch() for c in (1, 2, 3)]
        dev = (lp.lpd_i, lp.elpd_loo_i, lp.pareto_k, lp.loo_mean, lp.loo_sd, lp.loo_pit, lp.loo_lower, lp.loo_upper)
        host = _host_loo_predict(tables, X, y, res.burn_in, res.sampled, 90, False, 0.8)
        check_against_host(dev, tables, X, y, res.burn_in, res.sampled, 0.8, "Fit, 3 chains pooled", 0.05, 0.95)
        assert lp.coverage == host.coverage and lp.n_high_k == host.n_high_k
        B = np.concatenate([eta_bound(t, X, res.burn_in, res.sampled) for t in tables], axis=1).max(axis=1)
        amax = np.abs(np.concatenate([_host_eta(t, X, res.burn_in, res.sampled) for t in tables], axis=1)).max(axis=1)
        # the fallback over chain 1's table, and a fit without pool_chains: chain 1 alone through the same entry point
        solo = bnr_amd.Fit(X, y, 3, return_state=True, loo_predict=True, **kw)
        one = cs.chains[1].loo_predict(res.burn_in + 1, res.sampled)
        assert solo.stat_chains == 1 and solo.loo_predictive.draws == 200 and np.array_equal(solo.loo_predictive.loo_mean, one[3])
        assert np.array_equal(solo.loo["elpd_loo_i"], one[1]) and np.array_equal(solo.loo_predictive.loo_upper, one[7])
        fb = bnr_amd.LOOPredict(dataclasses.replace(solo, loo_predictive=None), X, y, x_transform=False)
        assert np.all(np.abs(fb.loo_mean - solo.loo_predictive.loo_mean) <= B + 4 * KMEAN_MEASURED * amax)
    finally:
        cs.close()
    # a rank that does not hold every chain: refused before any sampling
    monkeypatch.setattr(api, "_rank_world", lambda: (0, 2))
    with pytest.raises(ValueError, match="one rank"):
        bnr_amd.Fit(X, y, 3, loo_predict=True, **kw)


def test_headline_group_pooled_loo_predict(gpu):
    """the 8-chain headline group (n = 500, V = 100, R = 7) over 2 000 rows per chain: every output finite wherever k-hat is; coverage and the KS
    distance are reported, not asserted"""
    n, V, R, nsamp = 500, 100, 7, 2000
    tot = nsamp + 1
    X, y, _ = bnr_amd.make_synthetic(n, V, R, seed=SEED + 5)
    chains = [bnr_amd.Chain(X, y, R, tot, SEED, 1, device=gpu)]
    chains += [bnr_amd.Chain.like(chains[0], SEED, c) for c in range(2, 9)]
    grp = bnr_amd.Group(chains)
    for ch in chains:
        ch.init_prior()
    grp.run(2, tot, tot)
    lp = api.device_loo_predict(chains, y, 1, nsamp, 95)
    fin = np.isfinite(lp.pareto_k)
    for a in (lp.loo_mean, lp.loo_sd, lp.loo_pit, lp.loo_lower, lp.loo_upper, lp.elpd_loo_i):
        assert np.all(np.isfinite(a[fin]))
    assert np.all(lp.loo_lower[fin] < lp.loo_upper[fin]) and lp.draws == 8 * nsamp
    old = _capi.pooled_loo(chains, 2, nsamp)
    loo_close((lp.lpd_i, lp.elpd_loo_i, lp.pareto_k), old)
    print("headline group, S = %d: coverage %.3f, KS %.3f, rmse_loo %.4f, r2_loo %.4f, n_high_k %d of %d"
          % (lp.draws, lp.coverage, lp.ks, lp.rmse_loo, lp.r2_loo, lp.n_high_k, n))
    grp.close()
    for ch in chains:
        ch.close()
