"""GPU tests of PSIS-LOO (run with -m gpu on an MI355X): bnr_chain_loo against the host restatement over the fetched table, bitwise equality
with bnr_chain_loglik_stats's lpd, across block sizes and calls, no side effects on the chain; bnr_psis_loo on crafted log-likelihood rows
(ties, constant rows, short windows, GPD tails of known shape, a NaN row, tails at and past the supported length); the 8-chain headline group;
Fit(..., loo=True).

Bounds: the device's l is the host's up to the rounding of eta (k_predict's own K order, see test_predict_gpu.py), a few ulps of l; every
sum of the PSIS is in a fixed order that differs from numpy's, so elpd_loo agrees to 1e-9 relative and the fitted shape to 1e-6."""
import dataclasses

import numpy as np
import pytest

import bnr_amd
from bnr_amd import _capi
from bnr_amd.api import _host_loglik, _loo_from_pointwise, _psis_host

pytestmark = pytest.mark.gpu
SEED = 4713


def close(dev, host, rel=1e-9, kabs=1e-6):
    lpd, e, k = dev
    hl, he, hk = host
    lf = np.isfinite(hl)
    assert np.array_equal(lf, np.isfinite(lpd))
    assert np.all(np.abs(lpd[lf] - hl[lf]) <= 1e-10 * np.abs(hl[lf]) + 1e-12), np.max(np.abs(lpd[lf] - hl[lf]))
    fin = np.isfinite(he)
    assert np.array_equal(fin, np.isfinite(e))
    assert np.all(np.abs(e[fin] - he[fin]) <= rel * np.abs(he[fin]) + 1e-12), np.max(np.abs(e[fin] - he[fin]) / np.abs(he[fin]))
    assert np.array_equal(np.isinf(k), np.isinf(hk)), (k, hk)
    kf = np.isfinite(hk)
    assert np.all(np.abs(k[kf] - hk[kf]) <= kabs), np.max(np.abs(k[kf] - hk[kf]))


@pytest.fixture(scope="module")
def lone(gpu):
    """n = 60, V = 12, R = 3, a 400-row table"""
    X, y, _ = bnr_amd.make_synthetic(60, 12, 3, seed=SEED)
    ch = bnr_amd.Chain(X, y, 3, 400, SEED, 1, device=gpu)
    ch.init_prior()
    ch.run(2, 400, 400)
    yield ch, X, y, ch.fetch()
    ch.close()


def test_lone_chain_loo_matches_the_host(lone):
    ch, X, y, table = lone
    for nburn, nsamp, r_eff in ((100, 300, None), (0, 400, 0.5), (150, 250, np.linspace(0.3, 2.0, 60))):
        got = ch.loo(nburn + 1, nsamp, r_eff)
        ll = _host_loglik(table, X, y, nburn, nsamp)
        close(got, _psis_host(ll, r_eff))
        assert np.all(np.isfinite(got[2]))
        # lpd bit for bit bnr_chain_loglik_stats's
        assert np.array_equal(got[0], ch.loglik_stats(nburn + 1, nsamp)[0])


def test_loo_is_bitwise_stable_across_block_sizes_and_calls(lone):
    ch = lone[0]
    base = ch.loo(51, 333)
    try:
        for rows in (64, 20, 8, 1):
            ch.set_option("predict_block_rows", rows)
            for u, v in zip(base, ch.loo(51, 333)):
                assert np.array_equal(u, v), rows
    finally:
        ch.set_option("predict_block_rows", 0)
    for u, v in zip(base, ch.loo(51, 333)):
        assert np.array_equal(u, v)


def test_loo_has_no_side_effects_on_the_chain(gpu):
    X, y, _ = bnr_amd.make_synthetic(60, 12, 3, seed=SEED + 3)
    k, tot = 40, 80
    a = bnr_amd.Chain(X, y, 3, tot, SEED, 1, device=gpu)
    b = bnr_amd.Chain(X, y, 3, tot, SEED, 1, device=gpu)
    for ch in (a, b):
        ch.init_prior()
        ch.run(2, tot, k)
    a.loo(2, k - 1)
    a.loo(1, k, 0.25)
    ta0, tb0 = a.fetch(), b.fetch()
    for col in ta0:
        assert np.array_equal(ta0[col], tb0[col]), col
    for ch in (a, b):
        ch.run(k + 1, tot, tot)
    ta, tb = a.fetch(), b.fetch()
    for col in ta:
        assert np.array_equal(ta[col], tb[col]), col
    assert a.counters() == b.counters() and a.iter == b.iter
    a.close(); b.close()


def crafted_rows(S, rng):
    rows = [-0.5 * rng.standard_normal(S) ** 2 - 0.9189385332046727,
            np.full(S, -2.0),                                                      # constant: k-hat inf, elpd = lpd
            np.round(rng.standard_normal(S), 1)]                                   # many ties (at the cutoff too)
    for k in (0.3, 0.7, 1.2):                                                      # ratios with a GPD tail of shape k
        u = rng.random(S)
        rows.append(-np.log(((1 - u) ** (-k) - 1) / k + 1e-300))
    return np.array(rows)


@pytest.mark.parametrize("S", [1, 7, 20, 21, 24, 25, 400, 20000])
def test_psis_matrix_matches_the_host(gpu, S):
    rng = np.random.default_rng(S)
    ll = crafted_rows(S, rng)
    got = _capi.psis_loo_raw(ll, None, gpu)
    host = _psis_host(ll)
    close(got, host)
    assert np.all(np.abs(got[1][1] - got[0][1]) < 1e-14)                          # the constant row
    if S >= 400:
        assert np.all(np.isfinite(got[2][[0, 3, 4, 5]]))
    d = bnr_amd.psis_loo(ll, device=gpu)
    assert np.array_equal(d["elpd_loo_i"], got[1]) and np.array_equal(d["pareto_k"], got[2])


def test_psis_matrix_known_shapes_and_nan_row(gpu):
    rng = np.random.default_rng(9)
    S = 100000
    rows = []
    for k in (0.2, 0.5, 0.9):
        u = rng.random(S)
        rows.append(-np.log(2.0 * ((1 - u) ** (-k) - 1) / k))
    bad = rng.standard_normal(S)
    bad[123] = np.nan
    rows.append(bad)
    ll = np.array(rows)
    got = _capi.psis_loo_raw(ll, None, gpu)
    close(got, _psis_host(ll))
    assert np.all(np.abs(got[2][:3] - [0.2, 0.5, 0.9]) < 0.15), got[2]          # the tail fit (M = 949) sees the shape of the ratios
    assert np.isnan(got[1][3]) and np.isinf(got[2][3])


def test_psis_tail_lengths_near_and_past_the_limit(gpu):
    rng = np.random.default_rng(10)
    S = 50000
    ll = np.array([-0.5 * rng.standard_normal(S) ** 2, -np.log(((1 - rng.random(S)) ** -0.6 - 1) / 0.6)])
    r_ok = S * 9.0 / 8192.0 ** 2 * 1.0001                                          # M = ceil(3 sqrt(S / r)) = 8192
    assert bnr_amd.api._tail_length(S, r_ok) == 8192
    got = _capi.psis_loo_raw(ll, r_ok, gpu)
    close(got, _psis_host(ll, r_ok))
    r_bad = S * 9.0 / 8193.0 ** 2 * 0.999                                          # M = 8193 (or 8194)
    assert bnr_amd.api._tail_length(S, r_bad) > 8192
    with pytest.raises(bnr_amd.BnrError) as e:
        _capi.psis_loo_raw(ll, [1.0, r_bad], gpu)
    assert e.value.code == _capi.BNR_ERR_BAD_ARG and "8192" in str(e.value)


def test_headline_group_chain1_over_20000_rows(gpu):
    n, V, R, nsamp = 500, 100, 7, 20000
    tot = nsamp + 1
    X, y, _ = bnr_amd.make_synthetic(n, V, R, seed=SEED + 5)
    chains = [bnr_amd.Chain(X, y, R, tot, SEED, 1, device=gpu)]
    chains += [bnr_amd.Chain.like(chains[0], SEED, c) for c in range(2, 9)]
    grp = bnr_amd.Group(chains)
    for ch in chains:
        ch.init_prior()
    grp.run(2, tot, tot)
    ch1 = chains[0]
    got = ch1.loo(2, nsamp)
    table = ch1.fetch(1, tot)
    close(got, _psis_host(_host_loglik(table, X, y, 1, nsamp)))
    assert np.array_equal(got[0], ch1.loglik_stats(2, nsamp)[0])
    grp.close()
    for ch in chains:
        ch.close()


def test_fit_carries_loo(gpu):
    X, y, _ = bnr_amd.make_synthetic(50, 10, 3, seed=SEED + 6)
    kw = dict(nburn=100, nsamples=200, x_transform=False, num_chains=2, seed=99, suppress_timer=True, filename=None, loo=True, waic=True,
              device=gpu)
    res = bnr_amd.Fit(X, y, 3, return_state=True, **kw)
    d = res.loo
    assert d is not None and bnr_amd.LOO(res) is d
    host = bnr_amd.LOO(dataclasses.replace(res, loo=None), X, y, x_transform=False)
    close((d["lpd_i"], d["elpd_loo_i"], d["pareto_k"]), (host["lpd_i"], host["elpd_loo_i"], host["pareto_k"]))
    assert d["elpd_loo"] == pytest.approx(host["elpd_loo"], rel=1e-9) and d["looic"] == -2 * d["elpd_loo"]
    assert d["khat_threshold"] == host["khat_threshold"] and d["n_high_k"] == host["n_high_k"]
    assert np.array_equal(d["lpd_i"], res.waic["lpd_i"])
    again = _loo_from_pointwise(d["lpd_i"], d["elpd_loo_i"], d["pareto_k"], res.sampled)
    assert again["se"] == d["se"] and again["p_loo"] == d["p_loo"]
    res2 = bnr_amd.Fit(X, y, 3, return_state=False, loo_r_eff=0.5, **kw)
    host2 = bnr_amd.LOO(dataclasses.replace(res, loo=None), X, y, x_transform=False, r_eff=0.5)
    close((res2.loo["lpd_i"], res2.loo["elpd_loo_i"], res2.loo["pareto_k"]), (host2["lpd_i"], host2["elpd_loo_i"], host2["pareto_k"]))


def test_chain_loo_bad_arguments(lone):
    ch = lone[0]
    for first, nsamp in ((0, 10), (350, 60), (1, 0)):
        with pytest.raises(bnr_amd.BnrError) as e:
            ch.loo(first, nsamp)
        assert e.value.code == _capi.BNR_ERR_BAD_ARG
    out = [np.empty(60) for _ in range(3)]
    rc = ch.L.bnr_chain_loo(ch.h, 1, 10, _capi._ptr(np.full(60, -1.0)), *[_capi._ptr(o) for o in out])
    assert rc == _capi.BNR_ERR_BAD_ARG
    rc = ch.L.bnr_chain_loo(ch.h, 1, 10, None, _capi._ptr(out[0]), None, _capi._ptr(out[2]))
    assert rc == _capi.BNR_ERR_BAD_ARG
    rc = ch.L.bnr_chain_loo(ch.h, 1, 10, None, None, _capi._ptr(out[1]), _capi._ptr(out[2]))      # lpd may be NULL
    assert rc == _capi.BNR_OK and np.array_equal(out[1], ch.loo(1, 10)[1])
    ch.run_async(2, 400, 3)
    try:
        with pytest.raises(bnr_amd.BnrError) as e:
            ch.loo(1, 10)
        assert e.value.code == _capi.BNR_ERR_BAD_ARG
    finally:
        ch.sync()
