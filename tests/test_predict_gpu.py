"""GPU tests of posterior prediction and WAIC (run with -m gpu on an MI355X): bnr_chain_predict / bnr_chain_predict_from_matrices /
bnr_chain_loglik_stats against the host formulas over the fetched table, bitwise independence of the input format and of the block size,
no side effects on the chain, and the Fit(..., predict_X=..., waic=True) path.

Bounds: the device sums x_ie gamma_se in its own fixed order on the f64 matrix pipe, so an eta differs from the host's by at most
1e-12 sum_e |x_ie gamma_se| + 1e-14 (a few hundred roundings of at most 2^-53 each); the mean and the order statistics of eta over the
draws move by no more than the largest such bound of their row."""
import dataclasses

import numpy as np
import pytest

import bnr_amd
from bnr_amd import _capi
from bnr_amd.api import _host_eta, _host_pointwise, _summary_ranks

pytestmark = pytest.mark.gpu
SEED = 4711


def eta_bound(table, X, nburn, nsamp):
    g = table["gamma"][nburn:nburn + nsamp, :, 0]
    return 1e-12 * (np.abs(X) @ np.abs(g).T) + 1e-14


def check_prediction(table, X, y, nburn, nsamp, mean, lo, hi, lpd):
    E = _host_eta(table, X, nburn, nsamp)
    B = eta_bound(table, X, nburn, nsamp).max(axis=1)
    k_lo, k_hi = _summary_ranks(nsamp, 95)
    srt = np.sort(E, axis=1)
    assert np.all(np.abs(mean - E.mean(axis=1)) <= B), np.max(np.abs(mean - E.mean(axis=1)) - B)
    assert np.all(np.abs(lo - srt[:, k_lo - 1]) <= B)
    assert np.all(np.abs(hi - srt[:, k_hi - 1]) <= B)
    if y is not None:
        ref = _host_pointwise(table, X, y, nburn, nsamp)[0]
        assert np.all(np.abs(lpd - ref) <= 1e-10 * np.abs(ref) + 1e-13), np.max(np.abs(lpd - ref) / np.abs(ref))


@pytest.fixture(scope="module")
def lone(gpu):
    """n = 60, V = 12, R = 3, a 400-row table; 37 new rows with responses"""
    X, y, _ = bnr_amd.make_synthetic(60, 12, 3, seed=SEED)
    ch = bnr_amd.Chain(X, y, 3, 400, SEED, 1, device=gpu)
    ch.init_prior()
    ch.run(2, 400, 400)
    Xn, yn, _ = bnr_amd.make_synthetic(37, 12, 3, seed=SEED + 1)
    yield ch, X, y, Xn, yn, ch.fetch()
    ch.close()


def test_lone_chain_prediction_matches_the_host(lone):
    ch, _X, _y, Xn, yn, table = lone
    nburn, nsamp = 100, 300
    k_lo, k_hi = _summary_ranks(nsamp, 95)
    mean, lo, hi, lpd, pw = ch.predict(Xn, nburn + 1, nsamp, k_lo, k_hi, y=yn)
    check_prediction(table, Xn, yn, nburn, nsamp, mean, lo, hi, lpd)
    assert np.all(pw >= 0)
    # eta itself, draw by draw: a one-row window returns that draw's eta as mean and as both order statistics
    E = _host_eta(table, Xn, nburn, nsamp)
    B = eta_bound(table, Xn, nburn, nsamp)
    for s in (0, 1, 17, 150, nsamp - 1):
        m1, l1, h1, lp1, pw1 = ch.predict(Xn, nburn + 1 + s, 1, 1, 1)
        assert lp1 is None and pw1 is None
        assert np.array_equal(m1, l1) and np.array_equal(m1, h1)
        assert np.all(np.abs(m1 - E[:, s]) <= B[:, s]), s
    # the same without responses: same statistics bit for bit
    m2, l2, h2, lp2, _ = ch.predict(Xn, nburn + 1, nsamp, k_lo, k_hi)
    assert lp2 is None and np.array_equal(m2, mean) and np.array_equal(l2, lo) and np.array_equal(h2, hi)


def test_input_formats_give_bitwise_equal_results(lone):
    ch = lone[0]
    V, q = 12, 78
    rng = np.random.default_rng(SEED + 2)
    Xb = rng.random((37, q)) < 0.5
    yn = rng.standard_normal(37) + 10.0
    mats = [bnr_amd.create_lower_tri(Xb[i], V) for i in range(37)]
    assert mats[0].dtype == np.bool_
    args = (101, 300, 8, 292)
    a = ch.predict(Xb.astype(np.float64), *args, y=yn)
    b = ch.predict(Xb, *args, y=yn)
    c = ch.predict(mats, *args, y=yn, x_transform=True)
    d = ch.predict(Xb.astype(np.int64), *args, y=yn)
    for other in (b, c, d):
        for u, v in zip(a, other):
            assert np.array_equal(u, v)


def test_block_size_does_not_change_results(lone):
    ch, _X, _y, Xn, yn, _t = lone
    base = ch.predict(Xn, 51, 333, 9, 325, y=yn)
    base_ll = ch.loglik_stats(51, 333)
    try:
        for rows in (64, 20, 8, 1):
            ch.set_option("predict_block_rows", rows)
            got = ch.predict(Xn, 51, 333, 9, 325, y=yn)
            for u, v in zip(base, got):
                assert np.array_equal(u, v), rows
            for u, v in zip(base_ll, ch.loglik_stats(51, 333)):
                assert np.array_equal(u, v), rows
    finally:
        ch.set_option("predict_block_rows", 0)


def test_no_side_effects_on_the_chain(gpu):
    X, y, _ = bnr_amd.make_synthetic(60, 12, 3, seed=SEED + 3)
    Xn, yn, _ = bnr_amd.make_synthetic(37, 12, 3, seed=SEED + 4)
    k, tot = 40, 80
    a = bnr_amd.Chain(X, y, 3, tot, SEED, 1, device=gpu)
    b = bnr_amd.Chain(X, y, 3, tot, SEED, 1, device=gpu)
    for ch in (a, b):
        ch.init_prior()
        ch.run(2, tot, k)
    a.predict(Xn, 2, k - 1, 1, k - 1, y=yn)
    a.loglik_stats(1, k)
    for ch in (a, b):
        ch.run(k + 1, tot, tot)
    ta, tb = a.fetch(), b.fetch()
    for col in ta:
        assert np.array_equal(ta[col], tb[col]), col
    assert a.counters() == b.counters() and a.iter == b.iter
    a.close(); b.close()


def test_waic_on_training_rows_of_a_group_at_the_headline_size(gpu):
    n, V, R, tot, nburn = 500, 100, 7, 260, 60
    nsamp = tot - nburn
    X, y, _ = bnr_amd.make_synthetic(n, V, R, seed=SEED + 5)
    chains = [bnr_amd.Chain(X, y, R, tot, SEED, 1, device=gpu)]
    chains += [bnr_amd.Chain.like(chains[0], SEED, c) for c in range(2, 9)]
    grp = bnr_amd.Group(chains)
    for ch in chains:
        ch.init_prior()
    grp.run(2, tot, tot)
    ch1 = chains[0]
    table = ch1.fetch()
    lpd, pw = ch1.loglik_stats(nburn + 1, nsamp)
    ref_lpd, ref_pw = _host_pointwise(table, X, y, nburn, nsamp)
    assert np.all(np.abs(lpd - ref_lpd) <= 1e-10 * np.abs(ref_lpd) + 1e-13), np.max(np.abs(lpd - ref_lpd) / np.abs(ref_lpd))
    assert np.all(np.abs(pw - ref_pw) <= 1e-8 * ref_pw + 1e-12)
    # the training rows handed in as new rows: the same numbers bit for bit, and the statistics of eta within the bounds
    k_lo, k_hi = _summary_ranks(nsamp, 95)
    mean, lo, hi, lpd2, pw2 = ch1.predict(X, nburn + 1, nsamp, k_lo, k_hi, y=y)
    assert np.array_equal(lpd, lpd2) and np.array_equal(pw, pw2)
    check_prediction(table, X, y, nburn, nsamp, mean, lo, hi, lpd2)
    # chain 1 of the group = the same chain run alone
    alone = bnr_amd.Chain(X, y, R, tot, SEED, 1, device=gpu)
    alone.init_prior()
    alone.run(2, tot, tot)
    for u, v in zip((lpd, pw), alone.loglik_stats(nburn + 1, nsamp)):
        assert np.array_equal(u, v)
    alone.close()
    grp.close()
    for ch in chains:
        ch.close()


def test_fit_carries_prediction_and_waic(gpu):
    X, y, _ = bnr_amd.make_synthetic(50, 10, 3, seed=SEED + 6)
    Xn, yn, _ = bnr_amd.make_synthetic(21, 10, 3, seed=SEED + 7)
    kw = dict(nburn=100, nsamples=200, x_transform=False, num_chains=2, seed=99, suppress_timer=True, filename=None,
              predict_X=Xn, predict_y=yn, waic=True, device=gpu)
    res = bnr_amd.Fit(X, y, 3, return_state=True, **kw)
    p = res.prediction
    assert p is not None and p.ci_level == 95 and p.lpd.shape == (21,) and p.elpd == pytest.approx(np.sum(p.lpd), rel=1e-15)
    check_prediction(res.state, Xn, yn, res.burn_in, res.sampled, p.estimate, p.lower_bound, p.upper_bound, p.lpd)
    host = bnr_amd.Predict(res, Xn, yn, x_transform=False)
    B = eta_bound(res.state, Xn, res.burn_in, res.sampled).max(axis=1)
    assert np.all(np.abs(host.estimate - p.estimate) <= B)
    assert bnr_amd.Predict(res) is not None and np.array_equal(bnr_amd.Predict(res).estimate, p.estimate)
    w = bnr_amd.WAIC(res)
    hw = bnr_amd.WAIC(dataclasses.replace(res, waic=None), X, y, x_transform=False)
    assert w["waic"] == pytest.approx(hw["waic"], rel=1e-9) and w["p_waic"] >= 0
    assert np.all(np.abs(w["lpd_i"] - hw["lpd_i"]) <= 1e-10 * np.abs(hw["lpd_i"]) + 1e-13)
    res2 = bnr_amd.Fit(X, y, 3, return_state=False, **kw)
    assert res2.state is None
    for f in ("estimate", "lower_bound", "upper_bound", "lpd"):
        assert np.array_equal(getattr(res2.prediction, f), getattr(p, f)), f
    assert np.array_equal(res2.waic["lpd_i"], w["lpd_i"])


def test_bad_arguments_return_bad_arg(lone):
    ch, _X, _y, Xn, yn, _t = lone
    for first, nsamp in ((0, 10), (350, 60), (1, 0)):
        with pytest.raises(bnr_amd.BnrError) as e:
            ch.predict(Xn, first, nsamp, 1, 1)
        assert e.value.code == _capi.BNR_ERR_BAD_ARG
        with pytest.raises(bnr_amd.BnrError) as e:
            ch.loglik_stats(first, nsamp)
        assert e.value.code == _capi.BNR_ERR_BAD_ARG
    with pytest.raises(bnr_amd.BnrError) as e:
        ch.predict(Xn, 1, 10, 0, 11)
    assert e.value.code == _capi.BNR_ERR_BAD_ARG
    Xf = np.asfortranarray(Xn)
    out = [np.empty(37) for _ in range(5)]
    rc = ch.L.bnr_chain_predict(ch.h, 1, 10, 37, _capi._ptr(Xf), 9, None, 1, 10, *[_capi._ptr(o) for o in out])
    assert rc == _capi.BNR_ERR_BAD_ARG
    rc = ch.L.bnr_chain_predict(ch.h, 1, 10, 0, _capi._ptr(Xf), 0, None, 1, 10, *[_capi._ptr(o) for o in out])
    assert rc == _capi.BNR_ERR_BAD_ARG
    rc = ch.L.bnr_chain_predict(ch.h, 1, 10, 37, _capi._ptr(Xf), 0, _capi._ptr(np.asarray(yn)), 1, 10, *[_capi._ptr(o) for o in out[:3]], None, None)
    assert rc == _capi.BNR_ERR_BAD_ARG
    # a pending asynchronous run: refused, and the run completes as usual afterwards
    ch.run_async(2, 400, 3)
    try:
        with pytest.raises(bnr_amd.BnrError) as e:
            ch.predict(Xn, 1, 10, 1, 10)
        assert e.value.code == _capi.BNR_ERR_BAD_ARG
        with pytest.raises(bnr_amd.BnrError) as e:
            ch.loglik_stats(1, 10)
        assert e.value.code == _capi.BNR_ERR_BAD_ARG
    finally:
        ch.sync()
