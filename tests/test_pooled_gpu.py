"""GPU tests of the pooled-chain statistics, the predictive interval of a new observation and the PIT (run with -m gpu on an MI355X):
bnr_chains_summary / _predict / _predict_from_matrices / _loglik_stats / _loo against the host restatements over the fetched tables of a
3-chain lockstep group, the bitwise equalities (one chain = the single-chain entry points; block sizes, input formats, repeated calls, the
row-keyed noise), no side effects on any member, the refusals, and Fit(..., pool_chains=True, predict_observation=True).

Bounds.  eta: test_predict_gpu.eta_bound, B_is = 1e-12 sum_e |x_ie gamma_se| + 1e-14 (derived there).  A predictive draw is
y~_is = eta_is + sqrt(tau2_s) z_is, on both sides one rounding each for the sqrt, the product and the sum, so the device's differs from the
host's by at most B_is + 2^-53 (4 |eta_is| + (4 + K_Z) |sqrt(tau2_s) z_is|): the eta bound, the three roundings (doubled), and the K_Z ulps by
which the device's bnr_normal may differ from the host's (their log, sin and cos come from different math libraries).  An order statistic of
a row moves by no more than the largest such bound of the row.  K_Z cannot be derived here; test_noise_counter_layout_and_ulp_gap measures it
(KZ_MEASURED, recorded in DESIGN.md section 8) and the bounds use 4 x it.  The tighter B_is + 4 2^-53 |y~_is| (no allowance for z) is
printed beside it.
PIT: |pit_dev - pit_host| <= 0.3990 B_i / min_s sqrt(tau2_s) (the slope of Phi is at most 1 / sqrt(2 pi) = 0.3990) + K_ERFC 2^-53, K_ERFC =
4 x the gap measured between the device's and the host's sums of erfc on this fixture's own arguments (KERFC_MEASURED)."""
import numpy as np
import pytest

import bnr_amd
from bnr_amd import _capi, api
from bnr_amd.api import _host_eta, _host_loglik, _psis_host, _summary_ranks
from test_loo_gpu import close as loo_close
from test_predict_gpu import eta_bound

pytestmark = pytest.mark.gpu
SEED = 4717
PS = 0xC0FFEE12345                 # pred_seed of the direct calls
KZ_MEASURED = 3                    # largest ulp distance between the device's and the host's bnr_normal over the draws of the measuring test
KERFC_MEASURED = 1                 # largest |pit_dev - pit_host| / 2^-53 on the fixture
U = 2.0 ** -53
NB, NS = 100, 300


@pytest.fixture(scope="module")
def trio(gpu):
    """a 3-chain lockstep group, n = 60, V = 12, R = 3, 400-row tables; 37 new rows with responses"""
    X, y, _ = bnr_amd.make_synthetic(60, 12, 3, seed=SEED)
    chains = [bnr_amd.Chain(X, y, 3, 400, SEED, 1, device=gpu)]
    chains += [bnr_amd.Chain.like(chains[0], SEED, c) for c in (2, 3)]
    grp = bnr_amd.Group(chains)
    for ch in chains:
        ch.init_prior()
    grp.run(2, 400, 400)
    Xn, yn, _ = bnr_amd.make_synthetic(37, 12, 3, seed=SEED + 1)
    yield chains, X, y, Xn, yn, [ch.fetch() for ch in chains]
    grp.close()
    for ch in chains:
        ch.close()


def pooled_cols(tables, X, nb, ns):
    """(eta, B, tau2) over the pooled window: 37 x S, 37 x S, S"""
    eta = np.concatenate([_host_eta(t, X, nb, ns) for t in tables], axis=1)
    B = np.concatenate([eta_bound(t, X, nb, ns) for t in tables], axis=1)
    tau2 = np.concatenate([t["tau2"][nb:nb + ns, 0, 0] for t in tables])
    return eta, B, tau2


def test_pooled_prediction_matches_the_host(trio):
    chains, _X, _y, Xn, yn, tables = trio
    S = 3 * NS
    k_lo, k_hi = _summary_ranks(S, 95)
    mean, lo, hi, lpd, pw, plo, phi, pit = _capi.pooled_predict(chains, Xn, NB + 1, NS, k_lo, k_hi, y=yn, pred_seed=PS, pit=True)
    eta, B, tau2 = pooled_cols(tables, Xn, NB, NS)
    Bm = B.max(axis=1)
    srt = np.sort(eta, axis=1)
    assert np.all(np.abs(mean - eta.mean(axis=1)) <= Bm) and np.all(np.abs(lo - srt[:, k_lo - 1]) <= Bm) and np.all(np.abs(hi - srt[:, k_hi - 1]) <= Bm)
    host = api._host_pooled_predict(tables, Xn, yn, NB, NS, pred_seed=PS)
    assert host.draws == S
    assert np.all(np.abs(mean - host.estimate) <= 2 * Bm)             # (the restatement sums over the concatenated table: same bound, twice over)
    ref_lpd, ref_pw, ref_pit = api._host_pooled_pointwise(tables, Xn, yn, NB, NS)
    assert np.all(np.abs(lpd - ref_lpd) <= 1e-10 * np.abs(ref_lpd) + 1e-13), np.max(np.abs(lpd - ref_lpd) / np.abs(ref_lpd))
    assert np.all(np.abs(pw - ref_pw) <= 1e-8 * ref_pw + 1e-12)
    # predictive bounds
    sz = np.sqrt(tau2)[None, :] * _capi.host_pred_noise(PS, 0, S, 0, 37)
    yt = eta + sz
    ys = np.sort(yt, axis=1)
    bound = (B + U * (4 * np.abs(eta) + (4 + 4 * KZ_MEASURED) * np.abs(sz))).max(axis=1)
    tight = (B + 4 * U * np.abs(yt)).max(axis=1)
    dl, dh = np.abs(plo - ys[:, k_lo - 1]), np.abs(phi - ys[:, k_hi - 1])
    print("predictive bounds: worst error / bound %.3g (lower) %.3g (upper); against B + 4 u |y~|: %.3g, %.3g"
          % (np.max(dl / bound), np.max(dh / bound), np.max(dl / tight), np.max(dh / tight)))
    assert np.all(dl <= bound) and np.all(dh <= bound), (np.max(dl / bound), np.max(dh / bound))
    # PIT
    pit_host = api._host_pit(eta, tau2, yn)
    gap = np.abs(pit - pit_host)
    eta_part = 0.3990 * Bm / np.sqrt(tau2).min()
    print("PIT: worst |dev - host| = %.3g = %.2f x 2^-53; eta part of the bound up to %.3g" % (gap.max(), gap.max() / U, eta_part.max()))
    assert np.all(gap <= eta_part + 4 * KERFC_MEASURED * U), gap.max() / U
    assert np.all((pit >= 0) & (pit <= 1))
    # the training rows through bnr_chains_loglik_stats: same kernels, and the PIT of the training responses
    X, y = trio[1], trio[2]
    l2, p2, t2 = _capi.pooled_loglik_stats(chains, NB + 1, NS, pit=True)
    rl, rp, rt = api._host_pooled_pointwise(tables, X, y, NB, NS)
    Bt = np.concatenate([eta_bound(t, X, NB, NS) for t in tables], axis=1).max(axis=1)
    assert np.all(np.abs(l2 - rl) <= 1e-10 * np.abs(rl) + 1e-13) and np.all(np.abs(p2 - rp) <= 1e-8 * rp + 1e-12)
    assert np.all(np.abs(t2 - rt) <= 0.3990 * Bt / np.sqrt(tau2).min() + 4 * KERFC_MEASURED * U), np.max(np.abs(t2 - rt)) / U
    l3, p3, t3 = _capi.pooled_loglik_stats(chains, NB + 1, NS)
    assert t3 is None and np.array_equal(l3, l2) and np.array_equal(p3, p2)


def test_pooled_summary_matches_numpy(trio):
    chains, _X, _y, _Xn, _yn, tables = trio
    for nb, ns, interval in ((NB, NS, 95), (0, 400, 50), (17, 101, 90)):
        g = np.concatenate([t["gamma"][nb:nb + ns, :, 0] for t in tables], axis=0)
        xi = np.concatenate([t["xi"][nb:nb + ns, :, 0] for t in tables], axis=0)
        gs = np.sort(g, axis=0)
        lw, hi = _summary_ranks(3 * ns, interval)
        dev = bnr_amd.device_summary_pooled(chains, nb, ns, interval)
        assert np.array_equal(dev["lower_bound"], gs[lw - 1]) and np.array_equal(dev["upper_bound"], gs[hi - 1])
        assert np.all(np.abs(dev["estimate"] - g.mean(axis=0)) <= 1e-13 * np.abs(g).mean(axis=0))
        assert np.allclose(dev["probability"], xi.mean(axis=0), rtol=1e-13)
        host = api._host_pooled_summary(tables, nb, ns, interval)
        assert np.array_equal(dev["lower_bound"], host["lower_bound"]) and np.array_equal(dev["upper_bound"], host["upper_bound"])
    base = _capi.pooled_summary(chains, NB + 1, NS, 23, 878)
    try:
        for cols in (1, 7, 32, 89, 90):                                            # q + V = 90 parameter columns
            chains[0].set_option("summary_block_cols", cols)
            for u, v in zip(base, _capi.pooled_summary(chains, NB + 1, NS, 23, 878)):
                assert np.array_equal(u, v), cols
    finally:
        chains[0].set_option("summary_block_cols", 0)


def test_pooled_loo_matches_the_host(trio):
    chains, X, y, _Xn, _yn, tables = trio
    for nb, ns, r_eff in ((NB, NS, None), (0, 400, 0.5), (150, 250, np.linspace(0.3, 2.0, 60))):
        got = _capi.pooled_loo(chains, nb + 1, ns, r_eff)
        ll = np.concatenate([_host_loglik(t, X, y, nb, ns) for t in tables], axis=1)
        loo_close(got, _psis_host(ll, r_eff))
        assert np.all(np.isfinite(got[2]))
        assert np.array_equal(got[0], _capi.pooled_loglik_stats(chains, nb + 1, ns)[0])          # lpd bit for bit the pooled loglik_stats's


def test_one_chain_without_extras_is_the_single_chain_call(trio):
    chains, _X, _y, Xn, yn, _t = trio
    for ch in chains[:2]:
        a = ch.predict(Xn, 51, 333, 9, 325, y=yn)
        b = _capi.pooled_predict([ch], Xn, 51, 333, 9, 325, y=yn)
        assert b[5] is None and b[6] is None and b[7] is None
        for u, v in zip(a, b[:5]):
            assert np.array_equal(u, v)
        # ... and the extras do not disturb the eta statistics
        c = _capi.pooled_predict([ch], Xn, 51, 333, 9, 325, y=yn, pred_seed=PS, pit=True)
        for u, v in zip(a, c[:5]):
            assert np.array_equal(u, v)
        for u, v in zip(ch.loglik_stats(51, 333), _capi.pooled_loglik_stats([ch], 51, 333)[:2]):
            assert np.array_equal(u, v)
        for u, v in zip(ch.loo(51, 333, 0.7), _capi.pooled_loo([ch], 51, 333, 0.7)):
            assert np.array_equal(u, v)
        for u, v in zip(ch.summary(51, 333, 9, 325), _capi.pooled_summary([ch], 51, 333, 9, 325)):
            assert np.array_equal(u, v)
    mats = [bnr_amd.create_lower_tri(Xn[i], 12) for i in range(37)]
    a = chains[0].predict(mats, 51, 333, 9, 325, y=yn, x_transform=True)
    b = _capi.pooled_predict(chains[:1], mats, 51, 333, 9, 325, y=yn, x_transform=True)
    for u, v in zip(a, b[:5]):
        assert np.array_equal(u, v)


def test_blocks_formats_and_repeated_calls_give_bitwise_equal_results(trio):
    chains, _X, _y, Xn, yn, _t = trio
    args = (NB + 1, NS, 23, 878)
    base = _capi.pooled_predict(chains, Xn, *args, y=yn, pred_seed=PS, pit=True)
    base_ll = _capi.pooled_loglik_stats(chains, NB + 1, NS, pit=True)
    base_loo = _capi.pooled_loo(chains, NB + 1, NS)
    try:
        for rows in (32, 64, 0):
            chains[0].set_option("predict_block_rows", rows)
            for u, v in zip(base, _capi.pooled_predict(chains, Xn, *args, y=yn, pred_seed=PS, pit=True)):
                assert np.array_equal(u, v), rows
            for u, v in zip(base_ll, _capi.pooled_loglik_stats(chains, NB + 1, NS, pit=True)):
                assert np.array_equal(u, v), rows
            for u, v in zip(base_loo, _capi.pooled_loo(chains, NB + 1, NS)):
                assert np.array_equal(u, v), rows
    finally:
        chains[0].set_option("predict_block_rows", 0)
    # matrix input against n x q input, and the element types of a 0/1 X
    mats = [bnr_amd.create_lower_tri(Xn[i], 12) for i in range(37)]
    for u, v in zip(base, _capi.pooled_predict(chains, mats, *args, y=yn, x_transform=True, pred_seed=PS, pit=True)):
        assert np.array_equal(u, v)
    Xb = np.random.default_rng(SEED + 2).random((37, 78)) < 0.5
    f64 = _capi.pooled_predict(chains, Xb.astype(np.float64), *args, y=yn, pred_seed=PS, pit=True)
    bmats = [bnr_amd.create_lower_tri(Xb[i], 12) for i in range(37)]
    for other in (_capi.pooled_predict(chains, Xb.astype(np.uint8), *args, y=yn, pred_seed=PS, pit=True),
                  _capi.pooled_predict(chains, Xb, *args, y=yn, pred_seed=PS, pit=True),
                  _capi.pooled_predict(chains, bmats, *args, y=yn, x_transform=True, pred_seed=PS, pit=True)):
        for u, v in zip(f64, other):
            assert np.array_equal(u, v)
    # the noise is keyed by the row's index in the call: row 5 of rows 0..36 = row 5 of rows 0..5; the same row at another index is another draw
    short = _capi.pooled_predict(chains, Xn[:6], *args, y=yn[:6], pred_seed=PS, pit=True)
    for u, v in zip(base, short):
        assert np.array_equal(u[:6], v)
    moved = _capi.pooled_predict(chains, Xn[5:6], *args, y=yn[5:6], pred_seed=PS, pit=True)
    for k in (0, 1, 2, 3, 4, 7):
        assert moved[k][0] == base[k][5], k
    assert moved[5][0] != base[5][5] and moved[6][0] != base[6][5]
    other_seed = _capi.pooled_predict(chains, Xn, *args, y=yn, pred_seed=PS + 1, pit=True)
    assert not np.array_equal(other_seed[5], base[5]) and np.array_equal(other_seed[7], base[7]) and np.array_equal(other_seed[0], base[0])


def test_noise_counter_layout_and_ulp_gap(gpu):
    """gamma = 0, mu = 0, tau2 = 1 (loaded): a one-row window of one chain returns z_i0 itself as both predictive bounds; a one-row window of
    three chains the three draws z_i0, z_i1, z_i2 through the ranks 1, 2, 3.  The largest ulp distance to bnr_host_pred_noise is K_Z."""
    m = 12000
    X, y, _ = bnr_amd.make_synthetic(60, 12, 3, seed=SEED + 9)
    chains = [bnr_amd.Chain(X, y, 3, 4, SEED, 1, device=gpu)]
    chains += [bnr_amd.Chain.like(chains[0], SEED, c) for c in (2, 3)]
    t = _capi.new_table(4, 12, 3, dead=False)
    t["tau2"][:] = 1.0
    for ch in chains:
        ch.load(t)
    Xm = np.random.default_rng(3).standard_normal((m, 78))
    worst = 0.0
    for seed in (1, PS, 2**64 - 5):
        mean, lo, hi, _l, _p, plo, phi, _pit = _capi.pooled_predict(chains[:1], Xm, 2, 1, 1, 1, pred_seed=seed)
        assert np.all(mean == 0) and np.all(lo == 0) and np.array_equal(plo, phi)
        z = _capi.host_pred_noise(seed, 0, 3, 0, m)
        ulps = np.abs(plo - z[:, 0]) / np.spacing(np.abs(z[:, 0]))
        worst = max(worst, ulps.max())
        got = np.stack([_capi.pooled_predict(chains, Xm, 2, 1, k, k, pred_seed=seed)[5] for k in (1, 2, 3)], axis=1)
        zs = np.sort(z, axis=1)
        ulps3 = np.abs(got - zs) / np.spacing(np.abs(zs))
        worst = max(worst, ulps3.max())
        assert np.mean(got == zs) > 0.5                     # the layout (it = pooled draw, elem = row): most draws agree to the last bit
    print("K_Z: largest ulp distance between the device's and the host's noise over %d draws: %.1f" % (3 * 4 * m, worst))
    assert worst <= 4 * KZ_MEASURED, worst
    for ch in chains:
        ch.close()


def test_no_side_effects_on_any_member(gpu):
    X, y, _ = bnr_amd.make_synthetic(60, 12, 3, seed=SEED + 3)
    Xn, yn, _ = bnr_amd.make_synthetic(37, 12, 3, seed=SEED + 4)
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
    _capi.pooled_predict(a, Xn, 2, k - 1, 1, 3 * (k - 1), y=yn, pred_seed=PS, pit=True)
    _capi.pooled_loglik_stats(a, 1, k, pit=True)
    _capi.pooled_loo(a, 1, k, 0.5)
    _capi.pooled_summary(a, 1, k, 2, 100)
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
    chains, X, y, Xn, yn, _t = trio
    calls = lambda cs, first=NB + 1, ns=NS: (lambda: _capi.pooled_predict(cs, Xn, first, ns, 1, 1, y=yn, pred_seed=PS, pit=True),
                                            lambda: _capi.pooled_loglik_stats(cs, first, ns, pit=True),
                                            lambda: _capi.pooled_loo(cs, first, ns),
                                            lambda: _capi.pooled_summary(cs, first, ns, 1, 1))
    for call in calls([chains[0], chains[1], chains[0]]):                          # a duplicate chain
        assert "twice" in refused(call)
    for first, ns in ((0, 10), (350, 60), (1, 0)):                                 # a window outside the table
        for call in calls(chains, first, ns):
            refused(call)
    refused(lambda: _capi.pooled_predict(chains, Xn, NB + 1, NS, 0, 5))            # ranks outside 1 .. S
    refused(lambda: _capi.pooled_predict(chains, Xn, NB + 1, NS, 1, 3 * NS + 1))
    refused(lambda: _capi.pooled_summary(chains, NB + 1, NS, 1, 3 * NS + 1))
    _capi.pooled_summary(chains, NB + 1, NS, 1, 3 * NS)                            # (S itself is a rank)
    # chains of another V; a shorter table
    X2, y2, _ = bnr_amd.make_synthetic(60, 10, 3, seed=SEED + 5)
    other = bnr_amd.Chain(X2, y2, 3, 400, SEED, 1, device=gpu)
    short = bnr_amd.Chain.like(chains[0], SEED, 9, 300)
    lone = bnr_amd.Chain.like(chains[0], SEED, 8, 400)
    try:
        for ch in (other, short, lone):
            ch.init_prior()
        lone.run(2, 400, 20)
        for call in calls([chains[0], other]):
            assert "equal n, V, R" in refused(call)
        for call in calls([chains[0], short]):
            assert "window" in refused(call)
        # a pending asynchronous run on a member: refused, and the run completes as usual afterwards
        lone.run_async(21, 400, 24)
        try:
            for cs in ([chains[0], lone], [lone, chains[0]]):
                for call in calls(cs):
                    assert "pending" in refused(call)
        finally:
            lone.sync()
        _capi.pooled_summary([chains[0], lone], 2, 20, 1, 40)
    finally:
        for ch in (other, short, lone):
            ch.close()


def test_pooled_loo_tail_at_and_past_the_limit(gpu):
    """3 chains x 14 000 rows of the small model: S = 42 000, 0.2 S = 8 400 > BNR_PSIS_MAX_TAIL, so the tail is 3 sqrt(S / r_eff) = 615 with
    r_eff = 1 and is refused once that exceeds 8 192 too"""
    rows = 14000
    X, y, _ = bnr_amd.make_synthetic(60, 12, 3, seed=SEED + 6)
    chains = [bnr_amd.Chain(X, y, 3, rows, SEED, 1, device=gpu)]
    chains += [bnr_amd.Chain.like(chains[0], SEED, c) for c in (2, 3)]
    grp = bnr_amd.Group(chains)
    for ch in chains:
        ch.init_prior()
    grp.run(2, rows, rows)
    S = 3 * rows
    assert api._tail_length(S, 1.0) == 615
    got = _capi.pooled_loo(chains, 1, rows)
    ll = np.concatenate([_host_loglik(ch.fetch(), X, y, 0, rows) for ch in chains], axis=1)
    loo_close(got, _psis_host(ll))
    r_bad = S * 9.0 / 8193.0 ** 2 * 0.999
    assert api._tail_length(S, r_bad) > 8192
    assert "8192" in refused(lambda: _capi.pooled_loo(chains, 1, rows, r_bad))
    _capi.pooled_loo(chains[:1], 1, rows, r_bad)                                   # (one chain: 0.2 x 14 000 = 2 800 draws of tail at most)
    grp.close()
    for ch in chains:
        ch.close()


def test_fit_pools_the_chains(gpu):
    X, y, _ = bnr_amd.make_synthetic(50, 10, 3, seed=SEED + 7)
    Xn, yn, _ = bnr_amd.make_synthetic(21, 10, 3, seed=SEED + 8)
    kw = dict(x_transform=False, num_chains=3, seed=99, suppress_timer=True, summary_interval=95, predict_X=Xn, predict_y=yn, waic=True, loo=True,
              return_state=False, device=gpu)
    res = bnr_amd.Fit(X, y, 3, nburn=100, nsamples=200, filename=None, pool_chains=True, predict_observation=True, **kw)
    keep = []
    again = bnr_amd.generate_samples(X, y, 3, nburn=100, nsamp=200, maxburn=300, psrf_cutoff=1.01, pool_chains=True, predict_observation=True, _keep=keep,
                                     **kw)
    cs = keep[0]
    try:
        chains = [cs.chains[c] for c in (1, 2, 3)]
        nb, ns = res.burn_in, res.sampled
        S = 3 * ns
        assert res.stat_chains == 3 and res.state is None and res.prediction.draws == S and again.burn_in == nb and again.sampled == ns
        k_lo, k_hi = _summary_ranks(S, 95)
        d = _capi.pooled_predict(chains, Xn, nb + 1, ns, k_lo, k_hi, y=yn, pred_seed=99, pit=True)
        for r in (res, again):
            p = r.prediction
            for got, want in zip((p.estimate, p.lower_bound, p.upper_bound, p.lpd, p.pred_lower_bound, p.pred_upper_bound, p.pit),
                                 (d[0], d[1], d[2], d[3], d[5], d[6], d[7])):
                assert np.array_equal(got, want)
            sm = _capi.pooled_summary(chains, nb + 1, ns, k_lo, k_hi)
            for key, want in zip(("estimate", "lower_bound", "upper_bound", "probability"), sm):
                assert np.array_equal(r.summary_device[key], want), key
            lpd, pw, pit = _capi.pooled_loglik_stats(chains, nb + 1, ns, pit=True)
            assert np.array_equal(r.waic["lpd_i"], lpd) and np.array_equal(r.waic["p_waic_i"], pw) and np.array_equal(r.waic["pit_i"], pit)
            l = _capi.pooled_loo(chains, nb + 1, ns)
            assert np.array_equal(r.loo["lpd_i"], l[0]) and np.array_equal(r.loo["elpd_loo_i"], l[1]) and np.array_equal(r.loo["pareto_k"], l[2])
            assert r.loo["khat_threshold"] == api._loo_from_pointwise(*l, S)["khat_threshold"]
    finally:
        cs.close()
    # pool_chains off, predict_observation off: exactly the single-chain calls on chain 1 (the parent's behaviour)
    keep = []
    plain = bnr_amd.generate_samples(X, y, 3, nburn=100, nsamp=200, maxburn=300, psrf_cutoff=1.01, _keep=keep, **kw)
    fit = bnr_amd.Fit(X, y, 3, nburn=100, nsamples=200, filename=None, pool_chains=False, predict_observation=False, **kw)
    cs = keep[0]
    try:
        ch = cs.chains[1]
        nb, ns = plain.burn_in, plain.sampled
        k_lo, k_hi = _summary_ranks(ns, 95)
        d = ch.predict(Xn, nb + 1, ns, k_lo, k_hi, y=yn)
        for r in (plain, fit):
            p = r.prediction
            assert r.stat_chains == 1 and p.pred_lower_bound is None and p.pred_upper_bound is None and p.pit is None and p.draws is None
            for got, want in zip((p.estimate, p.lower_bound, p.upper_bound, p.lpd), d[:4]):
                assert np.array_equal(got, want)
            for key, want in zip(("estimate", "lower_bound", "upper_bound", "probability"), ch.summary(nb + 1, ns, k_lo, k_hi)):
                assert np.array_equal(r.summary_device[key], want), key
            lpd, pw = ch.loglik_stats(nb + 1, ns)
            assert np.array_equal(r.waic["lpd_i"], lpd) and np.array_equal(r.waic["p_waic_i"], pw) and "pit_i" not in r.waic
            l = ch.loo(nb + 1, ns)
            assert np.array_equal(r.loo["elpd_loo_i"], l[1]) and np.array_equal(r.loo["pareto_k"], l[2])
        # predict_observation alone: chain 1's window through the pooled entry point
        solo = bnr_amd.Fit(X, y, 3, nburn=100, nsamples=200, filename=None, predict_observation=True, pred_seed=7, **kw)
        e = _capi.pooled_predict([ch], Xn, nb + 1, ns, k_lo, k_hi, y=yn, pred_seed=7, pit=True)
        sp = solo.prediction
        assert solo.stat_chains == 1 and sp.draws == ns
        for got, want in zip((sp.estimate, sp.lower_bound, sp.upper_bound, sp.lpd, sp.pred_lower_bound, sp.pred_upper_bound, sp.pit),
                             (d[0], d[1], d[2], d[3], e[5], e[6], e[7])):
            assert np.array_equal(got, want)
    finally:
        cs.close()
