"""GPU tests of chain stacking (ABI 16; run with -m gpu on an MI355X): k_wsummary alone (bnr_wquantile against the numpy restatement
api._host_wquantile, itself pinned to a draw-by-draw transcription of the definition by tests/test_stacking_host.py), the dyadic identity
with the unweighted order statistics, bnr_chains_wsummary / bnr_chains_wpredict / bnr_chains_stack on loaded tables, the side effects and
refusals, and Fit(..., stack_chains=True).

The weighted mean and order statistics are compared bit for bit: the kernel's arithmetic is the strided sums of k_summary, integer counts and
K products and additions rounded one by one, which numpy does in the same order.  Where a libm call of the device enters (lpd, elpd_stack,
the predictive noise) the tolerances are those the issue and tests/test_pooled_gpu.py set.

Chains as in test_hdi_gpu.py: three Chains of n = 8, V = 16, R = 2 with 640-row tables, never run; tables come in by Chain.load."""
import numpy as np
import pytest

import bnr_amd
import diag_ref as dr
import hdi_cases as hc
import pred_ref as pr
import rank_diag_cases as rc
import sort_cases as sc
from bnr_amd import _capi, api

pytestmark = pytest.mark.gpu
NSAMPS = (1, 5, 255, 256, 257, 1025)
KS = (1, 2, 3, 8, 32)
U = 2.0 ** -53
KZ_MEASURED = 3                                    # tests/test_pooled_gpu.py: ulps between the device's and the host's bnr_normal
WINDOWS = ((38, 601), (3, 101))


@pytest.fixture(scope="module")
def chains(gpu):
    X, y, _ = bnr_amd.make_synthetic(dr.N, dr.V, dr.R, seed=3)
    cs = [bnr_amd.Chain(X, y, dr.R, dr.TOT, 99, 1, device=gpu)]
    cs += [bnr_amd.Chain.like(cs[0], 99, c) for c in (2, 3)]
    yield cs
    for c in cs:
        c.close()


def _load(chains, tabs):
    for ch, t in zip(chains, tabs):
        ch.load(t)


# ------------------------------------------------------------------------------------------------------------------ the kernel alone
def _ranks(S):
    c = lambda r: min(max(int(r), 1), S)
    return [(1, S), (c(2), c(S - 1)), (c(round(0.025 * S)), c(round(0.975 * S)))]


def _weights(K, rng):
    ws = [("uniform", np.full(K, 1.0 / K)), ("dirichlet", rng.dirichlet(np.ones(K))), ("sparse dirichlet", rng.dirichlet(np.full(K, 0.2)))]
    if K > 1:
        z = rng.dirichlet(np.ones(K))
        z[K // 2] = 0.0
        ws.append(("one chain at 0", z / z.sum()))
    ws += [("e_%d" % k, np.eye(K)[k]) for k in sorted({0, K // 2, K - 1})]
    return ws


def _matrix(K, nsamp):
    """rows of K nsamp draws: key rows of sort_cases (a key row is repeated or cut to the length, so its keys tie across chains), ties across
    chains, all draws equal, signed zeros, +-Inf"""
    S = K * nsamp
    rng = np.random.default_rng([31, K, nsamp])
    keys = sc.key_rows()
    nkey = int(min(48, max(4, 4_000_000 // (S * K))))
    pick = rng.choice(len(keys), size=nkey, replace=False)
    rows = [np.resize(keys[j][1], S) for j in pick]
    rows.append(np.round(rng.standard_normal(S) * 2) / 2)                   # ties across chains
    rows.append(np.full(S, -3.75))                                          # all equal
    z = np.where(rng.random(S) < 0.5, -0.0, 0.0)
    rows.append(z)                                                          # -0 below +0
    v = rng.standard_normal(S)
    v[rng.integers(S)] = np.inf
    v[rng.integers(S)] = -np.inf
    z2 = v.copy()
    z2[::2] = np.where(rng.random(z2[::2].size) < 0.5, -0.0, 0.0)
    rows += [v, z2]
    return np.ascontiguousarray(np.stack(rows))


def _same3(got, want, what):
    for f, g in zip(_capi.WQUANTILE_FIELDS, got):
        assert hc.same_bits(g, want[f]), (what, f, np.flatnonzero(g.view(np.uint64) != np.asarray(want[f]).view(np.uint64))[:5])


@pytest.mark.parametrize("K", KS)
def test_wquantile_against_the_restatement(gpu, K):
    for nsamp in NSAMPS:
        M = _matrix(K, nsamp)
        S = K * nsamp
        rng = np.random.default_rng([32, K, nsamp])
        for name, w in _weights(K, rng):
            for k_lo, k_hi in _ranks(S):
                got = _capi.wquantile_raw(M, w, K, k_lo, k_hi, gpu)
                _same3(got, api._host_wquantile(M, w, K, k_lo, k_hi), (K, nsamp, name, k_lo, k_hi))
    # each output alone (the others NULL; the bounds come as a pair) is the same bits
    full = _capi.wquantile_raw(M, w, K, k_lo, k_hi, gpu)
    for fields in (("mean",), ("lower", "upper")):
        one = _capi.wquantile_raw(M, w, K, k_lo, k_hi, gpu, fields=fields)
        for f, a, b in zip(_capi.WQUANTILE_FIELDS, one, full):
            assert (a is None) if f not in fields else hc.same_bits(a, b), (K, fields, f)
    d = bnr_amd.wquantile(M, w, K, 95, device=gpu)
    lw, hi = api._summary_ranks(S, 95)
    _same3((d["mean"], d["lower"], d["upper"]), api._host_wquantile(M, w, K, lw, hi), (K, "wquantile"))


def test_wquantile_nan_rows(gpu):
    rng = np.random.default_rng(11)
    M = rng.standard_normal((4, 3 * 257))
    M[0, 3] = dr.NAN_POS
    M[2, 700] = dr.NAN_NEG                                                  # in chain 2
    M[2, 5] = np.inf
    for w in (np.array([0.2, 0.3, 0.5]), np.array([0.5, 0.5, 0.0])):         # also where the NaN's chain has weight 0
        got = _capi.wquantile_raw(M, w, 3, 20, 750, gpu)
        _same3(got, api._host_wquantile(M, w, 3, 20, 750), tuple(w))
        for g in got:
            assert np.isnan(g[[0, 2]]).all() and not np.isnan(g[[1, 3]]).any()
    clean = _capi.wquantile_raw(M[1:2], w, 3, 20, 750, gpu)                  # the neighbouring clean row is what it is alone
    for a, b in zip(clean, got):
        assert hc.same_bits(a[0], b[1])


def test_wquantile_indices_past_16_bits(gpu):
    rng = np.random.default_rng(40000)
    M = np.round(rng.standard_normal((1, 80000)) * 64) / 64                  # K = 2, nsamp = 40 000, heavily tied
    for w in (np.array([0.5, 0.5]), np.array([0.3, 0.7]), np.array([0.0, 1.0])):
        for k_lo, k_hi in _ranks(80000):
            _same3(_capi.wquantile_raw(M, w, 2, k_lo, k_hi, gpu), api._host_wquantile(M, w, 2, k_lo, k_hi), (tuple(w), k_lo))


@pytest.mark.parametrize("K", (2, 4, 8))
def test_dyadic_uniform_weights_are_the_pooled_order_statistics(gpu, K):
    for nsamp in (5, 256, 257):
        M = _matrix(K, nsamp)
        S = K * nsamp
        for k_lo, k_hi in _ranks(S) + [(S // 3 + 1, S // 2 + 1)]:
            _m, lo, hi = _capi.wquantile_raw(M, np.full(K, 1.0 / K), K, k_lo, k_hi, gpu)
            assert hc.same_bits(lo, dr.emu_order_stat(M.T, k_lo)) and hc.same_bits(hi, dr.emu_order_stat(M.T, k_hi)), (K, nsamp, k_lo, k_hi)


def test_wquantile_refusals(gpu):
    x = np.zeros((2, 6))
    L = _capi.lib()
    out = [np.empty(2) for _ in range(3)]

    def call(m=2, K=2, ns=3, w=(0.5, 0.5), k_lo=1, k_hi=6, outs=(0, 1, 2), dev=gpu):
        wa = np.asarray(w, dtype=np.float64)
        ptr = [_capi._ptr(out[j]) if j in outs else None for j in range(3)]
        return L.bnr_wquantile(dev, m, K, ns, _capi._ptr(x), _capi._ptr(wa), k_lo, k_hi, *ptr)

    assert call() == _capi.BNR_OK
    for kw in (dict(w=(0.5, 0.6)), dict(w=(1.5, -0.5)), dict(w=(0.0, 0.0)), dict(w=(np.nan, 1.0)), dict(w=(np.inf, 0.0)), dict(w=(0.5, 0.5 + 1e-8)),
               dict(k_lo=0), dict(k_hi=7), dict(m=0), dict(ns=0), dict(K=0), dict(K=33, ns=1), dict(outs=()), dict(outs=(0, 1)), dict(outs=(2,)),
               dict(dev=9999)):
        assert call(**kw) == _capi.BNR_ERR_BAD_ARG, kw
    assert call(w=(0.5, 0.5 + 1e-10)) == _capi.BNR_OK and call(outs=(0,), k_lo=0) == _capi.BNR_OK      # (ranks are not read without the bounds)


# ------------------------------------------------------------------------------------------------------------------ bnr_chains_wsummary
W3 = (np.array([0.5, 0.3, 0.2]), np.array([1 / 3, 1 / 3, 1 / 3]), np.array([0.75, 0.0, 0.25]))


@pytest.mark.parametrize("first,nsamp", WINDOWS)
def test_wsummary_against_the_restatement(chains, first, nsamp):
    _load(chains, rc.tables())
    fetched = [ch.fetch() for ch in chains]
    for w in W3:
        got = api.device_summary_stacked(chains, w, first - 1, nsamp)
        want = api._host_summary_stacked(fetched, w, first - 1, nsamp)
        for f in ("estimate", "lower_bound", "upper_bound", "probability"):
            assert hc.same_bits(got[f], want[f]), (first, nsamp, tuple(w), f)
        assert got["estimate"].shape == (dr.Q,) and got["probability"].shape == (dr.V,)
    S = 3 * nsamp
    for k in range(3):                                                      # w = e_k: chain k's own mean and prob_xi; the ceil(r / K)-th draws
        for k_lo, k_hi in _ranks(S):
            mean, lo, hi, pxi = _capi.stacked_summary(chains, np.eye(3)[k], first, nsamp, k_lo, k_hi)
            a, b = int(np.ceil(k_lo / 3)), int(np.ceil(k_hi / 3))
            m1, l1, h1, p1 = chains[k].summary(first, nsamp, a, b)
            assert hc.same_bits(mean, m1) and hc.same_bits(pxi, p1) and hc.same_bits(lo, l1) and hc.same_bits(hi, h1), (k, k_lo, k_hi)
    k_lo, k_hi = api._summary_ranks(2 * nsamp, 95)                           # two chains at 1/2 each: the pooled order statistics
    _m, lo, hi, _p = _capi.stacked_summary(chains[:2], [0.5, 0.5], first, nsamp, k_lo, k_hi)
    _m2, lo2, hi2, _p2 = _capi.pooled_summary(chains[:2], first, nsamp, k_lo, k_hi)
    assert hc.same_bits(lo, lo2) and hc.same_bits(hi, hi2)


def _state(chains):
    return [ch.fetch() for ch in chains], [ch.iter for ch in chains], [np.array(ch.counters()) for ch in chains]


def _unchanged(chains, state):
    before, iters, counters = state
    for ch, b, it, cn in zip(chains, before, iters, counters):
        after = ch.fetch()
        assert ch.iter == it and np.array_equal(np.array(ch.counters()), cn)
        for k in b:
            assert np.array_equal(b[k].view(np.uint64), after[k].view(np.uint64)), k


def test_wsummary_blocks_and_side_effects(chains):
    _load(chains, rc.tables())
    state = _state(chains)
    first, nsamp = 38, 601
    k_lo, k_hi = api._summary_ranks(3 * nsamp, 95)
    base = _capi.stacked_summary(chains, W3[0], first, nsamp, k_lo, k_hi)
    try:
        for blk in (1, 7, 0):
            chains[0].set_option("summary_block_cols", blk)
            for a, b in zip(base, _capi.stacked_summary(chains, W3[0], first, nsamp, k_lo, k_hi)):
                assert hc.same_bits(a, b), blk
    finally:
        chains[0].set_option("summary_block_cols", 0)
    _unchanged(chains, state)


# ------------------------------------------------------------------------------------------------------------------ bnr_chains_wpredict
def _exact_tables():
    return [pr.craft_exact(dict(t), 300 + c, pr.CHAIN_OFFSET * c, tau_lo=0.5, tau_hi=20.0) for c, t in enumerate(_copies(rc.tables()))]


def _copies(tabs):
    return [{k: v.copy() for k, v in t.items()} for t in tabs]


@pytest.mark.parametrize("m", (1, 17, 33))
def test_wpredict_against_the_restatement(chains, m):
    tabs = _exact_tables()
    _load(chains, tabs)
    state = _state(chains)
    first, nsamp = 38, 101
    S = 3 * nsamp
    X = pr.exact_X(m, dr.Q, 1600 + m)
    g, mu, tau2 = pr.window(tabs, first, nsamp)
    E = pr.exact_eta(X, g, mu)                                              # exactly representable: the device's eta bit for bit
    y = E[:, ::7].mean(axis=1) + np.linspace(-1.0, 1.0, m)
    k_lo, k_hi = api._summary_ranks(S, 95)
    seed = 0xC0FFEE
    for w in W3 + (np.array([0.0, 1.0, 0.0]),):
        mean, lo, hi, lpd, plo, phi = _capi.stacked_predict(chains, w, X, first, nsamp, k_lo, k_hi, y=y, pred_seed=seed)
        want = api._host_predict_stacked(tabs, w, X, y, first - 1, nsamp, pred_seed=seed, eta=E)
        assert hc.same_bits(mean, want.estimate) and hc.same_bits(lo, want.lower_bound) and hc.same_bits(hi, want.upper_bound), (m, tuple(w))
        # the predictive bounds: the device's noise is within KZ_MEASURED ulps of the host's, every draw of y~ within the bound of
        # test_pooled_gpu.py (eta exact here: B = 0), and a weighted order statistic moves by no more than the largest move of a draw
        sz = np.sqrt(tau2)[None, :] * _capi.host_pred_noise(seed, 0, S, 0, m)
        bound = (U * (4 * np.abs(E) + (4 + 4 * KZ_MEASURED) * np.abs(sz))).max(axis=1)
        dl, dh = np.abs(plo - want.pred_lower_bound), np.abs(phi - want.pred_upper_bound)
        print("m=%d w=%s: predictive bounds, worst error / bound %.3g, %.3g" % (m, tuple(w), np.max(dl / bound), np.max(dh / bound)))
        assert np.all(dl <= bound) and np.all(dh <= bound)
        # lpd: the weighted log-sum-exp of the chains' own lpds
        per = np.array([ch.predict(X, first, nsamp, 1, nsamp, y=y)[3] for ch in chains])
        ref = api._weighted_lse(per, w)
        assert np.all(np.abs(lpd - ref) <= 1e-13 * np.abs(ref)), np.max(np.abs(lpd - ref) / np.abs(ref))
        assert np.all(np.abs(lpd - want.lpd) <= 1e-10 * np.abs(want.lpd) + 1e-13)      # (and near the float64 restatement, as test_pooled_gpu.py asks)
        # without y, without the predictive bounds: the same bits
        m2, l2, h2, none, p2, p3 = _capi.stacked_predict(chains, w, X, first, nsamp, k_lo, k_hi)
        assert none is None and p2 is None and p3 is None and hc.same_bits(m2, mean) and hc.same_bits(l2, lo) and hc.same_bits(h2, hi)
    base = _capi.stacked_predict(chains, W3[0], X, first, nsamp, k_lo, k_hi, y=y, pred_seed=seed)
    try:
        for blk in (32, 0):
            chains[0].set_option("predict_block_rows", blk)
            for a, b in zip(base, _capi.stacked_predict(chains, W3[0], X, first, nsamp, k_lo, k_hi, y=y, pred_seed=seed)):
                assert hc.same_bits(a, b), blk
    finally:
        chains[0].set_option("predict_block_rows", 0)
    p = api.device_predict_stacked(chains, W3[0], first - 1, nsamp, X, y, pred_seed=seed)
    assert hc.same_bits(p.estimate, base[0]) and hc.same_bits(p.pred_upper_bound, base[5]) and p.draws == S and p.pit is None
    _unchanged(chains, state)


# ------------------------------------------------------------------------------------------------------------------ bnr_chains_stack
def _fit_tables(shift=(0.0, 0.0, 0.5), seed=77):
    """tables whose draws scatter around the truth of the chains' training data; chain c's gamma shifted by shift[c]"""
    truth = bnr_amd.make_synthetic(dr.N, dr.V, dr.R, seed=3)[2]
    tabs = _copies(rc.tables())
    for c, t in enumerate(tabs):
        rng = np.random.default_rng([seed, c])
        t["gamma"][:, :, 0] = truth["B"][None, :] + shift[c] + 0.05 * rng.standard_normal((dr.TOT, dr.Q))
        t["mu"][:, 0, 0] = 10.0 + 0.1 * rng.standard_normal(dr.TOT)
        t["tau2"][:, 0, 0] = np.exp(0.2 * rng.standard_normal(dr.TOT))
    return tabs


@pytest.mark.parametrize("first,nsamp", WINDOWS)
def test_stack_against_the_single_chain_loo(chains, first, nsamp):
    _load(chains, _fit_tables())
    state = _state(chains)
    for r_eff in (None, 0.5):
        w, el, kh, es, gap, it = _capi.chains_stack(chains, first, nsamp, r_eff)
        for k, ch in enumerate(chains):
            _lpd, e1, k1 = ch.loo(first, nsamp, r_eff)
            assert hc.same_bits(el[k], e1) and hc.same_bits(kh[k], k1), (k, r_eff)
        assert np.isfinite(el).all() and abs(w.sum() - 1) <= 1e-12 and np.all(w >= 0) and gap <= 1e-9 and it >= 1
        assert w[2] <= 1e-6, w                                              # the shifted chain fits y clearly worse
        ref = api._host_stacking_weights(el.T)
        fw = lambda v: float(np.mean(api._weighted_lse(el, v)))
        print("window (%d, %d) r_eff %s: weights %s, %d updates, gap %.3g; restatement %s" % (first, nsamp, r_eff, w, it, gap, ref["weights"]))
        if np.max(np.abs(w - ref["weights"])) > 1e-8:                        # (only if the instance is not strictly concave: compare f)
            assert abs(fw(w) - fw(ref["weights"])) <= 1e-9
        want = api._weighted_lse(el, w)
        assert np.all(np.abs(es - want) <= 1e-13 * np.abs(want))
        st = api.device_stack_chains(chains, first - 1, nsamp, r_eff)
        assert np.array_equal(st.weights, w) and hc.same_bits(st.elpd_chain_i, el) and hc.same_bits(st.pareto_k, kh) and hc.same_bits(st.elpd_stack_i, want)
        assert st.n_used == dr.N and st.chains == 3 and st.draws == 3 * nsamp and st.elpd_stack >= st.elpd_uniform
    # one chain: weight 1, no update; max_iter = 1: not an error
    w1, el1, _k, es1, gap1, it1 = _capi.chains_stack(chains[:1], first, nsamp)
    assert np.array_equal(w1, [1.0]) and it1 == 0 and gap1 <= 1e-9 and hc.same_bits(es1, el1[0])
    w2, _e, _k, _s, gap2, it2 = _capi.chains_stack(chains, first, nsamp, max_iter=1)
    assert it2 == 1 and gap2 > 1e-9 and abs(w2.sum() - 1) <= 1e-12
    _unchanged(chains, state)


def test_stack_leaves_out_a_row_that_is_not_finite(gpu):
    X, y, _ = bnr_amd.make_synthetic(dr.N, dr.V, dr.R, seed=3)
    y = y.copy()
    y[5] = np.inf                                                           # its log-likelihood is -Inf in every draw
    cs = [bnr_amd.Chain(X, y, dr.R, dr.TOT, 99, 1, device=gpu)]
    cs += [bnr_amd.Chain.like(cs[0], 99, c) for c in (2, 3)]
    try:
        _load(cs, _fit_tables())
        w, el, kh, es, gap, it = _capi.chains_stack(cs, 38, 601)
        assert np.isnan(es[5]) and not np.isfinite(el[:, 5]).any() and np.isfinite(np.delete(es, 5)).all()
        keep = np.arange(dr.N) != 5
        ref = api._host_stacking_weights(el[:, keep].T)
        assert np.max(np.abs(w - ref["weights"])) <= 1e-8 and gap <= 1e-9
        st = api.device_stack_chains(cs, 37, 601)
        assert st.n_used == dr.N - 1 and np.isnan(st.elpd_stack_i[5]) and np.isfinite(st.elpd_stack)
    finally:
        for c in cs:
            c.close()


# ------------------------------------------------------------------------------------------------------------------ refusals
def test_chain_call_refusals(chains):
    _load(chains, _fit_tables())
    state = _state(chains)
    X = pr.exact_X(3, dr.Q, 5)
    w = W3[0]
    calls = lambda cs, ww=w, first=1, ns=100: (lambda: _capi.chains_stack(cs, first, ns),
                                               lambda: _capi.stacked_summary(cs, ww, first, ns, 1, ns),
                                               lambda: _capi.stacked_predict(cs, ww, X, first, ns, 1, ns))

    def refused(call):
        with pytest.raises(bnr_amd.BnrError) as e:
            call()
        assert e.value.code == _capi.BNR_ERR_BAD_ARG
        return str(e.value)

    for kw in (dict(first=600, ns=100), dict(first=0, ns=100), dict(first=1, ns=0)):
        for call in calls(chains, **kw):
            refused(call)
    for call in calls([chains[0], chains[1], chains[0]]):
        refused(call)
    many = [chains[j % 3] for j in range(33)]                               # K = 33
    refused(lambda: _capi.chains_stack(many, 1, 100))
    refused(lambda: _capi.stacked_summary(many, np.full(33, 1 / 33), 1, 100, 1, 100))
    for bad in ([0.5, 0.3, 0.3], [1.5, -0.25, -0.25], [0.0, 0.0, 0.0], [np.nan, 0.5, 0.5], [0.5, 0.5, 1e-8]):
        for call in calls(chains, np.array(bad))[1:]:
            refused(call)
    refused(lambda: _capi.stacked_summary(chains, w, 1, 100, 0, 300))
    refused(lambda: _capi.stacked_summary(chains, w, 1, 100, 1, 301))
    refused(lambda: _capi.chains_stack(chains, 1, 100, max_iter=0))
    refused(lambda: _capi.chains_stack(chains, 1, 100, gap_tol=0.0))
    with pytest.raises(ValueError):
        _capi.stacked_summary(chains, [0.5, 0.5], 1, 100, 1, 300)
    with pytest.raises(ValueError):
        _capi.chains_stack(chains, 1, 100, r_eff=-1.0)
    # a pending asynchronous run on a member: refused, and the run completes as usual afterwards
    lone = bnr_amd.Chain.like(chains[0], 99, 4)
    try:
        lone.init_prior()
        lone.run_async(2, dr.TOT, 4)
        try:
            for cs in ([chains[0], lone], [lone, chains[0]]):
                for call in calls(cs, np.array([0.5, 0.5])):
                    assert "pending" in refused(call)
        finally:
            lone.sync()
    finally:
        lone.close()
    _unchanged(chains, state)


# ------------------------------------------------------------------------------------------------------------------ Fit
def test_fit_fills_stacking(gpu, tmp_path):
    X, y, _ = bnr_amd.make_synthetic(dr.N, dr.V, dr.R, seed=5)
    Xn, yn, _ = bnr_amd.make_synthetic(6, dr.V, dr.R, seed=6)
    kw = dict(nburn=40, nsamples=100, num_chains=3, seed=17, x_transform=False, suppress_timer=True, psrf_cutoff=np.inf, return_state=False,
              filename=str(tmp_path / "parameters.log"), device=gpu, summary_interval=95, predict_X=Xn, predict_y=yn)
    res = bnr_amd.Fit(X, y, dr.R, stack_chains=True, **kw)
    plain = bnr_amd.Fit(X, y, dr.R, **kw)
    st = res.stacking
    assert isinstance(st, bnr_amd.ChainStacking) and plain.stacking is None and bnr_amd.Stacking(res) is st
    assert st.weights.shape == (3,) and abs(st.weights.sum() - 1) <= 1e-12 and np.all(st.weights >= 0) and (st.chains, st.draws) == (3, 300)
    assert st.elpd_chain_i.shape == st.pareto_k.shape == (3, dr.N) and st.n_high_k.shape == (3,) and st.gap <= 1e-9
    assert st.summary["estimate"].shape == (dr.Q,) and st.summary["probability"].shape == (dr.V,) and st.summary["interval"] == 95
    assert st.prediction.estimate.shape == (6,) and st.prediction.lpd.shape == (6,) and st.prediction.draws == 300
    for f in ("estimate", "lower_bound", "upper_bound", "probability"):      # what the default returns is not changed
        assert hc.same_bits(res.summary_device[f], plain.summary_device[f]), f
    for f in ("estimate", "lower_bound", "upper_bound", "lpd"):
        assert hc.same_bits(getattr(res.prediction, f), getattr(plain.prediction, f)), f
    assert res.stat_chains == plain.stat_chains == 1
    pooled = bnr_amd.Fit(X, y, dr.R, stack_chains=True, pool_chains=True, **kw)
    pooled_plain = bnr_amd.Fit(X, y, dr.R, pool_chains=True, **kw)
    for f in ("estimate", "lower_bound", "upper_bound", "probability"):      # ... nor what pool_chains returns
        assert hc.same_bits(pooled.summary_device[f], pooled_plain.summary_device[f]), f
    assert np.array_equal(pooled.stacking.weights, st.weights)
    # the same chains again, kept alive: the fit's summary and prediction are device_summary_stacked / device_predict_stacked on them
    keep = []
    gs = dict(kw, nsamp=kw["nsamples"], maxburn=kw["nburn"] + kw["nsamples"])
    for k in ("nsamples", "filename"):
        gs.pop(k)
    r2 = bnr_amd.generate_samples(X, y, dr.R, stack_chains=True, _keep=keep, **gs)
    try:
        cs = [keep[0].chains[c] for c in keep[0].ids]
        assert np.array_equal(r2.stacking.weights, st.weights)
        s = api.device_summary_stacked(cs, st.weights, 40, 100, 95)
        for f in ("estimate", "lower_bound", "upper_bound", "probability"):
            assert hc.same_bits(st.summary[f], s[f]) and hc.same_bits(r2.stacking.summary[f], s[f]), f
        p = api.device_predict_stacked(cs, st.weights, 40, 100, Xn, yn, predict_observation=False)
        for f in ("estimate", "lower_bound", "upper_bound", "lpd"):
            assert hc.same_bits(getattr(st.prediction, f), getattr(p, f)), f
        host = api._host_summary_stacked([c.fetch() for c in cs], st.weights, 40, 100, 95)
        for f in ("estimate", "lower_bound", "upper_bound", "probability"):
            assert hc.same_bits(host[f], s[f]), f
    finally:
        keep[0].close()
