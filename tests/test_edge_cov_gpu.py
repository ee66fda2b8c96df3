"""GPU tests of the posterior covariance of the edge coefficients (ABI 17; run with -m gpu on an MI355X): k_cov and k_cov_finish alone
(bnr_cov on integer draws against the exact arithmetic of tests/cov_ref.py, bit for bit; the same draws shifted by 1e8; random draws of mixed
scales against the long-double restatement), bnr_chains_cov / bnr_chain_cov on live chains, the bitwise properties, non-finite columns, the
refusals and Fit(..., edge_cov=...).

Bounds.  On the integer cases every difference, product and partial sum is an integer below 2^53 (|x - c| <= 2^11, at most 195 products of
at most 2^22), the weights are dyadic and nsamp a power of two where there are weights: the only rounding is the last division, so the
result is float(Fraction).  Elsewhere |got - ref| <= (S + 8) 2^-52 sqrt(ref_aa ref_bb): S products and additions of relative error 2^-53
each in any order, the two differences, the weight and the division, against sum_s |d_sa d_sb| <= sqrt(sum d_sa^2 sum d_sb^2)
(Cauchy-Schwarz) -- the worst case, not a fitted figure; no entry is excluded."""
import ctypes as C
import functools

import numpy as np
import pytest

import bnr_amd
import cov_ref as cr
from bnr_amd import _capi, api

pytestmark = pytest.mark.gpu
LD = np.longdouble
V, R, N, TOT = 6, 2, 12, 50
Q = V * (V + 1) // 2
WINDOWS = ((4, 40), (7, 41))                                                 # (nburn, nsamp): first_row = nburn + 1
W3 = (np.array([0.5, 0.25, 0.25]), np.array([0.2, 0.3, 0.5]), np.array([0.0, 1.0, 0.0]))


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def within_bound(got, ref, S):
    ref = np.asarray(ref, dtype=LD)
    d = np.sqrt(np.diag(ref))
    bound = LD(S + 8) * LD(2.0) ** -52 * np.outer(d, d)
    err = np.abs(np.asarray(got, dtype=LD) - ref)
    return bool(np.all(err <= bound)), float(np.max(err / np.where(bound > 0, bound, 1)))


@functools.lru_cache(maxsize=None)
def _exact(K, ns, m, w):
    """(the draws, the exact centres and covariance rounded once to float64) of an integer case: computed once, shared by the tests"""
    x = cr.integer_case(K, ns, m, w)
    c, _G, cov = cr.exact(x, w)
    x.setflags(write=False)
    return x, cr.as_float(c), cr.as_float(cov)


# ------------------------------------------------------------------------------------------------------------------ the kernels alone
@pytest.mark.parametrize("K", cr.KS)
def test_integer_draws_are_exact(gpu, K):
    for KK, ns, m, w in cr.integer_cases():
        if KK != K:
            continue
        x, c, cov = _exact(K, ns, m, w)
        mean, got = _capi.cov_raw(x.reshape(K * ns, m), K, w, gpu)
        assert same_bits(mean, c), (K, ns, m, w, "mean")
        assert same_bits(got, cov), (K, ns, m, w, np.argwhere(got.view(np.uint64) != cov.view(np.uint64))[:4].tolist())


@pytest.mark.parametrize("K", cr.KS)
def test_columns_shifted_by_1e8_give_the_same_covariance(gpu, K):
    for KK, ns, m, w in cr.integer_cases():
        if KK != K:
            continue
        x, c, cov = _exact(K, ns, m, w)
        shift = np.where(np.arange(m) % 3 == (0 if m < 3 else 1), 1e8, 0.0)
        mean, got = _capi.cov_raw((x + shift).reshape(K * ns, m), K, w, gpu)
        assert same_bits(mean, c + shift), (K, ns, m, w, "mean")
        assert same_bits(got, cov), (K, ns, m, w, np.argwhere(got.view(np.uint64) != cov.view(np.uint64))[:4].tolist())


def _mixed(K, ns, m, seed):
    rng = np.random.default_rng([23, K, ns, m, seed])
    x = rng.standard_normal((K, ns, m)) * np.logspace(-6, 6, m)[None, None, :] + rng.standard_normal((K, 1, m)) * np.logspace(-6, 6, m)[None, None, :]
    x[:, :, m // 2] = 1e8 + rng.standard_normal((K, ns))
    return x


@pytest.mark.parametrize("K,ns,m", [(1, 65, 33), (3, 65, 33), (2, 1000, 17), (3, 64, 130)])
def test_mixed_scales_against_long_double(gpu, K, ns, m):
    x = _mixed(K, ns, m, 0)
    for w in (None,) + ((W3[0], W3[1]) if K == 3 else ((np.array([0.7, 0.3]),) if K == 2 else ())):
        mean, got = _capi.cov_raw(x.reshape(K * ns, m), K, w, gpu)
        c, ref = api._host_cov(x, w, dtype=LD)
        assert same_bits(mean, c), (K, ns, m, w)
        ok, worst = within_bound(got, ref, K * ns)
        print("mixed scales K=%d nsamp=%d m=%d weights=%s: worst error / bound = %.3g" % (K, ns, m, None if w is None else w.tolist(), worst))
        assert ok, (K, ns, m, w, worst)
        assert same_bits(got, got.T)
        d = bnr_amd.cov(x.reshape(K * ns, m), K, w, device=gpu)
        assert same_bits(d["cov"], got) and same_bits(d["mean"], mean)


def test_wide_matrix_takes_the_large_tiles(gpu):
    """from 512 workgroup tiles of 128 x 128 on (here 3 chains x 190 tiles) the call runs k_cov<4>, below k_cov<2>: the same sums, so a narrow
    call reproduces the entries of the wide one bit for bit, and the wide one meets the bound"""
    K, ns, m = 3, 5, 2305
    x = _mixed(K, ns, m, 2)
    for w in (None, W3[1]):
        mean, got = _capi.cov_raw(x.reshape(K * ns, m), K, w, gpu)
        c, ref = api._host_cov(x, w, dtype=LD)
        ok, worst = within_bound(got, ref, K * ns)
        assert same_bits(mean, c) and ok, (w, worst)
        assert same_bits(got, got.T)
        for cols in (np.arange(0, 40), np.arange(2290, 2305), np.array([5, 2304, 1152, 127, 128, 1151, 2176, 2175])):
            _m, sub = _capi.cov_raw(np.ascontiguousarray(x[:, :, cols]).reshape(K * ns, cols.size), K, w, gpu)
            assert same_bits(sub, got[np.ix_(cols, cols)]), (w, cols[:3])


def test_non_finite_columns_of_a_matrix(gpu):
    K, ns, m = 2, 37, 35
    x = _mixed(K, ns, m, 1)
    for w in (None, np.array([0.25, 0.75]), np.array([1.0, 0.0])):
        clean = _capi.cov_raw(x.reshape(K * ns, m), K, w, gpu)[1]
        y = x.copy()
        y[1, 36, 3] = np.nan                                                 # the last draw: beside the zero padding of the K tail
        y[0, 5, 17] = np.inf
        y[1, 0, 34] = -np.inf                                                # the last column: beside the zero padding of the column tail
        got = _capi.cov_raw(y.reshape(K * ns, m), K, w, gpu)[1]
        bad = np.zeros((m, m), dtype=bool)
        bad[[3, 17, 34], :] = True
        bad[:, [3, 17, 34]] = True
        assert np.isnan(got[bad]).all() and same_bits(got[~bad], clean[~bad]), w


# ------------------------------------------------------------------------------------------------------------------ live chains
@pytest.fixture(scope="module")
def chains(gpu):
    X, y, _ = bnr_amd.make_synthetic(N, V, R, seed=11)
    cs = [bnr_amd.Chain(X, y, R, TOT, 77, 1, device=gpu)]
    cs += [bnr_amd.Chain.like(cs[0], 77, c) for c in (2, 3)]
    for c in cs:
        c.init_prior()
        c.run(2, TOT, TOT)
    yield cs
    for c in cs:
        c.close()


def _state(chains):
    return [(c.fetch(), c.iter, c.counters()) for c in chains]


def _unchanged(chains, state):
    for c, (t, it, cnt) in zip(chains, state):
        now = c.fetch()
        assert c.iter == it and c.counters() == cnt
        for k in _capi.TABLE_COLUMNS:
            assert same_bits(now[k], t[k]), k


def test_live_chains_against_the_tables(chains):
    state = _state(chains)
    tabs = [s[0] for s in state]
    for nburn, ns in WINDOWS:
        for cs, tb in ((chains, tabs), (chains[:1], tabs[:1]), (chains[1:], tabs[1:])):
            K = len(cs)
            for w in (None,) + (W3 if K == 3 else ()):
                got = api.device_edge_cov(cs, nburn, ns, weights=w)
                ref = api._host_edge_cov(tb, nburn, ns, weights=w, dtype=LD)
                ok, worst = within_bound(got.cov, ref.cov, K * ns)
                print("live chains K=%d window=(%d, %d) weights=%s: worst error / bound = %.3g" % (K, nburn, ns, None if w is None else w.tolist(), worst))
                assert ok, (K, nburn, ns, w, worst)
                assert same_bits(got.mean, ref.mean) and got.cov.shape == (Q, Q) and (got.chains, got.draws) == (K, K * ns)
                if w is None:
                    summ = api.device_summary_pooled(cs, nburn, ns) if K > 1 else api.device_summary(cs[0], nburn, ns)
                else:
                    summ = api.device_summary_stacked(cs, w, nburn, ns)
                assert same_bits(got.mean, summ["estimate"]), (K, nburn, ns, w)
    _unchanged(chains, state)


def test_bitwise_properties(gpu, chains):
    state = _state(chains)
    nburn, ns = WINDOWS[1]
    for w in (None, W3[1]):
        full = api.device_edge_cov(chains, nburn, ns, weights=w)
        assert same_bits(full.cov, full.cov.T)
        again = api.device_edge_cov(chains, nburn, ns, weights=w)
        assert same_bits(again.cov, full.cov) and same_bits(again.mean, full.mean)
        cols = [20, 3, 17, 3, 0, 16, 15]                                     # a subset, permuted, with a duplicate
        sub = api.device_edge_cov(chains, nburn, ns, cols=cols, weights=w)
        assert same_bits(sub.cov, full.cov[np.ix_(cols, cols)]) and same_bits(sub.mean, full.mean[cols]) and np.array_equal(sub.cols, cols)
        one = api.device_edge_cov(chains, nburn, ns, cols=[7], weights=w)
        assert same_bits(one.cov, full.cov[7:8, 7:8])
        try:
            for blk in (16, 32, 1, 5):
                chains[0].set_option("cov_block_cols", blk)
                b = api.device_edge_cov(chains, nburn, ns, weights=w)
                assert same_bits(b.cov, full.cov) and same_bits(b.mean, full.mean), blk
                bs = api.device_edge_cov(chains, nburn, ns, cols=cols, weights=w)
                assert same_bits(bs.cov, sub.cov), blk
        finally:
            chains[0].set_option("cov_block_cols", 0)
    # one chain: the pooled call on a list of one is bnr_chain_cov
    m1, c1 = chains[1].cov(nburn + 1, ns)
    m2, c2 = _capi.pooled_cov(chains[1:2], nburn + 1, ns)
    assert same_bits(m1, m2) and same_bits(c1, c2)
    m3, c3 = chains[1].cov(nburn + 1, ns, cols=[4, 2])
    assert same_bits(c3, c1[np.ix_([4, 2], [4, 2])]) and same_bits(m3, m1[[4, 2]])
    # the same draws as a caller's matrix: the same sums
    x = np.concatenate([s[0]["gamma"][nburn:nburn + ns, :, 0] for s in state], axis=0)
    mm, cm = _capi.cov_raw(x, 3, None, gpu)
    full = api.device_edge_cov(chains, nburn, ns)
    assert same_bits(cm, full.cov) and same_bits(mm, full.mean)
    _unchanged(chains, state)


def test_non_finite_columns_of_a_chain(chains):
    state = _state(chains)
    nburn, ns = WINDOWS[0]
    try:
        for w in (None, W3[0]):
            clean = api.device_edge_cov(chains, nburn, ns, weights=w).cov
            t = {k: v.copy(order="F") for k, v in state[1][0].items()}
            t["gamma"][nburn + ns - 1, 2, 0] = np.nan                        # the window's last row
            t["gamma"][nburn, 20, 0] = np.inf                                # the last column, the window's first row
            t["gamma"][nburn - 1, 9, 0] = np.nan                             # outside the window: must not matter
            chains[1].load(t)
            got = api.device_edge_cov(chains, nburn, ns, weights=w).cov
            bad = np.zeros((Q, Q), dtype=bool)
            bad[[2, 20], :] = True
            bad[:, [2, 20]] = True
            assert np.isnan(got[bad]).all() and same_bits(got[~bad], clean[~bad]), w
            chains[1].load(state[1][0])
    finally:
        chains[1].load(state[1][0])
    for c, (t, _it, _cnt) in zip(chains, state):
        now = c.fetch()
        for k in _capi.TABLE_COLUMNS:
            assert same_bits(now[k], t[k]), k


def test_refusals(chains):
    state = _state(chains)
    L = chains[0].L
    arr = (C.c_void_p * 3)(*[c.h for c in chains])
    mean, cov = np.empty(Q), np.empty((Q, Q))
    p = _capi._ptr

    def refused(code):
        assert code == _capi.BNR_ERR_BAD_ARG, code

    idx = lambda v: np.ascontiguousarray(v, dtype=np.int32)
    for first, ns in ((TOT, 2), (0, 10), (1, 0), (1, TOT + 1)):
        refused(L.bnr_chains_cov(arr, 3, None, first, ns, Q, None, p(mean), p(cov)))
        refused(L.bnr_chain_cov(chains[0].h, first, ns, Q, None, p(mean), p(cov)))
    refused(L.bnr_chain_cov(chains[0].h, 5, 1, Q, None, p(mean), p(cov)))                                           # S = 1
    refused(L.bnr_chains_cov(arr, 3, None, 1, 10, Q - 1, None, p(mean), p(cov)))                                    # cols == NULL with ncols != q
    refused(L.bnr_chains_cov(arr, 3, None, 1, 10, 0, p(idx([0])), p(mean), p(cov)))
    for bad in ([Q], [-1], [0, 3, Q]):
        refused(L.bnr_chains_cov(arr, 3, None, 1, 10, len(bad), p(idx(bad)), p(mean), p(cov)))
    twice = (C.c_void_p * 3)(chains[0].h, chains[1].h, chains[0].h)
    refused(L.bnr_chains_cov(twice, 3, None, 1, 10, Q, None, p(mean), p(cov)))
    for bad in ([0.5, 0.3, 0.3], [1.5, -0.25, -0.25], [0.0, 0.0, 0.0], [np.nan, 0.5, 0.5], [0.5, 0.5, 1e-8]):
        refused(L.bnr_chains_cov(arr, 3, p(np.array(bad)), 1, 10, Q, None, p(mean), p(cov)))
    many = (C.c_void_p * 33)(*[chains[j % 3].h for j in range(33)])
    refused(L.bnr_chains_cov(many, 33, p(np.full(33, 1 / 33)), 1, 10, Q, None, p(mean), p(cov)))
    with pytest.raises(ValueError):
        api.device_edge_cov(chains, 0, 10, cols=[Q])
    with pytest.raises(ValueError):
        api.device_edge_cov(chains, 0, 10, weights=[0.5, 0.5])
    with pytest.raises(bnr_amd.BnrError):
        chains[0].set_option("cov_block_cols", -1)
    _unchanged(chains, state)


# ------------------------------------------------------------------------------------------------------------------ Fit
def test_fit_fills_edge_cov(gpu, tmp_path):
    X, y, _ = bnr_amd.make_synthetic(N, V, R, seed=5)
    kw = dict(nburn=20, nsamples=40, num_chains=3, seed=17, x_transform=False, suppress_timer=True, psrf_cutoff=np.inf, return_state=False,
              filename=str(tmp_path / "parameters.log"), device=gpu, summary_interval=95)
    res = bnr_amd.Fit(X, y, R, edge_cov=True, stack_chains=True, **kw)
    plain = bnr_amd.Fit(X, y, R, **kw)
    ec = res.edge_cov
    assert isinstance(ec, bnr_amd.EdgeCov) and bnr_amd.EdgeCov(res) is ec and plain.edge_cov is None
    assert ec.cov.shape == (Q, Q) and ec.mean.shape == (Q,) and (ec.chains, ec.draws) == (3, 120) and ec.weights is None
    assert np.array_equal(ec.cols, np.arange(Q)) and same_bits(ec.cov, ec.cov.T) and np.all(np.diag(ec.cov) >= 0)
    sc = res.stacking.edge_cov
    assert isinstance(sc, bnr_amd.EdgeCov) and np.array_equal(sc.weights, res.stacking.weights) and sc.cov.shape == (Q, Q)
    assert same_bits(sc.mean, res.stacking.summary["estimate"])
    for f in ("estimate", "lower_bound", "upper_bound", "probability"):      # the Summary of a fit is what it was without the keyword
        assert same_bits(res.summary_device[f], plain.summary_device[f]), f
    with pytest.raises(ValueError, match="edge_cov"):
        bnr_amd.EdgeCov(plain)                                               # no numbers from the device, no state
    only = bnr_amd.Fit(X, y, R, edge_cov=[(1, 2), (3, 2), (6, 6)], **kw)
    assert only.stacking is None and np.array_equal(only.edge_cov.cols, [1, 7, 20])
    assert np.array_equal(only.edge_cov.node1, [1, 2, 6]) and np.array_equal(only.edge_cov.node2, [2, 3, 6])
    assert same_bits(only.edge_cov.cov, ec.cov[np.ix_([1, 7, 20], [1, 7, 20])])
    # the same chains again, kept alive: the fit's numbers are device_edge_cov on them, and the pooled Summary's means
    keep = []
    gs = dict(kw, nsamp=kw["nsamples"], maxburn=kw["nburn"] + kw["nsamples"])
    for k in ("nsamples", "filename"):
        gs.pop(k)
    r2 = bnr_amd.generate_samples(X, y, R, edge_cov=np.array([0, 5, 5]), _keep=keep, **gs)
    try:
        cs = [keep[0].chains[c] for c in keep[0].ids]
        d = api.device_edge_cov(cs, 20, 40, cols=[0, 5, 5])
        assert same_bits(r2.edge_cov.cov, d.cov) and same_bits(d.cov, ec.cov[np.ix_([0, 5, 5], [0, 5, 5])])
        assert same_bits(ec.mean, api.device_summary_pooled(cs, 20, 40)["estimate"])
        host = api._host_edge_cov([c.fetch() for c in cs], 20, 40, dtype=LD)
        ok, worst = within_bound(ec.cov, host.cov, 120)
        assert ok, worst
    finally:
        keep[0].close()
