"""GPU tests of marginal PSIS-LOO (include/bnr_mloo.h, libbnr_mloo.so; kernels in csrc/bnr_mloo_kernels.h): the raw call against the mpmath
reference within the derived bound (tests/mloo_ref.py) at the edges of the 16-row MFMA tile, of the 4-deep K step and of the batch; against the
numpy restatement at the edges of the 32-row workgroup tile and through the 256-column passes of the factor kernel up to its limit; cases whose
answer is exact; the independence of a draw's bits from its batch, its neighbours and its place; bad draws; and live chains through Fit.

Past 256 rows (k_mloo_factor forms L^-1 in passes of 256 columns, every k loop of a pass from its first column i0, unrolled by 8, selecting 0.0
for k < i; a Cholesky thread owns the rows j + tid, j + tid + 256, ...; z, c and g are LDS arrays of MLOO_MAX_N = 2048):
  257   the second pass exists, with one column whose k loops run zero times
  258   the second pass has a column i > i0: the select k >= i first meets a slot that holds an entry of L (dense random L: every slot counts)
  300   44 columns in the second pass: full unrolled chunks and the remainder loop; the shape of the exact cases, of the independence from the
        batch, of the pivot that fails in a column j >= 256 and of the live chains (k_mloo_rhs: two workgroups along the rows)
  513   the third pass exists; a thread's third Cholesky row
  521   the third pass has nine columns, one full chunk and the remainder loop (also a shape of tests/mexact_ref.py, as is 265)
  2048  the limit: eight passes, eight rows per thread, the last element of zs, cs and gs
Measured on an MI355X: the call on one draw at n = 2048 takes 0.90 s (the estimate had been 1.1e7 dependent multiply-subtracts per thread in each of
the Cholesky and the inverse, unmeasured), test_the_largest_n 2.4 s with its second call and the restatement; no other case past 256 rows takes
more than 1.3 s.

Two choices the issue leaves open, and why:
  - the one-hot case uses S_e = 2^k - 1 with EVEN k: c_i comes from the columns of L^-1, L_ii = sqrt(1 + S_e) = 2^(k / 2) has to be a float64
    for 1 / L_ii, its square and the two divisions to be exact; an odd k rounds sqrt(2^k) and is then covered by the bound, not by equality.
  - logml "from the device's own resid and var" is checked where A is diagonal (X = 0, S = 0, one-hot rows): there log p(y | phi) = sum_i
    log p(y_i | y_-i, phi), c_i = tau2 / var_i, log L_ii = -log(c_i) / 2 and z_i^2 = resid_i^2 c_i.  Its allowance is the sum of the entries'
    allowances 16 eps (|log(2 pi var) / 2| + resid^2 / (2 var) + 1) plus n eps sum_i (|log(2 pi var_i) / 2| + resid_i^2 / (2 var_i)) for the n
    additions of each of the device's two sums."""
import math
import time

import numpy as np
import pytest

import bnr_amd
import mloo_ref as mr
from bnr_amd import _capi, api

pytestmark = pytest.mark.gpu
EPS = 2.0 ** -52
NAMES = ("loglik", "resid", "var", "logml")


def _call(c, draws, W=True, **kw):
    d = list(draws)
    r = bnr_amd.marginal_loglik(c["X"], c["y"], c["tau2"][d], c["mu"][d], c["S"][d], c["W"][d] if W else None, **kw)
    return r


def _same(a, b, cols_a=slice(None), cols_b=slice(None)):
    return all(np.array_equal(a[k][..., cols_a], b[k][..., cols_b], equal_nan=True) for k in NAMES)


# ------------------------------------------------------------------------------------------ against the mpmath reference
@pytest.mark.parametrize("ndraws", (1, 2, 5, 17))
@pytest.mark.parametrize("q", (1, 3, 4, 5, 15, 17, 45))
@pytest.mark.parametrize("n", (1, 2, 15, 16, 17, 33))
def test_raw_call_meets_the_bound_of_the_reference(gpu, n, q, ndraws):
    c = mr.case(n, q)
    r = _call(c, range(ndraws))
    assert r["n_bad"] == 0 and r["loglik"].shape == (n, ndraws) and r["logml"].shape == (ndraws,)
    worst, bl = mr.worst_ratios([r[k] for k in NAMES], n, q, range(ndraws))
    print("n=%d q=%d D=%d: error / bound %s, beta lam %.2e" % (n, q, ndraws, {k: "%.3g" % v for k, v in worst.items()}, bl))
    assert bl <= 0.1
    assert max(worst.values()) <= 2.0, worst


def test_raw_call_meets_the_bound_on_a_binary_matrix(gpu):
    for n, q in ((17, 45), (33, 17)):
        c = mr.case(n, q, True)
        r = _call(c, range(3))
        worst, bl = mr.worst_ratios([r[k] for k in NAMES], n, q, range(3), True)
        assert r["n_bad"] == 0 and bl <= 0.1 and max(worst.values()) <= 2.0, worst


# ------------------------------------------------------------------------------------------ against the numpy restatement
def _against_the_restatement(c, r, D):
    """the four outputs of a call on the first D draws of c against api._host_marginal_terms, each within its own gate of 2"""
    n, q = c["X"].shape
    h = api._host_marginal_terms(c["X"], c["y"], c["tau2"][:D], c["mu"][:D], c["S"][:D], c["W"][:D])
    assert r["n_bad"] == 0 and h[4] == 0
    worst = 0.0
    for d in range(D):
        b = mr.numpy_bounds(c["X"], c["y"], c["tau2"][d], c["mu"][d], c["S"][d], c["W"][d])
        assert b["beta_lam"] <= 0.1
        for j, name in enumerate(NAMES[:3]):
            ratio = np.abs(r[name][:, d] - h[j][:, d]) / b["tol_" + name]
            assert np.all(np.isfinite(r[name][:, d])) and np.all(ratio <= 4.0), (name, d, float(ratio.max()))      # each within its own gate of 2
            worst = max(worst, float(ratio.max()))
        ratio = abs(r["logml"][d] - h[3][d]) / b["tol_logml"]
        assert np.isfinite(r["logml"][d]) and ratio <= 4.0, ("logml", d, ratio)
        worst = max(worst, ratio)
    print("n=%d q=%d: worst difference / bound %.3g" % (n, q, worst))


# (258: the first column of the second pass with a k < i; 300: 44 columns; 513: the third pass, one column; 521: nine -- module docstring)
@pytest.mark.parametrize("n,q", [(n, q) for q in (64, 65, 300) for n in (64, 65, 128, 129, 257)] + [(258, 65), (300, 65), (513, 65), (521, 300)])
def test_raw_call_against_the_restatement(gpu, n, q):
    c = mr.case(n, q)
    _against_the_restatement(c, _call(c, range(3)), 3)


def test_the_largest_n(gpu):
    """n = 2048 = MLOO_MAX_N, q = 9, one draw: eight passes of the factor kernel, eight Cholesky rows per thread, and the last element of its
    three LDS arrays (2049 is refused: test_marginal_loo_host.py).  Against the restatement under the gates of
    test_raw_call_against_the_restatement, and with X = 0, where resid = y - mu and var = tau2 exactly at all 2048 rows.  0.90 s per call of one
    draw on an MI355X: two calls, one per library (the other is test_marginal_edges_gpu's), stay far below the 20 s at which they would be merged."""
    n, q = 2048, 9
    c = mr.case(n, q)
    t0 = time.perf_counter()
    r = _call(c, range(1))
    print("n=%d q=%d: one draw, the whole call, in %.2f s" % (n, q, time.perf_counter() - t0))
    _against_the_restatement(c, r, 1)
    r = bnr_amd.marginal_loglik(np.zeros((n, q)), c["y"], c["tau2"][:1], c["mu"][:1], c["S"][:1], c["W"][:1])
    assert r["n_bad"] == 0 and np.array_equal(r["resid"], c["y"][:, None] - c["mu"][None, :1]) and np.array_equal(r["var"], np.full((n, 1), c["tau2"][0]))
    _formula_checks(r, c["tau2"][:1], n)


# ------------------------------------------------------------------------------------------ exact cases
def _formula_checks(r, tau2, n):
    """loglik against its formula from the device's resid and var, and logml against the sum for a diagonal A (module docstring)"""
    rs, vr = r["resid"], r["var"]
    half = rs * rs / vr / 2
    allow = 16 * EPS * (np.abs(np.log(2 * np.pi * vr) / 2) + half + 1)
    want = -0.5 * (math.log(2 * math.pi) + np.log(vr)) - half
    assert np.all(np.abs(r["loglik"] - want) <= allow), float(np.max(np.abs(r["loglik"] - want) / allow))
    c = np.asarray(tau2)[None, :] / vr
    ml = -0.5 * n * np.log(2 * np.pi * np.asarray(tau2)) + 0.5 * np.sum(np.log(c), axis=0) - 0.5 * np.sum(rs * rs * c, axis=0) / np.asarray(tau2)
    allow_ml = allow.sum(axis=0) + n * EPS * np.sum(np.abs(np.log(2 * np.pi * vr) / 2) + half, axis=0)
    assert np.all(np.abs(r["logml"] - ml) <= allow_ml), float(np.max(np.abs(r["logml"] - ml) / allow_ml))


@pytest.mark.parametrize("n,q", ((1, 1), (17, 5), (33, 45), (65, 70), (300, 7), (513, 5), (300, 310)))
def test_exact_cases(gpu, n, q):
    c = mr.case(n, q)
    D = 5
    y, t2, mu = c["y"], c["tau2"][:D], c["mu"][:D]
    plain = y[:, None] - mu[None, :]
    r = bnr_amd.marginal_loglik(np.zeros((n, q)), y, t2, mu, c["S"][:D], c["W"][:D])               # X = 0
    assert r["n_bad"] == 0 and np.array_equal(r["resid"], plain) and np.array_equal(r["var"], np.tile(t2, (n, 1)))
    _formula_checks(r, t2, n)
    r = bnr_amd.marginal_loglik(c["X"], y, t2, mu, np.zeros((D, q)), None)                          # S = 0
    assert r["n_bad"] == 0 and np.array_equal(r["resid"], plain) and np.array_equal(r["var"], np.tile(t2, (n, 1)))
    _formula_checks(r, t2, n)
    if q >= n:                                                                                      # one-hot rows, S_e = 2^k - 1 with even k
        rng = np.random.default_rng([7, n, q])
        cols = rng.permutation(q)[:n]
        X = np.zeros((n, q))
        X[np.arange(n), cols] = 1.0
        k = 2 * rng.integers(0, 6, size=(D, q))
        r = bnr_amd.marginal_loglik(X, y, t2, mu, 2.0 ** k - 1.0, None)
        assert r["n_bad"] == 0 and np.array_equal(r["resid"], plain)
        assert np.array_equal(r["var"], t2[None, :] * 2.0 ** k[:, cols].T)                          # c_i = 2^-k exactly
        _formula_checks(r, t2, n)


# ------------------------------------------------------------------------------------------ independence
@pytest.fixture
def batch_option():
    yield lambda v: _capi.mloo_set_option("mloo_batch_draws", v)
    _capi.mloo_set_option("mloo_batch_draws", 0)


@pytest.mark.parametrize("n,q", ((17, 45), (33, 17), (70, 40), (300, 40)))
def test_a_draw_does_not_depend_on_its_batch_its_neighbours_or_its_place(gpu, batch_option, n, q):
    c = mr.case(n, q)
    full = _call(c, range(17))
    for b in (1, 3):
        batch_option(b)
        assert _same(full, _call(c, range(17))), b
    batch_option(0)
    for d in (0, 5, 16):
        assert _same(full, _call(c, [d]), slice(d, d + 1)), d                                       # alone and among 17
    order = [16] + list(range(1, 16)) + [0]                                                         # first and last swapped
    swapped = _call(c, order)
    assert _same(full, swapped, slice(16, 17), slice(0, 1)) and _same(full, swapped, slice(0, 1), slice(16, 17))
    batch_option(3)
    assert _same(swapped, _call(c, order))
    assert _same(full, _call(c, range(17), W=True, device=0))


# ------------------------------------------------------------------------------------------ bad draws
def test_bad_draws_are_nan_counted_and_alone(gpu):
    n, q = 33, 45
    c = mr.case(n, q)
    good = _call(c, range(17))
    S = c["S"].copy()
    S[2, 7] = np.nan
    S[9, :] = -1e6
    r = bnr_amd.marginal_loglik(c["X"], c["y"], c["tau2"], c["mu"], S, c["W"])                      # status OK: ordinary data
    assert r["n_bad"] == 2
    for k in NAMES:
        assert np.isnan(r[k][..., [2, 9]]).all(), k
    rest = [d for d in range(17) if d not in (2, 9)]
    assert _same(good, r, rest, rest)
    t2 = c["tau2"].copy()
    t2[4] = np.inf
    mu = c["mu"].copy()
    mu[11] = np.nan
    r = bnr_amd.marginal_loglik(c["X"], c["y"], t2, mu, c["S"], c["W"])
    assert r["n_bad"] == 2 and np.isnan(r["loglik"][:, [4, 11]]).all() and np.isnan(r["logml"][[4, 11]]).all()
    rest = [d for d in range(17) if d not in (4, 11)]
    assert _same(good, r, rest, rest)


def test_a_pivot_that_fails_past_the_first_256_columns(gpu):
    """n = 300: column 7 of X touches only the rows from 256 on and has S = -1e6 in draw 2, so columns 0 .. 255 of that draw factor as they do
    without it and the first pivot that is not > 0 lies in a column j >= 256, where every thread is on its second row or idle.  Ordinary data and
    a status, as above."""
    n, q, D, e = 300, 45, 5, 7
    c = mr.case(n, q)
    X = c["X"].copy()
    X[:256, e] = 0.0
    assert X[256, e] ** 2 * 1e6 > 1.0 + (X[256] ** 2 * c["S"][2]).sum()                              # A[256][256] < 0: pivot 256 cannot be > 0
    args = (X, c["y"], c["tau2"][:D], c["mu"][:D])
    good = bnr_amd.marginal_loglik(*args, c["S"][:D], c["W"][:D])
    S = c["S"][:D].copy()
    S[2, e] = -1e6
    r = bnr_amd.marginal_loglik(*args, S, c["W"][:D])
    assert good["n_bad"] == 0 and r["n_bad"] == 1
    for k in NAMES:
        assert np.isnan(r[k][..., 2]).all() and np.all(np.isfinite(good[k])), k
    assert _same(good, r, [0, 1, 3, 4], [0, 1, 3, 4])
    h = api._host_marginal_terms(X[:256], c["y"][:256], c["tau2"][2:3], c["mu"][2:3], S[2:3], c["W"][2:3])
    assert h[4] == 0                                                                                # the leading 256 x 256 block of that draw factors


# ------------------------------------------------------------------------------------------ live chains
TOT = 60


def _fit(n):
    X, y, _ = bnr_amd.make_synthetic(n, 6, 2, seed=7)
    chains = [bnr_amd.Chain(X, y, 2, TOT, 11, 1)]
    chains += [bnr_amd.Chain.like(chains[0], 11, k, TOT) for k in (2, 3)]
    for ch in chains:
        ch.init_prior()
        ch.run(2, TOT, TOT)
    tables = [ch.fetch() for ch in chains]
    yield np.asarray(X, dtype=np.float64), np.asarray(y, dtype=np.float64), chains, tables
    for ch in chains:
        ch.close()


@pytest.fixture(scope="module")
def fit(gpu):
    yield from _fit(20)


@pytest.fixture(scope="module")
def fit300(gpu):
    """the same chains at n = 300: k_mloo_rhs runs two workgroups along the rows and the factor kernel two passes on live draws"""
    yield from _fit(300)


@pytest.mark.parametrize("thin", (1, 3))
@pytest.mark.parametrize("nburn,nsamp", ((5, 40), (8, 41)))
def test_live_chains(fit, nburn, nsamp, thin):
    _live_chains(fit, 20, nburn, nsamp, thin)


@pytest.mark.parametrize("thin", (1, 3))
@pytest.mark.parametrize("nburn,nsamp", ((5, 40), (8, 41)))
def test_live_chains_past_256_rows(fit300, nburn, nsamp, thin):
    _live_chains(fit300, 300, nburn, nsamp, thin)


def _live_chains(fit, n, nburn, nsamp, thin):
    X, y, chains, tables = fit
    nd = -(-nsamp // thin)
    D = 3 * nd
    before = [(ch.iter, ch.counters()) for ch in chains]
    el, kh, lm, ls, ml, ll, nb = _capi.chains_marginal_loo(chains, nburn + 1, nsamp, thin, loglik=True)
    assert nb == 0 and ll.shape == (n, D) and ml.shape == (D,)
    h = api._host_marginal_loglik(tables, X, y, nburn, nsamp, thin)
    t2, mu, S, W = api._host_marginal_draws(tables, nburn, nsamp, thin)
    worst = 0.0
    for d in range(D):
        b = mr.numpy_bounds(X, y, t2[d], mu[d], S[d], W[d])
        ratio = np.abs(ll[:, d] - h[0][:, d]) / b["tol_loglik"]
        assert b["beta_lam"] <= 0.1 and np.all(np.isfinite(ll[:, d])) and np.all(ratio <= 4.0), (d, float(ratio.max()))
        worst = max(worst, float(ratio.max()), abs(ml[d] - h[3][d]) / b["tol_logml"])
    assert worst <= 4.0
    lw, el2, kh2 = _capi.psis_weights_raw(ll)                                                       # the PSIS core, unchanged: bit for bit
    assert np.array_equal(el, el2) and np.array_equal(kh, kh2)
    dev = bnr_amd.marginal_loglik(X, y, t2, mu, S, W)
    assert np.array_equal(dev["loglik"], ll) and np.array_equal(dev["logml"], ml)                   # the chain form = the raw call on the same draws
    rs, vr = dev["resid"], dev["var"]
    for i in range(n):
        a = bsum = 0.0
        for s in range(D):
            w = math.exp(lw[i, s])
            a = a + w * rs[i, s]
            m = y[i] - rs[i, s]
            bsum = bsum + w * (vr[i, s] + m * m)
        mean = y[i] - a
        sd = math.sqrt(bsum - mean * mean)
        assert abs(lm[i] - mean) <= 4 * np.spacing(abs(mean)) and abs(ls[i] - sd) <= 4 * np.spacing(sd), (i, lm[i], mean, ls[i], sd)
    r = api.device_marginal_loo(chains, nburn, nsamp, thin, per_chain=True)
    assert np.array_equal(r["elpd_loo_i"], el) and np.array_equal(r["pareto_k"], kh) and np.array_equal(r["loo_mean"], lm)
    assert r["draws"] == D and r["thin"] == thin and r["n_bad"] == 0 and r["elpd_chain"].shape == (3, n)
    for k, ch in enumerate(chains):
        one = _capi.chains_marginal_loo([ch], nburn + 1, nsamp, thin, loglik=True)
        assert np.array_equal(r["elpd_chain"][k], one[0]) and np.array_equal(r["pareto_k_chain"][k], one[1])
        assert np.array_equal(one[5], ll[:, k * nd:(k + 1) * nd]) and np.array_equal(one[4], ml[k * nd:(k + 1) * nd])
    w = bnr_amd.stacking_weights(r["elpd_chain"].T)["weights"]
    assert w.shape == (3,) and abs(w.sum() - 1) <= 1e-12
    assert [(ch.iter, ch.counters()) for ch in chains] == before                                    # nothing of any chain is written
    for ch, t in zip(chains, tables):
        now = ch.fetch()
        assert all(np.array_equal(now[k], t[k], equal_nan=True) for k in t)


def test_chain_call_refusals_and_view(fit):
    X, y, chains, _tables = fit
    v = chains[0].device_view()
    assert (v.n, v.V, v.R, v.q, v.tot) == (20, 6, 2, 21, TOT) and v.ldx >= v.n_pad >= v.n and v.rowlen >= v.o_S + v.q and v.X and v.trace
    v2 = chains[1].device_view()
    assert v2.X == v.X and v2.y == v.y and v2.trace != v.trace                                      # chains of one fit share the inputs
    for args in ((0, 10, 1), (1, TOT + 1, 1), (TOT, 2, 1)):
        with pytest.raises(bnr_amd.BnrError) as e:
            _capi.chains_marginal_loo(chains, *args)
        assert e.value.code == 1 and "window" in str(e.value)
    with pytest.raises(bnr_amd.BnrError) as e:
        _capi.chains_marginal_loo([chains[0], chains[0]], 1, 10, 1)
    assert "twice" in str(e.value)
    with pytest.raises(ValueError):
        _capi.chains_marginal_loo(chains, 1, 10, 0)


def test_fit_with_the_flag_adds_the_result_and_changes_nothing_else(gpu, tmp_path):
    X, y, _ = bnr_amd.make_synthetic(20, 6, 2, seed=7)
    kw = dict(nburn=30, nsamples=40, num_chains=2, seed=5, x_transform=False, suppress_timer=True, filename=str(tmp_path / "p.log"), loo=True)
    a = bnr_amd.Fit(X, y, 2, **kw)
    b = bnr_amd.Fit(X, y, 2, marginal_loo=True, marginal_loo_draws=15, **kw)
    assert a.marginal_loo is None and set(a.loo) == set(b.loo)
    for k in a.loo:
        assert np.array_equal(a.loo[k], b.loo[k], equal_nan=True), k
    assert all(np.array_equal(a.state[k], b.state[k], equal_nan=True) for k in a.state)
    m = bnr_amd.MarginalLOO(b)
    assert m["thin"] == 3 and m["draws"] == 14 and m["n_bad"] == 0 and m["loo_mean"].shape == (20,) and np.isfinite(m["elpd_loo"])
    h = api._host_marginal_loo([b.state], np.asarray(X, dtype=np.float64), y, b.burn_in, b.sampled, 3)
    assert abs(m["elpd_loo"] - h["elpd_loo"]) <= 1e-8 * abs(h["elpd_loo"]) and np.allclose(m["loo_mean"], h["loo_mean"], rtol=1e-9, atol=1e-12)
    p = bnr_amd.Fit(X, y, 2, marginal_loo=True, marginal_loo_draws=15, pool_chains=True, **kw)
    assert p.marginal_loo["draws"] == 28 and p.stat_chains == 2
