"""GPU tests of the marginal libraries (libbnr_mloo.so, libbnr_medge.so, libbnr_mpred.so, libbnr_mcov.so) bit for bit on draws whose every
intermediate is a float64 (tests/mexact_ref.py; DESIGN.md section 8, "Exact references of the marginal kernels"), through the public calls only.
Where the reference's report says that a sum is exact in any order the device's value has to be that float64, whatever the order of its tiles, of
its K loop and inside an MFMA: resid and var are one correctly rounded division of exact operands, v of an edge, var of a new row and an entry of
`within` are exact.  The means (m of an edge, mean of a new row) are sums over g_i = fl(resid_i fl(tau2 / var_i)), which is rounded: they are
restated in numpy in the device's order (i ascending, one accumulator) from the resid and var just proven, and compared bit for bit as well.

Choices the issue leaves open, and why:
  - loglik: the loglik half of test_marginal_loo_gpu._formula_checks, restated here (its logml half holds for a diagonal A only).
  - logml: against -(n / 2) log(2 pi tau2) - ln 2 sum k_j - ||z||^2 / (2 tau2) in mpmath; the allowance is (n + 8) u times the sum of the absolute
    terms plus pred_ref.LIBM_ULPS u |log| for each of the n + 1 logarithms the device takes.
  - vobs is not an output of the raw prediction call (it returns mean and var); var + tau2 is one addition of the var checked here.
  - the covariance cases mix the first 8 draws of n = 17 as 2 chains of 4 under the weights (1/4, 3/4), and the first 4 of n = 33 as one chain;
    n = 265 and n = 521 have one draw, one chain of it, at 129 columns.

The shapes are mexact_ref.SHAPES.  n = 257 reaches the factor kernel's second 256-column pass with a single column, whose k loops run zero times;
n = 265 gives that pass nine columns, a full unrolled chunk of eight non-zero terms, slots behind the select that hold entries of L, and the
Cholesky's second row of a thread a non-zero update; n = 521 does the same for the third pass and the third row, with the second pass full
(tests/test_marginal_exact_host.py asserts each of these from the integers of the reference, and that the mutants of those loops change a bit
compared here).
"""
import mpmath as mp
import numpy as np
import pytest

import bnr_amd
import mexact_ref as mx
from bnr_amd import _capi, api
from pred_ref import LIBM_ULPS

pytestmark = pytest.mark.gpu
EPS = 2.0 ** -52
U = 2.0 ** -53
SHAPES = tuple(mx.SHAPES)
COV_MIX = {17: (2, 4, (0.25, 0.75)), 33: (1, 4, (1.0,)), 265: (1, 1, (1.0,)), 521: (1, 1, (1.0,))}


def _phi(c, D=None):
    D = c["D"] if D is None else D
    return c["tau2"][:D], c["mu"][:D], c["S"][:D], c["W"][:D]


def _gi(n, d):
    """g_i = fl(resid_i fl(tau2 / var_i)) of draw d, as the projection kernels stage it, from the exact resid and var"""
    ex = mx.draw(n, d)
    return ex["resid"] * (ex["tau2"] / ex["var"])


def _dot_rows(rows, gi):
    """sum_i rows[i] gi[i], i ascending, one accumulator per column from 0.0"""
    acc = np.zeros(rows.shape[1])
    for i in range(rows.shape[0]):
        acc = acc + rows[i] * gi[i]
    return acc


# ------------------------------------------------------------------------------------------ marginal_loglik
def _check_loglik(r, n, draws):
    assert r["n_bad"] == 0
    for j, d in enumerate(draws):
        ex = mx.draw(n, d)
        assert ex["mloo_ok"].all()
        assert np.array_equal(r["resid"][:, j], ex["resid"]), (n, d, "resid", np.flatnonzero(r["resid"][:, j] != ex["resid"])[:8])
        assert np.array_equal(r["var"][:, j], ex["var"]), (n, d, "var", np.flatnonzero(r["var"][:, j] != ex["var"])[:8])
        rs, vr = r["resid"][:, j], r["var"][:, j]
        half = rs * rs / vr / 2
        allow = 16 * EPS * (np.abs(np.log(2 * np.pi * vr) / 2) + half + 1)
        want = -0.5 * (np.log(2 * np.pi) + np.log(vr)) - half
        assert np.all(np.abs(r["loglik"][:, j] - want) <= allow), (n, d, "loglik")
        with mp.workdps(50):
            t2 = mp.mpf(ex["tau2"])
            terms = [mp.mpf(n) / 2 * mp.log(2 * mp.pi * t2), mp.log(2) * int(ex["k"].sum()),
                     mp.mpf(int((ex["zi"] * ex["zi"]).sum())) / mp.mpf(2) ** (2 * ex["E"] + 4) / (2 * t2)]
            want_ml = -terms[0] - terms[1] - terms[2]
            allow_ml = (n + 8) * U * float(sum(abs(t) for t in terms)) + LIBM_ULPS * U * float(mp.log(2) * int(ex["k"].sum())
                                                                                            + abs(mp.mpf(n) / 2 * mp.log(t2)))
            err = abs(float(mp.mpf(float(r["logml"][j])) - want_ml))
        assert err <= allow_ml, (n, d, "logml", err, allow_ml)


@pytest.mark.parametrize("n", SHAPES)
def test_loglik_terms_bit_for_bit(gpu, n):
    c = mx.inputs(n)
    r = bnr_amd.marginal_loglik(c["X"], c["y"], *_phi(c))
    _check_loglik(r, n, range(c["D"]))


# ------------------------------------------------------------------------------------------ marginal_gamma
def _check_gamma(m, v, n, draws, cols=None):
    """m, v: D x (the columns cols of X, None: all)"""
    c = mx.inputs(n)
    idx = mx.edges_checked(n)
    pos = np.arange(c["q"]) if cols is None else np.asarray(cols)
    for j, d in enumerate(draws):
        ed = mx.edges(n, d)
        exact = dict(zip(idx.tolist(), zip(ed["v"].tolist(), ed["ok"].tolist())))
        want = np.array([exact[e][0] if e in exact and exact[e][1] else np.nan for e in pos.tolist()])
        chk = ~np.isnan(want)
        assert np.array_equal(v[j][chk], want[chk]), (n, d, "v", pos[chk][np.flatnonzero(v[j][chk] != want[chk])[:8]])
        p = _dot_rows(c["X"][:, pos], _gi(n, d))
        wm = c["W"][d][pos] + c["S"][d][pos] * p
        assert np.array_equal(m[j], wm), (n, d, "m", pos[np.flatnonzero(m[j] != wm)[:8]])
    return int(chk.sum())


@pytest.mark.parametrize("n", SHAPES)
def test_edge_terms_bit_for_bit(gpu, n):
    c = mx.inputs(n)
    r = bnr_amd.marginal_gamma(c["X"], c["y"], *_phi(c))
    assert r["n_bad"] == 0
    checked = _check_gamma(r["m"], r["v"], n, range(c["D"]))
    print("n=%d q=%d: v of %d edges of the last draw exact" % (n, c["q"], checked))
    assert checked >= (2000 if len(mx.edges_checked(n)) < c["q"] else 0.95 * np.count_nonzero(c["S"][c["D"] - 1]))


# ------------------------------------------------------------------------------------------ marginal_predict
@pytest.fixture
def options():
    used = []

    def setopt(lib, name, value):
        used.append((lib, name))
        getattr(_capi, lib + "_set_option")(name, value)
    yield setopt
    for lib, name in used:
        getattr(_capi, lib + "_set_option")(name, 0)


def _check_predict(r, n, draws):
    c = mx.inputs(n)
    assert r["n_bad"] == 0
    for j, d in enumerate(draws):
        pd = mx.predict(n, d)
        ok = pd["ok"]
        assert np.array_equal(r["var"][j][ok], pd["var"][ok]), (n, d, "var", np.flatnonzero(r["var"][j] != pd["var"])[:8])
        want = (c["mu"][d] + pd["a"]) + _dot_rows(pd["C"], _gi(n, d))
        assert np.array_equal(r["mean"][j], want), (n, d, "mean", np.flatnonzero(r["mean"][j] != want)[:8])


@pytest.mark.parametrize("n", SHAPES)
def test_new_row_terms_bit_for_bit(gpu, options, n):
    c = mx.inputs(n)
    for block in (0, 40):
        options("mpred", "mpred_block_rows", block)
        r = bnr_amd.marginal_predict_terms(c["X"], c["y"], c["Xn"], *_phi(c))
        _check_predict(r, n, range(c["D"]))


# ------------------------------------------------------------------------------------------ marginal_gamma_cov
def _cov_cols(n, ncols):
    return tuple(int(v) for v in np.random.default_rng([53, n, ncols]).choice(mx.inputs(n)["q"], size=ncols, replace=False))


def _check_cov(r, n, cols, K, nd, w):
    want, ok = mx.within(n, cols, K, nd, w)
    assert r["n_bad"] == 0 and np.array_equal(r["within"], r["within"].T) and np.array_equal(r["cov"], r["cov"].T)
    assert np.array_equal(r["within"][ok], want[ok]), (n, len(cols), np.argwhere(ok & (r["within"] != want))[:8])
    _check_gamma(r["m"], r["v"], n, range(K * nd), cols)


@pytest.mark.parametrize("n,ncols", [(n, ncols) for n in (17, 33) for ncols in (127, 128, 129)] + [(265, 129), (521, 129)])
def test_within_bit_for_bit(gpu, n, ncols):
    c = mx.inputs(n)
    K, nd, w = COV_MIX[n]
    cols = _cov_cols(n, ncols)
    r = bnr_amd.marginal_gamma_cov(c["X"], c["y"], *_phi(c, K * nd), list(cols), K, list(w))
    _check_cov(r, n, cols, K, nd, w)
    g = bnr_amd.marginal_gamma(c["X"], c["y"], *_phi(c, K * nd))
    assert np.array_equal(r["m"], g["m"][:, list(cols)]) and np.array_equal(r["v"], g["v"][:, list(cols)])    # the two libraries' copies of one kernel


# ------------------------------------------------------------------------------------------ the batch options
@pytest.mark.parametrize("batch", (1, 3))
def test_every_batch_size_gives_the_same_exact_bits(gpu, options, batch):
    n = 17
    c = mx.inputs(n)
    for lib in ("mloo", "medge", "mpred", "mcov"):
        options(lib, lib + "_batch_draws", batch)
    _check_loglik(bnr_amd.marginal_loglik(c["X"], c["y"], *_phi(c)), n, range(c["D"]))
    r = bnr_amd.marginal_gamma(c["X"], c["y"], *_phi(c))
    _check_gamma(r["m"], r["v"], n, range(c["D"]))
    _check_predict(bnr_amd.marginal_predict_terms(c["X"], c["y"], c["Xn"], *_phi(c)), n, range(c["D"]))
    K, nd, w = COV_MIX[n]
    cols = _cov_cols(n, 129)
    _check_cov(bnr_amd.marginal_gamma_cov(c["X"], c["y"], *_phi(c, K * nd), list(cols), K, list(w)), n, cols, K, nd, w)


# ------------------------------------------------------------------------------------------ the chain form past q = 256 and n = 33
def test_chain_form_with_two_workgroups_of_edges(gpu):
    """n = 40, V = 23, R = 2: q = 276 edges, the second workgroup of k_mloo_w and a chain-form n > 33; the chain form equals the raw call on the
    fetched draws bit for bit"""
    tot, nburn, nsamp, thin = 24, 6, 16, 2
    X, y, _ = bnr_amd.make_synthetic(40, 23, 2, seed=7)
    chains = [bnr_amd.Chain(X, y, 2, tot, 11, 1)]
    chains.append(bnr_amd.Chain.like(chains[0], 11, 2, tot))
    try:
        for ch in chains:
            ch.init_prior()
            ch.run(2, tot, tot)
        tables = [ch.fetch() for ch in chains]
        X, y = np.asarray(X, dtype=np.float64), np.asarray(y, dtype=np.float64)
        assert chains[0].device_view().q == 276 and X.shape == (40, 276)
        t2, mu, S, W = api._host_marginal_draws(tables, nburn, nsamp, thin)
        _el, _kh, _lm, _ls, ml, ll, nb = _capi.chains_marginal_loo(chains, nburn + 1, nsamp, thin, loglik=True)
        raw = bnr_amd.marginal_loglik(X, y, t2, mu, S, W)
        assert nb == 0 and raw["n_bad"] == 0 and np.all(np.isfinite(ll))
        assert np.array_equal(raw["loglik"], ll) and np.array_equal(raw["logml"], ml)
        cols = list(range(0, 276, 2)) + [275, 257, 255]
        for cl in (None, cols):
            mean, cov, within, m, v, nb = _capi.chains_marginal_edge_cov(chains, nburn + 1, nsamp, thin, cl, None, True)
            rc = bnr_amd.marginal_gamma_cov(X, y, t2, mu, S, W, cl, 2)
            assert nb == 0 and rc["n_bad"] == 0 and np.all(np.isfinite(cov))
            for k, got in (("mean", mean), ("cov", cov), ("within", within), ("m", m), ("v", v)):
                assert np.array_equal(rc[k], got), (cl is None, k)
    finally:
        for ch in chains:
            ch.close()
