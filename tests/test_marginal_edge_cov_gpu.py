"""GPU tests of the Rao-Blackwellised covariance of the edge coefficients (include/bnr_mcov.h, libbnr_mcov.so; kernels in csrc/bnr_mcov_kernels.h):
the raw call against the mpmath reference within the derived bound (tests/mcov_ref.py) at the edges of the 16-row MFMA tile, of the 32-row padding, of
the 16-column padding of the panel and of the 128-column Gram tile; against the numpy restatement beyond; cases whose answer is exact; large
neighbouring entries of L behind the triangle's mask; the independence of an entry's bits from the batch, the other columns, the place of a column,
the other chains and the call; bad draws; live chains through the chain form and Fit; and all seven libraries in one process.

Choices the issue leaves open, and why:
  - the long mixtures at q = 5 use n = 17 (a padded row tile) and repeat mloo_ref's pool of 17 draws (mcov_ref.long_case).
  - the Gram kernel uses one tile width, 128: the column counts 127, 128, 129 are the first columns of the (17, 130) case, two draws; the 16-column
    padding of the panel is met by q = 1, 3, 16, 17, 33, 45.
  - the X = I case uses S_e = 2^k - 1 with EVEN k (as the edge table's test does): every entry of L, T' and the products is then a float64.
"""
import dataclasses
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

import bnr_amd
import mcov_ref as cr
import medge_ref as er
import mloo_ref as mr
from bnr_amd import _capi, api

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = ("mean", "cov", "within", "m", "v")
TOT = 60


def _call(c, draws, K=1, cols=None, weights=None, W=True):
    d = list(draws)
    return bnr_amd.marginal_gamma_cov(c["X"], c["y"], c["tau2"][d], c["mu"][d], c["S"][d], c["W"][d] if W else None, cols, K, weights)


def _same(a, b, keys=OUT):
    return all(np.array_equal(a[k], b[k], equal_nan=True) for k in keys)


def _gate(r, ref, what):
    w = cr.worst(r, ref)
    print("%s: error / bound %s, beta lam %.2e" % (what, {k: "%.3g" % v for k, v in w.items()}, ref["ec_max"]))
    assert ref["ec_max"] <= 0.1
    assert r["n_bad"] == 0 and max(w.values()) <= 2.0, (what, w)
    assert np.array_equal(r["cov"], r["cov"].T) and np.array_equal(r["within"], r["within"].T)
    return max(w.values())


# ------------------------------------------------------------------------------------------ against the mpmath reference
@pytest.mark.parametrize("q", (1, 3, 16, 17, 33, 45))
@pytest.mark.parametrize("n", (1, 2, 15, 16, 17, 31, 32, 33))
def test_raw_call_meets_the_bound_of_the_reference(gpu, n, q):
    c = mr.case(n, q)
    for K, nd in ((1, 1), (1, 2), (2, 3)):
        r = _call(c, range(K * nd), K)
        _gate(r, cr.case_mixture(n, q, K, nd), "n=%d q=%d K=%d nd=%d" % (n, q, K, nd))
        if K == nd == 1:
            assert np.array_equal(r["cov"], r["within"])                           # one draw: its conditional covariance


@pytest.mark.parametrize("K,nd", ((1, 65), (3, 22), (2, 129)))
def test_long_mixtures(gpu, K, nd):
    c, _idx = cr.long_case(17, 5, K * nd)
    r = bnr_amd.marginal_gamma_cov(c["X"], c["y"], c["tau2"], c["mu"], c["S"], c["W"], None, K)
    _gate(r, cr.long_mixture(17, 5, K, nd), "long K=%d nd=%d" % (K, nd))


@pytest.mark.parametrize("ncols", (127, 128, 129))
def test_column_counts_around_the_gram_tile(gpu, ncols):
    c = mr.case(17, 130)
    r = _call(c, range(2), 1, cols=list(range(ncols)))
    _gate(r, cr.case_mixture(17, 130, 1, 2, False, tuple(range(ncols))), "ncols=%d" % ncols)


def test_raw_call_meets_the_bound_on_a_binary_matrix(gpu):
    for n, q in ((17, 45), (33, 31)):
        r = _call(mr.case(n, q, True), range(6), 2)
        _gate(r, cr.case_mixture(n, q, 2, 3, True), "binary n=%d q=%d" % (n, q))


@pytest.mark.parametrize("n", (17, 33))
def test_large_entries_of_l_behind_the_mask(gpu, n):
    """every S at scale 1e3: the slots M[r][i], i > r, hold entries of L of size ~ 1e2, a thousand times those of L^-1 -- a missing mask cannot stay
    within the bound; n = 17 and 33 also leave rows n .. np - 1 of the draw's matrix unwritten"""
    q = 45
    c = mr.case(n, q)
    S = np.abs(c["S"][:3]) / np.array(mr.S_SCALES)[:, None] * 1e3
    r = bnr_amd.marginal_gamma_cov(c["X"], c["y"], c["tau2"][:3], c["mu"][:3], S, c["W"][:3])
    draws = []
    for d in range(3):
        m, C, t = cr.a_inverse_cov(c["X"], c["y"], c["tau2"][d], c["mu"][d], S[d], c["W"][d])
        ref = er.reference(c["X"], c["y"], c["tau2"][d], c["mu"][d], S[d], c["W"][d])
        draws.append(dict(m=m, C=C, t=t, tau2=float(c["tau2"][d]), S=S[d], tol_m=ref["tol_m"], ec=ref["beta_lam"]))
    _gate(r, cr.mixture(draws, n, 1, 3), "mask n=%d" % n)


# ------------------------------------------------------------------------------------------ against the numpy restatement
# (258, 300, 513: the M that k_mcov_proj reads comes out of the second and third 256-column pass of k_mloo_factor; 258 is the first n at which a
# later pass has a column behind its first, 300 fills full unrolled chunks of the second pass, 513 opens the third -- tests/test_marginal_loo_gpu.py)
@pytest.mark.parametrize("n,q", [(n, q) for q in (64, 300) for n in (64, 65, 129, 257)] + [(258, 64), (300, 64), (513, 64)])
def test_raw_call_against_the_restatement(gpu, n, q):
    c = mr.case(n, q)
    r = _call(c, range(3))
    h = api._host_gamma_cov_terms(c["X"], c["y"], c["tau2"][:3], c["mu"][:3], c["S"][:3], c["W"][:3], 1)
    b = cr.mixture([cr.numpy_draw(c["X"], c["y"], c["tau2"][d], c["mu"][d], c["S"][d], c["W"][d]) for d in range(3)], n, 1, 3)
    assert r["n_bad"] == 0 and h[5] == 0 and b["ec_max"] <= 0.1
    worst = 0.0
    for k, hv in (("mean", h[0]), ("cov", h[1]), ("within", h[2])):
        ratio = cr.ratio(r[k], hv, b["tol_" + k])
        assert np.all(ratio <= 4.0), (k, float(ratio.max()))                        # each within its own gate of 2
        worst = max(worst, float(ratio.max()))
    print("n=%d q=%d: worst difference / bound %.3g" % (n, q, worst))


# ------------------------------------------------------------------------------------------ exact cases
@pytest.mark.parametrize("n,q", ((1, 1), (17, 5), (33, 45), (65, 130)))
def test_exact_cases(gpu, n, q):
    c = mr.case(n, q)
    K, nd = 2, 3
    D = K * nd
    y, t2, mu, S, W = c["y"], c["tau2"][:D], c["mu"][:D], c["S"][:D], c["W"][:D]
    r = _call(c, range(D), K)
    g = bnr_amd.marginal_gamma(c["X"], y, t2, mu, S, W)
    assert np.array_equal(r["m"], g["m"]) and np.array_equal(r["v"], g["v"])        # m and v: bnr_marginal_gamma's
    assert np.array_equal(r["mean"], bnr_amd.mixture_summary(g["m"], g["v"], K)["mean"])
    assert np.array_equal(r["cov"], r["cov"].T) and np.array_equal(r["within"], r["within"].T)
    cols = [q - 1, 0, q // 2]
    rc = _call(c, range(D), K, cols=cols)
    assert np.array_equal(rc["m"], g["m"][:, cols]) and np.array_equal(rc["v"], g["v"][:, cols])
    dg = api._medge_stat(t2[:, None] * S, K, np.full(K, 0.5))
    r0 = bnr_amd.marginal_gamma_cov(np.zeros((n, q)), y, t2, mu, S, W, None, K)     # X = 0: the diagonal's chain sums, off-diagonals +0
    assert np.array_equal(r0["within"], np.diag(dg)) and not np.signbit(r0["within"]).any() and np.array_equal(r0["m"], W)
    rs = bnr_amd.marginal_gamma_cov(c["X"], y, t2, mu, np.zeros((D, q)), W, None, K)  # S = 0
    assert np.array_equal(rs["within"], np.zeros((q, q))) and np.array_equal(rs["m"], W)
    rng = np.random.default_rng([8, n])                                             # X = I_n, S_e = 2^k - 1 with even k, tau2 a power of 4
    Di = 8                                                                           # 2 chains of 4 draws: the divisions by nd are exact as well
    k = 2 * rng.integers(0, 6, size=(Di, n))
    tq = np.array([1.0, 4.0, 0.25])[rng.integers(0, 3, size=Di)]
    ri = bnr_amd.marginal_gamma_cov(np.eye(n), y, tq, c["mu"][:Di], 2.0 ** k - 1.0, None, None, 2)
    exact = ((tq[:, None] * (2.0 ** k - 1.0)) * 2.0 ** -k).sum(axis=0) / Di         # (dyadic: every product and sum is exact)
    assert ri["n_bad"] == 0 and np.array_equal(ri["within"], np.diag(exact))


# ------------------------------------------------------------------------------------------ independence
@pytest.fixture
def batch_option():
    yield lambda v: _capi.mcov_set_option("mcov_batch_draws", v)
    _capi.mcov_set_option("mcov_batch_draws", 0)


@pytest.mark.parametrize("n,q", ((17, 45), (33, 17), (40, 300)))
def test_an_entry_does_not_depend_on_batch_columns_place_chains_or_call(gpu, batch_option, n, q):
    c = mr.case(n, q)
    K, nd = 3, 5
    full = _call(c, range(15), K)
    for b in (1, 3, 0):
        batch_option(b)
        assert _same(full, _call(c, range(15), K)), b
    assert _same(full, _call(c, range(15), K))                                      # two calls in a row
    rng = np.random.default_rng([9, n, q])
    cols = rng.choice(q, size=min(q, 7), replace=False)
    ix = np.ix_(cols, cols)
    sub = _call(c, range(15), K, cols=cols)                                         # a subset: the same entries of the all-column call
    assert np.array_equal(sub["cov"], full["cov"][ix]) and np.array_equal(sub["within"], full["within"][ix]) and np.array_equal(sub["mean"], full["mean"][cols])
    perm = rng.permutation(q)                                                        # a permutation of all columns
    pr = _call(c, range(15), K, cols=perm)
    assert np.array_equal(pr["cov"], full["cov"][np.ix_(perm, perm)]) and np.array_equal(pr["within"], full["within"][np.ix_(perm, perm)])
    rep = np.array([cols[0], cols[-1], cols[0]])                                     # a repeated column
    rr = _call(c, range(15), K, cols=rep)
    assert np.array_equal(rr["cov"], full["cov"][np.ix_(rep, rep)]) and np.array_equal(rr["within"], full["within"][np.ix_(rep, rep)])
    for k in range(K):                                                               # w = e_k against the one-chain call
        w = np.zeros(K)
        w[k] = 1.0
        one = _call(c, range(k * nd, (k + 1) * nd), 1)
        pick = _call(c, range(15), K, weights=w)
        assert _same(one, pick, ("mean", "cov", "within")), k
    other = _call(c, list(range(5, 10)) + list(range(12, 17)) + list(range(0, 5)), K, weights=[0.0, 0.0, 1.0])   # chain 0 placed last among other chains
    assert _same(other, _call(c, range(5), 1), ("mean", "cov", "within"))


# ------------------------------------------------------------------------------------------ bad draws
def test_bad_draws_make_every_output_nan(gpu):
    n, q = 33, 45
    c = mr.case(n, q)
    S = c["S"][:6].copy()
    S[2, 7] = np.nan
    r = bnr_amd.marginal_gamma_cov(c["X"], c["y"], c["tau2"][:6], c["mu"][:6], S, c["W"][:6], None, 2)   # status OK: ordinary data
    assert r["n_bad"] == 1 and all(np.isnan(r[k]).all() for k in ("mean", "cov", "within")) and np.isnan(r["m"][2]).all() and np.isnan(r["v"][2]).all()
    good = _call(c, range(6), 2)
    rest = [0, 1, 3, 4, 5]
    assert np.array_equal(r["m"][rest], good["m"][rest]) and np.array_equal(r["v"][rest], good["v"][rest])
    without = _call(c, [0, 1, 3, 4], 2)
    assert without["n_bad"] == 0 and all(np.isfinite(without[k]).all() for k in OUT)
    S[2, :] = -1e6                                                                   # a pivot that is not > 0
    assert bnr_amd.marginal_gamma_cov(c["X"], c["y"], c["tau2"][:6], c["mu"][:6], S, c["W"][:6], [3, 1], 2)["n_bad"] == 1


# ------------------------------------------------------------------------------------------ live chains
def _fit(n, K):
    X, y, _ = bnr_amd.make_synthetic(n, 6, 2, seed=7)
    chains = [bnr_amd.Chain(X, y, 2, TOT, 11, 1)]
    chains += [bnr_amd.Chain.like(chains[0], 11, k, TOT) for k in range(2, K + 1)]
    for ch in chains:
        ch.init_prior()
        ch.run(2, TOT, TOT)
    return np.asarray(X, dtype=np.float64), np.asarray(y, dtype=np.float64), chains, [ch.fetch() for ch in chains]


@pytest.fixture(scope="module", params=((17, 2), (33, 3)))
def fit(gpu, request):
    X, y, chains, tables = _fit(*request.param)
    yield X, y, chains, tables
    for ch in chains:
        ch.close()


@pytest.mark.parametrize("thin", (1, 3))
def test_live_chains(fit, thin):
    X, y, chains, tables = fit
    K, n, q, nburn, nsamp = len(chains), X.shape[0], 21, 8, 41
    nd = -(-nsamp // thin)
    before = [(ch.iter, ch.counters()) for ch in chains]
    cols = [20, 3, 7, 3]
    t2, mu, S, W = api._host_marginal_draws(tables, nburn, nsamp, thin)
    raws = {}
    for cl in (None, cols):
        mean, cov, within, m, v, nb = _capi.chains_marginal_edge_cov(chains, nburn + 1, nsamp, thin, cl, None, True)
        raws[cl is None] = raw = bnr_amd.marginal_gamma_cov(X, y, t2, mu, S, W, cl, K)
        assert nb == 0 and _same(raw, dict(mean=mean, cov=cov, within=within, m=m, v=v))   # the chain form = the raw call on the same draws
    rec = api.device_marginal_edge_cov(chains, nburn, nsamp, thin)
    assert rec.cov.shape == (q, q) and np.array_equal(rec.cov, raws[True]["cov"]) and np.array_equal(raws[False]["cov"], rec.cov[np.ix_(cols, cols)])
    h = api._host_marginal_edge_cov(tables, X, y, nburn, nsamp, thin)
    b = cr.mixture([cr.numpy_draw(X, y, t2[d], mu[d], S[d], W[d]) for d in range(K * nd)], n, K, nd)
    assert b["ec_max"] <= 0.1
    for k in ("mean", "cov", "within"):
        assert np.all(cr.ratio(getattr(rec, k), getattr(h, k), b["tol_" + k]) <= 4.0), k
    assert rec.chains == K and rec.draws == K * nd and rec.thin == thin and rec.n_bad == 0 and np.array_equal(rec.cov, rec.cov.T)
    assert np.all(np.diag(rec.cov) > 0) and np.all((rec.rb_share > 0) & (rec.rb_share <= 1)) and np.allclose(rec.between, rec.cov - rec.within)
    me = api.device_marginal_edges(chains, nburn, nsamp, thin)
    assert np.array_equal(rec.mean, me.estimate) and np.allclose(rec.sd, me.sd, rtol=1e-9) and np.allclose(np.diag(rec.within), me.var_within, rtol=1e-9, atol=1e-15)
    w = np.zeros(K)
    w[K - 1] = 1.0
    one = api.device_marginal_edge_cov(chains[K - 1:], nburn, nsamp, thin)
    pick = api.device_marginal_edge_cov(chains, nburn, nsamp, thin, weights=w)
    assert np.array_equal(one.cov, pick.cov) and np.array_equal(one.within, pick.within) and np.array_equal(one.mean, pick.mean)
    assert [(ch.iter, ch.counters()) for ch in chains] == before                    # nothing of any chain is written
    for ch, t in zip(chains, tables):
        now = ch.fetch()
        assert all(np.array_equal(now[k], t[k], equal_nan=True) for k in t)


def test_chain_call_refusals(fit):
    _X, _y, chains, _tables = fit
    K = len(chains)
    for args in ((0, 10, 1), (1, TOT + 1, 1), (TOT, 2, 1)):
        with pytest.raises(bnr_amd.BnrError) as e:
            _capi.chains_marginal_edge_cov(chains, *args)
        assert e.value.code == 1 and "window" in str(e.value)
    with pytest.raises(bnr_amd.BnrError) as e:
        _capi.chains_marginal_edge_cov([chains[0], chains[0]], 1, 10, 1)
    assert "twice" in str(e.value)
    with pytest.raises(bnr_amd.BnrError) as e:
        _capi.chains_marginal_edge_cov(chains, 1, 10, 1, weights=[0.75] * K)
    assert "sum to 1" in str(e.value)
    L = _capi.mcov_lib()
    arr = (bnr_amd._capi.C.c_void_p * K)(*[ch.h for ch in chains])
    out = np.empty(21 * 21)
    bad = np.array([21], dtype=np.int32)
    assert L.bnr_chains_marginal_edge_cov(arr, K, None, 1, 10, 1, 20, None, _capi._ptr(out), None, None, None, None, None) == 1
    assert b"every column" in _capi.lib().bnr_last_error()
    assert L.bnr_chains_marginal_edge_cov(arr, K, None, 1, 10, 1, 1, bad.ctypes.data_as(_capi._ip), _capi._ptr(out), None, None, None, None, None) == 1
    assert b"outside 0 .. 20" in _capi.lib().bnr_last_error()
    with pytest.raises(ValueError):
        _capi.chains_marginal_edge_cov(chains, 1, 10, 0)


def _digest(rec):
    h = hashlib.sha256()
    for k in ("mean", "cov", "within"):
        h.update(np.ascontiguousarray(getattr(rec, k)).tobytes())
    return h.hexdigest()


_CHILD = """
import sys
sys.path[:0] = [%r, %r]
import hashlib
import numpy as np
import bnr_amd
from bnr_amd import _capi, api
X, y, _ = bnr_amd.make_synthetic(17, 6, 2, seed=7)
ch = bnr_amd.Chain(X, y, 2, 60, 11, 1)
ch.init_prior()
ch.run(2, 60, 60)
if %d:
    api.device_marginal_edges([ch], 5, 40, 3)
rec = api.device_marginal_edge_cov([ch], 5, 40, 3)
h = hashlib.sha256()
for k in ("mean", "cov", "within"):
    h.update(np.ascontiguousarray(getattr(rec, k)).tobytes())
print("DIGEST", h.hexdigest(), int(_capi._medge is not None))
ch.close()
"""


def test_all_seven_libraries_in_one_process(gpu):
    X, y, chains, _tables = _fit(17, 2)
    ed = lambda me: tuple(np.ascontiguousarray(getattr(me, k)).tobytes() for k in ("estimate", "sd", "lower_bound", "upper_bound", "p_pos", "p_neg", "var_within"))
    a = ed(api.device_marginal_edges(chains, 5, 40, 3))
    api.device_marginal_loo(chains, 5, 40, 3)
    api.device_marginal_loo_predict(chains, 5, 40, 3)
    api.device_marginal_stack(chains, 5, 40, 3)
    api.device_marginal_predict(chains, 5, 40, X[:3], None, 3)
    rec = api.device_marginal_edge_cov(chains[:1], 5, 40, 3)
    assert all(x is not None for x in (_capi._lib, _capi._mloo, _capi._medge, _capi._mpred, _capi._mcheck, _capi._mstack, _capi._mcov))
    assert ed(api.device_marginal_edges(chains, 5, 40, 3)) == a                     # the marginal edges before and after: identical bits
    digests = []
    for with_medge in (0, 1):                                                       # a fresh process each: with and without libbnr_medge.so loaded first
        r = subprocess.run([sys.executable, "-c", _CHILD % (ROOT, os.path.join(ROOT, "tests"), with_medge)], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                           text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        line = [l for l in r.stdout.splitlines() if l.startswith("DIGEST")][0].split()
        assert int(line[2]) == with_medge
        digests.append(line[1])
    assert digests[0] == digests[1] == _digest(rec)
    for ch in chains:
        ch.close()


def test_fit_with_the_flag_adds_the_result_and_changes_nothing_else(gpu, tmp_path):
    X, y, _ = bnr_amd.make_synthetic(20, 6, 2, seed=7)
    kw = dict(nburn=30, nsamples=40, num_chains=2, seed=5, x_transform=False, suppress_timer=True, filename=str(tmp_path / "p.log"), loo=True,
              summary_interval=95, marginal_edges=True, marginal_edges_draws=15)
    a = bnr_amd.Fit(X, y, 2, **kw)
    b = bnr_amd.Fit(X, y, 2, marginal_edge_cov=[(1, 2), (2, 3)], **kw)
    assert a.marginal_edge_cov is None
    for f in dataclasses.fields(a):
        if f.name in ("marginal_edge_cov", "state", "loo", "summary_device", "marginal_edges"):
            continue
        assert np.array_equal(getattr(a, f.name), getattr(b, f.name)), f.name
    for f in ("loo", "summary_device"):
        assert set(getattr(a, f)) == set(getattr(b, f)) and all(np.array_equal(getattr(a, f)[k], getattr(b, f)[k], equal_nan=True) for k in getattr(a, f)), f
    assert all(np.array_equal(a.state[k], b.state[k], equal_nan=True) for k in a.state)
    assert np.array_equal(a.marginal_edges.estimate, b.marginal_edges.estimate) and np.array_equal(a.marginal_edges.sd, b.marginal_edges.sd)
    rec = bnr_amd.MarginalEdgeCov(b)
    assert rec is b.marginal_edge_cov and rec.thin == 3 and rec.draws == 14 and rec.chains == 1 and rec.n_bad == 0 and rec.cov.shape == (2, 2)
    assert np.array_equal(rec.cols, [1, 7]) and np.array_equal(rec.node1, [1, 2]) and np.array_equal(rec.node2, [2, 3])
    assert np.array_equal(rec.mean, b.marginal_edges.estimate[[1, 7]])
    h = api._host_marginal_edge_cov([b.state], np.asarray(X, dtype=np.float64), y, b.burn_in, b.sampled, 3, cols=[1, 7])
    assert np.allclose(rec.cov, h.cov, rtol=1e-9, atol=1e-14) and np.allclose(rec.within, h.within, rtol=1e-9, atol=1e-14)
    con = rec.contrast([1.0, -1.0])
    assert np.isfinite(con["sd"]).all() and con["sd"][0] > 0
