"""CPU tests of the Rao-Blackwellised covariance of the edge coefficients (include/bnr_mcov.h, libbnr_mcov.so): the two statements of the mpmath
reference against each other, the numpy restatements api._host_gamma_cov and api._host_marginal_edge_cov against the reference within the derived
bound (tests/mcov_ref.py) and against api._host_mixture_summary, the conditional covariance against the sampler's own gamma draws on a seeded CPU
fit, what the library exports and which kernels its code object holds, the refusals and the Fit plumbing with the device call stubbed.  No GPU."""
import ctypes as C
import functools
import inspect
import math
import os
import re
import subprocess
import types

import numpy as np
import pytest

import bnr_amd
import code_objects as co
import mcov_ref as cr
import mloo_ref as mr
from bnr_amd import _capi, api
from oracle import bnr_oracle as bo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST_N = (1, 2, 16, 17, 33)
HOST_Q = (1, 3, 15, 45)


def _strip_comments(src):
    return re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", src, flags=re.S))


# ------------------------------------------------------------------------------------------ the reference
@pytest.mark.parametrize("n,q", [(1, 1), (2, 3), (15, 4), (16, 17), (17, 15)])
def test_the_two_statements_of_the_reference_agree(n, q):
    c = mr.case(n, q)
    for d in (0, 1, 2):
        _m, A, _t = cr.a_inverse_cov(c["X"], c["y"], c["tau2"][d], c["mu"][d], c["S"][d], c["W"][d])
        B = cr.precision_cov(c["X"], c["tau2"][d], c["S"][d])
        for a in range(q):
            for b in range(q):
                scale = max(1, abs(B[a][a]), abs(B[b][b]))
                assert abs(A[a][b] - B[a][b]) <= 1e-40 * scale, (a, b, d)


# ------------------------------------------------------------------------------------------ the numpy restatements within the bound
@pytest.mark.parametrize("binary", (False, True))
@pytest.mark.parametrize("q", HOST_Q)
@pytest.mark.parametrize("n", HOST_N)
def test_host_gamma_cov_meets_the_bound(n, q, binary):
    c = mr.case(n, q, binary)
    worst = 0.0
    for d in (0, 1, 2):
        ref = cr.mixture([cr.case_draw(n, q, d, binary)], n, 1, 1)
        assert ref["ec_max"] <= 0.1
        m, Cv = api._host_gamma_cov(c["X"], c["y"], c["tau2"][d], c["mu"][d], c["S"][d], c["W"][d])
        rm, rc = cr.ratio(m, ref["mean"], ref["tol_mean"]), cr.ratio(Cv, ref["cov"], ref["tol_cov"])
        assert np.all(rm <= 2.0) and np.all(rc <= 2.0), (d, float(rm.max()), float(rc.max()))
        assert np.all(ref["between"] == 0.0)
        worst = max(worst, float(rm.max()), float(rc.max()))
    print("n=%d q=%d binary=%d: worst error / bound %.3g" % (n, q, binary, worst))


def _tables(n, V, R, rows=4, seed=0):
    q = V * (V + 1) // 2
    rng = np.random.default_rng([184, n, V, seed])
    X = rng.normal(size=(n, q))
    y = rng.normal(size=n) * 2.0 + 1.0
    t = _capi.new_table(rows, V, R, dead=False)
    t["u"][:] = rng.normal(size=(rows, R, V)) * 0.7
    t["lam"][:, :, 0] = rng.integers(-1, 2, size=(rows, R))
    t["tau2"][:, 0, 0] = rng.exponential(size=rows) + 0.05
    t["mu"][:, 0, 0] = rng.normal(size=rows)
    t["S"][:, :, 0] = rng.exponential(size=(rows, q))
    return X, y, t


@pytest.mark.parametrize("n,q,K,nd", [(2, 3, 1, 1), (16, 15, 1, 3), (17, 15, 2, 3), (33, 45, 2, 2)])
def test_host_mixture_restatement_meets_the_bound(n, q, K, nd):
    c = mr.case(n, q)
    D = K * nd
    ref = cr.case_mixture(n, q, K, nd)
    assert ref["ec_max"] <= 0.1
    mean, cov, within, m, v, nb = api._host_gamma_cov_terms(c["X"], c["y"], c["tau2"][:D], c["mu"][:D], c["S"][:D], c["W"][:D], K)
    got = dict(mean=mean, cov=cov, within=within)
    w = cr.worst(got, ref)
    print("n=%d q=%d K=%d nd=%d: worst error / bound %s" % (n, q, K, nd, w))
    assert nb == 0 and max(w.values()) <= 2.0, w
    rb = cr.ratio(cov - within, ref["between"], ref["tol_between"] + ref["tol_within"] * 0 + 2 * mr.U * (np.abs(cov) + np.abs(within)))
    assert np.all(rb <= 2.0)
    if K == nd == 1:
        assert np.array_equal(cov, within)                                        # between == 0
    # the identities with the edge table's summary
    s = api._host_mixture_summary(m, v, K)
    assert np.array_equal(mean, s["mean"])
    noclamp = np.all(v > 0, axis=0)
    tol = 2.0 * np.diag(ref["tol_within"]) + 8 * mr.U * np.abs(s["var_within"])
    assert noclamp.any() and np.all(np.abs(np.diag(within) - s["var_within"])[noclamp] <= tol[noclamp])
    assert np.array_equal(cov, cov.T) or np.allclose(cov, cov.T, rtol=0, atol=4 * float(np.max(ref["tol_cov"])))


def test_host_restatement_columns_weights_and_bad_draws():
    X, y, t = _tables(6, 3, 2)
    other = {k: a.copy() for k, a in t.items()}
    other["mu"] += 0.5
    full = api._host_marginal_edge_cov([t, other], X, y, 0, 4, 2)
    assert isinstance(full, api.MarginalEdgeCov) and full.chains == 2 and full.draws == 4 and full.thin == 2 and full.n_bad == 0 and full.weights is None
    cols = [4, 0, 4, 2]
    sub = api._host_marginal_edge_cov([t, other], X, y, 0, 4, 2, cols=cols)
    assert np.allclose(sub.cov, full.cov[np.ix_(cols, cols)], rtol=1e-12, atol=1e-15) and np.array_equal(sub.mean, full.mean[cols])
    assert sub.cov[0, 2] == sub.cov[0, 0] and np.array_equal(sub.node1, full.node1[cols])     # a repeated edge is its own diagonal
    for k, tab in enumerate((t, other)):
        w = np.zeros(2)
        w[k] = 1.0
        one = api._host_marginal_edge_cov([t, other], X, y, 0, 4, 2, weights=w)
        own = api._host_marginal_edge_cov([tab], X, y, 0, 4, 2)
        assert np.array_equal(one.cov, own.cov) and np.array_equal(one.within, own.within) and np.array_equal(one.mean, own.mean)
    single = api._host_marginal_edge_cov([t], X, y, 0, 1, 1)
    assert np.array_equal(single.cov, single.within) and np.all(single.between == 0)
    assert np.all(full.rb_share > 0) and np.all(full.rb_share <= 1 + 1e-12)
    con = full.contrast(np.ones(6))
    assert np.allclose(con["sd"], math.sqrt(full.cov.sum())) and len(full.top_pairs(3)) == 3 and np.allclose(np.diag(full.corr), 1.0)
    bad = {k: a.copy() for k, a in t.items()}
    bad["S"][2, 1, 0] = np.nan
    b = api._host_marginal_edge_cov([bad], X, y, 0, 4, 2)
    assert b.n_bad == 1 and np.isnan(b.cov).all() and np.isnan(b.within).all() and np.isnan(b.mean).all()


# ------------------------------------------------------------------------------------------ the seeded CPU fit of the issue
@functools.lru_cache(maxsize=None)
def _fit():
    """n = 60, V = 10, R = 3, 3000 rows, seed 4242 (the fit of tests/test_marginal_edges_host.py): (X, y, table)"""
    X, y, _ = bnr_amd.make_synthetic(60, 10, 3, seed=7)
    o = bo.Oracle(X, y, 3, 3000, 4242, chain=1, pdf_mode=1)
    o.init_prior()
    o.run(2, 3000, 3000)
    return np.asarray(X, dtype=np.float64), np.asarray(y, dtype=np.float64).reshape(-1), o.t


def _w_of(u, lam):
    ek, el = api._edge_nodes_all(u.shape[2])
    w = np.zeros((u.shape[0], ek.size))
    for t in range(u.shape[1]):
        w = w + u[:, t, :][:, el] * lam[:, t][:, None] * u[:, t, :][:, ek]
    return w


def test_the_samplers_own_draws_are_chi_square_under_the_conditional_covariance():
    """gamma[i] is drawn given (tau2[i], u[i], lambda[i - 1], S[i - 1], mu[i - 1]) (update_gamma!): (gamma_i - m_i)^T (D_i^-1 + X^T X) (gamma_i - m_i)
    / tau2_i -- the quadratic form in the PRECISION, which the code under test never forms -- is chi-square with q = 55 degrees of freedom,
    independently per row: its mean over the 1500 rows lies within 6 sqrt(2 q / 1500) of q.  On the same rows the A^-1 form of api._host_gamma_cov
    is the inverse of that precision."""
    X, y, t = _fit()
    i = np.arange(1500, 3000)
    tau2, mu, S, W = t["tau2"][i, 0, 0], t["mu"][i - 1, 0, 0], t["S"][i - 1, :, 0], _w_of(t["u"][i], t["lam"][i - 1, :, 0])
    m, _v, nb = api._host_gamma_terms(X, y, tau2, mu, S, W)
    assert nb == 0
    q = X.shape[1]
    assert q == 55
    XtX = X.T @ X
    d = t["gamma"][i, :, 0] - m
    chi = np.array([d[j] @ ((np.diag(1.0 / S[j]) + XtX) @ d[j]) / tau2[j] for j in range(i.size)])
    print("mean quadratic form %.3f (q = %d) over %d rows" % (float(chi.mean()), q, i.size))
    assert abs(float(chi.mean()) - q) <= 6.0 * math.sqrt(2.0 * q / 1500.0)
    for j in (0, 700, 1499):
        mj, Cj = api._host_gamma_cov(X, y, tau2[j], mu[j], S[j], W[j])
        P = (np.diag(1.0 / S[j]) + XtX) / tau2[j]
        assert np.allclose(Cj @ P, np.eye(q), rtol=0, atol=1e-8) and np.allclose(mj, m[j], rtol=1e-10, atol=1e-12)


# ------------------------------------------------------------------------------------------ the library
def test_mcov_library_exports_exactly_what_its_header_declares():
    hdr = _strip_comments(open(os.path.join(ROOT, "include", "bnr_mcov.h")).read())
    declared = set(re.findall(r"\b(bnr_[a-zA-Z0-9_]+)\s*\(", hdr))
    assert declared == set(_capi.MCOV_EXPORTS) and len(declared) == 4
    assert os.path.exists(bnr_amd.MCOV_LIB), "libbnr_mcov.so has not been built"
    syms = subprocess.run(["nm", "-D", "--defined-only", bnr_amd.MCOV_LIB], check=True, stdout=subprocess.PIPE, text=True).stdout
    defined = {line.split()[-1] for line in syms.splitlines() if line.strip()}
    assert defined == declared, defined ^ declared                               # no kernel handle, host stub or template instance is exported
    L = _capi.mcov_lib()
    assert L.bnr_mcov_abi_version() == int(re.search(r"#define BNR_MCOV_ABI_VERSION (\d+)", hdr).group(1)) == 1
    for name in ("MarginalEdgeCov", "marginal_gamma_cov", "device_marginal_edge_cov", "mcov_lib", "MCOV_LIB"):
        assert hasattr(bnr_amd, name), name
    needed = subprocess.run(["readelf", "-d", bnr_amd.MCOV_LIB], check=True, stdout=subprocess.PIPE, text=True).stdout
    assert "libbnr_hip.so" in needed and "$ORIGIN" in needed and "libbnr_m" not in needed
    mk = open(os.path.join(ROOT, "bayesiannetworkregression.jl_amd", "csrc", "Makefile")).read()
    assert re.search(r"^MCOV_DEPS = .*\$\(MEDGE_DEPS\)", mk, flags=re.M)


def test_mcov_signatures_match_the_header():
    hdr = _strip_comments(open(os.path.join(ROOT, "include", "bnr_mcov.h")).read())
    kinds = {"int32_t": C.c_int32, "int64_t": C.c_int64, "double": C.c_double}
    for name, (res, args) in _capi._MCOV_SIGS.items():
        decl = re.search(r"int\s+%s\s*\(([^)]*)\)" % name, hdr).group(1).strip()
        params = [] if decl == "void" else [p.strip() for p in decl.split(",")]
        assert res is C.c_int and len(params) == len(args), name
        for p, a in zip(params, args):
            if "*" in p:
                want = {"int32_t": (_capi._ip,), "double": (_capi._dp,), "char": (C.c_char_p,), "bnr_chain": (C.POINTER(C.c_void_p),)}
                base = re.sub(r"\bconst\b|\*", " ", p).split()[0]
                assert a in want[base], (name, p)
            else:
                assert a is kinds[p.split()[0]], (name, p)


def test_mcov_code_object_holds_the_included_kernels_and_its_own(tmp_path, monkeypatch):
    if not (co.have_tools() and os.path.exists(bnr_amd.MCOV_LIB)):
        pytest.skip("no ROCm LLVM tools / no built library here")
    monkeypatch.setattr(co, "LIB", bnr_amd.MCOV_LIB)
    cos = co.code_objects(tmp_path)
    assert len(cos) == 1
    own = co.declared_kernels("bnr_mcov_kernels.h")
    assert own == {"k_mcov_proj", "k_mcov_gram", "k_mcov_center", "k_mcov_finish"}
    declared = own | co.declared_kernels("bnr_medge_kernels.h") | co.declared_kernels("bnr_mloo_kernels.h")
    assert len(declared) == 10 and set(cos[0]) == declared, set(cos[0]) ^ declared
    assert not declared & {re.sub(r"<.*", "", k) for k in co.SWEEP | co.ANALYSIS}


# ------------------------------------------------------------------------------------------ refusals
def test_refusals():
    L = _capi.mcov_lib()
    a = np.ones(16)
    p = _capi._ptr(a)
    err = lambda: _capi.lib().bnr_last_error()
    ip = lambda v: np.array(v, dtype=np.int32).ctypes.data_as(_capi._ip)

    def raw(n=2, q=2, K=1, nd=1, X=p, y=p, t2=p, mu=p, S=p, w=None, nc=2, cols=None, mean=p, cov=p):
        return L.bnr_marginal_gamma_cov(0, n, q, K, nd, X, y, t2, mu, S, None, w, nc, cols, mean, cov, None, None, None, None)

    for kw, word in ((dict(X=None), b"NULL"), (dict(S=None), b"NULL"), (dict(mean=None, cov=None), b"mean, cov or within"), (dict(n=0), b"n >= 1"),
                     (dict(q=0), b"n >= 1"), (dict(K=0), b"K >= 1"), (dict(nd=0), b"K >= 1"), (dict(n=2049), b"2048"), (dict(nc=0, cols=ip([0])), b"ncols >= 1"),
                     (dict(nc=1), b"every column"), (dict(nc=3), b"every column"), (dict(nc=2, cols=ip([0, 2])), b"outside 0 .. 1"),
                     (dict(nc=1, cols=ip([-1])), b"outside 0 .. 1"), (dict(K=2, w=_capi._ptr(np.array([0.5, 0.6]))), b"sum to 1"),
                     (dict(K=2, w=_capi._ptr(np.array([1.5, -0.5]))), b">= 0"), (dict(K=2, w=_capi._ptr(np.array([np.nan, 1.0]))), b"finite"),
                     (dict(K=2, w=_capi._ptr(np.zeros(2))), b"> 0"), (dict(K=33, w=_capi._ptr(np.full(33, 1 / 33))), b"32")):
        assert raw(**kw) == _capi.BNR_ERR_BAD_ARG and word in err(), (kw, err())
    h = (C.c_void_p * 1)(None)

    def chain(ch=h, K=1, w=None, first=1, ns=1, thin=1, nc=1, cols=None, mean=p):
        return L.bnr_chains_marginal_edge_cov(ch, K, w, first, ns, thin, nc, cols, mean, None, None, None, None, None)

    assert chain(ch=None) == 1 and chain(K=0) == 1 and chain(mean=None) == 1
    assert chain(thin=0) == 1 and b"thin" in err()
    assert chain() == 1 and b"NULL chain" in err()
    assert chain(K=0, w=_capi._ptr(np.array([2.0]))) == 1 and b"nchains" in err()          # the chain list is checked before the weights
    assert L.bnr_mcov_set_option(b"no_such", 1) == 1 and L.bnr_mcov_set_option(b"mcov_batch_draws", -1) == 1 and L.bnr_mcov_set_option(None, 1) == 1
    for other in (b"mloo_batch_draws", b"medge_batch_draws", b"mpred_batch_draws", b"mcheck_batch_draws", b"mstack_batch_draws"):
        assert L.bnr_mcov_set_option(other, 1) == 1, other                          # (the other libraries' options)
    assert L.bnr_mcov_set_option(b"mcov_batch_draws", 0) == 0
    X, y = np.ones((3, 2)), np.ones(3)
    for args, kw in (((np.ones(3), y, [1.0], [0.0], np.ones((1, 2))), {}), ((X, np.ones(4), [1.0], [0.0], np.ones((1, 2))), {}),
                     ((X, y, [1.0], [0.0], np.ones((1, 3))), {}), ((np.ones((2049, 1)), np.ones(2049), [1.0], [0.0], np.ones((1, 1))), {}),
                     ((X, y, [1.0], [0.0], np.ones((1, 2))), dict(cols=[2])), ((X, y, [1.0], [0.0], np.ones((1, 2))), dict(cols=[])),
                     ((X, y, [1.0], [0.0], np.ones((1, 2))), dict(cols=[0.5])), ((X, y, [1.0], [0.0], np.ones((1, 2))), dict(nchains=2)),
                     ((X, y, [1.0, 1.0], [0.0, 0.0], np.ones((2, 2))), dict(nchains=2, weights=[1.0]))):
        with pytest.raises(ValueError):
            bnr_amd.marginal_gamma_cov(*args, **kw)
    res = api.Results(None, np.zeros(1), np.zeros(1), 0, 1)
    with pytest.raises(ValueError):
        api.MarginalEdgeCov(res)
    with pytest.raises(TypeError):
        api.MarginalEdgeCov(cov=np.zeros((1, 1)))
    assert api._EDGE_COV_FIELDS == ("cols", "node1", "node2", "mean", "cov", "chains", "draws", "weights")
    assert api._MEDGE_COV_FIELDS == ("cols", "node1", "node2", "mean", "cov", "within", "chains", "draws", "thin", "n_bad", "weights")


# ------------------------------------------------------------------------------------------ Fit
def test_fit_plumbing_with_the_device_call_stubbed(monkeypatch):
    y = np.zeros(5)
    assert api._fit_requests(y, 2).marginal_edge_cov is None and api._fit_requests(y, 2, marginal_edge_cov=False).marginal_edge_cov is None
    assert api._fit_requests(y, 2, marginal_edge_cov=True).marginal_edge_cov == (2000, "all")
    draws, cols = api._fit_requests(y, 2, marginal_edge_cov=[4, 0, 4], marginal_edges_draws=7).marginal_edge_cov
    assert draws == 7 and np.array_equal(cols, [4, 0, 4]) and cols.dtype == np.int32
    xin = _capi.XInput(np.zeros((5, 6)), False)                                   # V = 3, q = 6
    draws, cols = api._fit_requests(y, 2, X_new=xin, nsamp=10, x_transform=False, marginal_edge_cov=[(1, 2), (3, 2)]).marginal_edge_cov
    assert np.array_equal(cols, [1, 4])
    for bad in ([], "all", [(0, 1)], [6], [(1, 4)]):
        with pytest.raises(ValueError):
            api._fit_requests(y, 2, X_new=xin, nsamp=10, x_transform=False, marginal_edge_cov=bad)
    for bad in (0, 1.5, -3, True):
        with pytest.raises(ValueError):
            api._fit_requests(y, 2, marginal_edge_cov=True, marginal_edges_draws=bad)
    with pytest.raises(ValueError):
        api._fit_requests(np.zeros(2049), 2, X_new=_capi.XInput(np.zeros((2049, 3))), nsamp=10, x_transform=False, marginal_edge_cov=True)
    for fn in (bnr_amd.Fit, bnr_amd.generate_samples, bnr_amd.generate_samples_dbl, api._fit_requests):
        par = inspect.signature(fn).parameters
        assert par["marginal_edge_cov"].default is False and list(par)[-3:] == ["marginal_edge_cov", "marginal_stack", "marginal_loo_predict"], fn
    names = [f.name for f in api.dataclasses.fields(api.Results)]
    assert names[-3:] == ["marginal_edge_cov", "marginal_stacking", "marginal_loo_predictive"]
    monkeypatch.setattr(api, "_rank_world", lambda: (0, 2))                         # chains spread over two ranks: refused before any sampling
    with pytest.raises(ValueError, match="marginal_edge_cov"):
        api._fit_requests(y, 2, marginal_edge_cov=True)
    with pytest.raises(ValueError, match="marginal_edge_cov"):
        bnr_amd.Fit(np.zeros((5, 3)), y, 2, x_transform=False, marginal_edge_cov=True, filename=None)
    monkeypatch.undo()

    calls = []

    def stub(chains, nburn, nsamp, thin=1, cols=None, weights=None, per_draw=False):
        calls.append((list(chains), nburn, nsamp, thin, cols, weights, per_draw))
        return {"stub": len(calls)}

    monkeypatch.setattr(api, "device_marginal_edge_cov", stub)
    c1, c2 = types.SimpleNamespace(name=1), types.SimpleNamespace(name=2)
    cs = types.SimpleNamespace(chains={1: c1, 2: c2}, ids=[1, 2])
    base = dict(return_state=False)
    new = lambda: api.Results(None, np.zeros(1), np.zeros(1), 30, 45)
    res = api._finish(cs, new(), api._fit_requests(y, 2, marginal_edge_cov=True, marginal_edges_draws=20, **base), 1)
    assert res.marginal_edge_cov == {"stub": 1} and calls[-1] == ([c1], 30, 45, 3, None, None, False)          # thin = ceil(45 / 20)
    res = api._finish(cs, new(), api._fit_requests(y, 2, marginal_edge_cov=[2, 1], pool_chains=True, **base), 1)
    assert res.marginal_edge_cov == {"stub": 2} and calls[-1][:4] == ([c1, c2], 30, 45, 1) and np.array_equal(calls[-1][4], [2, 1])
    assert api.MarginalEdgeCov(res) is res.marginal_edge_cov
    other = {f.name: getattr(res, f.name) for f in api.dataclasses.fields(res) if f.name != "marginal_edge_cov"}
    plain = api._finish(cs, new(), api._fit_requests(y, 2, pool_chains=True, **base), 1)
    assert len(calls) == 2 and plain.marginal_edge_cov is None
    assert {k: v for k, v in other.items() if k not in ("rhatxi", "rhatgamma")} == {
        f.name: getattr(plain, f.name) for f in api.dataclasses.fields(plain) if f.name not in ("marginal_edge_cov", "rhatxi", "rhatgamma")}


def test_accessor_falls_back_to_the_state_table():
    X, y, t = _tables(6, 2, 2)
    res = api.Results(t, np.zeros(1), np.zeros(1), 1, 3)
    got = api.MarginalEdgeCov(res, X, y, x_transform=False)
    ref = api._host_marginal_edge_cov([t], X, y, 1, 3)
    assert isinstance(got, api.MarginalEdgeCov) and isinstance(got, api.EdgeCov) and got.draws == 3 and got.thin == 1 and got.chains == 1
    assert np.array_equal(got.cov, ref.cov) and np.array_equal(got.within, ref.within) and np.array_equal(got.node1, [1, 1, 2])
    assert np.allclose(got.between, got.cov - got.within) and "MarginalEdgeCov(edges=3" in repr(got)
