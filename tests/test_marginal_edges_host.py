"""CPU tests of the Rao-Blackwellised edge summaries (include/bnr_medge.h, libbnr_medge.so): the two statements of the mpmath reference against
each other, the numpy restatement api._host_marginal_gamma against the reference within the derived bound (tests/medge_ref.py), the formulas
against the sampler's own gamma draws and the law of total expectation on a seeded CPU fit, api._host_mixture_summary, what the library exports
and which kernels its code object holds, the refusals and the Fit plumbing with the device call stubbed.  No GPU."""
import ctypes as C
import functools
import inspect
import math
import os
import re
import subprocess
import types

import mpmath as mp
import numpy as np
import pytest

import bnr_amd
import code_objects as co
import medge_ref as er
import mloo_ref as mr
from bnr_amd import _capi, api
from oracle import bnr_oracle as bo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST_N = (1, 2, 3, 15, 16, 17, 33)
HOST_V = {1: 1, 3: 2, 15: 5, 45: 9}                                      # q = V (V + 1) / 2


def _strip_comments(src):
    return re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", src, flags=re.S))


# ------------------------------------------------------------------------------------------ the reference
@pytest.mark.parametrize("n,q", [(1, 1), (2, 3), (15, 4), (16, 17), (17, 45)])
def test_the_two_statements_of_the_reference_agree(n, q):
    c = mr.case(n, q)
    for d in (0, 1, 2):
        a = er.a_inverse(c["X"], c["y"], c["tau2"][d], c["mu"][d], c["S"][d], c["W"][d])
        bm, bv = er.precision(c["X"], c["y"], c["tau2"][d], c["mu"][d], c["S"][d], c["W"][d])
        for e in range(q):
            assert abs(a["m"][e] - bm[e]) <= 1e-40 * max(1, abs(bm[e])), ("m", e, d)
            assert abs(a["v"][e] - bv[e]) <= 1e-40 * max(1, abs(bv[e])), ("v", e, d)


# ------------------------------------------------------------------------------------------ the numpy restatement within the bound
def _tables(n, V, R, binary):
    """state tables of 3 rows (one per S scale) with random u, lambda in {-1, 0, 1}, tau2, mu, S; X normal or 0/1; y"""
    q = V * (V + 1) // 2
    rng = np.random.default_rng([182, n, V, int(binary)])
    X = (rng.random(size=(n, q)) < 0.4).astype(np.float64) if binary else rng.normal(size=(n, q))
    y = rng.normal(size=n) * 2.0 + 1.0
    t = _capi.new_table(3, V, R, dead=False)
    t["u"][:] = rng.normal(size=(3, R, V)) * 0.7
    t["lam"][:, :, 0] = rng.integers(-1, 2, size=(3, R))
    t["tau2"][:, 0, 0] = rng.exponential(size=3) + 0.05
    t["mu"][:, 0, 0] = rng.normal(size=3)
    t["S"][:, :, 0] = rng.exponential(size=(3, q)) * np.array(mr.S_SCALES)[:, None]
    return X, y, t


@pytest.mark.parametrize("binary", (False, True))
@pytest.mark.parametrize("q", sorted(HOST_V))
@pytest.mark.parametrize("n", HOST_N)
def test_host_restatement_meets_the_bound(n, q, binary):
    V, R = HOST_V[q], 2
    X, y, t = _tables(n, V, R, binary)
    m, v, nb = api._host_marginal_gamma([t], X, y, 0, 3, 1)
    assert nb == 0 and m.shape == v.shape == (3, q)
    t2, mu, S, W = api._host_marginal_draws([t], 0, 3, 1)
    worst = 0.0
    for d in range(3):
        ref = er.reference(X, y, t2[d], mu[d], S[d], W[d])
        assert ref["beta_lam"] <= 0.1
        for name, got in (("m", m), ("v", v)):
            ratio = er.ratio(got[d], ref[name], ref["tol_" + name])
            assert np.all(np.isfinite(got[d])) and np.all(ratio <= 2.0), (name, d, float(ratio.max()))
            worst = max(worst, float(ratio.max()))
        assert np.all(v[d] >= 0)
    print("n=%d q=%d binary=%d: worst error / bound %.3g" % (n, q, binary, worst))


def test_host_restatement_bad_draws_and_chain_order():
    X, y, t = _tables(5, 2, 2, False)
    other = {k: v.copy() for k, v in t.items()}
    other["mu"] += 0.5
    m, v, nb = api._host_marginal_gamma([t, other], X, y, 0, 3, 2)                # rows 0, 2 of each
    assert m.shape == (4, 3) and nb == 0
    for j, (tab, row) in enumerate(((t, 0), (t, 2), (other, 0), (other, 2))):
        one = {k: a[row:row + 1] for k, a in tab.items()}
        a = api._host_marginal_gamma([one], X, y, 0, 1, 1)
        assert np.array_equal(a[0][0], m[j]) and np.array_equal(a[1][0], v[j])
    bad = {k: a.copy() for k, a in t.items()}
    bad["S"][2, 1, 0] = np.nan
    bm, bv, bnb = api._host_marginal_gamma([bad, other], X, y, 0, 3, 2)
    assert bnb == 1 and np.isnan(bm[1]).all() and np.isnan(bv[1]).all() and np.array_equal(bm[[0, 2, 3]], m[[0, 2, 3]])
    s = api._host_mixture_summary(bm, bv, 2)
    assert all(np.isnan(s[k]).all() for k in _capi.MEDGE_SUMMARY_FIELDS)
    neg = {k: a.copy() for k, a in t.items()}
    neg["S"][0, :, 0] = -1e6
    assert api._host_marginal_gamma([neg], X, y, 0, 3, 2)[2] == 1


# ------------------------------------------------------------------------------------------ the seeded CPU fit of the issue
@functools.lru_cache(maxsize=None)
def _fit():
    """n = 60, V = 10, R = 3, 3000 rows, seed 4242 (the fit of tests/test_marginal_loo_host.py): (X, y, table)"""
    X, y, _ = bnr_amd.make_synthetic(60, 10, 3, seed=7)
    o = bo.Oracle(X, y, 3, 3000, 4242, chain=1, pdf_mode=1)
    o.init_prior()
    o.run(2, 3000, 3000)
    return np.asarray(X, dtype=np.float64), np.asarray(y, dtype=np.float64).reshape(-1), o.t


def _w_of(u, lam):
    """W (rows x q) from u (rows, R, V) and lambda (rows, R): W_e = sum_t u[t, l(e)] lambda_t u[t, k(e)], t ascending"""
    ek, el = api._edge_nodes_all(u.shape[2])
    w = np.zeros((u.shape[0], ek.size))
    for t in range(u.shape[1]):
        w = w + u[:, t, :][:, el] * lam[:, t][:, None] * u[:, t, :][:, ek]
    return w


def test_the_samplers_own_draws_are_standard_normal_under_m_and_v():
    """gamma[i] is drawn given (tau2[i], u[i], lambda[i - 1], S[i - 1], mu[i - 1]) (update_gamma!, gibbs.jl:420-436): standardised with the m and v
    of exactly those values, z has E z^2 = 1.  The bound 6 sqrt(2 / 1500) treats the 55 edges of a draw as perfectly correlated."""
    X, y, t = _fit()
    i = np.arange(1500, 3000)
    m, v, nb = api._host_gamma_terms(X, y, t["tau2"][i, 0, 0], t["mu"][i - 1, 0, 0], t["S"][i - 1, :, 0], _w_of(t["u"][i], t["lam"][i - 1, :, 0]))
    assert nb == 0 and np.all(v > 0)
    z = (t["gamma"][i, :, 0] - m) / np.sqrt(v)
    mz2 = float(np.mean(z * z))
    print("mean z^2 = %.4f over %d x %d; smallest 1 - S t met: %.3g" % (mz2, z.shape[0], z.shape[1], float(np.min(v / (t["tau2"][i, 0, 0][:, None] * t["S"][i - 1, :, 0])))))
    assert abs(mz2 - 1.0) <= 6.0 * math.sqrt(2.0 / 1500.0)


def test_total_expectation_on_the_seeded_fit():
    """own-row phi: the Rao-Blackwellised mean of every edge against the mean of its draws, within 6 batch-means standard errors of the difference"""
    X, y, t = _fit()
    m, v, nb = api._host_marginal_gamma([t], X, y, 1500, 1500, 1)
    assert nb == 0
    g = t["gamma"][1500:3000, :, 0]
    d = (m - g).reshape(30, 50, -1).mean(axis=1)                                   # 30 batch means of the difference, per edge
    se = d.std(axis=0, ddof=1) / math.sqrt(30.0)
    gap = np.abs(d.mean(axis=0))
    share = v.mean(axis=0) / g.var(axis=0)
    bm = lambda a: a.reshape(30, 50, -1).mean(axis=1).var(axis=0, ddof=1)
    ratio = bm(g) / bm(m)
    s = api._host_mixture_summary(m, v, 1)
    counted = np.minimum((g > 0).mean(axis=0), (g < 0).mean(axis=0))
    print("largest gap %.3g posterior sd; E[v] / Var gamma: %.2f .. %.2f (median %.2f); batch-means variance ratio: median %.2f (%.2f .. %.2f); "
          "edges with a counted sign probability of 0 or 1: %d, their lfsr: %s"
          % (float(np.max(gap / g.std(axis=0))), share.min(), share.max(), np.median(share), np.median(ratio), ratio.min(), ratio.max(),
             int(np.sum(counted == 0)), np.minimum(s["p_pos"], s["p_neg"])[counted == 0]))
    assert np.all(gap <= 6.0 * se), float(np.max(gap / se))
    assert np.all(np.minimum(s["p_pos"], s["p_neg"]) > 0)                            # the mixture gives every edge a finite tail


# ------------------------------------------------------------------------------------------ the mixture summary on the host
def _mix(nd, K, q, seed=0):
    rng = np.random.default_rng([183, nd, K, q, seed])
    return rng.normal(size=(K * nd, q)) * 2.0 + rng.normal(size=q), rng.exponential(size=(K * nd, q)) + 0.01


def test_host_mixture_summary_weights():
    m, v = _mix(70, 3, 4)
    a = api._host_mixture_summary(m, v, 3)
    b = api._host_mixture_summary(m, v, 3, weights=np.full(3, 1.0 / 3.0))
    for k in _capi.MEDGE_SUMMARY_FIELDS:
        assert np.array_equal(a[k], b[k]), k
    for k in range(3):
        w = np.zeros(3)
        w[k] = 1.0
        one = api._host_mixture_summary(m, v, 3, weights=w)
        own = api._host_mixture_summary(m[k * 70:(k + 1) * 70], v[k * 70:(k + 1) * 70], 1)
        for f in ("mean", "sd", "var_within", "p_pos", "p_neg"):
            assert np.array_equal(one[f], own[f]), (k, f)
        # (the bracket of the pooled call covers every chain, the chain's own only its draws: the quantiles agree to the bisection widths)
        c = api._loo_bracket_c(0.025, 0.975)
        width = float(np.max(m + c * np.sqrt(v)) - np.min(m - c * np.sqrt(v)))
        assert np.all(np.abs(one["lower"] - own["lower"]) <= 2 * width * 2.0 ** -40) and np.all(np.abs(one["upper"] - own["upper"]) <= 2 * width * 2.0 ** -40)
    # the order of the sums: by definition, in Python floats
    nd = 70
    for e in range(2):
        lanes = [0.0] * 64
        for j in range(nd):
            lanes[j % 64] = lanes[j % 64] + float(m[j, e])
        off = 32
        while off:
            for l in range(off):
                lanes[l] = lanes[l] + lanes[l + off]
            off //= 2
        assert api._host_mixture_summary(m[:nd], v[:nd], 1)["mean"][e] == (lanes[0] / nd) * 1.0


def test_host_mixture_summary_point_masses_and_single_normal():
    m = np.array([[-1.0], [2.0], [3.0], [0.0]])
    s = api._host_mixture_summary(m, np.zeros((4, 1)), 1, p_lo=0.3, p_hi=0.7)
    assert s["mean"][0] == 1.0 and s["var_within"][0] == 0.0 and s["p_pos"][0] == 0.5 and s["p_neg"][0] == 0.25
    assert s["sd"][0] == math.sqrt(14.0 / 4.0 - 1.0)
    assert abs(s["lower"][0] - 0.0) <= 4.0 * 2.0 ** -40 and abs(s["upper"][0] - 2.0) <= 4.0 * 2.0 ** -40      # F jumps 0.25 -> 0.5 at 0 and 0.5 -> 0.75 at 2
    same = api._host_mixture_summary(np.full((5, 1), 7.0), np.zeros((5, 1)), 1)
    assert same["lower"][0] == 7.0 and same["upper"][0] == 7.0 and same["sd"][0] == 0.0
    # all components equal: the quantile of one normal, within the bisection width
    mu, var = 0.75, 2.25
    one = api._host_mixture_summary(np.full((130, 1), mu), np.full((130, 1), var), 2)
    c = api._loo_bracket_c(0.025, 0.975)
    width = 2 * c * 1.5
    for got, p in ((one["lower"][0], 0.025), (one["upper"][0], 0.975)):
        ref = mu + 1.5 * float(mp.sqrt(2) * mp.erfinv(2 * mp.mpf(p) - 1))
        assert abs(got - ref) <= width * 2.0 ** -40 + 1e-13
    assert abs(one["mean"][0] - mu) <= 4 * mr.U and abs(one["var_within"][0] - var) <= 8 * mr.U


def test_host_mixture_summary_sign_probabilities():
    m, v = _mix(65, 2, 5)
    s = api._host_mixture_summary(m, v, 2)
    assert np.all(np.abs(s["p_pos"] + s["p_neg"] - 1.0) <= 8 * mr.EPS)
    tail = api._host_mixture_summary(np.full((3, 1), 30.0), np.ones((3, 1)), 1)
    with mp.workdps(50):
        ref = mp.erfc(mp.mpf(30) / mp.sqrt(2)) / 2
        assert abs(mp.mpf(float(tail["p_neg"][0])) - ref) <= mp.mpf("1e-12") * ref
    assert tail["p_pos"][0] == 1.0
    nan = m.copy()
    nan[7, 2] = np.nan
    sn = api._host_mixture_summary(nan, v, 2)
    for k in _capi.MEDGE_SUMMARY_FIELDS:
        assert np.isnan(sn[k][2]) and np.array_equal(np.delete(sn[k], 2), np.delete(s[k], 2)), k


# ------------------------------------------------------------------------------------------ the library
def test_medge_library_exports_exactly_what_its_header_declares():
    hdr = _strip_comments(open(os.path.join(ROOT, "include", "bnr_medge.h")).read())
    declared = set(re.findall(r"\b(bnr_[a-zA-Z0-9_]+)\s*\(", hdr))
    assert declared == set(_capi.MEDGE_EXPORTS) and len(declared) == 5
    assert os.path.exists(bnr_amd.MEDGE_LIB), "libbnr_medge.so has not been built"
    syms = subprocess.run(["nm", "-D", "--defined-only", bnr_amd.MEDGE_LIB], check=True, stdout=subprocess.PIPE, text=True).stdout
    defined = {line.split()[-1] for line in syms.splitlines() if line.strip()}
    assert defined == declared, defined ^ declared                               # no kernel handle, host stub or template instance is exported
    L = _capi.medge_lib()
    assert L.bnr_medge_abi_version() == int(re.search(r"#define BNR_MEDGE_ABI_VERSION (\d+)", hdr).group(1)) == 1
    for name in ("MarginalEdges", "marginal_gamma", "mixture_summary", "device_marginal_edges", "medge_lib", "MEDGE_LIB"):
        assert hasattr(bnr_amd, name), name
    needed = subprocess.run(["readelf", "-d", bnr_amd.MEDGE_LIB], check=True, stdout=subprocess.PIPE, text=True).stdout
    assert "libbnr_hip.so" in needed and "$ORIGIN" in needed and "libbnr_mloo" not in needed


def test_medge_code_object_holds_the_mloo_kernels_and_its_own(tmp_path, monkeypatch):
    if not (co.have_tools() and os.path.exists(bnr_amd.MEDGE_LIB)):
        pytest.skip("no ROCm LLVM tools / no built library here")
    monkeypatch.setattr(co, "LIB", bnr_amd.MEDGE_LIB)
    cos = co.code_objects(tmp_path)
    assert len(cos) == 1
    own = co.declared_kernels("bnr_medge_kernels.h")
    assert own == {"k_medge_proj", "k_medge_summary"}
    declared = own | co.declared_kernels("bnr_mloo_kernels.h")
    assert len(declared) == 6 and set(cos[0]) == declared, set(cos[0]) ^ declared
    assert not declared & {re.sub(r"<.*", "", k) for k in co.SWEEP | co.ANALYSIS}


# ------------------------------------------------------------------------------------------ refusals
def test_refusals():
    L = _capi.medge_lib()
    a = np.ones(8)
    p = _capi._ptr(a)
    err = lambda: _capi.lib().bnr_last_error()

    def raw(n=2, q=2, D=1, X=p, y=p, t2=p, mu=p, S=p, m=p, v=None):
        return L.bnr_marginal_gamma(0, n, q, D, X, y, t2, mu, S, None, m, v, None)

    for kw, word in ((dict(X=None), b"NULL"), (dict(S=None), b"NULL"), (dict(m=None), b"m or v"), (dict(n=0), b"n >= 1"), (dict(q=0), b"n >= 1"),
                     (dict(D=0), b"n >= 1"), (dict(n=2049), b"2048")):
        assert raw(**kw) == _capi.BNR_ERR_BAD_ARG and word in err(), kw

    def mix(q=1, K=2, nd=2, m=p, v=p, w=None, p_lo=0.025, p_hi=0.975, mean=p, lower=None, upper=None):
        return L.bnr_mixture_summary(0, q, K, nd, m, v, w, p_lo, p_hi, mean, None, None, None, None, lower, upper)

    for kw, word in ((dict(m=None), b"NULL"), (dict(q=0), b"q >= 1"), (dict(K=0), b"q >= 1"), (dict(nd=0), b"q >= 1"), (dict(mean=None), b"at least one"),
                     (dict(lower=p), b"together"), (dict(lower=p, upper=p, p_lo=0.0), b"p_lo"), (dict(lower=p, upper=p, p_lo=0.6, p_hi=0.5), b"p_lo"),
                     (dict(lower=p, upper=p, p_hi=1.0), b"p_lo"), (dict(w=_capi._ptr(np.array([0.5, 0.6]))), b"sum to 1"),
                     (dict(w=_capi._ptr(np.array([1.5, -0.5]))), b">= 0"), (dict(w=_capi._ptr(np.array([np.nan, 1.0]))), b"finite"),
                     (dict(K=33, nd=1, w=p), b"32")):
        assert mix(**kw) == _capi.BNR_ERR_BAD_ARG and word in err(), kw
    h = (C.c_void_p * 1)(None)

    def chain(ch=h, K=1, w=None, first=1, ns=1, thin=1, mean=p):
        return L.bnr_chains_marginal_edges(ch, K, w, first, ns, thin, 0.025, 0.975, mean, None, None, None, None, None, None, None, None, None)

    assert chain(ch=None) == 1 and chain(K=0) == 1
    assert chain(thin=0) == 1 and b"thin" in err()
    assert chain() == 1 and b"NULL chain" in err()
    assert L.bnr_medge_set_option(b"no_such", 1) == 1 and L.bnr_medge_set_option(b"medge_batch_draws", -1) == 1 and L.bnr_medge_set_option(None, 1) == 1
    assert L.bnr_medge_set_option(b"mloo_batch_draws", 1) == 1                    # (the other library's option)
    assert L.bnr_medge_set_option(b"medge_batch_draws", 0) == 0
    X, y = np.ones((3, 2)), np.ones(3)
    for args in ((np.ones(3), y, [1.0], [0.0], np.ones((1, 2))), (X, np.ones(4), [1.0], [0.0], np.ones((1, 2))), (X, y, [1.0], [0.0, 1.0], np.ones((1, 2))),
                 (X, y, [1.0], [0.0], np.ones((1, 3))), (np.ones((2049, 1)), np.ones(2049), [1.0], [0.0], np.ones((1, 1)))):
        with pytest.raises(ValueError):
            bnr_amd.marginal_gamma(*args)
    with pytest.raises(ValueError):
        bnr_amd.marginal_gamma(X, y, [1.0], [0.0], np.ones((1, 2)), W=np.ones((2, 2)))
    for args, kw in (((np.ones((4, 2)), np.ones((4, 3))), {}), ((np.ones((5, 2)), np.ones((5, 2))), dict(nchains=2)), ((np.ones(4), np.ones(4)), {}),
                     ((np.ones((4, 2)), np.ones((4, 2))), dict(nchains=2, weights=[1.0])), ((np.ones((4, 2)), np.ones((4, 2))), dict(interval=100))):
        with pytest.raises(ValueError):
            bnr_amd.mixture_summary(*args, **kw)
    with pytest.raises(ValueError):
        _capi.mixture_summary_raw(np.ones((4, 2)), np.ones((4, 2)), fields=("lower",))
    res = api.Results(None, np.zeros(1), np.zeros(1), 0, 1)
    with pytest.raises(ValueError):
        api.MarginalEdges(res)
    with pytest.raises(TypeError):
        api.MarginalEdges(estimate=np.zeros(1))


# ------------------------------------------------------------------------------------------ Fit
def test_fit_plumbing_with_the_device_call_stubbed(monkeypatch):
    y = np.zeros(5)
    assert api._fit_requests(y, 2).marginal_edges is None
    assert api._fit_requests(y, 2, marginal_edges=True).marginal_edges == (2000, 95)
    assert api._fit_requests(y, 2, marginal_edges=True, marginal_edges_draws=7, predict_interval=90).marginal_edges == (7, 90)
    for bad in (0, 1.5, -3, True):
        with pytest.raises(ValueError):
            api._fit_requests(y, 2, marginal_edges=True, marginal_edges_draws=bad)
    with pytest.raises(ValueError):
        api._fit_requests(y, 2, marginal_edges=True, predict_interval=100)
    with pytest.raises(ValueError):
        api._fit_requests(np.zeros(2049), 2, X_new=_capi.XInput(np.zeros((2049, 3))), nsamp=10, x_transform=False, marginal_edges=True)
    for fn in (bnr_amd.Fit, bnr_amd.generate_samples, bnr_amd.generate_samples_dbl):
        par = inspect.signature(fn).parameters
        assert par["marginal_edges"].default is False and par["marginal_edges_draws"].default == 2000, fn
    monkeypatch.setattr(api, "_rank_world", lambda: (0, 2))                         # chains spread over two ranks: refused before any sampling
    with pytest.raises(ValueError, match="marginal_edges"):
        api._fit_requests(y, 2, marginal_edges=True)
    with pytest.raises(ValueError, match="marginal_edges"):
        bnr_amd.Fit(np.zeros((5, 3)), y, 2, x_transform=False, marginal_edges=True, filename=None)
    monkeypatch.undo()

    calls = []

    def stub(chains, nburn, nsamp, thin=1, weights=None, interval=95, per_draw=False):
        calls.append((list(chains), nburn, nsamp, thin, weights, interval, per_draw))
        return {"stub": len(calls)}

    monkeypatch.setattr(api, "device_marginal_edges", stub)
    stack = types.SimpleNamespace(weights=np.array([0.25, 0.75]), summary=None, prediction=None, edge_cov=None, marginal_edges=None)
    monkeypatch.setattr(api, "device_stack_chains", lambda chains, nb, ns, r_eff: stack)
    c1, c2 = types.SimpleNamespace(name=1), types.SimpleNamespace(name=2)
    cs = types.SimpleNamespace(chains={1: c1, 2: c2}, ids=[1, 2])
    base = dict(return_state=False)
    res = api._finish(cs, api.Results(None, np.zeros(1), np.zeros(1), 30, 45), api._fit_requests(y, 2, marginal_edges=True, marginal_edges_draws=20, **base), 1)
    assert res.marginal_edges == {"stub": 1} and calls[-1] == ([c1], 30, 45, 3, None, 95, False) and res.stat_chains == 1 and res.stacking is None
    res = api._finish(cs, api.Results(None, np.zeros(1), np.zeros(1), 30, 45),
                      api._fit_requests(y, 2, marginal_edges=True, pool_chains=True, predict_interval=90, **base), 1)
    assert res.marginal_edges == {"stub": 2} and calls[-1] == ([c1, c2], 30, 45, 1, None, 90, False) and res.stat_chains == 2
    assert api.MarginalEdges(res) is res.marginal_edges
    res = api._finish(cs, api.Results(None, np.zeros(1), np.zeros(1), 30, 45), api._fit_requests(y, 2, marginal_edges=True, stack_chains=True, **base), 1)
    assert len(calls) == 4 and calls[-2][0] == [c1, c2] and calls[-2][4] is stack.weights and calls[-1][0] == [c1] and calls[-1][4] is None
    assert res.stacking.marginal_edges == {"stub": 3} and res.marginal_edges == {"stub": 4}
    plain = api._finish(cs, api.Results(None, np.zeros(1), np.zeros(1), 30, 45), api._fit_requests(y, 2, **base), 1)
    assert len(calls) == 4 and plain.marginal_edges is None and plain.stat_chains is None
    assert plain == api.Results(None, plain.rhatxi, plain.rhatgamma, 30, 45)          # without the flag: what it was, field for field


def test_marginal_edges_accessor_falls_back_to_the_state_table():
    X, y, t = _tables(6, 2, 2, False)
    res = api.Results(t, np.zeros(1), np.zeros(1), 1, 2)
    got = api.MarginalEdges(res, X, y, x_transform=False)
    m, v, nb = api._host_marginal_gamma([t], X, y, 1, 2, 1)
    s = api._host_mixture_summary(m, v, 1)
    assert isinstance(got, api.MarginalEdges) and got.draws == 2 and got.thin == 1 and got.n_bad == 0 and got.chains == 1 and got.weights is None
    assert np.array_equal(got.estimate, s["mean"]) and np.array_equal(got.lower_bound, s["lower"]) and np.array_equal(got.upper_bound, s["upper"])
    assert np.array_equal(got.node1, [1, 1, 2]) and np.array_equal(got.node2, [1, 2, 2])
    assert np.array_equal(got.lfsr, np.minimum(s["p_pos"], s["p_neg"])) and np.allclose(got.rb_share, s["var_within"] / s["sd"] ** 2, rtol=1e-15)
    assert np.all(got.rb_share > 0) and np.all(got.rb_share <= 1 + 1e-12) and got.m is None and "MarginalEdges(edges=3" in repr(got)
