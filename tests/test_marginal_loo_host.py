"""CPU tests of marginal PSIS-LOO (include/bnr_mloo.h, libbnr_mloo.so): the two statements of the mpmath reference against each other, the numpy
restatement api._host_marginal_loglik against the reference within the derived bound (tests/mloo_ref.py), the k-hat fact that motivates the
feature on a seeded CPU fit, what the two libraries export and which kernels the new code object holds, the refusals, the thin arithmetic and
the Fit plumbing with the device call stubbed.  No GPU."""
import ctypes as C
import inspect
import os
import re
import subprocess
import types

import numpy as np
import pytest

import bnr_amd
import code_objects as co
import mloo_ref as mr
from bnr_amd import _capi, api
from oracle import bnr_oracle as bo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST_N = (1, 2, 3, 15, 16, 17, 33)
HOST_V = {1: 1, 3: 2, 15: 5, 45: 9}                                      # q = V (V + 1) / 2


def _strip_comments(src):
    return re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", src, flags=re.S))


# ------------------------------------------------------------------------------------------ the reference
@pytest.mark.parametrize("n,q", [(1, 1), (2, 3), (3, 15), (15, 4), (16, 17), (17, 45)])
def test_the_two_statements_of_the_reference_agree(n, q):
    c = mr.case(n, q)
    for d in (0, 1, 2):
        a = mr.brute(c["X"], c["y"], c["tau2"][d], c["mu"][d], c["S"][d], c["W"][d])
        b = mr.identity(c["X"], c["y"], c["tau2"][d], c["mu"][d], c["S"][d], c["W"][d])
        for x, name in zip(a, ("resid", "var", "loglik")):
            for i in range(n):
                assert abs(x[i] - b[name][i]) <= 1e-40 * max(1, abs(b[name][i])), (name, i, d)
    # logml against the chain rule: log p(y) = sum_i log p(y_i | y_1 .. y_i-1), by the same brute-force conditioning on growing prefixes
    import mpmath as mp
    with mp.workdps(mr.DPS):
        tot = mp.mpf(0)
        for m in range(1, n + 1):
            tot += mr.brute(c["X"][:m], c["y"][:m], c["tau2"][0], c["mu"][0], c["S"][0], c["W"][0])[2][m - 1]
        ref = mr.identity(c["X"], c["y"], c["tau2"][0], c["mu"][0], c["S"][0], c["W"][0])["logml"]
        assert abs(tot - ref) <= 1e-40 * max(1, abs(ref))


# ------------------------------------------------------------------------------------------ the numpy restatement within the bound
def _tables(n, V, R, binary):
    """state tables of 3 rows (one per S scale) with random u, lambda in {-1, 0, 1}, tau2, mu, S; X normal or 0/1; y"""
    q = V * (V + 1) // 2
    rng = np.random.default_rng([181, n, V, int(binary)])
    X = (rng.random(size=(n, q)) < 0.4).astype(np.float64) if binary else rng.normal(size=(n, q))
    y = rng.normal(size=n) * 2.0 + 1.0
    t = _capi.new_table(3, V, R, dead=False)
    t["u"][:] = rng.normal(size=(3, R, V)) * 0.7
    t["lam"][:, :, 0] = rng.integers(-1, 2, size=(3, R))
    t["tau2"][:, 0, 0] = rng.exponential(size=3) + 0.05
    t["mu"][:, 0, 0] = rng.normal(size=3)
    t["S"][:, :, 0] = rng.exponential(size=(3, q)) * np.array(mr.S_SCALES)[:, None]
    return X, y, t


def _w_by_definition(t, row):
    """W_e = sum_t u[t, l(e)] lambda_t u[t, k(e)], t ascending from 0.0, in Python floats: edges in the column-wise lower-triangle order"""
    R, V = t["u"].shape[1:]
    out = []
    for k in range(V):
        for l in range(k, V):
            s = 0.0
            for r in range(R):
                s += float(t["u"][row, r, l]) * float(t["lam"][row, r, 0]) * float(t["u"][row, r, k])
            out.append(s)
    return np.array(out)


@pytest.mark.parametrize("binary", (False, True))
@pytest.mark.parametrize("q", sorted(HOST_V))
@pytest.mark.parametrize("n", HOST_N)
def test_host_restatement_meets_the_bound(n, q, binary):
    V, R = HOST_V[q], 2
    X, y, t = _tables(n, V, R, binary)
    ll, rs, vr, ml, nb = api._host_marginal_loglik([t], X, y, 0, 3, 1)
    assert nb == 0 and ll.shape == rs.shape == vr.shape == (n, 3) and ml.shape == (3,)
    t2, mu, S, W = api._host_marginal_draws([t], 0, 3, 1)
    worst = 0.0
    for d in range(3):
        assert np.array_equal(W[d], _w_by_definition(t, d)) and np.array_equal(S[d], t["S"][d, :, 0])
        ref = mr.reference(X, y, t2[d], mu[d], S[d], W[d])
        assert ref["beta_lam"] <= 0.1
        for name, got in (("loglik", ll), ("resid", rs), ("var", vr)):
            ratio = np.abs(got[:, d] - ref[name]) / ref["tol_" + name]
            assert np.all(np.isfinite(got[:, d])) and np.all(ratio <= 2.0), (name, d, float(ratio.max()))
            worst = max(worst, float(ratio.max()))
        ratio = abs(ml[d] - ref["logml"]) / ref["tol_logml"]
        assert np.isfinite(ml[d]) and ratio <= 2.0, ("logml", d, ratio)
        worst = max(worst, ratio)
    print("n=%d q=%d binary=%d: worst error / bound %.3g" % (n, q, binary, worst))


def test_host_restatement_rows_thin_and_chain_order():
    """rows nburn + 1 + j thin of every table, chain k's draws first in order k; a bad draw is NaN and counted, the others unchanged"""
    X, y, t = _tables(5, 2, 2, False)
    big = _capi.new_table(9, 2, 2, dead=False)
    for k in ("u", "lam", "tau2", "mu", "S"):
        big[k][:] = np.concatenate([t[k]] * 3, axis=0)
        big[k][1::2] *= 1.25 if k in ("tau2", "S") else 1.0
    other = {k: v.copy() for k, v in big.items()}
    other["mu"] += 0.5
    ll, rs, vr, ml, nb = api._host_marginal_loglik([big, other], X, y, 2, 6, 3)        # 0-based rows 2, 5 of each
    assert ll.shape == (5, 4) and nb == 0
    for j, (tab, row) in enumerate(((big, 2), (big, 5), (other, 2), (other, 5))):
        one = {k: v[row:row + 1] for k, v in tab.items()}
        a = api._host_marginal_loglik([one], X, y, 0, 1, 1)
        assert np.array_equal(a[0][:, 0], ll[:, j]) and np.array_equal(a[3][0], ml[j])
    assert api._host_marginal_loglik([big], X, y, 2, 7, 3)[0].shape == (5, 3)          # ceil(7 / 3) rows
    bad = {k: v.copy() for k, v in big.items()}
    bad["S"][5, 1, 0] = np.nan
    b = api._host_marginal_loglik([bad, other], X, y, 2, 6, 3)
    assert b[4] == 1 and np.isnan(b[0][:, 1]).all() and np.isnan(b[3][1]) and np.array_equal(b[0][:, [0, 2, 3]], ll[:, [0, 2, 3]])
    neg = {k: v.copy() for k, v in big.items()}
    neg["S"][2, :, 0] = -1e6
    assert api._host_marginal_loglik([neg], X, y, 2, 6, 3)[4] == 1


# ------------------------------------------------------------------------------------------ the k-hat fact
def test_marginal_ratios_have_far_fewer_high_k_rows_than_conditional_ones():
    """the seeded CPU fit of the issue: n = 60, V = 10, R = 3, rows 1500 .. 2999 (0-based) of 3000; PSIS through api._psis_host"""
    X, y, _ = bnr_amd.make_synthetic(60, 10, 3, seed=7)
    o = bo.Oracle(X, y, 3, 3000, 4242, chain=1, pdf_mode=1)
    o.init_prior()
    o.run(2, 3000, 3000)
    X = np.asarray(X, dtype=np.float64)
    cond = api._loo_from_pointwise(*api._psis_host(api._host_loglik(o.t, X, y, 1500, 1500)), 1500)
    ll, _rs, _vr, _ml, nb = api._host_marginal_loglik([o.t], X, y, 1500, 1500, 1)
    assert nb == 0
    marg = api._loo_from_pointwise(*api._psis_host(ll), 1500)
    print("conditional: n_high_k %d median k %.2f max k %.2f elpd %.1f; marginal: n_high_k %d median k %.2f max k %.2f elpd %.1f"
          % (cond["n_high_k"], np.median(cond["pareto_k"]), cond["pareto_k"].max(), cond["elpd_loo"],
             marg["n_high_k"], np.median(marg["pareto_k"]), marg["pareto_k"].max(), marg["elpd_loo"]))
    assert cond["n_high_k"] == 42 and marg["n_high_k"] == 1
    assert marg["n_high_k"] <= cond["n_high_k"] / 2


# ------------------------------------------------------------------------------------------ the libraries
def test_mloo_library_exports_exactly_what_its_header_declares():
    hdr = _strip_comments(open(os.path.join(ROOT, "include", "bnr_mloo.h")).read())
    declared = set(re.findall(r"\b(bnr_[a-zA-Z0-9_]+)\s*\(", hdr))
    assert declared == set(_capi.MLOO_EXPORTS) and len(declared) == 4
    assert os.path.exists(bnr_amd.MLOO_LIB), "libbnr_mloo.so has not been built"
    syms = subprocess.run(["nm", "-D", "--defined-only", bnr_amd.MLOO_LIB], check=True, stdout=subprocess.PIPE, text=True).stdout
    exported = {line.split()[-1] for line in syms.splitlines() if re.search(r"\s[TW]\s+bnr_", line)}
    assert exported == declared, exported ^ declared
    L = _capi.mloo_lib()
    assert L.bnr_mloo_abi_version() == int(re.search(r"#define BNR_MLOO_ABI_VERSION (\d+)", hdr).group(1)) == 1
    assert int(re.search(r"#define BNR_MLOO_MAX_N (\d+)", hdr).group(1)) == _capi.MLOO_MAX_N == api.MLOO_MAX_N == 2048
    for name in ("MarginalLOO", "marginal_loglik", "device_marginal_loo"):
        assert hasattr(bnr_amd, name), name
    needed = subprocess.run(["readelf", "-d", bnr_amd.MLOO_LIB], check=True, stdout=subprocess.PIPE, text=True).stdout
    assert "libbnr_hip.so" in needed and "$ORIGIN" in needed                      # linked against the library beside it


def test_mloo_code_object_holds_exactly_the_kernels_of_its_header(tmp_path, monkeypatch):
    if not (co.have_tools() and os.path.exists(bnr_amd.MLOO_LIB)):
        pytest.skip("no ROCm LLVM tools / no built library here")
    monkeypatch.setattr(co, "LIB", bnr_amd.MLOO_LIB)
    cos = co.code_objects(tmp_path)
    assert len(cos) == 1
    declared = co.declared_kernels("bnr_mloo_kernels.h")
    assert declared == {"k_mloo_w", "k_mloo_rhs", "k_mloo_gram", "k_mloo_factor"}
    assert set(cos[0]) == declared, set(cos[0]) ^ declared
    assert not declared & {re.sub(r"<.*", "", k) for k in co.SWEEP | co.ANALYSIS}


def test_hip_library_exports_the_chain_view():
    hdr = open(os.path.join(ROOT, "include", "bnr_hip.h")).read()
    L = _capi.lib()
    assert int(re.search(r"#define BNR_ABI_VERSION (\d+)", hdr).group(1)) == L.bnr_abi_version() >= 18
    for name in ("bnr_chain_device_view", "bnr_set_last_error"):
        assert name in _capi.EXPORTS and getattr(L, name) is not None and re.search(r"\b%s\(" % name, hdr), name
    fields = re.search(r"typedef struct bnr_chain_view \{(.*?)\} bnr_chain_view;", hdr, flags=re.S).group(1)
    names = [v.strip().lstrip("*") for decl in _strip_comments(fields).split(";") if decl.strip()
             for v in decl.replace("const", "").replace("int32_t", "").replace("double", "").split(",")]
    assert names == [f[0] for f in _capi.ChainView._fields_], names              # the ctypes mirror, field for field
    assert L.bnr_chain_device_view(None, None) == 1 and b"NULL" in L.bnr_last_error()
    assert L.bnr_set_last_error(1, b"from beside") == 1 and L.bnr_last_error() == b"from beside"


# ------------------------------------------------------------------------------------------ refusals and arithmetic
def test_refusals():
    L = _capi.mloo_lib()
    a = np.ones(8)
    p = _capi._ptr(a)

    def raw(n=2, q=2, D=1, X=p, y=p, t2=p, mu=p, S=p, ll=p, rs=None, vr=None):
        return L.bnr_marginal_loglik(0, n, q, D, X, y, t2, mu, S, None, ll, rs, vr, None, None)

    for kw, word in ((dict(X=None), b"NULL"), (dict(S=None), b"NULL"), (dict(ll=None), b"loglik, resid or var"), (dict(n=0), b"n >= 1"),
                     (dict(q=0), b"n >= 1"), (dict(D=0), b"n >= 1"), (dict(n=2049), b"2048")):
        assert raw(**kw) == _capi.BNR_ERR_BAD_ARG and word in _capi.lib().bnr_last_error(), kw
    h = (C.c_void_p * 1)(None)
    assert L.bnr_chains_marginal_loo(None, 1, 1, 1, 1, None, p, p, None, None, None, None, None) == 1
    assert L.bnr_chains_marginal_loo(h, 0, 1, 1, 1, None, p, p, None, None, None, None, None) == 1
    assert L.bnr_chains_marginal_loo(h, 1, 1, 1, 0, None, p, p, None, None, None, None, None) == 1 and b"thin" in _capi.lib().bnr_last_error()
    assert L.bnr_chains_marginal_loo(h, 1, 1, 1, 1, None, p, p, None, None, None, None, None) == 1 and b"NULL chain" in _capi.lib().bnr_last_error()
    assert L.bnr_mloo_set_option(b"no_such", 1) == 1 and L.bnr_mloo_set_option(b"mloo_batch_draws", -1) == 1 and L.bnr_mloo_set_option(None, 1) == 1
    assert L.bnr_mloo_set_option(b"mloo_batch_draws", 0) == 0
    X, y = np.ones((3, 2)), np.ones(3)
    for args in ((np.ones(3), y, [1.0], [0.0], np.ones((1, 2))), (X, np.ones(4), [1.0], [0.0], np.ones((1, 2))), (X, y, [1.0], [0.0, 1.0], np.ones((1, 2))),
                 (X, y, [1.0], [0.0], np.ones((1, 3))), (np.ones((2049, 1)), np.ones(2049), [1.0], [0.0], np.ones((1, 1)))):
        with pytest.raises(ValueError):
            bnr_amd.marginal_loglik(*args)
    with pytest.raises(ValueError):
        bnr_amd.marginal_loglik(X, y, [1.0], [0.0], np.ones((1, 2)), W=np.ones((2, 2)))
    with pytest.raises(ValueError):
        _capi.marginal_loglik_raw(X, y, [1.0], [0.0], np.ones((1, 2)), fields=("logml",))
    res = api.Results(None, np.zeros(1), np.zeros(1), 0, 1)
    with pytest.raises(ValueError):
        api.MarginalLOO(res)


def test_thin_arithmetic():
    assert _capi.mloo_thin_draws(40, 1) == (1, 40) and _capi.mloo_thin_draws(41, 3) == (3, 14) and _capi.mloo_thin_draws(40, 3) == (3, 14)
    assert _capi.mloo_thin_draws(3, 7) == (7, 1)
    for bad in ((40, 0), (0, 1), (40, -2)):
        with pytest.raises(ValueError):
            _capi.mloo_thin_draws(*bad)
    assert api._marginal_loo_thin(20000, 2000) == 10 and api._marginal_loo_thin(20001, 2000) == 11 and api._marginal_loo_thin(100, 2000) == 1
    assert api._marginal_loo_thin(7, 7) == 1 and api._marginal_loo_thin(8, 7) == 2
    for bad in (0, -1, 2.5, True):
        with pytest.raises(ValueError):
            api._marginal_loo_thin(10, bad)


# ------------------------------------------------------------------------------------------ Fit
def test_fit_plumbing_with_the_device_call_stubbed(monkeypatch):
    y = np.zeros(5)
    assert api._fit_requests(y, 2).marginal_loo is None
    assert api._fit_requests(y, 2, marginal_loo=True).marginal_loo == 2000
    assert api._fit_requests(y, 2, marginal_loo=True, marginal_loo_draws=7).marginal_loo == 7
    for bad in (0, 1.5, -3):
        with pytest.raises(ValueError):
            api._fit_requests(y, 2, marginal_loo=True, marginal_loo_draws=bad)
    with pytest.raises(ValueError):
        api._fit_requests(np.zeros(2049), 2, X_new=_capi.XInput(np.zeros((2049, 3))), nsamp=10, x_transform=False, marginal_loo=True)
    for fn in (bnr_amd.Fit, bnr_amd.generate_samples, bnr_amd.generate_samples_dbl):
        par = inspect.signature(fn).parameters
        assert par["marginal_loo"].default is False and par["marginal_loo_draws"].default == 2000, fn
    monkeypatch.setattr(api, "_rank_world", lambda: (0, 2))                         # chains spread over two ranks: refused before any sampling
    with pytest.raises(ValueError, match="marginal_loo"):
        api._fit_requests(y, 2, marginal_loo=True)
    with pytest.raises(ValueError, match="marginal_loo"):
        bnr_amd.Fit(np.zeros((5, 3)), y, 2, x_transform=False, marginal_loo=True, filename=None)
    monkeypatch.undo()

    calls = []

    def stub(chains, nburn, nsamp, thin=1, r_eff=None, per_chain=False):
        calls.append((list(chains), nburn, nsamp, thin, r_eff, per_chain))
        return {"stub": len(calls)}

    monkeypatch.setattr(api, "device_marginal_loo", stub)
    c1, c2 = types.SimpleNamespace(name=1), types.SimpleNamespace(name=2)
    cs = types.SimpleNamespace(chains={1: c1, 2: c2}, ids=[1, 2])
    base = dict(return_state=False)
    res = api._finish(cs, api.Results(None, np.zeros(1), np.zeros(1), 30, 45), api._fit_requests(y, 2, marginal_loo=True, marginal_loo_draws=20, **base), 1)
    assert res.marginal_loo == {"stub": 1} and calls[-1] == ([c1], 30, 45, 3, None, False) and res.stat_chains == 1
    res = api._finish(cs, api.Results(None, np.zeros(1), np.zeros(1), 30, 45),
                      api._fit_requests(y, 2, marginal_loo=True, pool_chains=True, loo_r_eff=0.5, **base), 1)
    assert res.marginal_loo == {"stub": 2} and calls[-1] == ([c1, c2], 30, 45, 1, 0.5, False) and res.stat_chains == 2
    assert api.MarginalLOO(res) is res.marginal_loo
    plain = api._finish(cs, api.Results(None, np.zeros(1), np.zeros(1), 30, 45), api._fit_requests(y, 2, **base), 1)
    assert len(calls) == 2 and plain.marginal_loo is None and plain.stat_chains is None
    assert plain == api.Results(None, plain.rhatxi, plain.rhatgamma, 30, 45)          # without the flag: what it was, field for field


def test_marginal_loo_accessor_falls_back_to_the_state_table():
    X, y, t = _tables(6, 2, 2, False)
    res = api.Results(t, np.zeros(1), np.zeros(1), 1, 2)
    got = api.MarginalLOO(res, X, y, x_transform=False)
    ref = api._host_marginal_loo([t], X, y, 1, 2)
    assert got["draws"] == 2 and got["thin"] == 1 and got["n_bad"] == 0 and np.array_equal(got["elpd_loo_i"], ref["elpd_loo_i"])
    ll, rs, vr, ml, _nb = api._host_marginal_loglik([t], X, y, 1, 2, 1)
    lw, e, k = api._psis_weights_host(ll)
    w = np.exp(lw)
    assert np.array_equal(got["pareto_k"], k) and np.array_equal(got["logml"], ml)
    assert np.allclose(got["loo_mean"], y - (w * rs).sum(axis=1), rtol=1e-14) and np.all(got["loo_sd"] > 0)
    assert set(api._loo_from_pointwise(e, e, k, 2)) | {"loo_mean", "loo_sd", "rmse_loo", "r2_loo", "logml", "thin", "draws", "n_bad"} == set(got)
