"""CPU tests of the chain stacking on the marginal PSIS-LOO (include/bnr_mstack.h, libbnr_mstack.so): the numpy restatement
api._host_stacked_mixture against the mpmath reference within the derived bound (tests/mstack_ref.py), the identities of the definitions on the
restatement, api._host_marginal_stack on small tables, the fact that motivates the feature on seeded CPU fits, what the library exports and which
kernels its code object holds, the ctypes signatures, the refusals and the Fit plumbing with the device calls stubbed.  No GPU."""
import ctypes as C
import dataclasses
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
import mstack_ref as sr
from bnr_amd import _capi, api
from oracle import bnr_oracle as bo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("mean", "sd", "pit", "lower", "upper")
SHAPES = ((1, 1), (1, 257), (2, 1), (2, 128), (3, 85), (3, 86), (8, 32))


def _strip_comments(src):
    return re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", src, flags=re.S))


def _host(c, w, K, rows, p_lo, p_hi, with_y=True, solver=None):
    out = api._host_stacked_mixture(c["mean"][:rows], c["var"][:rows], c["logw"][:rows], w, K, c["y"][:rows] if with_y else None, p_lo, p_hi, solver)
    return dict(zip(FIELDS, out[:5]))


# ------------------------------------------------------------------------------------------ the numpy restatement within the bound
@pytest.mark.parametrize("pattern", sr.PATTERNS)
@pytest.mark.parametrize("wname", sr.WEIGHTS)
@pytest.mark.parametrize("K,nd", SHAPES)
def test_host_restatement_meets_the_bound(K, nd, wname, pattern):
    if K == 1 and wname != "uniform":
        return                                                           # (K = 1: every weight pattern is (1,))
    p_lo, p_hi = api._loo_interval_probs(95)
    c, w = sr.case(K, nd, pattern), sr.chain_weights(K, wname)
    for rows in (1, 3):
        got = _host(c, w, K, rows, p_lo, p_hi)
        worst = sr.check_case(K, nd, pattern, wname, rows, got, p_lo, p_hi)
    if (K, nd) in ((2, 128), (3, 85)):                                   # the library's own bisection instead of brentq, and the form without y
        sr.check_case(K, nd, pattern, wname, 3, _host(c, w, K, 3, p_lo, p_hi, solver="bisect"), p_lo, p_hi)
        noy = _host(c, w, K, 3, p_lo, p_hi, with_y=False)
        assert np.isnan(noy["pit"]).all()
        sr.check_case(K, nd, pattern, wname, 3, noy, p_lo, p_hi, with_y=False)
    print("K=%d nd=%d %s %s: worst error / bound %s" % (K, nd, wname, pattern, {k: "%.3g" % v for k, v in worst.items()}))


def test_identities_of_the_definitions_on_the_restatement():
    p_lo, p_hi = api._loo_interval_probs(95)
    for pattern in ("random", "points", "nanrow"):
        c = sr.case(1, 257, pattern)                                     # K = 1 is the weighted mixture
        a = api._host_stacked_mixture(c["mean"], c["var"], c["logw"], [1.0], 1, c["y"], p_lo, p_hi)
        b = api._host_weighted_mixture(c["mean"], c["var"], c["logw"], c["y"], p_lo, p_hi)
        assert all(np.array_equal(x, z, equal_nan=True) for x, z in zip(a, b)), pattern
        K, nd = 3, 85
        c = sr.case(K, nd, pattern)
        for k in range(K):                                               # w = e_k is the weighted mixture of chain k's columns
            w = np.eye(K)[k]
            cols = slice(k * nd, (k + 1) * nd)
            a = api._host_stacked_mixture(c["mean"], c["var"], c["logw"], w, K, c["y"], p_lo, p_hi)
            b = api._host_weighted_mixture(c["mean"][:, cols], c["var"][:, cols], c["logw"][:, cols], c["y"], p_lo, p_hi)
            assert all(np.array_equal(x, z, equal_nan=True) for x, z in zip(a, b)), (pattern, k)
        w = sr.chain_weights(K, "zero")                                  # the dropped chain's columns are not read
        base = api._host_stacked_mixture(c["mean"], c["var"], c["logw"], w, K, c["y"], p_lo, p_hi)
        m, v, lw = (np.array(c[f]) for f in ("mean", "var", "logw"))
        for a in (m, v, lw):
            a[:, (K // 2) * nd:(K // 2 + 1) * nd] = np.nan
        got = api._host_stacked_mixture(m, v, lw, w, K, c["y"], p_lo, p_hi)
        assert all(np.array_equal(x, z, equal_nan=True) for x, z in zip(base, got)), pattern
    c = sr.case(2, 128, "random")                                        # a log weight that is not finite in a retained chain: the row is NaN
    lw = np.array(c["logw"])
    lw[2, 130] = -np.inf
    got = api._host_stacked_mixture(c["mean"], c["var"], lw, [0.5, 0.5], 2, c["y"], p_lo, p_hi)
    base = api._host_stacked_mixture(c["mean"], c["var"], c["logw"], [0.5, 0.5], 2, c["y"], p_lo, p_hi)
    assert all(math.isnan(got[f][2]) for f in range(5)) and all(np.array_equal(np.delete(got[f], 2), np.delete(base[f], 2)) for f in range(5))
    for bad in ([0.5, 0.6], [1.0], [0.5, np.nan], [-0.5, 1.5], [0.0, 0.0]):
        with pytest.raises((ValueError, _capi.BnrError)):
            bnr_amd.stacked_mixture(c["mean"], c["var"], c["logw"], bad, 2)


# ------------------------------------------------------------------------------------------ _host_marginal_stack on small tables
def _table(rng, tot, V, R, q):
    t = _capi.new_table(tot, V, R, dead=False)
    t["u"][:] = rng.normal(size=(tot, R, V)) * 0.7
    t["lam"][:, :, 0] = rng.integers(-1, 2, size=(tot, R))
    t["tau2"][:, 0, 0] = rng.exponential(size=tot) + 0.05
    t["mu"][:, 0, 0] = rng.normal(size=tot)
    t["S"][:, :, 0] = rng.exponential(size=(tot, q))
    return t


def test_host_marginal_stack_on_small_tables(monkeypatch):
    V, R, n, tot = 2, 2, 7, 13
    q = V * (V + 1) // 2
    rng = np.random.default_rng(189)
    X, y = rng.normal(size=(n, q)), rng.normal(size=n)
    tabs = [_table(rng, tot, V, R, q) for _ in range(3)]
    for thin, nd in ((1, 12), (5, 3)):
        got = api._host_marginal_stack(tabs, X, y, 1, 12, thin)
        assert got.chains == 3 and got.draws == 3 * nd and got.thin == thin and got.n_bad == 0 and got.logml.shape == (3 * nd,) and got.n_used == n
        ll, rs, vr, ml, _nb = api._host_marginal_loglik(tabs, X, y, 1, 12, thin)
        lws = []
        for k in range(3):                                               # chain order: row k is chain k's own LOO, on its own draws
            one = api._host_marginal_loo([tabs[k]], X, y, 1, 12, thin)
            assert np.array_equal(got.elpd_chain_i[k], one["elpd_loo_i"]) and np.array_equal(got.pareto_k[k], one["pareto_k"]), (thin, k)
            lw, e, kh = api._psis_weights_host(ll[:, k * nd:(k + 1) * nd])
            assert np.array_equal(e, got.elpd_chain_i[k])
            lws.append(lw)
        r = api._host_stacking_weights(got.elpd_chain_i.T)
        assert np.array_equal(got.weights, r["weights"]) and got.gap == r["gap"] and got.iterations == r["iterations"]
        assert abs(got.weights.sum() - 1) <= 1e-12 and got.gap <= 1e-9
        mix = api._host_stacked_mixture(y[:, None] - rs, vr, np.concatenate(lws, axis=1), got.weights, 3, y, *api._loo_interval_probs(95))
        for f, a in zip(("loo_mean", "loo_sd", "loo_pit", "loo_lower", "loo_upper"), mix):
            assert np.array_equal(getattr(got, f), a), f
        for i in range(n):                                               # the stacked score against mpmath
            ref, tol = sr.elpd_stack_ref(got.elpd_chain_i[:, i], got.weights)
            assert abs(got.elpd_stack_i[i] - ref) <= sr.GATE * tol, (i, got.elpd_stack_i[i], ref)
        assert got.elpd_stack == float(np.sum(got.elpd_stack_i)) and got.elpd_stack >= got.elpd_uniform - 1e-9 * n
        assert got.coverage == float(np.mean((y >= got.loo_lower) & (y <= got.loo_upper))) and got.ks == api._ks_uniform(got.loo_pit)
        assert np.array_equal(got.elpd_chain, got.elpd_chain_i.sum(axis=1)) and got.khat_threshold == (min(1 - 1 / math.log10(nd), 0.7))
        for k in range(3):                                               # given weights e_k: chain k's own checks
            fx = api._host_marginal_stack(tabs, X, y, 1, 12, thin, weights=np.eye(3)[k])
            one = api._host_marginal_loo_predict([tabs[k]], X, y, 1, 12, thin)
            assert math.isnan(fx.gap) and fx.iterations == 0 and np.array_equal(fx.weights, np.eye(3)[k])
            for f in ("loo_mean", "loo_sd", "loo_pit", "loo_lower", "loo_upper"):
                assert np.array_equal(getattr(fx, f), getattr(one, f)), (k, f)
            assert np.array_equal(fx.elpd_stack_i, one.elpd_loo_i) and np.array_equal(fx.elpd_chain_i, got.elpd_chain_i)
    # the chains in another order: the rows follow
    swapped = api._host_marginal_stack(tabs[::-1], X, y, 1, 12, 1)
    plain = api._host_marginal_stack(tabs, X, y, 1, 12, 1)
    assert np.array_equal(swapped.elpd_chain_i, plain.elpd_chain_i[::-1]) and np.array_equal(swapped.pareto_k, plain.pareto_k[::-1])
    # rows left out: a row whose elpd is not finite in one chain (here: PSIS refuses row 3 of chain 1) is not among the rows the solver sees
    # and NaN in the stacked score
    psis, seen = api._psis_weights_host, []

    def spoilt(ll, r_eff=None):
        lw, e, k = psis(ll, r_eff)
        seen.append(1)
        if len(seen) == 2:
            e, lw = e.copy(), lw.copy()
            e[3], lw[3] = np.nan, np.nan
        return lw, e, k

    monkeypatch.setattr(api, "_psis_weights_host", spoilt)
    part = api._host_marginal_stack(tabs, X, y, 1, 12, 1)
    monkeypatch.undo()
    keep = np.arange(n) != 3
    assert part.n_used == n - 1 and math.isnan(part.elpd_stack_i[3]) and np.isfinite(part.elpd_stack_i[keep]).all()
    r = api._host_stacking_weights(part.elpd_chain_i[:, keep].T)
    assert np.array_equal(part.weights, r["weights"]) and part.elpd_stack == float(np.sum(part.elpd_stack_i[keep]))
    assert math.isnan(part.loo_mean[3]) and math.isnan(part.loo_upper[3]) and np.isfinite(part.loo_mean[keep]).all()
    # a bad draw in chain 1: NaN in every row of its chain, no row left, weights 1 / K, every check NaN
    bad = [dict(t) for t in tabs]
    bad[1] = {k: np.array(v) for k, v in tabs[1].items()}
    bad[1]["S"][4, 1, 0] = np.nan
    got = api._host_marginal_stack(bad, X, y, 1, 12, 1)
    assert got.n_bad == 1 and got.n_used == 0 and np.array_equal(got.weights, np.full(3, 1 / 3)) and math.isnan(got.gap) and got.iterations == 0
    assert np.isnan(got.elpd_chain_i[1]).all() and np.array_equal(got.elpd_chain_i[[0, 2]], plain.elpd_chain_i[[0, 2]]) and np.isnan(got.elpd_stack_i).all()
    assert all(np.isnan(getattr(got, f)).all() for f in ("loo_mean", "loo_sd", "loo_pit", "loo_lower", "loo_upper"))
    assert math.isnan(got.coverage) and math.isnan(got.rmse_loo)
    skip = api._host_marginal_stack(bad, X, y, 1, 12, 1, weights=[0.5, 0.0, 0.5])      # ... unless its chain is dropped
    ok = api._host_marginal_stack(tabs, X, y, 1, 12, 1, weights=[0.5, 0.0, 0.5])
    assert skip.n_bad == 1 and all(np.array_equal(getattr(skip, f), getattr(ok, f)) for f in ("loo_mean", "loo_sd", "loo_pit", "loo_lower", "loo_upper"))
    with pytest.raises(ValueError):
        api._host_marginal_stack([], X, y, 1, 12)
    res = api.Results(tabs, np.zeros(1), np.zeros(1), 1, 12)                            # the accessor's fallback
    acc = api.MarginalStack(res, X, y, x_transform=False)
    same = api._host_marginal_stack(tabs, api._dense_rows(api._new_rows(X, False, q, y)), y, 1, 12)      # (the accessor's own copy of X: the same bits in the same layout)
    assert np.array_equal(acc.weights, same.weights) and np.array_equal(acc.loo_pit, same.loo_pit) and acc.interval == 95
    assert np.allclose(acc.loo_pit, plain.loo_pit, rtol=1e-10, atol=1e-13)
    with pytest.raises(ValueError):
        api.MarginalStack(api.Results(tabs[0], np.zeros(1), np.zeros(1), 1, 12), X, y)


# ------------------------------------------------------------------------------------------ the fact behind the feature
def _oracle_table(X, y, seed, chain):
    o = bo.Oracle(X, y, 3, 3000, seed, chain=chain, pdf_mode=1)
    o.init_prior()
    o.run(2, 3000, 3000)
    return o.t


def test_marginal_stacking_rests_on_usable_loo_where_the_conditional_one_does_not():
    """the seeded CPU fits of the issue: make_synthetic(60, 10, 3, seed=7), oracle chains 1 .. 4 with seed 4242, pdf_mode = 1, rows 1500 .. 2999
    (0-based) of 3000.  Conditional n_high_k (of 60) 42 38 40 40, weight 0.99999995 on chain 3; marginal 1 3 1 1, weight 0.9999997 on chain 1."""
    X, y, _ = bnr_amd.make_synthetic(60, 10, 3, seed=7)
    X, y = np.asarray(X, dtype=np.float64), np.asarray(y, dtype=np.float64)
    tabs = [_oracle_table(X, y, 4242, c) for c in (1, 2, 3, 4)]
    cond = api._host_stack_chains(tabs, X, y, 1500, 1500)
    ll = api._host_marginal_loglik(tabs, X, y, 1500, 1500)[0]
    el, kh = zip(*[api._psis_weights_host(ll[:, k * 1500:(k + 1) * 1500])[1:] for k in range(4)])
    r = api._host_stacking_weights(np.array(el).T)
    marg = api._stacking(r["weights"], np.array(el), np.array(kh), r["gap"], r["iterations"], 1500)
    print("conditional: n_high_k %s weights %s updates %d\nmarginal:    n_high_k %s weights %s updates %d"
          % (cond.n_high_k, cond.weights, cond.iterations, marg.n_high_k, marg.weights, marg.iterations))
    assert np.all(2 * marg.n_high_k <= cond.n_high_k)
    assert list(cond.n_high_k) == [42, 38, 40, 40] and list(marg.n_high_k) == [1, 3, 1, 1]
    assert int(np.argmax(cond.weights)) == 2 and int(np.argmax(marg.weights)) == 0


# ------------------------------------------------------------------------------------------ the library
def test_mstack_library_exports_exactly_what_its_header_declares():
    hdr = _strip_comments(open(os.path.join(ROOT, "include", "bnr_mstack.h")).read())
    declared = set(re.findall(r"\b(bnr_[a-zA-Z0-9_]+)\s*\(", hdr))
    assert declared == set(_capi.MSTACK_EXPORTS) and len(declared) == 4
    assert declared == {"bnr_mstack_abi_version", "bnr_mstack_set_option", "bnr_stacked_mixture", "bnr_chains_marginal_stack"}
    assert os.path.exists(bnr_amd.MSTACK_LIB), "libbnr_mstack.so has not been built"
    syms = subprocess.run(["nm", "-D", "--defined-only", bnr_amd.MSTACK_LIB], check=True, stdout=subprocess.PIPE, text=True).stdout
    defined = {line.split()[-1] for line in syms.splitlines() if line.strip()}
    assert defined == declared, defined ^ declared                               # no kernel handle, host stub or template instance is exported
    L = _capi.mstack_lib()
    assert L.bnr_mstack_abi_version() == int(re.search(r"#define BNR_MSTACK_ABI_VERSION (\d+)", hdr).group(1)) == 1
    for name in ("MarginalStack", "MarginalStacking", "stacked_mixture", "device_marginal_stack", "mstack_lib", "MSTACK_LIB"):
        assert hasattr(bnr_amd, name), name
    needed = subprocess.run(["readelf", "-d", bnr_amd.MSTACK_LIB], check=True, stdout=subprocess.PIPE, text=True).stdout
    assert "libbnr_hip.so" in needed and "$ORIGIN" in needed
    assert not [x for x in ("libbnr_mloo", "libbnr_medge", "libbnr_mpred", "libbnr_mcheck") if x in needed]


def test_mstack_code_object_holds_the_shared_kernels_and_its_own(tmp_path, monkeypatch):
    if not (co.have_tools() and os.path.exists(bnr_amd.MSTACK_LIB)):
        pytest.skip("no ROCm LLVM tools / no built library here")
    monkeypatch.setattr(co, "LIB", bnr_amd.MSTACK_LIB)
    cos = co.code_objects(tmp_path)
    assert len(cos) == 1
    own = co.declared_kernels("bnr_mstack_kernels.h")
    assert own == {"k_mstack_stage"}
    check = co.declared_kernels("bnr_mcheck_kernels.h")                          # (k_mcheck_stage comes along with the include; it is not launched)
    assert check == {"k_mcheck_stage", "k_mcheck_moments", "k_mcheck_quantile"}
    four = co.declared_kernels("bnr_mloo_kernels.h")
    assert four == {"k_mloo_w", "k_mloo_rhs", "k_mloo_gram", "k_mloo_factor"}
    assert set(cos[0]) == own | check | four, set(cos[0]) ^ (own | check | four)
    assert not (own | check | four) & {re.sub(r"<.*", "", k) for k in co.SWEEP | co.ANALYSIS}


def test_ctypes_signatures():
    L = _capi.mstack_lib()
    dp = C.c_void_p
    f = L.bnr_stacked_mixture
    assert f.argtypes == [C.c_int32] * 4 + [dp] * 5 + [C.c_double] * 2 + [dp] * 5 and f.restype is C.c_int
    f = L.bnr_chains_marginal_stack
    assert f.argtypes == ([C.POINTER(C.c_void_p)] + [C.c_int32] * 4 + [dp] * 2 + [C.c_int32] + [C.c_double] * 3 + [dp] * 4
                          + [C.POINTER(C.c_double), C.POINTER(C.c_int32)] + [dp] * 6 + [C.POINTER(C.c_int32)]) and f.restype is C.c_int
    assert L.bnr_mstack_set_option.argtypes == [C.c_char_p, C.c_int64] and L.bnr_mstack_abi_version.argtypes == []
    hdr = _strip_comments(open(os.path.join(ROOT, "include", "bnr_mstack.h")).read())
    kinds = {"int32_t": C.c_int32, "double": C.c_double, "int64_t": C.c_int64}
    for name, sig in _capi._MSTACK_SIGS.items():                                 # parameter by parameter against the header
        params = re.search(r"\b%s\s*\((.*?)\)\s*;" % name, hdr, flags=re.S).group(1).strip()
        plist = [] if params == "void" else [p_.strip() for p_ in params.split(",")]
        assert len(sig[1]) == len(plist), name
        for ct, decl in zip(sig[1], plist):
            if "*" not in decl:
                assert ct is kinds[decl.split()[0]], (name, decl)
            elif decl.startswith("int32_t *"):
                assert ct == C.POINTER(C.c_int32), (name, decl)
            elif decl.startswith("const char"):
                assert ct is C.c_char_p, (name, decl)
            else:
                assert ct in (dp, C.POINTER(C.c_double), C.POINTER(C.c_void_p)), (name, decl)


# ------------------------------------------------------------------------------------------ refusals
def test_refusals(monkeypatch):
    L = _capi.mstack_lib()
    a = np.ones(8)
    p = _capi._ptr(a)
    half = np.array([0.5, 0.5])
    err = lambda: _capi.lib().bnr_last_error()

    def raw(rows=2, K=2, nd=2, mean=p, var=p, lw=p, w=_capi._ptr(half), y=p, p_lo=0.025, p_hi=0.975, om=p, sd=None, pit=None, lo=None, hi=None):
        return L.bnr_stacked_mixture(0, rows, K, nd, mean, var, lw, w, y, p_lo, p_hi, om, sd, pit, lo, hi)

    wbad = lambda *v: _capi._ptr(np.array(v, dtype=np.float64))
    keep = [np.array(v, dtype=np.float64) for v in ((0.5, 0.6), (0.5, np.nan), (-0.5, 1.5), (0.0, 0.0), (np.inf, 0.0))]
    for kw, word in ((dict(mean=None), b"NULL"), (dict(var=None), b"NULL"), (dict(lw=None), b"NULL"), (dict(w=None), b"NULL"),
                     (dict(om=None), b"at least one"), (dict(K=0), b"nchains"), (dict(K=33), b"nchains"), (dict(rows=0), b"rows >= 1"),
                     (dict(nd=0), b"rows >= 1"), (dict(rows=1 << 16, nd=1 << 14), b"2^31"), (dict(y=None, pit=p), b"pit needs y"),
                     (dict(lo=p, p_lo=0.0), b"p_lo"), (dict(hi=p, p_lo=0.6, p_hi=0.5), b"p_lo"), (dict(lo=p, p_lo=float("nan")), b"p_lo"),
                     (dict(w=_capi._ptr(keep[0])), b"sum to 1"), (dict(w=_capi._ptr(keep[1])), b"finite"), (dict(w=_capi._ptr(keep[2])), b"finite"),
                     (dict(w=_capi._ptr(keep[3])), b"one weight"), (dict(w=_capi._ptr(keep[4])), b"finite")):
        assert raw(**kw) == _capi.BNR_ERR_BAD_ARG and word in err(), kw
    h = (C.c_void_p * 1)(None)
    g, it = C.c_double(0.0), C.c_int32(0)

    def chain(ch=h, K=1, first=1, ns=1, thin=1, w=p, el=p, kh=p):
        return L.bnr_chains_marginal_stack(ch, K, first, ns, thin, None, None, 100, 1e-9, 0.025, 0.975, w, el, kh, None, C.byref(g), C.byref(it),
                                           None, None, None, None, None, None, None)

    assert chain(ch=None) == 1 and b"NULL argument" in err()                       # bnr_chains_marginal_loo's refusals, in its order
    assert chain(w=None) == 1 and b"NULL argument" in err()
    assert chain(el=None) == 1 and b"NULL argument" in err()
    assert chain(kh=None) == 1 and b"NULL argument" in err()
    assert chain(K=0) == 1 and b"nchains" in err()
    assert chain(thin=0) == 1 and b"thin" in err()
    assert chain() == 1 and b"NULL chain" in err()
    M = _capi.mloo_lib()
    assert M.bnr_chains_marginal_loo(h, 1, 1, 1, 1, None, p, p, None, None, None, None, None) == 1 and b"NULL chain" in err()
    assert L.bnr_mstack_set_option(b"no_such", 1) == 1 and L.bnr_mstack_set_option(b"mstack_batch_draws", -1) == 1 and L.bnr_mstack_set_option(None, 1) == 1
    assert L.bnr_mstack_set_option(b"mcheck_batch_draws", 1) == 1                  # (the other library's option)
    assert L.bnr_mstack_set_option(b"mstack_batch_draws", 0) == 0
    m = np.ones((3, 4))
    for args in ((np.ones(4), np.ones(4), np.ones(4), half, 2), (m, np.ones((3, 5)), m, half, 2), (m, m, np.ones((4, 3)), half, 2),
                 (m, m, m, np.ones(3) / 3, 3), (m, m, m, half, 0), (m, m, m, np.ones(3) / 3, 2)):
        with pytest.raises(ValueError):
            bnr_amd.stacked_mixture(*args)
    with pytest.raises(ValueError):
        bnr_amd.stacked_mixture(m, m, m, half, 2, y=np.ones(4))
    with pytest.raises(ValueError):
        bnr_amd.stacked_mixture(m, m, m, half, 2, interval=100)
    with pytest.raises(ValueError):
        _capi.stacked_mixture_raw(m, m, m, half, 2, fields=("pit",))                # pit only with y
    big = np.lib.stride_tricks.as_strided(np.ones(1), shape=(46341, 46342), strides=(0, 0))     # (a view of one double: refused before any copy)
    with pytest.raises(ValueError, match="2\\^31"):
        _capi.stacked_mixture_raw(big, big, big, half, 2)
    y = np.zeros(5)
    with pytest.raises(ValueError, match="2048"):
        api._fit_requests(np.zeros(2049), 2, X_new=_capi.XInput(np.zeros((2049, 3))), nsamp=10, x_transform=False, marginal_stack=True)
    with pytest.raises(ValueError, match="num_chains >= 2"):
        api._fit_requests(y, 1, marginal_stack=True)
    with pytest.raises(ValueError, match="at most 32"):
        api._fit_requests(y, 33, marginal_stack=True)
    for bad in (0, 1.5, -3, True):
        with pytest.raises(ValueError):
            api._fit_requests(y, 2, marginal_stack=True, marginal_loo_draws=bad)
    with pytest.raises(ValueError):
        api._fit_requests(y, 2, marginal_stack=True, predict_interval=100)
    monkeypatch.setattr(api, "_rank_world", lambda: (0, 2))                         # chains spread over two ranks: refused before any sampling
    with pytest.raises(ValueError, match="marginal_stack"):
        api._fit_requests(y, 2, marginal_stack=True)
    with pytest.raises(ValueError, match="marginal_stack"):
        bnr_amd.Fit(np.zeros((5, 3)), y, 2, x_transform=False, marginal_stack=True, num_chains=2, filename=None)
    monkeypatch.undo()
    with pytest.raises(ValueError, match="num_chains >= 2"):
        bnr_amd.Fit(np.zeros((5, 3)), y, 2, x_transform=False, marginal_stack=True, num_chains=1, filename=None)
    fake = types.SimpleNamespace(n=2049, q=3, h=None)
    monkeypatch.setattr(_capi, "_pooled", lambda chains: (fake, (None, 1)))
    with pytest.raises(ValueError, match="2048"):
        _capi.chains_marginal_stack([fake], 1, 10)
    monkeypatch.undo()
    for kw in (dict(max_iter=0), dict(gap_tol=0.0), dict(gap_tol=float("inf")), dict(interval=100), dict(thin=0)):
        with pytest.raises(ValueError):
            api.device_marginal_stack([fake], 0, 10, **kw)
    with pytest.raises(ValueError):
        api.MarginalStack(api.Results(None, np.zeros(1), np.zeros(1), 0, 1))


# ------------------------------------------------------------------------------------------ Fit
def test_fit_plumbing_with_the_device_calls_stubbed(monkeypatch):
    y = np.zeros(5)
    assert api._fit_requests(y, 2).marginal_stack is None
    assert api._fit_requests(y, 2, marginal_stack=True).marginal_stack == (2000, 95)
    assert api._fit_requests(y, 2, marginal_stack=True, marginal_loo_draws=7, predict_interval=50).marginal_stack == (7, 50)
    for fn in (bnr_amd.Fit, bnr_amd.generate_samples, bnr_amd.generate_samples_dbl, api._fit_requests):
        par = inspect.signature(fn).parameters
        assert par["marginal_stack"].default is False and list(par)[-2:] == ["marginal_stack", "marginal_loo_predict"], fn   # (an earlier test pins marginal_loo_predict as the last keyword: the new one goes just ahead of it)
    names = [f.name for f in dataclasses.fields(api.Results)]
    assert names[-2:] == ["marginal_stacking", "marginal_loo_predictive"]          # (likewise: the field pinned as the last one stays the last)
    assert {f.name: f.default for f in dataclasses.fields(api.Results)}["marginal_stacking"] is None
    cs_fields = [f.name for f in dataclasses.fields(api.ChainStacking)][:15]
    ms_fields = [f.name for f in dataclasses.fields(api.MarginalStacking)]
    assert ms_fields[:15] == cs_fields and cs_fields[-1] == "draws"
    assert ms_fields[15:] == ["loo_mean", "loo_sd", "loo_pit", "loo_lower", "loo_upper", "coverage", "ks", "rmse_loo", "r2_loo", "interval", "thin",
                              "n_bad", "logml", "summary", "prediction", "edge_cov", "marginal_edges", "marginal_prediction"]

    calls = {k: [] for k in ("mstack", "stack", "summary", "predict", "cov", "medges", "mpred")}
    wm, wc = np.array([0.25, 0.75]), np.array([0.9, 0.1])

    def mstack(chains, nburn, nsamp, thin=1, interval=95, r_eff=None, weights=None, max_iter=100000, gap_tol=1e-9):
        calls["mstack"].append((list(chains), nburn, nsamp, thin, interval, r_eff, weights))
        return types.SimpleNamespace(weights=wm, summary=None, prediction=None, edge_cov=None, marginal_edges=None, marginal_prediction=None)

    def stack(chains, nb, ns, r_eff):
        calls["stack"].append(list(chains))
        return types.SimpleNamespace(weights=wc, summary=None, prediction=None, edge_cov=None, marginal_edges=None)

    def named(key):
        def f(chains, *a, **kw):
            calls[key].append((list(chains), a, kw))
            return (key, len(calls[key]))
        return f

    monkeypatch.setattr(api, "device_marginal_stack", mstack)
    monkeypatch.setattr(api, "device_stack_chains", stack)
    monkeypatch.setattr(api, "device_summary_stacked", named("summary"))
    monkeypatch.setattr(api, "device_predict_stacked", named("predict"))
    monkeypatch.setattr(api, "device_edge_cov", named("cov"))
    monkeypatch.setattr(api, "device_marginal_edges", named("medges"))
    monkeypatch.setattr(api, "device_marginal_predict", named("mpred"))
    monkeypatch.setattr(api, "device_summary", lambda ch, nb, ns, iv: ("one", iv))
    c1, c2 = types.SimpleNamespace(name=1), types.SimpleNamespace(name=2)
    cs = types.SimpleNamespace(chains={1: c1, 2: c2}, ids=[1, 2])
    base = dict(return_state=False)
    new = lambda: api.Results(None, np.zeros(1), np.zeros(1), 30, 45)
    res = api._finish(cs, new(), api._fit_requests(y, 2, marginal_stack=True, marginal_loo_draws=20, loo_r_eff=0.5, predict_interval=50, **base), 1)
    ms = res.marginal_stacking
    assert calls["mstack"][-1] == ([c1, c2], 30, 45, 3, 50, 0.5, None)                 # every chain, thin = ceil(45 / 20); no weighted call unasked
    assert ms.summary is None and ms.edge_cov is None and ms.marginal_edges is None and res.stacking is None and res.stat_chains is None
    assert not calls["summary"] and not calls["cov"] and not calls["medges"] and api.MarginalStack(res) is ms
    # the fit's other requests under the record's weights, through the existing weighted calls
    res = api._finish(cs, new(), api._fit_requests(y, 2, marginal_stack=True, summary_interval=90, edge_cov=True, marginal_edges=True,
                                                   marginal_edges_draws=9, **base), 1)
    ms = res.marginal_stacking
    assert ms.summary == ("summary", 1) and calls["summary"][-1][0] == [c1, c2] and calls["summary"][-1][1][0] is wm and calls["summary"][-1][1][1:] == (30, 45, 90)
    assert [c[1][3] if len(c[1]) > 3 else None for c in calls["cov"]] == [None, wm] and ms.edge_cov == ("cov", 2) and res.edge_cov == ("cov", 1)
    assert [c[1][3] for c in calls["medges"]] == [wm, None] and ms.marginal_edges == ("medges", 1) and res.marginal_edges == ("medges", 2)
    assert calls["medges"][0][1][2] == 5 and calls["medges"][0][0] == [c1, c2] and calls["medges"][1][0] == [c1]
    assert res.summary_device == ("one", 90)
    # stack_chains beside it: both records, each under its own weights, independently
    for k in calls:
        calls[k].clear()
    res = api._finish(cs, new(), api._fit_requests(y, 2, marginal_stack=True, stack_chains=True, summary_interval=95, **base), 1)
    assert res.stacking.weights is wc and res.marginal_stacking.weights is wm and len(calls["stack"]) == 1 and len(calls["mstack"]) == 1
    assert [c[1][0] for c in calls["summary"]] == [wc, wm] and res.stacking.summary == ("summary", 1) and res.marginal_stacking.summary == ("summary", 2)
    assert not hasattr(res.stacking, "marginal_prediction")
    # without the flag: no call, and the Results field for field what it was
    plain = api._finish(cs, new(), api._fit_requests(y, 2, stack_chains=True, summary_interval=95, **base), 1)
    assert len(calls["mstack"]) == 1 and plain.marginal_stacking is None
    for f in api.Results.__dataclass_fields__:
        if f not in ("marginal_stacking", "stacking"):
            a, b = getattr(plain, f), getattr(res, f)
            assert (a is b) or np.array_equal(a, b) or a == b, f
    bare = api._finish(cs, new(), api._fit_requests(y, 2, **base), 1)
    assert bare == api.Results(None, bare.rhatxi, bare.rhatgamma, 30, 45) and bare.marginal_stacking is None
