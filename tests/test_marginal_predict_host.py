"""CPU tests of the Rao-Blackwellised prediction of new rows (include/bnr_mpred.h, libbnr_mpred.so): the two statements of the mpmath reference
against each other, the numpy restatement api._host_predict_terms against the reference within the derived bound (tests/mpred_ref.py), the
identities at X* = X against the marginal leave-one-out terms, the law of total expectation on a seeded CPU fit, api._host_mixture_score, what the
library exports and which kernels its code object holds, the refusals and the Fit plumbing with the device call stubbed.  No GPU."""
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
import mloo_ref as mr
import mpred_ref as pr
from bnr_amd import _capi, api
from oracle import bnr_oracle as bo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST_Q = (1, 3, 15, 45)
HOST_M = (1, 3, 17)


def _strip_comments(src):
    return re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", src, flags=re.S))


# ------------------------------------------------------------------------------------------ the reference
@pytest.mark.parametrize("n,q,m", [(1, 1, 1), (2, 3, 3), (15, 4, 2), (16, 17, 5), (17, 45, 3)])
def test_the_two_statements_of_the_reference_agree(n, q, m):
    c = mr.case(n, q)
    Xn = pr.new_rows(q)[:m]
    for d in (0, 1, 2):
        a = pr.a_inverse(c["X"], c["y"], Xn, c["tau2"][d], c["mu"][d], c["S"][d], c["W"][d])
        bm, bv = pr.precision(c["X"], c["y"], Xn, c["tau2"][d], c["mu"][d], c["S"][d], c["W"][d])
        for j in range(m):
            assert abs(a["mean"][j] - bm[j]) <= 1e-40 * max(1, abs(bm[j])), ("mean", j, d)
            assert abs(a["var"][j] - bv[j]) <= 1e-40 * max(1, abs(bv[j])), ("var", j, d)


# ------------------------------------------------------------------------------------------ the numpy restatement within the bound
@pytest.mark.parametrize("binary", (False, True))
@pytest.mark.parametrize("q", HOST_Q)
@pytest.mark.parametrize("n", range(1, 34))
def test_host_restatement_meets_the_bound(n, q, binary):
    """draws 0, 1, 2 of mloo_ref.case: the three S scales.  A new row's reference does not depend on the other rows, so it is computed once for
    17 rows and every m takes its prefix"""
    c = mr.case(n, q, binary)
    worst = 0.0
    for m in HOST_M:
        Xn = pr.new_rows(q, binary)[:m]
        mean, var, nb = api._host_predict_terms(c["X"], c["y"], Xn, c["tau2"][:3], c["mu"][:3], c["S"][:3], c["W"][:3])
        assert nb == 0 and mean.shape == var.shape == (3, m)
        for d in range(3):
            ref = pr.case_reference(n, q, d, max(HOST_M), binary)
            assert ref["beta_lam"] <= 0.1
            for name, got in (("mean", mean), ("var", var)):
                ratio = pr.ratio(got[d], ref[name][:m], ref["tol_" + name][:m])
                assert np.all(np.isfinite(got[d])) and np.all(ratio <= 2.0), (name, d, m, float(ratio.max()))
                worst = max(worst, float(ratio.max()))
            assert np.all(var[d] >= 0)
    print("n=%d q=%d binary=%d: worst error / bound %.3g" % (n, q, binary, worst))


@pytest.mark.parametrize("n,q", [(1, 1), (3, 3), (16, 15), (17, 45), (33, 45), (33, 3)])
def test_at_the_training_rows_the_terms_are_those_of_marginal_loo(n, q):
    """X* = X: mean_i = y_i - resid_i (tau2 / var_i) and var_i = tau2 (1 - tau2 / var_i) with resid, var of the marginal leave-one-out terms
    (E[eta_i | y] = y_i - (A^-1 r)_i, Var = tau2 (1 - (A^-1)_ii)), within the two bounds: this module's for the left-hand side, mloo_ref's
    propagated through the formula for the right-hand side"""
    c = mr.case(n, q)
    D = 3
    mean, var, nb = api._host_predict_terms(c["X"], c["y"], c["X"], c["tau2"][:D], c["mu"][:D], c["S"][:D], c["W"][:D])
    ll, rs, vr, ml, nb2 = api._host_marginal_terms(c["X"], c["y"], c["tau2"][:D], c["mu"][:D], c["S"][:D], c["W"][:D])
    assert nb == 0 and nb2 == 0
    for d in range(D):
        t2 = c["tau2"][d]
        pb = pr.numpy_bounds(c["X"], c["y"], c["X"], t2, c["mu"][d], c["S"][d], c["W"][d])
        lb = mr.numpy_bounds(c["X"], c["y"], t2, c["mu"][d], c["S"][d], c["W"][d])
        ci = t2 / vr[:, d]
        # g_i = resid_i c_i and c_i = tau2 / var_i: first-order errors of the right-hand sides, plus 4 u per formula
        tol_g = lb["tol_resid"] * ci + np.abs(rs[:, d]) * ci * (lb["tol_var"] / vr[:, d])
        tol_rm = tol_g + 4 * mr.U * (np.abs(c["y"]) + np.abs(rs[:, d] * ci))
        tol_rv = t2 * ci * (lb["tol_var"] / vr[:, d]) + 4 * mr.U * t2
        rm = c["y"] - rs[:, d] * (t2 / vr[:, d])
        rv = t2 * (1.0 - t2 / vr[:, d])
        assert np.all(np.abs(mean[d] - rm) <= 2.0 * (pb["tol_mean"] + tol_rm)), float(np.max(np.abs(mean[d] - rm) / (pb["tol_mean"] + tol_rm)))
        assert np.all(np.abs(var[d] - rv) <= 2.0 * (pb["tol_var"] + tol_rv)), float(np.max(np.abs(var[d] - rv) / (pb["tol_var"] + tol_rv)))


def test_host_restatement_bad_draws():
    c = mr.case(5, 3)
    Xn = pr.new_rows(3)[:4]
    S = c["S"][:4].copy()
    good = api._host_predict_terms(c["X"], c["y"], Xn, c["tau2"][:4], c["mu"][:4], S, c["W"][:4])
    S[1, 2] = np.nan
    S[3] = -1e6
    mean, var, nb = api._host_predict_terms(c["X"], c["y"], Xn, c["tau2"][:4], c["mu"][:4], S, c["W"][:4])
    assert nb == 2 and np.isnan(mean[[1, 3]]).all() and np.isnan(var[[1, 3]]).all()
    assert np.array_equal(mean[[0, 2]], good[0][[0, 2]]) and np.array_equal(var[[0, 2]], good[1][[0, 2]])
    nw = api._host_predict_terms(c["X"], c["y"], Xn, c["tau2"][:1], c["mu"][:1], c["S"][:1], None)
    zw = api._host_predict_terms(c["X"], c["y"], Xn, c["tau2"][:1], c["mu"][:1], c["S"][:1], np.zeros((1, 3)))
    assert np.array_equal(nw[0], zw[0]) and np.array_equal(nw[1], zw[1])


# ------------------------------------------------------------------------------------------ the seeded CPU fit of the issue
@functools.lru_cache(maxsize=None)
def _fit():
    """n = 60, V = 10, R = 3, 3000 rows, seed 4242 (the fit of tests/test_marginal_loo_host.py): (X, y, table), and 20 held-out rows"""
    X, y, _ = bnr_amd.make_synthetic(60, 10, 3, seed=7)
    o = bo.Oracle(X, y, 3, 3000, 4242, chain=1, pdf_mode=1)
    o.init_prior()
    o.run(2, 3000, 3000)
    Xn, _yn, _ = bnr_amd.make_synthetic(20, 10, 3, seed=8)
    return np.asarray(X, dtype=np.float64), np.asarray(y, dtype=np.float64).reshape(-1), o.t, np.asarray(Xn, dtype=np.float64)


def _w_of(u, lam):
    """W (rows x q) from u (rows, R, V) and lambda (rows, R): W_e = sum_t u[t, l(e)] lambda_t u[t, k(e)], t ascending"""
    ek, el = api._edge_nodes_all(u.shape[2])
    w = np.zeros((u.shape[0], ek.size))
    for t in range(u.shape[1]):
        w = w + u[:, t, :][:, el] * lam[:, t][:, None] * u[:, t, :][:, ek]
    return w


def test_total_expectation_on_the_seeded_fit():
    """gamma[i] is drawn given (tau2[i], u[i], lambda[i - 1], S[i - 1], mu[i - 1]) (update_gamma!, gibbs.jl:420-436), so with phi taken from exactly
    those values E[mu[i - 1] + x* . gamma[i] | phi] is the Rao-Blackwellised mean of the draw: the mean of the difference over rows 1500 .. 2999 is
    within 6 batch-means standard errors of 0 for every new row (30 batches of 50)"""
    X, y, t, Xn = _fit()
    i = np.arange(1500, 3000)
    mean, var, nb = api._host_predict_terms(X, y, Xn, t["tau2"][i, 0, 0], t["mu"][i - 1, 0, 0], t["S"][i - 1, :, 0],
                                            _w_of(t["u"][i], t["lam"][i - 1, :, 0]))
    assert nb == 0 and np.all(var >= 0)
    eta = t["mu"][i - 1, 0, 0][:, None] + t["gamma"][i, :, 0] @ Xn.T
    d = (mean - eta).reshape(30, 50, -1).mean(axis=1)
    se = d.std(axis=0, ddof=1) / math.sqrt(30.0)
    gap = np.abs(d.mean(axis=0))
    bm = lambda a: a.reshape(30, 50, -1).mean(axis=1).var(axis=0, ddof=1)
    rat = bm(eta) / bm(mean)
    share = var.mean(axis=0) / eta.var(axis=0)
    print("largest gap %.3g se; E[var] / Var eta: %.2f .. %.2f (median %.2f); batch-means variance ratio: median %.2f (%.2f .. %.2f)"
          % (float(np.max(gap / se)), share.min(), share.max(), np.median(share), np.median(rat), rat.min(), rat.max()))
    assert np.all(gap <= 6.0 * se), float(np.max(gap / se))


# ------------------------------------------------------------------------------------------ the mixture score on the host
def _mix(nd, K, m, seed=0):
    rng = np.random.default_rng([185, nd, K, m, seed])
    return rng.normal(size=(K * nd, m)) * 2.0 + rng.normal(size=m), rng.exponential(size=(K * nd, m)) + 0.01, rng.normal(size=m) * 2.0


def _mp_lpd(mean, vobs, y, w, nd):
    """log sum_s omega_s N(y | mean_s, vobs_s) of one column in mpmath"""
    with mp.workdps(50):
        tot = mp.mpf(0)
        for s in range(mean.size):
            v, dl = mp.mpf(float(vobs[s])), mp.mpf(float(y)) - mp.mpf(float(mean[s]))
            tot += mp.mpf(float(w[s // nd])) / nd * mp.exp(-(mp.log(2 * mp.pi) + mp.log(v)) / 2 - dl * dl / v / 2)
        return mp.log(tot)


def test_host_mixture_score_weights():
    mean, vobs, y = _mix(70, 3, 4)
    a = api._host_mixture_score(mean, vobs, y, 3)
    b = api._host_mixture_score(mean, vobs, y, 3, weights=np.full(3, 1.0 / 3.0))
    assert np.array_equal(a["lpd"], b["lpd"]) and np.array_equal(a["pit"], b["pit"])
    for k in range(3):
        w = np.zeros(3)
        w[k] = 1.0
        one = api._host_mixture_score(mean, vobs, y, 3, weights=w)
        own = api._host_mixture_score(mean[k * 70:(k + 1) * 70], vobs[k * 70:(k + 1) * 70], y, 1)
        assert np.array_equal(one["lpd"], own["lpd"]) and np.array_equal(one["pit"], own["pit"]), k
    # against mpmath: 70 terms per chain of relative error <= (a few u) (1 + |l|) each, |l| < 40 here, and the sums: 1e-13 is ample and 1000 times
    # below anything a wrong weight or order would give
    w = np.array([0.2, 0.5, 0.3])
    got = api._host_mixture_score(mean, vobs, y, 3, weights=w)
    for j in range(4):
        assert abs(mp.mpf(float(got["lpd"][j])) - _mp_lpd(mean[:, j], vobs[:, j], y[j], w, 70)) <= 1e-13 * 40
    assert np.all((got["pit"] > 0) & (got["pit"] < 1))


def test_host_mixture_score_one_normal_point_mass_tail_and_nan():
    # one normal: every component the same -> the closed form
    mu, var, y = 0.75, 2.25, 1.5
    one = api._host_mixture_score(np.full((130, 1), mu), np.full((130, 1), var), [y], 2)
    ref_l = -0.5 * (math.log(2 * math.pi) + math.log(var)) - 0.5 * (y - mu) ** 2 / var
    ref_p = 0.5 * math.erfc(-((y - mu) / 1.5) / math.sqrt(2.0))
    assert abs(one["lpd"][0] - ref_l) <= 8 * mr.EPS * (1 + abs(ref_l)) and abs(one["pit"][0] - ref_p) <= 8 * mr.EPS
    # point masses: pit counts the components at or below y; lpd is +inf on a point mass, -inf where there is nothing else
    m = np.array([[-1.0], [2.0], [3.0], [0.0]])
    z = np.zeros((4, 1))
    s = api._host_mixture_score(m, z, [2.0], 1)
    assert s["pit"][0] == 0.75 and s["lpd"][0] == np.inf
    s = api._host_mixture_score(m, z, [1.0], 1)
    assert s["pit"][0] == 0.5 and s["lpd"][0] == -np.inf
    v = z.copy()
    v[1, 0] = 1.0                                                                  # one normal N(2, 1) among three point masses
    s = api._host_mixture_score(m, v, [1.0], 1)
    assert abs(s["lpd"][0] - (math.log(0.25) - 0.5 * math.log(2 * math.pi) - 0.5)) <= 8 * mr.EPS * 3
    assert abs(s["pit"][0] - (0.5 + 0.25 * 0.5 * math.erfc(1.0 / math.sqrt(2.0)))) <= 8 * mr.EPS
    # a chain of weight 0 takes no part in lpd, even where y sits on one of its point masses
    s = api._host_mixture_score(np.array([[1.0], [0.0]]), np.array([[0.0], [1.0]]), [1.0], 2, weights=[0.0, 1.0])
    assert abs(s["lpd"][0] - (-0.5 * math.log(2 * math.pi) - 0.5)) <= 8 * mr.EPS and s["pit"][0] == 0.5 * math.erfc(-1.0 / math.sqrt(2.0)) * 1.0
    # a tail at 30 sd keeps its relative precision
    tail = api._host_mixture_score(np.full((3, 1), 30.0), np.ones((3, 1)), [0.0], 1)
    with mp.workdps(50):
        ref = mp.erfc(mp.mpf(30) / mp.sqrt(2)) / 2
        assert abs(mp.mpf(float(tail["pit"][0])) - ref) <= mp.mpf("1e-12") * ref
    assert abs(tail["lpd"][0] - (-0.5 * math.log(2 * math.pi) - 450.0)) <= 8 * mr.EPS * 451
    # NaN: the row, and only the row
    mean, vobs, y = _mix(65, 2, 5)
    s = api._host_mixture_score(mean, vobs, y, 2)
    for what in ("mean", "vobs", "y", "neg"):
        a, b, c = mean.copy(), vobs.copy(), y.copy()
        if what == "mean":
            a[7, 2] = np.nan
        elif what == "vobs":
            b[7, 2] = np.nan
        elif what == "neg":
            b[7, 2] = -1.0
        else:
            c[2] = np.nan
        sn = api._host_mixture_score(a, b, c, 2)
        for k in ("lpd", "pit"):
            assert np.isnan(sn[k][2]) and np.array_equal(np.delete(sn[k], 2), np.delete(s[k], 2)), (what, k)
    # ... also in a chain of weight 0
    a = mean.copy()
    a[7, 2] = np.nan
    sn = api._host_mixture_score(a, vobs, y, 2, weights=[0.0, 1.0])
    assert np.isnan(sn["lpd"][2]) and np.isnan(sn["pit"][2]) and not np.isnan(np.delete(sn["lpd"], 2)).any()


# ------------------------------------------------------------------------------------------ the library
def test_mpred_library_exports_exactly_what_its_header_declares():
    hdr = _strip_comments(open(os.path.join(ROOT, "include", "bnr_mpred.h")).read())
    declared = set(re.findall(r"\b(bnr_[a-zA-Z0-9_]+)\s*\(", hdr))
    assert declared == set(_capi.MPRED_EXPORTS) and len(declared) == 5
    assert os.path.exists(bnr_amd.MPRED_LIB), "libbnr_mpred.so has not been built"
    syms = subprocess.run(["nm", "-D", "--defined-only", bnr_amd.MPRED_LIB], check=True, stdout=subprocess.PIPE, text=True).stdout
    defined = {line.split()[-1] for line in syms.splitlines() if line.strip()}
    assert defined == declared, defined ^ declared                               # no kernel handle, host stub or template instance is exported
    L = _capi.mpred_lib()
    assert L.bnr_mpred_abi_version() == int(re.search(r"#define BNR_MPRED_ABI_VERSION (\d+)", hdr).group(1)) == 1
    for name in ("MarginalPredict", "MarginalPrediction", "marginal_predict_terms", "mixture_score", "device_marginal_predict", "mpred_lib", "MPRED_LIB"):
        assert hasattr(bnr_amd, name), name
    needed = subprocess.run(["readelf", "-d", bnr_amd.MPRED_LIB], check=True, stdout=subprocess.PIPE, text=True).stdout
    assert "libbnr_hip.so" in needed and "$ORIGIN" in needed and "libbnr_mloo" not in needed and "libbnr_medge" not in needed


def test_mpred_code_object_holds_the_six_kernels_and_its_own(tmp_path, monkeypatch):
    if not (co.have_tools() and os.path.exists(bnr_amd.MPRED_LIB)):
        pytest.skip("no ROCm LLVM tools / no built library here")
    monkeypatch.setattr(co, "LIB", bnr_amd.MPRED_LIB)
    cos = co.code_objects(tmp_path)
    assert len(cos) == 1
    own = co.declared_kernels("bnr_mpred_kernels.h")
    assert own == {"k_mpred_rhs", "k_mpred_cross", "k_mpred_proj", "k_mpred_score"}
    six = co.declared_kernels("bnr_medge_kernels.h") | co.declared_kernels("bnr_mloo_kernels.h")
    declared = own | six
    assert len(six) == 6 and len(declared) == 10 and set(cos[0]) == declared, set(cos[0]) ^ declared
    assert not declared & {re.sub(r"<.*", "", k) for k in co.SWEEP | co.ANALYSIS}


# ------------------------------------------------------------------------------------------ refusals
def test_refusals():
    L = _capi.mpred_lib()
    a = np.ones(8)
    p = _capi._ptr(a)
    err = lambda: _capi.lib().bnr_last_error()

    def raw(n=2, q=2, m=2, D=1, X=p, y=p, Xn=p, t2=p, mu=p, S=p, mean=p, var=None):
        return L.bnr_marginal_predict(0, n, q, m, D, X, y, Xn, t2, mu, S, None, mean, var, None)

    for kw, word in ((dict(X=None), b"NULL"), (dict(Xn=None), b"NULL"), (dict(S=None), b"NULL"), (dict(mean=None), b"mean or var"), (dict(n=0), b"n >= 1"),
                     (dict(q=0), b"n >= 1"), (dict(D=0), b"n >= 1"), (dict(m=0), b"m >= 1"), (dict(n=2049), b"2048")):
        assert raw(**kw) == _capi.BNR_ERR_BAD_ARG and word in err(), kw

    def score(m=1, K=2, nd=2, mean=p, vobs=p, y=p, w=None, lpd=p, pit=None):
        return L.bnr_mixture_score(0, m, K, nd, mean, vobs, y, w, lpd, pit)

    for kw, word in ((dict(mean=None), b"NULL"), (dict(y=None), b"NULL"), (dict(m=0), b"m >= 1"), (dict(K=0), b"m >= 1"), (dict(nd=0), b"m >= 1"),
                     (dict(lpd=None), b"lpd or pit"), (dict(w=_capi._ptr(np.array([0.5, 0.6]))), b"sum to 1"),
                     (dict(w=_capi._ptr(np.array([1.5, -0.5]))), b">= 0"), (dict(w=_capi._ptr(np.array([np.nan, 1.0]))), b"finite"),
                     (dict(K=33, nd=1, w=p), b"32")):
        assert score(**kw) == _capi.BNR_ERR_BAD_ARG and word in err(), kw
    h = (C.c_void_p * 1)(None)

    def chain(ch=h, K=1, first=1, ns=1, thin=1, Xn=p, m=1, yn=None, mean=p, lower=None, upper=None, lpd=None):
        return L.bnr_chains_marginal_predict(ch, K, None, first, ns, thin, Xn, m, yn, 0.025, 0.975, mean, None, None, lower, upper, None, None, None, lpd,
                                             None, None, None, None)

    assert chain(ch=None) == 1 and chain(K=0) == 1 and chain(Xn=None) == 1
    assert chain(thin=0) == 1 and b"thin" in err()
    assert chain(m=0) == 1 and b"m >= 1" in err()
    assert chain() == 1 and b"NULL chain" in err()
    one = (C.c_void_p * 1)(1)                                                      # (never dereferenced: the argument checks come first)
    assert chain(ch=one, mean=None) == 1 and b"at least one" in err()
    assert chain(ch=one, lpd=p) == 1 and b"ynew" in err()
    assert chain(ch=one, lower=p) == 1 and b"together" in err()
    assert L.bnr_mpred_set_option(b"no_such", 1) == 1 and L.bnr_mpred_set_option(b"mpred_batch_draws", -1) == 1 and L.bnr_mpred_set_option(None, 1) == 1
    assert L.bnr_mpred_set_option(b"mpred_block_rows", -1) == 1 and L.bnr_mpred_set_option(b"medge_batch_draws", 1) == 1   # (the other library's option)
    assert L.bnr_mpred_set_option(b"mpred_batch_draws", 0) == 0 and L.bnr_mpred_set_option(b"mpred_block_rows", 0) == 0
    X, y, Xn = np.ones((3, 2)), np.ones(3), np.ones((4, 2))
    for args in ((np.ones(3), y, Xn, [1.0], [0.0], np.ones((1, 2))), (X, np.ones(4), Xn, [1.0], [0.0], np.ones((1, 2))), (X, y, np.ones((4, 3)), [1.0], [0.0], np.ones((1, 2))),
                 (X, y, np.ones(2), [1.0], [0.0], np.ones((1, 2))), (X, y, Xn, [1.0], [0.0, 1.0], np.ones((1, 2))), (X, y, Xn, [1.0], [0.0], np.ones((1, 3))),
                 (np.ones((2049, 1)), np.ones(2049), np.ones((1, 1)), [1.0], [0.0], np.ones((1, 1)))):
        with pytest.raises(ValueError):
            bnr_amd.marginal_predict_terms(*args)
    with pytest.raises(ValueError):
        bnr_amd.marginal_predict_terms(X, y, Xn, [1.0], [0.0], np.ones((1, 2)), W=np.ones((2, 2)))
    for args, kw in (((np.ones((4, 2)), np.ones((4, 3)), np.ones(2)), {}), ((np.ones((5, 2)), np.ones((5, 2)), np.ones(2)), dict(nchains=2)),
                     ((np.ones(4), np.ones(4), np.ones(1)), {}), ((np.ones((4, 2)), np.ones((4, 2)), np.ones(3)), {}),
                     ((np.ones((4, 2)), np.ones((4, 2)), np.ones(2)), dict(nchains=2, weights=[1.0]))):
        with pytest.raises(ValueError):
            bnr_amd.mixture_score(*args, **kw)
    with pytest.raises(ValueError):
        _capi.mixture_score_raw(np.ones((4, 2)), np.ones((4, 2)), np.ones(2), fields=("mean",))
    res = api.Results(None, np.zeros(1), np.zeros(1), 0, 1)
    with pytest.raises(ValueError):
        api.MarginalPredict(res)
    with pytest.raises(TypeError):
        api.MarginalPrediction(estimate=np.zeros(1))


# ------------------------------------------------------------------------------------------ Fit
def test_fit_plumbing_with_the_device_call_stubbed(monkeypatch):
    y = np.zeros(5)
    Xt = _capi.XInput(np.zeros((5, 3)), False)
    Pn = np.ones((2, 3))
    assert api._fit_requests(y, 2).marginal_predict is None
    assert api._fit_requests(y, 2, predict_X=Pn, marginal_predict=True).marginal_predict == 2000
    r = api._fit_requests(y, 2, X_new=Xt, nsamp=10, x_transform=False, predict_X=Pn, predict_y=[1.0, 2.0], marginal_predict=True, marginal_predict_draws=7,
                          predict_interval=90)
    assert r.marginal_predict == 7 and r.predict[0].n == 2 and np.array_equal(r.predict[1], [1.0, 2.0]) and r.predict[2] == 90
    with pytest.raises(ValueError, match="predict_X"):
        api._fit_requests(y, 2, marginal_predict=True)
    for bad in (0, 1.5, -3, True):
        with pytest.raises(ValueError):
            api._fit_requests(y, 2, predict_X=Pn, marginal_predict=True, marginal_predict_draws=bad)
    with pytest.raises(ValueError):
        api._fit_requests(y, 2, predict_X=Pn, marginal_predict=True, predict_interval=100)
    with pytest.raises(ValueError, match="2048"):
        api._fit_requests(np.zeros(2049), 2, X_new=_capi.XInput(np.zeros((2049, 3))), nsamp=10, x_transform=False, predict_X=Pn, marginal_predict=True)
    for fn in (bnr_amd.Fit, bnr_amd.generate_samples, bnr_amd.generate_samples_dbl):
        par = inspect.signature(fn).parameters
        assert par["marginal_predict"].default is False and par["marginal_predict_draws"].default == 2000, fn
    assert "pred_seed" not in inspect.signature(bnr_amd.device_marginal_predict).parameters
    monkeypatch.setattr(api, "_rank_world", lambda: (0, 2))                         # chains spread over two ranks: refused before any sampling
    with pytest.raises(ValueError, match="marginal_predict"):
        api._fit_requests(y, 2, predict_X=Pn, marginal_predict=True)
    with pytest.raises(ValueError, match="marginal_predict"):
        bnr_amd.Fit(np.zeros((5, 3)), y, 2, x_transform=False, predict_X=Pn, marginal_predict=True, filename=None)
    monkeypatch.undo()

    calls = []

    def stub(chains, nburn, nsamp, X_new, y_new=None, thin=1, weights=None, interval=95, per_draw=False, x_transform=False):
        calls.append((list(chains), nburn, nsamp, X_new, y_new, thin, weights, interval, per_draw))
        return {"stub": len(calls)}

    monkeypatch.setattr(api, "device_marginal_predict", stub)
    monkeypatch.setattr(api, "device_predict", lambda ch, nb, ns, rows, yn, interval: "plain")
    monkeypatch.setattr(api, "device_predict_pooled", lambda chains, nb, ns, rows, yn, interval, seed, predict_observation=False: "pooled")
    monkeypatch.setattr(api, "device_predict_stacked", lambda chains, w, nb, ns, rows, yn, interval, seed, predict_observation=False: "stacked")
    stack = types.SimpleNamespace(weights=np.array([0.25, 0.75]), summary=None, prediction=None, edge_cov=None, marginal_edges=None)
    monkeypatch.setattr(api, "device_stack_chains", lambda chains, nb, ns, r_eff: stack)
    c1, c2 = types.SimpleNamespace(name=1), types.SimpleNamespace(name=2)
    cs = types.SimpleNamespace(chains={1: c1, 2: c2}, ids=[1, 2])
    base = dict(return_state=False, X_new=Xt, nsamp=45, x_transform=False, predict_X=Pn, predict_y=[1.0, 2.0])
    new = lambda: api.Results(None, np.zeros(1), np.zeros(1), 30, 45)
    res = api._finish(cs, new(), api._fit_requests(y, 2, marginal_predict=True, marginal_predict_draws=20, **base), 1)
    got = calls[-1]
    assert res.marginal_prediction == {"stub": 1} and got[0] == [c1] and got[1:3] == (30, 45) and got[3].n == 2 and np.array_equal(got[4], [1.0, 2.0])
    assert got[5:] == (3, None, 95, False) and res.stat_chains == 1 and res.stacking is None and res.prediction == "plain"
    res = api._finish(cs, new(), api._fit_requests(y, 2, marginal_predict=True, pool_chains=True, predict_interval=90, **base), 1)
    assert res.marginal_prediction == {"stub": 2} and calls[-1][0] == [c1, c2] and calls[-1][5:] == (1, None, 90, False) and res.stat_chains == 2
    assert api.MarginalPredict(res) is res.marginal_prediction
    res = api._finish(cs, new(), api._fit_requests(y, 2, marginal_predict=True, stack_chains=True, **base), 1)
    assert len(calls) == 4 and calls[-2][0] == [c1, c2] and calls[-2][6] is stack.weights and calls[-1][0] == [c1] and calls[-1][6] is None
    assert res.stacking.marginal_prediction == {"stub": 3} and res.marginal_prediction == {"stub": 4}
    # without the flag: no call, no attribute on the stacking record, and the Results field for field what it was
    stack2 = types.SimpleNamespace(weights=np.array([0.25, 0.75]), summary=None, prediction=None, edge_cov=None, marginal_edges=None)
    monkeypatch.setattr(api, "device_stack_chains", lambda chains, nb, ns, r_eff: stack2)
    plain = api._finish(cs, new(), api._fit_requests(y, 2, stack_chains=True, **base), 1)
    assert len(calls) == 4 and plain.marginal_prediction is None and not hasattr(stack2, "marginal_prediction")
    with_flag = api._finish(cs, new(), api._fit_requests(y, 2, stack_chains=True, marginal_predict=True, **base), 1)
    for f in api.Results.__dataclass_fields__:
        if f != "marginal_prediction":
            a, b = getattr(plain, f), getattr(with_flag, f)
            assert (a is b) or np.array_equal(a, b), f
    bare = api._finish(cs, new(), api._fit_requests(y, 2, return_state=False), 1)
    assert bare == api.Results(None, bare.rhatxi, bare.rhatgamma, 30, 45) and bare.marginal_prediction is None


def test_marginal_predict_accessor_falls_back_to_the_state_table():
    V, R, n, m = 2, 2, 6, 4
    q = V * (V + 1) // 2
    rng = np.random.default_rng(186)
    X, y, Xn, yn = rng.normal(size=(n, q)), rng.normal(size=n), rng.normal(size=(m, q)), rng.normal(size=m)
    t = _capi.new_table(3, V, R, dead=False)
    t["u"][:] = rng.normal(size=(3, R, V)) * 0.7
    t["lam"][:, :, 0] = rng.integers(-1, 2, size=(3, R))
    t["tau2"][:, 0, 0] = rng.exponential(size=3) + 0.05
    t["mu"][:, 0, 0] = rng.normal(size=3)
    t["S"][:, :, 0] = rng.exponential(size=(3, q))
    res = api.Results(t, np.zeros(1), np.zeros(1), 1, 2)
    got = api.MarginalPredict(res, X, y, Xn, yn, x_transform=False)
    t2, mu, S, W = api._host_marginal_draws([t], 1, 2, 1)
    mean, var, nb = api._host_predict_terms(X, y, Xn, t2, mu, S, W)
    s = api._host_mixture_summary(mean, var, 1)
    o = api._host_mixture_summary(mean, var + t2[:, None], 1)
    sc = api._host_mixture_score(mean, var + t2[:, None], yn, 1)
    assert isinstance(got, api.MarginalPrediction) and got.draws == 2 and got.thin == 1 and got.n_bad == 0 and got.chains == 1 and got.weights is None
    assert np.array_equal(got.estimate, s["mean"]) and np.array_equal(got.lower_bound, s["lower"]) and np.array_equal(got.upper_bound, s["upper"])
    assert np.array_equal(got.sd, s["sd"]) and np.array_equal(got.var_within, s["var_within"]) and np.array_equal(got.pred_sd, o["sd"])
    assert np.array_equal(got.pred_lower_bound, o["lower"]) and np.array_equal(got.pred_upper_bound, o["upper"])
    assert np.array_equal(got.lpd, sc["lpd"]) and np.array_equal(got.pit, sc["pit"]) and got.elpd == float(np.sum(sc["lpd"]))
    assert np.all(got.pred_sd > got.sd) and np.all(got.rb_share > 0) and np.all(got.rb_share <= 1 + 1e-12) and got.mean is None
    assert "MarginalPrediction(rows=4" in repr(got)
    none = api.MarginalPredict(res, X, y, Xn, x_transform=False)
    assert none.lpd is None and none.pit is None and none.elpd is None and np.array_equal(none.estimate, got.estimate)
