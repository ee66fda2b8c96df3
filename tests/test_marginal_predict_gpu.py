"""GPU tests of the Rao-Blackwellised prediction of new rows (include/bnr_mpred.h, libbnr_mpred.so; kernels in csrc/bnr_mpred_kernels.h): the raw
call against the mpmath reference within the derived bound (tests/mpred_ref.py) at the edges of the 16-row MFMA tile, of the 32-row padding, of
the K step and of k_mpred_proj's 128-row block; against the numpy restatement beyond, through n = 258, 300 and 513 (the second and third
256-column pass of k_mloo_factor, whose M the projection reads); cases whose answer is exact; large neighbouring entries of L
behind the triangle's mask; the independence of a draw's bits from its batch, the blocking of the new rows, its neighbours and its place; bad
draws; bnr_mixture_score against mpmath and its host mirror; live chains through the chain form and Fit; and all four libraries in one process.

Choices the issue leaves open, and why:
  - the tile edges are met by eleven cases that pair the four lists (every n, q, m and draw count at least once; checked), not by their product.
  - the X = X* = I case uses S_e = 2^k - 1 with EVEN k: L_ee = 2^(k / 2) is then a float64, so t_j = S^2 2^-k and d_j - t_j = 1 - 2^-k exactly.
  - lpd against mpmath: every l_s is six rounded operations on quantities of size at most |log 2 pi vobs| / 2 + (y - mean)^2 / (2 vobs) + 1,
    the difference l_s - mx one more of size |l_s - mx|, exp and log are good to an ulp, the nd + K + 4 sums and products of positive terms
    move the sum by that many u relatively, and the last sum by u |lpd|:
        tol = 6 u max_s (|log 2 pi vobs_s| / 2 + (y - mean_s)^2 / (2 vobs_s) + 1) + u (max_s |l_s - mx| + nd + K + 8) + 2 u |log sum| + u |lpd|
    gated at twice that, like every bound here.
  - pit: the order of the sums is the host mirror's, erfc is not: the allowance of tests/test_marginal_edges_gpu.py for p_pos -- (nd + K + 4) u of
    the statistic for the sums plus (a^2 + 4) u per term for each of the two erfc implementations, a^2 = (y - mean)^2 / (2 vobs).
"""
import dataclasses
import hashlib

import mpmath as mp
import numpy as np
import pytest

import bnr_amd
import mloo_ref as mr
import mpred_ref as pr
from bnr_amd import _capi, api

pytestmark = pytest.mark.gpu
U = 2.0 ** -53
PROJ_BLOCK = 128                                                         # MPRED_JB of csrc/bnr_mpred_kernels.h


def _call(c, Xn, draws, W=True, **kw):
    d = list(draws)
    return bnr_amd.marginal_predict_terms(c["X"], c["y"], Xn, c["tau2"][d], c["mu"][d], c["S"][d], c["W"][d] if W else None, **kw)


def _same(a, b, rows_a=slice(None), rows_b=slice(None), cols_a=slice(None), cols_b=slice(None)):
    return all(np.array_equal(a[k][rows_a][:, cols_a], b[k][rows_b][:, cols_b], equal_nan=True) for k in ("mean", "var"))


# ------------------------------------------------------------------------------------------ against the mpmath reference
EDGE_N = (1, 2, 15, 16, 17, 31, 32, 33)
EDGE_Q = (1, 3, 4, 5, 31, 32, 33, 45)
EDGE_M = (1, 2, 15, 16, 17, 31, 32, 33, PROJ_BLOCK - 1, PROJ_BLOCK, PROJ_BLOCK + 1)
EDGE_D = (1, 2, 5, 17)
# every entry of every list at least once; the large draw counts ride on the shapes whose reference is cheap
EDGE_CASES = [(1, 5, 1, 17), (2, 31, 2, 17), (15, 32, 15, 5), (16, 33, 16, 2), (17, 45, 17, 1), (31, 1, 31, 5), (32, 3, 32, 17), (33, 4, 33, 2),
              (2, 4, PROJ_BLOCK - 1, 2), (17, 3, PROJ_BLOCK, 1), (33, 5, PROJ_BLOCK + 1, 2)]


def test_the_edge_cases_meet_every_edge():
    n, q, m, d = (set(x) for x in zip(*EDGE_CASES))
    assert n == set(EDGE_N) and q == set(EDGE_Q) and m == set(EDGE_M) and d == set(EDGE_D), EDGE_CASES


@pytest.mark.parametrize("n,q,m,ndraws", EDGE_CASES)
def test_raw_call_meets_the_bound_of_the_reference(gpu, n, q, m, ndraws):
    c = mr.case(n, q)
    r = _call(c, pr.new_rows(q)[:m], range(ndraws))
    assert r["n_bad"] == 0 and r["mean"].shape == r["var"].shape == (ndraws, m) and np.all(r["var"] >= 0)
    worst, bl = pr.worst_ratios(r["mean"], r["var"], n, q, range(ndraws), m)
    print("n=%d q=%d m=%d D=%d: error / bound %s, beta lam %.2e" % (n, q, m, ndraws, {k: "%.3g" % v for k, v in worst.items()}, bl))
    assert bl <= 0.1
    assert max(worst.values()) <= 2.0, worst


def test_raw_call_meets_the_bound_on_a_binary_matrix(gpu):
    for n, q, m in ((17, 45, 17), (33, 31, 33)):
        c = mr.case(n, q, True)
        r = _call(c, pr.new_rows(q, True)[:m], range(3))
        worst, bl = pr.worst_ratios(r["mean"], r["var"], n, q, range(3), m, True)
        print("binary n=%d q=%d m=%d: error / bound %s" % (n, q, m, worst))
        assert r["n_bad"] == 0 and bl <= 0.1 and max(worst.values()) <= 2.0, worst


@pytest.mark.parametrize("n", (17, 33))
def test_large_entries_of_l_behind_the_mask(gpu, n):
    """every S at scale 1e3: the slots M[r][i], i > r, hold entries of L of size ~ 1e2, a thousand times those of L^-1 -- a missing mask cannot
    stay within the bound; n = 17 and 33 also leave rows n .. np - 1 of the draw's matrix unwritten"""
    q, m = 45, 17
    c = mr.case(n, q)
    Xn = pr.new_rows(q)[:m]
    S = np.abs(c["S"][:3]) / np.array(mr.S_SCALES)[:, None] * 1e3
    r = bnr_amd.marginal_predict_terms(c["X"], c["y"], Xn, c["tau2"][:3], c["mu"][:3], S, c["W"][:3])
    assert r["n_bad"] == 0
    for d in range(3):
        ref = pr.reference(c["X"], c["y"], Xn, c["tau2"][d], c["mu"][d], S[d], c["W"][d])
        assert ref["beta_lam"] <= 0.1
        for name in ("mean", "var"):
            ratio = pr.ratio(r[name][d], ref[name], ref["tol_" + name])
            assert np.all(ratio <= 2.0), (name, d, float(ratio.max()))


# ------------------------------------------------------------------------------------------ against the numpy restatement
# (258, 300, 513: the M that k_mpred_proj reads comes out of the second and third 256-column pass of k_mloo_factor; 258 is the first n at which a
# later pass has a column behind its first, 300 fills full unrolled chunks of the second pass, 513 opens the third -- tests/test_marginal_loo_gpu.py)
@pytest.mark.parametrize("n", (64, 65, 129, 257, 258, 300, 513))
def test_raw_call_against_the_restatement(gpu, n):
    q, m = 300, 70
    c = mr.case(n, q)
    Xn = pr.new_rows(q)[:m]
    r = _call(c, Xn, range(3))
    hm, hv, hb = api._host_predict_terms(c["X"], c["y"], Xn, c["tau2"][:3], c["mu"][:3], c["S"][:3], c["W"][:3])
    assert r["n_bad"] == 0 and hb == 0
    worst = 0.0
    for d in range(3):
        b = pr.numpy_bounds(c["X"], c["y"], Xn, c["tau2"][d], c["mu"][d], c["S"][d], c["W"][d])
        assert b["beta_lam"] <= 0.1
        for name, h in (("mean", hm), ("var", hv)):
            ratio = pr.ratio(r[name][d], h[d], b["tol_" + name])
            assert np.all(ratio <= 4.0), (name, d, float(ratio.max()))                              # each within its own gate of 2
            worst = max(worst, float(ratio.max()))
    print("n=%d q=%d m=%d: worst difference / bound %.3g" % (n, q, m, worst))


# ------------------------------------------------------------------------------------------ exact cases
@pytest.mark.parametrize("n,q,m", ((1, 1, 1), (17, 5, 33), (33, 45, 17), (65, 130, 129)))
def test_exact_cases(gpu, n, q, m):
    c = mr.case(n, q)
    D = 5
    Xn = pr.new_rows(q)[:m]
    y, t2, mu, S, W = c["y"], c["tau2"][:D], c["mu"][:D], c["S"][:D], c["W"][:D]
    r = bnr_amd.marginal_predict_terms(c["X"], y, np.zeros((m, q)), t2, mu, S, W)                   # X* = 0
    assert r["n_bad"] == 0 and np.array_equal(r["mean"], np.repeat(mu[:, None], m, axis=1)) and np.array_equal(r["var"], np.zeros((D, m)))
    a = np.zeros((D, m))
    for e in range(q):                                                                             # a_j: e ascending from 0.0, every product and sum rounded
        a = a + Xn[:, e][None, :] * W[:, e][:, None]
    r = bnr_amd.marginal_predict_terms(c["X"], y, Xn, t2, mu, np.zeros((D, q)), W)                  # S = 0
    assert r["n_bad"] == 0 and np.array_equal(r["mean"], mu[:, None] + a) and np.array_equal(r["var"], np.zeros((D, m)))
    r = bnr_amd.marginal_predict_terms(c["X"], y, Xn, t2, mu, np.zeros((D, q)), None)               # no W: a = 0.0
    assert np.array_equal(r["mean"], np.repeat(mu[:, None], m, axis=1))
    rng = np.random.default_rng([9, n])                                                             # X = X* = I_n, S_e = 2^k - 1 with even k
    k = 2 * rng.integers(0, 6, size=(D, n))
    r = bnr_amd.marginal_predict_terms(np.eye(n), y, np.eye(n), t2, mu, 2.0 ** k - 1.0, None)
    assert r["n_bad"] == 0 and np.array_equal(r["var"], t2[:, None] * (1.0 - 2.0 ** -k))


# ------------------------------------------------------------------------------------------ independence
@pytest.fixture
def options():
    yield _capi.mpred_set_option
    _capi.mpred_set_option("mpred_batch_draws", 0)
    _capi.mpred_set_option("mpred_block_rows", 0)


@pytest.mark.parametrize("n,q,m", ((17, 45, 33), (33, 17, 17), (70, 140, 129)))
def test_a_result_does_not_depend_on_batch_block_neighbours_or_place(gpu, options, n, q, m):
    c = mr.case(n, q)
    Xn = pr.new_rows(q)[:m]
    full = _call(c, Xn, range(17))
    for b in (1, 3):
        options("mpred_batch_draws", b)
        assert _same(full, _call(c, Xn, range(17))), b
    options("mpred_batch_draws", 0)
    for rows in (1, 3):
        options("mpred_block_rows", rows)
        assert _same(full, _call(c, Xn, range(17))), rows
    options("mpred_batch_draws", 3)                                                                 # both at once
    assert _same(full, _call(c, Xn, range(17)))
    options("mpred_batch_draws", 0)
    options("mpred_block_rows", 0)
    for d in (0, 5, 16):
        assert _same(full, _call(c, Xn, [d]), slice(d, d + 1)), d                                   # a draw alone and among 17
    for j in (0, m // 2, m - 1):
        assert _same(full, _call(c, Xn[j:j + 1], range(17)), cols_a=slice(j, j + 1)), j             # a new row alone and among m
    order = [16] + list(range(1, 16)) + [0]                                                         # first and last draw swapped
    swapped = _call(c, Xn, order)
    assert _same(full, swapped, slice(16, 17), slice(0, 1)) and _same(full, swapped, slice(0, 1), slice(16, 17))
    rev = _call(c, Xn[::-1], range(17))                                                             # the new rows in reverse order
    assert np.array_equal(full["mean"], rev["mean"][:, ::-1]) and np.array_equal(full["var"], rev["var"][:, ::-1])
    assert _same(full, _call(c, Xn, range(17)))                                                     # two identical calls


# ------------------------------------------------------------------------------------------ bad draws
def test_bad_draws_are_nan_counted_and_alone(gpu):
    n, q, m = 33, 45, 17
    c = mr.case(n, q)
    Xn = pr.new_rows(q)[:m]
    good = _call(c, Xn, range(17))
    S = c["S"].copy()
    S[2, 7] = np.nan
    S[9, :] = -1e6
    r = bnr_amd.marginal_predict_terms(c["X"], c["y"], Xn, c["tau2"], c["mu"], S, c["W"])           # status OK: ordinary data
    assert r["n_bad"] == 2 and np.isnan(r["mean"][[2, 9]]).all() and np.isnan(r["var"][[2, 9]]).all()
    rest = [d for d in range(17) if d not in (2, 9)]
    assert _same(good, r, rest, rest)
    s = bnr_amd.mixture_score(r["mean"], r["var"] + c["tau2"][:, None], np.zeros(m))
    assert np.isnan(s["lpd"]).all() and np.isnan(s["pit"]).all()                                    # every score of that call is NaN


# ------------------------------------------------------------------------------------------ the mixture score
def _mix(nd, K, m):
    rng = np.random.default_rng([187, nd, K, m])
    return rng.normal(size=(K * nd, m)) * 2.0 + rng.normal(size=m), rng.exponential(size=(K * nd, m)) + 0.01, rng.normal(size=m) * 2.0


def _check_score(mean, vobs, y, K, w, dev):
    D, m = mean.shape
    nd = D // K
    host = api._host_mixture_score(mean, vobs, y, K, w)
    wk = np.full(K, 1.0 / K) if w is None else np.asarray(w, dtype=np.float64)
    om = np.repeat(wk / nd, nd)
    with np.errstate(all="ignore"):
        a2 = np.where(vobs == 0, 0.0, 0.5 * (y[None, :] - mean) ** 2 / vobs)
        terms = np.where(vobs == 0, y[None, :] >= mean, 0.5 * api._erfc(((y[None, :] - mean) / np.sqrt(vobs)) * -0.70710678118654752440))
    allow = (nd + K + 4) * U * host["pit"] + 2 * U * np.sum(om[:, None] * (a2 + 4) * terms, axis=0)
    erfc_free = np.all(vobs == 0, axis=0)
    assert np.array_equal(dev["pit"][erfc_free], host["pit"][erfc_free])                           # no erfc involved: bit for bit
    assert np.all(np.abs(dev["pit"] - host["pit"]) <= allow), float(np.max(np.abs(dev["pit"] - host["pit"]) / (allow + 1e-300)))
    with mp.workdps(50):
        for j in range(m):
            on = (om > 0) & (vobs[:, j] > 0)                                                       # (a point mass elsewhere adds nothing)
            size = 0.5 * np.abs(np.log(2 * np.pi * vobs[on, j])) + a2[on, j] + 1.0
            l = -0.5 * np.log(2 * np.pi * vobs[on, j]) - a2[on, j]
            tot = mp.mpf(0)
            for s in np.flatnonzero(on):
                v, dl = mp.mpf(float(vobs[s, j])), mp.mpf(float(y[j])) - mp.mpf(float(mean[s, j]))
                tot += mp.mpf(float(om[s])) * mp.exp(-(mp.log(2 * mp.pi) + mp.log(v)) / 2 - dl * dl / v / 2)
            ref = mp.log(tot)
            mx = float(l.max())
            tol = 6 * U * float(size.max()) + U * (float(np.max(np.abs(l - mx))) + nd + K + 8) + 2 * U * abs(float(ref) - mx) + U * abs(float(ref))
            assert abs(mp.mpf(float(dev["lpd"][j])) - ref) <= 2.0 * tol, (j, float(abs(mp.mpf(float(dev["lpd"][j])) - ref) / tol))
            assert abs(dev["lpd"][j] - host["lpd"][j]) <= 4.0 * tol


@pytest.mark.parametrize("K", (1, 3))
@pytest.mark.parametrize("nd", (1, 2, 63, 64, 65, 257))
def test_mixture_score(gpu, nd, K):
    mean, vobs, y = _mix(nd, K, 5)
    for w in (None, np.array([1.0]) if K == 1 else np.array([0.2, 0.5, 0.3])):
        _check_score(mean, vobs, y, K, w, bnr_amd.mixture_score(mean, vobs, y, K, w))
    if K == 3:                                                                                      # w = e_k picks chain k
        one = bnr_amd.mixture_score(mean, vobs, y, 3, [0.0, 1.0, 0.0])
        own = bnr_amd.mixture_score(mean[nd:2 * nd], vobs[nd:2 * nd], y, 1)
        assert np.array_equal(one["lpd"], own["lpd"]) and np.array_equal(one["pit"], own["pit"])


def test_mixture_score_point_masses_nan_and_tails(gpu):
    mean, vobs, y = _mix(65, 3, 6)
    mean, vobs, y = mean.copy(), vobs.copy(), y.copy()
    vobs[:, 1] = 0.0                                                                                # only point masses, y on none of them
    vobs[:, 2] = 0.0
    y[2] = mean[100, 2]                                                                             # ... y on one of them
    vobs[::3, 3] = 0.0                                                                              # some point masses among normals
    dev = bnr_amd.mixture_score(mean, vobs, y, 3)
    host = api._host_mixture_score(mean, vobs, y, 3)
    assert dev["lpd"][1] == -np.inf and dev["lpd"][2] == np.inf and np.array_equal(dev["pit"][[1, 2]], host["pit"][[1, 2]])
    assert abs(dev["pit"][1] - np.mean(y[1] >= mean[:, 1])) <= 1e-15
    keep = [0, 3, 4, 5]
    _check_score(mean[:, keep], vobs[:, keep], y[keep], 3, None, {k: dev[k][keep] for k in dev})
    w0 = bnr_amd.mixture_score(mean, vobs, y, 3, [0.5, 0.0, 0.5])                                   # mean[100, 2] sits in chain 1, whose weight is 0
    assert w0["lpd"][2] == -np.inf and np.array_equal(w0["pit"][[1, 2]], api._host_mixture_score(mean, vobs, y, 3, [0.5, 0.0, 0.5])["pit"][[1, 2]])
    bad, vbad, ybad = mean.copy(), vobs.copy(), y.copy()
    bad[100, 0] = np.nan
    vbad[7, 3] = np.nan
    vbad[8, 4] = -1.0
    ybad[5] = np.nan
    nan = bnr_amd.mixture_score(bad, vbad, ybad, 3)
    for k in ("lpd", "pit"):
        assert np.isnan(nan[k][[0, 3, 4, 5]]).all() and np.array_equal(nan[k][[1, 2]], dev[k][[1, 2]]), k
    nan0 = bnr_amd.mixture_score(bad, vobs, y, 3, [0.5, 0.0, 0.5])                                  # a NaN in a chain of weight 0 still makes the row NaN
    assert np.isnan(nan0["lpd"][0]) and np.isnan(nan0["pit"][0]) and np.isfinite(nan0["lpd"][[3, 4, 5]]).all()
    tail = bnr_amd.mixture_score(np.full((3, 1), 30.0), np.ones((3, 1)), [0.0])
    with mp.workdps(50):
        ref = mp.erfc(mp.mpf(30) / mp.sqrt(2)) / 2
        assert abs(mp.mpf(float(tail["pit"][0])) - ref) <= mp.mpf("1e-12") * ref
    assert abs(tail["lpd"][0] - (-0.5 * np.log(2 * np.pi) - 450.0)) <= 16 * U * 451


# ------------------------------------------------------------------------------------------ live chains
TOT = 60
M_NEW = 9


@pytest.fixture(scope="module")
def fit(gpu):
    X, y, _ = bnr_amd.make_synthetic(20, 6, 2, seed=7)
    Xn, yn, _ = bnr_amd.make_synthetic(M_NEW, 6, 2, seed=8)
    chains = [bnr_amd.Chain(X, y, 2, TOT, 11, 1)]
    chains += [bnr_amd.Chain.like(chains[0], 11, k, TOT) for k in (2, 3)]
    for ch in chains:
        ch.init_prior()
        ch.run(2, TOT, TOT)
    tables = [ch.fetch() for ch in chains]
    yield (np.asarray(X, dtype=np.float64), np.asarray(y, dtype=np.float64), chains, tables, np.asarray(Xn, dtype=np.float64),
           np.asarray(yn, dtype=np.float64).reshape(-1))
    for ch in chains:
        ch.close()


FIELDS = _capi.MPRED_SUMMARY_FIELDS


def _summaries_of(mean, var, t2, yn, K, w=None):
    """the ten outputs of the chain form from bnr_mixture_summary / bnr_mixture_score of the per-draw matrices"""
    vobs = var + t2[:, None]
    e = dict(zip(_capi.MEDGE_SUMMARY_FIELDS, _capi.mixture_summary_raw(mean, var, K, w, fields=("mean", "sd", "var_within", "lower", "upper"))))
    o = dict(zip(_capi.MEDGE_SUMMARY_FIELDS, _capi.mixture_summary_raw(mean, vobs, K, w, fields=("sd", "lower", "upper"))))
    lpd, pit = _capi.mixture_score_raw(mean, vobs, yn, K, w)
    return (e["mean"], e["sd"], e["var_within"], e["lower"], e["upper"], o["sd"], o["lower"], o["upper"], lpd, pit)


@pytest.mark.parametrize("thin", (1, 3))
@pytest.mark.parametrize("nburn,nsamp", ((5, 40), (8, 41)))
def test_live_chains(fit, nburn, nsamp, thin):
    X, y, chains, tables, Xn, yn = fit
    nd = -(-nsamp // thin)
    D = 3 * nd
    before = [(ch.iter, ch.counters()) for ch in chains]
    out, dm, dv, nb = _capi.chains_marginal_predict(chains, nburn + 1, nsamp, Xn, yn, thin, per_draw=True)
    assert nb == 0 and dm.shape == dv.shape == (D, M_NEW) and np.all(dv > 0)
    t2, mu, S, W = api._host_marginal_draws(tables, nburn, nsamp, thin)
    raw = bnr_amd.marginal_predict_terms(X, y, Xn, t2, mu, S, W)
    assert np.array_equal(raw["mean"], dm) and np.array_equal(raw["var"], dv)                       # the chain form = the raw call on the same draws
    hm, hv, hb = api._host_predict_terms(X, y, Xn, t2, mu, S, W)
    for d in range(0, D, 7):
        b = pr.numpy_bounds(X, y, Xn, t2[d], mu[d], S[d], W[d])
        assert b["beta_lam"] <= 0.1 and np.all(pr.ratio(dm[d], hm[d], b["tol_mean"]) <= 4.0) and np.all(pr.ratio(dv[d], hv[d], b["tol_var"]) <= 4.0), d
    for k, a, b in zip(FIELDS, out, _summaries_of(dm, dv, t2, yn, 3)):
        assert np.array_equal(a, b), k                                                              # the summaries = those of the matrices, bit for bit
    nodraws = _capi.chains_marginal_predict(chains, nburn + 1, nsamp, Xn, yn, thin)
    assert nodraws[1] is None and all(np.array_equal(a, b) for a, b in zip(out, nodraws[0]))
    noy = _capi.chains_marginal_predict(chains, nburn + 1, nsamp, Xn, None, thin)
    assert noy[0][8] is None and noy[0][9] is None and all(np.array_equal(a, b) for a, b in zip(out[:8], noy[0][:8]))
    mp_ = api.device_marginal_predict(chains, nburn, nsamp, Xn, yn, thin, interval=95)
    assert np.array_equal(mp_.estimate, out[0]) and np.array_equal(mp_.upper_bound, out[4]) and np.array_equal(mp_.pred_sd, out[5])
    assert np.array_equal(mp_.lpd, out[8]) and mp_.elpd == float(np.sum(out[8])) and mp_.draws == D and mp_.thin == thin and mp_.chains == 3
    assert np.all(mp_.lower_bound < mp_.estimate) and np.all(mp_.estimate < mp_.upper_bound) and np.all((mp_.rb_share > 0) & (mp_.rb_share <= 1))
    assert np.all(mp_.pred_lower_bound < mp_.lower_bound) and np.all(mp_.upper_bound < mp_.pred_upper_bound) and np.all(mp_.pred_sd > mp_.sd)
    assert np.all((mp_.pit > 0) & (mp_.pit < 1)) and np.all(np.isfinite(mp_.lpd))
    for k, ch in enumerate(chains):                                                                 # per-chain calls against the pooled call with w = e_k
        w = np.zeros(3)
        w[k] = 1.0
        one = _capi.chains_marginal_predict([ch], nburn + 1, nsamp, Xn, yn, thin, per_draw=True)
        pick = _capi.chains_marginal_predict(chains, nburn + 1, nsamp, Xn, yn, thin, weights=w)
        assert np.array_equal(one[1], dm[k * nd:(k + 1) * nd]) and np.array_equal(one[2], dv[k * nd:(k + 1) * nd])
        for f, a, b in zip(FIELDS, one[0], pick[0]):
            if f not in ("lower", "upper", "pred_lower", "pred_upper"):                             # (the pooled bracket covers every chain)
                assert np.array_equal(a, b), (k, f)
        for f, a, b in zip(FIELDS, pick[0], _summaries_of(dm, dv, t2, yn, 3, w)):
            assert np.array_equal(a, b), (k, f)
    assert [(ch.iter, ch.counters()) for ch in chains] == before                                    # nothing of any chain is written
    for ch, t in zip(chains, tables):
        now = ch.fetch()
        assert all(np.array_equal(now[k], t[k], equal_nan=True) for k in t)


def test_chain_call_refusals(fit):
    _X, _y, chains, _tables, Xn, yn = fit
    for args in ((0, 10), (1, TOT + 1), (TOT, 2)):
        with pytest.raises(bnr_amd.BnrError) as e:
            _capi.chains_marginal_predict(chains, *args, Xn)
        assert e.value.code == 1 and "window" in str(e.value)
    with pytest.raises(bnr_amd.BnrError) as e:
        _capi.chains_marginal_predict([chains[0], chains[0]], 1, 10, Xn)
    assert "twice" in str(e.value)
    with pytest.raises(bnr_amd.BnrError) as e:
        _capi.chains_marginal_predict(chains, 1, 10, Xn, weights=[0.5, 0.5, 0.5])
    assert "sum to 1" in str(e.value)
    for bad in (dict(thin=0), dict(y_new=np.zeros(M_NEW + 1)), dict(fields=("lpd",))):
        with pytest.raises(ValueError):
            _capi.chains_marginal_predict(chains, 1, 10, Xn, **bad)
    with pytest.raises(ValueError):
        _capi.chains_marginal_predict(chains, 1, 10, Xn[:, :5])


def _digest(rec, names):
    h = hashlib.sha256()
    for k in names:
        h.update(np.ascontiguousarray(rec[k] if isinstance(rec, dict) else getattr(rec, k)).tobytes())
    return h.hexdigest()


def test_all_four_libraries_in_one_process(fit):
    _X, _y, chains, _tables, Xn, yn = fit
    edge_fields = ("estimate", "sd", "lower_bound", "upper_bound", "p_pos", "p_neg", "var_within")
    loo_a = api.device_marginal_loo(chains, 5, 40, 3)
    me_a = api.device_marginal_edges(chains, 5, 40, 3)
    p1 = api.device_marginal_predict(chains, 5, 40, Xn, yn, 3)
    loo_b = api.device_marginal_loo(chains, 5, 40, 3)
    me_b = api.device_marginal_edges(chains, 5, 40, 3)
    p2 = api.device_marginal_predict(chains, 5, 40, Xn, yn, 3)
    assert _capi._mloo is not None and _capi._medge is not None and _capi._mpred is not None
    assert set(loo_a) == set(loo_b) and all(np.array_equal(loo_a[k], loo_b[k], equal_nan=True) for k in loo_a)
    assert _digest(me_a, edge_fields) == _digest(me_b, edge_fields)
    pf = ("estimate", "sd", "lower_bound", "upper_bound", "var_within", "pred_sd", "pred_lower_bound", "pred_upper_bound", "lpd", "pit")
    assert _digest(p1, pf) == _digest(p2, pf)


def test_fit_with_the_flag_adds_the_result_and_changes_nothing_else(gpu, tmp_path):
    X, y, _ = bnr_amd.make_synthetic(20, 6, 2, seed=7)
    Xn, yn, _ = bnr_amd.make_synthetic(M_NEW, 6, 2, seed=8)
    kw = dict(nburn=30, nsamples=40, num_chains=2, seed=5, x_transform=False, suppress_timer=True, filename=str(tmp_path / "p.log"), loo=True,
              summary_interval=95, stack_chains=True, predict_X=Xn, predict_y=yn)
    a = bnr_amd.Fit(X, y, 2, **kw)
    b = bnr_amd.Fit(X, y, 2, marginal_predict=True, marginal_predict_draws=15, **kw)
    assert a.marginal_prediction is None and not hasattr(a.stacking, "marginal_prediction")
    for f in ("rhatxi", "rhatgamma", "burn_in", "sampled", "stat_chains"):
        assert np.array_equal(getattr(a, f), getattr(b, f)), f
    for f in ("loo", "summary_device"):
        assert set(getattr(a, f)) == set(getattr(b, f)) and all(np.array_equal(getattr(a, f)[k], getattr(b, f)[k], equal_nan=True) for k in getattr(a, f)), f
    assert all(np.array_equal(a.state[k], b.state[k], equal_nan=True) for k in a.state)
    for f in dataclasses.fields(a.prediction):
        va, vb = getattr(a.prediction, f.name), getattr(b.prediction, f.name)
        assert (va is None and vb is None) or np.array_equal(va, vb, equal_nan=True), f.name
    assert np.array_equal(a.stacking.weights, b.stacking.weights) and np.array_equal(a.stacking.elpd_chain, b.stacking.elpd_chain)
    assert all(np.array_equal(a.stacking.summary[k], b.stacking.summary[k], equal_nan=True) for k in a.stacking.summary)
    assert np.array_equal(a.stacking.prediction.estimate, b.stacking.prediction.estimate)
    seen = {"rhatxi", "rhatgamma", "burn_in", "sampled", "stat_chains", "loo", "summary_device", "state", "stacking", "prediction", "marginal_prediction"}
    for f in dataclasses.fields(a):                                                                 # every other field: not requested, None in both
        assert f.name in seen or (getattr(a, f.name) is None and getattr(b, f.name) is None), f.name
    mp_ = bnr_amd.MarginalPredict(b)
    assert mp_ is b.marginal_prediction and mp_.thin == 3 and mp_.draws == 14 and mp_.chains == 1 and mp_.n_bad == 0 and mp_.estimate.shape == (M_NEW,)
    h = api._host_marginal_predict([b.state], np.asarray(X, dtype=np.float64), y, np.asarray(Xn, dtype=np.float64), yn, b.burn_in, b.sampled, 3)
    assert np.allclose(mp_.estimate, h.estimate, rtol=1e-9, atol=1e-12) and np.allclose(mp_.sd, h.sd, rtol=1e-9) and np.allclose(mp_.pred_sd, h.pred_sd, rtol=1e-9)
    assert np.allclose(mp_.lower_bound, h.lower_bound, rtol=1e-8, atol=1e-9) and np.allclose(mp_.pred_upper_bound, h.pred_upper_bound, rtol=1e-8, atol=1e-9)
    assert np.allclose(mp_.lpd, h.lpd, rtol=1e-9, atol=1e-12) and np.allclose(mp_.pit, h.pit, rtol=1e-9, atol=1e-12)
    st = b.stacking.marginal_prediction
    assert st.chains == 2 and st.draws == 28 and np.array_equal(st.weights, b.stacking.weights) and np.all(np.isfinite(st.estimate))
