"""GPU tests of the Rao-Blackwellised edge summaries (include/bnr_medge.h, libbnr_medge.so; kernels in csrc/bnr_medge_kernels.h): the raw call
against the mpmath reference within the derived bound (tests/medge_ref.py) at the edges of the 16-row MFMA tile, of the 32-row padding, of the
128-edge block and of the K step; against the numpy restatement beyond, up to the limit n = 2048; cases whose answer is exact; large neighbouring entries of L behind the
triangle's mask; the independence of a draw's bits from its batch, its neighbours and its place; bad draws; bnr_mixture_summary against its host
mirror and, for the quantiles, against their defining property in mpmath; live chains through the chain form and Fit; and both libraries that hold
the marginal kernels in one process.

Past 256 rows the M that k_medge_proj reads is the work of the later 256-column passes of k_mloo_factor (tests/test_marginal_loo_gpu.py has
the list): 258 the first column of the second pass with a k < i, 300 a second pass of 44 columns (also X = I at 300 rows), 513 the third pass,
521 nine columns of it, 2048 all eight passes.

Choices the issue leaves open, and why:
  - the X = I case uses S_e = 2^k - 1 with EVEN k (as the marginal LOO test does): L_ee = 2^(k / 2) is then a float64, so t_e = 2^-k exactly.
  - the driver has no debug hook to poison a work matrix, so the mask is tested by the reference at n = 17 and n = 33 with every S at scale 1e3.
  - sd is compared within 2 ulp: it is the square root of bits that equal the host's, by a square root that may round differently.
"""
import dataclasses
import hashlib
import os
import subprocess
import sys

import mpmath as mp
import numpy as np
import pytest

import bnr_amd
import medge_ref as er
import mloo_ref as mr
from bnr_amd import _capi, api

pytestmark = pytest.mark.gpu
U = 2.0 ** -53
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = _capi.MEDGE_SUMMARY_FIELDS


def _call(c, draws, W=True, **kw):
    d = list(draws)
    return bnr_amd.marginal_gamma(c["X"], c["y"], c["tau2"][d], c["mu"][d], c["S"][d], c["W"][d] if W else None, **kw)


def _same(a, b, rows_a=slice(None), rows_b=slice(None)):
    return all(np.array_equal(a[k][rows_a], b[k][rows_b], equal_nan=True) for k in ("m", "v"))


# ------------------------------------------------------------------------------------------ against the mpmath reference
@pytest.mark.parametrize("q", (1, 3, 4, 5, 31, 32, 33, 45))
@pytest.mark.parametrize("n", (1, 2, 15, 16, 17, 31, 32, 33))
def test_raw_call_meets_the_bound_of_the_reference(gpu, n, q):
    c = mr.case(n, q)
    for ndraws in (1, 2, 5, 17):
        r = _call(c, range(ndraws))
        assert r["n_bad"] == 0 and r["m"].shape == r["v"].shape == (ndraws, q) and np.all(r["v"] >= 0)
        worst, bl = er.worst_ratios(r["m"], r["v"], n, q, range(ndraws))
        print("n=%d q=%d D=%d: error / bound %s, beta lam %.2e" % (n, q, ndraws, {k: "%.3g" % v for k, v in worst.items()}, bl))
        assert bl <= 0.1
        assert max(worst.values()) <= 2.0, (ndraws, worst)


def test_raw_call_meets_the_bound_on_a_binary_matrix(gpu):
    for n, q in ((17, 45), (33, 31)):
        c = mr.case(n, q, True)
        r = _call(c, range(3))
        worst, bl = er.worst_ratios(r["m"], r["v"], n, q, range(3), True)
        print("binary n=%d q=%d: error / bound %s" % (n, q, worst))
        assert r["n_bad"] == 0 and bl <= 0.1 and max(worst.values()) <= 2.0, worst


@pytest.mark.parametrize("n", (17, 33))
def test_large_entries_of_l_behind_the_mask(gpu, n):
    """every S at scale 1e3: the slots M[r][i], i > r, hold entries of L of size ~ 1e2, a thousand times those of L^-1 -- a missing mask cannot
    stay within the bound; n = 17 and 33 also leave rows n .. np - 1 of the draw's matrix unwritten"""
    q = 45
    c = mr.case(n, q)
    S = np.abs(c["S"][:3]) / np.array(mr.S_SCALES)[:, None] * 1e3
    r = bnr_amd.marginal_gamma(c["X"], c["y"], c["tau2"][:3], c["mu"][:3], S, c["W"][:3])
    assert r["n_bad"] == 0
    for d in range(3):
        ref = er.reference(c["X"], c["y"], c["tau2"][d], c["mu"][d], S[d], c["W"][d])
        assert ref["beta_lam"] <= 0.1
        for name in ("m", "v"):
            ratio = er.ratio(r[name][d], ref[name], ref["tol_" + name])
            assert np.all(ratio <= 2.0), (name, d, float(ratio.max()))


# ------------------------------------------------------------------------------------------ against the numpy restatement
def _against_the_restatement(c, r, D):
    """m and v of a call on the first D draws of c against api._host_gamma_terms, each within its own gate of 2"""
    n, q = c["X"].shape
    hm, hv, hb = api._host_gamma_terms(c["X"], c["y"], c["tau2"][:D], c["mu"][:D], c["S"][:D], c["W"][:D])
    assert r["n_bad"] == 0 and hb == 0
    worst = 0.0
    for d in range(D):
        b = er.numpy_bounds(c["X"], c["y"], c["tau2"][d], c["mu"][d], c["S"][d], c["W"][d])
        assert b["beta_lam"] <= 0.1
        for name, h in (("m", hm), ("v", hv)):
            ratio = er.ratio(r[name][d], h[d], b["tol_" + name])
            assert np.all(ratio <= 4.0), (name, d, float(ratio.max()))                              # each within its own gate of 2
            worst = max(worst, float(ratio.max()))
    print("n=%d q=%d: worst difference / bound %.3g" % (n, q, worst))


# (258, 300, 513, 521: the M that the projection reads comes out of the second and third 256-column pass of k_mloo_factor -- module docstring)
@pytest.mark.parametrize("n,q", [(n, q) for q in (64, 65, 300) for n in (64, 65, 129, 257)] + [(258, 65), (300, 65), (513, 65), (521, 300)])
def test_raw_call_against_the_restatement(gpu, n, q):
    c = mr.case(n, q)
    _against_the_restatement(c, _call(c, range(3)), 3)


def test_the_largest_n(gpu):
    """n = 2048 = MLOO_MAX_N, q = 9, one draw: the projection over the M of all eight passes of the factor kernel, 128 row tiles (1.4 s on an
    MI355X, the restatement included)"""
    c = mr.case(2048, 9)
    _against_the_restatement(c, _call(c, range(1)), 1)


# ------------------------------------------------------------------------------------------ exact cases
@pytest.mark.parametrize("n,q", ((1, 1), (17, 5), (33, 45), (65, 130), (300, 310)))
def test_exact_cases(gpu, n, q):
    c = mr.case(n, q)
    D = 5
    y, t2, mu, S, W = c["y"], c["tau2"][:D], c["mu"][:D], c["S"][:D], c["W"][:D]
    r = bnr_amd.marginal_gamma(np.zeros((n, q)), y, t2, mu, S, W)                                   # X = 0
    assert r["n_bad"] == 0 and np.array_equal(r["m"], W) and np.array_equal(r["v"], t2[:, None] * S)
    r = bnr_amd.marginal_gamma(c["X"], y, t2, mu, np.zeros((D, q)), W)                              # S = 0
    assert r["n_bad"] == 0 and np.array_equal(r["m"], W) and np.array_equal(r["v"], np.zeros((D, q)))
    r = bnr_amd.marginal_gamma(np.zeros((n, q)), y, t2, mu, S, None)                                # no W: 0.0
    assert np.array_equal(r["m"], np.zeros((D, q)))
    rng = np.random.default_rng([8, n])                                                             # X = I_n, S_e = 2^k - 1 with even k
    k = 2 * rng.integers(0, 6, size=(D, n))
    r = bnr_amd.marginal_gamma(np.eye(n), y, t2, mu, 2.0 ** k - 1.0, None)
    assert r["n_bad"] == 0 and np.array_equal(r["v"], (t2[:, None] * (2.0 ** k - 1.0)) * 2.0 ** -k)


# ------------------------------------------------------------------------------------------ independence
@pytest.fixture
def batch_option():
    yield lambda v: _capi.medge_set_option("medge_batch_draws", v)
    _capi.medge_set_option("medge_batch_draws", 0)


@pytest.mark.parametrize("n,q", ((17, 45), (33, 17), (70, 140)))
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
    assert _same(full, _call(c, range(17)))                                                         # two identical calls
    sub = bnr_amd.marginal_gamma(c["X"][:, :q - 3], c["y"], c["tau2"], c["mu"], c["S"][:, :q - 3], None)
    assert sub["v"].shape == (17, q - 3)


# ------------------------------------------------------------------------------------------ bad draws
def test_bad_draws_are_nan_counted_and_alone(gpu):
    n, q = 33, 45
    c = mr.case(n, q)
    good = _call(c, range(17))
    S = c["S"].copy()
    S[2, 7] = np.nan
    S[9, :] = -1e6
    r = bnr_amd.marginal_gamma(c["X"], c["y"], c["tau2"], c["mu"], S, c["W"])                       # status OK: ordinary data
    assert r["n_bad"] == 2 and np.isnan(r["m"][[2, 9]]).all() and np.isnan(r["v"][[2, 9]]).all()
    rest = [d for d in range(17) if d not in (2, 9)]
    assert _same(good, r, rest, rest)
    s = bnr_amd.mixture_summary(r["m"], r["v"])
    assert all(np.isnan(s[k]).all() for k in FIELDS)                                                # every summary of that call is NaN


# ------------------------------------------------------------------------------------------ the mixture summary
def _mix(nd, K, q):
    rng = np.random.default_rng([184, nd, K, q])
    return rng.normal(size=(K * nd, q)) * 2.0 + rng.normal(size=q), rng.exponential(size=(K * nd, q)) + 0.01


def _mp_cdf(t, ms, ss, om):
    """F(t) = sum omega Phi((t - m) / sqrt v) in mpmath (20 digits), v = 0: [t >= m]; ms, ss: the components' m and sqrt(2 v) as mpf (erfc itself: half the time
    of mp.ncdf).  A component more than 12 sds away contributes its limit 0 or 1 (off by less than 1e-32)"""
    tot = mp.mpf(0)
    for m_, s_, w_ in zip(ms, ss, om):
        d = t - m_
        if s_ == 0 or abs(d) > 8.5 * s_:
            tot += 2 * w_ if d >= 0 else 0
        else:
            tot += w_ * mp.erfc(-d / s_)
    return tot / 2


def _check_summary(m, v, K, w, dev, interval=95):
    """the device's summary against the host mirror and, for the quantiles, against their defining property"""
    p_lo, p_hi = api._loo_interval_probs(interval)
    D, q = m.shape
    nd = D // K
    host = api._host_mixture_summary(m, v, K, w, p_lo, p_hi)
    assert np.array_equal(dev["mean"], host["mean"]) and np.array_equal(dev["var_within"], host["var_within"])
    assert np.all(np.abs(dev["sd"] - host["sd"]) <= 2 * np.spacing(host["sd"]))
    om = np.repeat((np.full(K, 1.0 / K) if w is None else np.asarray(w)) / nd, nd)
    # p_pos, p_neg: the order of the sums is the host's, erfc is not.  The terms are >= 0, so sum |terms| is the statistic: (nd + K + 4) u of it
    # for the sums, as the issue has it.  One term was missing there: the two erfc implementations themselves.  erfc(a) ~ exp(-a^2) / (a sqrt pi)
    # and an implementation that rounds a^2 before the exponential is off by a^2 u relatively (observed: 18 u at a^2 = 31), so each of the two
    # is allowed (a^2 + 4) u per term -- 450 u = 5e-14 at m / sqrt v = 30, inside the 1e-12 asked for there.
    with np.errstate(all="ignore"):
        r = m / np.sqrt(v)
        a2 = np.where(v == 0, 0.0, 0.5 * r * r)
        terms = dict(p_pos=np.where(v == 0, m > 0, 0.5 * api._erfc(r * -0.70710678118654752440)),
                     p_neg=np.where(v == 0, m < 0, 0.5 * api._erfc(r * 0.70710678118654752440)))
    for k in ("p_pos", "p_neg"):
        allow = (nd + K + 4) * U * host[k] + 2 * U * np.sum(om[:, None] * (a2 + 4) * terms[k], axis=0)
        assert np.all(np.abs(dev[k] - host[k]) <= allow), (k, float(np.max(np.abs(dev[k] - host[k]) / (allow + 1e-300))))
    c = api._loo_bracket_c(p_lo, p_hi)
    with mp.workdps(20):
        for e in range(q):
            sd = np.sqrt(v[:, e])
            width = float(np.max(m[:, e] + c * sd) - np.min(m[:, e] - c * sd))
            wd = width * 2.0 ** -40
            ms, ss = [mp.mpf(float(x)) for x in m[:, e]], [mp.sqrt(2 * mp.mpf(float(x))) for x in v[:, e]]
            for got, p in ((dev["lower"][e], p_lo), (dev["upper"][e], p_hi)):
                if width == 0:
                    assert got == m[0, e]
                    continue
                assert _mp_cdf(mp.mpf(float(got)) - wd, ms, ss, om) <= p <= _mp_cdf(mp.mpf(float(got)) + wd, ms, ss, om), (e, p, got)


@pytest.mark.parametrize("q", (1, 33))
@pytest.mark.parametrize("K", (1, 3))
@pytest.mark.parametrize("nd", (1, 2, 63, 64, 65, 257))
def test_mixture_summary(gpu, nd, K, q):
    m, v = _mix(nd, K, q)
    for w in (None, np.array([1.0]) if K == 1 else np.array([0.2, 0.5, 0.3])):
        dev = bnr_amd.mixture_summary(m, v, K, w)
        _check_summary(m, v, K, w, dev)
    if K == 3:                                                                                      # w = e_k picks chain k
        one = bnr_amd.mixture_summary(m, v, 3, [0.0, 1.0, 0.0])
        own = bnr_amd.mixture_summary(m[nd:2 * nd], v[nd:2 * nd], 1)
        for k in ("mean", "sd", "var_within", "p_pos", "p_neg"):
            assert np.array_equal(one[k], own[k]), k


def test_mixture_summary_point_masses_nan_and_tails(gpu):
    m, v = _mix(65, 3, 5)
    v = v.copy()
    v[::3, 1] = 0.0                                                                                 # some point masses
    v[:, 2] = 0.0                                                                                   # only point masses
    m = m.copy()
    m[:, 4] = 7.0
    v[:, 4] = 0.0                                                                                   # one point: the bracket has no width
    dev = bnr_amd.mixture_summary(m, v, 3, interval=90)
    _check_summary(m, v, 3, None, dev, 90)
    assert dev["lower"][4] == 7.0 and dev["upper"][4] == 7.0 and dev["p_pos"][4] == 1.0 and dev["p_neg"][4] == 0.0 and dev["var_within"][4] == 0.0
    assert abs(dev["p_pos"][2] - np.mean(m[:, 2] > 0)) <= 1e-15 and dev["var_within"][2] == 0.0
    bad = m.copy()
    bad[100, 3] = np.nan
    vbad = v.copy()
    vbad[7, 0] = np.nan
    nan = bnr_amd.mixture_summary(bad, vbad, 3, interval=90)
    for k in FIELDS:
        assert np.isnan(nan[k][[0, 3]]).all() and np.array_equal(nan[k][[1, 2, 4]], dev[k][[1, 2, 4]]), k
    tail = bnr_amd.mixture_summary(np.array([[30.0, -30.0]] * 3), np.ones((3, 2)))
    with mp.workdps(50):
        ref = mp.erfc(mp.mpf(30) / mp.sqrt(2)) / 2
        assert abs(mp.mpf(float(tail["p_neg"][0])) - ref) <= mp.mpf("1e-12") * ref and abs(mp.mpf(float(tail["p_pos"][1])) - ref) <= mp.mpf("1e-12") * ref
    assert tail["p_pos"][0] == 1.0 and tail["p_neg"][1] == 1.0


# ------------------------------------------------------------------------------------------ live chains
TOT = 60


@pytest.fixture(scope="module")
def fit(gpu):
    X, y, _ = bnr_amd.make_synthetic(20, 6, 2, seed=7)
    chains = [bnr_amd.Chain(X, y, 2, TOT, 11, 1)]
    chains += [bnr_amd.Chain.like(chains[0], 11, k, TOT) for k in (2, 3)]
    for ch in chains:
        ch.init_prior()
        ch.run(2, TOT, TOT)
    tables = [ch.fetch() for ch in chains]
    yield np.asarray(X, dtype=np.float64), np.asarray(y, dtype=np.float64), chains, tables
    for ch in chains:
        ch.close()


@pytest.mark.parametrize("thin", (1, 3))
@pytest.mark.parametrize("nburn,nsamp", ((5, 40), (8, 41)))
def test_live_chains(fit, nburn, nsamp, thin):
    X, y, chains, tables = fit
    q, nd = 21, -(-nsamp // thin)
    D = 3 * nd
    before = [(ch.iter, ch.counters()) for ch in chains]
    out, m, v, nb = _capi.chains_marginal_edges(chains, nburn + 1, nsamp, thin, per_draw=True)
    assert nb == 0 and m.shape == v.shape == (D, q) and np.all(v > 0)
    t2, mu, S, W = api._host_marginal_draws(tables, nburn, nsamp, thin)
    raw = bnr_amd.marginal_gamma(X, y, t2, mu, S, W)
    assert np.array_equal(raw["m"], m) and np.array_equal(raw["v"], v)                              # the chain form = the raw call on the same draws
    hm, hv, hb = api._host_marginal_gamma(tables, X, y, nburn, nsamp, thin)
    for d in range(0, D, 7):
        b = er.numpy_bounds(X, y, t2[d], mu[d], S[d], W[d])
        assert b["beta_lam"] <= 0.1 and np.all(er.ratio(m[d], hm[d], b["tol_m"]) <= 4.0) and np.all(er.ratio(v[d], hv[d], b["tol_v"]) <= 4.0), d
    s = _capi.mixture_summary_raw(m, v, 3)
    for k, a, b in zip(FIELDS, out, s):
        assert np.array_equal(a, b), k                                                              # the summaries = bnr_mixture_summary of those, bit for bit
    nodraws = _capi.chains_marginal_edges(chains, nburn + 1, nsamp, thin)
    assert nodraws[1] is None and all(np.array_equal(a, b) for a, b in zip(out, nodraws[0]))
    me = api.device_marginal_edges(chains, nburn, nsamp, thin, interval=95)
    assert np.array_equal(me.estimate, out[0]) and np.array_equal(me.lower_bound, out[5]) and me.draws == D and me.thin == thin and me.chains == 3
    assert np.all(me.lower_bound < me.estimate) and np.all(me.estimate < me.upper_bound) and np.all((me.rb_share > 0) & (me.rb_share <= 1))
    for k, ch in enumerate(chains):                                                                 # per-chain calls against the pooled call with w = e_k
        w = np.zeros(3)
        w[k] = 1.0
        one = _capi.chains_marginal_edges([ch], nburn + 1, nsamp, thin, per_draw=True)
        pick = _capi.chains_marginal_edges(chains, nburn + 1, nsamp, thin, weights=w)
        assert np.array_equal(one[1], m[k * nd:(k + 1) * nd]) and np.array_equal(one[2], v[k * nd:(k + 1) * nd])
        for f, a, b in zip(FIELDS[:5], one[0], pick[0]):
            assert np.array_equal(a, b), (k, f)
    assert [(ch.iter, ch.counters()) for ch in chains] == before                                    # nothing of any chain is written
    for ch, t in zip(chains, tables):
        now = ch.fetch()
        assert all(np.array_equal(now[k], t[k], equal_nan=True) for k in t)


def test_chain_call_refusals(fit):
    _X, _y, chains, _tables = fit
    for args in ((0, 10, 1), (1, TOT + 1, 1), (TOT, 2, 1)):
        with pytest.raises(bnr_amd.BnrError) as e:
            _capi.chains_marginal_edges(chains, *args)
        assert e.value.code == 1 and "window" in str(e.value)
    with pytest.raises(bnr_amd.BnrError) as e:
        _capi.chains_marginal_edges([chains[0], chains[0]], 1, 10, 1)
    assert "twice" in str(e.value)
    with pytest.raises(bnr_amd.BnrError) as e:
        _capi.chains_marginal_edges(chains, 1, 10, 1, weights=[0.5, 0.5, 0.5])
    assert "sum to 1" in str(e.value)
    with pytest.raises(ValueError):
        _capi.chains_marginal_edges(chains, 1, 10, 0)


def _digest(me):
    h = hashlib.sha256()
    for k in ("estimate", "sd", "lower_bound", "upper_bound", "p_pos", "p_neg", "var_within"):
        h.update(np.ascontiguousarray(getattr(me, k)).tobytes())
    return h.hexdigest()


_CHILD = """
import sys
sys.path[:0] = [%r, %r]
import dataclasses
import hashlib
import numpy as np
import bnr_amd
from bnr_amd import _capi, api
X, y, _ = bnr_amd.make_synthetic(20, 6, 2, seed=7)
ch = bnr_amd.Chain(X, y, 2, 60, 11, 1)
ch.init_prior()
ch.run(2, 60, 60)
if %d:
    api.device_marginal_loo([ch], 5, 40, 3)
me = api.device_marginal_edges([ch], 5, 40, 3)
h = hashlib.sha256()
for k in ("estimate", "sd", "lower_bound", "upper_bound", "p_pos", "p_neg", "var_within"):
    h.update(np.ascontiguousarray(getattr(me, k)).tobytes())
print("DIGEST", h.hexdigest(), int(_capi._mloo is not None))
ch.close()
"""


def test_both_libraries_in_one_process(fit):
    _X, _y, chains, _tables = fit
    a = api.device_marginal_loo(chains, 5, 40, 3)
    me = api.device_marginal_edges(chains[:1], 5, 40, 3)
    b = api.device_marginal_loo(chains, 5, 40, 3)
    assert set(a) == set(b) and all(np.array_equal(a[k], b[k], equal_nan=True) for k in a)          # marginal LOO before and after: identical bits
    digests = []
    for with_mloo in (0, 1):                                                                        # a fresh process each: with and without libbnr_mloo.so loaded first
        r = subprocess.run([sys.executable, "-c", _CHILD % (ROOT, os.path.join(ROOT, "tests"), with_mloo)], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                           text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        line = [l for l in r.stdout.splitlines() if l.startswith("DIGEST")][0].split()
        assert int(line[2]) == with_mloo
        digests.append(line[1])
    assert digests[0] == digests[1] == _digest(me)


def test_fit_with_the_flag_adds_the_result_and_changes_nothing_else(gpu, tmp_path):
    X, y, _ = bnr_amd.make_synthetic(20, 6, 2, seed=7)
    kw = dict(nburn=30, nsamples=40, num_chains=2, seed=5, x_transform=False, suppress_timer=True, filename=str(tmp_path / "p.log"), loo=True,
              summary_interval=95, stack_chains=True)
    a = bnr_amd.Fit(X, y, 2, **kw)
    b = bnr_amd.Fit(X, y, 2, marginal_edges=True, marginal_edges_draws=15, **kw)
    assert a.marginal_edges is None and a.stacking.marginal_edges is None
    for f in ("rhatxi", "rhatgamma", "burn_in", "sampled", "stat_chains"):
        assert np.array_equal(getattr(a, f), getattr(b, f)), f
    for f in ("loo", "summary_device"):
        assert set(getattr(a, f)) == set(getattr(b, f)) and all(np.array_equal(getattr(a, f)[k], getattr(b, f)[k], equal_nan=True) for k in getattr(a, f)), f
    assert all(np.array_equal(a.state[k], b.state[k], equal_nan=True) for k in a.state)
    assert np.array_equal(a.stacking.weights, b.stacking.weights) and np.array_equal(a.stacking.elpd_chain, b.stacking.elpd_chain)
    assert all(np.array_equal(a.stacking.summary[k], b.stacking.summary[k], equal_nan=True) for k in a.stacking.summary)
    seen = {"rhatxi", "rhatgamma", "burn_in", "sampled", "stat_chains", "loo", "summary_device", "state", "stacking", "marginal_edges"}
    for f in dataclasses.fields(a):                                                                 # every other field: not requested, None in both
        assert f.name in seen or (getattr(a, f.name) is None and getattr(b, f.name) is None), f.name
    me = bnr_amd.MarginalEdges(b)
    assert me is b.marginal_edges and me.thin == 3 and me.draws == 14 and me.chains == 1 and me.n_bad == 0 and me.estimate.shape == (21,)
    h = api._host_marginal_edges([b.state], np.asarray(X, dtype=np.float64), y, b.burn_in, b.sampled, 3)
    assert np.allclose(me.estimate, h.estimate, rtol=1e-9, atol=1e-12) and np.allclose(me.sd, h.sd, rtol=1e-9) and np.allclose(me.lfsr, h.lfsr, rtol=1e-8, atol=1e-300)
    assert np.allclose(me.lower_bound, h.lower_bound, rtol=1e-8, atol=1e-9) and np.allclose(me.upper_bound, h.upper_bound, rtol=1e-8, atol=1e-9)
    st = b.stacking.marginal_edges
    assert st.chains == 2 and st.draws == 28 and np.array_equal(st.weights, b.stacking.weights) and np.all(np.isfinite(st.estimate))
