"""GPU tests of the marginal LOO predictive checks (include/bnr_mcheck.h, libbnr_mcheck.so; kernels in csrc/bnr_mcheck_kernels.h): the raw call
against the mpmath reference within the derived bound (tests/mcheck_ref.py) at the edges of the wave stride (64) and of the workgroup stride (256);
cases whose answer is exact; the independence of a row's bits from the other rows, its place, the outputs asked for, the call and the batch;
NaN rows; live chains against bnr_chains_marginal_loo, the raw call and the numpy restatement; Fit.

Choices the issue leaves open, and why:
  - a case of k rows is the first k rows of the same five (mcheck_ref.case): a row's reference is computed once, in mpmath, for every case that
    holds the row -- the bitwise independence the second group of tests asserts is what makes that the same check.
  - the chain call's pit and bounds are compared with bnr_weighted_mixture on mean = y - resid formed in numpy: the same rounding the stage
    kernel applies, so the comparison is bit for bit (include/bnr_mcheck.h says how resid is taken back from it).
  - device against numpy restatement on the SAME matrices: each is within the gate of its own bound of the exact value, so they are within twice
    the gate of each other; for the bounds, the restatement's CDF at the device's bound has to be within both bounds of p (plus the slope over
    the last bracket).  The restatement over the fetched TABLES (its own factorization, its own PSIS) has no first-order bound through the
    Pareto fit: it is held to test_marginal_loo_gpu's precedent for loo_mean (rtol 1e-9)."""
import math

import numpy as np
import pytest

import bnr_amd
import mcheck_ref as cr
from bnr_amd import _capi, api

pytestmark = pytest.mark.gpu
FIELDS = _capi.MCHECK_FIELDS
WORST = {}


def _raw(c, rows, interval=95, with_y=True, fields=None, sel=None):
    p_lo, p_hi = api._loo_interval_probs(interval)
    idx = list(range(rows)) if sel is None else list(sel)
    out = _capi.weighted_mixture_raw(c["mean"][idx], c["var"][idx], c["logw"][idx], c["y"][idx] if with_y else None, p_lo, p_hi, 0, fields)
    return dict(zip(FIELDS, out))


def _same(a, b, ia=slice(None), ib=slice(None), fields=FIELDS):
    return all(np.array_equal(a[k][ia], b[k][ib], equal_nan=True) for k in fields)


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    print("\nweighted mixture, largest error over its first-order bound (gate %g):" % cr.GATE, {k: "%.3g" % v for k, v in sorted(WORST.items())})


# ------------------------------------------------------------------------------------------ against the reference
@pytest.mark.parametrize("pattern", cr.PATTERNS)
@pytest.mark.parametrize("D", (1, 2, 63, 64, 65, 255, 256, 257, 1025))
@pytest.mark.parametrize("rows", (1, 3, 5))
def test_raw_call_meets_the_bound_of_the_reference(gpu, rows, D, pattern):
    c = cr.case(D, pattern)
    for interval in (95, 50):
        p_lo, p_hi = api._loo_interval_probs(interval)
        got = _raw(c, rows, interval)
        w = cr.check_case(D, pattern, rows, got, p_lo, p_hi)
        for k, v in w.items():
            WORST[k] = max(WORST.get(k, 0.0), v)
        ok = np.isfinite(got["lower"])
        assert np.all(got["lower"][ok] <= got["upper"][ok])              # (equal for one point mass alone)
    if pattern == "nanrow" and rows > 1:                                 # the NaN row leaves its neighbours' bits unchanged
        clean = _raw(cr.case(D, "random"), rows)
        keep = [i for i in range(rows) if i not in c["nan_rows"]]
        assert _same(_raw(c, rows), clean, keep, keep)
    if rows == 5 and D in (2, 257):                                      # the form without y: mean = sum w m, no pit
        noy = _raw(c, rows, with_y=False)
        assert noy["pit"] is None
        cr.check_case(D, pattern, rows, dict(noy, pit=np.full(rows, np.nan)), *api._loo_interval_probs(95), with_y=False)


def test_exact_cases(gpu):
    rng = np.random.default_rng(189)
    D = 65
    m, v = rng.normal(size=(4, D)) * 2, np.zeros((4, D))
    lw = np.full((4, D), -800.0)
    hot = [0, 63, 64, 17]
    for i, s in enumerate(hot):
        lw[i, s] = 0.0
    y = np.array([m[0, 0] + 1.0, m[1, 63] - 1.0, m[2, 64], np.nan])
    r = bnr_amd.weighted_mixture(m, v, lw)                              # one point mass carries the weight: w = 1 and 0 exactly, no erfc
    assert np.array_equal(r["mean"], [m[i, s] for i, s in enumerate(hot)]) and np.array_equal(r["sd"], np.zeros(4)) and r["pit"] is None
    r = bnr_amd.weighted_mixture(m, v, lw, y)
    assert np.array_equal(r["pit"][:3], [1.0, 0.0, 1.0]) and math.isnan(r["pit"][3])                # [y >= m]; y = m counts
    assert math.isnan(r["mean"][3]) and math.isnan(r["sd"][3]) and np.isfinite(r["lower"][3]) and np.isfinite(r["upper"][3])
    w = np.max(m, axis=1) - np.min(m, axis=1)                            # the step is found to 2^-40 of the bracket, from below or above
    for k in ("lower", "upper"):
        assert np.all(np.abs(r[k] - [m[i, s] for i, s in enumerate(hot)]) <= w * 2.0 ** -40), k
    # every draw the same point: the bracket has no width and is its own midpoint
    one = bnr_amd.weighted_mixture(np.full((2, 5), 1.5), np.zeros((2, 5)), np.full((2, 5), math.log(0.2)), interval=50)
    assert np.array_equal(one["lower"], [1.5, 1.5]) and np.array_equal(one["upper"], [1.5, 1.5])
    # D = 1 with var > 0: mean = m (no y), sd^2 = (var + m^2) - m^2, pit = Phi((y - m) / sd) to the erfc allowance
    m1, v1, y1 = np.array([[0.75], [-3.0]]), np.array([[4.0], [0.25]]), np.array([1.0, -3.5])
    r = bnr_amd.weighted_mixture(m1, v1, np.zeros((2, 1)), y1)
    z = (y1 - m1[:, 0]) / np.sqrt(v1[:, 0])
    ref = np.array([0.5 * math.erfc(-t / math.sqrt(2)) for t in z])
    assert np.all(np.abs(r["pit"] - ref) <= 2 * (0.5 * z * z + 4 + 9) * cr.U * ref) and np.array_equal(r["sd"], [2.0, 0.5])
    assert np.array_equal(bnr_amd.weighted_mixture(m1, v1, np.zeros((2, 1)))["mean"], m1[:, 0])


def test_many_rows_cross_the_launch_chunk(gpu):
    """more rows than one launch of the row kernels takes (2^20), one draw each: the last rows are those of a small call, bit for bit"""
    rows = (1 << 20) + 3
    rng = np.random.default_rng(190)
    m, v, y = rng.normal(size=(rows, 1)), rng.exponential(size=(rows, 1)) + 0.5, rng.normal(size=rows)
    lw = np.zeros((rows, 1))
    big = dict(zip(FIELDS, _capi.weighted_mixture_raw(m, v, lw, y)))
    tail = slice(rows - 6, rows)
    small = dict(zip(FIELDS, _capi.weighted_mixture_raw(m[tail], v[tail], lw[tail], y[tail])))
    assert _same(big, small, tail)
    head = dict(zip(FIELDS, _capi.weighted_mixture_raw(m[:4], v[:4], lw[:4], y[:4])))
    assert _same(big, head, slice(0, 4)) and np.isfinite(big["lower"]).all() and np.all(big["lower"] < big["upper"])


# ------------------------------------------------------------------------------------------ independence
@pytest.mark.parametrize("D", (65, 257, 1025))
def test_a_row_does_not_depend_on_the_others_its_place_the_outputs_or_the_call(gpu, D):
    c = cr.case(D, "points")
    full = _raw(c, 5)
    for i in range(5):
        assert _same(full, _raw(c, 1, sel=[i]), slice(i, i + 1)), i                                 # alone and among five
    order = [4, 1, 2, 3, 0]
    swapped = _raw(c, 5, sel=order)
    assert _same(full, swapped, order)                                                              # its place in the call
    assert _same(full, _raw(c, 5))                                                                  # a repeated call
    for fields in (("mean",), ("sd",), ("pit",), ("lower",), ("upper",), ("lower", "upper"), ("mean", "pit", "upper")):
        part = _raw(c, 5, fields=fields)
        assert _same(full, part, fields=fields) and all(part[k] is None for k in FIELDS if k not in fields), fields
    other = _raw(c, 5, interval=50)                                                                 # the interval moves the bounds alone
    assert _same(full, other, fields=("mean", "sd", "pit")) and np.all(other["lower"] > full["lower"]) and np.all(other["upper"] < full["upper"])
    noy = _raw(c, 5, with_y=False)
    assert _same(full, noy, fields=("lower", "upper"))                                              # the bounds do not read y


def test_nan_rows(gpu):
    c = cr.case(257, "random")
    base = _raw(c, 5)
    spoil = (("var", np.nan), ("var", -1.0), ("mean", np.nan), ("logw", np.inf), ("logw", -np.inf), ("logw", np.nan))
    for name, val in spoil:
        d = {k: (c[k].copy() if k != "nan_rows" else ()) for k in c}
        d[name][2, 200] = val
        got = _raw(d, 5)
        assert all(math.isnan(got[k][2]) for k in FIELDS), (name, val)
        assert _same(base, got, [0, 1, 3, 4], [0, 1, 3, 4]), (name, val)
    d = {k: (c[k].copy() if k != "nan_rows" else ()) for k in c}
    d["y"][3] = np.nan
    got = _raw(d, 5)
    assert all(math.isnan(got[k][3]) for k in ("mean", "sd", "pit")) and _same(base, got, fields=("lower", "upper"))
    assert _same(base, got, [0, 1, 2, 4], [0, 1, 2, 4])


# ------------------------------------------------------------------------------------------ live chains
TOT = 40


@pytest.fixture(scope="module", params=(17, 33))
def fit(gpu, request):
    n = request.param
    X, y, _ = bnr_amd.make_synthetic(n, 6, 2, seed=7)
    chains = [bnr_amd.Chain(X, y, 2, TOT, 11, 1)]
    chains.append(bnr_amd.Chain.like(chains[0], 11, 2, TOT))
    for ch in chains:
        ch.init_prior()
        ch.run(2, TOT, TOT)
    tables = [ch.fetch() for ch in chains]
    yield n, np.asarray(X, dtype=np.float64), np.asarray(y, dtype=np.float64), chains, tables
    for ch in chains:
        ch.close()


@pytest.fixture
def batch_option():
    yield lambda v: _capi.mcheck_set_option("mcheck_batch_draws", v)
    _capi.mcheck_set_option("mcheck_batch_draws", 0)


@pytest.mark.parametrize("thin", (1, 3))
def test_live_chains(fit, batch_option, thin):
    n, X, y, chains, tables = fit
    nburn, nsamp = 9, 31                                                                            # 31 rows per chain: 62 draws, or 2 x 11 thinned
    nd = -(-nsamp // thin)
    D = 2 * nd
    p_lo, p_hi = api._loo_interval_probs(95)
    before = [(ch.iter, ch.counters()) for ch in chains]
    el0, kh0, lm0, ls0, ml0, ll0, nb0 = _capi.chains_marginal_loo(chains, nburn + 1, nsamp, thin, loglik=True)
    el, kh, (mean, sd, pit, lo, hi), ml, ll, nb = _capi.chains_marginal_loo_predict(chains, nburn + 1, nsamp, thin, None, p_lo, p_hi, loglik=True)
    assert nb == nb0 == 0 and ll.shape == (n, D)
    assert np.array_equal(el, el0) and np.array_equal(kh, kh0) and np.array_equal(ll, ll0) and np.array_equal(ml, ml0)   # with ==
    # the matrices the kernels saw: the raw marginal call on the same draws (bit for bit the chain form's), and PSIS on its loglik
    t2, mu, S, W = api._host_marginal_draws(tables, nburn, nsamp, thin)
    dev = bnr_amd.marginal_loglik(X, y, t2, mu, S, W)
    assert np.array_equal(dev["loglik"], ll)
    rs, vr = dev["resid"], dev["var"]
    lw, _e, _k = _capi.psis_weights_raw(ll)
    m = y[:, None] - rs
    b = cr.numpy_bounds(m, vr, lw, y)
    assert np.all(b["sd2"] >= cr.SD_FLOOR * b["e2"])
    # loo_mean, loo_sd against bnr_chains_marginal_loo's (a host loop in draw order): each within its bound
    assert np.all(np.abs(mean - lm0) <= 2 * cr.GATE * b["tol_mean"]), float(np.max(np.abs(mean - lm0) / b["tol_mean"]))
    assert np.all(np.abs(sd - ls0) <= 2 * cr.GATE * b["tol_sd"]), float(np.max(np.abs(sd - ls0) / b["tol_sd"]))
    # every output against the raw call on the fetched matrices, bit for bit
    raw = dict(zip(FIELDS, _capi.weighted_mixture_raw(m, vr, lw, y, p_lo, p_hi)))
    got = dict(mean=mean, sd=sd, pit=pit, lower=lo, upper=hi)
    assert _same(got, raw)
    # ... and the numpy restatement on them within the bound
    h = dict(zip(FIELDS, api._host_weighted_mixture(m, vr, lw, y, p_lo, p_hi)[:5]))
    for k in ("mean", "sd", "pit"):
        r = np.abs(got[k] - h[k]) / b["tol_" + k]
        assert np.all(r <= 2 * cr.GATE), (k, float(r.max()))
        WORST["chain " + k] = max(WORST.get("chain " + k, 0.0), float(r.max()))
    c = api._loo_bracket_c(p_lo, p_hi)
    for i in range(n):
        hh = cr.bracket_width(m[i], vr[i], c) * 2.0 ** -40
        for t, p in ((lo[i], p_lo), (hi[i], p_hi)):                                                 # the restatement's CDF brackets p at the device's bound
            (Fa, ea), (Fb, eb) = cr.numpy_cdf(t - hh, m[i], vr[i], lw[i]), cr.numpy_cdf(t + hh, m[i], vr[i], lw[i])
            assert Fa - 2 * cr.GATE * ea <= p <= Fb + 2 * cr.GATE * eb, (i, p, t, Fa, Fb)
    # the batch option changes no bit
    for bd in (1, 3):
        batch_option(bd)
        again = _capi.chains_marginal_loo_predict(chains, nburn + 1, nsamp, thin, None, p_lo, p_hi, loglik=True)
        assert np.array_equal(again[0], el) and np.array_equal(again[1], kh) and np.array_equal(again[4], ll)
        assert _same(got, dict(zip(FIELDS, again[2])))
    batch_option(0)
    # outputs asked for
    part = _capi.chains_marginal_loo_predict(chains, nburn + 1, nsamp, thin, fields=("pit", "upper"))
    assert np.array_equal(part[2][2], pit) and np.array_equal(part[2][4], hi) and part[2][0] is None and np.array_equal(part[0], el)
    none = _capi.chains_marginal_loo_predict(chains, nburn + 1, nsamp, thin, fields=())
    assert np.array_equal(none[0], el) and np.array_equal(none[1], kh) and all(o is None for o in none[2])
    # the record, and the restatement over the fetched tables
    rec = api.device_marginal_loo_predict(chains, nburn, nsamp, thin)
    assert np.array_equal(rec.loo_pit, pit) and np.array_equal(rec.loo_lower, lo) and rec.draws == D and rec.thin == thin and rec.chains == 2
    assert rec.n_bad == 0 and np.array_equal(rec.loo["elpd_loo_i"], el) and np.array_equal(rec.loo["loo_mean"], mean) and rec.interval == 95
    assert rec.coverage == float(np.mean((y >= lo) & (y <= hi))) and rec.ks == api._ks_uniform(pit)
    host = api._host_marginal_loo_predict(tables, X, y, nburn, nsamp, thin)
    for k in ("loo_mean", "loo_sd", "loo_pit", "loo_lower", "loo_upper"):
        assert np.allclose(getattr(rec, k), getattr(host, k), rtol=1e-9, atol=1e-12), k
    assert [(ch.iter, ch.counters()) for ch in chains] == before                                    # nothing of any chain is written
    for ch, t in zip(chains, tables):
        now = ch.fetch()
        assert all(np.array_equal(now[k], t[k], equal_nan=True) for k in t)


def test_a_bad_draw_makes_every_row_nan(fit):
    n, X, y, chains, tables = fit
    ch = bnr_amd.Chain.like(chains[0], 11, 3, TOT)
    try:
        t = {k: v.copy() for k, v in tables[0].items()}
        t["S"][20, 3, 0] = np.nan
        ch.load(t)
        el, kh, out, ml, ll, nb = _capi.chains_marginal_loo_predict([chains[1], ch], 10, 31, 1, loglik=True)
        assert nb == 1 and np.isnan(ll[:, 31 + 11]).all() and math.isnan(ml[31 + 11])
        assert all(np.isnan(o).all() for o in out)                                                  # every row, all five outputs
        el0, kh0 = _capi.chains_marginal_loo([chains[1], ch], 10, 31, 1)[:2]
        assert np.array_equal(el, el0, equal_nan=True) and np.array_equal(kh, kh0, equal_nan=True)  # pareto_k: bnr_psis_weights' convention
        ok = _capi.chains_marginal_loo_predict([chains[1], ch], 22, 19, 1)                          # the window behind the bad row
        assert ok[5] == 0 and all(np.isfinite(o).all() for o in ok[2])
    finally:
        ch.close()


def test_chain_call_refusals(fit):
    n, X, y, chains, _tables = fit
    for args in ((0, 10, 1), (1, TOT + 1, 1), (TOT, 2, 1)):
        with pytest.raises(bnr_amd.BnrError) as e:
            _capi.chains_marginal_loo_predict(chains, *args)
        assert e.value.code == 1 and "window" in str(e.value)
    with pytest.raises(bnr_amd.BnrError) as e:
        _capi.chains_marginal_loo_predict([chains[0], chains[0]], 1, 10, 1)
    assert "twice" in str(e.value)
    with pytest.raises(ValueError):
        _capi.chains_marginal_loo_predict(chains, 1, 10, 0)
    with pytest.raises(ValueError):
        _capi.chains_marginal_loo_predict(chains, 1, 10, 1, p_lo=0.6, p_hi=0.4)


def test_marginal_loo_is_unchanged_with_all_five_libraries_loaded(fit):
    n, X, y, chains, _tables = fit
    _capi.medge_lib(), _capi.mpred_lib()
    a = _capi.chains_marginal_loo(chains, 10, 31, 1, loglik=True)
    api.device_marginal_loo_predict(chains, 9, 31)
    b = _capi.chains_marginal_loo(chains, 10, 31, 1, loglik=True)
    assert _capi._lib is not None and _capi._mloo is not None and _capi._medge is not None and _capi._mpred is not None and _capi._mcheck is not None
    assert all(np.array_equal(x, z) for x, z in zip(a[:6], b[:6])) and a[6] == b[6]
    ra = api.device_marginal_loo(chains, 9, 31)
    api.device_marginal_loo_predict(chains, 9, 31, 3, 50)
    rb = api.device_marginal_loo(chains, 9, 31)
    assert all(np.array_equal(ra[k], rb[k]) for k in ra)


def test_fit_with_the_flag_adds_the_result_and_changes_nothing_else(gpu, tmp_path):
    X, y, _ = bnr_amd.make_synthetic(20, 6, 2, seed=7)
    kw = dict(nburn=30, nsamples=40, num_chains=2, seed=5, x_transform=False, suppress_timer=True, filename=str(tmp_path / "p.log"), loo=True,
              marginal_loo=True, marginal_loo_draws=15)
    a = bnr_amd.Fit(X, y, 2, **kw)
    b = bnr_amd.Fit(X, y, 2, marginal_loo_predict=True, predict_interval=90, **kw)
    assert a.marginal_loo_predictive is None and b.marginal_loo_predictive is not None
    for f in api.Results.__dataclass_fields__:
        if f == "marginal_loo_predictive":
            continue
        x, z = getattr(a, f), getattr(b, f)
        if isinstance(x, dict):
            assert set(x) == set(z) and all(np.array_equal(x[k], z[k], equal_nan=True) for k in x), f
        else:
            assert (x is z) or np.array_equal(x, z, equal_nan=True), f
    r = bnr_amd.MarginalLOOPredict(b)
    assert r is b.marginal_loo_predictive and r.thin == 3 and r.draws == 14 and r.chains == 1 and r.n_bad == 0 and r.interval == 90
    assert r.loo_mean.shape == (20,) and np.all(r.loo_lower < r.loo_mean) and np.all(r.loo_mean < r.loo_upper) and 0.0 <= r.coverage <= 1.0
    for k in ("elpd_loo_i", "pareto_k", "lpd_i", "logml"):                                          # one call serves both needs
        assert np.array_equal(r.loo[k], b.marginal_loo[k]), k
    h = api._host_marginal_loo_predict([b.state], np.asarray(X, dtype=np.float64), y, b.burn_in, b.sampled, 3, 90)
    for k in ("loo_mean", "loo_sd", "loo_pit", "loo_lower", "loo_upper"):
        assert np.allclose(getattr(r, k), getattr(h, k), rtol=1e-9, atol=1e-12), k
    p = bnr_amd.Fit(X, y, 2, marginal_loo_predict=True, pool_chains=True, **kw)
    assert p.marginal_loo_predictive.draws == 28 and p.marginal_loo_predictive.chains == 2 and p.stat_chains == 2
