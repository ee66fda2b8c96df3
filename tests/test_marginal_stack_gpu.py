"""GPU tests of the chain stacking on the marginal PSIS-LOO (include/bnr_mstack.h, libbnr_mstack.so; kernel in csrc/bnr_mstack_kernels.h): the raw
call against the mpmath reference within the derived bound (tests/mstack_ref.py) at the edges of the 256-component strip and of the chains; the
cases that are exact; the independence of a row's bits from the other rows, the outputs asked for and the call; live chains against
bnr_chains_marginal_loo, bnr_chains_marginal_loo_predict, bnr_stacking_weights, the raw call and the numpy restatement; Fit.

Choices the issue leaves open, and why:
  - a case of k rows is the first k rows of the same five (mstack_ref.case): a row's reference is computed once, in mpmath, for every case that
    holds the row -- the bitwise independence the third group of tests asserts is what makes that the same check.
  - the chain call's checks are compared with bnr_stacked_mixture on mean = y - resid formed in numpy: the same rounding the staging kernel
    applies, so the comparison is bit for bit.
  - the restatement over the fetched TABLES (its own factorization, its own PSIS) is given the device's weights -- the solver's own agreement is
    the == against bnr_stacking_weights -- and has no first-order bound through the Pareto fit: it is held to test_marginal_loo_predict_gpu's
    precedent (rtol 1e-9)."""
import math

import numpy as np
import pytest

import bnr_amd
import mstack_ref as sr
from bnr_amd import _capi, api

pytestmark = pytest.mark.gpu
FIELDS = _capi.MCHECK_FIELDS
WORST = {}
SHAPES = ((1, 1), (1, 2), (1, 257), (2, 128), (3, 85), (3, 86), (2, 513), (32, 8))


def _raw(c, w, K, rows, interval=95, with_y=True, fields=None, sel=None):
    p_lo, p_hi = api._loo_interval_probs(interval)
    idx = list(range(rows)) if sel is None else list(sel)
    out = _capi.stacked_mixture_raw(c["mean"][idx], c["var"][idx], c["logw"][idx], w, K, c["y"][idx] if with_y else None, p_lo, p_hi, 0, fields)
    return dict(zip(FIELDS, out))


def _plain(mean, var, logw, y, interval=95):
    p_lo, p_hi = api._loo_interval_probs(interval)
    return dict(zip(FIELDS, _capi.weighted_mixture_raw(mean, var, logw, y, p_lo, p_hi)))


def _same(a, b, ia=slice(None), ib=slice(None), fields=FIELDS):
    return all(np.array_equal(a[k][ia], b[k][ib], equal_nan=True) for k in fields)


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    print("\nstacked mixture, largest error over its first-order bound (gate %g):" % sr.GATE, {k: "%.3g" % v for k, v in sorted(WORST.items())})


# ------------------------------------------------------------------------------------------ against the reference
@pytest.mark.parametrize("pattern", sr.PATTERNS)
@pytest.mark.parametrize("wname", sr.WEIGHTS)
@pytest.mark.parametrize("K,nd", SHAPES)
def test_raw_call_meets_the_bound_of_the_reference(gpu, K, nd, wname, pattern):
    if K == 1 and wname != "uniform":
        return                                                           # (K = 1: every weight pattern is (1,))
    c, w = sr.case(K, nd, pattern), sr.chain_weights(K, wname)
    for interval in (95, 50):
        p_lo, p_hi = api._loo_interval_probs(interval)
        full = None
        for rows in (5, 3, 1):
            got = _raw(c, w, K, rows, interval)
            worst = sr.check_case(K, nd, pattern, wname, rows, got, p_lo, p_hi)
            for k, v in worst.items():
                WORST[k] = max(WORST.get(k, 0.0), v)
            ok = np.isfinite(got["lower"])
            assert np.all(got["lower"][ok] <= got["upper"][ok])          # (equal for one point mass alone)
            full = full or got
            assert _same(full, got, slice(0, rows))
    if pattern == "nanrow":                                              # the NaN row leaves its neighbours' bits unchanged
        clean = _raw(sr.case(K, nd, "random"), w, K, 5)
        keep = [i for i in range(5) if i not in sr.nan_rows(K, nd, pattern, w)]
        assert _same(_raw(c, w, K, 5), clean, keep, keep)
    if (K, nd) in ((1, 2), (3, 86)):                                     # the form without y: mean = sum w m, no pit
        noy = _raw(c, w, K, 5, with_y=False)
        assert noy["pit"] is None
        sr.check_case(K, nd, pattern, wname, 5, dict(noy, pit=np.full(5, np.nan)), *api._loo_interval_probs(95), with_y=False)


@pytest.mark.parametrize("pattern", sr.PATTERNS)
def test_a_dropped_chain_brings_the_mixture_to_one_strip(gpu, pattern):
    """(3, 128) with w = (1/2, 0, 1/2): D+ = 256 is reached by dropping a chain.  The reference is the case's own through a StackRow."""
    K, nd, w = 3, 128, np.array([0.5, 0.0, 0.5])
    c = sr.case(K, nd, pattern)
    cols = sr.retained_columns(K, nd, w)
    cref = sr.case(K, nd, sr.mc.ref_pattern(pattern))
    for interval in (95, 50):
        p_lo, p_hi = api._loo_interval_probs(interval)
        got = _raw(c, w, K, 5, interval)
        cw = sr.mc.bracket_c(p_lo, p_hi)
        for i in range(5):
            if i in sr.nan_rows(K, nd, pattern, w):
                assert all(math.isnan(got[k][i]) for k in FIELDS)
                continue
            row = sr.StackRow(cref["mean"][i], cref["var"][i], cref["logw"][i], w, cref["y"][i])
            mo = row.moments()
            assert mo["sd2"] >= sr.SD_FLOOR * mo["e2"]
            assert abs(got["mean"][i] - mo["mean"]) <= sr.GATE * mo["tol_mean"] and abs(got["sd"][i] - mo["sd"]) <= sr.GATE * mo["tol_sd"], (pattern, i)
            ref, tol = row.pit()
            assert abs(got["pit"][i] - ref) <= sr.GATE * tol, (pattern, i)
            width = sr.mc.bracket_width(cref["mean"][i][cols], cref["var"][i][cols], cw)
            for k, p in (("lower", p_lo), ("upper", p_hi)):
                assert sr.mc.quantile_ok(row, float(got[k][i]), p, width)[0], (pattern, i, k)
    two = dict(mean=c["mean"][:, cols], var=c["var"][:, cols], logw=c["logw"][:, cols], y=c["y"])      # ... and the two chains alone, bit for bit
    assert _same(_raw(c, w, K, 5), _raw(two, np.array([0.5, 0.5]), 2, 5))


# ------------------------------------------------------------------------------------------ exact cases
@pytest.mark.parametrize("pattern", ("random", "points", "nanrow", "onehot"))
def test_exact_cases(gpu, pattern):
    for D in (1, 2, 257):                                                # K = 1 is bnr_weighted_mixture
        c = sr.case(1, D, pattern)
        for interval in (95, 50):
            assert _same(_raw(c, [1.0], 1, 5, interval), _plain(c["mean"], c["var"], c["logw"], c["y"], interval)), (D, interval)
        noy = _raw(c, [1.0], 1, 5, with_y=False)
        ref = dict(zip(FIELDS, _capi.weighted_mixture_raw(c["mean"], c["var"], c["logw"])))
        assert _same(noy, ref, fields=("mean", "sd", "lower", "upper"))
    for K, nd in ((3, 85), (3, 86), (2, 513)):                           # w = e_k is bnr_weighted_mixture on chain k's columns
        c = sr.case(K, nd, pattern)
        for k in range(K):
            cols = slice(k * nd, (k + 1) * nd)
            got = _raw(c, np.eye(K)[k], K, 5)
            assert _same(got, _plain(c["mean"][:, cols], c["var"][:, cols], c["logw"][:, cols], c["y"])), (K, nd, k)
    K, nd = 3, 86                                                        # the dropped chain's columns filled with NaN change no bit
    c = sr.case(K, nd, pattern)
    for w in (sr.chain_weights(K, "zero"), sr.chain_weights(K, "unit")):
        d = {k: np.array(c[k]) for k in ("mean", "var", "logw", "y")}
        for k in range(K):
            if w[k] == 0:
                for f in ("mean", "var", "logw"):
                    d[f][:, k * nd:(k + 1) * nd] = np.nan
        assert _same(_raw(c, w, K, 5), _raw(d, w, K, 5)), w


# ------------------------------------------------------------------------------------------ independence
@pytest.mark.parametrize("K,nd", ((3, 85), (2, 513)))
def test_a_row_does_not_depend_on_the_others_the_outputs_or_the_call(gpu, K, nd):
    c, w = sr.case(K, nd, "points"), sr.chain_weights(K, "random")
    full = _raw(c, w, K, 5)
    for i in range(5):
        assert _same(full, _raw(c, w, K, 1, sel=[i]), slice(i, i + 1)), i                           # alone and among five
    order = [4, 1, 2, 3, 0]
    assert _same(full, _raw(c, w, K, 5, sel=order), order)                                          # its place in the call
    assert _same(full, _raw(c, w, K, 5))                                                            # a repeated call
    for fields in (("mean",), ("sd",), ("pit",), ("lower",), ("upper",), ("lower", "upper"), ("mean", "pit", "upper")):
        part = _raw(c, w, K, 5, fields=fields)
        assert _same(full, part, fields=fields) and all(part[k] is None for k in FIELDS if k not in fields), fields
    other = _raw(c, w, K, 5, interval=50)                                                           # the interval moves the bounds alone
    assert _same(full, other, fields=("mean", "sd", "pit")) and np.all(other["lower"] > full["lower"]) and np.all(other["upper"] < full["upper"])
    assert _same(full, _raw(c, w, K, 5, with_y=False), fields=("lower", "upper"))                   # the bounds do not read y
    lw = np.array(c["logw"])                                                                        # a log weight that is not finite: its row alone
    lw[2, nd + 3] = -np.inf
    got = _raw(dict(c, logw=lw), w, K, 5)
    assert all(math.isnan(got[k][2]) for k in FIELDS) and _same(full, got, [0, 1, 3, 4], [0, 1, 3, 4])


# ------------------------------------------------------------------------------------------ live chains
TOT = 40
NBURN, NSAMP = 9, 31


# (n = 300: the job setup of bnr_mloo_job.h with two workgroups of k_mloo_rhs along the rows and two 256-column passes of k_mloo_factor per draw)
@pytest.fixture(scope="module", params=((17, 2), (33, 3), (300, 2)), ids=("n17-K2", "n33-K3", "n300-K2"))
def fit(gpu, request):
    n, K = request.param
    X, y, _ = bnr_amd.make_synthetic(n, 6, 2, seed=7)
    chains = [bnr_amd.Chain(X, y, 2, TOT, 11, 1)]
    for k in range(1, K):
        chains.append(bnr_amd.Chain.like(chains[0], 11, k + 1, TOT))
    for ch in chains:
        ch.init_prior()
        ch.run(2, TOT, TOT)
    tables = [ch.fetch() for ch in chains]
    yield n, K, np.asarray(X, dtype=np.float64), np.asarray(y, dtype=np.float64), chains, tables
    for ch in chains:
        ch.close()


@pytest.fixture
def batch_option():
    yield lambda v: _capi.mstack_set_option("mstack_batch_draws", v)
    _capi.mstack_set_option("mstack_batch_draws", 0)


@pytest.mark.parametrize("thin", (1, 3))
def test_live_chains(fit, batch_option, thin):
    n, K, X, y, chains, tables = fit
    nd = -(-NSAMP // thin)
    D = K * nd
    p_lo, p_hi = api._loo_interval_probs(95)
    before = [(ch.iter, ch.counters()) for ch in chains]
    w, el, kh, es, gap, it, out, ml, nb = _capi.chains_marginal_stack(chains, NBURN + 1, NSAMP, thin, None, None, 100000, 1e-9, p_lo, p_hi)
    got = dict(zip(FIELDS, out))
    assert nb == 0 and el.shape == (K, n) and ml.shape == (D,) and np.isfinite(el).all()
    pooled = _capi.chains_marginal_loo(chains, NBURN + 1, NSAMP, thin, loglik=True)
    assert np.array_equal(ml, pooled[4])                                                            # logml: the pooled call's
    ll = pooled[5]
    for k in range(K):                                                                              # row k: chain k alone, with ==
        one = _capi.chains_marginal_loo([chains[k]], NBURN + 1, NSAMP, thin)
        assert np.array_equal(el[k], one[0]) and np.array_equal(kh[k], one[1]), k
    sw = _capi.stacking_weights_raw(el.T, 100000, 1e-9)                                             # the exported solver on the returned elpd_chain
    assert np.array_equal(w, sw[0]) and gap == sw[2] and it == sw[3] and gap <= 1e-9
    for i in range(n):                                                                              # the stacked score against mpmath
        ref, tol = sr.elpd_stack_ref(el[:, i], w)
        assert abs(es[i] - ref) <= sr.GATE * tol, (i, es[i], ref)
    st = api._stacking(w, el, kh, gap, it, nd)
    tol = np.array([sr.elpd_stack_ref(el[:, i], w)[1] for i in range(n)])                           # (the record's numpy form of the same formula: each
    assert np.all(np.abs(st.elpd_stack_i - es) <= 2 * sr.GATE * tol)                                # within its gate of the exact value)
    # the matrices the kernels saw: the raw marginal call on the same draws (bit for bit the chain form's), PSIS on every chain's slice
    t2, mu, S, W = api._host_marginal_draws(tables, NBURN, NSAMP, thin)
    dev = bnr_amd.marginal_loglik(X, y, t2, mu, S, W)
    assert np.array_equal(dev["loglik"], ll)
    rs, vr = dev["resid"], dev["var"]
    lw = np.concatenate([_capi.psis_weights_raw(ll[:, k * nd:(k + 1) * nd])[0] for k in range(K)], axis=1)
    m = y[:, None] - rs
    raw = dict(zip(FIELDS, _capi.stacked_mixture_raw(m, vr, lw, w, K, y, p_lo, p_hi)))
    assert _same(got, raw)                                                                          # bit for bit
    for k in range(K):                                                                              # given weights e_k: chain k's own checks, with ==
        fx = _capi.chains_marginal_stack(chains, NBURN + 1, NSAMP, thin, None, np.eye(K)[k], 100000, 1e-9, p_lo, p_hi)
        one = _capi.chains_marginal_loo_predict([chains[k]], NBURN + 1, NSAMP, thin, None, p_lo, p_hi)
        assert _same(dict(zip(FIELDS, fx[6])), dict(zip(FIELDS, one[2]))), k
        assert np.array_equal(fx[0], np.eye(K)[k]) and math.isnan(fx[4]) and fx[5] == 0 and np.array_equal(fx[1], el) and np.array_equal(fx[3], el[k])
    # the numpy restatement over the fetched tables under the device's weights
    host = api._host_marginal_stack(tables, X, y, NBURN, NSAMP, thin, weights=w)
    for f in FIELDS:
        assert np.allclose(got[f], getattr(host, "loo_" + f), rtol=1e-9, atol=1e-12), f
    assert np.allclose(host.elpd_chain_i, el, rtol=1e-9, atol=1e-12)
    # the batch option changes no bit
    for bd in (1, 3):
        batch_option(bd)
        again = _capi.chains_marginal_stack(chains, NBURN + 1, NSAMP, thin, None, None, 100000, 1e-9, p_lo, p_hi)
        assert np.array_equal(again[0], w) and np.array_equal(again[1], el) and np.array_equal(again[2], kh) and np.array_equal(again[3], es)
        assert _same(got, dict(zip(FIELDS, again[6]))) and np.array_equal(again[7], ml)
    batch_option(0)
    # outputs asked for
    part = _capi.chains_marginal_stack(chains, NBURN + 1, NSAMP, thin, fields=("pit", "upper"))
    assert np.array_equal(part[6][2], got["pit"]) and np.array_equal(part[6][4], got["upper"]) and part[6][0] is None and np.array_equal(part[0], w)
    none = _capi.chains_marginal_stack(chains, NBURN + 1, NSAMP, thin, fields=())
    assert np.array_equal(none[0], w) and np.array_equal(none[1], el) and all(o is None for o in none[6])
    # the record
    rec = api.device_marginal_stack(chains, NBURN, NSAMP, thin)
    assert np.array_equal(rec.weights, w) and np.array_equal(rec.loo_pit, got["pit"]) and np.array_equal(rec.loo_lower, got["lower"])
    assert rec.draws == D and rec.thin == thin and rec.chains == K and rec.n_bad == 0 and rec.interval == 95 and rec.n_used == n
    assert np.array_equal(rec.elpd_stack_i, st.elpd_stack_i) and rec.iterations == it and rec.gap == gap and np.array_equal(rec.logml, ml)
    assert rec.coverage == float(np.mean((y >= got["lower"]) & (y <= got["upper"]))) and rec.ks == api._ks_uniform(got["pit"])
    assert [(ch.iter, ch.counters()) for ch in chains] == before                                    # nothing of any chain is written
    for ch, t in zip(chains, tables):
        now = ch.fetch()
        assert all(np.array_equal(now[k], t[k], equal_nan=True) for k in t)


def test_a_bad_draw_leaves_no_row(fit):
    n, K, X, y, chains, tables = fit
    ch = bnr_amd.Chain.like(chains[0], 11, 7, TOT)
    try:
        t = {k: v.copy() for k, v in tables[0].items()}
        t["S"][20, 3, 0] = np.nan
        ch.load(t)
        w, el, kh, es, gap, it, out, ml, nb = _capi.chains_marginal_stack([chains[1], ch], 10, 31, 1)
        assert nb == 1 and math.isnan(ml[31 + 11]) and not np.isfinite(el[1]).any() and np.isfinite(el[0]).all()
        assert np.array_equal(w, [0.5, 0.5]) and math.isnan(gap) and it == 0 and np.isnan(es).all()
        assert all(np.isnan(o).all() for o in out)                                                  # every row, all five outputs
        ok = _capi.chains_marginal_stack([chains[1], ch], 22, 19, 1)                                # the window behind the bad row
        assert ok[8] == 0 and all(np.isfinite(o).all() for o in ok[6]) and abs(ok[0].sum() - 1) <= 1e-12
    finally:
        ch.close()


def test_chain_call_refusals(fit):
    n, K, X, y, chains, _tables = fit
    for args in ((0, 10, 1), (1, TOT + 1, 1), (TOT, 2, 1)):
        with pytest.raises(bnr_amd.BnrError) as e:
            _capi.chains_marginal_stack(chains, *args)
        assert e.value.code == 1 and "window" in str(e.value)
    with pytest.raises(bnr_amd.BnrError) as e:
        _capi.chains_marginal_stack([chains[0], chains[0]], 1, 10, 1)
    assert "twice" in str(e.value)
    for kw, word in ((dict(max_iter=0), "max_iter"), (dict(gap_tol=0.0), "gap_tol"), (dict(gap_tol=float("nan")), "gap_tol"),
                     (dict(weights=[0.7] * K), "sum to 1"), (dict(weights=[-1.0] + [2.0 / (K - 1)] * (K - 1)), "finite"),
                     (dict(weights=[0.0] * K), "one weight")):
        with pytest.raises(bnr_amd.BnrError) as e:
            _capi.chains_marginal_stack(chains, 1, 10, 1, **kw)
        assert e.value.code == 1 and word in str(e.value), kw
    with pytest.raises(ValueError):
        _capi.chains_marginal_stack(chains, 1, 10, 0)
    with pytest.raises(ValueError):
        _capi.chains_marginal_stack(chains, 1, 10, 1, p_lo=0.6, p_hi=0.4)
    with pytest.raises(ValueError):
        _capi.chains_marginal_stack(chains, 1, 10, 1, weights=[1.0])
    assert _capi.chains_marginal_stack(chains, 1, 10, 1, p_lo=0.6, p_hi=0.4, fields=("mean",))[8] == 0   # p is read only where a bound is asked for


def test_marginal_loo_is_unchanged_with_all_six_libraries_loaded(fit):
    n, K, X, y, chains, _tables = fit
    _capi.medge_lib(), _capi.mpred_lib(), _capi.mcheck_lib()
    a = _capi.chains_marginal_loo(chains, 10, 31, 1, loglik=True)
    api.device_marginal_stack(chains, 9, 31)
    b = _capi.chains_marginal_loo(chains, 10, 31, 1, loglik=True)
    assert all(getattr(_capi, x) is not None for x in ("_lib", "_mloo", "_medge", "_mpred", "_mcheck", "_mstack"))
    assert all(np.array_equal(x, z) for x, z in zip(a[:6], b[:6])) and a[6] == b[6]
    ra = api.device_marginal_loo(chains, 9, 31)
    api.device_marginal_stack(chains, 9, 31, 3, 50)
    rb = api.device_marginal_loo(chains, 9, 31)
    assert all(np.array_equal(ra[k], rb[k]) for k in ra)
    pa = api.device_marginal_loo_predict(chains, 9, 31)
    api.device_marginal_stack(chains, 9, 31)
    pb = api.device_marginal_loo_predict(chains, 9, 31)
    assert np.array_equal(pa.loo_pit, pb.loo_pit) and np.array_equal(pa.loo_upper, pb.loo_upper)


def _same_field(x, z):
    if isinstance(x, dict):
        return set(x) == set(z) and all(_same_field(x[k], z[k]) for k in x)
    if hasattr(x, "__dataclass_fields__"):
        return all(_same_field(getattr(x, f), getattr(z, f)) for f in x.__dataclass_fields__)
    if hasattr(x, "__dict__") and not isinstance(x, np.ndarray):
        return _same_field(vars(x), vars(z))
    return (x is z) or np.array_equal(x, z, equal_nan=True)


def test_fit_with_the_flag_adds_the_record_and_changes_nothing_else(gpu, tmp_path, monkeypatch):
    X, y, _ = bnr_amd.make_synthetic(20, 6, 2, seed=7)
    kw = dict(nburn=30, nsamples=40, num_chains=2, seed=5, x_transform=False, suppress_timer=True, filename=str(tmp_path / "p.log"),
              summary_interval=95, marginal_edges=True, marginal_loo_draws=15, stack_chains=True)
    a = bnr_amd.Fit(X, y, 2, **kw)
    inner, seen = api.device_summary_stacked, []

    def summary_stacked(chains, weights, *rest):                         # (the call itself, with what it was given and what it gave back)
        seen.append((np.array(weights), rest, inner(chains, weights, *rest)))
        return seen[-1][2]

    monkeypatch.setattr(api, "device_summary_stacked", summary_stacked)
    b = bnr_amd.Fit(X, y, 2, marginal_stack=True, predict_interval=95, **kw)
    monkeypatch.undo()
    assert a.marginal_stacking is None and b.marginal_stacking is not None and b.stacking is not None
    for f in api.Results.__dataclass_fields__:
        if f != "marginal_stacking":
            assert _same_field(getattr(a, f), getattr(b, f)), f
    r = bnr_amd.MarginalStack(b)
    assert r is b.marginal_stacking and r.thin == 3 and r.draws == 28 and r.chains == 2 and r.n_bad == 0 and r.interval == 95
    assert r.weights.shape == (2,) and abs(r.weights.sum() - 1) <= 1e-12 and r.elpd_chain_i.shape == (2, 20) and r.loo_mean.shape == (20,)
    assert np.all(r.loo_lower < r.loo_mean) and np.all(r.loo_mean < r.loo_upper) and 0.0 <= r.coverage <= 1.0 and r.elpd_stack >= r.elpd_uniform - 1e-9
    assert r.summary is not None and r.marginal_edges is not None and r.prediction is None and r.edge_cov is None
    assert r.marginal_edges.thin == 1 and r.marginal_edges.chains == 2 and np.array_equal(r.marginal_edges.weights, r.weights)   # (marginal_edges_draws, not marginal_loo_draws)
    assert len(seen) == 2 and r.summary is seen[1][2] and np.array_equal(seen[1][0], r.weights) and seen[1][1] == (30, 40, 95)   # device_summary_stacked with its weights
    assert b.stacking.summary is seen[0][2] and np.array_equal(seen[0][0], b.stacking.weights) and np.array_equal(r.summary["weights"], r.weights)
