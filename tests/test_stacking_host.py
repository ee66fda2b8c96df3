"""CPU tests of chain stacking (ABI 16; Yao, Vehtari & Gelman 2022): the weight solver bnr_stacking_weights against the duality bound and a
long-double run of the numpy restatement, its known answers and refusals, api._host_wquantile against an independent sort-and-scan
transcription of the definition, and the Python plumbing.  No GPU.

One bound differs from the issue's wording: 0 <= f_ref - objective is asserted as -1e-12 max(1, |f|) <= f_ref - objective.  The inequality
f(w*) >= f(w) holds for the exact f(w); the reported objective is a float64 sum of n rounded terms, which the same issue only asks to be
within 1e-12 max(1, |f|) of f(w), so with K = 1 (f(w) = f(w*) exactly) its rounding alone puts it above f_ref half of the time."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import bnr_amd
import code_objects as co
from bnr_amd import _capi, api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LD = np.longdouble
INSTANCES = ((8, 3), (40, 8), (500, 8), (16, 16), (1, 2), (5, 1), (7, 32))
GAP_TOL = 1e-9
NEW = ("bnr_stacking_weights", "bnr_chains_stack", "bnr_chains_wsummary", "bnr_chains_wpredict", "bnr_wquantile")


def test_abi_version_and_exports():
    hdr = open(os.path.join(ROOT, "include", "bnr_hip.h")).read()
    ver = int(re.search(r"#define BNR_ABI_VERSION (\d+)", hdr).group(1))
    L = _capi.lib()
    assert ver >= 16 and L.bnr_abi_version() == ver
    assert int(re.search(r"#define BNR_STACK_MAX_CHAINS (\d+)", hdr).group(1)) == api.STACK_MAX_CHAINS == 32
    for name in NEW:
        assert name in _capi.EXPORTS and getattr(L, name) is not None and re.search(r"\b%s\(" % name, hdr), name
    for name in ("Stacking", "ChainStacking", "stacking_weights", "wquantile", "device_stack_chains", "device_summary_stacked", "device_predict_stacked"):
        assert hasattr(bnr_amd, name), name


def _instance(n, K):
    rng = np.random.default_rng([16, n, K])
    return rng.normal(size=(n, K)) * 2.0 - 3.0 + rng.normal(size=(1, K))


def _f_and_g(lpd, w):
    """f(w) and the gradient g of the definition, in long double"""
    a = np.asarray(lpd, dtype=LD)
    mx = a.max(axis=1)
    p = np.exp(a - mx[:, None])
    d = p @ np.asarray(w, dtype=LD)
    return (mx + np.log(d)).sum() / a.shape[0], (p / d[:, None]).sum(axis=0) / a.shape[0]


@pytest.mark.parametrize("n,K", INSTANCES)
def test_solver_reaches_the_duality_bound(n, K):
    lpd = _instance(n, K)
    r = bnr_amd.stacking_weights(lpd, gap_tol=GAP_TOL)
    w = r["weights"]
    assert w.shape == (K,) and np.all(w >= 0) and abs(w.sum() - 1.0) <= 1e-12
    assert r["gap"] <= GAP_TOL and 0 <= r["iterations"] < 100000
    f, g = _f_and_g(lpd, w)
    print("n=%d K=%d: %d updates, gap %.3e, recomputed %.3e, objective %.15g" % (n, K, r["iterations"], r["gap"], float(g.max() - 1), r["objective"]))
    assert float(g.max() - 1) <= GAP_TOL + 1e-12
    assert abs(r["objective"] - float(f)) <= 1e-12 * max(1.0, abs(float(f)))
    ref = api._host_stacking_weights(lpd, max_iter=1000000, gap_tol=1e-12, dtype=LD)
    assert ref["gap"] <= 1e-12
    diff = float(ref["objective"] - LD(r["objective"]))
    assert -1e-12 * max(1.0, abs(float(f))) <= diff <= GAP_TOL, diff                # the duality bound (module docstring)
    h = api._host_stacking_weights(lpd, gap_tol=GAP_TOL)                            # the float64 restatement walks the same iteration
    assert h["iterations"] == r["iterations"] and np.max(np.abs(h["weights"] - w)) <= 1e-12


def test_known_answers():
    rng = np.random.default_rng(5)
    col = rng.normal(size=(30, 1))
    for K in (1, 2, 3, 7, 32):
        r = bnr_amd.stacking_weights(np.repeat(col, K, axis=1))
        assert r["iterations"] == 0 and np.array_equal(r["weights"], np.full(K, 1.0 / K)), K
    base = rng.normal(size=(40, 5))
    dom = base.copy()
    dom[:, 3] = base.max(axis=1) + 1.0                                              # column 3 dominates every row by 1.0
    r = bnr_amd.stacking_weights(dom)
    assert r["weights"][3] >= 1 - 1e-6 and r["gap"] <= 1e-9
    lpd = _instance(60, 6)                                                          # n >= K, distinct columns: strictly concave
    perm = np.array([4, 0, 5, 2, 1, 3])
    a, b = bnr_amd.stacking_weights(lpd, gap_tol=1e-13), bnr_amd.stacking_weights(lpd[:, perm], gap_tol=1e-13)
    assert a["gap"] <= 1e-13 and b["gap"] <= 1e-13
    assert np.max(np.abs(a["weights"][perm] - b["weights"])) <= 1e-9
    assert abs(a["objective"] - b["objective"]) <= 1e-12
    ninf = lpd.copy()
    ninf[3, :5] = -np.inf                                                           # -Inf entries are allowed while one entry of the row is finite
    r = bnr_amd.stacking_weights(ninf)
    assert r["gap"] <= 1e-9 and r["weights"][5] > 0 and np.isfinite(r["objective"])


def test_max_iter_is_not_an_error():
    lpd = _instance(40, 8)
    r = bnr_amd.stacking_weights(lpd, max_iter=1)
    assert r["iterations"] == 1 and r["gap"] > 1e-9 and abs(r["weights"].sum() - 1) <= 1e-12
    _f, g = _f_and_g(lpd, r["weights"])
    assert abs(float(g.max() - 1) - r["gap"]) <= 1e-12                              # the gap is that of the weights returned
    full = bnr_amd.stacking_weights(lpd)
    assert r["objective"] < full["objective"] <= r["objective"] + r["gap"]          # ... and bounds their distance from the optimum


def test_refusals():
    L = _capi.lib()
    good = np.ascontiguousarray(_instance(6, 3))
    w = np.empty(64)

    def call(n, K, a, max_iter=10, tol=1e-9):
        return L.bnr_stacking_weights(n, K, _capi._ptr(a), max_iter, tol, _capi._ptr(w), None, None, None)

    assert call(6, 3, good) == _capi.BNR_OK
    bad = []
    for v in (np.nan, np.inf):
        a = good.copy()
        a[2, 1] = v
        bad.append((6, 3, a, 10, 1e-9))
    a = good.copy()
    a[4, :] = -np.inf
    bad.append((6, 3, a, 10, 1e-9))
    bad += [(0, 3, good, 10, 1e-9), (6, 0, good, 10, 1e-9), (1, 33, np.zeros((1, 33)), 10, 1e-9), (6, 3, good, 0, 1e-9), (6, 3, good, 10, 0.0),
            (6, 3, good, 10, -1e-9), (6, 3, good, 10, np.inf), (6, 3, good, 10, np.nan)]
    for args in bad:
        assert call(*args) == _capi.BNR_ERR_BAD_ARG, args[:2] + args[3:]
        assert L.bnr_last_error()
    assert L.bnr_stacking_weights(6, 3, None, 10, 1e-9, _capi._ptr(w), None, None, None) == _capi.BNR_ERR_BAD_ARG
    for kw in (dict(max_iter=0), dict(gap_tol=0.0), dict(gap_tol=float("nan"))):
        with pytest.raises(ValueError):
            bnr_amd.stacking_weights(good, **kw)
        with pytest.raises(ValueError):
            api._host_stacking_weights(good, **kw)
    with pytest.raises(bnr_amd.BnrError):
        bnr_amd.stacking_weights(np.full((3, 2), np.nan))


# ------------------------------------------------------------------------------------------------------------------ the weighted quantile
def _key(v):
    """bnr_key_of of one double as a Python int"""
    if v != v:
        return 2 ** 64 - 1
    u = int(np.array([v], dtype=np.float64).view(np.uint64)[0])
    return (~u) & (2 ** 64 - 1) if u >> 63 else u | (1 << 63)


def scan_wquantile(row, w, K, r):
    """The definition, draw by draw: the draws sorted by key; at every draw x the counts c_k(x) of draws with key <= key(x), W(x) summed k
    ascending from 0.0 in float64, the first x with W(x) >= T = r / K; else the largest draw of the chains with w_k > 0"""
    ns = len(row) // K
    if any(v != v for v in row):
        return float("nan")
    items = sorted((_key(v), j // ns, v) for j, v in enumerate(row))
    T = float(r) / float(K)
    for key, _k, v in items:
        W = 0.0
        for k in range(K):
            c = sum(1 for kk, ch, _v in items if ch == k and kk <= key)
            W = W + w[k] * float(c)
        if W >= T:
            return v
    return max((it for it in items if w[it[1]] > 0), key=lambda it: it[0])[2]


def _tied(m, S, seed):
    rng = np.random.default_rng(seed)
    x = np.round(rng.normal(size=(m, S)) * 2) / 2
    x[0, : S // 2] = 0.0
    x[0, ::3] = -0.0
    return x


def _ranks(S):
    return sorted({1, min(2, S), max(1, int(round(0.025 * S))), int(round(0.975 * S)), max(1, S - 1), S})


@pytest.mark.parametrize("K", (1, 2, 4, 8))
@pytest.mark.parametrize("nsamp", (5, 64, 257))
def test_restatement_is_the_pooled_order_statistic_for_dyadic_uniform_weights(K, nsamp):
    S = K * nsamp
    x = _tied(3, S, [K, nsamp])
    srt = np.sort(x, axis=1)
    for r in _ranks(S):
        h = api._host_wquantile(x, np.full(K, 1.0 / K), K, r, S + 1 - r)
        assert np.array_equal(h["lower"], srt[:, r - 1]) and np.array_equal(h["upper"], srt[:, S - r]), (K, nsamp, r)


@pytest.mark.parametrize("K,nsamp", ((1, 7), (2, 5), (3, 11), (5, 4), (8, 3), (32, 2)))
def test_restatement_against_the_scan(K, nsamp):
    S = K * nsamp
    rng = np.random.default_rng([7, K, nsamp])
    x = _tied(4, S, [1, K, nsamp])
    x[1, rng.integers(S)] = np.inf
    x[1, rng.integers(S)] = -np.inf
    x[2, rng.integers(S)] = np.nan
    x[3] = 1.25
    ws = [np.full(K, 1.0 / K), rng.dirichlet(np.ones(K)), rng.dirichlet(np.full(K, 0.3))]
    if K > 1:
        z = rng.dirichlet(np.ones(K))
        z[K // 2] = 0.0
        ws.append(z / z.sum())
    ws += [np.eye(K)[k] for k in sorted({0, K // 2, K - 1})]
    for w in ws:
        for r in _ranks(S):
            h = api._host_wquantile(x, w, K, r, S + 1 - r)
            for i in range(x.shape[0]):
                for f, rr in (("lower", r), ("upper", S + 1 - r)):
                    want = scan_wquantile(list(x[i]), list(w), K, rr)
                    got = h[f][i]
                    assert (np.isnan(got) and want != want) or (got == want and np.signbit(got) == np.signbit(want)), (K, nsamp, r, i, f, got, want)
        seg = x.reshape(4, K, nsamp)
        with np.errstate(invalid="ignore"):
            want_mean = sum(w[k] * api._strided_mean(seg[:, k]) for k in range(K))
        assert np.allclose(h["mean"][[0, 3]], np.asarray(want_mean)[[0, 3]], rtol=1e-14, atol=0) and np.isnan(h["mean"][2])
    # w = e_k: chain k's ceil(T)-th smallest draw
    for k in range(K):
        for r in _ranks(S):
            h = api._host_wquantile(x[:1], np.eye(K)[k], K, r, r)
            assert h["lower"][0] == np.sort(x[0, k * nsamp:(k + 1) * nsamp])[int(np.ceil(r / K)) - 1], (K, k, r)


def test_restatement_refuses_bad_weights():
    x = np.zeros((2, 6))
    for w in ([0.5, 0.6], [1.5, -0.5], [0.0, 0.0], [np.nan, 1.0], [1.0], [0.5, 0.5 + 1e-8]):
        with pytest.raises(ValueError):
            api._host_wquantile(x, w, 2, 1, 6)
    with pytest.raises(ValueError):
        api._host_wquantile(x, [0.5, 0.5], 2, 0, 6)
    with pytest.raises(ValueError):
        api._host_wquantile(np.zeros((2, 7)), [0.5, 0.5], 2, 1, 6)
    api._host_wquantile(x, [0.5, 0.5 + 1e-10], 2, 1, 6)


# ------------------------------------------------------------------------------------------------------------------ plumbing
def test_stack_chains_is_refused_before_sampling(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("sampling started")
    monkeypatch.setattr(api, "ChainSet", boom)
    X, y, _ = bnr_amd.make_synthetic(8, 4, 2, seed=1)
    kw = dict(nburn=4, nsamples=8, x_transform=False, suppress_timer=True, filename=None, stack_chains=True)
    for nc in (1, 33):
        with pytest.raises(ValueError, match="stack_chains"):
            bnr_amd.Fit(X, y, 2, num_chains=nc, **kw)
    with pytest.raises(ValueError, match="stack_chains"):
        bnr_amd.generate_samples(X, y, 2, nburn=4, nsamp=8, x_transform=False, num_chains=1, stack_chains=True)
    with pytest.raises(ValueError, match="stack_chains"):
        bnr_amd.generate_samples_dbl(X, y, 2, mingen=8, maxgen=8, x_transform=False, num_chains=1, stack_chains=True)
    with pytest.raises(AssertionError, match="sampling started"):                   # two chains pass the check
        bnr_amd.Fit(X, y, 2, num_chains=2, **kw)


def _tables(X, y, K, tot, seed):
    """K hand-made state tables around a least-squares fit of (X, y): chain c's gamma shifted by 0.3 c"""
    n, q = X.shape
    beta = np.linalg.lstsq(np.c_[np.ones(n), X], y, rcond=None)[0]
    out = []
    for c in range(K):
        rng = np.random.default_rng([seed, c])
        t = dict(gamma=np.asfortranarray((beta[1:] + 0.3 * c + 0.05 * rng.normal(size=(tot, q))).reshape(tot, q, 1)),
                 mu=np.asfortranarray((beta[0] + 0.05 * rng.normal(size=tot)).reshape(tot, 1, 1)),
                 tau2=np.asfortranarray(np.exp(0.1 * rng.normal(size=tot)).reshape(tot, 1, 1)),
                 xi=np.asfortranarray((rng.random((tot, 4)) < 0.5).astype(np.float64).reshape(tot, 4, 1)))
        out.append(t)
    return out


def test_stacking_of_results_holding_tables():
    rng = np.random.default_rng(3)
    X = rng.normal(size=(12, 10))
    y = X[:, 0] - 0.5 * X[:, 3] + 0.1 * rng.normal(size=12)
    tabs = _tables(X, y, 3, 60, 9)
    res = bnr_amd.Results(tabs, None, None, 10, 50)
    got = bnr_amd.Stacking(res, X, y, x_transform=False)
    want = api._host_stack_chains(tabs, X, y, 10, 50)
    assert isinstance(got, bnr_amd.ChainStacking) and (got.chains, got.draws, got.n_used) == (3, 150, 12)
    for f in ("weights", "elpd_chain", "elpd_chain_i", "pareto_k", "n_high_k", "elpd_stack_i"):
        assert np.array_equal(getattr(got, f), getattr(want, f), equal_nan=True), f
    assert (got.elpd_stack, got.se, got.elpd_uniform, got.gap, got.iterations) == (want.elpd_stack, want.se, want.elpd_uniform, want.gap, want.iterations)
    assert abs(got.weights.sum() - 1) <= 1e-12 and got.gap <= 1e-9 and got.weights[0] > got.weights[2]      # the shifted chains fit worse
    slack = 12 * got.gap + 1e-12                                                    # f is the mean over the 12 rows: the gap bounds f, the totals 12 times that
    assert got.elpd_stack >= got.elpd_uniform - slack and got.elpd_stack >= got.elpd_chain.max() - slack
    for k in range(3):                                                              # every chain's numbers are its own PSIS-LOO
        _l, e, kh = api._psis_host(api._host_loglik(tabs[k], X, y, 10, 50))
        assert np.array_equal(got.elpd_chain_i[k], e) and np.array_equal(got.pareto_k[k], kh)
    r = api._host_stacking_weights(got.elpd_chain_i.T)
    assert np.array_equal(r["weights"], got.weights)
    # the fit's own numbers win; one table is refused
    marked = bnr_amd.Results(None, None, None, 10, 50, stacking=want)
    assert bnr_amd.Stacking(marked) is want
    with pytest.raises(ValueError):
        bnr_amd.Stacking(bnr_amd.Results(tabs[0], None, None, 10, 50), X, y, x_transform=False)
    # summaries under the weights from the tables
    s = api._host_summary_stacked(tabs, got.weights, 10, 50)
    one = api._host_summary_stacked(tabs, [1.0, 0.0, 0.0], 10, 50)
    g0 = tabs[0]["gamma"][10:60, :, 0]
    assert np.array_equal(one["estimate"], api._strided_mean(g0.T)) and s["estimate"].shape == (10,) and s["probability"].shape == (4,)
    assert np.all(s["lower_bound"] <= s["upper_bound"])
    p = api._host_predict_stacked(tabs, got.weights, X[:5], y[:5], 10, 50, pred_seed=4)
    assert p.estimate.shape == (5,) and np.all(p.lower_bound <= p.upper_bound) and np.all(p.pred_lower_bound <= p.lower_bound) and p.draws == 150
    assert np.isfinite(p.lpd).all() and p.elpd == float(np.sum(p.lpd))


def test_k_wsummary_sits_behind_the_sweep(tmp_path):
    """k_wsummary is declared last in csrc/bnr_kernels.h, as k_summary's companion, and instantiated last in csrc/bnr_hip.hip: its two instances
    are in the sweep's code object at addresses above every other kernel there (whose order and sizes are therefore what they were), none is
    in the analysis one, whose kernels are what they were"""
    assert os.path.exists(co.LIB), "libbnr_hip.so has not been built"
    if not co.have_tools():
        pytest.skip("no ROCm LLVM tools here")
    sweep, analysis = co.sweep_and_analysis(tmp_path)
    mine = sorted(k for k in sweep if k.startswith("k_wsummary"))
    assert mine == ["k_wsummary<10>", "k_wsummary<8>"] and "k_summary" in sweep
    assert not [k for k in analysis if k.startswith(("k_wsummary", "k_wpred", "k_summary"))] and co.ANALYSIS <= set(analysis)
    src = open(os.path.join(ROOT, "bayesiannetworkregression.jl_amd", "csrc", "bnr_kernels.h")).read()
    declared = re.findall(r"__global__\s+(?:__launch_bounds__\([^)]*\)\s+)?void\s+(k_\w+)\s*\(", src)
    assert declared[-1] == "k_wsummary" and {re.sub(r"<.*", "", k) for k in sweep} == set(declared)
    assert min(sweep[k][0] for k in mine) > max(v[0] for k, v in sweep.items() if k not in mine)
