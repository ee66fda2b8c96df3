"""CPU tests of the posterior covariance of the edge coefficients (ABI 17): the ABI and its exports, the place of k_cov in the code objects, the
numpy restatement api._host_cov / _host_edge_cov against the exact arithmetic of tests/cov_ref.py, a hand-computed example of the derived values,
the parsing of Fit's keyword, the accessor's refusal and the library's refusals that return before any device work.  No GPU."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import bnr_amd
import code_objects as co
import cov_ref as cr
from bnr_amd import _capi, api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("bnr_chain_cov", "bnr_chains_cov", "bnr_cov")


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def test_abi_version_and_exports():
    hdr = open(os.path.join(ROOT, "include", "bnr_hip.h")).read()
    ver = int(re.search(r"#define BNR_ABI_VERSION (\d+)", hdr).group(1))
    L = _capi.lib()
    assert ver >= 17 and L.bnr_abi_version() == ver
    for name in NAMES:
        assert name in bnr_amd.EXPORTS and getattr(L, name) is not None and re.search(r"\bint %s\(" % name, hdr), name
    assert '"cov_block_cols"' in hdr
    for name in ("EdgeCov", "cov", "device_edge_cov"):
        assert hasattr(bnr_amd, name), name
    shim = open(os.path.join(ROOT, "julia", "BNRHip.jl")).read()
    assert "function edge_cov(" in shim and ":bnr_chains_cov" in shim


def _kernels_named(co_file, name):
    """the demangled FUNC symbols of a code object whose name contains `name`, namespaces included (code_objects.code_objects lists the
    global-scope k_* kernels alone)"""
    syms = subprocess.run([os.path.join(co.LLVM, "llvm-readelf"), "-sW", str(co_file)], check=True, stdout=subprocess.PIPE, text=True).stdout
    names = subprocess.run(["c++filt"], input=syms, check=True, stdout=subprocess.PIPE, text=True).stdout
    out = set()
    for line in names.splitlines():
        m = re.match(r"\s*\d+:\s+[0-9a-f]+\s+\d+\s+FUNC\s+\S+\s+\S+\s+\S+\s+(?:void )?([\w:]*%s\w*(?:<[^>]*>)?)\(" % re.escape(name), line)
        if m:
            out.add(m.group(1))
    return out


def test_k_cov_lives_in_the_analysis_code_object(tmp_path):
    if not (co.have_tools() and os.path.exists(co.LIB)):
        pytest.skip("no ROCm LLVM tools / no built library here")
    sweep, analysis = co.sweep_and_analysis(tmp_path)                            # (leaves co0.o and co1.o, the two code objects, in tmp_path)
    files = [tmp_path / "co0.o", tmp_path / "co1.o"]
    is_sweep = [bool(_kernels_named(f, "k_chol_step")) for f in files]
    assert sorted(is_sweep) == [False, True]
    mine = _kernels_named(files[is_sweep.index(False)], "k_cov")
    assert mine == {"k_cov<2>", "k_cov<4>", "k_cov_finish"}, mine                # at global scope, like every other kernel
    assert not _kernels_named(files[is_sweep.index(True)], "k_cov")
    assert {k for k in analysis if "k_cov" in k} == mine and mine <= co.ANALYSIS and not [k for k in sweep if "k_cov" in k]
    src = open(os.path.join(ROOT, "bayesiannetworkregression.jl_amd", "csrc", "bnr_kernels.h")).read()
    assert "k_cov" not in src


# ------------------------------------------------------------------------------------------------------------------ the restatement is exact
def _check_exact(x, w, what):
    c, _G, cov = cr.exact(x, w)
    mean, got = api._host_cov(x, w)
    assert same_bits(mean, cr.as_float(c)) and same_bits(got, cr.as_float(cov)), what
    assert same_bits(got, got.T), what


def test_host_cov_equals_the_exact_reference_on_integer_draws():
    for K, ns, m, w in cr.integer_cases():
        if m == 33 and ns in (63, 65) and K == 3:
            continue                                                         # (the GPU test runs every case; here the largest cost a second each)
        x = cr.integer_case(K, ns, m, w)
        assert np.all(np.abs(x) <= 1024) and np.all(x == np.round(x))
        c = cr.exact(x, w)[0]
        assert all(v.denominator == 1 for v in c), (K, ns, m, w)
        _check_exact(x, w, (K, ns, m, w))


def test_host_cov_of_shifted_columns_is_the_same_bits():
    for K, ns, m, w in ((1, 5, 15, None), (2, 63, 17, None), (3, 64, 16, (0.5, 0.25, 0.25)), (2, 64, 17, (1.0, 0.0))):
        x = cr.integer_case(K, ns, m, w, seed=1)
        shift = np.where(np.arange(m) % 3 == 1, 1e8, 0.0)
        m0, c0 = api._host_cov(x, w)
        m1, c1 = api._host_cov(x + shift, w)
        assert same_bits(c0, c1) and same_bits(m1, m0 + shift), (K, ns, m, w)
        _check_exact(x + shift, w, (K, ns, m, w, "shifted"))


def _table(x):
    """one table per chain with the draws x[k] as its gamma rows, behind 3 rows that must not be read"""
    K, ns, q = x.shape
    pad = np.full((3, q), 7e7)
    return [dict(gamma=np.asfortranarray(np.concatenate([pad, x[k], pad])[:, :, None])) for k in range(K)]


def test_host_edge_cov_on_tables():
    V = 8
    q = V * (V + 1) // 2
    for K, ns, w in ((1, 5, None), (3, 64, None), (3, 64, (0.5, 0.25, 0.25))):
        x = cr.integer_case(K, ns, q, w, seed=2)
        full = api._host_edge_cov(_table(x), 3, ns, weights=w)
        c, _G, cov = cr.exact(x, w)
        assert same_bits(full.mean, cr.as_float(c)) and same_bits(full.cov, cr.as_float(cov))
        assert (full.chains, full.draws) == (K, K * ns) and np.array_equal(full.cols, np.arange(q))
        assert (full.weights is None) if w is None else np.array_equal(full.weights, w)
        assert np.array_equal(full.node1[:V], np.ones(V)) and np.array_equal(full.node2[:V], np.arange(1, V + 1)) and (full.node1[-1], full.node2[-1]) == (V, V)
        for e in (0, 5, 8, 20, q - 1):
            assert _capi.lib().bnr_host_edge_index(V, int(full.node2[e]) - 1, int(full.node1[e]) - 1) == e
        cols = [20, 3, 35, 3, 0]                                             # a subset, permuted, with a duplicate
        sub = api._host_edge_cov(_table(x), 3, ns, cols=cols, weights=w)
        assert same_bits(sub.cov, full.cov[np.ix_(cols, cols)]) and same_bits(sub.mean, full.mean[cols]) and np.array_equal(sub.cols, cols)
    with pytest.raises(ValueError):
        api._host_edge_cov(_table(x), 3, ns, cols=[q])
    with pytest.raises(ValueError):
        api._host_edge_cov(_table(x[:1, :1]), 3, 1)
    with pytest.raises(ValueError):
        api._host_edge_cov(_table(x), 3, ns, weights=[0.5, 0.25, 0.3])


def test_non_finite_columns_of_the_restatement():
    rng = np.random.default_rng(3)
    x = rng.standard_normal((2, 9, 5))
    clean = api._host_cov(x)[1]
    x[1, 4, 1] = np.nan
    x[0, 2, 3] = np.inf
    got = api._host_cov(x)[1]
    bad = np.zeros((5, 5), dtype=bool)
    bad[[1, 3], :] = True
    bad[:, [1, 3]] = True
    assert np.isnan(got[bad]).all() and same_bits(got[~bad], clean[~bad])


# ------------------------------------------------------------------------------------------------------------------ the derived values, by hand
def _hand():
    # draws: a = 1 3 5 7 (mean 4, deviations -3 -1 1 3), b = 2 2 2 2, c = 0 4 0 4 (mean 2, deviations -2 2 -2 2)
    x = np.array([[1.0, 2.0, 0.0], [3.0, 2.0, 4.0], [5.0, 2.0, 0.0], [7.0, 2.0, 4.0]])
    mean, cov = api._host_cov(x[None])
    return api.EdgeCov(cols=np.array([0, 1, 2]), node1=np.array([1, 1, 1]), node2=np.array([1, 2, 3]), mean=mean, cov=cov, chains=1, draws=4, weights=None)


def test_hand_computed_example():
    ec = _hand()
    assert np.array_equal(ec.mean, [4.0, 2.0, 2.0])
    assert np.array_equal(ec.cov, np.array([[20.0, 0.0, 8.0], [0.0, 0.0, 0.0], [8.0, 0.0, 16.0]]) / 3.0)       # (20 = 9+1+1+9, 8 = 6-2-2+6, 16 = 4 x 4)
    assert np.allclose(ec.sd, [math.sqrt(20 / 3), 0.0, math.sqrt(16 / 3)], rtol=1e-15, atol=0)
    r = ec.corr
    assert np.isnan(r[1, :]).all() and np.isnan(r[:, 1]).all()                   # the constant column: sd 0
    assert abs(r[0, 0] - 1) <= 1e-15 and abs(r[2, 2] - 1) <= 1e-15 and abs(r[0, 2] - 1 / math.sqrt(5)) <= 1e-15 and r[0, 2] == r[2, 0]
    ct = ec.contrast([[1, 0, 1], [1, 0, -1], [0, 1, 0]])
    assert np.array_equal(ct["mean"], [6.0, 2.0, 2.0])
    assert np.allclose(ct["sd"], [math.sqrt(52 / 3), math.sqrt(20 / 3), 0.0], rtol=1e-15, atol=0)               # 20/3 + 16/3 +- 2 x 8/3
    one = ec.contrast([1, 0, 1])
    assert one["mean"].shape == (1,) and one["sd"][0] == ct["sd"][0]
    with pytest.raises(ValueError):
        ec.contrast([1, 1])
    tp = ec.top_pairs(5)
    assert len(tp) == 1 and tp[0][:2] == (0, 2) and abs(tp[0][2] - 1 / math.sqrt(5)) <= 1e-15                   # the pairs with b have no correlation
    assert ec.top_pairs(0) == []


def test_top_pairs_order_and_ties():
    a = np.array([1.0, 3.0, 5.0, 7.0])
    c = np.array([0.0, 4.0, 0.0, 4.0])
    a2 = np.array([1.0, 3.0, 5.0, 8.0])                                      # 3 var = 26.75, 3 cov(a, a2) = 23, 3 cov(c, a2) = 10
    x = np.stack([a, c, -a2, c], axis=1)
    # |corr|: (1,3) 1; (0,2) 23 / sqrt(20 x 26.75) = 0.994; (1,2) and (2,3) 10 / sqrt(16 x 26.75) = 0.483, the same numbers: a tie, by index;
    # (0,1) and (0,3) 8 / sqrt(20 x 16) = 0.447, a tie again
    mean, cov = api._host_cov(x[None])
    ec = api.EdgeCov(cols=np.arange(4), node1=np.ones(4, dtype=int), node2=np.arange(1, 5), mean=mean, cov=cov, chains=1, draws=4, weights=None)
    tp = ec.top_pairs(10)
    assert [t[:2] for t in tp] == [(1, 3), (0, 2), (1, 2), (2, 3), (0, 1), (0, 3)]
    want = [1.0, -23 / math.sqrt(20 * 26.75), -10 / math.sqrt(16 * 26.75), -10 / math.sqrt(16 * 26.75), 1 / math.sqrt(5), 1 / math.sqrt(5)]
    assert np.allclose([t[2] for t in tp], want, rtol=1e-14, atol=0) and tp[2][2] == tp[3][2] and tp[4][2] == tp[5][2]
    assert [t[:2] for t in ec.top_pairs(3)] == [(1, 3), (0, 2), (1, 2)]


# ------------------------------------------------------------------------------------------------------------------ the keyword and the accessor
def test_keyword_parsing():
    V = 4                                                                    # q = 10; edges in Summary's order: (1,1) (1,2) (1,3) (1,4) (2,2) ...
    assert api._edge_cov_cols(False) is None and api._edge_cov_cols(None) is None and api._edge_cov_cols(True, V) == "all"
    got = api._edge_cov_cols([9, 0, 4, 4], V)
    assert got.dtype == np.int32 and np.array_equal(got, [9, 0, 4, 4])
    assert np.array_equal(api._edge_cov_cols(np.array([2.0, 7.0]), V), [2, 7])
    pairs = api._edge_cov_cols([(1, 2), (3, 1), (4, 4), (2, 2)], V)
    assert np.array_equal(pairs, [1, 2, 9, 4])
    L = _capi.lib()
    for (a, b), e in zip([(1, 2), (3, 1), (4, 4), (2, 2)], pairs):
        assert L.bnr_host_edge_index(V, a - 1, b - 1) == e
    for bad in ("all", 3, 2.5, [], [[1, 2, 3]], [0.5, 1], [-1, 2], [10], [(0, 1)], [(1, 5)], {"a": 1}, [True, False], np.zeros((2, 2, 2))):
        with pytest.raises(ValueError):
            api._edge_cov_cols(bad, V)
    # Fit's first check (no X yet) refuses what can be refused without V, before anything is sampled or written
    y = np.zeros(5)
    for bad in ("all", [], [-1], [(0, 1)], 7):
        with pytest.raises(ValueError):
            api._fit_requests(y, 2, edge_cov=bad)
    req = api._fit_requests(y, 2, X_new=_capi.XInput(np.zeros((5, 10))), nsamp=10, x_transform=False, edge_cov=[(1, 2), (2, 1)])
    assert np.array_equal(req.edge_cov, [1, 1])
    assert api._fit_requests(y, 2).edge_cov is None and api._fit_requests(y, 2, edge_cov=True).edge_cov == "all"
    import inspect
    for fn in (bnr_amd.Fit, bnr_amd.generate_samples, bnr_amd.generate_samples_dbl):
        assert inspect.signature(fn).parameters["edge_cov"].default is False, fn


def test_accessor():
    res = bnr_amd.Results(None, np.ones(3), np.ones(6), 2, 5)
    assert res.edge_cov is None
    with pytest.raises(ValueError, match="edge_cov"):
        bnr_amd.EdgeCov(res)
    rng = np.random.default_rng(5)
    res.state = dict(gamma=np.asfortranarray(rng.standard_normal((7, 6, 1))))
    ec = bnr_amd.EdgeCov(res)                                                # the host fallback: chain 1's table, rows 3 .. 7
    assert isinstance(ec, bnr_amd.EdgeCov) and (ec.chains, ec.draws) == (1, 5) and ec.weights is None
    assert np.allclose(ec.cov, np.cov(res.state["gamma"][2:7, :, 0].T), rtol=1e-13, atol=1e-15)
    res.edge_cov = _hand()
    assert bnr_amd.EdgeCov(res) is res.edge_cov
    with pytest.raises(TypeError):
        api.EdgeCov(cols=np.arange(2))


# ------------------------------------------------------------------------------------------------------------------ refusals before any device work
def test_refusals_that_need_no_device():
    L = _capi.lib()
    x = np.arange(12.0).reshape(4, 3)
    mean, cov = np.empty(3), np.empty((3, 3))
    p = _capi._ptr

    def refused(code):
        assert code == _capi.BNR_ERR_BAD_ARG, code
        return L.bnr_last_error().decode()

    refused(L.bnr_cov(0, 1, 4, 3, None, None, p(mean), p(cov)))
    refused(L.bnr_cov(0, 1, 4, 3, p(x), None, None, p(cov)))
    refused(L.bnr_cov(0, 1, 4, 3, p(x), None, p(mean), None))
    for K, ns, m in ((0, 4, 3), (1, 0, 3), (1, 4, 0), (-1, 4, 3)):
        refused(L.bnr_cov(0, K, ns, m, p(x), None, p(mean), p(cov)))
    assert "2 draws" in refused(L.bnr_cov(0, 1, 1, 3, p(x), None, p(mean), p(cov)))                               # S = 1
    for bad in ([0.5, 0.3], [1.5, -0.5], [0.0, 0.0], [np.nan, 0.5], [0.5, 0.5 + 1e-8]):
        w = np.array(bad)
        refused(L.bnr_cov(0, 2, 2, 3, p(x), p(w), p(mean), p(cov)))
    w33 = np.full(33, 1 / 33)
    big = np.zeros((66, 1))
    refused(L.bnr_cov(0, 33, 2, 1, p(big), p(w33), p(mean), p(cov)))                                              # more chains than a weighted call takes
    refused(L.bnr_chains_cov(None, 1, None, 1, 4, 3, None, p(mean), p(cov)))
    refused(L.bnr_chain_cov(None, 1, 4, 3, None, p(mean), p(cov)))
    # the Python layer refuses the same before it reaches the library
    for bad in (np.zeros(5), np.zeros((1, 3)), np.zeros((5, 3))):
        with pytest.raises(ValueError):
            _capi.cov_raw(bad, 2 if bad.shape[0] == 5 else 1)
    with pytest.raises(ValueError):
        _capi.cov_raw(x, 2, weights=[1.0])
    for bad in ([], [0.5], [-1], [6], [[0, 1]], [True]):
        with pytest.raises(ValueError):
            _capi.cov_cols(bad, 6)
    assert _capi.cov_cols(None, 6) is None and _capi.cov_cols([5, 0, 5], 6).dtype == np.int32
