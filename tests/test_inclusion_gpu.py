"""GPU tests of the joint posterior of the node indicators (ABI 15; run with -m gpu on an MI355X): the three k_incl_* kernels alone
(bnr_inclusion against the numpy restatement api._host_inclusion, itself pinned to the brute force of tests/incl_ref.py by
tests/test_inclusion_host.py), bnr_chains_inclusion / bnr_chain_inclusion through device_node_sets against the restatement over the fetched
tables, the bitwise properties, the refusals and Fit(..., node_sets=True).

Every comparison is of bits or integers: every result is an integer count, divided once by S in double on both sides; no tolerance exists.

Chains as in test_hdi_gpu.py: three Chains of n = 8, V = 16, R = 2 with 640-row tables, never run; tables come in by Chain.load.  A second pair
has V = 70 (two pattern words), R = 3 and 130-row tables."""
import ctypes as C

import numpy as np
import pytest

import bnr_amd
import diag_ref as dr
import incl_ref as ir
import rank_diag_cases as rc
from bnr_amd import _capi, api

pytestmark = pytest.mark.gpu
NS_ARRAYS = ("prob_nodes", "co_inclusion", "size_pmf", "top_prob", "map_model", "median_model", "prob_active", "dim_pmf")
V2, R2, TOT2 = 70, 3, 130
WINDOWS2 = ((1, 130), (3, 101), (1, 9), (66, 65))
PAIR = (5, 9)                                                               # 0-based nodes that are never selected together


def _tables(V, R, tot, nch, seed):
    """zero tables with a fresh xi column -- Bernoulli draws, node PAIR[1] only where node PAIR[0] is out -- and lambda over {0, 1, -1}"""
    tabs = []
    for c in range(nch):
        rng = np.random.default_rng([seed, V, c])
        t = dr.new_table(tot, V, R)
        xi = (rng.random((tot, V)) < 0.1 + 0.8 * np.arange(V) / V).astype(np.float64)
        xi[:, PAIR[1]] = (rng.random(tot) < 0.6) & (xi[:, PAIR[0]] == 0)
        t["xi"][:, :, 0] = xi
        t["lam"][:, :, 0] = rng.integers(-1, 2, size=(tot, R)).astype(np.float64)
        tabs.append(t)
    return tabs


@pytest.fixture(scope="module")
def chains(gpu):
    X, y, _ = bnr_amd.make_synthetic(dr.N, dr.V, dr.R, seed=3)
    cs = [bnr_amd.Chain(X, y, dr.R, dr.TOT, 99, 1, device=gpu)]
    cs += [bnr_amd.Chain.like(cs[0], 99, c) for c in (2, 3)]
    yield cs
    for c in cs:
        c.close()


@pytest.fixture(scope="module")
def wide_chains(gpu):
    X, y, _ = bnr_amd.make_synthetic(dr.N, V2, R2, seed=4)
    cs = [bnr_amd.Chain(X, y, R2, TOT2, 98, 1, device=gpu)]
    cs.append(bnr_amd.Chain.like(cs[0], 98, 2))
    yield cs
    for c in cs:
        c.close()


def _load(chains, tabs):
    for ch, t in zip(chains, tabs):
        ch.load(t)


# ------------------------------------------------------------------------------------------------------------------ the kernels alone
def _check(z, ntop, gpu, what):
    want = api._host_inclusion(z, ntop)
    got = _capi.inclusion_raw(z, ntop, gpu)
    ir.same(got, want, (what, ntop))
    return dict(zip(ir.FIELDS, got))


@pytest.mark.parametrize("S", ir.S_GRID)
def test_kernels_against_the_restatement(gpu, S):
    for what, z in ir.grid_cases():
        if what[1] != S:
            continue
        for ntop in ir.NTOPS:
            full = _check(z, ntop, gpu, what)
            assert np.all(np.diff(full["top_count"]) <= 0) and full["top_count"].sum() <= S
            assert not full["top_sets"][full["n_distinct"]:].any() and not full["top_count"][full["n_distinct"]:].any()     # the padding is zeros
        # each output alone (every other pointer NULL; the top sets come as a pair) is the same bits
        for fields in (("prob",), ("joint",), ("size_pmf",), ("n_distinct",), ("top_sets", "top_count")):
            one = _capi.inclusion_raw(z, ntop, gpu, fields=fields)
            assert all((a is None) == (f not in fields) for f, a in zip(ir.FIELDS, one)), (what, fields)
            ir.same(one, full, (what, fields), fields)
        counts = full["size_pmf"] * S                                       # the sizes: integer counts that sum to S, shares that sum to 1
        assert np.array_equal(counts, np.rint(counts)) and counts.sum() == S and abs(full["size_pmf"].sum() - 1.0) <= (z.shape[1] + 1) * 2.0 ** -53
        assert np.array_equal(np.diag(full["joint"]), full["prob"]) and np.array_equal(full["joint"], full["joint"].T)


def test_kernels_indices_past_16_bits(gpu):
    z = ir.long_matrix()
    for ntop in (1, 256):
        got = _check(z, ntop, gpu, "long")
    assert got["n_distinct"] == 8 and got["top_count"][:8].sum() == z.shape[0] and got["top_count"][0] > 4096      # long runs


def test_kernels_constant_matrices_and_the_public_function(gpu):
    for v, B in ((0, 70), (1, 70), (1, 64), (0, 1)):
        z = np.full((257, B), v, dtype=np.uint8)
        got = _check(z, 4, gpu, ("constant", v, B))
        assert got["n_distinct"] == 1 and got["top_count"].tolist() == [257, 0, 0, 0] and got["size_pmf"][v * B] == 1.0
    z = ir.bernoulli(257, 65)
    out = bnr_amd.inclusion(z, ntop=3, device=gpu)
    ir.same(out, api._host_inclusion(z, 3), "inclusion")
    few = bnr_amd.inclusion(z.astype(np.float64) * -2.5, ntop=0, device=gpu)   # any number != 0 is 1; no rows asked for
    assert sorted(few) == ["joint", "n_distinct", "prob", "size_pmf"] and np.array_equal(few["joint"], out["joint"]) and few["n_distinct"] == out["n_distinct"]


# ------------------------------------------------------------------------------------------------------------------ chains against the restatement
def _compare_node_sets(got, want, what):
    for f in NS_ARRAYS:
        g, w = np.asarray(getattr(got, f)), np.asarray(getattr(want, f))
        assert g.shape == w.shape and np.array_equal(g.view(np.uint64) if g.dtype == np.float64 else g, w.view(np.uint64) if w.dtype == np.float64 else w), (what, f)
    assert [s.tolist() for s in got.top_sets] == [s.tolist() for s in want.top_sets], what
    assert (got.n_distinct, got.size_mean, got.size_mode, got.dim_mean, got.chains, got.draws) == \
        (want.n_distinct, want.size_mean, want.size_mode, want.dim_mean, want.chains, want.draws), what


@pytest.mark.parametrize("first,nsamp,_lag", rc.WINDOWS)
def test_device_against_the_restatement(chains, first, nsamp, _lag):
    tabs = _tables(dr.V, dr.R, dr.TOT, 3, seed=21)
    _load(chains, tabs)
    fetched = [ch.fetch() for ch in chains]
    for nch in (3, 1):
        for ntop in (10, 256):
            got = api.device_node_sets(chains[:nch], first - 1, nsamp, ntop)
            want = api._host_node_sets(fetched[:nch], first - 1, nsamp, ntop)
            _compare_node_sets(got, want, (nch, first, nsamp, ntop))
            assert (got.chains, got.draws) == (nch, nch * nsamp) and got.co_inclusion.shape == (dr.V, dr.V) and got.dim_pmf.shape == (dr.R + 1,)
        assert got.co_inclusion[PAIR] == 0.0 and got.co_inclusion[PAIR[::-1]] == 0.0                 # the planted pair: one instead of the other
        assert nsamp < 100 or (got.prob_nodes[PAIR[0]] > 0 and got.prob_nodes[PAIR[1]] > 0)
    _compare_node_sets(api.device_node_sets(chains, first - 1, nsamp), api._host_node_sets(tabs, first - 1, nsamp), "the tables as they were loaded")


@pytest.mark.parametrize("first,nsamp", WINDOWS2)
def test_device_against_the_restatement_with_two_pattern_words(wide_chains, first, nsamp):
    _load(wide_chains, _tables(V2, R2, TOT2, 2, seed=22))
    fetched = [ch.fetch() for ch in wide_chains]
    for nch in (2, 1):
        got = api.device_node_sets(wide_chains[:nch], first - 1, nsamp, 7)
        _compare_node_sets(got, api._host_node_sets(fetched[:nch], first - 1, nsamp, 7), (nch, first, nsamp))
        assert got.co_inclusion.shape == (V2, V2) and got.co_inclusion[PAIR] == 0.0 and got.dim_pmf.shape == (R2 + 1,)
        assert any(s.size and s.max() > 64 for s in got.top_sets)                # nodes of the second word


# ------------------------------------------------------------------------------------------------------------------ bitwise properties
def test_bitwise_properties(chains):
    _load(chains, _tables(dr.V, dr.R, dr.TOT, 3, seed=23))
    first, nsamp = 38, 601
    S = 3 * nsamp
    before = [ch.fetch() for ch in chains]
    iters = [ch.iter for ch in chains]
    base = _capi.pooled_inclusion(chains, first, nsamp, 0, 8)
    hdi = _capi.pooled_hdi(chains, first, nsamp, 0.9)
    again = _capi.pooled_inclusion(chains, first, nsamp, 0, 8)              # a repeated call, with an HDI call in between
    ir.same(again, dict(zip(ir.FIELDS, base)), "repeated")
    prob, joint, size_pmf, n_distinct, top_sets, top_count = base
    _mean, _lo, _up, prob_xi = _capi.pooled_summary(chains, first, nsamp, *api._summary_ranks(S, 95))
    assert np.array_equal(prob.view(np.uint64), prob_xi.view(np.uint64))       # three exact counts over S
    assert np.array_equal(prob.view(np.uint64), hdi[3][dr.Q:].view(np.uint64))
    assert np.array_equal(np.diag(joint), prob) and np.array_equal(joint, joint.T)
    counts = size_pmf * S
    assert np.array_equal(counts, np.rint(counts)) and counts.sum() == S and abs(size_pmf.sum() - 1.0) <= (dr.V + 1) * 2.0 ** -53
    assert np.all(np.diff(top_count) <= 0) and top_count.sum() <= S and 8 <= n_distinct <= S
    assert joint[PAIR] == 0.0 and prob[PAIR[0]] > 0 and prob[PAIR[1]] > 0      # the planted pair: one instead of the other
    for fields in (("prob",), ("joint",), ("size_pmf",), ("n_distinct",), ("top_sets", "top_count")):      # the outputs requested
        one = _capi.pooled_inclusion(chains, first, nsamp, 0, 8, fields=fields)
        assert all((a is None) == (f not in fields) for f, a in zip(ir.FIELDS, one)), fields
        ir.same(one, dict(zip(ir.FIELDS, base)), fields, fields)
    for which in (0, 1):                                                      # the single-chain entry point is the pooled call with one chain
        one = chains[1].inclusion(first, nsamp, which, 4)
        ir.same(one, dict(zip(ir.FIELDS, _capi.pooled_inclusion([chains[1]], first, nsamp, which, 4))), ("one chain", which))
        z = before[1]["lam" if which else "xi"][first - 1:first - 1 + nsamp, :, 0]
        ir.same(one, api._host_inclusion(z, 4), ("one chain against the restatement", which))
    for ch, b, it in zip(chains, before, iters):                              # nothing of any chain is written
        after = ch.fetch()
        assert ch.iter == it
        for k in b:
            assert np.array_equal(b[k].view(np.uint64), after[k].view(np.uint64)), k


def test_a_nan_counts_as_included(chains):
    first, nsamp, row, node = 38, 601, 300, 3
    res = {}
    for name, v in (("nan", dr.NAN_NEG), ("one", 1.0), ("zero", 0.0), ("minus zero", -0.0)):
        tabs = _tables(dr.V, dr.R, dr.TOT, 3, seed=24)
        tabs[1]["xi"][row, node, 0] = v
        _load(chains, tabs)
        res[name] = dict(zip(ir.FIELDS, _capi.pooled_inclusion(chains, first, nsamp, 0, 6)))
    ir.same(res["nan"], res["one"], "a NaN is a 1")
    ir.same(res["minus zero"], res["zero"], "-0 is a 0")
    others = np.arange(dr.V) != node
    assert np.array_equal(res["nan"]["prob"][others], res["zero"]["prob"][others])
    assert np.rint(res["nan"]["prob"][node] * 3 * nsamp) == np.rint(res["zero"]["prob"][node] * 3 * nsamp) + 1
    assert np.array_equal(res["nan"]["joint"][np.ix_(others, others)], res["zero"]["joint"][np.ix_(others, others)])


# ------------------------------------------------------------------------------------------------------------------ refusals
def _raw_pooled(chains, first_row, nsamp, which, ntop, outs):
    """bnr_chains_inclusion as the library takes it: no check of the binding in front"""
    arr = (C.c_void_p * len(chains))(*[ch.h for ch in chains])
    return chains[0].L.bnr_chains_inclusion(arr, len(chains), first_row, nsamp, which, ntop, *[_capi._ptr(o) for o in outs])


def test_refusals(chains):
    _load(chains, _tables(dr.V, dr.R, dr.TOT, 3, seed=25))
    bad = [dict(first_row=600, nsamp=100), dict(first_row=0, nsamp=100), dict(first_row=1, nsamp=0)]
    for kw in bad:
        for call in (lambda: _capi.pooled_inclusion(chains, which=0, ntop=2, **kw), lambda: chains[0].inclusion(which=0, ntop=2, **kw)):
            with pytest.raises(bnr_amd.BnrError) as e:
                call()
            assert e.value.code == _capi.BNR_ERR_BAD_ARG, kw
    for call in (lambda: _capi.pooled_inclusion([chains[0], chains[1], chains[0]], 1, 640, 0, 2), lambda: _capi.pooled_inclusion(chains, 1, 640, 2, 2),
                 lambda: chains[0].inclusion(1, 640, -1, 2), lambda: _capi.inclusion_raw(np.zeros((4, 2)), 1, 9999)):
        with pytest.raises(bnr_amd.BnrError) as e:
            call()
        assert e.value.code == _capi.BNR_ERR_BAD_ARG
    out = [np.empty(dr.V), np.empty((dr.V, dr.V)), np.empty(dr.V + 1), np.zeros(1, dtype=np.int64), np.zeros((2, 1), dtype=np.uint64), np.zeros(2, dtype=np.int64)]
    assert _raw_pooled(chains, 1, 640, 0, 2, out) == _capi.BNR_OK and out[3][0] >= 2
    big = [np.zeros((257, 1), dtype=np.uint64), np.zeros(257, dtype=np.int64)]
    for which, ntop, outs in ((2, 2, out), (0, 257, out[:4] + big), (0, -1, out), (0, 2, out[:5] + [None]), (0, 2, out[:4] + [None, out[5]]), (0, 0, out),
                              (0, 2, [None] * 6)):
        assert _raw_pooled(chains, 1, 640, which, ntop, outs) == _capi.BNR_ERR_BAD_ARG, (which, ntop)
        assert chains[0].L.bnr_last_error()
    with pytest.raises(ValueError):
        _capi.pooled_inclusion([], 1, 640, 0, 2)
    for ntop in (0, 257):
        with pytest.raises(ValueError):
            api.device_node_sets(chains, 0, 640, ntop)
    few = _capi.pooled_inclusion(chains, 1, 640, 1, 0, fields=("prob", "n_distinct"))       # no top sets, ntop = 0: allowed
    assert few[0].shape == (dr.R,) and 1 <= few[3] <= 4 and few[1] is None


# ------------------------------------------------------------------------------------------------------------------ Fit
def test_fit_fills_node_sets(gpu, tmp_path):
    X, y, _ = bnr_amd.make_synthetic(20, 5, 2, seed=5)
    kw = dict(nburn=20, nsamples=40, num_chains=2, seed=17, x_transform=False, suppress_timer=True, psrf_cutoff=np.inf,
              filename=str(tmp_path / "parameters.log"), device=gpu)
    res = bnr_amd.Fit(X, y, 2, node_sets=True, top_sets=5, **kw)
    ns = res.node_sets
    assert ns is not None and (ns.chains, ns.draws) == (2, 80)
    assert ns.prob_nodes.shape == (5,) and ns.co_inclusion.shape == (5, 5) and ns.size_pmf.shape == (6,) and ns.dim_pmf.shape == (3,) and ns.prob_active.shape == (2,)
    assert 1 <= len(ns.top_sets) <= 5 and len(ns.top_sets) == len(ns.top_prob) == min(5, ns.n_distinct) and ns.map_model is ns.top_sets[0]
    assert np.array_equal(np.diag(ns.co_inclusion), ns.prob_nodes) and np.all(np.diff(ns.top_prob) <= 0) and ns.top_prob.sum() <= 1.0
    assert bnr_amd.NodeSets(res) is ns
    one = bnr_amd.NodeSets(bnr_amd.Results(res.state, None, None, res.burn_in, res.sampled), top_sets=5)      # chain 1 alone, on the host
    assert one.chains == 1 and one.draws == 40
    assert bnr_amd.Fit(X, y, 2, **kw).node_sets is None
