"""CPU tests of the joint posterior of the node indicators (ABI 15): the numpy restatement api._host_inclusion against the brute force of
tests/incl_ref.py (Python integers and Counter), _host_node_sets on a hand-computed example, the ABI and its exports, the refusals that need no
GPU, Fit's refusals before sampling and the k_incl_* kernels' place in the code objects.  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import bnr_amd
import code_objects as co
import diag_ref as dr
import incl_ref as ir
from bnr_amd import _capi, api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_restatement_against_the_brute_force_on_the_grid():
    for what, z in ir.grid_cases():
        for ntop in ir.NTOPS if what[1] in (2, 65) else (4,):
            got = api._host_inclusion(z, ntop)
            ir.same(got, ir.brute(z, ntop), (what, ntop))
            assert got["top_count"].sum() <= z.shape[0] and np.all(np.diff(got["top_count"]) <= 0)
            assert np.array_equal(np.diag(got["joint"]), got["prob"]) and np.array_equal(got["joint"], got["joint"].T)
    z = ir.long_matrix()
    ir.same(api._host_inclusion(z, 256), ir.brute(z, 256), "long")
    for z in (np.zeros((65, 70), dtype=np.uint8), np.ones((65, 70), dtype=np.uint8)):
        got = api._host_inclusion(z, 4)
        ir.same(got, ir.brute(z, 4), "constant")
        assert got["n_distinct"] == 1 and got["top_count"].tolist() == [65, 0, 0, 0] and not got["top_sets"][1:].any()
    assert api._host_inclusion(np.ones((3, 70)), 1)["top_sets"].tolist() == [[2**64 - 1, 2**6 - 1]]      # the unused high bits are 0


def test_the_tie_rule_and_the_indicator_convention():
    # counts 2, 2, 2, 1: among the equal counts the pattern as an integer decides (indicator 0 is the lowest bit), then the single draw
    z = np.array([[0, 1, 1], [1, 0, 0], [0, 1, 0], [1, 0, 0], [0, 1, 1], [0, 1, 0], [1, 1, 1]])
    got = api._host_inclusion(z, 5)
    assert got["top_sets"][:, 0].tolist() == [1, 2, 6, 7, 0] and got["top_count"].tolist() == [2, 2, 2, 1, 0] and got["n_distinct"] == 4
    # x != 0.0: -0 is zero, a NaN counts as included, any other number is 1
    x = np.array([[0.0, -0.0, np.nan], [1.0, -2.5, 0.0], [-0.0, 5e-324, dr.NAN_NEG]])
    got = api._host_inclusion(x, 3)
    assert got["prob"].tolist() == [1 / 3, 2 / 3, 2 / 3] and got["top_sets"][:, 0].tolist() == [3, 4, 6] and got["size_pmf"].tolist() == [0, 1 / 3, 2 / 3, 0]
    ir.same(got, ir.brute(x, 3), "floats")
    for bad in (np.zeros((0, 3)), np.zeros((3, 0)), np.zeros(3)):
        with pytest.raises(ValueError):
            api._host_inclusion(bad, 1)
    for ntop in (-1, 257):
        with pytest.raises(ValueError):
            api._host_inclusion(z, ntop)


def _table(xi, lam, pad=2):
    """a table whose rows pad .. pad + len(xi) - 1 hold the given indicators (the rows around them hold ones)"""
    xi, lam = np.asarray(xi, dtype=np.float64), np.asarray(lam, dtype=np.float64)
    t = dr.new_table(xi.shape[0] + 2 * pad, xi.shape[1], lam.shape[1])
    t["xi"][:] = 1.0
    t["lam"][:] = 1.0
    t["xi"][pad:pad + xi.shape[0], :, 0] = xi
    t["lam"][pad:pad + lam.shape[0], :, 0] = lam
    return t


def test_node_sets_of_a_four_draw_three_node_example():
    """draws: {1, 2}, {3}, {1, 2}, {1}; lambda: (1, -1), (0, 1), (0, 0), (-1, 1).  By hand:
    prob_nodes = (3, 2, 1) / 4; co-inclusion of (1, 2) = 2 / 4, of (1, 3) and (2, 3) = 0; sizes 1, 1, 2, 2 -> pmf (0, 1/2, 1/2, 0);
    three distinct sets: {1, 2} twice, then {1} (pattern 1) before {3} (pattern 4); active dimensions 2, 1, 0, 2 -> pmf (1/4, 1/4, 1/2)"""
    xi = [[1, 1, 0], [0, 0, 1], [1, 1, 0], [1, 0, 0]]
    lam = [[1, -1], [0, 1], [0, 0], [-1, 1]]
    ns = api._host_node_sets([_table(xi, lam)], 2, 4, ntop=10)
    assert ns.prob_nodes.tolist() == [0.75, 0.5, 0.25]
    assert ns.co_inclusion.tolist() == [[0.75, 0.5, 0.0], [0.5, 0.5, 0.0], [0.0, 0.0, 0.25]]
    assert ns.size_pmf.tolist() == [0.0, 0.5, 0.5, 0.0] and ns.size_mean == 1.5 and ns.size_mode == 1
    assert ns.n_distinct == 3 and [s.tolist() for s in ns.top_sets] == [[1, 2], [1], [3]] and ns.top_prob.tolist() == [0.5, 0.25, 0.25]
    assert ns.map_model.tolist() == [1, 2] and ns.median_model.tolist() == [1]              # (0.5 is not above 0.5)
    assert ns.prob_active.tolist() == [0.5, 0.75] and ns.dim_pmf.tolist() == [0.25, 0.25, 0.5] and ns.dim_mean == 1.25
    assert (ns.chains, ns.draws) == (1, 4)
    two = api._host_node_sets([_table(xi, lam), _table(xi[:2] + xi[:2], lam)], 2, 4, ntop=1)  # a second chain: {1, 2}, {3}, {1, 2}, {3}
    assert (two.chains, two.draws, two.n_distinct) == (2, 8, 3) and [s.tolist() for s in two.top_sets] == [[1, 2]] and two.top_prob.tolist() == [0.5]
    assert two.prob_nodes.tolist() == [0.625, 0.5, 0.375]
    # through Results: the host path on chain 1's table, and the stored result as it is
    res = bnr_amd.Results(_table(xi, lam), None, None, 2, 4)
    assert res.node_sets is None
    got = bnr_amd.NodeSets(res)
    assert isinstance(got, bnr_amd.NodeSets) and got.co_inclusion.tolist() == ns.co_inclusion.tolist() and len(got.top_sets) == 3
    assert len(bnr_amd.NodeSets(res, top_sets=2).top_sets) == 2
    res.node_sets = ns
    assert bnr_amd.NodeSets(res) is ns and bnr_amd.NodeSets(res, top_sets=3) is ns
    assert bnr_amd.NodeSets(res, top_sets=7) is ns                            # all 3 distinct sets are there: nothing more to ask for
    res.node_sets = api._host_node_sets([_table(xi, lam)] * 2, 2, 4, ntop=2)  # a fit that kept 2 of 3 sets over two chains
    assert bnr_amd.NodeSets(res, top_sets=2).chains == 2
    with pytest.raises(ValueError, match="top_sets"):                         # never chain 1's host result in place of the stored one
        bnr_amd.NodeSets(res, top_sets=3)
    with pytest.raises(ValueError):
        bnr_amd.NodeSets(bnr_amd.Results(None, None, None, 2, 4))
    for bad in (0, 257, 2.5, True):
        with pytest.raises(ValueError):
            api._host_node_sets([_table(xi, lam)], 2, 4, ntop=bad)
    with pytest.raises(ValueError):
        api._host_node_sets([], 2, 4)
    with pytest.raises(TypeError):
        bnr_amd.NodeSets(prob_nodes=ns.prob_nodes)


def test_abi_15_and_its_exports():
    hdr = open(os.path.join(ROOT, "include", "bnr_hip.h")).read()
    ver = int(re.search(r"#define BNR_ABI_VERSION (\d+)", hdr).group(1))
    L = bnr_amd.lib()
    assert ver >= 15 and L.bnr_abi_version() == ver
    raw = C.CDLL(bnr_amd.LIB)
    for name in ("bnr_chain_inclusion", "bnr_chains_inclusion", "bnr_inclusion"):
        assert hasattr(raw, name) and hasattr(L, name) and name in bnr_amd.EXPORTS and re.search(r"\bint %s\(" % name, hdr), name
    for name in ("NodeSets", "device_node_sets", "inclusion"):
        assert hasattr(bnr_amd, name), name
    assert hasattr(_capi, "pooled_inclusion") and hasattr(_capi, "inclusion_raw") and hasattr(_capi.Chain, "inclusion") and _capi.INCL_FIELDS == ir.FIELDS


def test_refusals_that_need_no_gpu():
    z = ir.bernoulli(16, 5)
    for kw in (dict(ntop=-1), dict(ntop=257), dict(ntop=0), dict(ntop=2, fields=("top_sets",)), dict(ntop=2, fields=("prob", "top_count")),
               dict(ntop=2, fields=()), dict(ntop=2, fields=("prob", "median"))):
        with pytest.raises(ValueError):
            _capi.inclusion_raw(z, **kw)
    for bad in (np.zeros((0, 3)), np.zeros((3, 0)), np.zeros(3)):
        with pytest.raises(ValueError):
            _capi.inclusion_raw(bad, 1)
    # the library's own checks that precede its first HIP call
    L = bnr_amd.lib()
    P = _capi._ptr
    zz = np.ascontiguousarray(z)
    out = [np.empty(5), np.empty((5, 5)), np.empty(6), np.zeros(1, dtype=np.int64), np.zeros((2, 1), dtype=np.uint64), np.zeros(2, dtype=np.int64)]

    def call(zp=zz, S=16, B=5, ntop=2, outs=out):
        return L.bnr_inclusion(0, S, B, P(zp), ntop, *[P(o) for o in outs])

    for kw in (dict(zp=None), dict(S=0), dict(B=0), dict(ntop=-1), dict(ntop=257), dict(ntop=0), dict(outs=[None] * 6), dict(outs=out[:4] + [out[4], None]),
               dict(outs=out[:4] + [None, out[5]])):
        assert call(**kw) == _capi.BNR_ERR_BAD_ARG, kw
        assert L.bnr_last_error()
    wide = np.zeros((1, 4097), dtype=np.uint8)                               # more indicators than k_incl_pack's counters in LDS hold
    assert L.bnr_inclusion(0, 1, 4097, P(wide), 0, P(np.empty(4097)), *[None] * 5) == _capi.BNR_ERR_BAD_ARG and b"4096" in L.bnr_last_error()
    assert L.bnr_chains_inclusion(None, 1, 1, 8, 0, 0, *[None] * 6) == _capi.BNR_ERR_BAD_ARG
    assert L.bnr_chain_inclusion(None, 1, 8, 0, 0, *[None] * 6) == _capi.BNR_ERR_BAD_ARG


def test_fit_refuses_node_sets_it_cannot_compute_before_sampling(monkeypatch):
    X, y, _ = bnr_amd.make_synthetic(8, 4, 2, seed=1)
    made = []
    monkeypatch.setattr(api, "ChainSet", lambda *a, **k: made.append(1))
    kw = dict(nburn=4, nsamples=8, x_transform=False, suppress_timer=True, filename=None, node_sets=True)
    for bad in (0, 257, 1.5):
        with pytest.raises(ValueError):
            bnr_amd.Fit(X, y, 2, top_sets=bad, **kw)
        with pytest.raises(ValueError):
            bnr_amd.generate_samples(X, y, 2, nburn=4, nsamp=8, x_transform=False, suppress_timer=True, node_sets=True, top_sets=bad)
    monkeypatch.setattr(api, "_rank_world", lambda: (0, 2))                  # chains spread over two ranks
    with pytest.raises(ValueError, match="one rank"):
        bnr_amd.Fit(X, y, 2, **kw)
    assert not made                                                          # no chain was created


def test_the_inclusion_kernels_sit_in_the_analysis_code_object(tmp_path):
    """k_incl_pack, k_incl_joint and k_incl_group are compiled in csrc/bnr_analysis.hip: all in the analysis code object, none in the sweep's,
    and the sweep's code object lists the kernels it listed before (every kernel of csrc/bnr_kernels.h, none of the analysis header)"""
    assert os.path.exists(co.LIB), "libbnr_hip.so has not been built"
    if not co.have_tools():
        pytest.skip("no ROCm LLVM tools here")
    sweep, analysis = co.sweep_and_analysis(tmp_path)
    incl = sorted(k for k in analysis if k.startswith("k_incl"))
    assert incl == ["k_incl_group", "k_incl_joint", "k_incl_pack"], sorted(analysis)
    assert not [k for k in sweep if k.startswith("k_incl")]
    assert set(analysis) == co.ANALYSIS, sorted(set(analysis) ^ co.ANALYSIS)
    declared = co.declared_kernels("bnr_kernels.h")
    assert {re.sub(r"<.*", "", k) for k in sweep} == declared, sorted({re.sub(r"<.*", "", k) for k in sweep} ^ declared)
