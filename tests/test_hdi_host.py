"""CPU tests of the highest-density intervals and the edge selection (ABI 13): the numpy restatement api._host_hdi against the independent
transcription of ArviZ's _hdi in tests/hdi_ref.py and its brute-force check, the selection rule on hand-made lfsr vectors, the ABI, the
library's argument checks that precede its first HIP call, Fit's refusals before sampling and k_hdi's place in the code object.  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import bnr_amd
import code_objects as co
import hdi_cases as hc
import hdi_ref as hr
import rank_diag_cases as rc
from bnr_amd import _capi, api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _samples():
    rng = np.random.default_rng(2027)
    out = {}
    for n in (1, 2, 3, 20, 257, 1000):
        out["normal", n] = rng.standard_normal(n)
        out["exp", n] = rng.exponential(size=n)
        out["clipped", n] = np.clip(rng.standard_normal(n), -0.8, 0.8)
        out["binary", n] = (rng.random(n) < 0.3).astype(np.float64)
        out["constant", n] = np.full(n, 2.5)
        out["tied widths", n] = np.arange(n, dtype=np.float64)            # every window has the same width: the first one wins
        out["signed zeros", n] = np.where(rng.random(n) < 0.5, -0.0, 0.0)
    return out


@pytest.mark.parametrize("prob", hc.LEVELS + (0.999, 0.001))
def test_restatement_against_the_transcription(prob):
    seen_arviz = 0
    for (name, n), x in _samples().items():
        h = api._host_hdi(x, prob)
        lo, hi = float(h["lower"][0, 0]), float(h["upper"][0, 0])
        assert (lo, hi) == hr.hdi(x, prob), (name, n)
        if n <= 257:
            assert hr.no_shorter_window(x, prob, lo, hi), (name, n)
        av = hr.arviz_hdi(x, prob) if n >= 20 else None
        if av is not None:
            seen_arviz += 1
            assert av == (lo, hi), (name, n)
        xs = np.sort(x)
        assert h["median"][0] == ((xs[n // 2 - 1] + xs[n // 2]) / 2.0 if n >= 2 else xs[0])
        assert h["p_pos"][0] == np.mean(x > 0) and h["p_neg"][0] == np.mean(x < 0)
        assert not np.signbit(h["lower"][0, 0]) or lo != 0.0                # -0 is reported as +0
    print("arviz compared on %d samples" % seen_arviz)


def test_restatement_shapes_levels_and_conventions():
    M = hc.rows(257)
    h = api._host_hdi(M, hc.LEVELS)
    assert h["lower"].shape == h["upper"].shape == (3, 8) and h["median"].shape == h["p_pos"].shape == h["p_neg"].shape == (8,)
    for k, prob in enumerate(hc.LEVELS):                                    # every level on its own is the same bits
        one = api._host_hdi(M, prob)
        assert hc.same_bits(one["lower"][0], h["lower"][k]) and hc.same_bits(one["upper"][0], h["upper"][k])
    assert np.all(h["lower"][:, 1] == -1.5) and np.all(h["upper"][:, 1] == -1.5) and h["p_neg"][1] == 1.0 and h["p_pos"][1] == 0.0
    assert np.isnan(h["lower"][:, 5]).all() and np.isnan(h["upper"][:, 5]).all() and np.isnan(h["median"][5])     # +-Inf: the shares are counted
    assert h["p_pos"][5] == np.mean(M[5] > 0) and h["p_neg"][5] == np.mean(M[5] < 0)
    assert np.all(h["p_pos"] + h["p_neg"] <= 1.0) and h["p_pos"][2] == np.mean(M[2] == 1.0) and h["p_neg"][2] == 0.0
    widths = h["upper"] - h["lower"]
    ok = ~np.isnan(widths[0])
    assert np.all(widths[0, ok] <= widths[1, ok]) and np.all(widths[1, ok] <= widths[2, ok])
    M[0, 3] = np.nan
    h = api._host_hdi(M, hc.LEVELS)
    for f in hc.FIELDS:
        assert np.isnan(h[f][..., 0]).all() and not np.isnan(h[f][..., 3]).any(), f
    for bad in ((), 0.0, 1.0, (0.5, np.nan), -0.1, [0.5] * 9):
        if np.size(bad):
            with pytest.raises(ValueError):
                api._host_hdi(M, bad)
    with pytest.raises(ValueError):
        api._host_hdi(np.zeros((2, 0)), 0.9)


def test_hdi_is_shorter_than_the_equal_tailed_interval_of_a_skewed_sample():
    x = np.random.default_rng(3).exponential(size=4000)
    h = api._host_hdi(x, 0.95)
    xs = np.sort(x)
    assert h["upper"][0, 0] - h["lower"][0, 0] < xs[3899] - xs[99]
    assert h["lower"][0, 0] == xs[0]                                       # the mode of an exponential sample is its smallest draw


def test_selection_rule():
    sel, efsr = api._select_by_lfsr([0.01, 0.5, 0.02, np.nan, 0.2, 0.03], 0.05)
    assert sel.tolist() == [True, False, True, False, False, True] and efsr == pytest.approx(0.02)
    # the prefix mean, not the values: 0.09 alone is above 0.05 but the mean of (0.01, 0.01, 0.01, 0.09) is 0.03
    sel, efsr = api._select_by_lfsr([0.09, 0.01, 0.01, 0.01, 0.4], 0.05)
    assert sel.tolist() == [True, True, True, True, False] and efsr == pytest.approx(0.03)
    # ties by edge index: behind the two 0.0 the three 0.1 come in the order of their indices 0, 2, 4
    lf = np.array([0.1, 0.0, 0.1, 0.0, 0.1])
    sel, efsr = api._select_by_lfsr(lf, 0.05)
    assert sel.tolist() == [True, True, True, True, False] and efsr == pytest.approx(0.05)
    sel, efsr = api._select_by_lfsr(lf, 0.049)
    assert sel.tolist() == [True, True, False, True, False] and efsr == pytest.approx(0.1 / 3)
    sel, efsr = api._select_by_lfsr([0.3, 0.2, np.nan], 0.05)               # nothing selected
    assert not sel.any() and efsr == 0.0
    sel, efsr = api._select_by_lfsr([0.3, 0.2, 0.0], 1.0)                   # everything selected
    assert sel.all() and efsr == pytest.approx(0.5 / 3)
    sel, efsr = api._select_by_lfsr([np.nan, np.nan], 1.0)
    assert not sel.any() and efsr == 0.0
    sel, efsr = api._select_by_lfsr([], 0.05)
    assert sel.shape == (0,) and efsr == 0.0
    sel, efsr = api._select_by_lfsr([0.0, 0.0, 0.5], 0.0)                   # fdr = 0: only the edges whose every draw has one sign
    assert sel.tolist() == [True, True, False] and efsr == 0.0


def test_edge_selection_on_a_table_and_the_results_path():
    t = rc.tables()[0]
    es = api._host_edge_selection([t], 37, 601, 0.9, 0.05)
    q, V = t["gamma"].shape[1], t["xi"].shape[1]
    assert (es.chains, es.draws, es.hdi_prob, es.fdr) == (1, 601, 0.9, 0.05)
    assert es.node1.shape == es.node2.shape == es.estimate.shape == es.selected.shape == (q,) and es.prob_nodes.shape == es.xi_hdi_lower.shape == (V,)
    assert (es.node1[0], es.node2[0], es.node1[V], es.node2[V], es.node1[-1], es.node2[-1]) == (1, 1, 2, 2, V, V)
    g = t["gamma"][37:638, :, 0]
    for j in (0, 1, 2, 5):
        assert (es.hdi_lower[j], es.hdi_upper[j]) == hr.hdi(g[:, j], 0.9), j
    assert np.array_equal(es.lfsr, 1.0 - np.maximum(es.p_pos, es.p_neg), equal_nan=True)
    assert np.array_equal(es.hdi_excludes_zero, (es.hdi_lower > 0) | (es.hdi_upper < 0))
    assert np.array_equal(es.prob_nodes, t["xi"][37:638, :, 0].mean(axis=0))
    assert es.n_selected == es.selected.sum() and (es.n_selected == 0 or es.expected_fsr == pytest.approx(es.lfsr[es.selected].mean()))
    both = api._host_edge_selection(rc.tables()[:2], 37, 601, 0.9, 0.05)
    assert (both.chains, both.draws) == (2, 1202)
    res = bnr_amd.Results(t, None, None, 37, 601)
    assert res.edge_selection is None
    got = bnr_amd.EdgeSelect(res, 0.9)
    assert np.array_equal(got.hdi_lower, es.hdi_lower, equal_nan=True) and np.array_equal(got.selected, es.selected)
    assert bnr_amd.EdgeSelect(res).hdi_prob == 0.95
    res.edge_selection = es                                                  # what the fit carried: returned as it is, or re-selected at another fdr
    assert bnr_amd.EdgeSelect(res) is es and bnr_amd.EdgeSelect(res, 0.9, 0.05) is es
    loose = bnr_amd.EdgeSelect(res, fdr=0.5)
    assert loose.fdr == 0.5 and loose.n_selected >= es.n_selected and loose.hdi_lower is es.hdi_lower
    assert np.array_equal(loose.selected, api._select_by_lfsr(es.lfsr, 0.5)[0])
    with pytest.raises(ValueError):
        bnr_amd.EdgeSelect(bnr_amd.Results(None, None, None, 37, 601))
    for bad in (dict(hdi_prob=0.0), dict(hdi_prob=1.0), dict(fdr=-0.1), dict(fdr=1.5), dict(hdi_prob=np.nan)):
        with pytest.raises(ValueError):
            api._host_edge_selection([t], 37, 601, **bad)


def test_abi_13_and_its_exports():
    hdr = open(os.path.join(ROOT, "include", "bnr_hip.h")).read()
    ver = int(re.search(r"#define BNR_ABI_VERSION (\d+)", hdr).group(1))
    L = bnr_amd.lib()
    assert ver >= 13 and L.bnr_abi_version() == ver
    raw = C.CDLL(bnr_amd.LIB)
    for name in ("bnr_chain_hdi", "bnr_chains_hdi", "bnr_hdi"):
        assert hasattr(raw, name) and name in bnr_amd.EXPORTS and re.search(r"\bint %s\(" % name, hdr), name
    for name in ("EdgeSelect", "EdgeSelection", "device_edge_selection", "hdi"):
        assert hasattr(bnr_amd, name), name
    assert hasattr(_capi, "pooled_hdi") and hasattr(_capi, "hdi_raw") and hasattr(_capi.Chain, "hdi")


def test_argument_checks_that_precede_the_first_hip_call():
    L = bnr_amd.lib()
    x = np.ascontiguousarray(np.random.default_rng(1).standard_normal((2, 16)))
    out = [np.empty((3, 2)), np.empty((3, 2)), np.empty(2), np.empty(2), np.empty(2)]
    P = _capi._ptr

    def call(xx=x, m=2, S=16, probs=(0.5, 0.9, 0.95), nprob=None, outs=out):
        pr = np.ascontiguousarray(probs, dtype=np.float64)
        return L.bnr_hdi(0, m, S, P(xx), pr.size if nprob is None else nprob, P(pr) if pr.size else None, *[P(o) for o in outs])

    bad = [dict(xx=None), dict(m=0), dict(S=0), dict(outs=[None] * 5), dict(outs=[out[0], None] + out[2:]), dict(outs=[None, out[1]] + out[2:]),
           dict(probs=[0.5] * 9), dict(nprob=-1), dict(probs=(0.5, 0.0)), dict(probs=(1.0,)), dict(probs=(np.nan,)), dict(probs=(-0.5,)),
           dict(probs=()), dict(probs=(), nprob=2, outs=[None, None] + out[2:])]
    for kw in bad:
        assert call(**kw) == _capi.BNR_ERR_BAD_ARG, kw
        assert L.bnr_last_error()
    null5 = [None] * 5
    assert L.bnr_chains_hdi(None, 1, 1, 8, 0, None, *null5) == _capi.BNR_ERR_BAD_ARG
    assert L.bnr_chain_hdi(None, 1, 8, 0, None, *null5) == _capi.BNR_ERR_BAD_ARG
    for probs in ([0.5] * 9, 0.0, 1.0, (0.5, np.nan)):                          # the binding refuses these before it calls the library
        with pytest.raises(ValueError):
            _capi.hdi_raw(x, probs)
    with pytest.raises(ValueError):
        _capi.hdi_raw(np.zeros((2, 0)), 0.9)


def test_fit_refuses_an_edge_selection_it_cannot_compute_before_sampling(monkeypatch):
    X, y, _ = bnr_amd.make_synthetic(8, 4, 2, seed=1)
    made = []
    monkeypatch.setattr(api, "ChainSet", lambda *a, **k: made.append(1))
    kw = dict(nburn=4, nsamples=8, x_transform=False, suppress_timer=True, filename=None, edge_selection=True)
    for bad in (dict(hdi_prob=0.0), dict(hdi_prob=1.0), dict(hdi_prob=95), dict(fdr=-0.01), dict(fdr=2.0), dict(hdi_prob=float("nan"))):
        with pytest.raises(ValueError):
            bnr_amd.Fit(X, y, 2, **kw, **bad)
        with pytest.raises(ValueError):
            bnr_amd.generate_samples(X, y, 2, nburn=4, nsamp=8, x_transform=False, suppress_timer=True, edge_selection=True, **bad)
    monkeypatch.setattr(api, "_rank_world", lambda: (0, 2))                  # chains spread over two ranks
    with pytest.raises(ValueError, match="one rank"):
        bnr_amd.Fit(X, y, 2, **kw)
    assert not made                                                          # no chain was created


def test_k_hdi_and_k_rank_sit_outside_the_code_object_of_the_sweep(tmp_path):
    """k_hdi, k_rank and k_fold are compiled in csrc/bnr_analysis.hip: they are in the analysis code object and not in the sweep's"""
    assert os.path.exists(co.LIB), "libbnr_hip.so has not been built"
    if not co.have_tools():
        pytest.skip("no ROCm LLVM tools here")
    sweep, analysis = co.sweep_and_analysis(tmp_path)
    hdi = [k for k in analysis if k.startswith("k_hdi")]
    rank = [k for k in analysis if k.startswith(("k_rank", "k_fold"))]
    assert len(hdi) == 1 and len(rank) == 2 and set(hdi + rank) <= co.ANALYSIS, sorted(analysis)
    assert not [k for k in sweep if k.startswith(("k_hdi", "k_rank", "k_fold"))]
