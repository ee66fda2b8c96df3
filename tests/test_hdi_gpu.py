"""GPU tests of the highest-density intervals, sign probabilities and edge selection (ABI 13; run with -m gpu on an MI355X): k_hdi alone
(bnr_hdi against the numpy restatement api._host_hdi, itself pinned to a transcription of ArviZ's _hdi by tests/test_hdi_host.py),
bnr_chains_hdi / bnr_chain_hdi through device_edge_selection against the restatement over the fetched windows, the bitwise properties, what
the feature is for, the refusals and Fit(..., edge_selection=True).

Every comparison is of bits: the kernel's arithmetic is one f64 subtraction per window, integer counts over n and the mean of two draws, all
of which numpy does in the same way, so no tolerance is needed.

Chains as in test_diagnostics_gpu.py: three Chains of n = 8, V = 16, R = 2 with 640-row tables, never run; tables come in by Chain.load."""
import numpy as np
import pytest

import bnr_amd
import diag_ref as dr
import hdi_cases as hc
import rank_diag_cases as rc
from bnr_amd import _capi, api

pytestmark = pytest.mark.gpu
ES_ARRAYS = ("estimate", "hdi_lower", "hdi_upper", "p_pos", "p_neg", "lfsr", "xi_estimate", "xi_hdi_lower", "xi_hdi_upper", "prob_nodes")


@pytest.fixture(scope="module")
def chains(gpu):
    X, y, _ = bnr_amd.make_synthetic(dr.N, dr.V, dr.R, seed=3)
    cs = [bnr_amd.Chain(X, y, dr.R, dr.TOT, 99, 1, device=gpu)]
    cs += [bnr_amd.Chain.like(cs[0], 99, c) for c in (2, 3)]
    yield cs
    for c in cs:
        c.close()


def _load(chains, tabs):
    for ch, t in zip(chains, tabs):
        ch.load(t)


def _same(got, want, what):
    for f, g in zip(_capi.HDI_FIELDS, got):
        assert hc.same_bits(g, want[f]), (what, f)


# ------------------------------------------------------------------------------------------------------------------ the kernel alone
def _check_rows(M, gpu):
    want = api._host_hdi(M, hc.LEVELS)
    got = _capi.hdi_raw(M, hc.LEVELS, gpu)
    _same(got, want, M.shape)
    assert np.array_equal(got[3] + got[4] <= 1.0, ~np.isnan(got[3]))
    return got


@pytest.mark.parametrize("S", hc.ROW_LENGTHS)
def test_hdi_kernel_against_the_restatement(gpu, S):
    M = hc.rows(S)
    full = _check_rows(M, gpu)
    # each output alone (every other pointer NULL; the bounds come as a pair) is the same bits
    for fields in (("lower", "upper"), ("median",), ("p_pos",), ("p_neg",)):
        one = _capi.hdi_raw(M, hc.LEVELS, gpu, fields=fields)
        for f, a, b in zip(_capi.HDI_FIELDS, one, full):
            assert (a is None) if f not in fields else hc.same_bits(a, b), (S, fields, f)
    for k, prob in enumerate(hc.LEVELS):                                  # every level alone
        lo, up = _capi.hdi_raw(M, prob, gpu, fields=("lower", "upper"))[:2]
        assert hc.same_bits(lo[0], full[0][k]) and hc.same_bits(up[0], full[1][k]), (S, prob)
    none = _capi.hdi_raw(M, (), gpu, fields=("median", "p_pos", "p_neg"))  # no level at all: no window is searched
    assert none[0] is None and hc.same_bits(none[2], full[2]) and hc.same_bits(none[3], full[3])


def test_hdi_kernel_indices_past_16_bits(gpu):
    M = hc.long_row()
    got = _check_rows(M, gpu)
    assert got[0][2, 0] == -1.2 and got[1][2, 0] == 1.2                   # 11.5 % of the draws sit on either clip: many windows of width 2.4, the first wins


def test_hdi_kernel_nan_and_inf_rows(gpu):
    M = np.random.default_rng(11).standard_normal((5, 257))
    M[0, 3] = dr.NAN_POS
    M[2, 256] = dr.NAN_NEG
    M[2, 5] = np.inf                                                      # a NaN and an Inf: the NaN rules
    M[4, 0], M[4, 100] = np.inf, -np.inf
    got = dict(zip(_capi.HDI_FIELDS, _check_rows(M, gpu)))
    for f in hc.FIELDS:
        assert np.isnan(got[f][..., 0]).all() and np.isnan(got[f][..., 2]).all(), f
        assert not np.isnan(got[f][..., 1]).any() and not np.isnan(got[f][..., 3]).any(), f
    assert np.isnan(got["lower"][:, 4]).all() and np.isnan(got["upper"][:, 4]).all() and np.isnan(got["median"][4])
    assert got["p_pos"][4] == np.mean(M[4] > 0) and got["p_neg"][4] == np.mean(M[4] < 0)
    clean = _capi.hdi_raw(M[1:2], hc.LEVELS, gpu)                         # the neighbouring clean row is what it is alone
    for f, a in zip(_capi.HDI_FIELDS, clean):
        assert hc.same_bits(a[..., 0], got[f][..., 1]), f
    v = bnr_amd.hdi(M[1], 0.9, device=gpu)                                # a vector is one row, one level a scalar
    assert v["lower"].shape == () and v["median"].shape == () and float(v["lower"]) == api._host_hdi(M[1], 0.9)["lower"][0, 0]
    m = bnr_amd.hdi(M, hc.LEVELS, device=gpu)
    assert m["lower"].shape == (3, 5) and m["p_pos"].shape == (5,) and hc.same_bits(m["upper"], got["upper"])


# ------------------------------------------------------------------------------------------------------------------ chains against the restatement
def _compare_selection(got, want, what):
    for f in ES_ARRAYS:
        assert hc.same_bits(getattr(got, f), getattr(want, f)), (what, f)
    for f in ("node1", "node2", "hdi_excludes_zero", "selected"):
        assert np.array_equal(getattr(got, f), getattr(want, f)), (what, f)
    assert (got.n_selected, got.expected_fsr, got.chains, got.draws, got.hdi_prob, got.fdr) == \
        (want.n_selected, want.expected_fsr, want.chains, want.draws, want.hdi_prob, want.fdr), what


@pytest.mark.parametrize("first,nsamp,_lag", rc.WINDOWS)
def test_device_against_the_restatement(chains, first, nsamp, _lag):
    _load(chains, rc.tables())
    fetched = [ch.fetch() for ch in chains]
    for nch in (3, 1):
        for prob, fdr in ((0.95, 0.05), (0.5, 0.2)):
            got = api.device_edge_selection(chains[:nch], first - 1, nsamp, prob, fdr)
            want = api._host_edge_selection(fetched[:nch], first - 1, nsamp, prob, fdr)
            _compare_selection(got, want, (nch, first, nsamp, prob))
            assert (got.chains, got.draws) == (nch, nch * nsamp) and got.estimate.shape == (dr.Q,) and got.prob_nodes.shape == (dr.V,)
    const = [j for j in range(dr.Q) if dr.family_of(j) in dr.CONSTANT]     # a constant column: lower = upper = the constant
    assert np.array_equal(got.hdi_lower[const], got.hdi_upper[const]) and np.array_equal(got.hdi_lower[const], got.estimate[const])


# ------------------------------------------------------------------------------------------------------------------ bitwise properties
def test_bitwise_properties(chains):
    _load(chains, rc.tables())
    first, nsamp, lag = 38, 601, 150
    before = [ch.fetch() for ch in chains]
    iters = [ch.iter for ch in chains]
    base = _capi.pooled_hdi(chains, first, nsamp, hc.LEVELS)
    rank = _capi.pooled_rank_diag(chains, first, nsamp, lag)
    again = _capi.pooled_hdi(chains, first, nsamp, hc.LEVELS)                 # a repeated call, with a rank-diagnostics call in between
    rank2 = _capi.pooled_rank_diag(chains, first, nsamp, lag)
    for a, b in zip(base, again):
        assert hc.same_bits(a, b)
    for a, b in zip(rank, rank2):
        assert np.array_equal(a, b, equal_nan=True)
    try:
        for blk in (1, 7, 0):
            chains[0].set_option("rank_block_cols", blk)
            for f, a, b in zip(_capi.HDI_FIELDS, base, _capi.pooled_hdi(chains, first, nsamp, hc.LEVELS)):
                assert hc.same_bits(a, b), (blk, f)
    finally:
        chains[0].set_option("rank_block_cols", 0)
    for fields in (("lower", "upper"), ("median",), ("p_pos",), ("p_neg",)):  # the outputs requested
        one = _capi.pooled_hdi(chains, first, nsamp, hc.LEVELS, fields=fields)
        for f, a, b in zip(_capi.HDI_FIELDS, one, base):
            assert (a is None) if f not in fields else hc.same_bits(a, b), (fields, f)
    one = chains[1].hdi(first, nsamp, hc.LEVELS)
    for a, b in zip(one, _capi.pooled_hdi([chains[1]], first, nsamp, hc.LEVELS)):
        assert hc.same_bits(a, b)
    for ch, b, it in zip(chains, before, iters):                              # nothing of any chain is written
        after = ch.fetch()
        assert ch.iter == it
        for k in b:
            assert np.array_equal(b[k].view(np.uint64), after[k].view(np.uint64)), k


# ------------------------------------------------------------------------------------------------------------------ what the feature is for
def signal_tables(seed=12):
    """gamma_0: exponential draws; gamma_j, j >= 1: N(delta, 1) with delta = (0, 0.5, 3)[j % 3]; xi the crafted columns"""
    tabs = []
    delta = np.array([0.0, 0.5, 3.0])[np.arange(dr.Q) % 3]
    for c, t in enumerate(rc.tables()):
        t = dict(t)
        rng = np.random.default_rng([seed, c])
        g = rng.standard_normal((dr.TOT, dr.Q)) + delta
        g[:, 0] = rng.exponential(size=dr.TOT)
        t["gamma"] = np.asfortranarray(g.reshape(dr.TOT, dr.Q, 1))
        tabs.append(t)
    return tabs, delta


def test_hdi_beats_the_equal_tailed_interval_and_the_selection_finds_the_signal(chains):
    tabs, delta = signal_tables()
    _load(chains, tabs)
    S = 3 * dr.TOT
    es = api.device_edge_selection(chains, 0, dr.TOT, 0.95, 0.05)
    _mean, lo, up, _pxi = _capi.pooled_summary(chains, 1, dr.TOT, *api._summary_ranks(S, 95))
    print("exponential column: HDI [%.4f, %.4f] (width %.4f), equal-tailed [%.4f, %.4f] (width %.4f); %d edges selected, expected FSR %.4f"
          % (es.hdi_lower[0], es.hdi_upper[0], es.hdi_upper[0] - es.hdi_lower[0], lo[0], up[0], up[0] - lo[0], es.n_selected, es.expected_fsr))
    assert es.hdi_upper[0] - es.hdi_lower[0] < up[0] - lo[0]
    assert es.hdi_lower[0] < lo[0] and es.p_pos[0] == 1.0 and es.lfsr[0] == 0.0 and es.selected[0]
    j = np.arange(1, dr.Q)
    strong, null = j[delta[1:] == 3.0], j[delta[1:] == 0.0]
    assert es.selected[strong].all() and es.hdi_excludes_zero[strong].all() and not es.selected[null].any()
    assert 0.0 < es.expected_fsr <= 0.05 and es.n_selected == es.selected.sum() >= strong.size + 1
    assert es.expected_fsr == pytest.approx(es.lfsr[es.selected].mean(), rel=1e-12)


# ------------------------------------------------------------------------------------------------------------------ refusals
def test_refusals(chains):
    _load(chains, rc.tables())
    bad = [dict(first_row=600, nsamp=100), dict(first_row=0, nsamp=100), dict(first_row=1, nsamp=0)]
    for kw in bad:
        for call in (lambda: _capi.pooled_hdi(chains, probs=0.9, **kw), lambda: chains[0].hdi(probs=0.9, **kw)):
            with pytest.raises(bnr_amd.BnrError) as e:
                call()
            assert e.value.code == _capi.BNR_ERR_BAD_ARG, kw
    for call in (lambda: _capi.pooled_hdi([chains[0], chains[1], chains[0]], 1, 640, 0.9), lambda: _capi.pooled_hdi(chains, 1, 640, 0.9, fields=()),
                 lambda: chains[0].hdi(1, 640, 0.9, fields=()), lambda: _capi.pooled_hdi(chains, 1, 640, 0.9, fields=("lower",)),
                 lambda: _capi.pooled_hdi(chains, 1, 640, 0.9, fields=("upper", "median")), lambda: _capi.pooled_hdi(chains, 1, 640, ()),
                 lambda: _capi.hdi_raw(np.zeros((2, 4)), 0.9, 9999)):
        with pytest.raises(bnr_amd.BnrError) as e:
            call()
        assert e.value.code == _capi.BNR_ERR_BAD_ARG
    with pytest.raises(ValueError):
        _capi.pooled_hdi([], 1, 640, 0.9)
    for kw in (dict(hdi_prob=1.0), dict(hdi_prob=0.0), dict(fdr=-1.0)):
        with pytest.raises(ValueError):
            api.device_edge_selection(chains, 0, 640, **kw)
    med = _capi.pooled_hdi(chains, 1, 640, (), fields=("median",))            # no level, no bounds: allowed
    assert med[0] is None and med[2].shape == (dr.Q + dr.V,)


# ------------------------------------------------------------------------------------------------------------------ Fit
def test_fit_fills_edge_selection(gpu, tmp_path):
    X, y, _ = bnr_amd.make_synthetic(20, 5, 2, seed=5)
    kw = dict(nburn=20, nsamples=40, num_chains=2, seed=17, x_transform=False, suppress_timer=True, psrf_cutoff=np.inf,
              filename=str(tmp_path / "parameters.log"), device=gpu)
    res = bnr_amd.Fit(X, y, 2, edge_selection=True, hdi_prob=0.9, fdr=0.1, **kw)
    es = res.edge_selection
    assert es is not None and (es.chains, es.draws, es.hdi_prob, es.fdr) == (2, 80, 0.9, 0.1)
    assert es.estimate.shape == (15,) and es.prob_nodes.shape == (5,) and np.isfinite(es.hdi_lower).all() and np.all(es.hdi_lower <= es.hdi_upper)
    assert np.all((es.hdi_lower <= es.estimate) & (es.estimate <= es.hdi_upper)) and np.all((es.lfsr >= 0) & (es.lfsr <= 1))
    assert bnr_amd.EdgeSelect(res) is es
    one = bnr_amd.EdgeSelect(bnr_amd.Results(res.state, None, None, res.burn_in, res.sampled), 0.9, 0.1)      # chain 1 alone, on the host
    assert one.chains == 1 and one.draws == 40
    assert bnr_amd.Fit(X, y, 2, **kw).edge_selection is None
