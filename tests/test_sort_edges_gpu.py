"""GPU tests of the sort-based analysis kernels at the edges of their radix passes (run with -m gpu on an MI355X): k_rank, k_hdi and
k_incl_group -- one LSD radix sort (bnr_sort_build_keys / bnr_sort_passes) with three users -- and k_summary's radix select, on the inputs
of tests/sort_cases.py: single live passes at every key byte, skipped passes between live ones, 2, 3 and 7 live passes, placed tie runs,
planted ties of the minimal HDI width, the ends of the window length, the zero boundary, and pattern matrices that differ in one byte of
one word.  tests/test_sort_edges_host.py shows on the CPU that these inputs tell a subtly wrong kernel from a right one.

Every comparison is of bits -- ranks against scipy's rankdata, k_hdi against api._host_hdi, the inclusion outputs against api._host_inclusion,
order statistics against np.sort -- but two: z, held to Phi^-1 by mpmath within 2 E_AS |z| + 16 ulp (tests/ndtri_ref.py: E_AS is the measured
error of AS 241 itself, the 16 ulp what tests/test_rank_diag_gpu.py grants the device's log and sqrt), and the rank diagnostics, held to the
restatement by rank_diag_cases.compare as in tests/test_rank_diag_gpu.py.  The largest z ratio is printed (pytest -s).

Chains as in test_rank_diag_gpu.py: three Chains of n = 8, V = 16, R = 2 with 640-row tables, never run; tables come in by Chain.load."""
import numpy as np
import pytest
from scipy.stats import rankdata

import bnr_amd
import diag_ref as dr
import hdi_cases as hc
import incl_ref as ir
import ndtri_ref as nr
import rank_diag_cases as rc
import sort_cases as sc
from bnr_amd import _capi, api

pytestmark = pytest.mark.gpu
WORST = {}
CHAIN_WINDOWS = ((38, 601, 150), (3, 101, 25))


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    print("\nsort edges, largest z error over its allowance 2 E_AS |z| + 16 ulp:", {k: "%.3g" % v for k, v in sorted(WORST.items())})


# ------------------------------------------------------------------------------------------------------------------ k_rank alone
@pytest.mark.parametrize("S", sorted(sc.rank_matrices()))
def test_ranks_and_normal_scores(gpu, S):
    names, M = sc.rank_matrices()[S]
    out = bnr_amd.rank_normalize(M, device=gpu)
    want = np.stack([rankdata(r, method="average") for r in M])
    for i, name in enumerate(names):
        assert np.array_equal(out["ranks"][i], want[i]), name
    # z is a function of the rank and S alone; every distinct rank is held to mpmath
    ur, first = np.unique(want.reshape(-1), return_index=True)
    z = out["z"].reshape(-1)
    assert np.array_equal(z.view(np.uint64), z[first][np.searchsorted(ur, want.reshape(-1))].view(np.uint64))
    ratio = nr.bound_ratios((ur - 0.375) / (S + 0.25), z[first], nr.E_AS, nr.DEVICE_ULPS)
    WORST["S=%d" % S] = float(ratio.max())
    print("rank kernel S = %d: %d rows, %d distinct ranks, z error / allowance at most %.3g" % (S, len(names), ur.size, ratio.max()))
    assert ratio.max() <= 1.0, (S, float(ratio.max()), float(ur[np.argmax(ratio)]))
    # each output alone (the other pointer NULL) is the same bits
    r_only, none = _capi.rank_normalize_raw(M, gpu, z=False)
    none2, z_only = _capi.rank_normalize_raw(M, gpu, ranks=False)
    assert none is None and none2 is None and np.array_equal(r_only, out["ranks"]) and np.array_equal(z_only.view(np.uint64), out["z"].view(np.uint64))


# ------------------------------------------------------------------------------------------------------------------ k_hdi alone
@pytest.mark.parametrize("case", range(len(sc.hdi_matrices())))
def test_hdi_against_the_restatement(gpu, case):
    lv, names, M = sc.hdi_matrices()[case]
    with np.errstate(over="ignore"):
        want = api._host_hdi(M, lv)
    got = _capi.hdi_raw(M, lv, gpu)
    for f, g in zip(_capi.HDI_FIELDS, got):
        for i, name in enumerate(names):
            assert hc.same_bits(g[..., i], want[f][..., i]), (name, f, lv)
    assert not np.isnan(got[2]).any() and not (np.signbit(got[2]) & (got[2] == 0.0)).any()       # every row is finite; the median may be +0 only
    for fields in (("lower", "upper"), ("median",), ("p_pos",), ("p_neg",)):
        one = _capi.hdi_raw(M, lv, gpu, fields=fields)
        for f, a, b in zip(_capi.HDI_FIELDS, one, got):
            assert (a is None) if f not in fields else hc.same_bits(a, b), (fields, f)


# ------------------------------------------------------------------------------------------------------------------ k_incl_* alone
@pytest.mark.parametrize("B", sorted({z.shape[1] for _, z in sc.inclusion_cases()}))
def test_inclusion_against_the_restatement(gpu, B):
    for name, z in sc.inclusion_cases():
        if z.shape[1] != B:
            continue
        for ntop in sc.INCL_NTOPS:
            want = api._host_inclusion(z, ntop)
            full = _capi.inclusion_raw(z, ntop, gpu)
            ir.same(full, want, (name, ntop))
            for fields in (("prob",), ("joint",), ("size_pmf",), ("n_distinct",), ("top_sets", "top_count")):
                one = _capi.inclusion_raw(z, ntop, gpu, fields=fields)
                assert all((a is None) == (f not in fields) for f, a in zip(ir.FIELDS, one)), (name, fields)
                ir.same(one, want, (name, ntop, fields), fields)
        if name.startswith("every draw distinct"):
            assert full[3] == z.shape[0]
        if name.startswith("counts"):
            assert full[3] == 7 and full[5][:7].tolist() == [300, 299, 256, 255, 2, 1, 1] and not full[5][7:].any()      # ntop = 256 > n_distinct


# ------------------------------------------------------------------------------------------------------------------ the chain path
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


def _order_statistics(chains, nch, first, nsamp):
    """the (lo, hi) of every rank pair of dr.summary_ranks, from Chain.summary (one chain) or pooled_summary"""
    out = []
    for k_lo, k_hi in dr.summary_ranks(nch * nsamp):
        res = chains[0].summary(first, nsamp, k_lo, k_hi) if nch == 1 else _capi.pooled_summary(chains[:nch], first, nsamp, k_lo, k_hi)
        out.append((k_lo, k_hi, res[1], res[2]))
    return out


def _blocks(chains, call, same):
    """call() under rank_block_cols 1, 7 and 0 has the bits of call() now"""
    base = call()
    try:
        for blk in (1, 7, 0):
            chains[0].set_option("rank_block_cols", blk)
            same(base, call(), blk)
    finally:
        chains[0].set_option("rank_block_cols", 0)
    return base


@pytest.mark.parametrize("nch", (3, 1))
@pytest.mark.parametrize("first,nsamp,lag", sc.CHAIN_WINDOWS)
@pytest.mark.parametrize("k", range(sc.CHAIN_SETS))
def test_chain_order_statistics_and_hdi(chains, k, first, nsamp, lag, nch):
    """k_summary's radix select and k_hdi behind the staged columns, on the full-range rows"""
    tabs = sc.chain_tables(k)
    _load(chains, tabs)
    names = sc.chain_names(k)
    win = np.concatenate(rc.windows_of(tabs[:nch], first, nsamp), axis=0)
    gs = np.sort(win[:, :dr.Q], axis=0)

    def same_order(a, b, blk):
        for (_k, _l, lo, hi), (_m, _n, lo2, hi2) in zip(a, b):
            assert hc.same_bits(lo, lo2) and hc.same_bits(hi, hi2), blk

    for k_lo, k_hi, lo, hi in _blocks(chains, lambda: _order_statistics(chains, nch, first, nsamp), same_order):
        for j, name in enumerate(names):
            # (+ 0.0: np.sort leaves the order of -0 and +0 open, k_summary's keys put -0 first; only the rows of +-0 hold a -0)
            assert hc.same_bits(lo[j] + 0.0, gs[k_lo - 1, j] + 0.0) and hc.same_bits(hi[j] + 0.0, gs[k_hi - 1, j] + 0.0), (name, k_lo, k_hi)

    def same_hdi(a, b, blk):
        for f, x, y in zip(_capi.HDI_FIELDS, a, b):
            assert hc.same_bits(x, y), (blk, f)

    got = _blocks(chains, lambda: _capi.pooled_hdi(chains[:nch], first, nsamp, sc.LEVELS), same_hdi)
    with np.errstate(over="ignore"):
        want = api._host_hdi(np.ascontiguousarray(win.T), sc.LEVELS)
    for f, g in zip(_capi.HDI_FIELDS, got):
        for j in range(dr.Q + dr.V):
            assert hc.same_bits(g[..., j], want[f][..., j]), (names[j] if j < dr.Q else "xi %d" % (j - dr.Q), f)


def compare_every_column(got, want, wins, names, what):
    """rank_diag_cases.compare takes its numeric gamma columns from the families of the crafted tables, by index; here EVERY gamma column that
    is not constant in the ranked draws is held to RTOL in every field (the same NaN pattern, which compare has checked).  Returns how many."""
    X = np.concatenate([np.concatenate([w[:w.shape[0] // 2], w[w.shape[0] - w.shape[0] // 2:]]) for w in wins])[:, :dr.Q]
    varies = (X != X[0]).any(axis=0)
    assert not rc.degenerate(wins)[:dr.Q].any()
    for f in rc.FIELDS:
        g, w = np.asarray(got[f])[:dr.Q], np.asarray(want[f])[:dr.Q]
        if f in ("rhat", "rhat_bulk", "ess_bulk", "ess_mean", "mcse_mean"):
            assert np.isfinite(w[varies]).all() and np.isnan(w[~varies]).all(), (what, f, [names[j] for j in np.flatnonzero(~np.isfinite(w) & varies)])
        ok = ~np.isnan(w)
        with np.errstate(all="ignore"):
            rel = np.where(g[ok] == w[ok], 0.0, np.abs(g[ok] - w[ok]) / np.abs(w[ok]))
        assert rel.size == 0 or rel.max() <= rc.RTOL, (what, f, float(rel.max()), names[np.flatnonzero(ok)[np.argmax(rel)]])
    return int(varies.sum())


COMPARED = {(0, 101, 1): 136, (1, 101, 1): 130, (2, 101, 1): 110, (3, 101, 1): 134}      # (set, nsamp, chains): fewer than the 136 (135 in set 3:
                                                                                         # the row of +-0) only where 101 draws of a presorted row tie


@pytest.mark.parametrize("nch", (3, 1))
@pytest.mark.parametrize("first,nsamp,lag", sc.CHAIN_WINDOWS)
@pytest.mark.parametrize("k", range(sc.CHAIN_SETS))
def test_chain_rank_diagnostics(chains, k, first, nsamp, lag, nch):
    """k_rank behind the split halves (an odd window drops its middle row: the `gap` addressing), rows of the full exponent range moderated"""
    tabs = sc.chain_tables(k, True)
    _load(chains, tabs)
    wins = rc.windows_of(tabs[:nch], first, nsamp)
    with np.errstate(all="ignore"):
        host = rc.as_dict(api._host_rank_diagnostics(tabs[:nch], first - 1, nsamp, lag))

    def same_rank(a, b, blk):
        for f, x, y in zip(_capi.RANK_DIAG_FIELDS, a, b):
            assert hc.same_bits(x, y), (blk, f)

    _blocks(chains, lambda: _capi.pooled_rank_diag(chains[:nch], first, nsamp, lag), same_rank)
    got = rc.as_dict(api.device_rank_diagnostics(chains[:nch], first - 1, nsamp, lag))
    gaps = rc.compare(got, host, wins, (k, nch, first, nsamp, lag))
    n = compare_every_column(got, host, wins, sc.chain_names(k), (k, nch, first, nsamp, lag))
    print("sort edges, set %d, %d chain(s), window %s: %d gamma columns compared at rtol %g;" % (k, nch, (first, nsamp, lag), n, rc.RTOL),
          {f: "%.2g" % v for f, v in gaps.items()})
    assert n == COMPARED.get((k, nsamp, nch), 135 if k == 3 else 136), n
