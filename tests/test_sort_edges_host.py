"""CPU tests of the inputs of tests/sort_cases.py (no GPU): do they tell a subtly wrong sort kernel from a right one?

1. tests/sort_emu.py, a model of bnr_sort_passes, k_rank's tie sweep, k_hdi's scan and searches and k_incl_group in the kernels' order, equals
   the plain references (scipy's rankdata, np.sort / hdi_ref.hdi, incl_ref.brute) bit for bit on every new row and on the old eight rows
   (hdi_cases.rows at every length of hdi_cases.ROW_LENGTHS).
2. With each of sort_emu.DEFECTS switched on it differs from the references on at least one new row; the table printed (pytest -s; copied to
   DESIGN.md) says for every defect whether the old eight rows alone would have shown it.  OLD_ROWS_CATCH pins that column.
3. The yardsticks of the GPU file -- api._host_hdi, api._host_inclusion, api._average_ranks -- against the same references on all new rows.
4. E_AS: the largest relative error of bnr_host_ndtri (AS 241) against Phi^-1 by mpmath at 40 digits (tests/ndtri_ref.py), over every
   argument (r - 3/8) / (S + 1/4) the GPU rows produce and over the arguments of test_rank_diag_host.test_ndtri_against_scipy.  Measured here
   as ndtri_ref.E_AS = 7.29e-16 (the figures per set are in DESIGN.md); the test holds it below twice that."""
import functools

import numpy as np
import pytest
from scipy.stats import rankdata

import hdi_cases as hc
import hdi_ref as hr
import incl_ref as ir
import ndtri_ref as nr
import sort_cases as sc
import sort_emu as se
from bnr_amd import _capi, api

E_AS = nr.E_AS                                         # 7.29e-16, measured by the two tests at the end (at S = 160 000); written into DESIGN.md
OLD_ROWS_CATCH = {1: False, 2: True, 3: True, 4: True, 5: True, 6: True}


# ------------------------------------------------------------------------------------------------------------------ references, computed once
@functools.lru_cache(maxsize=None)
def old_rows():
    """the eight rows every earlier GPU test of these kernels used, at all eleven lengths (none holds a NaN; row 5 holds +-Inf)"""
    return tuple(("old row %d, S=%d" % (i, S), r) for S in hc.ROW_LENGTHS for i, r in enumerate(hc.rows(S)))


def _levels_of(rows):
    return [(n, r, sc.LEVELS) for n, r in rows]


def _ws(lv, n):
    return [min(int(np.floor(p * n)), n - 1) for p in lv]


def hdi_want(x, lv):
    """(lower, upper, median, p_pos, p_neg) of a NaN-free row by np.sort, hdi_ref.hdi and counts; bounds and median only of a finite row"""
    n = x.size
    xs = np.sort(x + 0.0)
    p_pos, p_neg = np.count_nonzero(x > 0) / n, np.count_nonzero(x < 0) / n
    if not np.isfinite(x).all():
        return None, None, None, p_pos, p_neg
    with np.errstate(over="ignore"):
        pairs = [hr.hdi(x + 0.0, p) for p in lv]
        med = (xs[n // 2 - 1] + xs[n // 2]) / 2.0 if n >= 2 else xs[0]
    return np.array([a for a, _ in pairs]), np.array([b for _, b in pairs]), med, p_pos, p_neg


def hdi_differs(x, lv, defect):
    want = hdi_want(x, lv)
    if want[0] is None:                                                 # an infinite draw: the kernel reports the shares alone
        got = se.hdi_row(x, (), defect)
        return (got[3], got[4]) != (want[3], want[4])
    got = se.hdi_row(x, _ws(lv, x.size), defect)
    return not (all(hc.same_bits(g, w) for g, w in zip(got[:3], want[:3])) and (got[3], got[4]) == (want[3], want[4]))


def rank_differs(x, defect):
    return not np.array_equal(se.rank_row(x, defect), rankdata(x, method="average"))


def words_of(z):
    S, B = z.shape
    W = (B + 63) // 64
    pad = np.zeros((S, 64 * W), dtype=np.uint8)
    pad[:, :B] = z != 0
    return np.packbits(pad, axis=1, bitorder="little").view("<u8").reshape(S, W)


@functools.lru_cache(maxsize=None)
def incl_want(i, ntop):
    return ir.brute(sc.inclusion_cases()[i][1], ntop)


def incl_differs(i, ntop, defect):
    want = incl_want(i, ntop)
    nd, ts, tc = se.incl_group(words_of(sc.inclusion_cases()[i][1]), ntop, defect)
    return not (nd == want["n_distinct"] and np.array_equal(ts, want["top_sets"]) and np.array_equal(tc, want["top_count"]))


def new_hdi_rows():
    return [(n, r, lv) for lv, names, M in sc.hdi_matrices() for n, r in zip(names, M)]


def caught(defect, old):
    """the names of the rows (old eight, or new) on which the emulation with `defect` differs from the references, in any output the defect
    can reach: the sort's (1, 2) every output, the tie sweep's (3, 4) the ranks, the window's and the searches' (5, 6) k_hdi's"""
    ranks = old_rows() if old else sc.key_rows() + sc.tie_rows()
    hdis = _levels_of(old_rows()) if old else new_hdi_rows()
    out = []
    if defect in (1, 2, 3, 4):
        out += [n for n, r in ranks if rank_differs(r, defect)]
    if defect in (1, 2, 5, 6):
        out += [n for n, r, lv in hdis if hdi_differs(r, lv, defect)]
    if defect in (1, 2) and not old:
        out += [sc.inclusion_cases()[i][0] for i in range(len(sc.inclusion_cases())) if incl_differs(i, 4, defect)]
    return out


# ------------------------------------------------------------------------------------------------------------------ 1. the clean emulation
def test_live_pass_patterns():
    """the old rows run five shapes of live passes; the new rows add single passes at every byte, gaps and 2, 3 and 7 live passes"""
    old = {sc.live_bytes(r) for _, r in old_rows() if r.size > 1}
    assert old == {(), (6,), (6, 7), (0, 1), tuple(range(8))}, old
    new = {sc.live_bytes(r) for _, r in sc.key_rows()}
    assert new == {(b,) for b in range(8)} | set(sc.SKIP_PATTERNS), new
    print("\nlive passes of the old rows:", sorted(old), "\nlive passes of the new key rows:", sorted(new))


def test_clean_emulation_equals_the_references():
    for name, r in sc.key_rows() + sc.tie_rows() + old_rows():
        assert not rank_differs(r, None), name
    for name, r, lv in new_hdi_rows() + _levels_of(old_rows()):
        assert not hdi_differs(r, lv, None), name
    for i, (name, _z) in enumerate(sc.inclusion_cases()):
        for ntop in sc.INCL_NTOPS:
            assert not incl_differs(i, ntop, None), (name, ntop)


def test_the_sorted_data_ends_in_either_buffer():
    counts = {se.sort_passes(sc.key_of(r))[3] for _, r in sc.key_rows()}
    assert counts == {1, 2, 3, 7}, counts


# ------------------------------------------------------------------------------------------------------------------ 2. the defects
TABLE = {}


@pytest.mark.parametrize("defect", sorted(se.DEFECTS))
def test_every_defect_is_caught_by_a_new_row(defect):
    new, old = caught(defect, False), caught(defect, True)
    TABLE[defect] = (bool(old), len(new), new[0] if new else None)
    print("\ndefect %d (%s): old eight rows %s it; %d new rows catch it, the first: %s"
          % (defect, se.DEFECTS[defect], "catch" if old else "do NOT catch", len(new), new[0] if new else None))
    assert new, defect
    assert bool(old) == OLD_ROWS_CATCH[defect], (defect, old[:3])
    if defect == 1:         # every shuffled row with an odd gap whose low bytes matter (an even gap swaps back; all but byte 4: bytes 5-7 decide)
        gaps = {n for n, _ in sc.key_rows() if n.split(",")[0] in ("live bytes 02", "live bytes 35", "live bytes 037") and "shuffled" in n}
        assert len(gaps) == 30 and gaps <= set(new) and not [n for n in new if n.startswith("one live byte")]
    if defect == 5:                                                      # every planted row: its first minimum is not the lowest thread's
        assert {n for n in new if n.startswith("minimal width")} == {n for n, _r, _lv in sc.hdi_rows() if n.startswith("minimal width")}


def test_defect_table():
    if len(TABLE) < len(se.DEFECTS):
        for d in se.DEFECTS:
            TABLE.setdefault(d, (bool(caught(d, True)), len(caught(d, False)), None))
    print("\n| defect | caught by the old eight rows | new rows that catch it |\n|---|---|---|")
    for d in sorted(se.DEFECTS):
        print("| %d. %s | %s | %d |" % (d, se.DEFECTS[d], "yes" if TABLE[d][0] else "no", TABLE[d][1]))
    assert all(v[1] > 0 for v in TABLE.values())


# ------------------------------------------------------------------------------------------------------------------ 3. the GPU file's yardsticks
def test_host_rank_restatement_against_rankdata():
    for name, r in sc.key_rows() + sc.tie_rows():
        got, xs = api._average_ranks(r)
        assert np.array_equal(got, rankdata(r, method="average")) and np.array_equal(xs, np.sort(r)), name


def test_host_hdi_against_the_references():
    for lv, names, M in sc.hdi_matrices():
        with np.errstate(over="ignore"):
            got = api._host_hdi(M, lv)
        for i, (name, r) in enumerate(zip(names, M)):
            want = hdi_want(r, lv)
            for f, w in zip(hc.FIELDS, want):
                assert hc.same_bits(got[f][..., i], w), (name, f)
            assert not np.signbit(got["median"][i]) or got["median"][i] != 0.0, name            # the median may be +0 only
            for k, p in enumerate(lv):
                if r.size <= 600:
                    with np.errstate(over="ignore"):
                        assert hr.no_shorter_window(r + 0.0, p, got["lower"][k, i], got["upper"][k, i]), (name, p)


def test_host_inclusion_against_brute_force():
    for i, (name, z) in enumerate(sc.inclusion_cases()):
        for ntop in sc.INCL_NTOPS:
            ir.same(api._host_inclusion(z, ntop), incl_want(i, ntop), (name, ntop))
        want = incl_want(i, 256)
        if name.startswith("every draw distinct"):
            assert want["n_distinct"] == z.shape[0]
        if name.startswith("counts"):                                                           # ntop = 256 lies beyond n_distinct
            assert want["n_distinct"] == 7 and want["top_count"][:7].tolist() == [300, 299, 256, 255, 2, 1, 1] and not want["top_count"][7:].any()


def test_chain_tables_keep_the_live_bytes():
    """what the chain path of the GPU file sees: in the window of 601 rows every gamma column keeps the live bytes of its row (one column of
    one chain loses a byte), in the window of 101 rows the columns printed do not (presorted rows tie there), and every case still holds every
    pattern of live passes"""
    import diag_ref as dr
    import rank_diag_cases as rc
    need = {(b,) for b in range(8)} | set(sc.SKIP_PATTERNS)
    for first, nsamp, _lag in sc.CHAIN_WINDOWS:
        for nch in (3, 1):
            seen, lost = set(), []
            for k in range(sc.CHAIN_SETS):
                for moderated in (False, True):
                    win = np.concatenate(rc.windows_of(sc.chain_tables(k, moderated)[:nch], first, nsamp))
                    for j, col in enumerate(sc.chain_columns()[dr.Q * k:dr.Q * (k + 1)]):
                        lb = sc.live_bytes(win[:, j])
                        seen.add(lb)
                        if lb != sc.live_bytes(col[2 if moderated else 1]) and not moderated:
                            lost.append(col[0])
            print("\nwindow (%d, %d), %d chain(s): %d of 544 columns lose a live byte: %s" % (first, nsamp, nch, len(lost), lost))
            assert need <= seen, (first, nsamp, nch, need - seen)
            assert nsamp != 601 or len(lost) <= (nch == 1), lost
    for name, full, _mod in sc.chain_columns():                          # the placed runs are what the ranked draws hold
        if "placed for" in name:
            nch = int(name.split("placed for ")[1][0])
            first, nsamp = (38, 601) if "(38, 601)" in name else (3, 101)
            at = np.concatenate([c * 640 + sc.ranked_rows(first, nsamp) for c in range(nch)])
            heads = sc.run_heads(full[at]).tolist()
            want = np.cumsum([0] + sc._runs(sc.STAIRCASE if name.startswith("staircase") else sc.CARRY, at.size, 0 if name.startswith("staircase") else 1))
            assert heads == want[:-1].tolist(), name


# ------------------------------------------------------------------------------------------------------------------ 4. Phi^-1
def gpu_row_arguments():
    """every (r - 3/8) / (S + 1/4) that k_rank forms on the rows of the GPU file, as one sorted vector per row length"""
    return {S: (np.unique(np.stack([rankdata(r, method="average") for r in M])) - 0.375) / (S + 0.25) for S, (_n, M) in sc.rank_matrices().items()}


def _worst(p):
    return float(nr.rel_errors(p, _capi.host_ndtri(p)).max())


def test_e_as_over_the_arguments_of_the_gpu_rows():
    worst = {S: _worst(p) for S, p in gpu_row_arguments().items()}
    print("\nbnr_host_ndtri against mpmath, largest relative error per row length:", {S: "%.3g" % v for S, v in worst.items()})
    assert max(worst.values()) <= 2 * E_AS, worst


def test_e_as_over_the_arguments_of_test_ndtri_against_scipy():
    worst = {}
    for S in (2, 16, 1280, 160000):
        r = np.arange(1.0, S + 0.25, 0.5)
        worst[S] = _worst((r - 0.375) / (S + 0.25))
    worst["ends"] = _worst(np.array([1e-300, 1e-17, 1.0 - 2.0 ** -53]))
    print("\nbnr_host_ndtri against mpmath, largest relative error per set:", {k: "%.3g" % v for k, v in worst.items()})
    assert max(worst.values()) <= 2 * E_AS, worst
