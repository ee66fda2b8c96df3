"""What tests/test_rank_diag_host.py and tests/test_rank_diag_gpu.py share: the windows, the crafted tables and their yardsticks (computed once),
the column sets and the comparison."""
import functools

import numpy as np

import diag_ref as dr

WINDOWS = ((38, 601, 150), (1, 640, 160), (1, 9, 4), (3, 101, 25))                # (first_row, nsamp, max_lag)
NUMERIC_FAMILIES = ("normal", "ar1", "ramp", "big_mean", "tiny")
FIELDS = ("rhat", "rhat_bulk", "rhat_tail", "ess_bulk", "ess_tail", "ess_mean", "mcse_mean")
RTOL = 1e-9                                                                       # (test_diagnostics_gpu.py's tolerance for ESS from messages)
XI1, XI4 = dr.Q + 1, dr.Q + 4


@functools.lru_cache(maxsize=None)
def tables():
    return tuple(dr.crafted_table(dr.TOT, dr.V, dr.R, chain=c) for c in range(3))


def windows_of(tabs, first, nsamp):
    return [dr.window(t, first, nsamp) for t in tabs]


def degenerate(wins):
    """columns that are constant inside every split chain but not overall: W = 0 in exact arithmetic, R-hat +Inf or astronomically large, ESS
    unspecified.  Only xi_1 (0 in chain 0, 1 elsewhere) and xi_4 (the mid-table step, where the window's halves fall on its two sides) can be."""
    import rank_diag_ref as rr
    X = rr.split_draws(wins)
    inside = np.all(X == X[:, :1, :], axis=1).all(axis=0)
    flat = X.reshape(-1, X.shape[2])
    return inside & (flat != flat[0]).any(axis=0)


def numeric_columns(wins):
    """the columns compared as numbers: the gamma families NUMERIC_FAMILIES and every xi column, without the degenerate ones"""
    cols = [j for j in range(dr.Q) if dr.family_of(j) in NUMERIC_FAMILIES] + list(range(dr.Q, dr.Q + dr.V))
    deg = degenerate(wins)
    assert set(np.flatnonzero(deg)) <= {XI1, XI4}
    return np.array([c for c in cols if not deg[c] and c not in (XI1,)]), deg


def compare(got, want, wins, what):
    """got, want: dicts of FIELDS -> (q + V,) arrays.  The NaN pattern must be identical on ALL columns outside the degenerate ones (whose ESS is
    unspecified); rtol RTOL on the numeric columns; the degenerate columns have rhat >= 1e6 or +Inf.  Returns the largest relative gap per field."""
    cols, deg = numeric_columns(wins)
    gaps = {}
    for f in FIELDS:
        g, w = np.asarray(got[f]), np.asarray(want[f])
        assert np.array_equal(np.isnan(g)[~deg], np.isnan(w)[~deg]), (what, f, np.flatnonzero(np.isnan(g) != np.isnan(w)))
        gc, wc = g[cols], w[cols]
        ok = ~np.isnan(wc)
        with np.errstate(all="ignore"):
            rel = np.abs(gc[ok] - wc[ok]) / np.abs(wc[ok])
        rel = np.where(gc[ok] == wc[ok], 0.0, rel)
        gaps[f] = float(rel.max()) if rel.size else 0.0
        assert gaps[f] <= RTOL, (what, f, gaps[f], cols[ok][np.argmax(rel)])
    for c in np.flatnonzero(deg):
        assert got["rhat"][c] >= 1e6, (what, c, got["rhat"][c])
    return gaps


def as_dict(d):
    """a RankDiagnostics as the dict of FIELDS"""
    return {f: d.full(f) for f in FIELDS}


@functools.lru_cache(maxsize=None)
def host(nchains, first, nsamp, lag):
    """the package's numpy restatement on the first `nchains` crafted tables (computed once per case)"""
    from bnr_amd import api
    return as_dict(api._host_rank_diagnostics(tables()[:nchains], first - 1, nsamp, lag))
