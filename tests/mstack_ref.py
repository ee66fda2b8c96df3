"""The reference of the stacked mixture of normals of include/bnr_mstack.h in mpmath, built on mcheck_ref (its Row, its quantile check, its cases),
and the error bounds that a float64 evaluation has to meet.  Data only comes in as float64 (mean, var, the log weights normalised within every
chain, the chain weights and y); nothing here is rounded to float64 before the results are.

For one row, chains k = 0 .. K - 1 with nd draws each and chain weights w_k: the components are those of the chains with w_k > 0, in chain order
and then draw order (D+ = K+ nd of them), the weight of one  mp(w_k) exp(mp(lw_ks)).  Everything else is mcheck_ref's row on those components.

The bounds are mcheck_ref's with one more rounding per term for the product w_k exp(lw):  a weighted sum of x is bounded by
(D+ + 9) u sum w |x|,  u = 2^-52, gate 2.  (mcheck_ref.Row forms its bounds from its attribute D as (D + 8) u ...: a StackRow carries D = D+ + 1.)

elpd_stack_i = M + log sum_{k: w_k > 0} w_k exp(elpd_k - M) against mpmath: first order (K + 6) u max(1, |value|), gate 2 -- K rounded exps, K
products, K - 1 additions, one log and one addition.
"""
import functools
import math

import mpmath as mp
import numpy as np

import mcheck_ref as mc

DPS, U, GATE, SD_FLOOR, PATTERNS, CASE_ROWS = mc.DPS, mc.U, mc.GATE, mc.SD_FLOOR, mc.PATTERNS, mc.CASE_ROWS
WEIGHTS = ("uniform", "random", "unit", "zero")


class StackRow(mc.Row):
    """one row of a stacked case in mpmath: the retained components with the weights mp(w_k) exp(mp(lw)); the terms with lw < -700 are left
    out and charged as in mcheck_ref, under their chain weight"""

    def __init__(self, mean, var, logw, weights, y=None):
        w = np.asarray(weights, dtype=np.float64).reshape(-1)
        K = w.size
        lw_all = np.asarray(logw, dtype=np.float64).reshape(-1)
        nd = lw_all.size // K
        keep_cols = np.concatenate([np.arange(k * nd, (k + 1) * nd) for k in range(K) if w[k] > 0])
        with mp.workdps(DPS):
            m, v, lw = (mc._mpf(np.asarray(a, dtype=np.float64).reshape(-1)[keep_cols]) for a in (mean, var, logw))
            wk = [mp.mpf(float(w[c // nd])) for c in keep_cols]
            lwf = lw_all[keep_cols]
            Dp = len(m)
            self.Dp = Dp
            self.D = Dp + 1                                        # (D + 8) u of mcheck_ref.Row -> (D+ + 9) u: the product's rounding
            self.y = None if y is None else mp.mpf(float(y))
            keep = [s for s in range(Dp) if lwf[s] >= -700.0]
            self.dropped = mp.fsum(wk[s] * mp.exp(lw[s]) for s in range(Dp) if lwf[s] < -700.0)
            self.w = [wk[s] * mp.exp(lw[s]) for s in keep]
            self.m = [m[s] for s in keep]
            self.v = [v[s] for s in keep]
            self.s2 = [mp.sqrt(2 * x) for x in self.v]
            self.mag = max([abs(x) for x in m] + [abs(self.y) if self.y is not None else 0])
            self.vmag = max(abs(a) + b * b for a, b in zip(v, m))


def elpd_stack_ref(el, weights):
    """(elpd_stack_i, its first-order bound) of one row from the K per-chain values el and the chain weights, in mpmath"""
    el, w = np.asarray(el, dtype=np.float64).reshape(-1), np.asarray(weights, dtype=np.float64).reshape(-1)
    with mp.workdps(DPS):
        val = mp.log(mp.fsum(mp.mpf(float(wk)) * mp.exp(mp.mpf(float(e))) for e, wk in zip(el, w) if wk > 0))
        return float(val), (w.size + 6) * U * max(1.0, abs(float(val)))


# ------------------------------------------------------------------------------------------ the shared cases
def chain_weights(K, name):
    """the chain weights of a case: uniform; random on the simplex; unit = e_k with k = K // 2; zero = the random ones with chain K // 2 set to 0
    and the others divided by their sum (K = 1: every pattern is (1,))"""
    assert name in WEIGHTS
    if K == 1:
        return np.ones(1)
    rng = np.random.default_rng([187, K])
    w = rng.dirichlet(np.ones(K))
    if name == "uniform":
        w = np.full(K, 1.0 / K)
    elif name == "unit":
        w = np.zeros(K)
        w[K // 2] = 1.0
    elif name == "zero":
        w[K // 2] = 0.0
        w = w / w.sum()
    assert abs(w.sum() - 1.0) <= 1e-12
    return w


@functools.lru_cache(maxsize=None)
def case(K, nd, pattern):
    """CASE_ROWS rows of K chains with nd draws each: mcheck_ref.case(K nd, pattern)'s mean, var and y (so the point masses and the spoilt entry
    of row 1 are its), with log weights normalised within every chain: uniform -log nd; onehot one draw per chain with lw = 0 (a different one per
    row and chain), the others -800; otherwise mcheck_ref's random log weights minus the log of their sum over the chain.  nan_col: the column of
    row 1 that is spoilt (nanrow), or None -- the row is NaN only while that column's chain is retained."""
    c = mc.case(K * nd, pattern)
    D = K * nd
    logw = np.array(c["logw"])
    if pattern == "uniform":
        logw = np.full((CASE_ROWS, D), -math.log(nd))
    elif pattern == "onehot":
        logw = np.full((CASE_ROWS, D), -800.0)
        for i in range(CASE_ROWS):
            for k in range(K):
                logw[i, k * nd + (7 * i + 3 + k) % nd] = 0.0
    else:
        for k in range(K):
            blk = logw[:, k * nd:(k + 1) * nd]
            logw[:, k * nd:(k + 1) * nd] = blk - np.log(np.sum(np.exp(blk - blk.max(axis=1, keepdims=True)), axis=1, keepdims=True)) - blk.max(axis=1, keepdims=True)
    logw.setflags(write=False)
    return dict(mean=c["mean"], var=c["var"], logw=logw, y=c["y"], nan_col=(D // 2) if pattern == "nanrow" else None)


def nan_rows(K, nd, pattern, weights):
    """the rows of case(K, nd, pattern) that have to come out NaN under the chain weights"""
    col = case(K, nd, pattern)["nan_col"]
    return (1,) if col is not None and weights[col // nd] > 0 else ()


@functools.lru_cache(maxsize=None)
def case_row(K, nd, pattern, wname, i, with_y=True):
    c = case(K, nd, mc.ref_pattern(pattern))
    return StackRow(c["mean"][i], c["var"][i], c["logw"][i], chain_weights(K, wname), c["y"][i] if with_y else None)


@functools.lru_cache(maxsize=None)
def case_moments(K, nd, pattern, wname, i, with_y=True):
    return case_row(K, nd, pattern, wname, i, with_y).moments()


@functools.lru_cache(maxsize=None)
def case_pit(K, nd, pattern, wname, i):
    return case_row(K, nd, pattern, wname, i).pit()


@functools.lru_cache(maxsize=None)
def case_quantile_ok(K, nd, pattern, wname, i, t, p, width):
    return mc.quantile_ok(case_row(K, nd, pattern, wname, i), t, p, width)


def retained_columns(K, nd, weights):
    return np.concatenate([np.arange(k * nd, (k + 1) * nd) for k in range(K) if weights[k] > 0])


def check_case(K, nd, pattern, wname, rows, got, p_lo, p_hi, with_y=True):
    """the five outputs `got` (dict of mean, sd, pit, lower, upper; rows values each) of the first `rows` rows of case(K, nd, pattern) under
    chain_weights(K, wname) against the reference: mcheck_ref.check_case on the retained components"""
    c = case(K, nd, pattern)
    w = chain_weights(K, wname)
    cols = retained_columns(K, nd, w)
    cw = mc.bracket_c(p_lo, p_hi)
    bad = nan_rows(K, nd, pattern, w)
    worst = dict(mean=0.0, sd=0.0, pit=0.0, quantile=0.0)
    for i in range(rows):
        if i in bad:
            assert all(math.isnan(got[k][i]) for k in ("mean", "sd", "lower", "upper")) and (not with_y or math.isnan(got["pit"][i])), (K, nd, pattern, i)
            continue
        mo = case_moments(K, nd, pattern, wname, i, with_y)
        var_i = np.where(np.isnan(c["var"][i][cols]), mc.case(K * nd, "random")["var"][i][cols], c["var"][i][cols])   # (a spoilt entry in a dropped chain is not among cols)
        single_point = cols.size == 1 and var_i[0] == 0.0
        if not single_point:
            assert mo["sd2"] >= SD_FLOOR * mo["e2"], ("the case breaks the sd floor", K, nd, pattern, wname, i)      # (about the inputs)
        for k in ("mean", "sd"):
            if k == "sd" and single_point:
                assert got["sd"][i] == 0.0
                continue
            r = abs(got[k][i] - mo[k]) / mo["tol_" + k]
            assert math.isfinite(got[k][i]) and r <= GATE, (K, nd, pattern, wname, i, k, got[k][i], mo[k], r)
            worst[k] = max(worst[k], r)
        if with_y:
            ref, tol = case_pit(K, nd, pattern, wname, i)
            r = abs(got["pit"][i] - ref) / tol if tol > 0 else (0.0 if got["pit"][i] == ref else math.inf)
            assert r <= GATE, (K, nd, pattern, wname, i, "pit", got["pit"][i], ref, r)
            worst["pit"] = max(worst["pit"], r)
        width = mc.bracket_width(c["mean"][i][cols], var_i, cw)
        for k, p in (("lower", p_lo), ("upper", p_hi)):
            ok, viol = case_quantile_ok(K, nd, pattern, wname, i, float(got[k][i]), p, width)
            assert ok, (K, nd, pattern, wname, i, k, got[k][i], viol)
            worst["quantile"] = max(worst["quantile"], viol)
    return worst
