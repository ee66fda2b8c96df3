"""Host tests of the exact reference of the marginal kernels (tests/mexact_ref.py; DESIGN.md section 8, "Exact references of the marginal kernels"):
the report of the any-order condition at every shape the GPU file uses; a float64 emulation of the kernels, written in the order their headers
document (left-looking Cholesky, k ascending, rows ascending, the lane groups' ((t0 + t1) + t2) + t3), that has to reproduce the exact values bit
for bit; the numpy restatements of api.py inside their existing bounds on these inputs; and a set of mutants of the emulation, each of which has to
change at least one checked bit at every shape it can affect -- with the verdict of the bound-based gates on the same mutants printed beside it.

The shapes past 256 rows and what first runs there.  The factor kernel forms L^-1 in passes of 256 columns (i0 = 0, 256, 512), every k loop of a
pass from i0, unrolled by 8, selecting 0.0 for k < i; in the Cholesky a thread owns the rows j + tid, j + tid + 256, ...
  257  the second pass exists: one column, both of its k loops run zero times (pass2_i0 is all it can show)
  258  the first second-pass column with a k < i: the select of the pass meets a slot that holds an entry of L (bound-based GPU files)
  265  the second pass has nine columns: row 264 runs one full unrolled chunk, k = 256 .. 263, all eight terms non-zero in column 256; the rows
       before it the remainder loop; the Cholesky's second row of a thread (row 264, columns 4, 6, 8) gets a non-zero update
  513  the third pass exists, with one column (bound-based GPU files)
  521  the third pass has nine columns and its full chunk, k = 512 .. 519; the second pass is full (256 columns, every lane of it); the
       Cholesky's third row of a thread (row 520) gets a non-zero update
test_the_passes_behind_the_first_carry_data asserts this from the integer L and M of the reference, and
test_the_old_shapes_let_the_pass_mutants_through that n = 257 shows none of pass_mask_off, pass_k_chunk and chol_two_rows.

The mutants, as the emulation states them:
  mask_lt      i < r instead of i <= r in the mask of M in the projection kernels
  mask_off     the mask removed: a slot with i > r holds L[i][r + 1]
  kend_16rt    the K loop of a row tile stops at 16 rt instead of behind the tile's diagonal
  gram_tail    the Gram's last partial K step dropped
  gram_swap    ti and tj swapped where the Gram stores a tile (the lower off-diagonal tiles stay 0.0)
  m_noshift    M read without its one-column shift: slot (r, i) is M[r - 1][i] below the diagonal and L[r][r] on it
  c_skip_diag  c_i summed from r = i + 1
  pass2_i0     the second 256-column pass of the factor kernel works on the first pass's columns: c and g of the columns from 256 on are never formed
  pass3_i0     the third pass works on the second pass's columns: c and g of the columns from 512 on are never formed (n > 512)
  pass_mask_off  in the passes i0 >= 256 of the factor kernel the select k >= i is dropped: slot (k, i) with k < i contributes L[i][k + 1] (n >= 258)
  pass_k_chunk   in the passes i0 >= 256 the first full chunk of 8 of the k loop is skipped: a row rr >= i0 + 8 starts at k = i0 + 8 (n >= 265)
  chol_two_rows  the Cholesky's update loop handles the rows j + tid and j + tid + 256 only: L[rr][j] = A[rr][j] / L[j][j] for rr >= j + 512 (n >= 514)
and two of the size the bound-based gates were not made for, a float32 where a float64 belongs:
  c_f32        c_i passes through a float32 before the two divisions
  t_f32        the four lane groups' parts of t pass through a float32 before they are added
"""
import functools
import math

import numpy as np
import pytest

import mcov_ref as cr
import medge_ref as er
import mexact_ref as mx
import mloo_ref as mr
import mpred_ref as pr
from bnr_amd import api

SHAPES = tuple(mx.SHAPES)
GRAM_MUTANTS = ("gram_tail", "gram_swap")
FACTOR_MUTANTS = ("c_skip_diag", "pass2_i0", "c_f32", "pass_mask_off", "pass_k_chunk", "pass3_i0", "chol_two_rows")
PASS_MUTANTS = FACTOR_MUTANTS[3:]
PROJ_MUTANTS = ("mask_lt", "mask_off", "kend_16rt", "m_noshift", "t_f32")
MUTANTS = PROJ_MUTANTS + GRAM_MUTANTS + FACTOR_MUTANTS
LOG_2PI = 1.8378770664093454835606594728112


# ------------------------------------------------------------------------------------------ the emulation
def _gram_sum(X, S, Xj, q):
    """sum_e (x_ie S_e) x'_je, e ascending, one accumulator per entry (columns with S_e = 0 add 0.0)"""
    acc = np.zeros((X.shape[0], Xj.shape[0]))
    for e in range(q):
        if S[e] == 0.0:
            continue
        ni, nj = np.nonzero(X[:, e])[0], np.nonzero(Xj[:, e])[0]
        acc[np.ix_(ni, nj)] += (X[ni, e] * S[e])[:, None] * Xj[nj, e][None, :]
    return acc


@functools.lru_cache(maxsize=None)
def emu_gram(n, d, mutant=None):
    """k_mloo_gram: the draw's np x np storage, lower 32 x 32 tiles only, the identity added to the finished sums"""
    c = mx.inputs(n)
    q = c["q"]
    npad = -(-n // 32) * 32
    acc = np.zeros((npad, npad))
    acc[:n, :n] = _gram_sum(c["X"], c["S"][d], c["X"], q - q % 32 if mutant == "gram_tail" else q)
    acc += np.eye(npad)
    G = np.zeros((npad, npad))
    for ti in range(npad // 32):
        for tj in range(ti + 1):
            a, b = (tj, ti) if mutant == "gram_swap" else (ti, tj)
            G[a * 32:(a + 1) * 32, b * 32:(b + 1) * 32] = acc[ti * 32:(ti + 1) * 32, tj * 32:(tj + 1) * 32]
    return G


@functools.lru_cache(maxsize=None)
def emu_factor(n, d, gram=None, mutant=None):
    """k_mloo_rhs and k_mloo_factor over emu_gram(n, d, gram): dict of L, z, M, c, g and the four outputs"""
    c = mx.inputs(n)
    A = emu_gram(n, d, gram)[:n, :n]
    t2, mu = float(c["tau2"][d]), float(c["mu"][d])
    acc = np.zeros(n)
    for e in range(c["q"]):
        acc = acc + c["X"][:, e] * c["W"][d][e]
    r = (c["y"] - mu) - acc
    L, z = np.zeros((n, n)), np.zeros(n)
    sumlog = zz = 0.0
    for j in range(n):
        s = A[j:, j].copy()
        zrow = r[j]
        for k in range(j):
            s = s - L[j:, k] * L[j, k]
            zrow = zrow - z[k] * L[j, k]
        if mutant == "chol_two_rows":
            s[512:] = A[j + 512:, j]
        if not s[0] > 0.0:
            return None                                                  # (a bad draw: NaN everywhere on the device)
        sd = math.sqrt(s[0])
        sumlog = sumlog + math.log(sd)
        L[j, j] = sd
        L[j + 1:, j] = s[1:] / sd
        z[j] = zrow / sd
        zz = zz + z[j] * z[j]
    M, cc, g = np.zeros((n, n)), np.zeros(n), np.zeros(n)
    for i0 in range(0, n, 256):                                          # a pass: the columns i0 .. i1 - 1, one lane each, every k loop from i0
        i1, far = min(i0 + 256, n), i0 >= 256
        cols = np.arange(i0, i1)
        for rr in range(i0, n):
            sv = (cols == rr).astype(np.float64)
            k0 = i0 + 8 if mutant == "pass_k_chunk" and far and i0 + 8 <= rr else i0
            for k in range(k0, rr):
                mk = M[k, i0:i1]                                         # (0.0 in the columns i > k: the select)
                if mutant == "pass_mask_off" and far:
                    mk = np.where(cols > k, L[cols, k + 1], mk)
                sv = sv - L[rr, k] * mk
            w = min(rr + 1, i1) - i0                                     # the columns i <= rr of the pass
            x = sv[:w] / L[rr, rr]
            M[rr, i0:i0 + w] = x
            wc = w - 1 if mutant == "c_skip_diag" and rr < i1 else w
            cc[i0:i0 + wc] = cc[i0:i0 + wc] + x[:wc] * x[:wc]
            g[i0:i0 + w] = g[i0:i0 + w] + x * z[rr]
    if mutant in ("pass2_i0", "pass3_i0"):
        cc[256 if mutant == "pass2_i0" else 512:] = 0.0
        g[256 if mutant == "pass2_i0" else 512:] = 0.0
    if mutant == "c_f32":
        cc = cc.astype(np.float32).astype(np.float64)
    with np.errstate(all="ignore"):
        resid, var = g / cc, t2 / cc
        loglik = -0.5 * (LOG_2PI + np.log(var)) - 0.5 * ((resid * resid) / var)
    logml = -(0.5 * n) * (LOG_2PI + math.log(t2)) - sumlog - 0.5 * (zz / t2)
    return dict(A=A, r=r, L=L, z=z, zz=zz, M=M, c=cc, g=g, resid=resid, var=var, loglik=loglik, logml=logml)


def _a_operand(M, L, n, mutant):
    """the A operand of the projection kernels' MFMAs: slot (r, i) of the rows r < 16 ceil(n / 16) and the K range of row tile r / 16"""
    nr, npad = -(-n // 16) * 16, -(-n // 32) * 32
    r, i = np.arange(nr)[:, None], np.arange(npad)[None, :]
    Mp, Lt, Ms, Ld = np.zeros((nr, npad)), np.zeros((nr, npad)), np.zeros((nr, npad)), np.zeros((nr, npad))
    Mp[:n, :n] = M
    Lt[:n - 1, :n] = L[:, 1:].T                                          # slot (r, i), i > r: L[i][r + 1]
    Ms[1:n, :n] = M[:n - 1]                                              # without the shift: M[r - 1][i]
    Ld[np.arange(n), np.arange(n)] = np.diag(L)
    kend = (r // 16 + 1) * 16
    if mutant == "mask_lt":
        a = np.where(i < r, Mp, 0.0)
    elif mutant == "mask_off":
        a = np.where(i <= r, Mp, Lt)
    elif mutant == "kend_16rt":
        a = np.where((i <= r) & (i < kend - 16), Mp, 0.0)
    elif mutant == "m_noshift":
        a = np.where(i < r, Ms, np.where(i == r, Ld, 0.0))
    else:
        a = np.where(i <= r, Mp, 0.0)
    return np.where((r < n) & (i < -(-kend // 32) * 32), a, 0.0)


def _project(a, cols, n, f32=False):
    """T = a cols, one accumulator per entry, i ascending; t: lane group g sums the squares of rows 16 rt + g + 4 j (j, then rt ascending); the four
    groups as ((t0 + t1) + t2) + t3"""
    T = np.zeros((a.shape[0], cols.shape[1]))
    for i in range(n):
        T += a[:, i][:, None] * cols[i][None, :]
    ts = np.zeros((4, cols.shape[1]))
    for rt in range(a.shape[0] // 16):
        for j in range(4):
            for g in range(4):
                ts[g] = ts[g] + T[16 * rt + g + 4 * j] * T[16 * rt + g + 4 * j]
    if f32:
        ts = ts.astype(np.float32).astype(np.float64)
    return T, ((ts[0] + ts[1]) + ts[2]) + ts[3]


@functools.lru_cache(maxsize=None)
def emu_cross(n, d):
    c = mx.inputs(n)
    return _gram_sum(c["X"], c["S"][d], c["Xn"], c["q"])


@functools.lru_cache(maxsize=None)
def emulate(n, d, mutant=None):
    """every checked output of draw d under one mutant (None: the kernels as documented)"""
    c = mx.inputs(n)
    f = emu_factor(n, d, mutant if mutant in GRAM_MUTANTS else None, mutant if mutant in FACTOR_MUTANTS else None)
    if f is None:
        nan = np.full(n, np.nan)
        return dict(resid=nan, var=nan, loglik=nan, logml=np.nan, v=None, m=None, pvar=None, pmean=None)
    idx = mx.edges_checked(n)
    t2, mu, S, W = float(c["tau2"][d]), float(c["mu"][d]), c["S"][d], c["W"][d]
    a = _a_operand(f["M"], f["L"], n, mutant if mutant in PROJ_MUTANTS else None)
    with np.errstate(all="ignore"):
        gi = f["resid"] * (t2 / f["var"])
        Xs = c["X"][:, idx]
        _T, t = _project(a, Xs, n, mutant == "t_f32")
        p = np.zeros(len(idx))
        for i in range(n):
            p = p + Xs[i] * gi[i]
        m = W[idx] + S[idx] * p
        v = (t2 * S[idx]) * np.fmax(1.0 - S[idx] * t, 0.0)
        C = emu_cross(n, d)
        _T, tj = _project(a, C, n, mutant == "t_f32")
        aj, dj, h = np.zeros(c["m"]), np.zeros(c["m"]), np.zeros(c["m"])
        for e in range(c["q"]):
            xv = c["Xn"][:, e]
            aj = aj + xv * W[e]
            dj = dj + (xv * S[e]) * xv
        for i in range(n):
            h = h + C[i] * gi[i]
        pvar = t2 * np.fmax(dj - tj, 0.0)
        pmean = (mu + aj) + h
    out = dict(f)
    out.update(v=v, m=m, t=t, pvar=pvar, pmean=pmean, C=C, a=aj, dq=dj)
    return out


def _differs(got, want, mask=None):
    if got is None:
        return True
    mask = np.ones(np.shape(want), dtype=bool) if mask is None else mask
    return bool(np.any(~(np.asarray(got)[mask] == np.asarray(want)[mask])))


# ------------------------------------------------------------------------------------------ the report
@pytest.mark.parametrize("n", SHAPES)
def test_the_report_holds_at_every_shape(n):
    c = mx.inputs(n)
    q = c["q"]
    assert (q % 32 == 0) if mx.SHAPES[n]["qmod32"] == 0 else (q % 4 != 0 and q % 32 != 0)
    tail = [e for e in range(q - q % 32 if q % 32 else q - 32, q)]
    checked = mx.edges_checked(n)
    if len(checked) < q:
        assert len(checked) >= 2000
        rows = mx.edge_rows(n)
        assert set(mx.ROWS_257) | {n - 1} <= set(rows) and (n <= 512 or {511, 512} <= set(rows))
        hit = {e for e, key in enumerate(c["keys"]) if key is not None and (key[0] in rows or key[1] in rows)}
        assert hit <= set(checked.tolist())
    else:
        assert n <= 65 or q <= 2 * mx.SAMPLE_257
    for row in mx.summary(n):
        d = row["d"]
        print("n=%d q=%d draw %d: %s" % (n, q, d, {k: v for k, v in row.items() if k != "d"}))
        assert row["A"] and row["r"] and row["L"] and row["M"] and row["z"], row      # every sum of the Gram, the right-hand side and the factor
        assert row["mloo"] == n, row                                     # c and g of every row: resid and var are one division of exact operands
        assert row["v_live_ok"] >= 0.95 * row["live"] and row["live"] >= min(n, 2), row
        assert row["pred_ok"] >= 0.9 * row["m"], row
        if n > 257:
            assert row["v_ok"] >= 0.99 * row["edges"] and row["pred_ok"] >= 0.99 * row["m"], row
        assert np.any(c["S"][d][tail] != 0) or n == 1, "no live column in the last K step of the Gram"
        assert 0.0 <= row["density"] <= 1.0
    for ncols in ((127, 128, 129) if n in (17, 33) else (129,) if n in COV_MIX else ()):
        w, ok = mx.within(n, _cov_cols(n, ncols), *COV_MIX[n])
        off = ok & (w != 0) & ~np.eye(ncols, dtype=bool)
        print("n=%d within at %d columns: %d of %d entries exact, %d of them off the diagonal and not 0" % (n, ncols, ok.sum(), ok.size, off.sum()))
        assert ok.sum() >= 0.99 * ok.size and off.sum() >= (1000 if n <= 33 else 1) and np.array_equal(w, w.T)


# (K, nd, dyadic chain weights) of the covariance cases
COV_MIX = {17: (2, 4, (0.25, 0.75)), 33: (1, 4, (1.0,)), 265: (1, 1, (1.0,)), 521: (1, 1, (1.0,))}


def _pass_conditions(n, d):
    """What draw d gives the loops of the factor kernel that first run past 256 rows, from the integer L and M of the reference.  Per pass
    i0 >= 256: terms, the most non-zero terms L[rr][k] M[k][i], k >= i0, of one (rr, i); chunk, the (rr, i) whose first full chunk k = i0 .. i0 + 7
    has eight non-zero terms; slots, the (k, i), i0 <= k < i, whose slot L[i][k + 1] is not 0 and meets a non-zero L[rr][k] of a row rr >= i.
    cols: the columns i >= 256 with a non-zero M[rr][i] below the diagonal.  chol: per offset 256, 512 the entries (rr, j), rr >= j + offset,
    whose Cholesky update has a non-zero term L[rr][k] L[j][k]."""
    L = mx.inputs(n)["facs"][d][2]
    nzL = np.tril(L != 0, -1).astype(np.int64)
    nzM = (mx.draw(n, d)["Mi"] != 0).astype(np.int64)
    out = dict(passes={}, cols=sum(1 for i in range(256, n) if nzM[i + 1:, i].any()), chol={})
    for i0 in range(256, n, 256):
        i1 = min(i0 + 256, n)
        terms = int((nzL[:, i0:] @ nzM[i0:, i0:i1]).max())
        chunk = int((nzL[i0 + 8:, i0:i0 + 8] @ nzM[i0:i0 + 8, i0:i1] == 8).sum()) if n >= i0 + 9 else 0
        slots = sum(1 for i in range(i0 + 1, i1) for k in range(i0, i) if L[i, k + 1] != 0 and nzL[i:, k].any())
        out["passes"][i0] = dict(terms=terms, chunk=chunk, slots=slots)
    for off in (256, 512):
        out["chol"][off] = sum(int(((nzL[j + off:, :j] * nzL[j, :j][None, :]).sum(axis=1) > 0).sum()) for j in range(1, n - off))
    return out


@pytest.mark.parametrize("n", tuple(s for s in SHAPES if s > 257))
def test_the_passes_behind_the_first_carry_data(n):
    for d in range(mx.inputs(n)["D"]):
        cond = _pass_conditions(n, d)
        print("n=%d draw %d: %r" % (n, d, cond))
        assert set(cond["passes"]) == set(range(256, n, 256))
        for i0, p in cond["passes"].items():
            assert p["terms"] >= 8 and p["chunk"] >= 1, (n, i0, p)             # (a) a full unrolled chunk of every pass carries data
            assert p["slots"] >= 1, (n, i0, p)                                 # (c) a missing select reads a non-zero entry of L
        assert cond["cols"] >= 8, cond                                         # (b)
        assert cond["chol"][256] >= 1 and (n <= 512 or cond["chol"][512] >= 1), cond      # (d)


def _cov_cols(n, ncols):
    return tuple(int(v) for v in np.random.default_rng([53, n, ncols]).choice(mx.inputs(n)["q"], size=ncols, replace=False))


# ------------------------------------------------------------------------------------------ the emulation against the exact values
@pytest.mark.parametrize("n", SHAPES)
def test_the_emulation_in_the_documented_order_gives_the_exact_bits(n):
    c = mx.inputs(n)
    for d in range(c["D"]):
        ex, ed, pd, em = mx.draw(n, d), mx.edges(n, d), mx.predict(n, d), emulate(n, d)
        assert np.array_equal(np.tril(em["A"]), np.tril(ex["A"])), (n, d, "A")             # (the Gram stores the lower tiles only)
        for k in ("L", "M", "z", "c", "g", "r", "resid", "var"):
            assert np.array_equal(em[k], ex[k]), (n, d, k)
        if ex["report"]["zz"]:
            assert em["zz"] == ex["zz"]
        assert np.array_equal(em["t"][ed["t_ok"]], ed["t"][ed["t_ok"]])
        assert np.array_equal(em["v"][ed["ok"]], ed["v"][ed["ok"]]), (n, d, "v")
        assert np.array_equal(em["C"], pd["C"]) and np.array_equal(em["a"], pd["a"]) and np.array_equal(em["dq"], pd["dq"])
        assert np.array_equal(em["pvar"][pd["ok"]], pd["var"][pd["ok"]]), (n, d, "pvar")


# ------------------------------------------------------------------------------------------ the restatements of api.py inside their bounds
@pytest.mark.parametrize("n", tuple(s for s in SHAPES if s <= 65))
def test_the_host_restatements_stay_inside_their_bounds(n):
    c = mx.inputs(n)
    D = c["D"]
    h = api._host_marginal_terms(c["X"], c["y"], c["tau2"], c["mu"], c["S"], c["W"])
    hm, hv, nb = api._host_gamma_terms(c["X"], c["y"], c["tau2"], c["mu"], c["S"], c["W"])
    pm, pv, nb2 = api._host_predict_terms(c["X"], c["y"], c["Xn"], c["tau2"], c["mu"], c["S"], c["W"])
    assert h[4] == 0 and nb == 0 and nb2 == 0
    for d in range(D):
        ex, ed, pd, em = mx.draw(n, d), mx.edges(n, d), mx.predict(n, d), emulate(n, d)
        args = (c["X"], c["y"], c["tau2"][d], c["mu"][d], c["S"][d], c["W"][d])
        b = mr.numpy_bounds(*args)
        assert np.all(np.abs(h[1][:, d] - ex["resid"]) <= 2 * b["tol_resid"]) and np.all(np.abs(h[2][:, d] - ex["var"]) <= 2 * b["tol_var"])
        be = er.numpy_bounds(*args)
        idx, ok = ed["idx"], ed["ok"]
        assert np.all(er.ratio(hv[d][idx][ok], ed["v"][ok], be["tol_v"][idx][ok]) <= 2.0)
        assert np.all(er.ratio(hm[d][idx], em["m"], be["tol_m"][idx]) <= 2.0)
        bp = pr.numpy_bounds(c["X"], c["y"], c["Xn"], c["tau2"][d], c["mu"][d], c["S"][d], c["W"][d])
        assert np.all(er.ratio(pv[d][pd["ok"]], pd["var"][pd["ok"]], bp["tol_var"][pd["ok"]]) <= 2.0)
        assert np.all(er.ratio(pm[d], em["pmean"], bp["tol_mean"]) <= 2.0)


def test_the_host_covariance_stays_inside_its_bound():
    n, ncols = 17, 127
    K, nd, w = COV_MIX[n]
    c = mx.inputs(n)
    cols = _cov_cols(n, ncols)
    D = K * nd
    got = api._host_gamma_cov_terms(c["X"], c["y"], c["tau2"][:D], c["mu"][:D], c["S"][:D], c["W"][:D], K, np.array(cols), list(w))
    ref = cr.mixture([cr.numpy_draw(c["X"], c["y"], c["tau2"][d], c["mu"][d], c["S"][d], c["W"][d]) for d in range(D)], n, K, nd, cols, w)
    ew, ok = mx.within(n, cols, K, nd, w)
    assert np.all(er.ratio(got[2][ok], ew[ok], ref["tol_within"][ok]) <= 2.0)


# ------------------------------------------------------------------------------------------ the mutants
def _affects(mutant, n, q):
    return not ((mutant == "mask_off" and n < 2) or (mutant == "gram_tail" and q % 32 == 0) or (mutant == "gram_swap" and n <= 32)
                or (mutant == "pass2_i0" and n <= 256) or (mutant in ("c_f32", "t_f32") and n < 16)
                or (mutant == "pass_mask_off" and n < 258) or (mutant == "pass_k_chunk" and n < 265) or (mutant == "pass3_i0" and n <= 512)
                or (mutant == "chol_two_rows" and n < 514))


def _caught(n, d, mutant):
    """whether the mutant changes a bit that the GPU file checks at draw d: resid and var of every row, v of the exact edges, var of the exact rows"""
    ex, ed, pd, em = mx.draw(n, d), mx.edges(n, d), mx.predict(n, d), emulate(n, d, mutant)
    return (_differs(em["resid"], ex["resid"]) or _differs(em["var"], ex["var"]) or _differs(em["v"], ed["v"], ed["ok"])
            or _differs(em["pvar"], pd["var"], pd["ok"]))


def _old_gate(n, d, mutant):
    """the largest error / bound of the mutant's outputs under the tolerances of mloo_ref and medge_ref (the gate is 2), against the exact values"""
    c = mx.inputs(n)
    ex, ed, base, em = mx.draw(n, d), mx.edges(n, d), emulate(n, d), emulate(n, d, mutant)
    args = (c["X"], c["y"], c["tau2"][d], c["mu"][d], c["S"][d], c["W"][d])
    b, be = mr.numpy_bounds(*args), er.numpy_bounds(*args)
    idx = ed["idx"]
    if em["v"] is None:
        return np.inf
    worst = 0.0
    for k in ("resid", "var", "loglik"):
        worst = max(worst, float(np.max(er.ratio(em[k], base[k], b["tol_" + k]))))
    worst = max(worst, float(er.ratio(np.array([em["logml"]]), np.array([base["logml"]]), np.array([b["tol_logml"]]))[0]))
    worst = max(worst, float(np.max(er.ratio(em["v"], np.where(ed["ok"], ed["v"], base["v"]), be["tol_v"][idx]))))
    return max(worst, float(np.max(er.ratio(em["m"], base["m"], be["tol_m"][idx]))))


@pytest.mark.parametrize("n", SHAPES)
def test_every_mutant_changes_a_checked_bit(n):
    c = mx.inputs(n)
    for mutant in MUTANTS:
        if not _affects(mutant, n, c["q"]):
            continue
        hits = [_caught(n, d, mutant) for d in range(c["D"])]
        # (a float32 mutant shows only where a value has more than 24 bits: at some draw of every shape, not at every draw)
        assert any(hits) if mutant in ("c_f32", "t_f32") else all(hits), (n, mutant, hits)
    assert not any(_caught(n, d, None) for d in range(c["D"]))


def test_the_old_shapes_let_the_pass_mutants_through():
    """what the shapes up to n = 257 could not show: there the emulation under each of these mutants is the emulation, bit for bit"""
    for mutant in ("pass_mask_off", "pass_k_chunk", "chol_two_rows"):
        assert not _affects(mutant, 257, mx.inputs(257)["q"]) and not _caught(257, 0, mutant), mutant
        base, em = emulate(257, 0), emulate(257, 0, mutant)
        assert all(np.array_equal(em[k], base[k]) for k in ("L", "z", "M", "c", "g", "resid", "var", "loglik", "v", "m", "pvar", "pmean")), mutant
    assert all(_affects(m, n, mx.inputs(n)["q"]) for m in ("pass_mask_off", "pass_k_chunk") for n in SHAPES if n > 257)
    assert _affects("pass3_i0", 521, 0) and _affects("chol_two_rows", 521, 0)


def test_the_mutants_under_the_bound_based_gates():
    """The table of DESIGN.md: per mutant the largest error / bound under the old tolerances over the draws of n = 17 and n = 33 (the shapes of the
    mpmath gate of 2), and at how many of the draws that gate lets the mutant pass; for the mutants of the passes behind the first, which reach
    neither, the same at the first exact shape past 256 rows that they reach.  Recorded, not asserted: it measures the gap, the test above closes
    it."""
    print("%-14s %-30s %-30s %s" % ("mutant", "n=17: worst err/bound, passes", "n=33: worst err/bound, passes", "past 256 rows (the pass mutants)"))
    through = []
    for mutant in MUTANTS:
        cells = []
        # (a pass mutant reaches neither 17 nor 33: its third cell is the first shape past 256 rows that it reaches)
        for n in (17, 33) + ((265 if mutant in ("pass_mask_off", "pass_k_chunk") else 521,) if mutant in PASS_MUTANTS else ()):
            c = mx.inputs(n)
            if not _affects(mutant, n, c["q"]):
                cells.append("not reached")
                continue
            w = [_old_gate(n, d, mutant) for d in range(c["D"])]
            npass = sum(1 for v in w if v <= 2.0)
            cells.append("%s%.3g, %d of %d draws" % ("n=%d: " % n if n > 33 else "", max(w), npass, len(w)))
            through += [(mutant, n, npass)] if npass else []
        print("%-14s %-30s %-30s %s" % (mutant, *cells, *([""] if len(cells) == 2 else [])))
    print("let through by the old gates (mutant, n, draws):", through)
