"""Draws of the marginal libraries whose every intermediate is a float64, and their exact reference in Python integers (DESIGN.md section 8,
"Exact references of the marginal kernels").

The construction.  L = diag(2^k_i) + N with N a strictly lower triangle of small integers: a few dense columns at the edges of the 16- and 32-row
tiles and of the factor kernel's 256-column passes, a dense last row and, at the small shapes, random extras.  A = L L^T is an integer matrix
whose Cholesky factor is L: the pivots are 4^k_i, so sqrt and every division by a pivot are exact.  The k_i are raised until P = A - I is diagonally dominant; then
    P = sum_{i>j} |P_ij| (e_i +- e_j)(e_i +- e_j)^T + sum_i (P_ii - sum_j |P_ij|) e_i e_i^T = X diag(S) X^T
with X in {0, +-1} and integer S >= 0.  The draws of a shape share one X, the union of the columns any of them needs; S selects.  On top of that:
a value of S is split over several columns in chunks of CH significant bits (so that S_e t_e keeps few bits), a column is scaled (x_e 2^a, S_e 4^-a,
a in {-1, 0, 1}), columns of small integers with S = 0 in every draw pad q to the residue chosen, and a seeded permutation puts live columns into the
last partial step of every K loop.  y, W are small integers, mu a multiple of 1/2, tau2 a power of 4; a new row holds one to three small integers.

The any-order condition.  A sum whose terms are all multiples of 2^-E with sum |terms| < 2^(53 - E) is exact in every order: every partial sum of
every order is a multiple of 2^-E below 2^53 2^-E, hence a float64, and so is every term (a product, fused into the sum or rounded first).  Where
the condition holds the expected bits do not depend on the order of the tiles, of the K loop or inside an MFMA.  Everything below is computed in
Python integers on power-of-two scales (value = integer / 2^scale); nothing is rounded before the final conversion, and the report says for every
sum the device forms whether the condition holds.  A single operation (a product, a difference) is exact where its exact result is a float64.

For the tests: SHAPES, inputs(n), draw(n, d), edges_checked(n), edges(n, d), predict(n, d), within(n, cols, K, nd, weights) and summary(n), all cached."""
import functools
import math
from fractions import Fraction

import numpy as np

CH = 5                                                                   # significant bits of S per column
ROWS_257 = (0, 1, 15, 16, 31, 32, 255, 256)                              # large q: every edge incident to these rows (edge_rows) is checked, plus a sample
SAMPLE_257 = 600

# per n: draws of the pool, dense columns of N, random extras of N (spots: placed ones), q mod 32 (None: the next q with q mod 4 != 0), new rows
SHAPES = {
    1: dict(draws=1, dense=(), extras=0, qmod32=0, m=1),
    2: dict(draws=5, dense=(0,), extras=0, qmod32=None, m=1),
    16: dict(draws=9, dense=(0, 8), extras=6, qmod32=0, m=33),
    17: dict(draws=9, dense=(0, 15), extras=8, qmod32=None, m=33),
    32: dict(draws=5, dense=(0, 15, 16), extras=8, qmod32=None, m=33),
    33: dict(draws=5, dense=(0, 15, 16, 31), extras=10, qmod32=None, m=129),
    65: dict(draws=1, dense=(0, 31, 32), extras=0, qmod32=None, m=33),
    257: dict(draws=1, dense=(0, 255), extras=0, qmod32=None, m=129),
    # past the factor kernel's first 256-column pass (test_marginal_exact_host.test_the_passes_behind_the_first_carry_data): the dense column at a
    # pass's first column and the dense last row, nine rows behind it, fill one unrolled chunk of eight of that pass; the placed extras in the
    # first rows give the Cholesky non-zero updates of the last row, 256 and 512 rows below its column.  Column 0 is left out: with it and two
    # more dense columns no attempt reaches the any-order condition at these sizes.
    265: dict(draws=1, dense=(255, 256, 263), extras=0, spots=((4, 3), (6, 5), (8, 7)), qmod32=None, m=33),
    521: dict(draws=1, dense=(256, 512), extras=0, spots=((4, 3), (6, 5), (8, 7)), qmod32=None, m=33),
}
TWO53 = 1 << 53


# ------------------------------------------------------------------------------------------ integers on a power-of-two scale
def _tz(o):
    return (o & -o).bit_length() - 1


def _anyorder(sabs, orr):
    """the any-order condition of a sum whose terms (integers on one scale) have the absolute sum sabs and the bitwise or of magnitudes orr"""
    return orr == 0 or (sabs >> _tz(orr)) < TWO53


def _rep(v):
    """whether the integer v (on any power-of-two scale) is a float64"""
    v = abs(int(v))
    return v == 0 or (v >> _tz(v)) < TWO53


def _f(v, scale):
    """integer / 2^scale as a float64 (exact where _rep(v); rounded, and then never compared, elsewhere)"""
    return math.ldexp(float(int(v)), -scale)


def _farr(a, scale):
    return np.array([_f(v, scale) for v in np.asarray(a, dtype=object).reshape(-1)], dtype=np.float64).reshape(np.shape(a))


def _sum_check(terms, axis):
    """(the sums, whether each meets the any-order condition) of an object array of integer terms along axis"""
    mag = np.abs(terms)
    s, sa, o = terms.sum(axis=axis), mag.sum(axis=axis), np.bitwise_or.reduce(mag, axis=axis)
    ok = np.array([_anyorder(int(a), int(b)) for a, b in zip(np.reshape(sa, -1), np.reshape(o, -1))], dtype=bool).reshape(np.shape(s))
    return s, ok


def _chunks(v):
    out = []
    while v:
        hb = v.bit_length()
        c = v if hb <= CH else (v >> (hb - CH)) << (hb - CH)
        out.append(c)
        v -= c
    return out


# ------------------------------------------------------------------------------------------ the generator
def _factor(n, spec, d, attempt):
    """(N, k, L, P) of draw d: the strictly lower integer part and the exponents of the diagonal, raised until P = L L^T - I is diagonally
    dominant.  The dependency depth of L^-1 is limited: with more than three dense columns a draw leaves one of them out (draw d the column
    d mod len(dense); the union over the draws has them all), and an extra sits in an odd column and an even row outside the dense columns and
    the last row, so that no two extras chain."""
    rng = np.random.default_rng([41, n, d, attempt])
    N = np.zeros((n, n), dtype=np.int64)
    dense = [c for c in spec["dense"] if c < n - 1]
    if len(dense) > 3:
        dense = [c for t, c in enumerate(dense) if t != d % len(dense)]
    for c in dense:
        N[c + 1:, c] = rng.choice([-2, -1, 1, 1, 2] if n <= 33 and attempt == 0 else [-1, 1], size=n - 1 - c)
    if n >= 2:
        N[n - 1, :n - 1] = rng.choice([-1, 1], size=n - 1)
    odd = [c for c in range(1, n - 1, 2) if c not in spec["dense"]]
    for _ in range(spec["extras"] if attempt < 3 else 0):
        c = int(rng.choice(odd))
        even = [r for r in range(c + 1, n - 1, 2) if r not in spec["dense"]]
        if even:
            N[int(rng.choice(even)), c] = rng.choice([-1, 1])
    for t, (r, c) in enumerate(spec.get("spots", ())):                   # placed extras (odd column, even row, as above; no random number drawn)
        assert c % 2 == 1 and r % 2 == 0 and c < r < n - 1 and r not in spec["dense"] and c not in spec["dense"]
        N[r, c] = 1 - 2 * (t % 2)
    k = rng.integers(0, 2, size=n) + (1 if n <= 2 else 0)
    while True:
        L = N + np.diag(2 ** k)
        P = L @ L.T - np.eye(n, dtype=np.int64)
        short = np.diag(P) < np.abs(P).sum(axis=1) - np.abs(np.diag(P))
        if not short.any():
            return N, k, L, P
        k[short] += 1


def _columns(P):
    """{(i, j, sign, chunk): S} of one draw: the non-negative decomposition of a diagonally dominant integer P, S in chunks of CH bits"""
    n = P.shape[0]
    out = {}
    for i in range(n):
        for j in range(i):
            v = int(P[i, j])
            if v:
                for c, s in enumerate(_chunks(abs(v))):
                    out[(i, j, 1 if v > 0 else -1, c)] = s
        slack = int(P[i, i]) - int(np.abs(P[i]).sum() - abs(P[i, i]))
        for c, s in enumerate(_chunks(slack)):
            out[(i, i, 1, c)] = s
    return out


def _shift(key):
    return (key[0] * 7 + key[1] * 3 + key[3]) % 3 - 1


@functools.lru_cache(maxsize=None)
def inputs(n):
    """_inputs(n, attempts) with the first attempts at which every row of every draw has any-order exact c and g (the generator verifies, it does
    not assume); AssertionError if eight rounds do not get there"""
    attempts = [0] * SHAPES[n]["draws"]
    for _ in range(8):
        c = _inputs(n, tuple(attempts))
        c["draws"] = [_draw(c, d) for d in range(c["D"])]
        short = [d for d in range(c["D"]) if not c["draws"][d]["mloo_ok"].all()]
        if not short:
            return c
        for d in short:
            attempts[d] += 1
    raise AssertionError("n = %d: no draw with every sum of c and g exact in any order: %r" % (n, attempts))


def _inputs(n, attempts):
    """The seeded inputs of shape n: X (n x q), y, new rows Xn (m x q), and per draw tau2, mu, S, W -- float64 arrays, never written to -- with the
    integers behind them (keys: the (i, j, sign, chunk) of every column, None for a padding column; facs: (N, k, L, P) per draw)"""
    spec = SHAPES[n]
    D = spec["draws"]
    facs = [_factor(n, spec, d, attempts[d]) for d in range(D)]
    cols = [_columns(f[3]) for f in facs]
    keys = sorted(set().union(*[set(c) for c in cols]))
    q = len(keys) + 2
    if spec["qmod32"] is None:
        while q % 4 == 0 or q % 32 in (0, 1):
            q += 1
    else:
        q += (spec["qmod32"] - q) % 32
    rng = np.random.default_rng([43, n])
    perm = rng.permutation(q)
    place = [None] * q                                                   # the key of every column
    for key, p in zip(keys, perm):
        place[p] = key
    X = np.zeros((n, q))
    S = np.zeros((D, q))
    for e, key in enumerate(place):
        if key is None:
            X[:, e] = rng.integers(-1, 2, size=n)
            continue
        i, j, sg, _c = key
        a = _shift(key)
        X[i, e] = 2.0 ** a
        if j != i:
            X[j, e] = sg * 2.0 ** a
        for d in range(D):
            S[d, e] = cols[d].get(key, 0) * 4.0 ** -a
    y = rng.integers(-4, 5, size=n).astype(np.float64)
    mu = rng.integers(-4, 5, size=D) / 2.0
    tau2 = 4.0 ** rng.integers(-1, 3, size=D)
    W = rng.integers(-1, 2, size=(D, q)).astype(np.float64)
    m = spec["m"]
    Xn = np.zeros((m, q))
    for j in range(m):
        for e in rng.choice(q, size=min(q, 1 + j % 3), replace=False):
            Xn[j, e] = rng.choice([-2, -1, 1, 2])
    out = dict(n=n, q=q, D=D, m=m, X=X, y=y, Xn=Xn, tau2=tau2, mu=mu, S=S, W=W)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    out.update(keys=place, facs=facs, attempts=attempts)
    return out


def edge_rows(n):
    """the rows at the edges of the 16- and 32-row tiles and of the factor kernel's 256-column passes, and the last row (ROWS_257 at n = 257)"""
    return tuple(sorted(r for r in set(ROWS_257) | {511, 512, n - 1} if r < n))


def edges_checked(n):
    """the columns whose edge outputs are checked: all of them up to n = 65 and wherever q <= 2 SAMPLE_257; elsewhere every live column incident
    to edge_rows(n) and a seeded sample of SAMPLE_257 of the others"""
    c = inputs(n)
    if n <= 65 or c["q"] <= 2 * SAMPLE_257:
        return np.arange(c["q"])
    rows = edge_rows(n)
    hit = [e for e, key in enumerate(c["keys"]) if key is not None and (key[0] in rows or key[1] in rows)]
    rest = sorted(set(range(c["q"])) - set(hit))
    extra = np.random.default_rng([47, n]).choice(rest, size=SAMPLE_257, replace=False)
    return np.array(sorted(hit + [int(e) for e in extra]))


# ------------------------------------------------------------------------------------------ the exact reference of one draw
def _draw(c, d):
    """Everything of draw d of the inputs c in integers.  Scales: L, A 0; X 1 (2 X is an integer matrix); S 2; r 2; M E; z E + 2; c 2 E; g 2 E + 2"""
    n, q = c["n"], c["q"]
    N, k, L, P = c["facs"][d]
    rep = {}
    X2 = np.rint(2 * c["X"]).astype(np.int64)
    S4 = np.rint(4 * c["S"][d]).astype(np.int64)
    Wi = np.rint(c["W"][d]).astype(np.int64)
    assert np.array_equal(X2 / 2.0, c["X"]) and np.array_equal(S4 / 4.0, c["S"][d])
    # ---- the Gram: A = I + X diag(S) X^T, every product x S and (x S) x exact, the K sum in any order
    X2f, S4f = X2.astype(np.float64), S4.astype(np.float64)              # (float64 products of integers: exact below 2^53, which ab proves)
    ab = (np.abs(X2f) * S4f[None, :]) @ np.abs(X2f).T
    rep["A"] = bool(np.all(ab < float(TWO53 >> 4)))                     # terms: multiples of 1/16 whose absolute sum stays below 2^49
    G16 = (X2f * S4f[None, :]) @ X2f.T                                   # 16 P
    assert rep["A"] and np.array_equal(G16, 16.0 * P), "the decomposition does not give back P"
    A = P + np.eye(n, dtype=np.int64)
    # ---- the right-hand side: r = (y - mu) - sum_e x_e W_e
    xw2 = X2 @ Wi                                                        # scale 1
    rep["r"] = bool(np.all(np.abs(X2) @ np.abs(Wi) < TWO53))
    r4 = 4 * np.rint(c["y"]).astype(np.int64) - int(round(4 * c["mu"][d])) - 2 * xw2
    # ---- the left-looking Cholesky: s_r = A[r][j] - sum_{k<j} L[r][k] L[j][k], integers
    Lo = L.astype(object)
    ok = True
    for j in range(n):
        terms = np.abs(Lo[j:, :j] * Lo[j, :j][None, :]).sum(axis=1) + np.abs(A[j:, j]).astype(object)
        ok = ok and all(int(t) < TWO53 for t in terms)
    rep["L"] = ok
    # ---- M = L^-1 by forward substitution, column i, rows ascending; terms [r == i] and L[r][k] M[k][i]
    kk = [int(v) for v in k]
    nzL = [[(kc, int(L[r, kc])) for kc in range(r) if L[r, kc]] for r in range(n)]
    Mf = [[0] * n for _ in range(n)]
    okM = True
    for i in range(n):
        for r in range(i, n):
            terms = [Fraction(1 if r == i else 0)] + [-lv * Mf[kc][i] for kc, lv in nzL[r] if kc >= i and Mf[kc][i] != 0]
            den = max(t.denominator for t in terms)
            mags = [abs(int(t * den)) for t in terms]
            okM = okM and _anyorder(sum(mags), functools.reduce(lambda a, b: a | b, mags))
            Mf[r][i] = sum(terms) / (1 << kk[r])
    E = max(max(Fraction(v).denominator for v in row) for row in Mf).bit_length() - 1
    Mi = np.array([[int(Fraction(v) * (1 << E)) for v in row] for row in Mf], dtype=object)
    rep["M"] = okM and all(_rep(v) for v in Mi.reshape(-1))
    # ---- z = L^-1 r by the forward substitution that rides along: z_j = (r_j - sum_{k<j} z_k L[j][k]) / L[j][j]
    r4o = np.array([int(v) for v in r4], dtype=object)
    zi = Mi @ r4o                                                        # scale E + 2
    okz = True
    for j in range(n):
        sabs, orr = abs(int(r4o[j])) << E, abs(int(r4o[j])) << E
        for kc, lv in nzL[j]:
            t = abs(int(zi[kc]) * lv)
            sabs += t
            orr |= t
        okz = okz and _anyorder(sabs, orr)
    rep["z"] = okz and all(_rep(v) for v in zi)
    zz, okzz = _sum_check((zi * zi)[None, :], 1)
    rep["zz"] = bool(okzz[0])
    # ---- c_i = sum_r M[r][i]^2, g_i = sum_r M[r][i] z_r
    ci, okc = _sum_check(Mi * Mi, 0)
    gi, okg = _sum_check(Mi * zi[:, None], 0)
    rep["c"], rep["g"] = okc, okg
    t2 = float(c["tau2"][d])
    lt = int(round(math.log2(t2)))                                      # tau2 = 2^lt, lt even
    resid = np.array([float(Fraction(int(g), 4 * int(cc))) for g, cc in zip(gi, ci)])
    var = np.array([float(Fraction((1 << (2 * E + 8)), int(cc)) * Fraction(2) ** (lt - 8)) for cc in ci])
    out = dict(n=n, q=q, d=d, E=E, k=np.array(kk), tau2=t2, lt=lt, Mi=Mi, zi=zi, ci=ci, gi=gi, report=rep,
               A=A.astype(np.float64), L=L.astype(np.float64), M=_farr(Mi, E), z=_farr(zi, E + 2), zz=_f(int(zz[0]), 2 * E + 4), c=_farr(ci, 2 * E),
               g=_farr(gi, 2 * E + 2), r=r4 / 4.0, resid=resid, var=var,
               density=float(np.count_nonzero(Mi) - n) / max(1, n * (n - 1) // 2),
               c_bits=max((int(v) >> _tz(int(v))).bit_length() for v in ci))
    out["mloo_ok"] = okc & okg & bool(rep["A"] and rep["r"] and rep["L"] and rep["M"] and rep["z"])
    return out


def draw(n, d):
    return inputs(n)["draws"][d]


def _project(dr, cols2, scale_extra):
    """T = M C for the integer columns cols2 (n x m object array on scale scale_extra) and t = the sums of squares of its columns:
    (T on scale E + scale_extra, its any-order flags per column, t on twice that scale, its flags)"""
    Mi = dr["Mi"]
    n, m = cols2.shape
    T = np.zeros((n, m), dtype=object)
    okT = np.ones(m, dtype=bool)
    for j in range(m):
        rows = [i for i in range(n) if cols2[i, j]]
        if not rows:
            continue
        terms = np.stack([Mi[:, i] * cols2[i, j] for i in rows], axis=1)
        s, ok = _sum_check(terms, 1)
        T[:, j] = s
        okT[j] = bool(ok.all())
    t, okt = _sum_check(T * T, 0)
    return T, okT, t, okt & okT


@functools.lru_cache(maxsize=None)
def edges(n, d):
    """The edge outputs of draw d at the columns edges_checked(n): dict with v (exact float64 where ok), ok (T, t, S t, 1 - S t, tau2 S and the
    product all exact), t (float64 where t_ok), and the integer T (n x ne, scale E + 1) of those columns.  A column with S = 0 has v = 0 whatever t."""
    c, dr = inputs(n), draw(n, d)
    idx = edges_checked(n)
    E = dr["E"]
    X2 = np.rint(2 * c["X"][:, idx]).astype(np.int64).astype(object)
    S4 = [int(round(4 * v)) for v in c["S"][d][idx]]
    T, okT, t, okt = _project(dr, X2, 1)                                 # t on scale 2 E + 2
    one = 1 << (2 * E + 4)
    v = np.zeros(len(idx))
    ok = np.zeros(len(idx), dtype=bool)
    for a in range(len(idx)):
        if S4[a] == 0:
            ok[a] = True                                                 # (tau2 0) fmax(1 - 0 t, 0) = 0
            continue
        st = S4[a] * int(t[a])                                           # scale 2 E + 4
        om = one - st
        assert om >= 0
        vv = S4[a] * om                                                  # tau2 S (1 - S t): scale 2 E + 6, times 2^lt
        ok[a] = bool(okt[a]) and _rep(st) and _rep(om) and _rep(vv)
        v[a] = _f(vv, 2 * E + 6 - dr["lt"])
    return dict(idx=idx, v=v, ok=ok, T=T, okT=okT, t=_farr(t, 2 * E + 2), t_ok=okt & np.array([_rep(x) for x in t]))


@functools.lru_cache(maxsize=None)
def predict(n, d):
    """The new-row outputs of draw d: dict with a, dq, C (n x m, all exact float64 where the flags hold), var (exact where ok) and ok"""
    c, dr = inputs(n), draw(n, d)
    E, m = dr["E"], c["m"]
    X2 = np.rint(2 * c["X"]).astype(np.int64)
    S4 = np.rint(4 * c["S"][d]).astype(np.int64)
    Xn = np.rint(c["Xn"]).astype(np.int64)
    Wi = np.rint(c["W"][d]).astype(np.int64)
    a = Xn @ Wi
    d4 = (Xn * S4[None, :] * Xn).sum(axis=1)                            # scale 2
    XS = X2.astype(np.float64) * S4.astype(np.float64)[None, :]
    small = bool(np.all(np.abs(XS) @ np.abs(Xn).T.astype(np.float64) < float(TWO53))) and bool(np.all((np.abs(Xn) * S4[None, :] * np.abs(Xn)).sum(axis=1) < TWO53))
    C8 = np.rint(XS @ Xn.T.astype(np.float64)).astype(np.int64)          # scale 3 (float64 products of integers: exact, as `small` proves)
    T, okT, t, okt = _project(dr, C8.astype(object), 3)                  # t on scale 2 E + 6
    var = np.zeros(m)
    ok = np.zeros(m, dtype=bool)
    for j in range(m):
        dj = int(d4[j]) << (2 * E + 4)
        df = dj - int(t[j])
        assert df >= 0
        ok[j] = small and bool(okt[j]) and _rep(t[j]) and _rep(df)
        var[j] = _f(df, 2 * E + 6 - dr["lt"])
    return dict(a=a.astype(np.float64), dq=d4 / 4.0, C=C8 / 8.0, var=var, ok=ok, small=small)


@functools.lru_cache(maxsize=None)
def within(n, cols, K, nd, weights):
    """The exact `within` of marginal_gamma_cov over the first K nd draws of shape n, the columns `cols` (a tuple) and the dyadic chain weights
    `weights` (a tuple; nd a power of two): (within as float64, ok per entry).  The device forms T' = (sqrt(tau2) S_a) T_ia (one product of exact
    operands), the chains' Grams of T' (any order over rows and draws), Gw / nd w_k summed over k, the diagonal's chain sums of tau2 S, and the
    difference; an entry is ok where every one of those is exact."""
    c = inputs(n)
    nc = len(cols)
    assert nd & (nd - 1) == 0 and len(weights) == K
    wi = [int(round(w * 1024)) for w in weights]
    assert all(v / 1024.0 == w for v, w in zip(wi, weights))
    Emax = max(draw(n, d)["E"] for d in range(K * nd))
    lnd = nd.bit_length() - 1
    X2 = np.rint(2 * c["X"][:, list(cols)]).astype(np.int64).astype(object)
    gw = np.zeros((nc, nc), dtype=object)                                # scale 2 Emax + 6 - ltmin ... kept on SC below
    dg = np.zeros(nc, dtype=object)
    okall = np.ones((nc, nc), dtype=bool)
    LT = 4                                                               # tau2 >= 4^-1: sqrt(tau2) 2^LT and tau2 4^LT are integers
    SC = 2 * (Emax + 1 + 2 + LT) + lnd + 10                              # the scale of gw and dg: T' on Emax + 3 + LT, / nd, w on 10
    for kch in range(K):
        G = np.zeros((nc, nc), dtype=object)
        sa = np.zeros((nc, nc), dtype=object)
        orr = np.zeros((nc, nc), dtype=object)
        dsum, dabs, dor = np.zeros(nc, dtype=object), np.zeros(nc, dtype=object), np.zeros(nc, dtype=object)
        okp = np.ones(nc, dtype=bool)
        for d in range(kch * nd, (kch + 1) * nd):
            dr = draw(n, d)
            S4 = np.array([int(round(4 * v)) for v in c["S"][d][list(cols)]], dtype=object)
            live = np.array([int(v) != 0 for v in S4])
            T = np.zeros((n, nc), dtype=object)
            okT = np.ones(nc, dtype=bool)
            if live.any():
                T[:, live], okT[live], _t, _ = _project(dr, X2[:, live], 1)
            st = 1 << (dr["lt"] // 2 + LT)
            Tp = T * (S4 * st)[None, :] * (1 << (Emax - dr["E"]))        # scale Emax + 1 + 2 + LT
            okp &= okT & np.array([all(_rep(v) for v in Tp[:, a]) for a in range(nc)])
            G = G + Tp.T @ Tp
            aT = np.abs(Tp)
            sa = sa + aT.T @ aT
            for r in range(n):
                row = aT[r]
                nzc = [a for a in range(nc) if row[a]]
                for a in nzc:
                    for b in nzc:
                        orr[a, b] |= row[a] * row[b]
            dd = S4 * (1 << (dr["lt"] + 2 * LT))                         # tau2 S: scale 2 + 2 LT
            dsum, dabs, dor = dsum + dd, dabs + dd, dor | dd
        okG = np.array([[_anyorder(int(sa[a, b]), int(orr[a, b])) for b in range(nc)] for a in range(nc)]) & okp[:, None] & okp[None, :]
        term = G * (wi[kch] << (SC - 2 * (Emax + 3 + LT) - lnd - 10))     # (Gw / nd) w_k on SC
        okall &= okG & np.array([[_rep(v) for v in row] for row in term])
        gw = gw + term
        okall &= np.array([[_rep(v) for v in row] for row in gw])
        dterm = dsum * (wi[kch] << (SC - (2 + 2 * LT) - lnd - 10))
        okd = np.array([_anyorder(int(a), int(b)) and _rep(t) for a, b, t in zip(dabs, dor, dterm)])
        dg = dg + dterm
        okd &= np.array([_rep(v) for v in dg])
        okall &= okd[:, None]
    same = np.array([[cols[a] == cols[b] for b in range(nc)] for a in range(nc)])
    wv = np.where(same, dg[:, None], 0) - gw
    okall &= np.array([[_rep(v) for v in row] for row in wv])
    return _farr(wv, SC), okall


def summary(n):
    """one line of the report of shape n: which sums are any-order exact, the density of M and the bits of c"""
    c = inputs(n)
    rows = []
    for d in range(c["D"]):
        dr, ed, pr = draw(n, d), edges(n, d), predict(n, d)
        rep = dr["report"]
        live = np.array([c["keys"][e] is not None and c["S"][d][e] != 0 for e in ed["idx"]])
        rows.append(dict(d=d, A=rep["A"], r=rep["r"], L=rep["L"], M=rep["M"], z=rep["z"], zz=rep["zz"], c=int(rep["c"].sum()), g=int(rep["g"].sum()),
                         mloo=int(dr["mloo_ok"].sum()), edges=int(len(ed["idx"])), v_ok=int(ed["ok"].sum()), live=int(live.sum()),
                         v_live_ok=int((ed["ok"] & live).sum()), pred_ok=int(pr["ok"].sum()), m=c["m"], density=dr["density"], c_bits=dr["c_bits"],
                         E=dr["E"], kmax=int(dr["k"].max())))
    return rows
