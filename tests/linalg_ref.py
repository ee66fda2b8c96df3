"""Exact and extended-precision host references for the gamma update's linear algebra (gibbs.jl:420-437), numpy only.

The device computes, per gamma update,
    G  = X diag(S) X'                       (k_gram / k_gram8 in f64, or k_sdigits + k_gram_i8 on the i8 pipe for a 0/1 X)
    b  = (y - X W - mu)/tau - (X sz + z2)   (k_xpass*, k_rhs;  sz = sqrt(S) z1, so that tau sz = Delta gamma_1 of gibbs.jl:429)
    A  = G + I = L L',  Y = L^-T            (k_chol_step / k_chol_step2)
    a4 = Y (Y' b) = A^-1 b                  (k_solve_w, k_solve_a4)
    gamma = W + tau (sz + S (X' a4))        (k_backproj*)
and this module restates each of them without rounding (or in long double), so that a test can bound the device's error
by a rigorous a-priori bound instead of comparing two implementations of the same double-precision algorithm.

Exactness comes from integer arithmetic inside float64 BLAS.  X is either 0/1 or holds small dyadic rationals k/16 with
|k| <= 128, so Xi = X * xscale is an integer matrix with |Xi| <= 128.  A real vector s is cut into fixed-point pieces of
PIECE_BITS bits under its largest exponent, s = 2^e sum_p d_p 2^(-PIECE_BITS (p + 1)) (+ a remainder, carried explicitly),
every d_p an integer vector with |d_p| < 2^PIECE_BITS.  Every product and partial sum of Xi diag(d_p) Xi' or Xi' d_p is then
an integer below 2^53: exact in float64 whatever order the BLAS adds in.  The pieces are recombined in np.longdouble; that
last step is the only rounding, and ld_rel() bounds it.
"""
import numpy as np

LD = np.longdouble
U = 2.0 ** -53                                    # unit roundoff of float64
PIECE_BITS = 17
MAX_PIECES = 10


def gamma_m(m):
    """Higham's gamma_m = m u / (1 - m u): the relative bound of m successive float64 roundings (any order)."""
    return m * U / (1.0 - m * U)


def ld_rel(npieces):
    """relative bound of summing `npieces` exact long-double terms (plus one final conversion): tiny beside any float64 bound"""
    return (npieces + 2) * float(np.finfo(LD).eps)


def integer_image(X):
    """(Xi, xscale): Xi = X * xscale as float64 integers with |Xi| <= 128 (0/1: xscale 1; k/16: xscale 16); ValueError otherwise"""
    Xf = np.asarray(X, dtype=np.float64)
    for sc in (1.0, 16.0):
        Xi = Xf * sc
        if np.all(Xi == np.round(Xi)) and np.abs(Xi).max(initial=0.0) <= 128.0:
            return Xi, sc
    raise ValueError("X must hold 0/1 or multiples of 1/16 of magnitude <= 8")


def split_pieces(s, max_pieces=MAX_PIECES):
    """s (float64 or longdouble vector) = 2^e sum_p pieces[p] 2^(-PIECE_BITS (p + 1)) + rem, |rem| <= trunc elementwise.
    Returns (pieces as float64 integer vectors, e, trunc).  Every step is exact: scaling by powers of two and x - trunc(x)."""
    s = np.asarray(s)
    work = s.astype(LD) if s.dtype == LD else s.astype(np.float64)
    amax = np.abs(work).max(initial=0)
    if amax == 0:
        return [], 0, 0.0
    _, e = np.frexp(np.float64(amax))
    e = int(e) + (1 if np.float64(amax) < amax else 0)      # amax < 2^e (long double amax can exceed its float64 rounding)
    r = np.ldexp(work, -e)
    pieces = []
    for _ in range(max_pieces):
        r = np.ldexp(r, PIECE_BITS)
        d = np.trunc(r)
        pieces.append(d.astype(np.float64))
        r = r - d
        if not np.any(r):
            break
    trunc = float(np.ldexp(np.float64(1.0), e - PIECE_BITS * len(pieces))) if np.any(r) else 0.0
    return pieces, e, trunc


def _check_int_range(Xi, npieces_len, k):
    """every partial sum of k products |Xi| <= 128 times |d| < 2^PIECE_BITS times |Xi| <= 128 stays below 2^53"""
    assert k * 128.0 * 128.0 * 2.0 ** PIECE_BITS < 2.0 ** 53, ("integer sums could exceed 2^53", k)


def exact_gram(X, S, rows=None, cols=None):
    """G* = X[rows] diag(S) X[cols]' exactly up to (trunc, ld) terms.  Returns (G* as longdouble, err) where err is an
    elementwise bound of |G* - exact| (the piece truncation plus the long-double recombination)."""
    Xi, xs = integer_image(X)
    S = np.asarray(S, dtype=np.float64)
    Xr = Xi if rows is None else Xi[rows]
    Xc = Xi if cols is None else Xi[cols]
    _check_int_range(Xi, 0, Xi.shape[1])
    pieces, e, trunc = split_pieces(S)
    G = np.zeros((Xr.shape[0], Xc.shape[0]), dtype=LD)
    for p, d in enumerate(pieces):
        Gp = (Xr * d) @ Xc.T                                      # integers < 2^53: exact
        G += np.ldexp(Gp.astype(LD), e - PIECE_BITS * (p + 1))
    G /= LD(xs * xs)
    absX = np.abs(Xr) @ np.abs(Xc).T / (xs * xs)                  # integer counts / 256: exact
    absG = (np.abs(Xr) * np.abs(S)) @ np.abs(Xc).T / (xs * xs) * (1 + 2 * gamma_m(Xi.shape[1]))
    err = trunc * absX + ld_rel(len(pieces)) * absG
    return G, err


def abs_gram(X, S, rows=None, cols=None):
    """(|X| |S| |X|')[rows, cols] rounded up (it only enters bounds)"""
    Xa = np.abs(np.asarray(X, dtype=np.float64))
    Xr = Xa if rows is None else Xa[rows]
    Xc = Xa if cols is None else Xa[cols]
    return (Xr * np.abs(S)) @ Xc.T * (1 + 2 * gamma_m(Xa.shape[1]))


class IntMatrix:
    """X held as its integer image, streamed in column chunks (a float64 copy of the window shape's X would not fit), with exact
    products X v and X' v for float64 or long-double v (to the piece truncation, which is returned)."""

    def __init__(self, X, chunk=4096):
        self.X = X                                   # any dtype (Bool for the big shapes): converted chunk by chunk
        self.n, self.q = X.shape
        self.chunk = chunk
        probe = np.asarray(X[:, :min(self.q, 256)], dtype=np.float64)
        self.xscale = integer_image(probe)[1] if probe.size else 1.0
        self.binary = X.dtype == np.bool_ or bool(np.all((probe == 0) | (probe == 1)))
        if self.binary:
            self.xscale = 1.0
        assert max(self.n, self.q) * 128.0 * 128.0 * 2.0 ** PIECE_BITS < 2.0 ** 53

    def _cols(self, c0, c1):
        Xc = np.asarray(self.X[:, c0:c1], dtype=np.float64) * self.xscale
        if not self.binary:
            assert np.all(Xc == np.round(Xc)) and np.abs(Xc).max(initial=0.0) <= 128.0
        return Xc

    def matvec(self, v):
        """X v (v: q) in long double; returns (result, elementwise error bound)"""
        pieces, e, trunc = split_pieces(v)
        out = np.zeros(self.n, dtype=LD)
        absx = np.zeros(self.n)
        if not pieces:
            return out, absx
        P = np.stack(pieces, axis=1)                                  # q x npieces
        acc = np.zeros((self.n, P.shape[1]))
        for c0 in range(0, self.q, self.chunk):
            Xc = self._cols(c0, min(self.q, c0 + self.chunk))
            acc += Xc @ P[c0:c0 + Xc.shape[1]]                        # integer partial sums < 2^53, exact; acc itself stays exact too
            if trunc:
                absx += np.abs(Xc).sum(axis=1)
        for p in range(P.shape[1]):
            out += np.ldexp(acc[:, p].astype(LD), e - PIECE_BITS * (p + 1))
        out /= LD(self.xscale)
        absv = np.abs(v).astype(np.float64)
        err = trunc * absx / self.xscale + ld_rel(len(pieces)) * self.absmatvec(absv)
        return out, err

    def rmatvec(self, v):
        """X' v (v: n) in long double; returns (result, elementwise error bound)"""
        pieces, e, trunc = split_pieces(v)
        out = np.zeros(self.q, dtype=LD)
        if not pieces:
            return out, np.zeros(self.q)
        P = np.stack(pieces, axis=1)
        acc = np.empty((self.q, P.shape[1]))
        for c0 in range(0, self.q, self.chunk):
            Xc = self._cols(c0, min(self.q, c0 + self.chunk))
            acc[c0:c0 + Xc.shape[1]] = Xc.T @ P
        for p in range(P.shape[1]):
            out += np.ldexp(acc[:, p].astype(LD), e - PIECE_BITS * (p + 1))
        out /= LD(self.xscale)
        absv = np.abs(v).astype(np.float64)
        err = trunc * self.absrmatvec(np.ones(self.n)) + ld_rel(len(pieces)) * self.absrmatvec(absv)
        return out, err

    def absmatvec(self, v):
        """|X| v for v >= 0 (float64, rounded up: bounds only)"""
        out = np.zeros(self.n)
        for c0 in range(0, self.q, self.chunk):
            Xc = np.abs(self._cols(c0, min(self.q, c0 + self.chunk)))
            out += Xc @ np.asarray(v[c0:c0 + Xc.shape[1]], dtype=np.float64)
        return out / self.xscale * (1 + 2 * gamma_m(self.q))

    def absrmatvec(self, v):
        """|X|' v for v >= 0 (float64, rounded up: bounds only)"""
        out = np.empty(self.q)
        vv = np.asarray(v, dtype=np.float64)
        for c0 in range(0, self.q, self.chunk):
            Xc = np.abs(self._cols(c0, min(self.q, c0 + self.chunk)))
            out[c0:c0 + Xc.shape[1]] = Xc.T @ vv
        return out / self.xscale * (1 + 2 * gamma_m(self.n))

    def apply_A(self, S, v):
        """(X diag(S) X' + I) v in long double (two exact GEMVs around a long-double scaling); returns (result, error bound)"""
        t, et = self.rmatvec(v)
        w = np.asarray(S, dtype=LD) * t
        r, er = self.matvec(w)
        ew = np.abs(S) * et + float(np.finfo(LD).eps) * np.abs(w).astype(np.float64)
        return r + np.asarray(v, dtype=LD), er + self.absmatvec(ew)

    def norm_abs_gram_inf(self, S):
        """|| |X| |S| |X|' ||_inf (row sums; an upper bound of the 2-norm of the nonnegative matrix and of || G ||_2)"""
        return float(self.absmatvec(np.abs(S) * self.absrmatvec(np.ones(self.n))).max(initial=0.0))


def spectral_norm_upper(apply, n, iters=60, seed=0):
    """||M||_2 of a symmetric positive semidefinite operator by power iteration, rounded up by the iteration's own residual
    (Rayleigh quotient + ||M v - rho v||: an upper bound on the eigenvalue nearest rho; with a dominant start it is the top one)"""
    rng = np.random.default_rng(seed)
    v = rng.random(n) + 0.5
    v /= np.linalg.norm(v)
    rho = 0.0
    for _ in range(iters):
        w = apply(v)
        rho = float(v @ w)
        nw = np.linalg.norm(w)
        if nw == 0:
            return 0.0
        v = w / nw
    w = apply(v)
    rho = float(v @ w)
    return (rho + float(np.linalg.norm(w - rho * v))) * (1 + 1e-12)


def refined_solve(A64, apply_ld, b, steps=3):
    """a4* with A a4* = b: float64 solve, then `steps` rounds of iterative refinement with long-double residuals
    (apply_ld(v) = A v in long double).  A >= I, so every round gains about 53 - log2(||A||) bits."""
    b = np.asarray(b, dtype=LD)
    x = np.linalg.solve(A64, b.astype(np.float64)).astype(LD)
    for _ in range(steps):
        r = b - apply_ld(x)
        x = x + np.linalg.solve(A64, r.astype(np.float64)).astype(LD)
    return x


def compute_W(u_row, lam_row):
    """W = lower_triangle(u' diag(lam) u) (gibbs.jl:219-221, utils.jl:50-55) in long double, and sum_r |u_rl lam_r u_rk| (for bounds).
    u_row: R x V, lam_row: R"""
    u = np.asarray(u_row, dtype=LD)
    lam = np.asarray(lam_row, dtype=LD)
    R, V = u.shape
    M = (u * lam[:, None]).T @ u
    Ma = (np.abs(u) * np.abs(lam)[:, None]).T @ np.abs(u)
    k, l = np.meshgrid(np.arange(V), np.arange(V), indexing="ij")
    sel = l >= k                                                   # column-wise lower triangle: e runs over l for each k
    order = np.argsort((k * V + l)[sel], kind="stable")
    W = M[l[sel], k[sel]][order]
    Wa = Ma[l[sel], k[sel]][order].astype(np.float64)
    return W, Wa


# ----------------------------------------------------------------------------------------- checkers (device output vs reference)
def ratio(err, bound):
    """largest err / bound (0 where both are 0; inf where only the bound is 0)"""
    err = np.asarray(err, dtype=np.float64)
    bound = np.asarray(bound, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, err / bound)
    return float(np.nanmax(r)) if r.size else 0.0


def sum_partials_ld(P):
    """the K-split partial tiles [ksplit][ntl][64 x 64] summed in long double -> [ntl][64 x 64] (j-major as on the device)"""
    return np.asarray(P, dtype=LD).sum(axis=0)


def tiles_to_lower(T, ntile):
    """[ntl][j][i] tiles (tile (ti >= tj) at ti (ti + 1) / 2 + tj, element (i, j) at [j 64 + i]) -> lower block triangle of an n_pad x n_pad matrix"""
    n_pad = 64 * ntile
    G = np.zeros((n_pad, n_pad), dtype=T.dtype)
    for ti in range(ntile):
        for tj in range(ti + 1):
            G[ti * 64:(ti + 1) * 64, tj * 64:(tj + 1) * 64] = T[ti * (ti + 1) // 2 + tj].reshape(64, 64).T
    return G


def check_gram_f64(G_dev, G_ref, G_err, absG, m):
    """|G - G*| <= gamma_m (|X| S |X|') + ref error, on the lower block triangle of the first n rows / columns.  Returns the ratio."""
    err = np.abs((np.asarray(G_dev, dtype=LD) - G_ref)).astype(np.float64)
    return ratio(err, gamma_m(m) * absG + G_err)


def i8_bound(count, e_top, L, absG, m):
    """the i8 Gram's bound: rounding every S_k to nearest on the grid 2^(e - 8L + 2) (k_sdigits) is off by at most 2^(e - 8L + 1), so
    |G - G*|_ij <= (|X| |X|')_ij 2^(e - 8L + 1) (two-sided), plus the f64 recombination of the L exact i32 planes and the K slices"""
    step = 2.0 ** (e_top - 8 * L + 1)
    return count * step + gamma_m(m) * (absG + count * step)


def check_gram_i8(G_dev, G_ref, G_err, count, e_top, L, absG, m):
    err = np.abs((np.asarray(G_dev, dtype=LD) - G_ref)).astype(np.float64)
    return ratio(err, i8_bound(count, e_top, L, absG, m) + G_err)


def solve_bound(n_pad, normA, normAbsG, m, normb, norma):
    """||a4 - A^-1 b||_2 for a4 = Y (Y' b) from the device's own b (||A^-1||_2 <= 1 since A >= I; ||a|| = ||A^-1 b||):
    the factor and the columns of Y = L^-T, each backward stable, put 8 n_pad u ||A||_2 ||a|| into Y w and 8 n_pad u ||A||_2^(1/2) ||b|| into
    w = Y' b; the Gram's own error ||dG||_2 <= gamma_m || |X| S |X|' ||_2 adds ||dG|| ||a|| to first order"""
    return (8 * n_pad * U * normA + gamma_m(m) * normAbsG) * norma + 8 * n_pad * U * np.sqrt(normA) * normb


def check_solve(a4_dev, a4_ref, bound):
    return float(np.linalg.norm((np.asarray(a4_dev, dtype=LD) - a4_ref).astype(np.float64))) / bound


def block_upper_Y(E, n_pad, ld):
    """Y = L^-T from rows n_pad.. of the column-major E, on the block upper triangle k_solve_* read (block(r) <= block(c)); 0 elsewhere"""
    Y = np.asarray(E).reshape(n_pad, ld).T[n_pad:2 * n_pad, :].copy()
    rb = np.arange(n_pad) // 32
    Y[rb[:, None] > rb[None, :]] = 0.0
    return Y


def check_Y(Y, apply_A_ld, cols, n_pad, normA, normAbsG, m, c=16):
    """columns j of Y' A Y - I, each within (c n_pad u ||A||_2 + gamma_m || |X| S |X|' ||_2) in the 2-norm.  Returns the ratio."""
    worst = 0.0
    bound = c * n_pad * U * normA + gamma_m(m) * normAbsG
    for j in cols:
        y = Y[:, j]
        z = apply_A_ld(y)
        r = (Y.T.astype(LD) @ z)
        r[j] -= 1
        worst = max(worst, float(np.linalg.norm(r.astype(np.float64))) / bound)
    return worst


def check_b(b_dev, b_ref, b_bnd):
    err = np.abs((np.asarray(b_dev, dtype=LD) - b_ref)).astype(np.float64)
    return ratio(err, b_bnd)


def check_gamma(g_dev, g_ref, g_bnd):
    err = np.abs((np.asarray(g_dev, dtype=LD) - g_ref)).astype(np.float64)
    return ratio(err, g_bnd)
