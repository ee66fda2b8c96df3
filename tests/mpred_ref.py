"""The reference of the conditional posterior of the mean response of new rows (include/bnr_mpred.h) in mpmath at 50 digits, stated two
independent ways, and the error bounds that a float64 evaluation has to meet.  Inputs are mloo_ref.case's plus seeded new rows; nothing here is
rounded to float64 before the results are.

For one draw phi = (tau2, mu, S, W), an n x q matrix X and new rows X* (m x q):  eta*_j | phi, y ~ N(mean_j, var_j).
  a_inverse(...)   A = I + X diag(S) X^T = L L^T, C = X diag(S) X*^T, g = A^-1 (y - mu - X W):
                   mean_j = mu + x*_j . W + C_j . g,   var_j = tau2 (x*_j^T diag(S) x*_j - C_j^T A^-1 C_j)
  precision(...)   Cov gamma = tau2 (D^-1 + X^T X)^-1 as a q x q solve, E gamma = Cov (D^-1 W + X^T (y - mu)) / tau2:
                   mean_j = mu + x*_j . E gamma,   var_j = x*_j^T Cov x*_j   (needs S > 0)
The two agree to 1e-40 (tests/test_marginal_predict_host.py).

The bounds (float64, eps = 2^-52, u = eps / 2), to first order, the gate twice that for the second-order terms.  beta, Lam and rho are
mloo_ref's, ec = beta Lam, c_i = (A^-1)_ii; dg is medge_ref's: sqrt(c_i) (ec ||g||_2 + rho) + 4 u |g_i|.
  C_ij = sum_e (x_ie S_e) x*_je: q products of two roundings each and q sums in the matrix pipe's order:
      |dC_ij| <= (q + 2) u sum_e |x_ie S_e x*_je|
  t_j = ||L^-1 C_j||^2: medge_ref's bound of t_e with C_j in place of x_e (t_j >= ||C_j||^2 / Lam), plus what the error of C_j itself moves:
  ||L^-1||_2 <= 1, so |d(||M C_j||^2)| <= 2 sqrt(t_j) ||dC_j||_2:
      |dt_j| <= (ec + (n + 2) u) t_j + 2 sqrt(t_j) ||dC_j||_2
  d_j = sum_e (x*_je S_e) x*_je, q non-negative terms (S >= 0):   |dd_j| <= (q + 2) u d_j
  var_j = tau2 max(d_j - t_j, 0): absolute, because d - t cancels where the data determine the row; the difference and the product are two
  rounded operations on quantities of size <= d_j (t_j <= d_j), the 3 u tau2 d_j:
      |dvar_j| <= tau2 (|dd_j| + |dt_j|) + 3 u tau2 d_j
  h_j = sum_i C_ij g_i (n products, n sums):
      |dh_j| <= ||C_j||_2 ||dg||_2 + ||dC_j||_2 ||g||_2 + (n + 2) u sum_i |C_ij g_i|
  a_j = sum_e x*_je W_e:   |da_j| <= (q + 2) u sum_e |x*_je W_e|
  mean_j = (mu + a_j) + h_j: the issue's list ends with a and h; the two sums that join them are rounded too, each on a quantity of size at most
  |mu| + |a_j| + |h_j|, so 2 u (|mu| + |a_j| + |h_j|) is added:
      |dmean_j| <= |da_j| + |dh_j| + 2 u (|mu| + |a_j| + |h_j|)
"""
import functools

import mpmath as mp
import numpy as np

import medge_ref as er
import mloo_ref as mr

DPS = mr.DPS
EPS = mr.EPS
U = mr.U
M_POOL = 129                                                             # new rows per (n, q, kind of X): a call of m rows uses the first m

_vec = er._vec
ratio = er.ratio


def a_inverse(X, y, Xn, tau2, mu, S, W=None):
    """dict of the A^-1 form: mean, var, t, h, a, d (m lists of mpf) through A = L L^T: with T_j = L^-1 C_j and z = L^-1 r, t_j = ||T_j||^2 and
    h_j = T_j . z"""
    with mp.workdps(DPS):
        X, Xn = np.asarray(X, dtype=np.float64), np.asarray(Xn, dtype=np.float64)
        n, q = X.shape
        m = Xn.shape[0]
        Xr = [_vec(X[i]) for i in range(n)]
        Nr = [_vec(Xn[j]) for j in range(m)]
        Sm, Wm, t2, mum = _vec(S), (_vec(W) if W is not None else [mp.mpf(0)] * q), mp.mpf(float(tau2)), mp.mpf(float(mu))
        XS = [[x * s for x, s in zip(Xr[i], Sm)] for i in range(n)]
        L = [[mp.mpf(0)] * n for _ in range(n)]
        for i in range(n):
            for j in range(i + 1):
                a = mp.fdot(XS[i], Xr[j]) + (1 if i == j else 0) - mp.fdot(L[i][:j], L[j][:j])
                L[i][j] = mp.sqrt(a) if i == j else a / L[j][j]
        r = [yi - mum - mp.fdot(Xr[i], Wm) for i, yi in enumerate(_vec(y))]

        def forward(b):
            z = []
            for i in range(n):
                z.append((b[i] - mp.fdot(L[i][:i], z)) / L[i][i])
            return z
        z = forward(r)
        T = [forward([mp.fdot(XS[i], Nr[j]) for i in range(n)]) for j in range(m)]
        t = [mp.fdot(T[j], T[j]) for j in range(m)]
        h = [mp.fdot(T[j], z) for j in range(m)]
        a = [mp.fdot(Nr[j], Wm) for j in range(m)]
        d = [mp.fdot([x * s for x, s in zip(Nr[j], Sm)], Nr[j]) for j in range(m)]
        return dict(mean=[mum + a[j] + h[j] for j in range(m)], var=[t2 * (d[j] - t[j]) for j in range(m)], t=t, h=h, a=a, d=d)


def precision(X, y, Xn, tau2, mu, S, W=None):
    """(mean, var), m lists of mpf, from Cov = tau2 (D^-1 + X^T X)^-1 and E gamma = Cov (D^-1 W + X^T (y - mu)) / tau2; every S must be > 0"""
    with mp.workdps(DPS):
        X, Xn = np.asarray(X, dtype=np.float64), np.asarray(Xn, dtype=np.float64)
        n, q = X.shape
        Xm, Nm = mr._mat(X), mr._mat(Xn)
        Sm, Wm, t2, mum = _vec(S), (_vec(W) if W is not None else [mp.mpf(0)] * q), mp.mpf(float(tau2)), mp.mpf(float(mu))
        P = Xm.T * Xm
        for e in range(q):
            P[e, e] += 1 / Sm[e]
        Cov = mp.inverse(P) * t2
        b = Xm.T * mp.matrix([v - mum for v in _vec(y)])
        for e in range(q):
            b[e] += Wm[e] / Sm[e]
        eg = Cov * b / t2
        mean = Nm * eg
        NC = Nm * Cov
        return [mum + mean[j] for j in range(Nm.rows)], [sum(NC[j, e] * Nm[j, e] for e in range(q)) for j in range(Nm.rows)]


def bounds(X, y, Xn, tau2, mu, S, W, g, c, t, h, a, d, lam):
    """the first-order bounds tol_mean, tol_var (m,), and beta lam, from float64 values of the quantities of the module docstring"""
    X, Xn = np.asarray(X, dtype=np.float64), np.asarray(Xn, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64).reshape(-1)
    S = np.asarray(S, dtype=np.float64).reshape(-1)
    n, q = X.shape
    Wv = np.zeros(q) if W is None else np.asarray(W, dtype=np.float64).reshape(-1)
    t2 = float(tau2)
    ec = (n * (q + 2) + 4 * n * (3 * n + 1)) * EPS * lam
    mag = np.abs(y) + abs(float(mu)) + (np.abs(X) @ np.abs(Wv) if W is not None else 0.0)
    rho = ((q + 2) if W is not None else 1) * EPS * float(np.linalg.norm(mag))
    dg = np.sqrt(c) * (ec * float(np.linalg.norm(g)) + rho) + 4 * U * np.abs(g)
    C = (X * S[None, :]) @ Xn.T                                         # n x m
    dC = (q + 2) * U * ((np.abs(X) * np.abs(S)[None, :]) @ np.abs(Xn).T)
    dCn, Cn = np.linalg.norm(dC, axis=0), np.linalg.norm(C, axis=0)
    tol_t = (ec + (n + 2) * U) * t + 2 * np.sqrt(np.fmax(t, 0.0)) * dCn
    tol_d = (q + 2) * U * np.abs(d)
    tol_var = t2 * (tol_d + tol_t) + 3 * U * t2 * np.abs(d)
    tol_h = Cn * float(np.linalg.norm(dg)) + dCn * float(np.linalg.norm(g)) + (n + 2) * U * (np.abs(C).T @ np.abs(g))
    tol_a = (q + 2) * U * (np.abs(Xn) @ np.abs(Wv))
    tol_mean = tol_a + tol_h + 2 * U * (abs(float(mu)) + np.abs(a) + np.abs(h))
    return dict(tol_mean=tol_mean, tol_var=tol_var, beta_lam=ec)


def _a_inv_float(X, S):
    Xf, Sf = np.asarray(X, dtype=np.float64), np.asarray(S, dtype=np.float64).reshape(-1)
    A = np.eye(Xf.shape[0]) + (Xf * Sf[None, :]) @ Xf.T
    return A, np.linalg.inv(A)


def reference(X, y, Xn, tau2, mu, S, W=None):
    """One draw: dict with the float64 values mean, var (m,), their first-order bounds tol_mean, tol_var and beta_lam.  A test gates at twice the
    tol_*.  g, c = diag A^-1 and Lam come from numpy on the float64 A: they only scale a tolerance"""
    d = a_inverse(X, y, Xn, tau2, mu, S, W)
    f = lambda x: np.array([float(v) for v in x])
    A, Ai = _a_inv_float(X, S)
    Xf = np.asarray(X, dtype=np.float64)
    r = np.asarray(y, dtype=np.float64).reshape(-1) - float(mu) - (Xf @ np.asarray(W, dtype=np.float64).reshape(-1) if W is not None else 0.0)
    out = bounds(X, y, Xn, tau2, mu, S, W, Ai @ r, np.diag(Ai).copy(), f(d["t"]), f(d["h"]), f(d["a"]), f(d["d"]), float(np.linalg.eigvalsh(A)[-1]))
    out.update(mean=f(d["mean"]), var=f(d["var"]))
    return out


def numpy_bounds(X, y, Xn, tau2, mu, S, W=None):
    """bounds() for one draw with every quantity taken from a float64 evaluation instead of mpmath (for shapes where mpmath is too slow: the
    comparison of two float64 evaluations against each other, each within its own gate)"""
    X, Xn = np.asarray(X, dtype=np.float64), np.asarray(Xn, dtype=np.float64)
    S = np.asarray(S, dtype=np.float64).reshape(-1)
    A, Ai = _a_inv_float(X, S)
    Wv = None if W is None else np.asarray(W, dtype=np.float64).reshape(-1)
    r = np.asarray(y, dtype=np.float64).reshape(-1) - float(mu) - (X @ Wv if W is not None else 0.0)
    g = Ai @ r
    C = (X * S[None, :]) @ Xn.T
    t = np.sum(C * (Ai @ C), axis=0)
    return bounds(X, y, Xn, tau2, mu, S, W, g, np.diag(Ai).copy(), t, C.T @ g, (Xn @ Wv if W is not None else np.zeros(Xn.shape[0])),
                  np.sum((Xn * S[None, :]) * Xn, axis=1), float(np.linalg.eigvalsh(A)[-1]))


@functools.lru_cache(maxsize=None)
def new_rows(q, binary=False):
    """the M_POOL seeded new rows for q edges, normal or 0/1 (never written to); a call of m rows uses the first m"""
    rng = np.random.default_rng([184, q, int(binary)])
    Xn = (rng.random(size=(M_POOL, q)) < 0.4).astype(np.float64) if binary else rng.normal(size=(M_POOL, q))
    Xn.setflags(write=False)
    return Xn


@functools.lru_cache(maxsize=None)
def case_reference(n, q, d, m, binary=False):
    """reference() of draw d of mloo_ref.case(n, q, binary) for the first m of new_rows(q, binary): computed once, shared by every test that needs
    it (a row's reference does not depend on the other rows: a test with fewer rows takes a prefix)"""
    c = mr.case(n, q, binary)
    return reference(c["X"], c["y"], new_rows(q, binary)[:m], c["tau2"][d], c["mu"][d], c["S"][d], c["W"][d])


def worst_ratios(mean, var, n, q, draws, m_ref, binary=False):
    """the largest |got - reference| / tolerance of (mean, var) over the draws listed (mean, var: D x m of a call on exactly those draws, in
    order, for the first m <= m_ref new rows), and the largest beta lam met"""
    worst, bl = dict(mean=0.0, var=0.0), 0.0
    for j, d in enumerate(draws):
        ref = case_reference(n, q, d, m_ref, binary)
        bl = max(bl, ref["beta_lam"])
        for name, a in (("mean", mean), ("var", var)):
            got = np.asarray(a)[j]
            k = got.shape[0]
            worst[name] = max(worst[name], float(np.max(ratio(got, ref[name][:k], ref["tol_" + name][:k]))))
    return worst, bl
