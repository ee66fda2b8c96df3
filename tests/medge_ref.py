"""The reference of the conditional posterior of the edge coefficients (include/bnr_medge.h) in mpmath at 50 digits, stated two independent ways,
and the error bounds that a float64 evaluation has to meet.  Inputs are mloo_ref.case's; nothing here is rounded to float64 before the results are.

For one draw phi = (tau2, mu, S, W) and an n x q matrix X with columns x_e:  gamma | phi, y ~ N(m, Cov).
  a_inverse(...)   A = I + X diag(S) X^T, g = A^-1 (y - mu - X W):  m_e = W_e + S_e x_e^T g,  v_e = tau2 S_e (1 - S_e x_e^T A^-1 x_e)
  precision(...)   Cov = tau2 (D^-1 + X^T X)^-1,  m = Cov (D^-1 W + X^T (y - mu)) / tau2,  v = diag Cov: a q x q solve (needs S > 0)
The two agree to 1e-40 (tests/test_marginal_edges_host.py).

The bounds (float64, eps = 2^-52, u = eps / 2), to first order, the gate twice that for the second-order terms.  beta, Lam and rho are
mloo_ref's: beta = (n (q + 2) + 4 n (3 n + 1)) eps, Lam = lambda_max(A), rho = (q + 2) eps || |y| + |mu| + |X| |W| ||_2 (eps || |y| + |mu| ||_2
without W); c_i = (A^-1)_ii; ec = beta Lam.
  t_e = ||L^-1 x_e||^2.  The computed M = L^-1 has column-wise backward errors gamma_n |L|, every entry of T = M X is a dot product of at most n
  terms, and ||M||_2 <= 1 (every eigenvalue of A is >= 1): |dT_re| <= gamma_n ||M_r|| ||x_e||, so |dt_e| <= 2 sqrt(t_e) gamma_n sqrt(n) ||x_e||
  <= 2 gamma_n sqrt(n Lam) t_e  (t_e >= ||x_e||^2 / Lam), which is below beta Lam t_e; the n squares and their sums add (n + 2) u t_e:
      |dt_e| <= ec t_e + (n + 2) u t_e
  v_e = (tau2 S_e) max(1 - S_e t_e, 0): three rounded operations on quantities of size <= 1 times tau2 S_e, one on v_e itself.  Through
  1 / (1 - S_e t_e) the error is large RELATIVE to v_e when the data determine the coefficient, so the bound is absolute:
      |dv_e| <= tau2 S_e^2 |dt_e| + 3 u tau2 S_e + u v_e
  g: mloo_ref's |dg_i| <= sqrt(c_i) (ec ||g||_2 + rho) for the solve, plus 4 u |g_i|: the device forms g_i = resid_i (tau2 / var_i) from the
  factor kernel's outputs resid_i = g_i / c_i and var_i = tau2 / c_i -- two rounded divisions there, one division and one product here (the
  issue counts the last two only; the first two are roundings of the same size on the same path).
  m_e = W_e + S_e p_e, p_e = sum_i x_ie g_i (n products, n sums, then one product and one sum):
      |dm_e| <= S_e (||x_e||_2 ||dg||_2 + (n + 2) u sum_i |x_ie g_i|) + 2 u (|W_e| + S_e |p_e|)
"""
import functools

import mpmath as mp
import numpy as np

import mloo_ref as mr

DPS = mr.DPS
EPS = mr.EPS
U = mr.U


def _vec(a):
    return [mp.mpf(float(x)) for x in np.asarray(a, dtype=np.float64).reshape(-1)]


def a_inverse(X, y, tau2, mu, S, W=None):
    """dict of the A^-1 form: m, v, t, p (q lists of mpf) and g (n list), through A = L L^T: with T = L^-1 X and z = L^-1 r, t_e = ||T_e||^2,
    p_e = T_e . z and g = L^-T z.  Lists and mp.fdot instead of mp.matrix products: the same numbers several times faster"""
    with mp.workdps(DPS):
        X = np.asarray(X, dtype=np.float64)
        n, q = X.shape
        Xr = [_vec(X[i]) for i in range(n)]
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
        g = [mp.mpf(0)] * n
        for i in range(n - 1, -1, -1):
            g[i] = (z[i] - mp.fdot([L[k][i] for k in range(i + 1, n)], g[i + 1:])) / L[i][i]
        T = [forward([Xr[i][e] for i in range(n)]) for e in range(q)]
        t = [mp.fdot(T[e], T[e]) for e in range(q)]
        p = [mp.fdot(T[e], z) for e in range(q)]
        m = [Wm[e] + Sm[e] * p[e] for e in range(q)]
        v = [t2 * Sm[e] * (1 - Sm[e] * t[e]) for e in range(q)]
        return dict(m=m, v=v, t=t, p=p, g=g)


def precision(X, y, tau2, mu, S, W=None):
    """(m, v), q lists of mpf, from Cov = tau2 (D^-1 + X^T X)^-1 and m = Cov (D^-1 W + X^T (y - mu)) / tau2; every S must be > 0"""
    with mp.workdps(DPS):
        X = np.asarray(X, dtype=np.float64)
        n, q = X.shape
        Xm = mr._mat(X)
        Sm, Wm, t2, mum = _vec(S), (_vec(W) if W is not None else [mp.mpf(0)] * q), mp.mpf(float(tau2)), mp.mpf(float(mu))
        P = Xm.T * Xm
        for e in range(q):
            P[e, e] += 1 / Sm[e]
        Cov = mp.inverse(P) * t2
        yc = mp.matrix([v - mum for v in _vec(y)])
        b = Xm.T * yc
        for e in range(q):
            b[e] += Wm[e] / Sm[e]
        m = Cov * b / t2
        return [m[e] for e in range(q)], [Cov[e, e] for e in range(q)]


def bounds(X, y, tau2, mu, S, W, g, c, t, p, v, lam):
    """the first-order bounds tol_m, tol_v (q,), and beta lam, from float64 values of the quantities of the module docstring"""
    X = np.asarray(X, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64).reshape(-1)
    S = np.asarray(S, dtype=np.float64).reshape(-1)
    n, q = X.shape
    Wv = np.zeros(q) if W is None else np.asarray(W, dtype=np.float64).reshape(-1)
    t2 = float(tau2)
    ec = (n * (q + 2) + 4 * n * (3 * n + 1)) * EPS * lam
    mag = np.abs(y) + abs(float(mu)) + (np.abs(X) @ np.abs(Wv) if W is not None else 0.0)
    rho = ((q + 2) if W is not None else 1) * EPS * float(np.linalg.norm(mag))
    dg = np.sqrt(c) * (ec * float(np.linalg.norm(g)) + rho) + 4 * U * np.abs(g)
    tol_t = ec * t + (n + 2) * U * t
    tol_v = t2 * S * S * tol_t + 3 * U * t2 * np.abs(S) + U * np.abs(v)
    xn = np.linalg.norm(X, axis=0)
    tol_m = np.abs(S) * (xn * float(np.linalg.norm(dg)) + (n + 2) * U * (np.abs(X).T @ np.abs(g))) + 2 * U * (np.abs(Wv) + np.abs(S * p))
    return dict(tol_m=tol_m, tol_v=tol_v, beta_lam=ec)


def reference(X, y, tau2, mu, S, W=None):
    """One draw: dict with the float64 values m, v (q,), their first-order bounds tol_m, tol_v and beta_lam.  A test gates at twice the tol_*.
    c = diag A^-1 and Lam come from numpy on the float64 A: they only scale a tolerance"""
    d = a_inverse(X, y, tau2, mu, S, W)
    f = lambda x: np.array([float(a) for a in x])
    Xf, Sf = np.asarray(X, dtype=np.float64), np.asarray(S, dtype=np.float64).reshape(-1)
    A = np.eye(Xf.shape[0]) + (Xf * Sf[None, :]) @ Xf.T
    out = bounds(X, y, tau2, mu, S, W, f(d["g"]), np.diag(np.linalg.inv(A)).copy(), f(d["t"]), f(d["p"]), f(d["v"]), float(np.linalg.eigvalsh(A)[-1]))
    out.update(m=f(d["m"]), v=f(d["v"]))
    return out


def numpy_bounds(X, y, tau2, mu, S, W=None):
    """bounds() for one draw with every quantity taken from a float64 evaluation instead of mpmath (for shapes where mpmath is too slow: the
    comparison of two float64 evaluations against each other, each within its own gate)"""
    X = np.asarray(X, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64).reshape(-1)
    S = np.asarray(S, dtype=np.float64).reshape(-1)
    n, q = X.shape
    A = np.eye(n) + (X * S[None, :]) @ X.T
    Ai = np.linalg.inv(A)
    r = y - float(mu) - (X @ np.asarray(W, dtype=np.float64).reshape(-1) if W is not None else 0.0)
    g, c = Ai @ r, np.diag(Ai).copy()
    t = np.sum(X * (Ai @ X), axis=0)
    p = X.T @ g
    v = float(tau2) * S * np.fmax(1.0 - S * t, 0.0)
    return bounds(X, y, tau2, mu, S, W, g, c, t, p, v, float(np.linalg.eigvalsh(A)[-1]))


def ratio(got, ref, tol):
    """|got - ref| / tol, elementwise; where the bound is 0 (a column of X that is all zero with W_e = 0: nothing is rounded) 0 for an exact
    value and inf otherwise; a value that is not finite never passes"""
    err = np.abs(np.asarray(got, dtype=np.float64) - ref)
    with np.errstate(all="ignore"):
        r = np.where(tol > 0, err / tol, np.where(err == 0, 0.0, np.inf))
    return np.where(np.isfinite(r), r, np.inf)


@functools.lru_cache(maxsize=None)
def case_reference(n, q, d, binary=False):
    """reference() of draw d of mloo_ref.case(n, q, binary): computed once, shared by every test that needs it"""
    c = mr.case(n, q, binary)
    return reference(c["X"], c["y"], c["tau2"][d], c["mu"][d], c["S"][d], c["W"][d])


def worst_ratios(m, v, n, q, draws, binary=False):
    """the largest |got - reference| / tolerance of (m, v) over the draws listed (m, v: D x q of a call on exactly those draws, in order), and
    the largest beta lam met"""
    worst, bl = dict(m=0.0, v=0.0), 0.0
    for j, d in enumerate(draws):
        ref = case_reference(n, q, d, binary)
        bl = max(bl, ref["beta_lam"])
        for name, a in (("m", m), ("v", v)):
            worst[name] = max(worst[name], float(np.max(ratio(np.asarray(a)[j], ref[name], ref["tol_" + name]))))
    return worst, bl
