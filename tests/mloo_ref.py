"""The reference of the marginal leave-one-out terms (include/bnr_mloo.h) in mpmath at 50 digits, stated two independent ways, and the error
bounds that a float64 evaluation has to meet.  Data only comes in as float64; nothing here is rounded to float64 before the results are.

For one draw phi = (tau2, mu, S, W) and an n x q matrix X:  y | phi ~ N(m, tau2 A),  m = mu + X W,  A = I + X diag(S) X^T.
  brute(...)     conditions N(m, tau2 A) on y_-i for every i, solving the (n - 1) x (n - 1) system of the other rows (n <= 17: n systems)
  identity(...)  the A^-1 identity: g = A^-1 r, c_i = (A^-1)_ii, resid_i = g_i / c_i, var_i = tau2 / c_i; logml from the Cholesky factor
The two agree to 1e-40 (tests/test_marginal_loo_host.py).

The bounds (float64, eps = 2^-52, u = eps / 2), to first order, the gate twice that for the second-order terms:
  beta = (n (q + 2) + 4 n (3 n + 1)) eps: the worst case of the Gram's q products and sums in any order, plus Higham's backward error of a
  Cholesky solve (Accuracy and Stability of Numerical Algorithms, Theorem 10.4); Lam = lambda_max(A) (numpy's eigvalsh of the reference's A:
  it only scales a tolerance).  Every eigenvalue of A is >= 1, so ||A^-1||_2 <= 1, and
      |dc_i| / c_i <= beta Lam,        |dg_i| <= sqrt(c_i) (beta Lam ||g||_2 + rho)
  rho = (q + 2) eps || |y| + |mu| + |X| |W| ||_2 bounds the rounding of r = y - mu - X W itself, which reaches g_i through row i of A^-1 (of
  2-norm <= sqrt(c_i)); the issue's bound takes r as exact, which it is only for W = 0.  A route that forms c_i from the columns of L^-1 and
  g_i = (L^-1 e_i)^T z by forward substitutions (the device's) has column-wise backward errors gamma_n |L| and so stays inside the same
  form: |dc_i| / c_i <= 2 gamma_n sqrt(Lam), |dg_i| <= 2 gamma_n Lam sqrt(c_i) ||g||, both below beta Lam.
Propagated through the formulas (ec = beta Lam, eg_i as above, one u per rounded operation of the formula itself):
      var:    var_i (ec + u)
      resid:  eg_i / c_i + |resid_i| (ec + u)
      loglik: dvar / (2 var) + (resid^2 / (2 var)) dvar / var + |resid| dresid / var + 16 eps (|log(2 pi var)| / 2 + resid^2 / (2 var) + 1)
      logml:  n ec / 2  [log det: n eigenvalues, each moved by at most beta Lam relatively to lambda_min >= 1]
              + (ec ||g||^2 + 2 ||g|| rho) / (2 tau2)  [r^T A^-1 r]
              + (n + 8) u (|n log(2 pi tau2) / 2| + sum |log L_jj| + r^T A^-1 r / (2 tau2))  [the n logs, the sums and the final operations]
"""
import functools

import mpmath as mp
import numpy as np

DPS = 50
EPS = 2.0 ** -52
U = 2.0 ** -53


def _mat(a):
    return mp.matrix(np.asarray(a, dtype=np.float64).tolist())


def _build(X, y, tau2, mu, S, W):
    """(A, m, r) in mpmath: A = I + X diag(S) X^T, m = mu + X W, r = y - m"""
    X = np.asarray(X, dtype=np.float64)
    n, q = X.shape
    Xm = _mat(X)
    XS = mp.matrix(n, q)
    Sm = [mp.mpf(float(v)) for v in np.asarray(S, dtype=np.float64).reshape(-1)]
    for i in range(n):
        for e in range(q):
            XS[i, e] = Xm[i, e] * Sm[e]
    A = mp.eye(n) + XS * Xm.T
    m = mp.matrix([mp.mpf(float(mu))] * n)
    if W is not None:
        m = m + Xm * mp.matrix([mp.mpf(float(v)) for v in np.asarray(W, dtype=np.float64).reshape(-1)])
    r = mp.matrix([mp.mpf(float(v)) for v in np.asarray(y, dtype=np.float64).reshape(-1)]) - m
    return A, m, r


def brute(X, y, tau2, mu, S, W=None):
    """(resid, var, loglik) of every row by conditioning N(m, tau2 A) on y_-i; lists of mpf"""
    with mp.workdps(DPS):
        A, _m, r = _build(X, y, tau2, mu, S, W)
        n = A.rows
        t2 = mp.mpf(float(tau2))
        C = A * t2
        resid, var, ll = [], [], []
        for i in range(n):
            o = [j for j in range(n) if j != i]
            if o:
                Coo = mp.matrix(len(o), len(o))
                cio = mp.matrix(len(o), 1)
                ro = mp.matrix(len(o), 1)
                for a, ja in enumerate(o):
                    cio[a] = C[i, ja]
                    ro[a] = r[ja]
                    for b, jb in enumerate(o):
                        Coo[a, b] = C[ja, jb]
                sol = mp.lu_solve(Coo, ro)
                sol2 = mp.lu_solve(Coo, cio)
                cm = sum(cio[a] * sol[a] for a in range(len(o)))       # E[y_i | y_-i] - m_i
                cv = C[i, i] - sum(cio[a] * sol2[a] for a in range(len(o)))
            else:
                cm, cv = mp.mpf(0), C[i, i]
            rs = r[i] - cm
            resid.append(rs)
            var.append(cv)
            ll.append(-(mp.log(2 * mp.pi) + mp.log(cv)) / 2 - rs * rs / cv / 2)
        return resid, var, ll


def identity(X, y, tau2, mu, S, W=None):
    """dict of the A^-1 identity: resid, var, loglik, c, g (lists of mpf), logml, and A as float64 (for lambda_max)"""
    with mp.workdps(DPS):
        A, _m, r = _build(X, y, tau2, mu, S, W)
        n = A.rows
        t2 = mp.mpf(float(tau2))
        L = mp.cholesky(A)
        Li = mp.matrix(n, n)                                           # L^-1 by forward substitution, column by column
        for i in range(n):
            for rr in range(i, n):
                s = mp.mpf(1 if rr == i else 0)
                for k in range(i, rr):
                    s -= L[rr, k] * Li[k, i]
                Li[rr, i] = s / L[rr, rr]
        z = Li * r
        g = Li.T * z
        c = [sum(Li[j, i] ** 2 for j in range(i, n)) for i in range(n)]
        resid = [g[i] / c[i] for i in range(n)]
        var = [t2 / c[i] for i in range(n)]
        ll = [-(mp.log(2 * mp.pi) + mp.log(var[i])) / 2 - resid[i] ** 2 / var[i] / 2 for i in range(n)]
        logs = [mp.log(L[j, j]) for j in range(n)]
        quad = sum(z[j] ** 2 for j in range(n))
        logml = -mp.mpf(n) / 2 * mp.log(2 * mp.pi * t2) - sum(logs) - quad / t2 / 2
        Af = np.array([[float(A[i, j]) for j in range(n)] for i in range(n)])
        return dict(resid=resid, var=var, loglik=ll, c=c, g=[g[i] for i in range(n)], logml=logml, A=Af, sumabslog=float(sum(abs(v) for v in logs)),
                    quad=float(quad))


def reference(X, y, tau2, mu, S, W=None):
    """One draw: dict with the float64 values resid, var, loglik (n,), logml, and their first-order bounds tol_resid, tol_var, tol_loglik (n,),
    tol_logml, with beta, lam and beta_lam = beta lam (module docstring).  A test gates at twice the tol_*."""
    X = np.asarray(X, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64).reshape(-1)
    n, q = X.shape
    d = identity(X, y, tau2, mu, S, W)
    f = lambda v: np.array([float(x) for x in v])
    resid, var, ll, c, g = f(d["resid"]), f(d["var"]), f(d["loglik"]), f(d["c"]), f(d["g"])
    lam = float(np.linalg.eigvalsh(d["A"])[-1])
    beta = (n * (q + 2) + 4 * n * (3 * n + 1)) * EPS
    ec = beta * lam
    gn = float(np.linalg.norm(g))
    mag = np.abs(y) + abs(float(mu)) + (np.abs(X) @ np.abs(np.asarray(W, dtype=np.float64).reshape(-1)) if W is not None else 0.0)
    rho = (q + 2) * EPS * float(np.linalg.norm(mag)) if W is not None else EPS * float(np.linalg.norm(mag))
    eg = np.sqrt(c) * (ec * gn + rho)
    t2 = float(tau2)
    tol_var = var * (ec + U)
    tol_resid = eg / c + np.abs(resid) * (ec + U)
    half = resid ** 2 / (2 * var)
    tol_ll = tol_var / (2 * var) + half * tol_var / var + np.abs(resid) * tol_resid / var + 16 * EPS * (np.abs(np.log(2 * np.pi * var)) / 2 + half + 1)
    tol_ml = (n * ec / 2 + (ec * gn * gn + 2 * gn * rho) / (2 * t2)
              + (n + 8) * U * (abs(n * np.log(2 * np.pi * t2) / 2) + d["sumabslog"] + d["quad"] / (2 * t2)))
    return dict(resid=resid, var=var, loglik=ll, logml=float(d["logml"]), tol_resid=tol_resid, tol_var=tol_var, tol_loglik=tol_ll, tol_logml=tol_ml,
                beta=beta, lam=lam, beta_lam=ec)


S_SCALES = (1e-3, 1.0, 1e3)
POOL = 17                                                                # draws per (n, q, kind of X): a call of D draws uses the first D


@functools.lru_cache(maxsize=None)
def case(n, q, binary=False):
    """The seeded inputs of shape (n, q) -- X normal or 0/1, y, and POOL draws of (tau2, mu, S, W), draw d with S ~ Exp(1) * S_SCALES[d % 3] --
    as a dict of float64 arrays (never written to)"""
    rng = np.random.default_rng([18, n, q, int(binary)])
    X = (rng.random(size=(n, q)) < 0.4).astype(np.float64) if binary else rng.normal(size=(n, q))
    y = rng.normal(size=n) * 2.0 + 1.0
    S = rng.exponential(size=(POOL, q)) * np.array([S_SCALES[d % 3] for d in range(POOL)])[:, None]
    out = dict(X=X, y=y, tau2=rng.exponential(size=POOL) + 0.05, mu=rng.normal(size=POOL), S=S, W=rng.normal(size=(POOL, q)) * 0.5)
    for v in out.values():
        v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def case_reference(n, q, d, binary=False):
    """reference() of draw d of case(n, q, binary): computed once, shared by every test that needs it"""
    c = case(n, q, binary)
    return reference(c["X"], c["y"], c["tau2"][d], c["mu"][d], c["S"][d], c["W"][d])


def worst_ratios(got, n, q, draws, binary=False):
    """the largest |got - reference| / tolerance of (loglik, resid, var, logml) over the draws listed (got: the four arrays of a call on exactly
    those draws, in order), and the largest beta lam met"""
    ll, rs, vr, ml = got
    worst = dict(loglik=0.0, resid=0.0, var=0.0, logml=0.0)
    bl = 0.0
    for j, d in enumerate(draws):
        ref = case_reference(n, q, d, binary)
        bl = max(bl, ref["beta_lam"])
        for name, a in (("loglik", ll), ("resid", rs), ("var", vr)):
            ratio = np.abs(np.asarray(a)[:, j] - ref[name]) / ref["tol_" + name]
            worst[name] = max(worst[name], float(np.max(np.where(np.isfinite(ratio), ratio, np.inf))))      # (a NaN never passes)
        ratio = abs(float(np.asarray(ml)[j]) - ref["logml"]) / ref["tol_logml"]
        worst["logml"] = max(worst["logml"], ratio if np.isfinite(ratio) else np.inf)
    return worst, bl


def numpy_bounds(X, y, tau2, mu, S, W=None):
    """The tol_* of reference() for one draw with every quantity taken from a float64 evaluation instead of mpmath (for shapes where mpmath is
    too slow: the comparison of two float64 evaluations against each other, each within its own gate)"""
    X = np.asarray(X, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64).reshape(-1)
    n, q = X.shape
    A = np.eye(n) + (X * np.asarray(S, dtype=np.float64)[None, :]) @ X.T
    L = np.linalg.cholesky(A)
    Ai = np.linalg.inv(A)
    r = y - float(mu) - (X @ np.asarray(W, dtype=np.float64) if W is not None else 0.0)
    g, c = Ai @ r, np.diag(Ai).copy()
    resid, var = g / c, float(tau2) / c
    lam = float(np.linalg.eigvalsh(A)[-1])
    ec = (n * (q + 2) + 4 * n * (3 * n + 1)) * EPS * lam
    gn = float(np.linalg.norm(g))
    mag = np.abs(y) + abs(float(mu)) + (np.abs(X) @ np.abs(np.asarray(W, dtype=np.float64)) if W is not None else 0.0)
    rho = ((q + 2) if W is not None else 1) * EPS * float(np.linalg.norm(mag))
    eg = np.sqrt(c) * (ec * gn + rho)
    t2 = float(tau2)
    tol_var = var * (ec + U)
    tol_resid = eg / c + np.abs(resid) * (ec + U)
    half = resid ** 2 / (2 * var)
    tol_ll = tol_var / (2 * var) + half * tol_var / var + np.abs(resid) * tol_resid / var + 16 * EPS * (np.abs(np.log(2 * np.pi * var)) / 2 + half + 1)
    tol_ml = (n * ec / 2 + (ec * gn * gn + 2 * gn * rho) / (2 * t2)
              + (n + 8) * U * (abs(n * np.log(2 * np.pi * t2) / 2) + float(np.sum(np.abs(np.log(np.diag(L))))) + float(r @ g) / (2 * t2)))
    return dict(tol_resid=tol_resid, tol_var=tol_var, tol_loglik=tol_ll, tol_logml=tol_ml, beta_lam=ec)
