"""The reference of the Rao-Blackwellised covariance of the edge coefficients (include/bnr_mcov.h) in mpmath at 50 digits, the conditional covariance
of a draw stated two independent ways, and the error bounds that a float64 evaluation has to meet.  Built on medge_ref; inputs are mloo_ref.case's,
taken as exactly the float64 numbers they are: nothing here is rounded before the results are.

For one draw phi = (tau2, mu, S, W) and an n x q matrix X:  gamma | phi, y ~ N(m, C).
  a_inverse_cov(...)   A = I + X D X^T = L L^T, T = L^-1 X, t_ab = T_a . T_b:   C_ab = tau2 (S_a [a == b] - S_a S_b t_ab);  m as medge_ref.a_inverse
  precision_cov(...)   C = tau2 (D^-1 + X^T X)^-1, the q x q inverse that medge_ref.precision forms (needs S > 0)
The two agree to 1e-40 (tests/test_marginal_edge_cov_host.py).  The mixture over D = K nd draws with omega_s = w_k / nd:
  mean = sum omega m_s,   within = sum omega C_s,   between = sum omega (m_s - mean)(m_s - mean)^T,   cov = within + between.

The bounds (float64, eps = 2^-52, u = eps / 2), to first order; a test gates at twice the bound for the second-order terms.  ec_s = beta Lam_s is
medge_ref's of draw s, tol_m its bound on m.
  t_ab.  medge_ref bounds the computed T column by column, ||dT_a|| <= (ec / 2) ||T_a|| to first order (its |dt_aa| <= ec t_aa); by Cauchy-Schwarz
  |d(T_a . T_b)| <= ||dT_a|| ||T_b|| + ||T_a|| ||dT_b|| <= ec sqrt(t_aa t_bb), and the n products and their sums add (n + 2) u sum_i |T_ia T_ib|
  <= (n + 2) u sqrt(t_aa t_bb):
      |dt_ab| <= (ec + (n + 2) u) sqrt(t_aa t_bb)
  The scaling of the header.  scale_a = fl(fl(sqrt tau2) S_a) carries 2 u, T'_ia = fl(scale_a T_ia) one more: 3 u per factor, 6 u per product
  T'_ia T'_ib, whose sum stands for tau2 S_a S_b t_ab:
      |d(tau2 S_a S_b t_ab)| <= tau2 S_a S_b (ec + (n + 8) u) sqrt(t_aa t_bb)
  The diagonal's term fl(tau2 S_a) carries u.
  The sums over draws and chains: nd terms per chain, K chains, a division by nd, a product with w_k and the last difference, (nd + K + 4) u times
  the sum of the absolute terms.  (The device continues ONE accumulator through the draws of a chain, so the roundings of a draw's n / 4 steps are
  relative to the chain's running sum, not to the draw's own: in the worst case n nd u sum |terms| instead.  beta >= 24 n^2 u, so that stays below
  ec sum |terms| while nd <= 24 n, which holds for every shape tested; the gate's factor 2 is left for it and no term is added.)
      tol_within[a, b] = sum_s omega_s tau2_s S_sa S_sb (ec_s + (n + 8) u) sqrt(t_s,aa t_s,bb) + [a == b] u sum_s omega_s tau2_s S_sa
                         + (nd + K + 4) u sum_s omega_s (tau2_s S_sa [a == b] + tau2_s S_sa S_sb |t_s,ab|)
  mean_a = sum omega m_sa:    tol_mean[a] = sum_s omega_s tol_m[s, a] + (nd + K + 4) u sum_s omega_s |m_sa|
  between, centred before the product (bnr_cov's bound): c_sa = m_sa - mean_a is computed with |dc_sa| <= e_sa = tol_m[s, a] + tol_mean[a] + u |c_sa|,
  a product c_sa c_sb with |c_sa| e_sb + |c_sb| e_sa + u |c_sa c_sb|:
      tol_between[a, b] = sum_s omega_s (|c_sa| e_sb + |c_sb| e_sa) + (nd + K + 5) u sum_s omega_s |c_sa c_sb|
  cov = within + between:     tol_cov = tol_within + tol_between + u |cov|
"""
import functools

import mpmath as mp
import numpy as np

import medge_ref as er
import mloo_ref as mr

DPS = mr.DPS
EPS = mr.EPS
U = mr.U


def a_inverse_cov(X, y, tau2, mu, S, W=None):
    """(m (q list of mpf), C, t (q x q lists of mpf)) of one draw through A = L L^T and T = L^-1 X"""
    with mp.workdps(DPS):
        X = np.asarray(X, dtype=np.float64)
        n, q = X.shape
        Xr = [er._vec(X[i]) for i in range(n)]
        Sm, t2 = er._vec(S), mp.mpf(float(tau2))
        XS = [[x * s for x, s in zip(Xr[i], Sm)] for i in range(n)]
        L = [[mp.mpf(0)] * n for _ in range(n)]
        for i in range(n):
            for j in range(i + 1):
                a = mp.fdot(XS[i], Xr[j]) + (1 if i == j else 0) - mp.fdot(L[i][:j], L[j][:j])
                L[i][j] = mp.sqrt(a) if i == j else a / L[j][j]
        T = []
        for e in range(q):
            z = []
            for i in range(n):
                z.append((Xr[i][e] - mp.fdot(L[i][:i], z)) / L[i][i])
            T.append(z)
        t = [[None] * q for _ in range(q)]
        for a in range(q):
            for b in range(a + 1):
                t[a][b] = t[b][a] = mp.fdot(T[a], T[b])
        C = [[t2 * ((Sm[a] if a == b else 0) - Sm[a] * Sm[b] * t[a][b]) for b in range(q)] for a in range(q)]
        return er.a_inverse(X, y, tau2, mu, S, W)["m"], C, t


def precision_cov(X, tau2, S):
    """C = tau2 (D^-1 + X^T X)^-1 as q x q lists of mpf; every S must be > 0"""
    with mp.workdps(DPS):
        X = np.asarray(X, dtype=np.float64)
        q = X.shape[1]
        Xm = mr._mat(X)
        Sm = er._vec(S)
        P = Xm.T * Xm
        for e in range(q):
            P[e, e] += 1 / Sm[e]
        Cov = mp.inverse(P) * mp.mpf(float(tau2))
        return [[Cov[a, b] for b in range(q)] for a in range(q)]


@functools.lru_cache(maxsize=None)
def case_draw(n, q, d, binary=False):
    """draw d of mloo_ref.case(n, q, binary), every edge: dict with m (q), C, t (q x q) as lists of mpf, and tau2, S, tol_m, ec as float64"""
    c = mr.case(n, q, binary)
    m, C, t = a_inverse_cov(c["X"], c["y"], c["tau2"][d], c["mu"][d], c["S"][d], c["W"][d])
    ref = er.case_reference(n, q, d, binary)
    return dict(m=m, C=C, t=t, tau2=float(c["tau2"][d]), S=np.array(c["S"][d]), tol_m=ref["tol_m"], ec=ref["beta_lam"])


def numpy_draw(X, y, tau2, mu, S, W=None):
    """case_draw's dict for one draw with every quantity taken from a float64 evaluation (for shapes where mpmath is too slow: two float64
    evaluations against each other, each within its own gate)"""
    X = np.asarray(X, dtype=np.float64)
    S = np.asarray(S, dtype=np.float64).reshape(-1)
    n, q = X.shape
    A = np.eye(n) + (X * S[None, :]) @ X.T
    t = X.T @ np.linalg.solve(A, X)
    Wv = np.zeros(q) if W is None else np.asarray(W, dtype=np.float64).reshape(-1)
    g = np.linalg.solve(A, np.asarray(y, dtype=np.float64).reshape(-1) - float(mu) - X @ Wv)
    b = er.numpy_bounds(X, y, tau2, mu, S, W)
    C = float(tau2) * (np.diag(S) - (S[:, None] * t) * S[None, :])
    return dict(m=Wv + S * (X.T @ g), C=C, t=t, tau2=float(tau2), S=S, tol_m=b["tol_m"], ec=b["beta_lam"])


def mixture(draws, n, K, nd, cols=None, weights=None):
    """The mixture of the draws listed (dicts of case_draw / numpy_draw, chain k's nd first in order k) at the columns cols (None: all): dict with the
    float64 values mean (c), cov, within, between (c x c) and their first-order bounds tol_mean, tol_cov, tol_within, tol_between, and the largest
    ec met (ec_max).  A test gates at twice the tol_*."""
    D = K * nd
    assert len(draws) == D
    q = len(draws[0]["m"])
    sel = list(range(q)) if cols is None else [int(e) for e in cols]
    c = len(sel)
    w = [1.0 / K] * K if weights is None else [float(x) for x in weights]
    f = lambda x: np.array([[float(v) for v in row] for row in x]) if isinstance(x[0], list) else np.array([float(v) for v in x])
    same = np.array([[1.0 if sel[a] == sel[b] else 0.0 for b in range(c)] for a in range(c)])
    if not isinstance(draws[0]["C"], list):                               # float64 draws (numpy_draw): the moments in long double
        ld = np.longdouble
        omf = np.array([w[s // nd] / nd for s in range(D)])
        msf = np.stack([np.asarray(d["m"], dtype=np.float64)[sel] for d in draws])
        mean = np.einsum("s,sa->a", omf.astype(ld), msf.astype(ld))
        within = sum(ld(omf[s]) * np.asarray(d["C"])[np.ix_(sel, sel)].astype(ld) for s, d in enumerate(draws))
        cen = msf.astype(ld) - mean[None, :]
        between = np.einsum("s,sa,sb->ab", omf.astype(ld), cen, cen)
        cov = within + between
        mean, within, between, cov, cen = (np.asarray(x, dtype=np.float64) for x in (mean, within, between, cov, cen))
    else:
      with mp.workdps(DPS):
        om = [mp.mpf(w[s // nd]) / nd for s in range(D)]
        ms = [[d["m"][e] if isinstance(d["m"][e], mp.mpf) else mp.mpf(float(d["m"][e])) for e in sel] for d in draws]
        Cs = [[[d["C"][a][b] for b in sel] for a in sel] for d in draws]
        mean = [mp.fsum(om[s] * ms[s][a] for s in range(D)) for a in range(c)]
        within = [[mp.fsum(om[s] * Cs[s][a][b] for s in range(D)) for b in range(c)] for a in range(c)]
        cen = [[ms[s][a] - mean[a] for a in range(c)] for s in range(D)]
        between = [[mp.fsum(om[s] * cen[s][a] * cen[s][b] for s in range(D)) for b in range(c)] for a in range(c)]
        cov = [[within[a][b] + between[a][b] for b in range(c)] for a in range(c)]
        mean, within, between, cov, cen = f(mean), f(within), f(between), f(cov), f(cen)
        msf = f(ms)
        omf = np.array([float(o) for o in om])
    tol_w, sumabs_w, diag_u = np.zeros((c, c)), np.zeros((c, c)), np.zeros((c, c))
    tol_m = np.stack([np.asarray(d["tol_m"], dtype=np.float64)[sel] for d in draws])
    for s, d in enumerate(draws):
        S = d["S"][sel]
        t = np.array([[float(d["t"][a][b]) for b in sel] for a in sel]) if isinstance(d["t"], list) else np.asarray(d["t"])[np.ix_(sel, sel)]
        ss = d["tau2"] * np.outer(S, S)
        rt = np.sqrt(np.outer(np.diag(t), np.diag(t)))
        tol_w += omf[s] * ss * (d["ec"] + (n + 8) * U) * rt
        diag_u += omf[s] * d["tau2"] * same * S[:, None]
        sumabs_w += omf[s] * (d["tau2"] * same * S[:, None] + ss * np.abs(t))
    tol_w = tol_w + U * diag_u + (nd + K + 4) * U * sumabs_w
    tol_mean = omf @ tol_m + (nd + K + 4) * U * (omf @ np.abs(msf))
    e = tol_m + tol_mean[None, :] + U * np.abs(cen)
    ac = np.abs(cen)
    tol_b = np.einsum("s,sa,sb->ab", omf, ac, e) + np.einsum("s,sa,sb->ab", omf, e, ac) + (nd + K + 5) * U * np.einsum("s,sa,sb->ab", omf, ac, ac)
    return dict(mean=mean, cov=cov, within=within, between=between, tol_mean=tol_mean, tol_within=tol_w, tol_between=tol_b,
                tol_cov=tol_w + tol_b + U * np.abs(cov), ec_max=max(d["ec"] for d in draws))


@functools.lru_cache(maxsize=None)
def case_mixture(n, q, K, nd, binary=False, cols=None, weights=None):
    """mixture() of the first K nd draws of mloo_ref.case(n, q, binary) (cols, weights: tuples or None): computed once, shared"""
    return mixture([case_draw(n, q, d, binary) for d in range(K * nd)], n, K, nd, cols, weights)


def long_case(n, q, D, binary=False):
    """The inputs of a mixture of D > mloo_ref.POOL draws: draw s is draw s % POOL of mloo_ref.case(n, q, binary) (the pool repeated)"""
    c = mr.case(n, q, binary)
    idx = np.arange(D) % mr.POOL
    return dict(X=c["X"], y=c["y"], tau2=c["tau2"][idx], mu=c["mu"][idx], S=c["S"][idx], W=c["W"][idx]), idx


@functools.lru_cache(maxsize=None)
def long_mixture(n, q, K, nd, binary=False):
    _c, idx = long_case(n, q, K * nd, binary)
    return mixture([case_draw(n, q, int(d), binary) for d in idx], n, K, nd)


ratio = er.ratio


def worst(got, ref, names=("mean", "cov", "within")):
    """the largest |got - ref| / tol over the entries of each named result"""
    return {k: float(np.max(ratio(got[k], ref[k], ref["tol_" + k]))) for k in names}
