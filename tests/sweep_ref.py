"""Extended-precision host references, with a-priori bounds on the device's float64 error, for the stages of a sweep other than the
gamma update (numpy + Python stdlib only): the node update (u, xi), tau2 and its carried sums, M and inv(M), theta, mu, Delta, Lambda, pi.

Every function takes state rows in the reference table layout (`Chain.fetch`: u (R, V), M (R, R), lam (R, 1), pi (R, 3), gamma / S (q, 1),
xi (V, 1), scalars (1, 1)) and the draw-site variates, and returns what the device computes, restated in np.longdouble, together with an
elementwise bound of the device's error.

The bounds.  Sums and dot products use Higham's gamma_m = m u / (1 - m u) over |terms| (any order of summation: the device's partitions of
a sum over threads, waves and blocks are all covered).  The R x R factorizations use the backward-error results of Higham, "Accuracy and
Stability of Numerical Algorithms" (2nd ed.): Cholesky L L' = A + dA with |dA| <= gamma_(R+1) |L| |L'| (Thm 10.3), solves through it
(A + dA) x = b with |dA| <= gamma_(3R+1) |L| |L'| (Thm 10.4), triangular inverses |T - L^-1| <= gamma_R |T| |L| |T| (Thm 8.5 applied by
columns).  Those backward errors, and the input errors carried from the previous stage, are propagated to each output by its exact first-order
sensitivity (evaluated in long double): d(A^-1 b) = A^-1 (db - dA x), d logdet A = tr(A^-1 dA), d chol(A) = L Phi(L^-1 dA L^-T).  The
first-order result is doubled (SAFETY) to cover the second-order terms; the module asserts that those are small (the relative backward
error times the condition number below 1e-3) before a bound is used.  Device libm (log, exp, sqrt, cos in the variates) may differ from
glibc in the last bits: every variate gets a budget of VARIATE_ULPS ulps and every elementary function LIBM_ULPS.

The reference's own error.  The same chains of operations evaluated in long double (64-bit significand, unit roundoff 2^-64) carry the
same bounds with u replaced by 2^-64: 2^-11 = 1/2048 of the device's.  So the reference error is below 1/100 of every device bound.
"""
import math

import numpy as np

LD = np.longdouble
assert np.finfo(LD).nmant >= 63, "the references need an x87 80-bit long double"
U = 2.0 ** -53
SAFETY = 2.0
LIBM_ULPS = 2.0
VARIATE_ULPS = 8.0
SITE_TAU2, SITE_XI, SITE_U_Z, SITE_THETA, SITE_DELTA, SITE_DELTA_COIN = 16, 17, 18, 23, 24, 25
SITE_M_CHI, SITE_M_N, SITE_MU, SITE_LAMBDA, SITE_PI = 26, 27, 28, 29, 30
LAMBDA_VALUES = (0.0, 1.0, -1.0)
LOG2PI = np.log(LD(2) * LD("3.14159265358979323846264338327950288"))


def gamma_m(m):
    return m * U / (1.0 - m * U)


def f64(x):
    return np.asarray(x, dtype=np.float64)


# ------------------------------------------------------------------------------------------------------------------ variates
class Variates:
    """The draw-site primitives of the library's host copy (bitwise the device's arithmetic, up to libm): bnr_host_*.  That copy and the device's
    own variates are held to an independent reference by tests/rng_ref.py (a normal's VARIATE_ULPS follows there from LIBM_ULPS)"""

    def __init__(self, lib, seed):
        import ctypes as C
        self.L, self.seed, self._C = lib, int(seed), C

    def uniform(self, it, site, elem, att=0):
        out = (self._C.c_double * 2)()
        self.L.bnr_host_uniform2(self.seed, it, site, elem, att, out)
        return out[0]

    def uniform2(self, it, site, elem, att=0):
        """both halves of the counter's draw: the pair (ru, rv) of one rejection attempt"""
        out = (self._C.c_double * 2)()
        self.L.bnr_host_uniform2(self.seed, it, site, elem, att, out)
        return out[0], out[1]

    def normal(self, it, site, elem, att=0):
        return self.L.bnr_host_normal(self.seed, it, site, elem, att)

    def gamma(self, shape, it, site, elem):
        return self.L.bnr_host_gamma(self.seed, float(shape), it, site, elem)


# ------------------------------------------------------------------------------------------------------------------ small dense LD algebra
def chol(A):
    """batched lower Cholesky in long double: (L, ok); A (..., R, R)"""
    A = np.asarray(A, dtype=LD)
    R = A.shape[-1]
    L = np.zeros_like(A)
    ok = np.ones(A.shape[:-2], dtype=bool)
    for j in range(R):
        d = A[..., j, j] - np.sum(L[..., j, :j] ** 2, axis=-1)
        ok &= d > 0
        ljj = np.sqrt(np.where(d > 0, d, LD(1)))
        L[..., j, j] = ljj
        if j + 1 < R:
            s = A[..., j + 1:, j] - np.einsum("...ik,...k->...i", L[..., j + 1:, :j], L[..., j, :j])
            L[..., j + 1:, j] = s / ljj[..., None]
    return L, ok


def fwd(L, B):
    """L^-1 B (B (..., R) or (..., R, m))"""
    vec = B.ndim == L.ndim - 1
    X = np.array(B[..., None] if vec else B, dtype=LD)
    R = L.shape[-1]
    for i in range(R):
        X[..., i, :] = (X[..., i, :] - np.einsum("...k,...km->...m", L[..., i, :i], X[..., :i, :])) / L[..., i, i][..., None]
    return X[..., 0] if vec else X


def bwd_t(L, B):
    """L^-T B"""
    vec = B.ndim == L.ndim - 1
    X = np.array(B[..., None] if vec else B, dtype=LD)
    R = L.shape[-1]
    for i in range(R - 1, -1, -1):
        X[..., i, :] = (X[..., i, :] - np.einsum("...k,...km->...m", L[..., i + 1:, i], X[..., i + 1:, :])) / L[..., i, i][..., None]
    return X[..., 0] if vec else X


def spd_inverse(L):
    R = L.shape[-1]
    I = np.broadcast_to(np.eye(R, dtype=LD), L.shape).copy()
    return bwd_t(L, fwd(L, I))


def tri_inverse(L):
    R = L.shape[-1]
    return fwd(L, np.broadcast_to(np.eye(R, dtype=LD), L.shape).copy())


def absm(x):
    return np.abs(f64(x))


def mm(a, b):
    return np.matmul(a, b)


def tr(a):
    return np.swapaxes(a, -1, -2)


def chol_sens(L, E):
    """elementwise bound of |d chol(A)| for |dA| <= E, first order: |L| Phi(|L^-1| E |L^-T|) (Phi: lower triangle, diagonal halved --
    taken whole here)"""
    Li = absm(tri_inverse(L))
    return mm(absm(L), np.tril(mm(mm(Li, E), tr(Li))))


def second_order_ok(E, Ainv):
    """the first-order bounds hold (with SAFETY) while ||A^-1|| ||dA|| stays small"""
    return float(np.max(np.sum(mm(absm(Ainv), E), axis=-1))) < 1e-3


# ------------------------------------------------------------------------------------------------------------------ edges
def edge_index(V, l, k):
    l, k = np.maximum(l, k), np.minimum(l, k)
    return k * V - (k * (k - 1)) // 2 + (l - k)


def edge_nodes(V):
    """(el, ek): the nodes of edge e, column-wise lower triangle (utils.jl:50-55)"""
    el, ek = [], []
    for k in range(V):
        for l in range(k, V):
            el.append(l)
            ek.append(k)
    return np.array(el), np.array(ek)


def compute_W(u, lam, el, ek, m=None):
    """W_e = sum_r lam_r u_rl u_rk in long double, and the device's error bound of its own sum (gamma_m sum |terms|, m = 2R+1 unless given)"""
    U = np.asarray(u, dtype=LD)
    lam = np.asarray(lam, dtype=LD).ravel()
    terms = U[:, el] * lam[:, None] * U[:, ek]
    R = U.shape[0]
    return terms.sum(axis=0), gamma_m(2 * R + 1 if m is None else m) * absm(terms).sum(axis=0)


# ------------------------------------------------------------------------------------------------------------------ node update
def inv_M_ref(M, route):
    """inv(M) and logdet M in long double with the bounds of the device's route: 'solve' (k_node's hooks: Cholesky, then forward and
    backward solves per column) or 'tri' (the scalar tail: Cholesky, T = L^-1, inv(M) = T' T)."""
    M = np.asarray(M, dtype=LD)
    R = M.shape[-1]
    L, ok = chol(M)
    assert np.all(ok), "M is not positive definite"
    Minv = spd_inverse(L)
    aL, aMi = absm(L), absm(Minv)
    G = mm(aL, tr(aL))
    EM = gamma_m(R + 1) * G
    if route == "solve":
        E = gamma_m(3 * R + 1) * mm(mm(aMi, G), aMi)
    else:
        T = absm(tri_inverse(L))
        E = mm(mm(aMi, EM), aMi) + 2 * gamma_m(R) * mm(tr(T), mm(mm(T, aL), T)) + gamma_m(R) * mm(tr(T), T)
    assert second_order_ok(EM, Minv)
    logd = 2 * np.log(np.diagonal(L, axis1=-2, axis2=-1))
    ld = logd.sum(axis=-1)
    e_ld = np.sum(aMi * EM, axis=(-1, -2)) + (LIBM_ULPS * U + gamma_m(R)) * absm(logd).sum(axis=-1)
    return Minv, ld, SAFETY * E, SAFETY * e_ld


def node_ref(prev, tau2, var, it, nodes=None, Minv=None, route="solve", jitter=0):
    """update_u_xi! (gibbs.jl:293-402) of the nodes `nodes` (default all) from row `prev` and this row's tau2.
    Minv: None -> inv(M) and logdet M from prev's M by `route` ('solve': the hook; 'tri': what the tail hands to a sweep's k_node);
    jitter: number of ladder steps the device takes (0, 1 or 2; 1e-5, then 4e-5 more on the diagonal).
    Returns a dict: u (R, K), u_err, xi (K), robust (K: the decision is farther from its boundary than the bound), w, logit, logit_err ..."""
    u = f64(prev["u"])
    R, V = u.shape
    m = V - 1
    nodes = np.arange(V) if nodes is None else np.asarray(nodes)
    K = len(nodes)
    lam = f64(prev["lam"]).ravel()
    gam, S = f64(prev["gamma"]).ravel(), f64(prev["S"]).ravel()
    Delta = float(f64(prev["Delta"]).ravel()[0])
    # the V - 1 other nodes of every k, in the device's order a = 0..V-2
    a = np.arange(m)[None, :]
    kk = nodes[:, None]
    l = np.where(a < kk, a, a + 1)
    e = edge_index(V, l, kk)
    h, g = S[e], gam[e]                                                    # (K, m)
    Um = (u * lam[:, None])[:, l]                                          # (R, K, m): u lam, exact
    UmL = np.asarray(Um, dtype=LD)
    hL, gL = np.asarray(h, dtype=LD), np.asarray(g, dtype=LD)
    A = np.einsum("xka,yka->kxy", UmL, UmL / hL[None])                      # U' H^-1 U
    c = np.einsum("xka,ka->kx", UmL, gL / hL)                              # U' H^-1 g
    absA = np.einsum("xka,yka->kxy", np.abs(Um), np.abs(Um) / h[None])
    absc = np.einsum("xka,ka->kx", np.abs(Um), np.abs(g) / h)
    eA, ec = gamma_m(m + 2) * absA, gamma_m(m + 2) * absc
    if Minv is None:
        Mi, ldM, eMi, eldM = inv_M_ref(f64(prev["M"]), route)
    else:
        Mi, ldM, eMi, eldM = Minv
    Mi = np.broadcast_to(np.asarray(Mi, dtype=LD), (K, R, R))
    t2 = LD(tau2)
    Sinv = A / t2 + Mi
    ES = eA / tau2 + eMi + gamma_m(2) * (absA / tau2 + absm(Mi))
    for step in range(jitter):
        add = LD("1e-5") if step == 0 else LD("4e-5")
        Sinv = Sinv + add * np.eye(R, dtype=LD)
        ES = ES + U * np.eye(R) * absm(Sinv)
    L, ok = chol(Sinv)
    assert np.all(ok), "Sigma^-1 not positive definite in the reference"
    aL = absm(L)
    G = mm(aL, tr(aL))
    Eall = ES + gamma_m(3 * R + 1) * G
    Sig = spd_inverse(L)
    assert second_order_ok(Eall, Sig), "too ill-conditioned for a first-order bound"
    aSig = absm(Sig)
    b = c / t2
    eb = ec / tau2 + U * absm(b)
    mu = np.einsum("kxy,ky->kx", Sig, b)
    amu = absm(mu)
    e_mu = np.einsum("kxy,ky->kx", aSig, eb + np.einsum("kxy,ky->kx", Eall, amu))
    logd = 2 * np.log(np.diagonal(L, axis1=-2, axis2=-1))
    ldS = logd.sum(axis=-1)
    e_ldS = np.sum(aSig * Eall, axis=(-1, -2)) + (LIBM_ULPS * U + gamma_m(R)) * absm(logd).sum(axis=-1)
    qf = np.sum(b * mu, axis=-1)
    e_qf = 2 * np.sum(amu * eb, axis=-1) + np.einsum("kx,kxy,ky->k", amu, Eall, amu) + gamma_m(R) * np.sum(absm(b * mu), axis=-1)
    lD, l1D = np.log(LD(Delta)), np.log1p(-LD(Delta))
    logit = lD - l1D - (ldM + ldS) / 2 + qf / 2
    e_logit = SAFETY * (0.5 * (e_ldS + e_qf)) + 0.5 * eldM + LIBM_ULPS * U * (abs(float(lD)) + abs(float(l1D))) \
        + gamma_m(4) * (abs(float(lD)) + abs(float(l1D)) + 0.5 * (absm(ldM) + absm(ldS) + absm(qf)))
    with np.errstate(over="ignore"):
        w = 1 / (1 + np.exp(logit))
    wf = f64(w)
    e_w = e_logit * np.exp(np.minimum(e_logit, 50.0)) * wf * (1 - wf) + (LIBM_ULPS + 3) * U
    # update_xi (gibbs.jl:385-402): xi = 1 iff ua <= 1 - w (w <= 0: 1, w >= 1: 0 without a draw)
    ua = np.array([var.uniform(it, SITE_XI, int(k)) for k in nodes])
    thr = 1 - w
    xi = (np.asarray(ua, dtype=LD) <= thr).astype(np.float64)
    xi = np.where(f64(thr) <= 0, 0.0, xi)
    robust = np.abs(f64(np.asarray(ua, dtype=LD) - thr)) > e_w
    # u_k = xi (mu_t + L^-T z)
    z = np.array([[var.normal(it, SITE_U_Z, int(k) * R + r) for r in range(R)] for k in nodes])
    y = bwd_t(L, np.asarray(z, dtype=LD))
    ay = absm(y)
    Lit = absm(tr(tri_inverse(L)))
    dL = chol_sens(L, Eall)
    e_y = np.einsum("kxy,ky->kx", Lit, np.einsum("kyx,ky->kx", dL, ay) + gamma_m(R) * np.einsum("kyx,ky->kx", aL, ay)
                    + VARIATE_ULPS * U * np.abs(z))
    un = mu + y
    e_u = SAFETY * (e_mu + e_y) + 2 * U * absm(un)
    return dict(u=(xi[:, None] * un).T, u_err=(xi[:, None] * e_u).T, u_if_one=un.T, u_if_one_err=e_u.T, xi=xi, robust=robust, w=wf, w_err=e_w,
                logit=f64(logit), logit_err=e_logit, ua=ua, nodes=nodes, mu_t=f64(mu), ldS=f64(ldS), ldM=f64(ldM), Sinv=Sinv)


def check_node(got_u, got_xi, ref):
    """(largest |u - u_ref| / bound over the nodes whose xi decision is robust, number of robust decisions that differ, skipped count)"""
    nodes, rob = ref["nodes"], ref["robust"]
    gu = f64(got_u)[:, nodes]
    gx = f64(got_xi).ravel()[nodes]
    bad = int(np.sum(rob & (gx != ref["xi"])))
    ok = rob & (gx == ref["xi"])
    err = np.abs(gu - ref["u"])[:, ok]
    bnd = ref["u_err"][:, ok]
    r = ratio(err, bnd)
    # a node whose decision is too close to call is still checked for u when the device took the reference's decision
    close = ~rob & (gx == ref["xi"])
    if np.any(close):
        r = max(r, ratio(np.abs(gu - ref["u"])[:, close], ref["u_err"][:, close]))
    return r, bad, int(np.sum(~rob))


# ------------------------------------------------------------------------------------------------------------------ tau2 and its sums
def xgamma(X, gam):
    """X gamma in long double and the device's bound gamma_q |X| |gamma|"""
    X = np.asarray(X, dtype=np.float64)
    g = f64(gam).ravel()
    xg = np.asarray(X, dtype=LD) @ np.asarray(g, dtype=LD)
    return xg, gamma_m(X.shape[1] + 1) * (np.abs(X) @ np.abs(g))


def carried_ref(row, X, y, el=None, ek=None):
    """rr = |y - mu - X gamma|^2 and sig_q = sum_e ((gamma_e - W_e)^2 / 2) / S_e of one row (gibbs.jl:270-273): (rr, e_rr, sigq, e_sigq)"""
    y = f64(y)
    n = y.size
    mu = float(f64(row["mu"]).ravel()[0])
    xg, e_xg = xgamma(X, row["gamma"])
    r = np.asarray(y, dtype=LD) - LD(mu) - xg
    ar = absm(r)
    e_r = e_xg + gamma_m(2) * (np.abs(y) + abs(mu) + absm(xg))
    rr = np.sum(r * r)
    e_rr = SAFETY * np.sum(2 * ar * e_r) + gamma_m(n + 1) * float(np.sum(ar * ar))
    u = f64(row["u"])
    R, V = u.shape
    if el is None:
        el, ek = edge_nodes(V)
    W, eW = compute_W(u, row["lam"], el, ek)
    gam, S = f64(row["gamma"]).ravel(), f64(row["S"]).ravel()
    d = np.asarray(gam, dtype=LD) - W
    t = d * d / 2 / np.asarray(S, dtype=LD)
    e_d = eW + U * (np.abs(gam) + absm(W))
    q = gam.size
    e_sigq = SAFETY * float(np.sum(absm(d) * e_d / S)) + gamma_m(q + 3) * float(np.sum(absm(t)))
    return rr, e_rr, np.sum(t), e_sigq


def tau2_ref(prev, X, y, V, var, it, el=None, ek=None):
    """update_tau2! (gibbs.jl:267-277): tau2 = (rr/2 + sig_q) / Gamma(n/2 + V(V+1)/4) from row prev; (tau2, bound, rr, e_rr, sigq, e_sigq)"""
    n = f64(y).size
    rr, e_rr, sq, e_sq = carried_ref(prev, X, y, el, ek)
    G = var.gamma(n / 2.0 + V * (V + 1) / 4.0, it, SITE_TAU2, 0)
    t2 = (rr / 2 + sq) / LD(G)
    e = (e_rr / 2 + e_sq) / G + (gamma_m(3) + VARIATE_ULPS * U) * float(t2)
    return t2, e, rr, e_rr, sq, e_sq


# ------------------------------------------------------------------------------------------------------------------ M
def M_ref(row, nu, var, it):
    """update_M! (gibbs.jl:516-547): Psi = I + sum_v u_v u_v'; C = chol(Psi); M = (C A^-T)(C A^-T)' with the Bartlett factor A.
    Returns (M, bound, Psi, df)."""
    u = f64(row["u"])
    R, V = u.shape
    xi = f64(row["xi"]).ravel()
    uL = np.asarray(u, dtype=LD)
    Psi = np.eye(R, dtype=LD) + uL @ uL.T
    ePsi = gamma_m(V + 1) * (np.eye(R) + np.abs(u) @ np.abs(u).T)
    df = float(nu) + float(np.sum(~(np.abs(xi) <= 0.1)))
    C, ok = chol(Psi)
    assert ok, "Psi is not positive definite"
    aC = absm(C)
    EC = ePsi + gamma_m(R + 1) * (aC @ aC.T)
    assert second_order_ok(EC, spd_inverse(C))
    dC = chol_sens(C, EC)
    A = np.zeros((R, R), dtype=LD)
    eA = np.zeros((R, R))
    for j in range(R):
        gj = var.gamma(0.5 * (df - j), it, SITE_M_CHI, j)
        A[j, j] = np.sqrt(2 * LD(gj))
        eA[j, j] = (VARIATE_ULPS / 2 + 2) * U * float(A[j, j])
        for i in range(j + 1, R):
            A[i, j] = var.normal(it, SITE_M_N, i * R + j)
            eA[i, j] = VARIATE_ULPS * U * abs(float(A[i, j]))
    T = tri_inverse(A)
    aT = absm(T)
    eT = aT @ eA @ aT + gamma_m(R) * (aT @ absm(A) @ aT)
    B = C @ T.T
    aB = absm(B)
    eB = dC @ aT.T + aC @ eT.T + gamma_m(R) * (aC @ aT.T)
    M = B @ B.T
    eM = SAFETY * (eB @ aB.T + aB @ eB.T) + gamma_m(R) * (aB @ aB.T)
    return M, eM, Psi, df


# ------------------------------------------------------------------------------------------------------------------ theta, mu, Delta, pi
def theta_ref(row, V, zeta, iota, var, it):
    """update_theta! (gibbs.jl:476-479): theta = Gamma(zeta + V(V+1)/2) * 2 / (2 iota + sum S)"""
    S = f64(row["S"]).ravel()
    sS = np.sum(np.asarray(S, dtype=LD))
    g = var.gamma(zeta + (V * (V + 1)) / 2.0, it, SITE_THETA, 0)
    th = LD(g) * 2 / (2 * LD(iota) + sS)
    e = (gamma_m(S.size + 1) * float(sS) / float(2 * LD(iota) + sS) + gamma_m(4) + VARIATE_ULPS * U) * float(th)
    return th, e


def mu_ref(row, X, y, var, it):
    """update_mu! (gibbs.jl:565-570): mu = sum(y - X gamma)/n + sqrt(tau2/n) z"""
    y = f64(y)
    n = y.size
    xg, e_xg = xgamma(X, row["gamma"])
    r = np.asarray(y, dtype=LD) - xg
    s = np.sum(r)
    e_s = float(np.sum(e_xg)) + gamma_m(n + 1) * float(np.sum(np.abs(y) + absm(xg)))
    tau2 = float(f64(row["tau2"]).ravel()[0])
    z = var.normal(it, SITE_MU, 0)
    sd = np.sqrt(LD(tau2) / n)
    mu = s / n + sd * LD(z)
    e = e_s / n + gamma_m(2) * abs(float(s / n)) + (gamma_m(4) + LIBM_ULPS * U + VARIATE_ULPS * U) * abs(float(sd * LD(z)))
    return mu, e


def Delta_ref(row, V, aDelta, bDelta, var, it):
    """update_Delta! (gibbs.jl:496-499, 130-140) with its degenerate branches: (Delta, bound)"""
    sx = float(np.sum(f64(row["xi"])))
    a, b = aDelta + sx, bDelta + (V - sx)
    if a > 0 and b > 0:
        g1, g2 = var.gamma(a, it, SITE_DELTA, 0), var.gamma(b, it, SITE_DELTA, 1)
        return LD(g1) / (LD(g1) + LD(g2)), (gamma_m(2) + 2 * VARIATE_ULPS * U) * g1 / (g1 + g2)
    if a > 0:
        return LD(1), 0.0
    if b > 0:
        return LD(0), 0.0
    return (LD(0) if var.uniform(it, SITE_DELTA_COIN, 0) < 0.5 else LD(1)), 0.0


def pi_ref(row, eta, var, it):
    """update_pi! (gibbs.jl:620-636): pi_r = g / sum g, g_c ~ Gamma(alpha_c) with alpha from lambda_r: (pi (R, 3), bound)"""
    lam = f64(row["lam"]).ravel()
    R = lam.size
    P = np.zeros((R, 3), dtype=LD)
    for r in range(R):
        base = float(np.power(float(r + 1), eta))
        al = [base, 2.0, 1.0] if lam[r] == 1.0 else ([base + 1.0, 1.0, 1.0] if lam[r] == 0.0 else [base, 1.0, 2.0])
        g = [LD(var.gamma(al[c], it, SITE_PI, 3 * r + c)) for c in range(3)]
        P[r] = np.array(g) / (g[0] + g[1] + g[2])
    return P, (gamma_m(4) + 2 * VARIATE_ULPS * U) * f64(P)


# ------------------------------------------------------------------------------------------------------------------ Lambda
def lambda_sums_ref(row, prev_lam, el=None, ek=None):
    """the 3R log-likelihood sums of update_Lambda! (gibbs.jl:586-613): ll[r, c] = sum_e logpdf(Normal(W_c,e, sqrt(tau2 S_e)), gamma_e),
    W_c = W with lambda_r (of row i-1) replaced by (0, 1, -1)[c], u, gamma, S, tau2 of this row.  Also sum S (update_theta!).
    Returns (ll (R, 3), e_ll (R, 3), sumS, e_sumS)."""
    u = f64(row["u"])
    R, V = u.shape
    if el is None:
        el, ek = edge_nodes(V)
    lam = f64(prev_lam).ravel()
    gam, S = f64(row["gamma"]).ravel(), f64(row["S"]).ravel()
    q = gam.size
    tau2 = float(f64(row["tau2"]).ravel()[0])
    uL = np.asarray(u, dtype=LD)
    dr = uL[:, el] * uL[:, ek]                                              # (R, q)
    W = np.sum(np.asarray(lam, dtype=LD)[:, None] * dr, axis=0)
    aW = np.sum(np.abs(lam)[:, None] * absm(dr), axis=0)
    sd = np.sqrt(LD(tau2) * np.asarray(S, dtype=LD))
    lsd = np.log(sd) + LOG2PI / 2
    alsd = absm(np.log(sd)) + float(LOG2PI / 2)
    ll = np.zeros((R, 3), dtype=LD)
    e_ll = np.zeros((R, 3))
    gL = np.asarray(gam, dtype=LD)
    for r in range(R):
        for c in range(3):
            Wc = W + (LD(LAMBDA_VALUES[c]) - LD(lam[r])) * dr[r]
            eWc = gamma_m(2 * R + 4) * (aW + 2 * absm(dr[r]))
            zz = (gL - Wc) / sd
            t = -zz * zz / 2 - lsd
            azz = absm(zz)
            e_z = (eWc + U * (np.abs(gam) + absm(Wc))) / f64(sd) + gamma_m(3) * azz        # sd itself: sqrt(tau2 S) to 3 u
            e_t = azz * e_z + (LIBM_ULPS + 3) * U * alsd + gamma_m(3) + gamma_m(3) * azz * azz
            ll[r, c] = np.sum(t)
            e_ll[r, c] = SAFETY * float(np.sum(e_t)) + gamma_m(q + 1) * float(np.sum(absm(t)))
    sS = np.sum(np.asarray(S, dtype=LD))
    return ll, e_ll, sS, gamma_m(q + 1) * float(sS)


def _lse(x):
    mx = np.max(x)
    return mx if mx == -np.inf else mx + np.log(np.sum(np.exp(x - mx)))


def lambda_ref(ll, e_ll, prev_pi, var, it):
    """the categorical draws of update_Lambda!: weights pi_prev[r, c] exp(ll_c - max), u01 sum(w) against the cumulative weights.
    Returns (lam (R), robust (R))"""
    R = ll.shape[0]
    pi = f64(prev_pi).reshape(R, 3)
    lam = np.zeros(R)
    rob = np.zeros(R, dtype=bool)
    for r in range(R):
        w = np.asarray(pi[r], dtype=LD) * np.exp(ll[r] - ll[r].max())
        tot = w.sum()
        cum = np.cumsum(w) / tot
        ua = var.uniform(it, SITE_LAMBDA, r)
        i = 0
        while i < 2 and cum[i] < LD(ua):
            i += 1
        lam[r] = LAMBDA_VALUES[i]
        # P_k = A / (A + B), A = sum_(c <= k) w_c, B = sum_(c > k) w_c; log(B / A) is off by at most d = 2 max_c e_ll[r, c]
        d = LD(2 * float(max(e_ll[r])))
        with np.errstate(divide="ignore"):
            lw = np.log(np.asarray(pi[r], dtype=LD)) + (ll[r] - ll[r].max())
        rob[r] = True
        for k in range(2):
            la, lb = _lse(lw[:k + 1]), _lse(lw[k + 1:])
            if la == -np.inf or lb == -np.inf:                                 # a zero prior weight: P_k is 0 or 1 exactly
                pmin = pmax = LD(0) if la == -np.inf else LD(1)
            else:
                with np.errstate(over="ignore"):
                    pmin, pmax = 1 / (1 + np.exp(lb - la + d)), 1 / (1 + np.exp(lb - la - d))
            if pmin - 16 * U <= LD(ua) <= pmax + 16 * U:
                rob[r] = False
    return lam, rob


# ------------------------------------------------------------------------------------------------------------------ checks
def ratio(err, bound):
    err = np.asarray(err, dtype=np.float64)
    bound = np.asarray(bound, dtype=np.float64)
    if err.size == 0:
        return 0.0
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, err / bound)
    return float(np.max(r))


def check(got, ref, bound):
    """largest |got - ref| / bound (got float64, ref long double)"""
    return ratio(absm(np.asarray(got, dtype=LD) - np.asarray(ref, dtype=LD)), bound)
