"""CPU tests of tests/sweep_ref.py: the long-double references agree with exact (Fraction) or 50-digit (decimal) restatements on small cases,
the CPU oracle's float64 sweep (the device's algorithm) lies inside every bound, and every checker rejects planted errors a few times its bound."""
import decimal
from fractions import Fraction

import numpy as np
import pytest

import bnr_amd
import sweep_ref as sr
from oracle import bnr_oracle as bo

D = decimal.Context(prec=50)


def _oracle(n, V, R, tot, seed, normal_x=False, **hyper):
    X, y, _ = bnr_amd.make_synthetic(n, V, R, seed=11 + V, normal_x=normal_x)
    o = bo.Oracle(X, y, R, tot, seed, chain=1, pdf_mode=1, **hyper)
    o.init_prior()
    o.run(2, tot, tot)
    return X, y, o


def _row(t, j):
    return {k: t[k][j] for k in bo.COLUMNS}


def _var(seed):
    return sr.Variates(bnr_amd.lib(), seed + 1)


# ------------------------------------------------------------------------------------------------------------------ exact restatements
def _dec(x):
    return D.create_decimal(float(x))


def _dec_chol(A):
    R = len(A)
    L = [[decimal.Decimal(0)] * R for _ in range(R)]
    for j in range(R):
        d = A[j][j] - sum(L[j][k] * L[j][k] for k in range(j))
        L[j][j] = D.sqrt(d)
        for i in range(j + 1, R):
            L[i][j] = D.divide(A[i][j] - sum(L[i][k] * L[j][k] for k in range(j)), L[j][j])
    return L


def _dec_solve(L, b, trans):
    R = len(L)
    x = list(b)
    order = range(R) if not trans else range(R - 1, -1, -1)
    for i in order:
        ks = range(i) if not trans else range(i + 1, R)
        s = x[i] - sum((L[i][k] if not trans else L[k][i]) * x[k] for k in ks)
        x[i] = D.divide(s, L[i][i])
    return x


@pytest.mark.parametrize("V,R", [(4, 1), (5, 2), (6, 4)])
def test_node_reference_equals_a_50_digit_restatement(V, R):
    X, y, o = _oracle(20, V, R, 4, 77)
    t = o.t
    p, c = _row(t, 1), _row(t, 2)
    tau2 = float(c["tau2"].ravel()[0])
    ref = sr.node_ref(p, tau2, _var(77), 3)
    u, lam = p["u"], p["lam"].ravel()
    gam, S = p["gamma"].ravel(), p["S"].ravel()
    Mi_ref = sr.inv_M_ref(p["M"], "solve")
    # inv(M) and logdet M exactly: M is a float64 matrix, its Cholesky in 50 digits
    Md = [[_dec(p["M"][i, j]) for j in range(R)] for i in range(R)]
    LM = _dec_chol(Md)
    Minv = [_dec_solve(LM, _dec_solve(LM, [decimal.Decimal(int(i == j)) for i in range(R)], False), True) for j in range(R)]   # columns
    ldM = sum(2 * D.ln(LM[i][i]) for i in range(R))
    assert abs(float(Mi_ref[1] - sr.LD(str(ldM)))) <= Mi_ref[3] / 100
    for k in range(V):
        nb = [l for l in range(V) if l != k]
        e = [bo.lib().orc_edge_index(V, l, k) for l in nb]
        Um = [[_dec(u[x, l] * lam[x]) for x in range(R)] for l in nb]
        A = [[sum(D.divide(Um[a][x] * Um[a][yy], _dec(S[e[a]])) for a in range(V - 1)) for yy in range(R)] for x in range(R)]
        cc = [sum(D.divide(Um[a][x] * _dec(gam[e[a]]), _dec(S[e[a]])) for a in range(V - 1)) for x in range(R)]
        Sinv = [[D.divide(A[x][yy], _dec(tau2)) + Minv[yy][x] for yy in range(R)] for x in range(R)]
        L = _dec_chol(Sinv)
        b = [D.divide(ci, _dec(tau2)) for ci in cc]
        mu = _dec_solve(L, _dec_solve(L, b, False), True)
        ldS = sum(2 * D.ln(L[i][i]) for i in range(R))
        qf = sum(b[i] * mu[i] for i in range(R))
        Dl = _dec(p["Delta"].ravel()[0])
        logit = D.ln(Dl) - D.ln(1 - Dl) - (ldM + ldS) / 2 + qf / 2
        z = [_dec(_var(77).normal(3, sr.SITE_U_Z, k * R + r)) for r in range(R)]
        yv = _dec_solve(L, z, True)
        un = [mu[i] + yv[i] for i in range(R)]
        assert abs(float(sr.LD(str(logit)) - sr.LD(ref["logit"][k]))) <= ref["logit_err"][k] / 100 + 1e-300
        for i in range(R):
            d = abs(float(sr.LD(str(un[i])) - sr.LD(1) * ref["u_if_one"][i, k]))
            assert d <= ref["u_if_one_err"][i, k] / 100, (k, i, d)


def test_carried_sums_equal_fraction_arithmetic():
    X, y, o = _oracle(13, 5, 2, 3, 91)
    p = _row(o.t, 1)
    rr, e_rr, sq, e_sq = sr.carried_ref(p, X, y)
    mu = Fraction(float(p["mu"].ravel()[0]))
    res = [Fraction(float(y[i])) - mu - sum(Fraction(float(X[i, e])) * Fraction(float(p["gamma"][e, 0])) for e in range(X.shape[1]))
           for i in range(X.shape[0])]
    rr_x = sum(r * r for r in res)
    el, ek = sr.edge_nodes(5)
    sq_x = Fraction(0)
    for e in range(X.shape[1]):
        W = sum(Fraction(float(p["lam"][r, 0])) * Fraction(float(p["u"][r, el[e]])) * Fraction(float(p["u"][r, ek[e]])) for r in range(2))
        d = Fraction(float(p["gamma"][e, 0])) - W
        sq_x += d * d / 2 / Fraction(float(p["S"][e, 0]))
    assert abs(float(Fraction(str(rr)) - rr_x)) <= e_rr / 100
    assert abs(float(Fraction(str(sq)) - sq_x)) <= e_sq / 100


def test_M_reference_equals_a_50_digit_restatement():
    X, y, o = _oracle(20, 6, 3, 3, 5)
    c = _row(o.t, 2)
    var = _var(5)
    M, eM, Psi, df = sr.M_ref(c, 10, var, 3)
    R, V = c["u"].shape
    P = [[sum(_dec(c["u"][a, v]) * _dec(c["u"][b, v]) for v in range(V)) + (1 if a == b else 0) for b in range(R)] for a in range(R)]
    C = _dec_chol(P)
    A = [[decimal.Decimal(0)] * R for _ in range(R)]
    for j in range(R):
        A[j][j] = D.sqrt(2 * _dec(var.gamma(0.5 * (df - j), 3, sr.SITE_M_CHI, j)))
        for i in range(j + 1, R):
            A[i][j] = _dec(var.normal(3, sr.SITE_M_N, i * R + j))
    T = [_dec_solve(A, [decimal.Decimal(int(i == j)) for i in range(R)], False) for j in range(R)]   # T[j] = column j of A^-1
    B = [[sum(C[a][k] * T[k][b] for k in range(R)) for b in range(R)] for a in range(R)]             # C (A^-1)' : B[a][b] = sum C[a,k] A^-1[b,k]
    Mx = [[sum(B[a][k] * B[b][k] for k in range(R)) for b in range(R)] for a in range(R)]
    for a in range(R):
        for b in range(R):
            assert abs(float(sr.LD(str(Mx[a][b])) - M[a, b])) <= eM[a, b] / 100


# ------------------------------------------------------------------------------------------------------------------ the oracle inside the bounds
@pytest.mark.parametrize("n,V,R", [(40, 9, 3), (30, 12, 1), (25, 10, 7), (12, 17, 11)])
def test_the_oracles_float64_sweep_lies_inside_every_bound(n, V, R):
    tot, seed = 5, 4242
    X, y, o = _oracle(n, V, R, tot, seed, nu=max(10, R + 1))
    t = o.t
    var = _var(seed)
    worst = {}
    skipped = 0
    for j in range(1, tot):
        it = j + 1
        p, c = _row(t, j - 1), _row(t, j)
        t2, e, *_ = sr.tau2_ref(p, X, y, V, var, it)
        worst["tau2"] = max(worst.get("tau2", 0), sr.check(c["tau2"].ravel()[0], t2, e))
        nr = sr.node_ref(p, float(c["tau2"].ravel()[0]), var, it)
        r, bad, sk = sr.check_node(c["u"], c["xi"], nr)
        assert bad == 0
        skipped += sk
        worst["u"] = max(worst.get("u", 0), r)
        worst["theta"] = max(worst.get("theta", 0), sr.check(c["theta"].ravel()[0], *sr.theta_ref(c, V, 1.0, 1.0, var, it)))
        worst["mu"] = max(worst.get("mu", 0), sr.check(c["mu"].ravel()[0], *sr.mu_ref(c, X, y, var, it)))
        worst["Delta"] = max(worst.get("Delta", 0), sr.check(c["Delta"].ravel()[0], *sr.Delta_ref(c, V, 1.0, 1.0, var, it)))
        M, eM, _, _ = sr.M_ref(c, max(10, R + 1), var, it)
        worst["M"] = max(worst.get("M", 0), sr.check(c["M"], M, eM))
        ll, ell, _, _ = sr.lambda_sums_ref(c, p["lam"])
        lam, rob = sr.lambda_ref(ll, ell, p["pi"], var, it)
        assert np.array_equal(lam[rob], c["lam"].ravel()[rob])
        worst["pi"] = max(worst.get("pi", 0), sr.check(c["pi"], *sr.pi_ref(c, 1.01, var, it)))
    print("oracle error/bound:", {k: "%.2g" % v for k, v in worst.items()}, "xi skipped", skipped)
    assert all(v <= 1.0 for v in worst.values()), worst
    assert skipped <= max(1, (tot - 1) * V // 20)


def test_oracle_node_params_agree_with_the_reference():
    """orc_node_params (the oracle's float64 node formulas) against the reference: mu_t and the logit within their bounds"""
    X, y, o = _oracle(30, 8, 4, 3, 17)
    ref = sr.node_ref(_row(o.t, 1), float(o.t["tau2"][2].ravel()[0]), _var(17), 3)
    for k in range(8):
        rc, w, mu_t, Lc, logit = o.node_params(2, k)
        assert rc == 0
        assert abs(logit - ref["logit"][k]) <= ref["logit_err"][k]
        assert abs(w - ref["w"][k]) <= ref["w_err"][k]
    Psi, df = o.M_params(2)
    M, eM, Psi_ref, df_ref = sr.M_ref(_row(o.t, 2), 10, _var(17), 3)
    assert df == df_ref and sr.check(Psi, Psi_ref, sr.gamma_m(9) * (1 + np.abs(Psi))) <= 1


# ------------------------------------------------------------------------------------------------------------------ planted errors
@pytest.fixture(scope="module")
def case():
    X, y, o = _oracle(40, 9, 3, 8, 4242)
    return X, y, o.t, _var(4242)


def test_checkers_reject_a_perturbed_u_or_M_entry(case):
    X, y, t, var = case
    j = next(j for j in range(1, 8) if np.any(t["xi"][j] == 1))          # a row with a node in the model
    p, c = _row(t, j - 1), _row(t, j)
    nr = sr.node_ref(p, float(c["tau2"].ravel()[0]), var, j + 1)
    k = int(np.argmax(nr["xi"]))
    assert nr["xi"][k] == 1
    u = c["u"].copy()
    u[0, k] += 5 * nr["u_err"][0, k]
    assert sr.check_node(c["u"], c["xi"], nr)[0] <= 1 < sr.check_node(u, c["xi"], nr)[0]
    M, eM, _, _ = sr.M_ref(c, 10, var, j + 1)
    Mp = c["M"].copy()
    Mp[1, 0] += 5 * eM[1, 0]
    assert sr.check(c["M"], M, eM) <= 1 < sr.check(Mp, M, eM)


def test_checkers_reject_float_rounded_log_and_sqrt(case):
    X, y, t, var = case
    p, c = _row(t, 2), _row(t, 3)
    nr = sr.node_ref(p, float(c["tau2"].ravel()[0]), var, 4)
    # logdet Sigma^-1 from float32 logarithms
    L = sr.chol(nr["Sinv"])[0]
    ld32 = np.sum(2 * np.log(np.diagonal(sr.f64(L), axis1=-2, axis2=-1).astype(np.float32)).astype(np.float64), axis=-1)
    logit32 = sr.f64(nr["logit"]) + 0.5 * (sr.f64(nr["ldS"]) - ld32)
    assert np.max(np.abs(logit32 - nr["logit"]) / nr["logit_err"]) > 1
    # theta and Lambda's sd with a float32 sqrt
    th, e = sr.theta_ref(c, 9, 1.0, 1.0, var, 4)
    assert sr.check(np.float64(np.float32(th)), th, e) > 1
    M, eM, _, _ = sr.M_ref(c, 10, var, 4)
    assert sr.check(sr.f64(M).astype(np.float32).astype(np.float64), M, eM) > 1


def test_checkers_reject_an_edge_left_out(case):
    X, y, t, var = case
    p = _row(t, 2)
    rr, e_rr, sq, e_sq = sr.carried_ref(p, X, y)
    el, ek = sr.edge_nodes(9)
    q = el.size
    keep = np.arange(q) != q - 1
    p2 = dict(p, gamma=p["gamma"][keep], S=p["S"][keep])
    _, _, sq2, _ = sr.carried_ref(p2, X[:, keep], y, el[keep], ek[keep])
    assert sr.check(sr.f64(sq2), sq, e_sq) > 1
    c = _row(t, 3)
    ll, ell, _, _ = sr.lambda_sums_ref(c, p["lam"])
    c2 = dict(c, gamma=c["gamma"][keep], S=c["S"][keep])
    ll2, _, _, _ = sr.lambda_sums_ref(c2, p["lam"], el[keep], ek[keep])
    assert sr.check(sr.f64(ll2), ll, ell) > 1


def test_checkers_reject_the_jitter_added_twice(case):
    X, y, t, var = case
    p, c = _row(t, 2), _row(t, 3)
    tau2 = float(c["tau2"].ravel()[0])
    ok = sr.node_ref(p, tau2, var, 4, jitter=1)
    twice = sr.node_ref(p, tau2, var, 4, jitter=2)
    assert np.min(np.max(np.abs(twice["u_if_one"] - ok["u_if_one"]) / ok["u_if_one_err"], axis=0)) > 1   # every node sees it


def test_checkers_reject_lambda_from_the_wrong_row(case):
    X, y, t, var = case
    j = next(j for j in range(1, 8) if np.sum(t["xi"][j] == 1) >= 2)     # W depends on lambda where two nodes are in the model
    c = _row(t, j)
    lam_prev = t["lam"][j - 1]
    wrong = lam_prev.copy()
    wrong[1:, 0] = np.where(lam_prev[1:, 0] != 1.0, 1.0, -1.0)             # (the sums of r replace lambda_r: the others must differ)
    ll, ell, _, _ = sr.lambda_sums_ref(c, lam_prev)
    llw, _, _, _ = sr.lambda_sums_ref(c, wrong)
    assert sr.check(sr.f64(llw), ll, ell) > 1
