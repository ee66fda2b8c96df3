"""CPU tests of tests/linalg_ref.py: the references of the gamma update's linear algebra are exact (against fractions.Fraction), and the
checkers the GPU tests use reject device outputs with one planted error each (computed here in numpy, no GPU)."""
from fractions import Fraction

import numpy as np
import pytest

import linalg_ref as lr


def frac(x):
    return Fraction(*np.longdouble(x).as_integer_ratio())


def dyadic_X(rng, n, q, binary):
    if binary:
        return (rng.random((n, q)) < 0.5).astype(np.float64)
    return rng.integers(-128, 129, size=(n, q)) / 16.0


def bad_S(rng, q):
    """log-uniform over [1e-6, 1e4] with some exact powers of two (the GPU tests' badly scaled S)"""
    S = np.exp(rng.uniform(np.log(1e-6), np.log(1e4), size=q))
    S[::5] = 2.0 ** rng.integers(-20, 13, size=S[::5].size)
    return S


@pytest.mark.parametrize("binary", [True, False])
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_exact_gram_matches_fractions(binary, seed):
    rng = np.random.default_rng(seed)
    n, q = 5, 11
    X = dyadic_X(rng, n, q, binary)
    S = bad_S(rng, q) if seed else rng.random(q)
    G, err = lr.exact_gram(X, S)
    absG = lr.abs_gram(X, S)
    for i in range(n):
        for j in range(n):
            exact = sum(Fraction(X[i, k]) * Fraction(S[k]) * Fraction(X[j, k]) for k in range(q))
            assert abs(frac(G[i, j]) - exact) <= Fraction(err[i, j]), (i, j)
            # and the bound is of long-double size, not float64 size
            assert err[i, j] <= 1e-17 * absG[i, j] + 1e-300, (i, j, err[i, j])


def test_int_matrix_products_and_operator_match_fractions():
    rng = np.random.default_rng(4)
    n, q = 6, 10
    X = dyadic_X(rng, n, q, False)
    S = bad_S(rng, q)
    v = rng.normal(size=n) * np.exp(rng.uniform(-20, 20, size=n))
    w = rng.normal(size=q)
    Xm = lr.IntMatrix(X, chunk=3)
    t, et = Xm.rmatvec(v)
    for k in range(q):
        exact = sum(Fraction(X[i, k]) * Fraction(v[i]) for i in range(n))
        assert abs(frac(t[k]) - exact) <= Fraction(et[k])
    r, er = Xm.matvec(w)
    for i in range(n):
        exact = sum(Fraction(X[i, k]) * Fraction(w[k]) for k in range(q))
        assert abs(frac(r[i]) - exact) <= Fraction(er[i])
    Av, ea = Xm.apply_A(S, v)
    for i in range(n):
        exact = Fraction(v[i]) + sum(Fraction(X[i, k]) * Fraction(S[k]) * sum(Fraction(X[j, k]) * Fraction(v[j]) for j in range(n)) for k in range(q))
        assert abs(frac(Av[i]) - exact) <= Fraction(ea[i])


def test_refined_solve_and_norm_bound():
    rng = np.random.default_rng(5)
    n, q = 40, 60
    X = dyadic_X(rng, n, q, True)
    S = bad_S(rng, q)
    Xm = lr.IntMatrix(X)
    G, _ = lr.exact_gram(X, S)
    A64 = G.astype(np.float64) + np.eye(n)
    b = rng.normal(size=n)
    a = lr.refined_solve(A64, lambda v: Xm.apply_A(S, v)[0], b)
    # the residual in exact arithmetic, through Fractions on a few rows
    for i in (0, n // 2, n - 1):
        row = [Fraction(1) * (i == j) + sum(Fraction(X[i, k]) * Fraction(S[k]) * Fraction(X[j, k]) for k in range(q)) for j in range(n)]
        res = sum(row[j] * frac(a[j]) for j in range(n)) - Fraction(b[i])
        assert abs(float(res)) <= 1e-15 * np.abs(b).max()
    nA = lr.spectral_norm_upper(lambda v: A64 @ v, n)
    assert nA >= np.linalg.eigvalsh(A64).max() * (1 - 1e-12)
    assert Xm.norm_abs_gram_inf(S) + 1 >= nA * (1 - 1e-12)


def test_compute_W_matches_fractions():
    rng = np.random.default_rng(6)
    R, V = 3, 5
    u = rng.normal(size=(R, V))
    lam = np.array([1.0, 0.0, -1.0])
    W, Wa = lr.compute_W(u, lam)
    e = 0
    for k in range(V):
        for l in range(k, V):
            exact = sum(Fraction(u[r, l]) * Fraction(lam[r]) * Fraction(u[r, k]) for r in range(R))
            assert abs(frac(W[e]) - exact) <= Fraction(1e-17) * (1 + abs(exact))
            assert Wa[e] >= abs(float(exact)) * (1 - 1e-15)
            e += 1


# ----------------------------------------------------------------------------------------- planted errors
def _synthetic_device_gram(X, S, ksplit):
    """what the device writes: float64 K-split partial tiles [ksplit][ntl][64 x 64], tile (i, j) at [j 64 + i]"""
    n, q = X.shape
    n_pad = 64 * ((n + 63) // 64)
    nt = n_pad // 64
    Xp = np.zeros((n_pad, q))
    Xp[:n] = X
    bounds = np.linspace(0, q, ksplit + 1).astype(int)
    P = np.zeros((ksplit, nt * (nt + 1) // 2, 4096))
    for ks in range(ksplit):
        k0, k1 = bounds[ks], bounds[ks + 1]
        Gk = (Xp[:, k0:k1] * S[k0:k1]) @ Xp[:, k0:k1].T
        for ti in range(nt):
            for tj in range(ti + 1):
                P[ks, ti * (ti + 1) // 2 + tj] = Gk[ti * 64:(ti + 1) * 64, tj * 64:(tj + 1) * 64].T.reshape(-1)
    return P, n_pad, nt


def _gram_ratio(P, X, S, nt, ksplit):
    n, q = X.shape
    Gd = lr.tiles_to_lower(lr.sum_partials_ld(P), nt)[:n, :n]
    Gs, Ge = lr.exact_gram(X, S)
    low = np.tril(np.ones((n, n), dtype=bool))
    absG = lr.abs_gram(X, S)
    return lr.check_gram_f64(np.where(low, Gd, 0), np.where(low, Gs, 0), Ge, absG, q + ksplit + 1)


def test_gram_checker_rejects_planted_errors():
    rng = np.random.default_rng(7)
    n, q, ks = 130, 12, 2                   # q small: the order-independent bound gamma_(q + ksplit + 1) is ~15 ulp, so 100 ulp must show
    X = dyadic_X(rng, n, q, False)
    S = bad_S(rng, q)
    P, n_pad, nt = _synthetic_device_gram(X, S, ks)
    assert _gram_ratio(P, X, S, nt, ks) < 1
    # one element off by 100 ulp (the largest element of tile (2, 1))
    Q = P.copy()
    t = 2 * 3 // 2 + 1
    idx = int(np.argmax(np.abs(P[0, t] + P[1, t])))
    tot = P[0, t, idx] + P[1, t, idx]
    Q[0, t, idx] += 100 * np.spacing(abs(tot))
    assert _gram_ratio(Q, X, S, nt, ks) > 1
    # one K-slice partial tile missing
    Q = P.copy()
    Q[1, 4] = 0.0
    assert _gram_ratio(Q, X, S, nt, ks) > 1
    # one tile transposed
    Q = P.copy()
    Q[:, 3] = Q[:, 3].reshape(ks, 64, 64).transpose(0, 2, 1).reshape(ks, 4096)
    assert _gram_ratio(Q, X, S, nt, ks) > 1


def _solve_case(rng, n, q):
    X = dyadic_X(rng, n, q, True)
    S = rng.random(q) * 0.1
    n_pad = 64 * ((n + 63) // 64)
    Xm = lr.IntMatrix(X)
    G, _ = lr.exact_gram(X, S)
    A64 = G.astype(np.float64) + np.eye(n)
    b = rng.normal(size=n)
    a_ref = lr.refined_solve(A64, lambda v: Xm.apply_A(S, v)[0], b)
    nA = lr.spectral_norm_upper(lambda v: A64 @ v, n)
    nAG = Xm.norm_abs_gram_inf(S)
    return X, S, n_pad, Xm, A64, b, a_ref, nA, nAG


def test_solve_checker_rejects_a_perturbed_a4():
    rng = np.random.default_rng(8)
    n, q = 60, 15
    X, S, n_pad, Xm, A64, b, a_ref, nA, nAG = _solve_case(rng, n, q)
    bound = lr.solve_bound(n_pad, nA, nAG, q + 2, np.linalg.norm(b), float(np.linalg.norm(a_ref.astype(np.float64))))
    assert bound <= 1e-3 * float(np.linalg.norm(a_ref.astype(np.float64)))           # not vacuous
    L = np.linalg.cholesky(A64)
    a_dev = np.linalg.solve(L.T, np.linalg.solve(L, b))                               # a float64 solve: passes
    assert lr.check_solve(a_dev, a_ref, bound) < 1
    a_bad = a_dev + 1e-9 * np.linalg.norm(a_dev) * (np.arange(n) == n // 3)
    assert lr.check_solve(a_bad, a_ref, bound) > 1


def test_Y_checker_rejects_a_perturbed_entry():
    rng = np.random.default_rng(9)
    n, q = 70, 15
    X, S, n_pad, Xm, A64, b, a_ref, nA, nAG = _solve_case(rng, n, q)
    Ap = np.eye(n_pad)
    Ap[:n, :n] = A64
    Y = np.linalg.inv(np.linalg.cholesky(Ap)).T                                        # upper triangular, = L^-T

    def applyA(v):
        r = np.asarray(v, dtype=np.longdouble).copy()
        r[:n] = Xm.apply_A(S, v[:n])[0]
        return r
    cols = range(n_pad)
    assert lr.check_Y(Y, applyA, cols, n_pad, nA, nAG, q + 2) < 1
    Yb = Y.copy()
    i, j = 40, 50                                                                       # a block-upper entry (block 1, block 1)
    Yb[i, j] += 1e-9 * np.abs(Y).max()
    assert lr.check_Y(Yb, applyA, cols, n_pad, nA, nAG, q + 2) > 1


def test_block_upper_Y_reads_the_device_layout():
    n_pad = 64
    ld = 2 * n_pad + 32
    E = np.arange(n_pad * ld, dtype=np.float64)                                        # column-major (ld x n_pad)
    Y = lr.block_upper_Y(E, n_pad, ld)
    assert Y[0, 63] == E[63 * ld + n_pad + 0] and Y[31, 0] == E[0 * ld + n_pad + 31]
    assert Y[32, 0] == 0 and Y[32, 33] == E[33 * ld + n_pad + 32]


def test_i8_bound_is_two_sided_and_tight_on_rounded_digits():
    """k_sdigits' arithmetic restated: S rounded to nearest on the grid 2^(e - BITS), BITS = 8L - 2; the Gram of the rounded S against the exact
    one has errors of BOTH signs (so the one-sided form 0 <= G* - G is wrong), within (|X||X|') 2^(e - 8L + 1)"""
    rng = np.random.default_rng(10)
    n, q, L = 64, 400, 7
    X = dyadic_X(rng, n, q, True)
    S = bad_S(rng, q)
    _, e = np.frexp(S.max())
    up = np.ldexp(1.0, 8 * L - 2 - e)
    Sr = np.floor(S * up + 0.5) / up
    Gs, Ge = lr.exact_gram(X, S)
    Gr, Gre = lr.exact_gram(X, Sr)
    d = (Gr - Gs).astype(np.float64)
    count = X @ X.T
    assert (d > 0).any() and (d < 0).any()
    assert lr.ratio(np.abs(d), count * 2.0 ** (e - 8 * L + 1) + Ge + Gre) <= 1
