"""The gamma update's linear algebra on the GPU (gibbs.jl:420-437) against exact references (tests/linalg_ref.py), stage by stage.

Every other GPU test of this code compares the device with the CPU oracle -- the same algorithm in the same double precision -- or kernel
variants with each other.  Here each stage's output (read with the diagnostics debug_copy / debug_dims and the table) is held against the
mathematically correct value of the same operation, within a rigorous a-priori rounding bound:

  Gram, f64 (k_gram, k_gram8)    |G - G*| <= gamma_m (|X| S |X|'),  m = q + ksplit + 4 (any order of f64 FMAs, the K-groups and the slices)
  Gram, i8 (k_sdigits, k_gram_i8) |G - G*| <= (|X||X|') 2^(e - 8 i8L + 1) + gamma_(i8L + ksplit + 2) (...): S rounded to nearest, TWO-sided
  b (X pass, k_rhs)              |b - b*| <= gamma_(q + 3R + 6) ((|y| + |X| |W| + |mu|)/tau + |X| |sz| + |z2|)
  a4 (factorization + solve)     ||a4 - A^-1 b||_2 <= (8 n_pad u ||A||_2 + gamma_m || |X| S |X|' ||_2) ||a4*||_2 + 8 n_pad u ||A||_2^(1/2) ||b||_2
                                 (b: the device's own; linalg_ref.solve_bound), and below 1e-3 ||a4*|| (not vacuous)
  Y = L^-T                       columns of Y' A Y - I within (16 n_pad u ||A||_2 + gamma_m || |X| S |X|' ||_2)
  gamma (back-projection)        |gamma - gamma*| <= gamma_(n + 4) (tau S (|X|'|a4|) + tau |sz| + |W|) + gamma_(3R + 2) |u|'|lam||u|  (a4: the device's own)

The observed ratios (error / bound) are printed; a failing check names its ratio.  Where they come near 1 the bound is close to tight by
construction: the i8 digits round S to nearest, so an element can sit near the half step in every column; and at the smallest shapes (n = 1, q = 3;
n = 63, q = 15) gamma_m covers only a handful of roundings, of which one or two already happen.
"""
import time

import numpy as np
import pytest

import bnr_amd
from oracle import bnr_oracle as bo
import linalg_ref as lr

pytestmark = pytest.mark.gpu
SITE_G_Z1, SITE_G_Z2 = 19, 20                    # oracle/bnr_oracle.c draw sites of gibbs.jl:429-430


def _note(stage, r, what):
    print("ratio %-8s %.3e  %s" % (stage, r, what))
    assert r < 1.0, (stage, r, what)


def dyadic_X(rng, n, q):
    return np.asfortranarray(rng.integers(-128, 129, size=(n, q)) / 16.0)


def binary_X(rng, n, q):
    return np.asfortranarray(rng.random((n, q)) < 0.5)


def bad_S(rng, q):
    """log-uniform over [1e-6, 1e4] with some exact powers of two"""
    S = np.exp(rng.uniform(np.log(1e-6), np.log(1e4), size=q))
    S[::7] = 2.0 ** rng.integers(-19, 13, size=S[::7].size)
    return S


def _draws(key, it, q, n):
    z1 = np.array([bo.normal(key, it, SITE_G_Z1, e) for e in range(q)])
    z2 = np.array([bo.normal(key, it, SITE_G_Z2, i) for i in range(n)])
    return z1, z2


def check_gamma_update(ch, Xm, X, y, key, row, it, what, dense=True, gram_tiles=None):
    """all stage checks of the gamma update the chain last ran (row `row`, iteration id `it`); X: the model matrix as given to the chain"""
    n, q, R = ch.n, ch.q, ch.R
    dm = ch.debug_dims()
    n_pad, ks, nt, L8 = dm["n_pad"], dm["ksplit"], dm["ntile"], dm["i8L"]
    i8 = ch.last_timing(4)[0] == 1
    t = ch.fetch(row - 1, row)
    S, mu, lam = t["S"][0, :, 0], LD(t["mu"][0, 0, 0]), t["lam"][0, :, 0]
    tau2, u, g_dev = t["tau2"][1, 0, 0], t["u"][1], t["gamma"][1, :, 0]
    tau = np.sqrt(LD(tau2))
    W, Wa = lr.compute_W(u, lam)
    z1, z2 = _draws(key, it, q, n)
    sz = np.sqrt(S.astype(LD)) * z1
    m = q + ks + 4
    # ---- Gram
    if dense:
        P = ch.debug_copy(3, ks * (nt * (nt + 1) // 2) * 4096).reshape(ks, -1, 4096)
        Gd = lr.tiles_to_lower(lr.sum_partials_ld(P), nt)
        assert not np.any(Gd[n:]), (what, "pad rows of the Gram are not zero")
        Gd = Gd[:n, :n]
        Gs, Ge = lr.exact_gram(X, S)
        low = np.tril(np.ones((n, n), dtype=bool))
        absG = lr.abs_gram(X, S)
        if i8:
            _, e = np.frexp(S.max())
            cnt = np.abs(np.asarray(X, dtype=np.float64)) @ np.abs(np.asarray(X, dtype=np.float64)).T
            r = lr.check_gram_i8(np.where(low, Gd, 0), np.where(low, Gs, 0), Ge, cnt, int(e), L8, absG, L8 + ks + 2)
            d = (Gd - Gs).astype(np.float64)[low]
            print("i8 Gram error signs: %d positive, %d negative (two-sided)" % ((d > 0).sum(), (d < 0).sum()))
            _note("gram_i8", r, what)
        else:
            _note("gram_f64", lr.check_gram_f64(np.where(low, Gd, 0), np.where(low, Gs, 0), Ge, absG, m), what)
    if gram_tiles:
        P = ch.debug_copy(3, ks * (nt * (nt + 1) // 2) * 4096).reshape(ks, -1, 4096)
        ti = nt - 1
        for tj in gram_tiles:
            T = lr.sum_partials_ld(P[:, ti * (ti + 1) // 2 + tj:ti * (ti + 1) // 2 + tj + 1])[0].reshape(64, 64).T
            rows = np.arange(ti * 64, min(n, ti * 64 + 64))
            cols = np.arange(tj * 64, min(n, tj * 64 + 64))
            Xr = np.asarray(X[rows], dtype=np.float64)
            Xc = np.asarray(X[cols], dtype=np.float64)
            Xrc = np.concatenate([Xr, Xc])
            Gs, Ge = lr.exact_gram(Xrc, S, rows=np.arange(len(rows)), cols=len(rows) + np.arange(len(cols)))
            absG = lr.abs_gram(Xrc, S, rows=np.arange(len(rows)), cols=len(rows) + np.arange(len(cols)))
            Td = T[:len(rows), :len(cols)]
            if i8:
                _, e = np.frexp(S.max())
                cnt = np.abs(Xr) @ np.abs(Xc).T
                _note("gram_i8", lr.check_gram_i8(Td, Gs, Ge, cnt, int(e), L8, absG, L8 + ks + 2), what + " tile (%d,%d)" % (ti, tj))
            else:
                _note("gram_f64", lr.check_gram_f64(Td, Gs, Ge, absG, m), what + " tile (%d,%d)" % (ti, tj))
    # ---- right-hand side
    b_dev = ch.debug_copy(1, n_pad)
    assert not np.any(b_dev[n:]), (what, "pad rows of b are not zero")
    b_dev = b_dev[:n]
    XW, eXW = Xm.matvec(W)
    Xsz, eXsz = Xm.matvec(sz)
    yl = np.asarray(y, dtype=LD)
    b_ref = (yl - XW - mu) / tau - (Xsz + z2)
    absz = np.abs(sz).astype(np.float64)
    b_bnd = lr.gamma_m(q + 3 * R + 6) * ((np.abs(y) + Xm.absmatvec(Wa) + abs(float(mu))) / float(tau) + Xm.absmatvec(absz) + np.abs(z2)) \
        + (eXW / float(tau) + eXsz)
    _note("rhs", lr.check_b(b_dev, b_ref, b_bnd), what)
    # ---- factorization + solve
    a4 = ch.debug_copy(2, n_pad)
    assert not np.any(a4[n:]), (what, "pad rows of a4 are not zero")
    a4 = a4[:n]
    def applyA(v):
        return Xm.apply_A(S, v)[0]
    nAG = Xm.norm_abs_gram_inf(S)
    normb = float(np.linalg.norm(b_dev))
    if dense:
        Gs64 = lr.exact_gram(X, S)[0].astype(np.float64)
        A64 = Gs64 + np.eye(n)
        nA = lr.spectral_norm_upper(lambda v: A64 @ v, n) + 1e-12 * nAG
        a_ref = lr.refined_solve(A64, applyA, b_dev)
        norma = float(np.linalg.norm(a_ref.astype(np.float64)))
        bound = lr.solve_bound(n_pad, nA, nAG, m, normb, norma)
        print("solve bound / ||a4*|| %.2e  %s" % (bound / norma if norma else 0.0, what))
        assert bound <= 1e-3 * norma or normb == 0, (what, "vacuous solve bound", bound / norma)
        _note("solve", lr.check_solve(a4, a_ref, bound), what + " (||A|| %.2e)" % nA)
        # Y = L^-T on the block triangle k_solve_* read
        ld = 2 * n_pad + 32
        Y = lr.block_upper_Y(ch.debug_copy(0, ld * n_pad), n_pad, ld)
        def applyA_pad(v):
            r = np.asarray(v, dtype=LD).copy()
            r[:n] = applyA(v[:n])
            return r
        cols = range(n_pad) if n_pad <= 256 else sorted(set(np.random.default_rng(0).integers(0, n_pad, 24).tolist() + [0, n - 1, n_pad - 1]))
        _note("Y", lr.check_Y(Y, applyA_pad, cols, n_pad, nA, nAG, m), what)
    else:
        # residual form (no dense A on the host): ||A a4 - b|| <= ||A|| * the forward bound; ||A||_2 <= 1 + || |X| S |X|' ||_inf
        nA = 1.0 + nAG
        Aa, eA = Xm.apply_A(S, a4)
        res = float(np.linalg.norm((Aa - np.asarray(b_dev, dtype=LD)).astype(np.float64))) - float(np.linalg.norm(eA))
        norma = float(np.linalg.norm(a4))
        _note("solve", max(res, 0.0) / (nA * lr.solve_bound(n_pad, nA, nAG, m, normb, norma)), what + " (residual)")
    # ---- back-projection
    Xa, eXa = Xm.rmatvec(a4)
    g_ref = W + tau * (sz + S.astype(LD) * Xa)
    g_bnd = lr.gamma_m(n + 4) * (float(tau) * S * Xm.absrmatvec(np.abs(a4)) + float(tau) * absz + np.abs(W).astype(np.float64)) \
        + lr.gamma_m(3 * R + 2) * Wa + float(tau) * S * eXa
    _note("backproj", lr.check_gamma(g_dev, g_ref, g_bnd), what)


LD = np.longdouble


def _chain(X, y, R, seed, cid=1, tot=4, **opts):
    ch = bnr_amd.Chain(bnr_amd.XInput(X, False), y, R, tot, seed, cid)
    for k, v in opts.items():
        ch.set_option(k, v)
    return ch


def _run_case(n, V, R, Xkind, Skind, opts, group=False, seed=11):
    rng = np.random.default_rng(n * 1000 + V)
    q = V * (V + 1) // 2
    X = dyadic_X(rng, n, q) if Xkind == "dyadic" else binary_X(rng, n, q)
    y = rng.normal(size=n) * 2.0
    Xm = lr.IntMatrix(X)
    what = "n=%d V=%d R=%d X=%s S=%s %s" % (n, V, R, Xkind, Skind, opts)
    ch = _chain(X, y, R, seed, 1, **opts)
    mates = []
    ch.init_prior()
    if Skind == "bad":
        t = ch.fetch(1, 1)
        S = bad_S(rng, q)
        # keep ||A||_2 <= 1 + || |X| S |X|' ||_inf below ~1e8 (a power-of-two scale: the range and the exact powers of two stay) so that the solve bound means something
        S *= 2.0 ** min(0, int(np.floor(np.log2(1e8 / max(1.0, Xm.norm_abs_gram_inf(S))))))
        t["S"][0, :, 0] = S
        ch.load(t, 1, 1)
    if group:                           # True: two members; a count N: N members, the checked chain (id 1) the last of them
        mates = [bnr_amd.Chain.like(ch, seed, c) for c in range(2, (2 if group is True else int(group)) + 1)]
        for m in mates:
            m.init_prior()
        g = bnr_amd.Group(mates + [ch])
        for k, v in opts.items():
            if k != "gram_i8":
                g.set_option(k, v)
        g.run(2, 2, 2)
        g.close()
    else:
        ch.run(2, 2, 2)
    assert ch.counters()["chol_fail"] == 0
    if n in ODD_PAIRS:                  # variant 3 updates the trailing matrix at every other launch only: an odd number of panel pairs ends on a lazy launch
        n_pad = ch.debug_dims()["n_pad"]
        assert n_pad == ODD_PAIRS[n] and (n_pad // 64) % 2 == 1, (n, n_pad)
    key = seed + 1
    check_gamma_update(ch, Xm, X, y, key, 2, ch.iter, what + (" group sweep" if group else " sweep"))
    # the same update through the test hook (separate reduction pass where the one-panel family runs)
    ch.set_option("fuse_reduce", 0)
    ch.update("gamma", 2, 2)
    check_gamma_update(ch, Xm, X, y, key, 2, 2, what + " hook")
    for c in [ch] + mates:
        c.close()


ODD_PAIRS = {1025: 1088, 1200: 1216}          # n -> n_pad: 17 / 19 panel pairs
STAGE_CASES = [  # n, V, R, X, S, options, group
    (1, 2, 1, "dyadic", "prior", {}, False), (63, 5, 2, "dyadic", "bad", {}, False), (64, 6, 2, "dyadic", "prior", {}, False),
    (65, 8, 3, "dyadic", "bad", {}, False), (129, 12, 3, "dyadic", "prior", {}, True), (129, 12, 3, "binary", "bad", {"gram_i8": 1}, False),
    (1000, 10, 3, "dyadic", "bad", {}, False),
    (1025, 8, 2, "dyadic", "prior", {"factor_variant": 0}, False), (1025, 8, 2, "dyadic", "bad", {"factor_variant": 2}, False),
    (1025, 8, 2, "dyadic", "prior", {"factor_variant": 3}, True), (1200, 8, 2, "dyadic", "bad", {"factor_variant": 3}, False),
    (1200, 8, 2, "dyadic", "prior", {"factor_variant": 0}, False), (1200, 8, 2, "dyadic", "prior", {"factor_variant": 2}, False),
    (500, 100, 7, "dyadic", "prior", {}, False), (500, 100, 7, "binary", "bad", {"gram_i8": 1}, False),
    (500, 300, 10, "binary", "prior", {"gram_i8": 1}, False), (500, 300, 10, "binary", "bad", {"gram_i8": 0}, False),
    (2000, 200, 5, "dyadic", "prior", {}, False),
]


@pytest.mark.parametrize("n,V,R,Xkind,Skind,opts,group", STAGE_CASES)
def test_gamma_update_stages_against_exact_references(gpu, n, V, R, Xkind, Skind, opts, group):
    _run_case(n, V, R, Xkind, Skind, opts, group)


def _plain_split(n, V, ncu=256, kg=2):
    """gram_plan's choice before the buffer-window guard (bnr_hip.hip), restated"""
    n_pad = 64 * ((n + 63) // 64)
    q = V * (V + 1) // 2
    nt = n_pad // 64
    ntl = nt * (nt + 1) // 2

    def best(slots):
        bestv, bk = -1.0, 1
        for ksp in range(1, 33):
            if ksp > 1 and (q + ksp - 1) // ksp < 32 * kg:
                break
            tasks = ntl * ksp
            eff = tasks / (((tasks + slots - 1) // slots) * slots)
            sc = eff - 0.005 * ksp
            if sc > bestv:
                bestv, bk = sc, ksp
        return bk
    ks = best(2 * ncu)
    if q // ks < 1024:
        ks = best(ncu)
    return ks


def test_the_gram_window_guard_shape(gpu):
    """n = 13 000, V = 370 (q = 68 635): the plain K split is 1, one K-group would span more than the 2 GiB buffer window, the guard raises the split
    to 2 (span 0.84 of the window).  X comes as Bool (0.9 GB): with gram_i8 = 0 the device builds its f64 image and the f64 Gram addresses it through the
    window; first with gram_i8 = 1 (the default at this size), then 0 on the same chain.  Checked: the Gram's tiles of the last tile row against exact ones, b, the solve by its residual, gamma."""
    n, V, R = 13000, 370, 2
    q = V * (V + 1) // 2
    plan = (bnr_amd._capi.C.c_int32 * 4)()
    bnr_amd._capi.check(bnr_amd._capi.lib().bnr_host_gram_plan(n, V, 256, plan))
    assert plan[0] > _plain_split(n, V) == 1, (list(plan), _plain_split(n, V))
    assert plan[3] / 2048.0 > 0.5                                           # a K-group spans most of the window
    rng = np.random.default_rng(5)
    X = np.empty((n, q), dtype=np.bool_, order="F")
    for c0 in range(0, q, 4096):
        X[:, c0:c0 + 4096] = rng.random((n, min(4096, q - c0)), dtype=np.float32) < 0.5
    y = rng.normal(size=n)
    Xm = lr.IntMatrix(X, chunk=2048)
    ch = bnr_amd.Chain(bnr_amd.XInput(X, False), y, R, 3, 17, 1)
    assert ch.debug_dims()["ksplit"] == plan[0]
    ch.init_prior()
    ch.run(2, 2, 2)
    nt = ch.debug_dims()["ntile"]
    for gi8 in (1, 0):                                                    # (the byte mask of the i8 path is the default here; switching it off drops it)
        if gi8 == 0:
            ch.set_option("gram_i8", 0)
        ch.update("gamma", 2, 2)
        assert ch.counters()["chol_fail"] == 0
        check_gamma_update(ch, Xm, X, y, 18, 2, 2, "window n=%d V=%d gram_i8=%d" % (n, V, gi8), dense=False, gram_tiles=[0, nt // 2, nt - 1])
    ch.close()


# ----------------------------------------------------------------------------------------- failure counts and the NaN sentinel
def _pivot_case(n, r, fv, seed=3):
    """0/1 X that is zero except X[r, 0] = 1, so that A = I + S_0 e_r e_r': with S_0 = -2 exactly one pivot (row r) is -1"""
    V, R = 8, 2
    q = V * (V + 1) // 2
    X = np.zeros((n, q), dtype=np.bool_, order="F")
    X[r, 0] = True
    y = np.random.default_rng(seed).normal(size=n)
    ch = _chain(X, y, R, seed, 1, factor_variant=fv, gram_i8=0)
    ch.init_prior()
    ch.run(2, 2, 2)
    assert ch.counters()["chol_fail"] == 0
    return ch


def _set_S0(ch, v):
    t = ch.fetch(1, 2)
    t["S"][0, 0, 0] = v
    ch.load(t, 1, 1)


@pytest.mark.parametrize("fv", [0, 2, 3])
@pytest.mark.parametrize("n,r", [(256, 100), (256, 250)])     # a middle panel (every later panel meets the NaN column) / the last panel only
def test_a_failed_factorization_counts_once_per_gamma_update(gpu, fv, n, r):
    ch = _pivot_case(n, r, fv)
    _set_S0(ch, -2.0)
    for k in (1, 2):
        with pytest.raises(bnr_amd.BnrError) as e:
            ch.update("gamma", 2, 2)
        assert e.value.code == 3 and "G+I %d" % k in str(e.value), (fv, n, r, str(e.value))
        c = ch.counters()
        assert c["chol_fail"] == k and c["where"] == [0, 0, 0, k], (fv, n, r, k, c)
    ch.close()


@pytest.mark.parametrize("fv", [0, 3])
def test_a_failed_factorization_counts_once_in_a_group(gpu, fv):
    """the same in a lockstep group sweep: the broken member's G + I count is exactly one, its total the sum of the places; the other member has none"""
    n, r = 256, 100
    ch = _pivot_case(n, r, fv)
    mate = bnr_amd.Chain.like(ch, 3, 2)
    mate.init_prior()
    mate.run(2, 2, 2)
    _set_S0(ch, -2.0)
    g = bnr_amd.Group([mate, ch])
    g.set_option("factor_variant", fv)
    with pytest.raises(bnr_amd.BnrError) as e:
        g.run(2, 2, 2)
    assert e.value.code == 3
    c = ch.counters()
    assert c["where"][3] == 1 and c["chol_fail"] == sum(c["where"]), c
    assert mate.counters()["chol_fail"] == 0
    g.close()
    mate.close()
    ch.close()


@pytest.mark.parametrize("fv", [0, 3])
def test_a_nan_with_the_sentinel_payload_fails_fast_and_once(gpu, fv):
    """An S entry that is a NaN with the payload of the panel pipeline's "not there yet" mark (0x7FF8DEAD in the high word).  The one-panel pipeline
    canonicalises every NaN where the panel is staged, so the failing update reports status 3 with exactly one count and takes about as long as a
    healthy one (were the payload to reach the staging, the consuming waves would poll each such column BNR_PIPE_SPINS times).  The payload survives
    the Gram's f64 MFMA: the partial tile element (r, r) of debug_copy(3) holds 0x7FF8DEAD in its high word (asserted), so without the canonicalisation
    the data would alias the mark."""
    n, r = 256, 100
    ch = _pivot_case(n, r, fv)
    _set_S0(ch, 1.0)
    ch.update("gamma", 2, 2)
    times = []
    for _ in range(5):
        t0 = time.perf_counter()
        ch.update("gamma", 2, 2)
        times.append(time.perf_counter() - t0)
    healthy = float(np.median(times))
    _set_S0(ch, np.uint64(0x7FF8DEAD00000000).view(np.float64))
    t0 = time.perf_counter()
    with pytest.raises(bnr_amd.BnrError) as e:
        ch.update("gamma", 2, 2)
    failing = time.perf_counter() - t0
    assert e.value.code == 3
    c = ch.counters()
    assert c["chol_fail"] == 1 and c["where"] == [0, 0, 0, 1], c
    dm = ch.debug_dims()
    nt, ks = dm["ntile"], dm["ksplit"]
    P = ch.debug_copy(3, ks * (nt * (nt + 1) // 2) * 4096).reshape(ks, -1, 4096)
    ti = r // 64
    v = P[:, ti * (ti + 1) // 2 + ti, (r % 64) * 64 + r % 64]
    hi = [hex(int(np.float64(x).view(np.uint64)) >> 32) for x in v]
    print("NaN payload in the Gram partial (r, r) per K slice:", hi, "healthy %.4f s failing %.4f s" % (healthy, failing))
    assert any(int(np.float64(x).view(np.uint64)) >> 32 == 0x7FF8DEAD for x in v), hi       # the payload reaches the Gram's output
    assert failing < 5 * healthy + 0.005, (healthy, failing)
    ch.close()


# ----------------------------------------------------------------------------------------- tunables never change results
def _table(X, y, R, opts, rows=5):
    ch = bnr_amd.Chain(X, y, R, rows, 9, 1)
    for k, v in opts.items():
        ch.set_option(k, v)
    ch.init_prior()
    ch.run(2, rows, rows)
    assert ch.counters()["chol_fail"] == 0
    t = ch.fetch()
    ch.close()
    return t


def _same(a, b, what):
    for k in bo.COLUMNS:
        assert np.array_equal(a[k], b[k], equal_nan=True), (what, k)


def _spw_per_launch(nb, nbk, cap, family, ncu=256):
    """super blocks per update workgroup of every factorization launch, restated from launch_chol (bnr_hip.hip) with the helpers of bnr_kernels.h;
    None: the launch has one 32 x 32 block per workgroup (spw does not apply).  ncu: the MI355X's 256 CUs"""
    def nsuper(p):
        ms = (nbk - (p + 1) + 1) // 2
        return 0 if p == 0 else ms * (ms + 1) // 2 + ms * ((p + 1) // 2)

    def nsuper2(P):
        m = nbk - 2 * P - 2
        ms = (m + 1) // 2
        if P == 0 or m <= 0:
            return 0
        return ms + P if not (P & 1) else ms * (ms + 1) // 2 + ms * P     # variant 3 (lazy): the next launch's super column only at even P

    out = []
    if family == 3:
        for P in range(nbk // 2):
            ns, freecu = nsuper2(P), ncu - nb * nbk
            out.append(min(cap, max(1, -(-nb * ns // freecu))) if (freecu > 0 and nbk <= 24 and ns > 0) else 1)
        return out
    for p in range(1, nbk):                                                  # (launch 0 sums the Gram's partials: no super blocks)
        m = nbk - (p + 1)
        ntile, npan = m * (m + 1) // 2 + m * p, nbk + 1
        if nb * ntile > max(64, 2 * ncu - nb * npan):
            freecu = ncu - nb * npan
            c = 1 if p <= 4 else cap
            out.append(min(c, max(1, -(-nb * nsuper(p) // freecu))) if (freecu > 0 and nbk <= 24) else 1)
        else:
            out.append(None)
    return out


@pytest.mark.parametrize("fv", [0, 3])
def test_spw_cap_never_changes_the_tables(gpu, fv):
    """spw_cap only acts where a launch's super blocks outnumber the CUs its panels leave free, with n_pad <= 768: a lockstep group of 8 chains at
    n_pad = 704 (22 panels).  The restated launch grids differ for every cap 1..4 in both families there (asserted, so that the comparison cannot go
    vacuous); the members' tables must be bitwise those of spw_cap = 1.  (A chain alone at n_pad 512, or any n_pad >= 1024, always runs spw = 1.)"""
    n, V, R, nb = 700, 10, 3, 8
    nbk = (64 * ((n + 63) // 64)) // 32
    grids = [tuple(_spw_per_launch(nb, nbk, cap, fv)) for cap in (1, 2, 3, 4)]
    assert len(set(grids)) == 4, grids
    X, y, _ = bnr_amd.make_synthetic(n, V, R, seed=5)
    tabs = {}
    for cap in (1, 2, 3, 4):
        chains = [bnr_amd.Chain(X, y, R, 5, 9, 1)]
        chains += [bnr_amd.Chain.like(chains[0], 9, c) for c in range(2, nb + 1)]
        for c in chains:
            c.init_prior()
        g = bnr_amd.Group(chains)
        g.set_option("factor_variant", fv)
        g.set_option("spw_cap", cap)
        g.run(2, 5, 5)
        tabs[cap] = [c.fetch() for c in chains]
        assert all(c.counters()["chol_fail"] == 0 for c in chains)
        g.close()
        for c in chains:
            c.close()
    for cap in (2, 3, 4):
        for i in range(nb):
            _same(tabs[cap][i], tabs[1][i], (fv, cap, "member", i + 1))


@pytest.mark.parametrize("n,V,R", [(500, 100, 4), (200, 50, 5)])
def test_branch_ordering_never_changes_the_tables(gpu, n, V, R):
    X, y, _ = bnr_amd.make_synthetic(n, V, R, seed=6)
    ref = _table(X, y, R, {})
    for ta in (0, -1):
        for na in (-1, 0, 3):
            _same(_table(X, y, R, {"tail_after": ta, "node_after": na}), ref, (n, V, ta, na))
