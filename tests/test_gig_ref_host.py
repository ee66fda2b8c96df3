"""CPU tests of tests/gig_ref.py, the reference of update_D!'s draw S ~ GIG(1/2, chi, psi).

The reference shares its formulas with gig.jl, so they are first proved at 50 digits (mpmath) to sample the GIG density, over a grid of
omega covering the three samplers and both sides of 0.2 and 3: the ratio-of-uniforms rectangle contains the region and touches it (extrema
by findroot on the stationarity condition), the three-piece hat lies above the density, its areas are the integrals of its pieces, the
inversion inverts the hat's CDF, the acceptance tests are U <= g(X) / hat(X), and the long-double value agrees with a 50-digit evaluation
within 1/100 of its bound.  Then the library's host copy (bnr_host_gig, bnr_host_gig_attempts) and the CPU oracle's float64 S lie inside
every bound with the same accepted attempt, within the skip and non-vacuity conditions, and the checker rejects planted errors."""
import mpmath
import numpy as np
import pytest

import bnr_amd
import gig_ref as gr
import sweep_ref as sr
from gig_ref import VE
from oracle import bnr_oracle as bo

mpmath.mp.dps = 50
LD = sr.LD
SKIP_FRACTION = 0.05
D30 = 2.0 ** -30
CONCAVE = [1e-8, 1e-6, 1e-3, 0.05, 0.2 * (1 - D30)]
NOSHIFT = [0.2 * (1 + D30), 0.5, 1.0, 2.9, 3.0 * (1 - D30)]
SHIFT = [3.0 * (1 + D30), 5.0, 30.0, 1000.0, 3e3]
SEED, IT = 90210, 2


def _mpf(x):
    """a long double as an mpf, exactly"""
    x = LD(x)
    hi = float(x)
    return mpmath.mpf(hi) + mpmath.mpf(float(x - LD(hi)))


def g(x, w):
    """the density of GIG(1/2, omega, omega), unnormalised: S = sqrt(chi / psi) X"""
    return x ** mpmath.mpf(-0.5) * mpmath.exp(-w / 2 * (x + 1 / x))


def mode(w):
    """the root of (log g)' = -1 / (2 x) - omega / 2 (1 - 1 / x^2): omega x^2 + x - omega = 0"""
    return (mpmath.sqrt(1 + 4 * w * w) - 1) / (2 * w)


def rou_extrema(w, shifted):
    """(ulo, uhi, xoff) of the smallest rectangle around {(u, v): 0 < v <= sqrt(g(u / v + xoff) / g(xm))}: the extrema of
    (x - xoff) sqrt(g(x) / g(xm)), at the roots of 1 + (x - xoff) (log g)'(x) / 2"""
    xm = mode(w)
    mu = xm if shifted else mpmath.mpf(0)
    f = lambda x: 1 + (x - mu) / 2 * (-1 / (2 * x) - w / 2 * (1 - 1 / (x * x)))
    b = lambda x: (x - mu) * mpmath.sqrt(g(x, w) / g(xm, w))
    # 4 x^2 f(x) is the cubic -w x^3 + (3 + mu w) x^2 + (w + mu) x - mu w: its positive roots start the search, findroot on f ends it
    start = sorted(r.real for r in mpmath.polyroots([-w, 3 + mu * w, w + mu, -mu * w], maxsteps=200, extraprec=200) if abs(r.imag) < 1e-30 and r.real > 0)
    roots = [mpmath.findroot(f, r, tol=1e-45) for r in start]
    assert len(roots) == (2 if shifted else 1) and roots[-1] > xm and (not shifted or 0 < roots[0] < xm)
    return (b(roots[0]) if shifted else mpmath.mpf(0)), b(roots[-1]), mu


def hat(x, w):
    """the three-piece hat of gig_concave at lambda = 1/2, from the density alone: its maximum up to x0 = 2 omega, x^-1/2 exp(-omega) (the
    exponent is at most -omega) up to 2 / omega, (2 / omega)^-1/2 exp(-omega x / 2) (x^-1/2 decreases) beyond"""
    if x <= 2 * w:
        return g(mode(w), w)
    if x <= 2 / w:
        return mpmath.exp(-w) / mpmath.sqrt(x)
    return mpmath.sqrt(w / 2) * mpmath.exp(-w * x / 2)


def hat_cdf(x, w):
    pts = [0] + [p for p in (2 * w, 2 / w) if p < x] + [x]
    return mpmath.quad(lambda z: hat(z, w), pts)


def _within(x, i, want):
    """entry i of the reference quantity x is `want` to 1/100 of the bound it carries for the device (its own rounding is 1/2048 of that)"""
    return abs(_mpf(x.v[i]) - want) <= mpmath.mpf(float(x.e[i])) / 100


def _om(ws):
    return VE(np.array(ws, dtype=LD))


# ------------------------------------------------------------------------------------------------------------------ the formulas sample GIG
@pytest.mark.parametrize("ws,shifted", [(NOSHIFT, False), (SHIFT, True)])
def test_ratio_of_uniforms_rectangle_is_the_smallest_around_the_region(ws, shifted):
    c = gr.rou_setup(_om(ws), np.full(len(ws), shifted))
    for i, w in enumerate(ws):
        w = mpmath.mpf(w)
        xm, gm = mode(w), g(mode(w), w)
        ulo, uhi, xoff = (_mpf(c[k].v[i]) for k in ("ulo", "uhi", "xoff"))
        assert _within(c["xm"], i, xm) and xoff == (_mpf(c["xm"].v[i]) if shifted else 0)
        assert _within(c["nc"], i, mpmath.log(gm) / 2) and c["t"].v[i] == -0.25 and _within(c["s"], i, w / 4)
        lo, hi, _ = rou_extrema(w, shifted)
        assert _within(c["uhi"], i, hi) and (_within(c["ulo"], i, lo) if shifted else ulo == 0), (w, uhi, hi, ulo, lo)
        tol = mpmath.mpf(float(c["uhi"].e[i] + c["ulo"].e[i])) / 100
        for x in (xm * mpmath.mpf(10) ** (mpmath.mpf(k) / 100) for k in range(-600, 601)):
            v = mpmath.sqrt(g(x, w) / gm)
            assert 0 <= v <= 1 and ulo - tol <= (x - xoff) * v <= uhi + tol, (w, x)


def test_concave_hat_dominates_and_its_areas_are_its_integrals():
    c = gr.concave_setup(_om(CONCAVE))
    for i, w in enumerate(CONCAVE):
        w = mpmath.mpf(w)
        x0, tw = 2 * w, 2 / w
        assert _within(c["xm"], i, mode(w)) and _mpf(c["x0"].v[i]) == x0 and _within(c["tw"], i, tw) and _within(c["x0l"], i, mpmath.sqrt(x0))
        assert _within(c["k0"], i, hat(x0 / 2, w)) and _within(c["k1"], i, hat(tw / 2, w) * mpmath.sqrt(tw / 2))
        assert _within(c["k2"], i, hat(2 * tw, w) * mpmath.exp(w * tw))
        for x in (mpmath.mpf(10) ** (mpmath.mpf(k) / 50) for k in range(-1000, 1001)):
            assert hat(x, w) >= g(x, w) * (1 - mpmath.mpf(10) ** -40), (w, x)
        assert _within(c["A0"], i, mpmath.quad(lambda z: hat(z, w), [0, x0]))
        assert _within(c["A1"], i, mpmath.quad(lambda z: hat(z, w), [x0, tw]))
        assert _within(c["A2"], i, mpmath.quad(lambda z: hat(z, w), [tw, 4 * tw, 40 * tw, mpmath.inf]))
        assert _within(c["Atot"], i, hat_cdf(40 * tw, w) + mpmath.quad(lambda z: hat(z, w), [40 * tw, mpmath.inf]))


def test_concave_inversion_inverts_the_cdf_of_the_hat_and_accepts_under_the_density():
    ru = np.array([1e-9, 1e-3, 0.05, 0.2, 0.35, 0.5, 0.65, 0.8, 0.93, 0.99, 1 - 1e-6])
    rv = np.linspace(0.03, 0.97, ru.size)
    seen = set()
    for w in CONCAVE:
        c = gr.concave_setup(_om([w] * ru.size))
        X, acc, sure, margin, region = gr.concave_try(c, ru, rv)
        seen |= set(region.tolist())
        w = mpmath.mpf(w)
        Atot = _mpf(c["Atot"].v[0])
        for j in range(ru.size):
            x = _mpf(X.v[j])
            slack = (hat(x, w) * mpmath.mpf(float(X.e[j])) + mpmath.mpf(float(c["Atot"].e[j]))) / 100        # dH = hat(X) dX
            assert abs(hat_cdf(x, w) - Atot * mpmath.mpf(ru[j])) <= slack, (w, ru[j], region[j])
            m = mpmath.log(g(x, w) / hat(x, w)) - mpmath.log(mpmath.mpf(rv[j]))          # U = rv hat(X) <= g(X)
            assert abs(_mpf(margin.v[j]) - m) <= margin.e[j] / 100, (w, j)
            assert (not sure[j]) or bool(acc[j]) == (m >= 0)
    assert seen == {0, 1, 2}


@pytest.mark.parametrize("ws,shifted", [(NOSHIFT, False), (SHIFT, True)])
def test_ratio_of_uniforms_accepts_inside_the_region(ws, shifted):
    ru = np.array([1e-6, 0.1, 0.3, 0.5, 0.7, 0.9, 1 - 1e-6])
    rv = np.array([0.9, 0.05, 0.5, 0.97, 0.3, 0.7, 0.2])
    accepted = 0
    for w in ws:
        c = gr.rou_setup(_om([w] * ru.size), np.full(ru.size, shifted))
        X, acc, sure, margin = gr.rou_try(c, ru, rv)
        w = mpmath.mpf(w)
        lo, hi, xoff = rou_extrema(w, shifted)
        gm = g(mode(w), w)
        for j in range(ru.size):
            x = (lo + mpmath.mpf(ru[j]) * (hi - lo)) / mpmath.mpf(rv[j]) + xoff
            assert abs(_mpf(X.v[j]) - x) <= X.e[j] / 100
            if x > 0:
                m = mpmath.log(g(x, w) / gm) / 2 - mpmath.log(mpmath.mpf(rv[j]))           # V <= sqrt(g(X) / g(xm))
                assert abs(_mpf(margin.v[j]) - m) <= margin.e[j] / 100, (w, j)
                assert (not sure[j]) or bool(acc[j]) == (m >= 0)
            else:
                assert not acc[j]
        accepted += int(acc.sum())
    assert accepted >= len(ws)


def _value_50_digits(chi, psi, ru, rv):
    """the draw from the uniforms of its accepted attempt, from the density's own extrema and integrals (no formula of gig.jl)"""
    chi, psi, ru, rv = (mpmath.mpf(float(v)) for v in (chi, psi, ru, rv))
    w = mpmath.sqrt(chi * psi)
    if w > mpmath.mpf(0.2):
        lo, hi, xoff = rou_extrema(w, w > 3)
        x = (lo + ru * (hi - lo)) / rv + xoff
    else:
        A = [hat_cdf(2 * w, w), hat_cdf(2 / w, w), mpmath.quad(lambda z: hat(z, w), [2 / w, 8 / w, 80 / w, mpmath.inf])]
        A[1] -= A[0]
        v = ru * sum(A)
        if v <= A[0]:
            x = 2 * w * v / A[0]
        elif v <= A[0] + A[1]:
            x = (mpmath.sqrt(2 * w) + (v - A[0]) / (2 * mpmath.exp(-w))) ** 2
        else:
            x = -2 / w * mpmath.log(mpmath.exp(-1) - (v - A[0] - A[1]) * w / (2 * mpmath.sqrt(w / 2)))     # k2 (2 / w) (e^-1 - e^(-w x / 2)) = v - A0 - A1
    return mpmath.sqrt(chi / psi) * x


def test_value_agrees_with_a_50_digit_evaluation_within_a_hundredth_of_its_bound():
    var = sr.Variates(bnr_amd.lib(), SEED)
    ws = np.array(CONCAVE + NOSHIFT + SHIFT)
    psi = 0.01                                              # (omega = 1e-8 at chi = 1e-14: above 10 eps)
    chi = np.repeat(ws * ws / psi, 3)
    edges = np.arange(chi.size)
    S, bound, robust, att, kind = gr.gig_half_ref(chi, np.zeros(chi.size), psi, var, IT, edges)
    assert robust.all() and set(kind.tolist()) == {2, 3, 5}
    for e in edges:
        ru, rv = var.uniform2(IT, gr.SITE_D_GIG, int(e), int(att[e]))
        want = _value_50_digits(chi[e], psi, ru, rv)
        assert abs(_mpf(S[e]) - want) <= bound[e] / 100, (e, chi[e], kind[e], float(S[e]), want)
    # the draws without a loop: Gamma(1/2) psi / 2 (chi ~ 0; the SCALE quirk of gig.jl:17) and 1 / (Gamma(1/2) chi / 2) (psi ~ 0)
    G = var.gamma(0.5, IT, gr.SITE_D_GAMMA, 0)
    S, bound, robust, att, kind = gr.gig_half_ref([0.0], [0.0], 0.37, var, IT, [0])
    assert kind[0] == 0 and att[0] == -1 and abs(_mpf(S[0]) - mpmath.mpf(G) * mpmath.mpf(0.37) / 2) <= bound[0] / 100
    S, bound, robust, att, kind = gr.gig_half_ref([1.7], [0.0], 1e-300, var, IT, [0])
    assert kind[0] == 1 and att[0] == -1 and abs(_mpf(S[0]) - 1 / (mpmath.mpf(G) * mpmath.mpf(1.7) / 2)) <= bound[0] / 100


def test_the_bound_of_x_plus_its_inverse_holds_and_is_first_order():
    """x + 1 / x carries (1 - 1 / x^2) dx: a float64 evaluation at x + dx lies inside the doubled bound, also at x = 1 +- 1e-4 where the
    shifted ratio of uniforms lives at large omega and two independent operands would charge 2 dx"""
    rng = np.random.default_rng(3)
    x = np.r_[1 + 10.0 ** rng.uniform(-6, -2, 400) * rng.choice([-1, 1], 400), 10.0 ** rng.uniform(-8, 8, 400)]
    dx = 1e-12 * x
    out = gr.vxinv(VE(x, dx))
    for sgn in (-1.0, 1.0):
        dev = (x + sgn * dx) + 1.0 / (x + sgn * dx)
        assert np.all(sr.absm(np.asarray(dev, dtype=LD) - out.v) <= sr.SAFETY * out.e)
    near = np.abs(x - 1) < 1e-3
    assert np.all(out.e[near] < 1e-2 * dx[near] + 4 * sr.U * 2)


# ------------------------------------------------------------------------------------------------------------------ the library's host copy
def _rows(t):
    return {k: t[k][0] for k in t}, {k: t[k][1] for k in t}


def _host_draws(t, V, seed, it, chi=None):
    """S and the accepted attempts of the library's host copy on the device's float64 chi of rows 0, 1 of t"""
    L = bnr_amd.lib()
    if chi is None:
        d = t["gamma"][1, :, 0] - gr.float64_W(t["u"][1], t["lam"][0, :, 0], V)
        chi = d * d / t["tau2"][1, 0, 0]
    psi = float(t["theta"][0, 0, 0])
    S = np.array([L.bnr_host_gig(seed, 0.5, float(c), psi, it, e) for e, c in enumerate(chi)])
    att = np.array([L.bnr_host_gig_attempts(seed, 0.5, float(c), psi, it, e) for e, c in enumerate(chi)])
    return S, att


def _crafted(V, R, theta, psi=None):
    t = bnr_amd.new_table(2, V, R, dead=False)
    info = gr.craft_D(t, V, R, 5 + V, theta)
    if psi is not None:
        t["theta"][0] = psi
    return t, info


def _assert_inside(S, ref, what, att=None):
    worst, skipped, bad = gr.check_S(S, ref)
    print(what, {k: "%.3g" % v for k, v in worst.items()}, "skipped %d of %d" % (skipped, S.size))
    assert bad == 0 and all(v <= 1.0 for v in worst.values()), (what, worst, bad)
    assert skipped <= SKIP_FRACTION * S.size, (what, skipped)
    if att is not None:
        assert np.array_equal(att[ref["robust"]], ref["attempt"][ref["robust"]]), what
    return worst


@pytest.mark.parametrize("V,R,theta,psi", [(2, 1, 0.01, None), (11, 2, 2.3, None), (23, 11, 0.01, None), (200, 2, 0.01, None),
                                           (23, 11, 0.01, 1e-300), (11, 2, 2.3, 1e-300)])
def test_the_host_copy_lies_inside_every_bound_on_the_crafted_grid(V, R, theta, psi):
    t, info = _crafted(V, R, theta, psi)
    ref = gr.S_ref(*_rows(t), V, sr.Variates(bnr_amd.lib(), SEED), IT)
    S, att = _host_draws(t, V, SEED, IT)
    _assert_inside(S, ref, "host V=%d R=%d psi=%g" % (V, R, ref["psi"]), att)
    # the grid is what it says: every boundary edge decided, and on the side it was built for
    want = {"omega 0.2-": 3, "omega 0.2+": 2, "omega 3-": 2, "omega 3+": 5, "chi 10eps-": 0, "chi 10eps+": 3, "chi 0": 0}
    for nm, ii in info["groups"].items():
        assert ref["robust"][ii].all() and (ref["kind"][ii] == (want[nm] if psi is None or want[nm] == 0 else 1)).all(), nm
    if psi is None:
        with np.errstate(divide="ignore"):
            assert np.allclose(np.log(ref["omega"][info["omega"] > 0]), np.log(info["omega"][info["omega"] > 0]), rtol=0, atol=1e-6)


def test_the_host_copy_lies_inside_every_bound_over_omega_and_psi():
    """40 000 draws of bnr_host_gig from an exact chi: omega log-uniform over [1e-8, 3e3], psi over [1e-3, 1e3] (chi < 10 eps where psi is large and omega small:
    the Gamma draw)"""
    L = bnr_amd.lib()
    rng = np.random.default_rng(40000)
    var = sr.Variates(L, SEED)
    worst, skipped, seen = {}, 0, set()
    for b, psi in enumerate(10.0 ** np.linspace(-3, 3, 8)):
        m = 5000
        om = 10.0 ** rng.uniform(np.log10(gr.OMEGA_LO), np.log10(gr.OMEGA_HI), m)
        chi, edges = om * om / psi, np.arange(b * m, (b + 1) * m)
        S, bound, robust, att, kind = gr.gig_half_ref(chi, np.zeros(m), psi, var, IT, edges)
        got = np.array([L.bnr_host_gig(SEED, 0.5, float(c), float(psi), IT, int(e)) for c, e in zip(chi, edges)])
        gatt = np.array([L.bnr_host_gig_attempts(SEED, 0.5, float(c), float(psi), IT, int(e)) for c, e in zip(chi, edges)])
        ref = dict(S=S, bound=bound, robust=robust, attempt=att, kind=kind, omega=sr.f64(np.sqrt(LD(psi) * np.asarray(chi, dtype=LD))))
        w, sk, bad = gr.check_S(got, ref)
        assert bad == 0 and np.array_equal(gatt[robust], att[robust]), psi
        skipped += sk
        seen |= set(kind.tolist())
        for k, v in w.items():
            worst[k] = max(worst.get(k, 0.0), v)
    print("host, 40 000 draws:", {k: "%.3g" % v for k, v in worst.items()}, "skipped", skipped)
    assert all(v <= 1.0 for v in worst.values()) and seen == {0, 2, 3, 5}, (worst, seen)
    assert skipped <= SKIP_FRACTION * 40000


@pytest.mark.parametrize("n,V,R", [(40, 9, 3), (30, 12, 1), (25, 10, 7), (12, 17, 11)])
def test_the_oracles_float64_S_lies_inside_every_bound(n, V, R):
    tot, seed = 6, 4242
    X, y, _ = bnr_amd.make_synthetic(n, V, R, seed=11 + V)
    o = bo.Oracle(X, y, R, tot, seed, chain=1, pdf_mode=1, nu=max(10, R + 1))
    o.init_prior()
    o.run(2, tot, tot)
    var = sr.Variates(bnr_amd.lib(), seed + 1)
    S, refs = [], []
    for j in range(1, tot):
        refs.append(gr.S_ref({k: o.t[k][j - 1] for k in bo.COLUMNS}, {k: o.t[k][j] for k in bo.COLUMNS}, V, var, j + 1))
        S.append(o.t["S"][j].ravel())
    ref = {k: np.concatenate([np.atleast_1d(r[k]) for r in refs]) for k in ("S", "bound", "robust", "attempt", "kind", "omega")}
    _assert_inside(np.concatenate(S), ref, "oracle n=%d V=%d R=%d" % (n, V, R))


# ------------------------------------------------------------------------------------------------------------------ planted errors
@pytest.fixture(scope="module")
def case():
    V, R = 23, 11
    t, info = _crafted(V, R, 0.01)
    var = sr.Variates(bnr_amd.lib(), SEED)
    ref = gr.S_ref(*_rows(t), V, var, IT)
    S, att = _host_draws(t, V, SEED, IT)
    w, _, bad = gr.check_S(S, ref)
    assert bad == 0 and max(w.values()) <= 1
    return t, info, ref, S, V, R


def _rejected(S, ref, only=None):
    """the checker's verdict on the edges `only` (default: all): the largest ratio"""
    if only is not None:
        ref = {k: (v[only] if isinstance(v, np.ndarray) else v) for k, v in ref.items()}
        S = S[only]
    w, _, _ = gr.check_S(S, ref)
    return max(w.values(), default=0.0)


def _loops(ref):
    with np.errstate(invalid="ignore"):
        return np.flatnonzero(ref["robust"] & (ref["attempt"] >= 0) & (ref["bound"] < gr.NONVACUOUS * sr.f64(ref["S"])))


def test_checker_rejects_a_relative_error_of_1e_9(case):
    t, info, ref, S, V, R = case
    inr = np.flatnonzero(ref["robust"] & (ref["omega"] >= gr.OMEGA_LO) & (ref["omega"] <= gr.OMEGA_HI))
    for e in inr[:: max(1, inr.size // 40)]:
        P = S.copy()
        P[e] *= 1 + 1e-9
        assert _rejected(P, ref, np.array([e])) > 1, e


class _Shifted(sr.Variates):
    """attempt k of element e is the library's attempt k + first[e]"""

    def __init__(self, lib, seed, first):
        super().__init__(lib, seed)
        self.first = first

    def uniform2(self, it, site, elem, att=0):
        return super().uniform2(it, site, elem, att + int(self.first[elem]))


class _Swapped(sr.Variates):
    def uniform2(self, it, site, elem, att=0):
        a, b = super().uniform2(it, site, elem, att)
        return b, a


def test_checker_rejects_the_next_accepted_attempt(case):
    t, info, ref, S, V, R = case
    nxt = gr.S_ref(*_rows(t), V, _Shifted(bnr_amd.lib(), SEED, ref["attempt"] + 1), IT)
    ii = _loops(ref)
    ii = ii[nxt["robust"][ii]]
    assert ii.size > 100
    for e in ii:
        assert _rejected(sr.f64(nxt["S"]), ref, np.array([e])) > 1, e


def test_checker_rejects_ru_and_rv_swapped(case):
    t, info, ref, S, V, R = case
    sw = gr.S_ref(*_rows(t), V, _Swapped(bnr_amd.lib(), SEED), IT)
    ii = _loops(ref)
    ii = ii[sw["robust"][ii]]
    assert ii.size > 100
    for e in ii:
        assert _rejected(sr.f64(sw["S"]), ref, np.array([e])) > 1, e


def test_checker_rejects_chi_from_the_wrong_row_or_without_tau2(case):
    t, info, ref, S, V, R = case
    el, ek = sr.edge_nodes(V)
    gam, tau2 = t["gamma"][1, :, 0], t["tau2"][1, 0, 0]
    live = np.flatnonzero((np.abs(t["u"][1][:, el] * t["u"][1][:, ek]).sum(axis=0) > 0) & ref["robust"]
                          & (ref["omega"] >= gr.OMEGA_LO) & (ref["omega"] <= gr.OMEGA_HI))
    assert live.size > 100
    for what, u, lam, div in (("u of the row before", t["u"][0], t["lam"][0, :, 0], tau2), ("lambda of this row", t["u"][1], t["lam"][1, :, 0], tau2),
                              ("no division by tau2", t["u"][1], t["lam"][0, :, 0], 1.0)):
        d = gam - gr.float64_W(u, lam, V)
        P, _ = _host_draws(t, V, SEED, IT, chi=d * d / div)
        some = live[np.abs(d[live] ** 2 / div / sr.f64(ref["chi"][live]) - 1) > 1e-7]      # (where |W| is far below |gamma - W| another W is no other chi)
        print(what, some.size, "of", live.size)
        assert some.size >= 20, what
        for e in some:
            assert _rejected(P, ref, np.array([e])) > 1, (what, e)


def test_checker_rejects_the_degenerate_scale_2_over_psi(case):
    t, info, ref, S, V, R = case
    ii = np.flatnonzero(ref["kind"] == 0)
    assert ii.size >= 2 and ref["robust"][ii].all()
    G = np.array([bnr_amd.lib().bnr_host_gamma(SEED, 0.5, IT, gr.SITE_D_GAMMA, int(e)) for e in ii])
    P = S.copy()
    P[ii] = G * (2.0 / ref["psi"])
    assert np.allclose(S[ii], G * (ref["psi"] / 2.0), rtol=1e-14)
    for e in ii:
        assert _rejected(P, ref, np.array([e])) > 1, e


def test_checker_rejects_the_threshold_0_25_on_the_boundary_edges(case, monkeypatch):
    """edges with omega in (0.2, 0.25]: the ratio of uniforms draws them; a sampler that sends them to the concave envelope draws another value"""
    t, info, ref, S, V, R = case
    t = {k: v.copy() for k, v in t.items()}
    ii = np.r_[info["groups"]["omega 0.2+"], info["groups"]["omega 0.2-"]]
    s = np.sqrt(t["tau2"][1, 0, 0] / t["theta"][0, 0, 0])
    t["gamma"][1, ii, 0] = np.linspace(0.2 * (1 + D30), 0.25 * (1 - D30), ii.size) * s           # (edges between nodes with u = 0: gamma is g)
    good = gr.S_ref(*_rows(t), V, sr.Variates(bnr_amd.lib(), SEED), IT)
    S, _ = _host_draws(t, V, SEED, IT)
    assert (good["kind"][ii] == 2).all() and good["robust"][ii].all() and _rejected(S, good, ii) <= 1
    monkeypatch.setattr(gr, "OMEGA_CONCAVE", 0.25)
    moved = gr.S_ref(*_rows(t), V, sr.Variates(bnr_amd.lib(), SEED), IT)
    assert (moved["kind"][ii] == 3).all() and moved["robust"][ii].all()
    for e in ii:
        assert _rejected(sr.f64(moved["S"]), good, np.array([e])) > 1, e
