"""Extended-precision host reference, with an a-priori bound of the device's float64 error, of update_D! (gibbs.jl:454-458): the draw
S_e ~ GIG(1/2, chi_e = (gamma_e - W_e)^2 / tau2, psi = theta_prev) of k_backproj / k_backproj64 (numpy + Python stdlib only).

For lambda = 1/2 the draw (bnr_gig, bnr_rng.h; gig.jl:8-168) is a deterministic function of (chi, psi) and the uniform pairs (ru, rv) of the
counters {it, SITE_D_GIG, e, k}, k = 0, 1, ...: choose the kind, build the envelope, take the first accepted attempt, scale by sqrt(chi / psi).
That function is transcribed here once over `VE`, an array of np.longdouble values each carrying a running first-order bound of the error of
the device's float64 evaluation of the same quantity: every + - * / sqrt adds u |z|, every log exp cos acos LIBM_ULPS u |z|, and the errors of
the operands are propagated by the operation's exact partial derivatives -- x + 1 / x, which every log density here contains, is one
operation of one operand (vxinv).  The final bound is multiplied by SAFETY (the second-order terms).
The reference's own rounding is the same chain with u = 2^-64: 1/2048 of the device's.

Decisions.  The kind (chi < 10 eps, psi < 10 eps, omega > 3, omega > 0.2), the region of the concave hat (Vv <= A0, Vv <= A1) and accept /
reject of every attempt compare a quantity with a threshold: where the margin lies within SAFETY x its bound the decision is too close to
call, the edge is not checked further and it is counted (`robust` False).  Attempts give unrelated values, so |S_dev - S*| <= bound pins the
accepted attempt's index as well.

Not vacuous: for omega in [1e-8, 3e3] a checked edge's bound is below NONVACUOUS S*; an edge with a larger bound counts as skipped too.
Above 3e3 the device's error grows like omega u (the acos of the shifted ratio of uniforms nears 1): only the bound itself is asserted there.
Every edge, checked or skipped, must be finite and positive.
"""
import numpy as np

import sweep_ref as sr
from sweep_ref import LD, U, SAFETY, LIBM_ULPS, VARIATE_ULPS, f64

SITE_D_GIG, SITE_D_GAMMA = 21, 22
EPS10 = 2.220446049250313e-16 * 10.0            # bnr_gig_setup's 10 eps, the same double
OMEGA_CONCAVE, OMEGA_SHIFT = 0.2, 3.0            # concave up to 0.2, ratio of uniforms above, shifted by the mode above 3 (the doubles of bnr_rng.h)
OMEGA_LO, OMEGA_HI = 1e-8, 3e3                   # where a bound must also be small
NONVACUOUS = 1e-10
MAX_ATTEMPTS = 400                               # of the reference's loop (the library's cap is 100 000; a draw that deep is not a test case)
KIND_NAMES = {0: "S Gamma", 1: "S inverse Gamma", 2: "S ratio of uniforms", 3: "S concave", 5: "S shifted ratio of uniforms"}
LD_PI = LD("3.14159265358979323846264338327950288")


# ------------------------------------------------------------------------------------------------------------------ value with error
def _r(z):
    return U * np.abs(f64(z))


class VE:
    """v: np.longdouble array, the exact algorithm's value; e: float64 array, first-order bound of |device float64 value - v|"""
    __slots__ = ("v", "e")

    def __init__(self, v, e=0.0):
        self.v = np.asarray(v, dtype=LD)
        self.e = np.zeros(self.v.shape) + np.asarray(e, dtype=np.float64)

    def __getitem__(self, i):
        return VE(self.v[i], self.e[i])

    def __len__(self):
        return len(self.v)

    def __neg__(self):
        return VE(-self.v, self.e)

    def __add__(self, o):
        o = ve(o)
        z = self.v + o.v
        return VE(z, self.e + o.e + _r(z))

    def __sub__(self, o):
        o = ve(o)
        z = self.v - o.v
        return VE(z, self.e + o.e + _r(z))

    def __mul__(self, o):
        o = ve(o)
        z = self.v * o.v
        return VE(z, np.abs(f64(self.v)) * o.e + np.abs(f64(o.v)) * self.e + _r(z))

    def __truediv__(self, o):
        o = ve(o)
        z = self.v / o.v
        ab = np.abs(f64(o.v))
        return VE(z, self.e / ab + np.abs(f64(z)) * o.e / ab + _r(z))

    __radd__ = __add__
    __rmul__ = __mul__

    def __rsub__(self, o):
        return ve(o) - self

    def __rtruediv__(self, o):
        return ve(o) / self


def ve(x):
    return x if isinstance(x, VE) else VE(x)


def vsqrt(a):
    z = np.sqrt(a.v)
    return VE(z, a.e / (2 * f64(z)) + _r(z))


def vlog(a):
    z = np.log(a.v)
    return VE(z, a.e / np.abs(f64(a.v)) + LIBM_ULPS * _r(z))


def vexp(a):
    z = np.exp(a.v)
    return VE(z, a.e * f64(z) + LIBM_ULPS * _r(z))


def vcos(a):
    z = np.cos(a.v)
    return VE(z, np.abs(f64(np.sin(a.v))) * a.e + LIBM_ULPS * _r(z))


def vacos(a):
    """d acos = -da / sqrt(1 - a^2); first order only while the operand's error is small against its distance to +-1 (else: no bound)"""
    z = np.arccos(a.v)
    room = f64(1 - np.abs(a.v))
    d = a.e / f64(np.sqrt((1 - a.v) * (1 + a.v)))
    return VE(z, np.where(a.e <= room / 4, d, np.inf) + LIBM_ULPS * _r(z))


def vxinv(a):
    """x + 1 / x, both occurrences of x carrying the same error: d = (1 - 1 / x^2) dx (as two independent operands it would be twice
    dx -- near x = 1, where the shifted ratio of uniforms lives at large omega, 1e4 times the truth); roundings: the quotient, the sum"""
    inv = 1 / a.v
    z = a.v + inv
    return VE(z, np.abs(f64(1 - inv * inv)) * a.e + _r(inv) + _r(z))


def _put(dst, mask, src):
    dst.v[mask] = src.v
    dst.e[mask] = src.e


def _sure(margin):
    """the sign of `margin` is decided: it is farther from zero than SAFETY x the bound of the device's own evaluation"""
    return np.abs(f64(margin.v)) > SAFETY * margin.e


# ------------------------------------------------------------------------------------------------------------------ the kind
def kind_ref(chi, e_chi, psi):
    """bnr_gig_kind for lambda = 1/2: (kind 0 chi ~ 0 | 1 psi ~ 0 | 2 ratio of uniforms | 3 concave | 4 none, shifted (omega > 3),
    robust: every test the device makes on the way is decided, omega as VE)"""
    C = VE(chi, e_chi)
    psi = float(psi)
    small = C.v < LD(EPS10)
    robust = _sure(VE(C.v - LD(EPS10), C.e))
    with np.errstate(invalid="ignore"):
        om = vsqrt(VE(LD(psi)) * C)
    if psi < EPS10:
        return np.where(small, 0, 1), np.zeros(small.shape, dtype=bool), robust, om
    for thr in (OMEGA_CONCAVE, OMEGA_SHIFT):
        robust = robust & (small | _sure(VE(om.v - LD(thr), om.e)))
    kind = np.where(small, 0, np.where(om.v > LD(OMEGA_CONCAVE), 2, np.where(om.v > 0, 3, 4)))
    return kind, (kind == 2) & (om.v > LD(OMEGA_SHIFT)), robust, om


# ------------------------------------------------------------------------------------------------------------------ the two samplers
def _mode(om):
    """bnr_gig_mode, lambda = 1/2 (gig.jl:170-176): omega / (sqrt((1 - lambda)^2 + omega^2) + (1 - lambda))"""
    return om / (vsqrt(0.25 + om * om) + 0.5)


def rou_setup(om, shift):
    """gig_ROU_shift (gig.jl:44-78) / gig_ROU_noshift (80-100) as bnr_gig_setup's kind 2: t, s, xm, nc, ulo, uhi, xoff"""
    m = len(om)
    t, s = VE(np.full(m, LD(-0.25))), 0.25 * om
    xm = _mode(om)
    nc = t * vlog(xm) - s * vxinv(xm)
    ulo, uhi, xoff = VE(np.zeros(m)), VE(np.zeros(m)), VE(np.zeros(m))
    if np.any(shift):
        o, x, sh, tt, n0 = om[shift], xm[shift], s[shift], t[shift], nc[shift]
        a = -(3.0 / o + x)                                           # 2 (lambda + 1) = 3
        b = (-1.0 * x) / o - 1.0                                     # 2 (lambda - 1) = -1
        p = b - a * a / 3.0
        q = 2.0 * a * a * a / 27.0 - a * b / 3.0 + x
        fi = vacos(-q / (2.0 * vsqrt(-p * p * p / 27.0)))
        fak = 2.0 * vsqrt(-p / 3.0)
        y1 = fak * vcos(fi / 3.0) - a / 3.0
        y2 = fak * vcos(fi / 3.0 + VE(4.0) / 3.0 * VE(LD_PI, U * float(LD_PI))) - a / 3.0
        _put(uhi, shift, (y1 - x) * vexp(tt * vlog(y1) - sh * vxinv(y1) - n0))
        _put(ulo, shift, (y2 - x) * vexp(tt * vlog(y2) - sh * vxinv(y2) - n0))
        _put(xoff, shift, x)
    ns = ~shift
    if np.any(ns):
        o, sh, n0 = om[ns], s[ns], nc[ns]
        ym = (1.5 + vsqrt(2.25 + o * o)) / o
        _put(uhi, ns, vexp(0.75 * vlog(ym) - sh * vxinv(ym) - n0))
    return dict(t=t, s=s, xm=xm, nc=nc, ulo=ulo, uhi=uhi, xoff=xoff, shift=shift)


def rou_try(c, ru, rv):
    """one attempt of kind 2 (bnr_gig_try): (X, accepted, decided, margin of the acceptance test)"""
    ru, rv = VE(ru), VE(rv)
    Uu = c["ulo"] + ru * (c["uhi"] - c["ulo"])
    X = Uu / rv + c["xoff"]
    pos = X.v > 0
    Xs = VE(np.where(pos, X.v, LD(1)), X.e)
    margin = c["t"] * vlog(Xs) - c["s"] * vxinv(Xs) - c["nc"] - vlog(rv)
    sure = _sure(X) & (~pos | _sure(margin))
    return X, pos & (margin.v >= 0), sure, margin


def concave_setup(om):
    """gig_concave (gig.jl:102-168) as bnr_gig_setup's kind 3 at lambda = 1/2, omega <= 0.2 (x0 = 2 omega < 2 / omega: three pieces)"""
    assert np.all(om.v < 1)
    xm = _mode(om)
    x0 = om / 0.5
    k0 = vexp(-0.5 * vlog(xm) - 0.5 * om * vxinv(xm))
    A0 = k0 * x0
    x0l = vsqrt(x0)
    k1 = vexp(-om)
    tw = 2.0 / om
    twl = vsqrt(tw)
    A1 = k1 / 0.5 * (twl - x0l)
    k2 = 1.0 / twl
    A2 = k2 * 2.0 * vexp(VE(np.full(len(om), LD(-1)))) / om
    return dict(om=om, xm=xm, x0=x0, k0=k0, A0=A0, A1=A1, A2=A2, k1=k1, k2=k2, Atot=A0 + A1 + A2, x0l=x0l, tw=tw)


def concave_try(c, ru, rv):
    """one attempt of kind 3 (bnr_gig_try): (X, accepted, decided, margin, region 0 / 1 / 2)"""
    ru, rv = VE(ru), VE(rv)
    m = len(ru)
    om = c["om"]
    Vv = c["Atot"] * ru
    d0 = c["A0"] - Vv
    V1 = Vv - c["A0"]
    d1 = c["A1"] - V1
    V2 = V1 - c["A1"]
    region = np.where(d0.v >= 0, 0, np.where(d1.v >= 0, 1, 2))
    sure = _sure(d0) & ((region == 0) | _sure(d1))
    X, hx = VE(np.ones(m)), VE(np.ones(m))
    r0, r1, r2 = region == 0, region == 1, region == 2
    if np.any(r0):
        _put(X, r0, c["x0"][r0] * Vv[r0] / c["A0"][r0])
        _put(hx, r0, c["k0"][r0])
    if np.any(r1):
        r = c["x0l"][r1] + (0.5 / c["k1"][r1] * V1[r1])
        _put(X, r1, r * r)
        _put(hx, r1, c["k1"][r1] / r)
    if np.any(r2):
        o = om[r2]
        with np.errstate(invalid="ignore", divide="ignore"):
            x2 = -2.0 / o * vlog(vexp(-o / 2.0 * c["tw"][r2]) - o / (2.0 * c["k2"][r2]) * V2[r2])
            _put(X, r2, x2)
            _put(hx, r2, c["k2"][r2] * vexp(-o / 2.0 * x2))
    with np.errstate(invalid="ignore", divide="ignore"):
        margin = -0.5 * vlog(X) - om / 2.0 * vxinv(X) - vlog(rv * hx)
    ok = np.isfinite(f64(margin.v)) & np.isfinite(margin.e)
    sure = sure & ok & _sure(margin)
    return X, ok & (margin.v >= 0), sure, margin, region


def _first_accepted(ctx, try_fn, edges, var, it):
    """the loop of bnr_gig over the attempts k = 0, 1, ...: (X as VE, attempt, decided all the way)"""
    m = len(edges)
    Xv, Xe = np.ones(m, dtype=LD), np.full(m, np.inf)
    att, rob = np.full(m, -1), np.ones(m, dtype=bool)
    open_ = np.arange(m)
    for k in range(MAX_ATTEMPTS):
        if open_.size == 0:
            break
        uv = np.array([var.uniform2(it, SITE_D_GIG, int(e), k) for e in edges[open_]])
        X, acc, sure = try_fn({n: v[open_] for n, v in ctx.items()}, uv[:, 0], uv[:, 1])[:3]
        rob[open_[~sure]] = False
        j = sure & acc
        Xv[open_[j]], Xe[open_[j]], att[open_[j]] = X.v[j], X.e[j], k
        open_ = open_[sure & ~acc]
    assert open_.size == 0, "a draw of the reference is still open after %d attempts" % MAX_ATTEMPTS
    return VE(Xv, Xe), att, rob


def gig_half_ref(chi, e_chi, psi, var, it, edges):
    """S ~ GIG(1/2, chi, psi) of the elements `edges` at iteration id `it`: chi long double with the bound e_chi of the device's own chi,
    psi exact.  Returns (S* long double, bound, robust, accepted attempt (-1: no loop), kind (2 -> 5 where shifted))"""
    chi = np.asarray(chi, dtype=LD).ravel()
    edges = np.asarray(edges).ravel()
    q = chi.size
    kind, shift, robust, om = kind_ref(chi, e_chi, psi)
    robust = robust.copy()
    C, P = VE(chi, e_chi), VE(LD(float(psi)))
    S, bound, att = np.full(q, LD("nan")), np.full(q, np.inf), np.full(q, -1)
    for kd in (0, 1):
        i = np.flatnonzero(robust & (kind == kd))
        if i.size:
            g = np.array([var.gamma(0.5, it, SITE_D_GAMMA, int(e)) for e in edges[i]])
            G = VE(g, VARIATE_ULPS * U * g)
            out = G * (P / 2.0) if kd == 0 else 1.0 / (G * (C[i] / 2.0))        # Gamma SCALE psi / 2: the quirk of gig.jl:17, kept
            S[i], bound[i] = out.v, SAFETY * out.e
    for kd in (2, 3):
        i = np.flatnonzero(robust & (kind == kd))
        if i.size == 0:
            continue
        ctx = rou_setup(om[i], shift[i]) if kd == 2 else concave_setup(om[i])
        X, a, rob = _first_accepted(ctx, rou_try if kd == 2 else concave_try, edges[i], var, it)
        out = vsqrt(C[i] / P) * X
        S[i], bound[i], att[i] = out.v, SAFETY * out.e, a
        robust[i] = rob
    bound = np.where(robust, bound, np.inf)
    return S, bound, robust, att, np.where(shift, 5, kind)


# ------------------------------------------------------------------------------------------------------------------ from table rows
def chi_ref(prev_row, row, V):
    """chi_e = (gamma_e - W_e)^2 / tau2 as VE: W* = sum_r lambda_r u_rl u_rk in long double (this row's u, the row before's lambda), the
    device's Wbuf charged with gamma_(3R+2) sum |lambda| |u| |u| (the allowance of tests/test_gamma_linalg_gpu.py); gamma and tau2 are the
    table's own values.  Edges in the order of bnr_edge_index."""
    W = VE(*sr.compute_W(row["u"], prev_row["lam"], *sr.edge_nodes(V), m=3 * f64(row["u"]).shape[0] + 2))
    g = VE(f64(row["gamma"]).ravel()) - W
    return g * g / VE(LD(float(f64(row["tau2"]).ravel()[0])))


def S_ref(prev_row, row, V, var, it):
    """update_D! of `row` from its own gamma, u, tau2 and the row before's lambda and theta: a dict with S, bound, robust, attempt, kind,
    omega, chi and psi"""
    chi = chi_ref(prev_row, row, V)
    psi = float(f64(prev_row["theta"]).ravel()[0])
    S, bound, robust, att, kind = gig_half_ref(chi.v, chi.e, psi, var, it, np.arange(chi.v.size))
    with np.errstate(invalid="ignore"):
        om = f64(np.sqrt(LD(psi) * chi.v))
    return dict(S=S, bound=bound, robust=robust, attempt=att, kind=kind, omega=om, chi=chi.v, e_chi=chi.e, psi=psi)


def check_S(S_dev, ref):
    """(largest |S_dev - S*| / bound per kind over the checked edges, number of skipped edges -- a decision too close to call, or a bound
    that would not be a check: at least NONVACUOUS S* with omega in [OMEGA_LO, OMEGA_HI] --, number of edges, checked or skipped, whose
    value is not finite and positive)"""
    got = f64(S_dev).ravel()
    om, bound, S = ref["omega"], ref["bound"], ref["S"]
    with np.errstate(invalid="ignore"):
        vacuous = (om >= OMEGA_LO) & (om <= OMEGA_HI) & ~(bound < NONVACUOUS * f64(S))
        checked = ref["robust"] & ~vacuous & np.isfinite(bound)
        err = sr.absm(np.asarray(got, dtype=LD) - S)
    worst = {}
    for kd, name in KIND_NAMES.items():
        i = checked & (ref["kind"] == kd)
        if np.any(i):
            worst[name] = sr.ratio(np.where(np.isfinite(err[i]), err[i], np.inf), bound[i])
    bad = int(np.sum(~(np.isfinite(got) & (got > 0))))
    return worst, int(np.sum(~checked)), bad


# ------------------------------------------------------------------------------------------------------------------ the crafted grid
def float64_W(u, lam, V):
    """W in float64, term by term in edge_W's order"""
    el, ek = sr.edge_nodes(V)
    W = np.zeros(el.size)
    for r in range(u.shape[0]):
        W = W + u[r, el] * lam[r] * u[r, ek]
    return W


def boundary_count(q):
    """edges per boundary group: at most 1 % of the edges"""
    return min(q // 100, 6)


def craft_D(t, V, R, seed, theta, tau2=0.37):
    """Rows 0 and 1 (0-based) of table t for update_D! of row 1: gamma = W_float64 + g with g per edge such that omega = |g| sqrt(theta / tau2)
    is log-uniform (stratified) over [1e-8, 3e3], a tenth of the edges over (3e3, 1e8], and -- on edges between nodes with u = 0, where
    W = 0 and gamma = g without rounding -- the boundary groups omega = 0.2 (1 +- 2^-30), 3 (1 +- 2^-30), chi = 10 eps (1 +- 2^-20) and
    chi = 0.  Node scales over five decades with the larger omega on the larger edges: |W| up to 10 |g|, so gamma - W cancels.  Rows 0 and 1
    differ in u, lambda, tau2 and theta: a chi from the wrong row is another chi.  Returns {"omega": targets, "groups": {name: edges}}."""
    rng = np.random.default_rng(seed)
    el, ek = sr.edge_nodes(V)
    q = el.size
    nb = boundary_count(q)
    nz = 0
    while nz * (nz + 1) // 2 < 7 * nb:
        nz += 1
    scale = 10.0 ** rng.uniform(-2.5, 2.5, V)
    u = rng.standard_normal((R, V)) * scale[None, :]
    u[:, V - nz:] = 0.0
    lam = rng.choice([1.0, -1.0, 0.0], R, p=[0.4, 0.4, 0.2])
    if not np.any(lam):
        lam[0] = 1.0
    zero = np.flatnonzero((el >= V - nz) & (ek >= V - nz))
    names = ["omega 0.2-", "omega 0.2+", "omega 3-", "omega 3+", "chi 10eps-", "chi 10eps+", "chi 0"]
    groups = {nm: zero[j * nb:(j + 1) * nb] for j, nm in enumerate(names)}
    special = zero[:7 * nb]
    rest = np.setdiff1d(np.arange(q), special)
    n_hi = rest.size // 10
    n_lo = rest.size - n_hi
    lo = np.log10(OMEGA_LO) + (np.arange(n_lo) + rng.random(n_lo)) / n_lo * (np.log10(OMEGA_HI) - np.log10(OMEGA_LO))
    hi = np.log10(OMEGA_HI) + (np.arange(n_hi) + rng.random(n_hi)) / max(n_hi, 1) * (8 - np.log10(OMEGA_HI))
    pool = np.sort(np.r_[lo, hi])
    aw = (np.abs(u[:, el]) * np.abs(lam)[:, None] * np.abs(u[:, ek])).sum(axis=0)
    dead, live = rest[aw[rest] == 0], rest[aw[rest] > 0]              # W = 0 (a node with u = 0): any omega; the others by size
    take = np.zeros(pool.size, dtype=bool)
    take[rng.choice(pool.size, dead.size, replace=False)] = True
    omega = np.zeros(q)
    omega[dead] = 10.0 ** pool[take]
    omega[live[np.argsort(aw[live] * (1 + 0.5 * rng.random(live.size)), kind="stable")]] = 10.0 ** pool[~take]
    s = np.sqrt(tau2 / theta)
    g = omega * s
    for nm, w, d in (("omega 0.2-", 0.2, -1), ("omega 0.2+", 0.2, 1), ("omega 3-", 3.0, -1), ("omega 3+", 3.0, 1)):
        omega[groups[nm]] = w * (1 + d * 2.0 ** -30)
        g[groups[nm]] = omega[groups[nm]] * s
    for nm, d in (("chi 10eps-", -1), ("chi 10eps+", 1)):
        chi = EPS10 * (1 + d * 2.0 ** -20)
        omega[groups[nm]] = np.sqrt(theta * chi)
        g[groups[nm]] = np.sqrt(chi * tau2)
    omega[groups["chi 0"]] = 0.0
    g[groups["chi 0"]] = 0.0
    g = g * rng.choice([1.0, -1.0], q)
    if live.size:
        u *= np.sqrt(10.0 * np.min(np.abs(g[live]) / aw[live]))       # sum |lambda u u| <= 10 |g| on every edge, equal on one
    t["u"][1], t["u"][0] = u, rng.standard_normal((R, V))
    t["lam"][0, :, 0] = lam
    t["lam"][1, :, 0] = np.where(lam == 1.0, -1.0, 1.0)
    t["tau2"][0], t["tau2"][1] = 5.0 * tau2, tau2
    t["theta"][0], t["theta"][1] = theta, 7.7 * theta
    t["gamma"][1, :, 0] = float64_W(u, lam, V) + g
    t["gamma"][0, :, 0] = rng.standard_normal(q)
    return dict(omega=omega, groups=groups)
