"""An independent reference of the draw-site variates and of the prior row (numpy + Python stdlib only; nothing here calls the library or the
oracle): Philox-4x32-10, the word-to-uniform map, the normal, the Gamma sampler and initialize_variables! (gibbs.jl:191-224), each with an
a-priori bound of the device's float64 error.  The references of tests/sweep_ref.py and tests/gig_ref.py take their variates from the
library's host copy; this module is what that copy, the oracle's and the device's own variates (k_init_prior writes them into the table raw)
are held against.

Philox-4x32-10 is written from Salmon, Moraes, Dror, Shaw, "Parallel random numbers: as easy as 1, 2, 3" (SC'11): one round maps the counter
(c0, c1, c2, c3) under the round key (k0, k1) to (hi(M1 c2) ^ c1 ^ k0, lo(M1 c2), hi(M0 c0) ^ c3 ^ k1, lo(M0 c0)), the key is bumped by the
Weyl constants (W0, W1) between rounds, ten rounds.  Vectorised over numpy uint64 arrays; a 32 x 32 bit product is exact in 64 bits.
One draw is the block of counter {iteration, site, element, attempt} under key {lo32(s), hi32(s)}, s = seed + chain id mod 2^64; its two
64-bit halves (word 0 | word 1 << 32, word 2 | word 3 << 32) give two uniforms.

The unit map, stated with integers: y = w >> 11; below 2^52 the uniform is (2 y + 1) / 2^54; from 2^52 upward y + 1/2 is a tie in float64 and
rounds to even, the uniform is (y + (y odd)) / 2^53; the one result 1 (y = 2^53 - 1) is replaced by 1 - 2^-53.  Every value is a float64.

The normal is sqrt(-2 ln ua) cos(2 pi ub) OF THE FLOAT64 UNIFORMS (they are the specification: 2 pi ub next to a zero of the cosine is as
accurate as ub, and the integers behind ub differ from it by up to 2^-54), in np.longdouble, cos(2 pi ub) through the exact reduction
4 ub - round(4 ub) -- exact in long double -- so that the reference keeps its relative accuracy at the zero crossings (ub = 1/4, 3/4: exactly 0,
as on the device).  The device's relative error, term by term (u = 2^-53, one unit per correctly rounded operation):
    log(ua)                                        LIBM_ULPS
    -2 log(ua)                                     exact
    sqrt                                           halves the incoming error, adds 1:      LIBM_ULPS / 2 + 1
    4 ub, the quadrant, 4 ub - quadrant            exact
    times the rounded pi / 2                       the constant 1, the product 1:          2
    sin / cos on [-pi/4, pi/4]                     condition at most 1, adds LIBM_ULPS:    2 + LIBM_ULPS
    the final product                              1
NORMAL_ULPS = (LIBM_ULPS / 2 + 1) + (2 + LIBM_ULPS) + 1 = 7 for LIBM_ULPS = 2, which the module asserts to lie within VARIATE_ULPS: the budget
of the stage references for a normal variate follows from LIBM_ULPS instead of being assumed.

The Gamma sampler (Marsaglia-Tsang with the boost u^(1/a) for a < 1) is transcribed once over gig_ref.VE: every operation carries its
first-order error, the final bound is multiplied by SAFETY; `robust` is False where v <= 0 or accept / reject lies within SAFETY x its bound.

The reference's own error: the same chains in long double, unit roundoff 2^-64 -- 1/2048 of the device's bounds.
"""
import functools

import numpy as np

import sweep_ref as sr
from gig_ref import VE, ve, vsqrt, vlog, _r, _put, _sure, LD_PI, NONVACUOUS
from sweep_ref import LD, U, SAFETY, LIBM_ULPS, VARIATE_ULPS, f64, gamma_m, absm

PHILOX_M0, PHILOX_M1 = 0xD2511F53, 0xCD9E8D57
PHILOX_W0, PHILOX_W1 = 0x9E3779B9, 0xBB67AE85          # golden ratio, sqrt(3) - 1
_M32, _S32, _S11, _ONE = np.uint64(0xFFFFFFFF), np.uint64(32), np.uint64(11), np.uint64(1)
ATT_BOOST = 0xFFFFFFFF
SITE_INIT_S, SITE_INIT_PI, SITE_INIT_LAM, SITE_INIT_XI, SITE_INIT_M_CHI, SITE_INIT_M_N, SITE_INIT_U, SITE_INIT_GAMMA = 1, 2, 3, 4, 5, 6, 7, 8
MAX_ATTEMPTS = 400
NORMAL_ULPS = (LIBM_ULPS / 2 + 1) + (2 + LIBM_ULPS) + 1
assert NORMAL_ULPS * U <= VARIATE_ULPS * U, "the stage references' budget for a normal variate no longer follows from LIBM_ULPS"
NORMAL_REL = gamma_m(NORMAL_ULPS)                      # (1 + d)^7 - 1, the products of the terms included


# ------------------------------------------------------------------------------------------------------------------ Philox-4x32-10
def philox4x32(ctr, key, rounds=10, swap_multipliers=False, bump_key=True):
    """the four output words (uint64 arrays holding 32-bit values) of counters ctr = (c0, c1, c2, c3) under keys key = (k0, k1); the optional
    arguments are mutations for the tests' power checks"""
    c0, c1, c2, c3, k0, k1 = np.broadcast_arrays(*[np.asarray(x, dtype=np.uint64) & _M32 for x in tuple(ctr) + tuple(key)])
    m0, m1 = np.uint64(PHILOX_M1 if swap_multipliers else PHILOX_M0), np.uint64(PHILOX_M0 if swap_multipliers else PHILOX_M1)
    for r in range(rounds):
        if r and bump_key:
            k0, k1 = (k0 + np.uint64(PHILOX_W0)) & _M32, (k1 + np.uint64(PHILOX_W1)) & _M32
        p0, p1 = m0 * c0, m1 * c2
        c0, c1, c2, c3 = (p1 >> _S32) ^ c1 ^ k0, p1 & _M32, (p0 >> _S32) ^ c3 ^ k1, p0 & _M32
    return c0, c1, c2, c3


def words(key, it, site, elem, att=0, **mutation):
    """the two 64-bit words of the draw {it, site, elem, att} under the 64-bit key (seed + chain id mod 2^64)"""
    key = np.asarray(key, dtype=np.uint64)
    r = philox4x32((it, site, elem, att), (key & _M32, key >> _S32), **mutation)
    return r[0] | (r[1] << _S32), r[2] | (r[3] << _S32)


def unit(w, clamp=True):
    """the uniform of a 64-bit word; clamp=False: the bare formula ((w >> 11) + 1/2) 2^-53 rounded to float64, which reaches 1"""
    y = np.asarray(w, dtype=np.uint64) >> _S11
    low = y < np.uint64(2 ** 52)
    num = np.where(low, (y << _ONE) + _ONE, y + (y & _ONE))                  # at most 2^53: a float64
    val = num.astype(np.float64) * np.where(low, 2.0 ** -54, 2.0 ** -53)     # a power of two: exact
    return np.where(val == 1.0, 1.0 - 2.0 ** -53, val) if clamp else val


def draw2(key, it, site, elem, att=0, **mutation):
    a, b = words(key, it, site, elem, att, **mutation)
    return unit(a), unit(b)


# ------------------------------------------------------------------------------------------------------------------ the normal
def cos2pi(ub, quadrant_sign=True):
    """cos(2 pi ub) in long double"""
    x = LD(4) * np.asarray(ub, dtype=LD)
    qd = np.floor(x + LD(0.5))
    t = (x - qd) * (LD_PI / 2)
    qi = qd.astype(np.int64) & 3
    c, s = np.cos(t), np.sin(t)
    if quadrant_sign:
        return np.where(qi == 0, c, np.where(qi == 1, -s, np.where(qi == 2, -c, s)))
    return np.where((qi == 0) | (qi == 2), c, s)


def normal_ref(ua, ub, quadrant_sign=True):
    """(z, bound): sqrt(-2 ln ua) cos(2 pi ub) of the float64 uniforms in long double, and the bound NORMAL_REL |z| of the device's error"""
    z = np.sqrt(-2 * np.log(np.asarray(ua, dtype=LD))) * cos2pi(ub, quadrant_sign)
    return z, NORMAL_REL * np.abs(f64(z))


def normal(key, it, site, elem, att=0, **mutation):
    qs = mutation.pop("quadrant_sign", True)
    return normal_ref(*draw2(key, it, site, elem, att, **mutation), quadrant_sign=qs)


# ------------------------------------------------------------------------------------------------------------------ the Gamma sampler
def vpow(x, y):
    """x^y of one libm call: d = z (y dx / x + log(x) dy)"""
    z = np.power(x.v, y.v)
    az = np.abs(f64(z))
    return VE(z, az * (np.abs(f64(y.v / x.v)) * x.e + np.abs(f64(np.log(x.v))) * y.e) + LIBM_ULPS * _r(z))


def gamma_ve(shape, key, it, site, elem, d_offset=None, boost_inverse=True, accept_reversed=False, candidates=None):
    """bnr_gamma over VE for the elements `elem` (an array) with the shapes `shape` (a VE, one per element or one for all): (draw as VE,
    accepted attempt, robust).  d_offset / boost_inverse / accept_reversed: mutations.  candidates: a list that receives (attempt, element
    positions, d v^3 boost of every position still open at that attempt, accepted or not)."""
    elem = np.atleast_1d(np.asarray(elem))
    m = elem.size
    a = ve(shape)
    a = VE(np.broadcast_to(a.v, (m,)).copy(), np.broadcast_to(a.e, (m,)).copy())
    robust = _sure(VE(a.v - 1, a.e)) | (a.e == 0)                          # the test a < 1
    small = a.v < 1
    boost = VE(np.ones(m))
    if np.any(small):
        ua, _ = draw2(key, it, site, elem[small], ATT_BOOST)
        _put(boost, small, vpow(VE(ua), 1.0 / a[small] if boost_inverse else a[small]))
        up = a + 1.0
        a = VE(np.where(small, up.v, a.v), np.where(small, up.e, a.e))
    d = a - (VE(1.0) / 3.0 if d_offset is None else VE(d_offset))
    c = 1.0 / vsqrt(9.0 * d)
    out, att = VE(np.ones(m), np.full(m, np.inf)), np.full(m, -1)
    open_ = np.flatnonzero(robust)
    for t in range(MAX_ATTEMPTS):
        if open_.size == 0:
            break
        e = elem[open_]
        x = VE(*normal(key, it, site, e, 2 * t))
        ua, _ = draw2(key, it, site, e, 2 * t + 1)
        dd = d[open_]
        v = 1.0 + c[open_] * x
        pos, sure = v.v > 0, _sure(v)                                       # the test v <= 0
        v = VE(np.where(pos, v.v, LD(1)), v.e)
        v3 = v * v * v
        margin = 0.5 * x * x + dd - dd * v3 + dd * vlog(v3) - vlog(VE(ua))
        sure = sure & (~pos | _sure(margin))
        acc = pos & ((margin.v < 0) if accept_reversed else (margin.v > 0))
        val = dd * v3 * boost[open_]
        if candidates is not None:
            candidates.append((t, open_.copy(), f64(val.v)))
        robust[open_[~sure]] = False
        j = sure & acc
        out.v[open_[j]], out.e[open_[j]], att[open_[j]] = val.v[j], val.e[j], t
        open_ = open_[sure & ~acc]
    robust[open_] = False                                                   # still open after MAX_ATTEMPTS: not a test case
    out.e[~robust] = np.inf
    return out, att, robust


def gamma_ref(shape, key, it, site, elem, **kw):
    """(value, bound, accepted attempt, robust) of the Gamma(shape, 1) draws of the elements `elem`; bound = SAFETY x the first-order bound"""
    g, att, robust = gamma_ve(shape, key, it, site, elem, **kw)
    return g.v, SAFETY * g.e, att, robust


def vacuous(value, bound):
    """a bound that would not be a check (gig_ref.NONVACUOUS of the value): such a draw counts as skipped"""
    return ~(bound < NONVACUOUS * np.abs(f64(value)))


# ------------------------------------------------------------------------------------------------------------------ the prior row
CASES = [(2, 1, 1, 0.5), (19, 5, 10, 1.01), (65, 7, 12, 1.01), (64, 32, 32, 2.0), (600, 32, 40, 1.01)]      # V, R, nu, eta
CHAIN_ID, LIKE_ID = 1, 4


def case_seed(i):
    """seed + CHAIN_ID has the low word 0xFFFFFFFF, seed + LIKE_ID carries into the high word, which is set from the second case on"""
    return (i + 1) * 2 ** 32 - 2


def _exact_or_rounded(v_ld):
    """a VE of a quantity the device forms by one float64 operation: no error where float64 holds it exactly"""
    v = np.asarray(v_ld, dtype=LD)
    return VE(v, np.where(np.asarray(f64(v), dtype=LD) == v, 0.0, _r(v)))


@functools.lru_cache(maxsize=16)
def init_ref(V, R, eta, nu, key):
    """initialize_variables! (gibbs.jl:191-224) as k_init_prior draws it: the counter sites SITE_INIT_*, iteration 1, element e for S and
    gamma, 3 r + c for pi, r for lambda, v for xi, j for the Bartlett diagonal, i R + j below it, v R + r for u.
    Returns a dict: row (columns in the table layout, long double), bound (elementwise, float64; 0 where equality is required), lam_robust (R),
    pi_robust (R), chi_robust (R), second_order_ok.  The result is shared between tests: do not modify it."""
    q, it = V * (V + 1) // 2, 1
    if eta <= 1.0:
        eta = 1.01                                                           # the local reset of gibbs.jl:193-196
    row = dict(theta=np.full((1, 1), LD(0.5)), Delta=np.full((1, 1), LD(0.5)), mu=np.full((1, 1), LD(1)), tau2=np.full((1, 1), LD(1)))
    bound = {k: np.zeros((1, 1)) for k in row}
    # S_e = -(theta / 2) / 2 ... = -ln(ua) / 4: the logarithm, one product
    ua, _ = draw2(key, it, SITE_INIT_S, np.arange(q))
    S = VE(-np.log(np.asarray(ua, dtype=LD)) / 4)
    S.e = (LIBM_ULPS + 1) * _r(S.v)
    row["S"], bound["S"] = S.v.reshape(q, 1), S.e.reshape(q, 1)
    # pi_r ~ Dirichlet(r^eta, 1, 1) from three Gamma draws; the device's pow may differ from the exact power by LIBM_ULPS (1^eta is 1 exactly)
    r = np.arange(R)
    base = np.power(np.asarray(r + 1, dtype=LD), LD(float(eta)))
    sh = VE(np.ones((R, 3), dtype=LD))
    sh.v[:, 0], sh.e[:, 0] = base, np.where(r == 0, 0.0, LIBM_ULPS * _r(base))
    g, _att, g_rob = gamma_ve(VE(sh.v.ravel(), sh.e.ravel()), key, it, SITE_INIT_PI, np.arange(3 * R))
    g_rob = g_rob & ~vacuous(g.v, SAFETY * g.e)
    G = VE(g.v.reshape(R, 3), np.where(g_rob, g.e, 0.0).reshape(R, 3))
    tot = (G[:, 0] + G[:, 1]) + G[:, 2]
    P = [G[:, c] / tot for c in range(3)]
    pi_robust = g_rob.reshape(R, 3).all(axis=1)
    row["pi"] = np.stack([p.v for p in P], axis=1)
    bound["pi"] = np.where(pi_robust[:, None], SAFETY * np.stack([p.e for p in P], axis=1), np.inf)
    # lambda_r: bnr_categorical3's scan of the cumulative weights (order 0, 1, -1) on the device's own pi
    ua, _ = draw2(key, it, SITE_INIT_LAM, r)
    t = VE(ua) * ((P[0] + P[1]) + P[2])
    d0, d1 = t - P[0], t - (P[0] + P[1])
    idx = np.where(d0.v > 0, np.where(d1.v > 0, 2, 1), 0)
    row["lam"] = np.asarray(sr.LAMBDA_VALUES, dtype=LD)[idx].reshape(R, 1)
    bound["lam"] = np.zeros((R, 1))
    lam_robust = pi_robust & _sure(d0) & ((idx == 0) | _sure(d1))
    # xi_v = [ua <= 1/2]
    ua, _ = draw2(key, it, SITE_INIT_XI, np.arange(V))
    row["xi"], bound["xi"] = np.asarray(ua <= 0.5, dtype=LD).reshape(V, 1), np.zeros((V, 1))
    # M ~ InverseWishart(nu, I) = T' T, T the inverse of the Bartlett factor A (sweep_ref.M_ref with C = I: B = T' without a product)
    j = np.arange(R)
    chi, _att, chi_robust = gamma_ve(_exact_or_rounded(LD(0.5) * (LD(float(nu)) - np.asarray(j, dtype=LD))), key, it, SITE_INIT_M_CHI, j)
    chi_robust = chi_robust & ~vacuous(chi.v, SAFETY * chi.e)
    Ad = vsqrt(2.0 * VE(chi.v, np.where(chi_robust, chi.e, 0.0)))
    A, eA = np.zeros((R, R), dtype=LD), np.zeros((R, R))
    A[j, j], eA[j, j] = Ad.v, Ad.e
    il, jl = np.tril_indices(R, -1)
    if il.size:
        A[il, jl], eA[il, jl] = normal(key, it, SITE_INIT_M_N, il * R + jl)
    T = sr.tri_inverse(A)
    aT, aA = absm(T), absm(A)
    ok2 = sr.second_order_ok(eA + gamma_m(R) * aA, T)
    eT = aT @ eA @ aT + gamma_m(R) * (aT @ aA @ aT)                          # the variates' errors, then Higham Thm 8.5
    row["M"] = T.T @ T
    bound["M"] = SAFETY * (eT.T @ aT + aT.T @ eT) + gamma_m(R) * (aT.T @ aT)
    if not (ok2 and chi_robust.all()):
        bound["M"] = np.full((R, R), np.inf)
    # u_rv
    z, ez = normal(key, it, SITE_INIT_U, np.arange(R * V))
    row["u"], bound["u"] = z.reshape(V, R).T.copy(), ez.reshape(V, R).T.copy()
    # gamma_e = W_e + sqrt(S_e) z_e; W as sweep_ref.compute_W, and the errors of the u it is summed from: each term twice NORMAL_REL
    el, ek = sr.edge_nodes(V)
    W, eW = sr.compute_W(row["u"], row["lam"], el, ek)
    eW = eW * (1 + 2 * NORMAL_REL / gamma_m(2 * R + 1))
    gam = VE(W, eW) + vsqrt(S) * VE(*normal(key, it, SITE_INIT_GAMMA, np.arange(q)))
    row["gamma"] = gam.v.reshape(q, 1)
    bound["gamma"] = np.where(lam_robust.all(), SAFETY * gam.e, np.inf).reshape(q, 1)
    return dict(row=row, bound=bound, lam_robust=lam_robust, pi_robust=pi_robust, chi_robust=chi_robust, second_order_ok=ok2)


EQUAL = ("theta", "Delta", "mu", "tau2", "xi", "lam")
RAW = ("S", "u")          # the columns that are one variate each: S one logarithm, u one normal


def raw_units(got, ref):
    """the largest error of the raw columns in rounding units u = 2^-53 of the value: what the device's log and normal were measured at"""
    out = {}
    for k in RAW:
        v = ref["row"][k]
        err = absm(np.asarray(f64(got[k]).reshape(v.shape), dtype=LD) - v)
        with np.errstate(divide="ignore", invalid="ignore"):
            out[k] = float(np.max(np.where(err > 0, err / (U * absm(v)), 0.0)))
    return out


def check_init(got, ref):
    """a fetched (or the oracle's) row against init_ref's: ({column: largest error / bound}, decisions checked, decisions skipped).  xi and the
    four constants must be equal; lambda must be equal unless its decision was too close to call; every other column lies within its bound
    (entries whose bound is infinite hang on a skipped decision and are not checked)."""
    assert ref["second_order_ok"], "the Bartlett factor is too ill-conditioned for a first-order bound: another seed"
    worst = {}
    for k in ("theta", "Delta", "mu", "tau2", "xi"):
        assert np.array_equal(f64(got[k]), f64(ref["row"][k])), k
        worst[k] = 0.0
    lam_eq = f64(got["lam"]).ravel() == f64(ref["row"]["lam"]).ravel()
    assert np.all(lam_eq | ~ref["lam_robust"]), ("lam", np.flatnonzero(~lam_eq))
    worst["lam"] = 0.0
    for k in ("S", "pi", "M", "u", "gamma"):
        g = f64(got[k]).reshape(ref["row"][k].shape)
        assert np.all(np.isfinite(g)), k
        b = ref["bound"][k]
        fin = np.isfinite(b)
        worst[k] = sr.ratio(absm(np.asarray(g, dtype=LD) - ref["row"][k])[fin], b[fin])
    R = ref["lam_robust"].size
    skipped = int(np.sum(~ref["lam_robust"])) + 3 * int(np.sum(~ref["pi_robust"])) + int(np.sum(~ref["chi_robust"]))
    return worst, 5 * R, skipped
