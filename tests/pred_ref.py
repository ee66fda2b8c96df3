"""Extended-precision host reference, with an a-priori bound of the device's float64 error, of the prediction, WAIC and PSIS-LOO kernels of
bnr_analysis_kernels.h: k_predict, k_pred_loglik, k_pred_pit, k_psis, k_psis_w, k_inv_sd, k_loo_moments, k_loo_quantile (numpy; scipy's erfc as a
cross-check).

The mathematical definitions (the kernels' headers; api._gpdfit, _psis_row, _psis_weights_row for loo 2.x's psis.R / gpdfit.R) are transcribed
once over gig_ref.VE: long double values that carry a running first-order bound of the error of the device's float64 evaluation.  On top of
VE's + - * / sqrt log exp:
  vlog1p, vexpm1   LIBM_ULPS u |z|, operand errors through 1 / (1 + a) and e^a
  verfc            erfc_ld, a long-double series / continued fraction.  scipy.special.erfc in float64 is too inaccurate to serve as the
                   reference (tests/test_pred_ref_host.py prints 31 ulp for |z| <= 8; hundreds in the far tail, where it rounds a^2 in
                   the exponent) and stays as a cross-check.  erfc_ld's own error ERFC_REF_ULPS u |z| (tests/test_pred_ref_host.py holds it against
                   mpmath) and the device's budget ERFC_ULPS u |z| both go into the bound
  vsum             thread-strided partial sums, then a tree: gamma_(ceil(S / stride) + levels) over sum |terms| (256 threads and 8 levels in
                   every kernel here; 64 lanes and 6 levels for the GPD grid)
  vlse             the running log-sum-exp merges (bnr_lse_merge): a term's path is at most ceil(S / 256) + 9 merges, each an exp, a product
                   and a sum; the maxima only grow along a path, so the roundings of the differences m - m2 add up to u (max - term)
  pow2             a product with a power of two is exact
A constant of the kernels that is a rounded real (log 2 pi, sqrt 2) is the real here with u |c| as its error.  An exp whose value is below
the smallest normal double gets an absolute 2^-1074 (the relative model does not hold for denormals).

Decisions (psis).  For a row given as data the device's lw = fl(fl(-l) - rmax) is formed in float64 here too, so membership and order of
the tail are exact: the M largest by (lw, draw) (k_psis_w); k_psis replaces the l of the tied keys by their largest, which moves elpd by at
most their spread (`tie_spread`, added to elpd's bound).  For a row that comes from eta, l carries a bound: the row is `decided` for the
per-draw weights only when every adjacent pair of the sorted tail and the cutoff pair are farther apart than SAFETY x their bounds.  The
fit's own tests (|hi - lo| < eps / 100, isfinite(k), sigma <= 0) follow the same too-close-to-call rule (`fit_decided`).  elpd and k-hat are
continuous in l and always carry a bound.  The final bounds are multiplied by SAFETY (the second-order terms).

What the bounds cannot see.  A deterministic bound adds the errors of the terms of a sum with one sign.  Where a result sums hundreds of
independently rounded terms -- the mean of eta over a window, loo_mean / loo_sd / loo_pit through the errors of all the weights, every sum
of the row of 2^21 + 513 draws (gamma_8200) -- the device's error is some 1000 times below the bound, and an error of that size in those
sums alone would pass.  So those stages are also checked where the terms are known exactly: the mean of eta against the strided sum of
the device's own per-draw eta, the LOO moments against the sums over the device's own weights (check_loo_sums); what is left in those
bounds is the rounding of the sum itself.  The 2^21 + 513-draw row has no such second check: it is there for the selection.
The reference's own rounding is the same chain with u = 2^-64: 1/2048 of the device's."""
import math

import numpy as np
from scipy.special import erfc as _erfc64

import sweep_ref as sr
from gig_ref import VE, ve, vsqrt, vlog, vexp, _r
from sweep_ref import LD, U, SAFETY, LIBM_ULPS, LOG2PI, gamma_m, f64

ERFC_REF_ULPS = 1.0 / 8       # erfc_ld against 40 digits over test_pred_ref_host's grid: 0.08 (scipy's float64 erfc: 31 ulp up to |z| = 8, 500 at 37)
ERFC_ULPS = 4.0               # the device's erfc: test_pred_exact_gpu's probe measured 1.76 ulp at most against erfc_ld on an MI355X (log: 0.36)
NONVACUOUS = 1e-9             # a bound that is a check: below NONVACUOUS max(|value|, 1)
SKIP_FRACTION = 0.05          # as tests/test_d_update_gpu.py
DENORM = 2.0 ** -1074
TINY = 2.0 ** -1022
EPS100 = 2.220446049250313e-16 / 100
LD_SQRT2 = np.sqrt(LD(2))
LD_2_SQRTPI = LD(2) / np.sqrt(LD("3.14159265358979323846264338327950288"))
C_LOG2PI = VE(LOG2PI, U * float(LOG2PI))
C_SQRT2 = VE(LD_SQRT2, U * float(LD_SQRT2))
C_INV_SQRT2 = VE(1 / LD_SQRT2, U * float(1 / LD_SQRT2))


# ------------------------------------------------------------------------------------------------------------------ operations on VE
def pow2(a, c):
    """a c for a power of two c: no rounding"""
    return VE(a.v * LD(c), a.e * abs(c))


def vsq(a):
    """a^2 with the second-order term of the operand's error (the first-order bound of a square vanishes at a = 0)"""
    z = a.v * a.v
    return VE(z, 2 * np.abs(f64(a.v)) * a.e + a.e * a.e + _r(z))


def vlog1p(a):
    z = np.log1p(a.v)
    return VE(z, a.e / np.abs(f64(1 + a.v)) + LIBM_ULPS * _r(z))


def vexpm1(a):
    z = np.expm1(a.v)
    return VE(z, a.e * f64(np.exp(a.v)) + LIBM_ULPS * _r(z))


def vexp_d(a):
    """vexp with the absolute floor of a denormal result"""
    z = vexp(a)
    return VE(z.v, z.e + np.where(f64(z.v) < TINY, DENORM, 0.0))


def _exp_neg_sq(a):
    """exp(-a^2) in long double without the rounding of a^2 in the exponent (a^2 up to 700): a = ah + al, ah of 24 bits, ah^2 exact"""
    ah = np.asarray(np.asarray(a, dtype=np.float32), dtype=LD)
    al = a - ah
    return np.exp(-ah * ah) * np.exp(-(2 * ah * al + al * al))


def erfc_ld(a):
    """erfc in long double.  Up to 1.5: 1 - erf(a), erf(a) = 2 / sqrt(pi) exp(-a^2) sum_n 2^n a^(2n+1) / (2n+1)!! (terms of one sign; below
    -9 the value is 2); above: exp(-a^2) / sqrt(pi) / (a + (1/2) / (a + 1 / (a + (3/2) / (a + ...)))), 300 levels from the back"""
    a = np.asarray(a, dtype=LD)
    small = a <= LD(1.5)
    x = np.where(small, np.maximum(a, LD(-9)), LD(0))
    t, s, x2 = x.copy(), x.copy(), 2 * x * x
    for n in range(600):
        t = t * x2 / LD(2 * n + 3)
        s = s + t
    lo = 1 - LD_2_SQRTPI * _exp_neg_sq(x) * s
    y = np.where(small, LD(2), a)
    f = y.copy()
    for k in range(300, 0, -1):
        f = y + LD(k) / 2 / f
    hi = _exp_neg_sq(y) * (LD_2_SQRTPI / 2) / f
    return np.where(small, lo, hi)


def verfc(a):
    z = erfc_ld(a.v)
    d = f64(LD_2_SQRTPI * _exp_neg_sq(a.v))
    return VE(z, d * a.e + (ERFC_REF_ULPS + ERFC_ULPS) * _r(z) + np.where(f64(z) < TINY, DENORM, 0.0))


def vsum(t, stride=256, levels=8):
    """the sum over the last axis in the kernels' order: thread-strided partial sums, then a tree"""
    n = t.v.shape[-1]
    z = np.sum(t.v, axis=-1)
    return VE(z, np.sum(t.e, axis=-1) + gamma_m(-(-n // stride) + levels) * np.sum(np.abs(f64(t.v)), axis=-1))


def vseq(t):
    """a sequential sum of one thread over the last axis"""
    return vsum(t, 1, 0)


def vlse(t, count=None, merges=None):
    """log sum_s c_s exp(t_s) over the last axis by running merges (bnr_lse_merge in thread-strided order, then bnr_psis_lse_tree);
    count: the multiplicities c_s (exact small integers), default 1"""
    n = t.v.shape[-1]
    nm = (-(-n // 256) + 9) if merges is None else merges
    m = np.max(t.v, axis=-1, keepdims=True)
    d = t.v - m
    ex = np.exp(d) * (1 if count is None else np.asarray(count, dtype=LD))
    s = np.sum(ex, axis=-1)
    rel = t.e + U * np.abs(f64(d)) + nm * (LIBM_ULPS + 2) * U
    es = np.sum(f64(ex) * rel, axis=-1) + DENORM * n
    z = m[..., 0] + np.log(s)
    return VE(z, es / f64(s) + LIBM_ULPS * _r(np.log(s)) + _r(z))


def vmin0(a):
    return VE(np.minimum(a.v, 0), a.e)


def _sure(margin):
    return np.abs(f64(margin.v)) > SAFETY * margin.e


# ------------------------------------------------------------------------------------------------------------------ k_predict
def eta(X, gamma, mu):
    """eta[i, s] = mu_s + sum_e X[i, e] gamma_s[e] (gamma: S x q, mu: S): one FMA per product in a fixed order over q16 columns on the f64
    matrix pipe, then the sum with mu: gamma_(q16 + 2) over |x| |gamma| + |mu|"""
    X, gamma, mu = f64(X), f64(gamma), f64(mu)
    q16 = -(-X.shape[1] // 16) * 16
    v = np.asarray(X, dtype=LD) @ np.asarray(gamma, dtype=LD).T + np.asarray(mu, dtype=LD)[None, :]
    return VE(v, gamma_m(q16 + 2) * (np.abs(X) @ np.abs(gamma).T + np.abs(mu)[None, :]))


# ------------------------------------------------------------------------------------------------------------------ k_pred_loglik, k_pred_pit
def ell(y, eta, tau2):
    """l[i, s] = log N(y_i | eta_is, tau2_s) = -(log 2 pi + log tau2_s) / 2 - (y_i - eta_is)^2 / (2 tau2_s) (bnr_pred_ell)"""
    t = VE(np.asarray(f64(tau2), dtype=LD))
    r = VE(np.asarray(f64(y), dtype=LD).reshape(-1, 1)) - ve(eta)
    return pow2(C_LOG2PI + vlog(t), -0.5) - r * r / pow2(t, 2.0)


def lpd_pwaic(l):
    """(lpd, pwaic) over the last axis: the log-mean-exp around the largest l (a constant of the formula: lpd does not depend on it) and the
    two-pass ddof-1 variance.  One draw: lpd = l, pwaic NaN (0 / 0)"""
    S = l.v.shape[-1]
    mx = VE(np.asarray(f64(np.max(l.v, axis=-1, keepdims=True)), dtype=LD))
    se = vsum(vexp_d(l - mx))
    lpd = VE(mx.v[..., 0]) + vlog(se / float(S))
    mean = vsum(l) / float(S)
    dl = l - VE(mean.v[..., None], mean.e[..., None])
    with np.errstate(invalid="ignore", divide="ignore"):
        pw = vsum(vsq(dl)) / float(S - 1)
    return lpd, pw


def phi(y, eta, tau2):
    """Phi((y - eta) / sqrt(tau2)) = erfc(-z / sqrt 2) / 2 per draw, as k_pred_pit and k_loo_moments form it"""
    z = (ve(y) - ve(eta)) / vsqrt(ve(tau2))
    return pow2(verfc(-z / C_SQRT2), 0.5)


def pit(y, eta, tau2):
    """pit_i = mean_s Phi((y_i - eta_is) / sqrt(tau2_s))"""
    p = phi(VE(np.asarray(f64(y), dtype=LD).reshape(-1, 1)), eta, VE(np.asarray(f64(tau2), dtype=LD)))
    return vsum(p) / float(p.v.shape[-1])


# ------------------------------------------------------------------------------------------------------------------ PSIS
def tail_length(S, r_eff=1.0):
    """loo's n_pareto: ceil(min(0.2 S, 3 sqrt(S / r_eff)))"""
    return int(math.ceil(min(0.2 * S, 3.0 * math.sqrt(S / r_eff))))


def r_eff_for(S, M):
    """an r_eff that makes the tail length of S draws M (3 sqrt(S / r) just below M); M <= 0.2 S"""
    r = 9.0 * S / (M - 0.5) ** 2
    assert tail_length(S, r) == M, (S, M, tail_length(S, r))
    return r


def gpdfit(x):
    """bnr_psis_gpd_fit on the ascending tail x (VE, M entries): (k after the prior adjustment, sigma, k before it), each a VE.
    The profile log-likelihood l(theta) = M (log(-theta / k(theta)) - k(theta) - 1), k = mean log1p(-theta x), is flat where its weight
    is, and the weighted mean of the grid moves only by the spread of the grid under a change of the weights.  Operand by operand both
    would be lost (M times the error of theta, and theta times the error of the weights), so these two stages are composite operations
    like gig_ref.vxinv: the errors of their inputs go through the exact partial derivatives, the roundings of the stage itself are those
    of its chain on error-free inputs"""
    M = x.v.shape[-1]
    mg = 30 + int(math.floor(math.sqrt(M)))
    xN, xstar = x[M - 1], x[int(math.floor(M / 4.0 + 0.5)) - 1]
    root = VE(np.sqrt(LD(mg) / (np.arange(mg, dtype=LD) + LD(0.5))))
    root = VE(root.v, 2 * _r(root.v))                                            # the quotient and the root
    theta = 1.0 / xN + (1.0 - root) / 3.0 / xstar
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        # l(theta_j): the chain on error-free inputs, then d l = M (1 / theta - (1 / k + 1) k') d theta + sum_t (1 / k + 1) theta / (1 - theta x_t) d x_t
        a, x0 = VE(-theta.v), VE(x.v)
        ax = VE(a.v[:, None]) * VE(x0.v[None, :])
        kj = vsum(vlog1p(ax), 64, 6) / float(M)
        lth = float(M) * (vlog(a / kj) - kj - 1.0)
        den = 1 + ax.v                                                            # 1 - theta_j x_t
        kp = np.mean(-x.v[None, :] / den, axis=1)
        g = 1 / kj.v + 1
        d_th = np.abs(f64(M * (1 / theta.v - g * kp)))
        d_x = np.abs(f64(g[:, None] * theta.v[:, None] / den))
        lth = VE(lth.v, lth.e + d_th * theta.e + d_x @ x.e)
        # theta_hat = sum_j theta_j w_j, w = softmax(l): d theta_hat = sum_j w_j d theta_j + sum_j w_j (theta_j - theta_hat) d l_j
        l0, t0 = VE(lth.v), VE(theta.v)
        jm = int(np.argmax(f64(l0.v)))
        rest = np.arange(mg) != jm
        lse = l0[jm] + vlog1p(vseq(vexp_d(l0[rest] - l0[jm])))
        th = vseq(t0 * vexp_d(l0 - lse))
        w = f64(np.exp(l0.v - lse.v))
        th = VE(th.v, th.e + np.sum(w * theta.e) + np.sum(w * np.abs(f64(theta.v - th.v)) * lth.e))
        k0 = vsum(vlog1p(-th * x)) / float(M)
        sigma = -k0 / th
        kh = k0 * float(M) / float(M + 10) + VE(LD(5) / LD(M + 10), U * 5.0 / (M + 10))
    return kh, sigma, k0


def psis(l, M, weights=True):
    with np.errstate(over="ignore", invalid="ignore"):                            # (|l| up to 1e300: a bound may overflow to inf)
        return _psis(l, M, weights)


def _psis(l, M, weights):
    """The PSIS of one row of S log-likelihood draws with tail length M.  l: a float64 array (data: FROM_E = 0, exact) or a VE (from eta).
    weights True: k_psis_w (the tail is the M largest in (lw, draw)); False: k_psis (elpd's bound carries the spread of l over the keys tied
    with the cutoff).  Returns a dict: lpd, elpd, khat (VE; khat None: no fit, the device returns +inf), sigma, cutoff (index), tail (indices,
    ascending in (lw, draw)), tail_lw (the smoothed tail, VE), lw (the normalised log weights, VE), smoothed, decided (membership and order
    of the tail), fit_decided, finite"""
    data = not isinstance(l, VE)
    if data:
        l64 = f64(l).ravel()
        l = VE(np.asarray(l64, dtype=LD))
    S = l.v.shape[0]
    out = dict(M=M, S=S, khat=None, sigma=None, k0=None, cutoff=None, tail=np.zeros(0, dtype=int), tail_lw=None, smoothed=False, decided=True,
               fit_decided=True, finite=bool(np.all(np.isfinite(f64(l.v)))), tie_spread=0.0)
    out["lpd"] = lpd_pwaic(l)[0]
    if not out["finite"]:
        return out
    if data:
        rmax = -np.min(l64)
        lw = VE(np.asarray((-l64) - rmax, dtype=LD))                              # the device's own float64 subtraction: exact keys
    else:
        i = int(np.argmin(l.v))
        lw = (-l) - VE(-l.v[i], l.e[i])
    terms_lw, cnt_tail = lw, None
    if M >= 5 and S > M:
        order = np.lexsort((np.arange(S), lw.v))
        tail, cut = order[S - M:], order[S - M - 1]
        out["tail"], out["cutoff"] = tail, cut
        chain = np.r_[cut, tail]
        gaps = VE(lw.v[chain[1:]] - lw.v[chain[:-1]], lw.e[chain[1:]] + lw.e[chain[:-1]])
        out["decided"] = bool(data or np.all(_sure(gaps)))
        if data:
            tied = f64(lw.v) == f64(lw.v[cut])
            out["tie_spread"] = float(np.max(l64[tied]) - np.min(l64[tied]))
        lt = lw[tail]
        spread = VE(np.abs(lt.v[-1] - lt.v[0]) - LD(EPS100), lt.e[-1] + lt.e[0] + _r(lt.v[-1] - lt.v[0]))
        out["fit_decided"] = bool(_sure(spread))
        if spread.v >= 0:
            ec = vexp_d(lw[cut])
            kh, sigma, _k0 = gpdfit(vexp_d(lt) - ec)
            out["khat"], out["sigma"], out["k0"] = kh, sigma, _k0
            fin = bool(np.isfinite(f64(kh.v)) and np.isfinite(kh.e))
            out["fit_decided"] = out["fit_decided"] and fin and bool(_sure(sigma))
            if fin and sigma.v > 0:
                p = VE((np.arange(M, dtype=LD) + LD(0.5)) / LD(M))
                p = VE(p.v, _r(p.v))
                qq = sigma * vexpm1(-kh * vlog1p(-p)) / kh
                sm = vmin0(vlog(qq + ec))
                out["tail_lw"], out["smoothed"] = sm, True
                v, e = lw.v.copy(), lw.e.copy()
                v[tail], e[tail] = sm.v, sm.e
                terms_lw = VE(v, e)
    elif M >= 5:
        raise ValueError("the tail length %d needs more than %d draws" % (M, S))
    terms_lw = vmin0(terms_lw)
    lz = vlse(terms_lw)
    num = vlse(terms_lw + l)
    elpd = num - lz
    out["elpd"] = VE(elpd.v, elpd.e + (0.0 if weights else out["tie_spread"] / SAFETY))
    out["lw"] = terms_lw - VE(np.full(S, lz.v), np.full(S, lz.e))
    out["lw_raw"] = lw
    return out


# ------------------------------------------------------------------------------------------------------------------ LOO predictive checks
def loo_moments(eta, tau2, y, lw):
    """k_loo_moments of one row: (mean, sd, pit) as VE from eta (S; VE or exact), tau2 (S), y (scalar) and the normalised log weights (VE)"""
    eta = eta if isinstance(eta, VE) else VE(np.asarray(f64(eta), dtype=LD))
    t = VE(np.asarray(f64(tau2), dtype=LD))
    w = vexp_d(lw)
    mean = vsum(w * eta)
    a2 = vsum(w * (t + eta * eta))
    pt = vsum(w * phi(VE(LD(float(y))), eta, t))
    with np.errstate(invalid="ignore"):
        sd = vsqrt(a2 - mean * mean)
    return mean, sd, pt


def inv_sd(tau2):
    """k_inv_sd: 1 / sqrt(tau2)"""
    return 1.0 / vsqrt(VE(np.asarray(f64(tau2), dtype=LD)))


def mixture_cdf(t, w, eta, sd):
    """F(t) = sum_s w_s Phi((t - eta_s) / sd_s) as k_loo_quantile evaluates it: z = (t - eta) isd, w (0.5 erfc(z (-1 / sqrt 2))).  w: VE
    (exp of the log weights); sd: the float64 sds (isd = 1 / sd carries its own roundings)"""
    isd = 1.0 / VE(np.asarray(f64(sd), dtype=LD), U * np.abs(f64(sd)))
    z = (VE(LD(float(t))) - ve(eta)) * isd
    return vsum(w * pow2(verfc(z * (-C_INV_SQRT2)), 0.5))


def mixture_pdf(t, w, eta, sd):
    """F'(t) in float64 (the slope that turns the bisection's last bracket into a residual of F)"""
    z = (float(t) - f64(eta)) / f64(sd)
    return float(np.sum(f64(w) * np.exp(-0.5 * z * z) / (math.sqrt(2 * math.pi) * f64(sd))))


def bracket_width(eta, sd, c):
    """the width of k_loo_quantile's starting bracket [min(eta - c sd), max(eta + c sd)]"""
    eta, sd = f64(eta), f64(sd)
    return float(np.max(eta + c * sd) - np.min(eta - c * sd))


# ------------------------------------------------------------------------------------------------------------------ checks
def nonvacuous(x):
    """the bound of x is a check: finite and below NONVACUOUS max(|value|, 1)"""
    with np.errstate(invalid="ignore"):
        return np.isfinite(x.e) & (SAFETY * x.e < NONVACUOUS * np.maximum(np.abs(f64(x.v)), 1.0))


def err_ratio(got, x):
    """largest |got - x.v| / (SAFETY x.e) (0 where got equals the reference exactly; inf where got is not finite)"""
    got = f64(got)
    with np.errstate(invalid="ignore"):
        err = sr.absm(np.asarray(got, dtype=LD) - x.v)
    err = np.where(np.isfinite(got), f64(err), np.inf)
    return sr.ratio(err, SAFETY * np.asarray(x.e))


# ------------------------------------------------------------------------------------------------------------------ the crafted inputs
def exact_X(m, q, seed, kmax=128):
    """m x q entries k / 16, |k| <= kmax"""
    return np.random.default_rng(seed).integers(-kmax, kmax + 1, (m, q)) / 16.0


def craft_exact(t, seed, offset=0, tau_lo=1e-3, tau_hi=1e3):
    """Overwrite gamma, mu and tau2 of the table t: gamma_s[e] = ((7 s' + 13 e) mod 127 - 63) / 8 and mu_s = (s' mod 17) / 4 with s' = the
    0-based table row + offset -- index-coded, so a mis-indexed operand changes eta, and with X = k / 16 every partial sum of eta is a
    multiple of 1 / 128 far below 2^53 / 128: eta is exact in any order --; tau2 log-uniform over [tau_lo, tau_hi]"""
    tot, q = t["gamma"].shape[:2]
    s = np.arange(tot) + offset
    t["gamma"][:, :, 0] = ((7 * s[:, None] + 13 * np.arange(q)[None, :]) % 127 - 63) / 8.0
    t["mu"][:, 0, 0] = (s % 17) / 4.0
    t["tau2"][:, 0, 0] = np.exp(np.random.default_rng(seed).uniform(math.log(tau_lo), math.log(tau_hi), tot))
    return t


def window(tables, first, nsamp):
    """(gamma S x q, mu, tau2) of rows first .. first + nsamp - 1 (1-based) of the tables, pooled in order"""
    sl = slice(first - 1, first - 1 + nsamp)
    return (np.concatenate([t["gamma"][sl, :, 0] for t in tables]), np.concatenate([t["mu"][sl, 0, 0] for t in tables]),
            np.concatenate([t["tau2"][sl, 0, 0] for t in tables]))


def exact_eta(X, gamma, mu):
    """eta of the exact tables as float64, with the proof that it is exact: the long-double value is a double"""
    e = eta(X, gamma, mu).v
    assert np.array_equal(np.asarray(f64(e), dtype=LD), e)
    return f64(e)


def gpd_row(S, k, rng, scale=1.0):
    """log-likelihoods whose ratios exp(-l) have a generalized Pareto tail of shape k"""
    u = rng.random(S)
    return -np.log(scale * ((1 - u) ** (-k) - 1) / k + 1e-300)


def _spaced(n, lo, hi, rng):
    """n distinct values in (lo, hi), no two closer than (hi - lo) / (4 n)"""
    return lo + (hi - lo) * (np.arange(n) + 0.25 + 0.5 * rng.random(n)) / n


def digits_row(S, M, rng, cluster=40, inside=8):
    """lw = -l (one draw has l = 0 = the largest ratio, so rmax = 0 and the keys are those of -l): `cluster` consecutive doubles around the
    cutoff, `inside` of them in the tail -- keys that agree in all but the lowest 9 bits, across a multiple of 512 --, the rest of the tail
    spread above, the other draws below"""
    base = 3.0
    bits = np.float64(base).view(np.int64)
    bits = (bits // 512) * 512 + 512 - cluster // 2                                # straddles a change of the second-lowest digit
    cl = (bits + np.arange(cluster)).astype(np.int64).view(np.float64)            # ascending l = descending lw
    top = _spaced(M - inside - 1, 0.05, 2.9, rng)                                  # smaller l: in the tail, with l = 0
    rest = _spaced(S - M - (cluster - inside), 3.1, 12.0, rng)
    l = np.r_[0.0, top, cl, rest]
    assert l.size == S
    return l[rng.permutation(S)]


def bins_row(S, M, rng, tiny=10):
    """lw = -l over all the bins of the select's top digit: |lw| from 1e-300 to 1e300, `tiny` draws below 1e-3, the rest of the tail in
    [1e-3, 3], everything else up to 1e300"""
    l = np.r_[0.0, 10.0 ** _spaced(tiny - 1, -300, -3, rng), _spaced(M - tiny + 1, 1e-3, 3.0, rng), 10.0 ** _spaced(S - M - 1, 0.5, 300, rng)]
    assert l.size == S
    return l[rng.permutation(S)]


def tie_row(S, M, rng, variant):
    """ties at the cutoff.  The sorted lw, from the top: `above` distinct keys, then a group of `ng` equal keys, then distinct keys.
    "more": the group is longer than M and starts at the top (a constant tail: no fit); "all": the group fills the end of the tail and
    the cutoff is the next distinct key; "none": the cutoff is the first of the group (want = 1); "some": the group straddles the cutoff;
    "rounded": as "some", but the group is six consecutive doubles of l that the rounding of -l - rmax (rmax = 100) merges into one key"""
    ng = 12
    above = {"more": 0, "all": M - ng, "none": M, "some": M - 5, "rounded": M - 3}[variant]
    if variant == "more":
        ng = M + 7
    if variant == "rounded":
        hi = _spaced(above, 1.0, 1.9, rng)
        grp = (np.float64(2.0).view(np.int64) + np.arange(6)).astype(np.int64).view(np.float64)
        lo = _spaced(S - above - 6 - 1, 2.1, 6.0, rng)
        l = np.r_[hi, grp, lo, -100.0]
        lw = (-l) - 100.0
        assert np.unique(lw[above:above + 6]).size == 1 and np.unique(l).size == S
        assert np.sum(lw > lw[above]) == above + 1                                  # (+ the draw that sets rmax: lw = 0)
    else:
        l = np.r_[0.0, _spaced(above - 1, 0.05, 1.9, rng), np.full(ng, 2.0), _spaced(S - above - ng, 2.1, 9.0, rng)] if above else \
            np.r_[np.full(ng, 0.0), _spaced(S - ng, 0.5, 9.0, rng)]
    assert l.size == S
    return l[rng.permutation(S)]


BIG_S = 2 ** 21 + 513
BIG_TIED = [5, 1023, 1024, 1500, 2047, 2048, 3000, 2 ** 21 - 1, 2 ** 21, 2 ** 21 + 100, 2 ** 21 + 512]
BIG_ABOVE = 59


def big_row(rng, S=BIG_S):
    """S = 2^21 + 513 draws with eleven keys tied at the cutoff, at draw indices on both sides of 2^10, 2^11 and 2^21: with M = BIG_ABOVE + t
    the t tied draws of the largest index join the tail, and s_c, the smallest of them, is found by the 11 + 11 + 10-bit select.  The other
    draws: BIG_ABOVE above the ties, the rest below"""
    l = 2.5 + 7.0 * rng.random(S)
    free = np.setdiff1d(rng.choice(S, 200, replace=False), BIG_TIED)[:BIG_ABOVE]
    l[free] = np.r_[0.0, _spaced(BIG_ABOVE - 1, 0.05, 1.9, rng)]
    l[BIG_TIED] = 2.0
    return l


PSIS_NAMES = ["crafted_rows S=25", "crafted_rows S=400", "digits, bins and ties S=600", "tail lengths S=1300", "S=255", "S=256", "S=257", "S=2^21+513"]
_CASES = {}


def psis_cases(big=True):
    """psis_cases_build, built once (the rows of 2^21 + 513 draws take 50 MB); big False: without that case"""
    if big not in _CASES:
        _CASES[big] = psis_cases(True)[:-1] if not big else psis_cases_build()
        assert [c[0] for c in _CASES[big]] == PSIS_NAMES[:len(_CASES[big])]
    return _CASES[big]


def psis_cases_build(big=True):
    """the crafted log-likelihood matrices of the PSIS tests: a list of (name, ll m x S, M per row); the tail lengths are set through
    r_eff_for.  Deterministic."""
    from test_loo_gpu import crafted_rows
    cases = []
    for S in (25, 400):
        cases.append(("crafted_rows S=%d" % S, crafted_rows(S, np.random.default_rng(S)), [tail_length(S)] * 6))
    rng = np.random.default_rng(600)
    S, M = 600, tail_length(600)
    rows = [digits_row(S, M, rng), digits_row(S, M, rng, 64, 12), bins_row(S, M, rng)] + [tie_row(S, M, rng, v) for v in ("more", "all", "none", "some", "rounded")]
    cases.append(("digits, bins and ties S=600", np.array(rows), [M] * len(rows)))
    rng = np.random.default_rng(1300)
    Ms = [4, 5, 8, 9, 64, 65, 255, 256, 257]
    cases.append(("tail lengths S=1300", np.array([gpd_row(1300, 0.4, rng) for _ in Ms]), Ms))
    for S in (255, 256, 257):
        rng = np.random.default_rng(S)
        Ms = [5, 17, 33, 48, 51]
        cases.append(("S=%d" % S, np.array([gpd_row(S, 0.1 + 0.15 * j, rng) for j in range(len(Ms))]), Ms))
    if big:
        rng = np.random.default_rng(21)
        row = big_row(rng)
        ts = [3, 6, 10]                                                           # s_c = 2^21, 2^11, 2^10 - 1
        cases.append(("S=2^21+513", np.array([row] * len(ts)), [BIG_ABOVE + t for t in ts]))
    return cases


# (V, rows m, nsamp, first row, predict_block_rows, chains pooled): every value of each axis once, the corners (m, nsamp) in {17, 33} x {33, 129}
PREDICT_V = {2: 3, 5: 15, 6: 21, 9: 45, 31: 496}                                   # V: q; 496 = 31 x 16: no padding in front of S
PREDICT_TOT = 300
PREDICT_CASES = [(2, 1, 1, 1, 0, 1), (2, 16, 15, 2, 0, 1), (2, 17, 16, 1, 1, 1), (2, 65, 257, 2, 32, 1),
                 (5, 31, 17, 3, 0, 1), (5, 32, 31, 1, 0, 1), (5, 33, 32, 7, 32, 1), (5, 65, 33, 1, 0, 1), (5, 17, 33, 5, 0, 3), (5, 33, 33, 1, 1, 3),
                 (6, 17, 33, 1, 0, 1), (6, 33, 33, 2, 0, 1), (6, 17, 129, 1, 0, 1), (6, 33, 129, 9, 32, 1), (6, 32, 128, 1, 1, 1),
                 (9, 65, 127, 1, 0, 1), (9, 16, 128, 11, 0, 1), (9, 1, 257, 1, 0, 1), (9, 32, 257, 40, 1, 1), (9, 33, 15, 1, 0, 1),
                 (31, 17, 33, 1, 0, 1), (31, 33, 129, 3, 0, 1), (31, 65, 257, 1, 32, 1), (31, 1, 1, 300, 0, 1), (31, 31, 16, 1, 1, 1)]
CHAIN_OFFSET = 50                                                                  # chain c of a pooled call is coded with s' = s + 50 c


def predict_X(V, m):
    return exact_X(m, PREDICT_V[V], 1000 * V + m)


def order_ranks(S):
    """the rank pairs of a whole-window call: (1, S), (2, S - 1) and the median pair, inside 1 .. S"""
    c = lambda k: min(max(k, 1), S)
    return [(1, S), (c(2), c(S - 1)), (c((S + 1) // 2), c(S // 2 + 1))]


def exact_mean(E):
    """the correctly rounded mean over the last axis of exact multiples of 1 / 128 (|sum| far below 2^63 / 128): the integer sum, one
    long-double quotient (the second rounding, to float64, is why the test allows an ulp)"""
    k = np.rint(E * 128.0).astype(np.int64)
    assert np.array_equal(k / 128.0, E)
    return f64(np.asarray(k.sum(axis=-1), dtype=LD) / LD(128 * E.shape[-1]))


# k_pred_loglik and k_pred_pit on the exact tables (q = 15): sparse small rows, so that only tau2 spreads l
LOGLIK_S = (1, 2, 255, 256, 257, 513)
LOGLIK_TOT = 520
LOGLIK_ROWS = 24


def loglik_rows(seed=77):
    """(X 24 x 15 with two entries +-1/16 or +-1/8 per row, y near the middle of eta); the first row is all zero"""
    rng = np.random.default_rng(seed)
    X = np.zeros((LOGLIK_ROWS, 15))
    for i in range(1, LOGLIK_ROWS):
        X[i, rng.choice(15, 2, replace=False)] = rng.choice([-2, -1, 1, 2], 2) / 16.0
    y = 2.0 + np.rint(8 * rng.standard_normal(LOGLIK_ROWS)) / 8.0
    return X, y


def craft_constant(t, kind):
    """mu = 1.25 in every row; "equal": tau2 = 0.37, so a zero row of X with any y has all l equal; "near": tau2 = 1 + d, d uniform over
    [0, 2e-9]: with y = mu + 44.75 l = -1002.2 with a spread of 1e-6 (the cancellation of the two-pass variance: ill-conditioned on purpose)"""
    tot = t["mu"].shape[0]
    t["mu"][:, 0, 0] = 1.25
    t["tau2"][:, 0, 0] = 0.37 if kind == "equal" else 1.0 + 2e-9 * np.random.default_rng(5).random(tot)
    return t


# the chain path: n = 20 training rows, 200 draws per chain, tau2 over [4, 40] (sd 2 .. 6.3 against a spread of eta of about 3)
LOO_N, LOO_S, LOO_FIRST = 20, 200, 3


def loo_training(seed=91):
    rng = np.random.default_rng(seed)
    X = rng.integers(-4, 5, (LOO_N, 15)) / 16.0
    y = 2.0 + np.rint(8 * 3.0 * rng.standard_normal(LOO_N)) / 8.0
    return X, y


def loo_reference(X, y, gamma, mu, tau2, p_lo, p_hi, c, r_eff=None):
    """the chain path's reference from the exact tables: per row the dict of psis (weights kept) plus l, eta, mean, sd, pit (VE), the
    bracket's width and F (a function t -> VE)"""
    E = exact_eta(X, gamma, mu)
    L = ell(y, VE(np.asarray(E, dtype=LD)), tau2)
    S = E.shape[1]
    sd = np.sqrt(f64(tau2))
    out = []
    for i in range(E.shape[0]):
        M = tail_length(S, 1.0 if r_eff is None else float(np.broadcast_to(r_eff, (E.shape[0],))[i]))
        d = psis(L[i], M)
        d["l"], d["eta"] = L[i], E[i]
        d["mean"], d["sd"], d["pit"] = loo_moments(E[i], tau2, y[i], d["lw"])
        d["width"] = bracket_width(E[i], sd, c)
        w = vexp_d(d["lw"])
        d["F"] = (lambda t, w=w, e=E[i]: mixture_cdf(t, w, VE(np.asarray(e, dtype=LD)), sd))
        d["dF"] = (lambda t, w=w, e=E[i]: mixture_pdf(t, w.v, e, sd))
        out.append(d)
    return out


def quantile_ratio(t_dev, p, d):
    """|F(t) - p| against F'(t) width 2^-40 + SAFETY e_F: the bisection's last bracket is 2^-40 of the first, every decision on the way is
    right unless F is within e_F of p"""
    F = d["F"](t_dev)
    return float(f64(np.abs(F.v - LD(p))) / (d["dF"](t_dev) * d["width"] * 2.0 ** -40 + SAFETY * F.e))


def check_psis(ref, elpd, khat, lw=None, lpd=None):
    """One row's outputs (of the device, or of a float64 restatement) against psis's dict: ({stage: error / bound}, skipped, problems).
    skipped: a test of the fit too close to call, or a bound that is no check (NONVACUOUS); such a row is only held to be finite.
    problems: what is wrong without a ratio (a fit where there is none, a draw in the wrong set)"""
    rat, bad = {}, []
    if not ref["finite"]:
        if not (np.isnan(elpd) and np.isposinf(khat) and (lw is None or np.all(np.isnan(lw)))):
            bad.append("a non-finite row must give elpd NaN, khat +inf, weights NaN")
        return rat, False, bad
    if lpd is not None:
        rat["lpd"] = err_ratio(lpd, ref["lpd"])
    kr = ref["khat"]
    skipped = not ref["fit_decided"] or not nonvacuous(ref["elpd"]) or (ref["smoothed"] and not nonvacuous(kr))
    if skipped:
        if not np.isfinite(elpd):
            bad.append("elpd not finite")
        return rat, True, bad
    rat["elpd"] = err_ratio(elpd, ref["elpd"])
    if ref["smoothed"]:
        rat["khat"] = err_ratio(khat, kr)
    elif not np.isposinf(khat):
        bad.append("khat %r where there is no fit" % khat)
    if lw is None or not ref["decided"]:
        return rat, lw is not None, bad
    lw = f64(lw)
    R, raw = ref["lw"], ref["lw_raw"]
    ok = nonvacuous(R)
    if not np.all(ok):
        skipped = True
    rat["weights"] = err_ratio(lw[ok], R[ok])
    with np.errstate(over="ignore", invalid="ignore"):
        w = f64(np.exp(R.v))
        rat["sum of weights"] = float(f64(np.abs(np.sum(np.exp(np.asarray(lw, dtype=LD))) - 1)) / (SAFETY * np.sum(w * R.e)))
        # outside the tail the normalisation is one subtraction of the same number: differences of the output are differences of the raw lw
        s0 = int(np.argmin(raw.v))
        d = np.abs(f64((np.asarray(lw, dtype=LD) - LD(lw[s0])) - (raw.v - raw.v[s0])))
        bnd = SAFETY * (U * (np.abs(lw) + abs(lw[s0])) + raw.e + raw.e[s0] + U * np.abs(f64(raw.v - raw.v[s0])))
    inside = np.zeros(lw.size, dtype=bool)
    if ref["smoothed"]:
        inside[ref["tail"]] = True
    rat["weights outside the tail"] = sr.ratio(d[~inside], bnd[~inside])
    moved = np.abs(f64(R.v - (raw.v + (R.v[s0] - raw.v[s0])))) > 2 * (bnd + SAFETY * R.e)       # the smoothing moved it visibly
    if np.any(inside & moved & ~(d > bnd)):
        bad.append("a draw of the reference's tail carries its raw weight")
    return rat, skipped, bad


# ------------------------------------------------------------------------------------------------------------------ cases and assertions shared by the host and the GPU test
def new_table(tot, V):
    """the columns of a state table that the prediction reads (Chain.load takes a table with the others missing)"""
    q = V * (V + 1) // 2
    return {k: np.zeros((tot, d, 1), order="F") for k, d in (("gamma", q), ("mu", 1), ("tau2", 1))}


def table(V, tot, seed, offset=0, **kw):
    return craft_exact(new_table(tot, V), seed, offset, **kw)


def real_case():
    """the real-valued case of k_predict: V = 12, normal X, gamma and mu"""
    rng = np.random.default_rng(12)
    t = new_table(300, 12)
    t["gamma"][:, :, 0] = rng.standard_normal((300, 78))
    t["mu"][:, 0, 0] = 10 * rng.standard_normal(300)
    t["tau2"][:] = 1.0
    return t, rng.standard_normal((37, 78))


def loglik_inputs():
    """(name, table, X, y, S values, ill-conditioned on purpose) of the log-likelihood cases"""
    X, y = loglik_rows()
    base = table(5, LOGLIK_TOT, 55)
    out = [("tau2 over 1e-3 .. 1e3", base, X, y, LOGLIK_S, False)]
    z = np.zeros((1, 15))
    out.append(("all l equal", craft_constant(table(5, LOGLIK_TOT, 55), "equal"), z, np.array([2.0]), (2, 257), False))
    out.append(("near-constant l", craft_constant(table(5, LOGLIK_TOT, 55), "near"), z, np.array([1.25 + 44.75]), (257, 513), True))
    return out


def check_pointwise(name, ref_lpd, ref_pw, ref_pit, lpd, pw, pit, S, ill, note):
    """the assertions shared with the GPU test: returns the number of rows skipped as vacuous"""
    n = len(lpd)
    note("lpd", err_ratio(lpd, ref_lpd), "%s S=%d" % (name, S))
    if S == 1:
        assert np.all(np.isnan(pw))
    else:
        note("pwaic", err_ratio(pw, ref_pw), "%s S=%d" % (name, S))
    note("pit", err_ratio(pit, ref_pit), "%s S=%d" % (name, S))
    if ill:
        return 0
    ok = nonvacuous(ref_lpd) & nonvacuous(ref_pit) & (nonvacuous(ref_pw) if S > 1 else True)
    return n - int(np.sum(ok))


_REFS = {}


def psis_ref(name, i, row, M):
    """psis(row, M) of row i of the case `name`: computed once, shared by the tests that need it and left unchanged"""
    key = (name, i, M)
    if key not in _REFS:
        _REFS[key] = psis(row, M)
    return _REFS[key]


def run_psis_case(name, ll, Ms, outputs, weights, note):
    """the assertions shared with the GPU test.  outputs: (lpd or None, elpd, khat, lw or None) of the m rows"""
    lpd, elpd, khat, lw = outputs
    skipped = 0
    for i, M in enumerate(Ms):
        ref = psis_ref(name, i, ll[i], M)
        if not weights:                                                           # k_psis: the spread of l over the keys tied with the cutoff
            ref = dict(ref, elpd=VE(ref["elpd"].v, ref["elpd"].e + ref["tie_spread"] / SAFETY))
        rat, skip, bad = check_psis(ref, elpd[i], khat[i], None if lw is None else lw[i], None if lpd is None else lpd[i])
        assert not bad, (name, i, M, bad)
        skipped += skip
        for stage, r in rat.items():
            note(("w " if weights else "") + stage, r, "%s row %d M=%d" % (name, i, M))
    return skipped


def loo_inputs(nc):
    X, y = loo_training()
    tabs = [table(5, LOGLIK_TOT, 200 + c, CHAIN_OFFSET * c, tau_lo=4.0, tau_hi=40.0) for c in range(nc)]
    return X, y, tabs


def check_loo_sums(name, E, tau2, y, lw, mean, sd, pit, note):
    """k_loo_moments alone: its outputs against the sums over the weights lw it was given (the device's own, as k_psis_w returns them for the
    device's own l), taken as exact: what is left in the bound is one exp, the products and the strided sum of every term -- a few ulps of
    sum w |eta|, where the bounds of check_loo also carry the whole error of the weights"""
    for i in range(E.shape[0]):
        m, s, p = loo_moments(E[i], tau2, y[i], VE(np.asarray(f64(lw[i]), dtype=LD)))
        what = "%s row %d" % (name, i)
        note("loo_mean over given weights", err_ratio(mean[i], m), what)
        note("loo_sd over given weights", err_ratio(sd[i], s), what)
        note("loo_pit over given weights", err_ratio(pit[i], p), what)


def check_loo(name, refs, fields, p_lo, p_hi, note):
    """the assertions shared with the GPU test.  fields: (lpd, elpd, khat, mean, sd, pit, lower, upper) per row; returns the rows skipped"""
    lpd, elpd, khat, mean, sd, pit, lower, upper = fields
    skipped = 0
    for i, d in enumerate(refs):
        rat, skip, bad = check_psis(d, elpd[i], khat[i], None, lpd[i])
        assert not bad, (name, i, bad)
        what = "%s row %d" % (name, i)
        for stage, r in rat.items():
            note("loo " + stage, r, what)
        ok = d["decided"] and not skip and all(bool(nonvacuous(d[k])) for k in ("mean", "sd", "pit"))
        if not ok:
            skipped += 1
            assert all(np.isfinite(v[i]) for v in (mean, sd, pit, lower, upper)), what
            continue
        note("loo_mean", err_ratio(mean[i], d["mean"]), what)
        note("loo_sd", err_ratio(sd[i], d["sd"]), what)
        note("loo_pit", err_ratio(pit[i], d["pit"]), what)
        note("loo_lower", quantile_ratio(lower[i], p_lo, d), what)
        note("loo_upper", quantile_ratio(upper[i], p_hi, d), what)
        assert lower[i] < mean[i] < upper[i], what
    return skipped


