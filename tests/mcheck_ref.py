"""The reference of the weighted mixture of normals of include/bnr_mcheck.h in mpmath at mloo_ref's precision (50 digits), and the error bounds
that a float64 evaluation has to meet.  Data only comes in as float64 (mean, var, the normalised log weights and y); nothing here is rounded to
float64 before the results are.

For one row with draws s = 1 .. D:  w_s = exp(lw_s),  m_s,  var_s,  sd_s = sqrt(var_s),  resid_s = y - m_s.
    mean = y - sum w resid  (without y: sum w m),   sd^2 = sum w (var + m^2) - mean^2,   F(t) = sum w Phi((t - m) / sd),   pit = F(y)
    Phi(z) = erfc(-z / sqrt 2) / 2;  var_s = 0 is the point mass [t >= m_s].

The bounds, to first order, with u = 2^-52 (the issue's; twice the unit roundoff), the gate twice that for the second-order terms:
    a weighted sum of x:   B(x) = (D + 8) u sum_s w_s |x_s|  -- D - 1 additions in any order, plus the rounded exp and products of a term
    mean:                  |d mean| <= B(resid) + u |y|                      (without y: B(m))
    sd^2:                  |d sd^2| <= B(var + m^2) + 2 |mean| |d mean| + u mean^2;   |d sd| = |d sd^2| / (2 sd), absolute
    pit and F:             per term (a^2 + 4) u of the term with a = |z| / sqrt 2 (the erfc allowance of the Rao-Blackwellised edge summaries'
                           tests, reused), plus B(Phi);  a point mass is exact and is charged nothing per term
The sd bound divides by sd: the cases keep sd^2 >= 1e-6 sum w (var + m^2) (asserted about the inputs, SD_FLOOR), so that the cancellation in
sd^2 costs at most 1e6 of the relative accuracy.
A quantile t is checked by its residual: F(t - h) - eps_F <= p <= F(t + h) + eps_F with h = 2^-40 of the bracket and eps_F the gate times the
bound of F at that point.

Two shortcuts, both charged to the bound: a term whose log weight is below -700 (w < 1e-304; float64's exp underflows below -745) is left out
of every sum and its weight times the largest |x| is added (for F: its weight); a component more than 12 sd away from t contributes its limit 0 or
1 to F (off by less than 1e-32 of its weight, added as 1e-32).
"""
import functools
import math

import mpmath as mp
import numpy as np

import mloo_ref as mr

DPS = mr.DPS
U = 2.0 ** -52
GATE = 2.0
SD_FLOOR = 1e-6
PATTERNS = ("uniform", "random", "onehot", "points", "nanrow")
CASE_ROWS = 5


def _mpf(a):
    return [mp.mpf(float(x)) for x in np.asarray(a, dtype=np.float64).reshape(-1)]


def bracket_c(p_lo, p_hi):
    """the library's half-width of the bracket in sds: the first of 1, 1.5, 2, ... with Phi(-c) < min(p_lo, 1 - p_hi) / 2, found in mpmath"""
    with mp.workdps(DPS):
        pm = min(mp.mpf(p_lo), 1 - mp.mpf(p_hi)) / 2
        c = mp.mpf(1)
        while not mp.erfc(c / mp.sqrt(2)) / 2 < pm and c < 40:
            c += mp.mpf(1) / 2
        return float(c)


class Row:
    """one row of a case in mpmath: the kept terms (w, m, var) and what the dropped ones (lw < -700) are charged"""

    def __init__(self, mean, var, logw, y=None):
        with mp.workdps(DPS):
            m, v, lw = _mpf(mean), _mpf(var), np.asarray(logw, dtype=np.float64).reshape(-1)
            self.D = len(m)
            self.y = None if y is None else mp.mpf(float(y))
            keep = [s for s in range(self.D) if lw[s] >= -700.0]
            self.dropped = mp.fsum(mp.exp(mp.mpf(float(lw[s]))) for s in range(self.D) if lw[s] < -700.0)
            self.w = [mp.exp(mp.mpf(float(lw[s]))) for s in keep]
            self.m = [m[s] for s in keep]
            self.v = [v[s] for s in keep]
            self.s2 = [mp.sqrt(2 * x) for x in self.v]               # sqrt(2 var): z / sqrt 2 = (t - m) / s2
            self.mag = max([abs(x) for x in m] + [abs(self.y) if self.y is not None else 0])
            self.vmag = max(abs(a) + b * b for a, b in zip(v, m))

    def B(self, xs, big):
        """(D + 8) u sum w |x| over the kept terms, plus the dropped weight times the largest |x|"""
        return (self.D + 8) * U * mp.fsum(w * abs(x) for w, x in zip(self.w, xs)) + self.dropped * big

    def moments(self):
        """dict of mean, sd (float64), tol_mean, tol_sd, and e2 = sum w (var + m^2), sd2 (float64, for the SD_FLOOR assertion)"""
        with mp.workdps(DPS):
            if self.y is not None:
                r = [self.y - m for m in self.m]
                mean = self.y - mp.fsum(w * x for w, x in zip(self.w, r))
                tol_mean = self.B(r, 2 * self.mag) + U * abs(self.y)
            else:
                mean = mp.fsum(w * m for w, m in zip(self.w, self.m))
                tol_mean = self.B(self.m, self.mag)
            x2 = [v + m * m for v, m in zip(self.v, self.m)]
            e2 = mp.fsum(w * x for w, x in zip(self.w, x2))
            sd2 = e2 - mean * mean
            tol_sd2 = self.B(x2, self.vmag) + 2 * abs(mean) * tol_mean + U * mean * mean
            sd = mp.sqrt(max(sd2, 0))
            tol_sd = tol_sd2 / (2 * sd) if sd > 0 else mp.inf
            return dict(mean=float(mean), sd=float(sd), tol_mean=float(tol_mean), tol_sd=float(tol_sd), e2=float(e2), sd2=float(sd2))

    def cdf(self, t):
        """(F(t), its first-order bound) as mpf"""
        with mp.workdps(DPS):
            t = mp.mpf(float(t)) if not isinstance(t, mp.mpf) else t
            F, per = mp.mpf(0), mp.mpf(0)
            for w, m, s2 in zip(self.w, self.m, self.s2):
                d = t - m
                if s2 == 0:
                    F += w if d >= 0 else 0
                elif abs(d) > mp.mpf("8.5") * s2:
                    F += w if d > 0 else 0
                    per += w * mp.mpf("1e-32")
                else:
                    a = d / s2
                    ph = mp.erfc(-a) / 2
                    F += w * ph
                    per += (a * a + 4) * U * w * ph
            return F, per + (self.D + 8) * U * F + self.dropped

    def pit(self):
        """(pit, its bound) as floats"""
        F, tol = self.cdf(self.y)
        return float(F), float(tol)


def bracket_width(mean, var, c):
    """the width of the library's bracket [min (m - c sd), max (m + c sd)] of one row, in float64 (it only scales h)"""
    m, sd = np.asarray(mean, dtype=np.float64), np.sqrt(np.asarray(var, dtype=np.float64))
    return float(np.max(m + c * sd) - np.min(m - c * sd))


def quantile_ok(row, t, p, width):
    """the residual check of a quantile t of `row` (a Row) at probability p: F(t - h) - eps <= p <= F(t + h) + eps, h = 2^-40 width; returns
    (ok, the larger of the two violations over its allowance: <= 0 where the inequality holds without the allowance)"""
    with mp.workdps(DPS):
        if width == 0:
            return t == float(row.m[0]), 0.0
        h = mp.mpf(width) * mp.mpf(2) ** -40
        Fa, ea = row.cdf(mp.mpf(float(t)) - h)
        Fb, eb = row.cdf(mp.mpf(float(t)) + h)
        p = mp.mpf(p)
        ok = Fa - GATE * ea <= p <= Fb + GATE * eb
        worst = max((Fa - p) / (GATE * ea) if ea > 0 else 0, (p - Fb) / (GATE * eb) if eb > 0 else 0)
        return bool(ok), float(worst)


# ------------------------------------------------------------------------------------------ the shared cases
@functools.lru_cache(maxsize=None)
def case(D, pattern):
    """CASE_ROWS rows of D draws: dict of mean, var, logw (CASE_ROWS x D), y (CASE_ROWS,) and nan_rows (the rows that have to come out NaN).
    uniform: lw = -log D; random: normalised random weights spread over six decades; onehot: one draw with lw = 0 (a different one per row),
    the others -800 (they underflow to 0); points: the random case with every third draw of a row (from the row's number on) a point mass,
    var = 0; nanrow: the random case with row 1 spoilt (a NaN var, or for D = 1 the only one).  Rows 0 .. k - 1 of a case are the case of k
    rows: no output of a row depends on the others."""
    assert pattern in PATTERNS
    rng = np.random.default_rng([186, D])
    mean = rng.normal(size=(CASE_ROWS, D)) * 2.0 + rng.normal(size=(CASE_ROWS, 1))
    var = rng.exponential(size=(CASE_ROWS, D)) + 0.01
    y = rng.normal(size=CASE_ROWS) * 2.0
    raw = rng.normal(size=(CASE_ROWS, D)) * 2.3
    logw = raw - np.log(np.sum(np.exp(raw), axis=1, keepdims=True))
    nan_rows = ()
    if pattern == "uniform":
        logw = np.full((CASE_ROWS, D), -math.log(D))
    elif pattern == "onehot":
        logw = np.full((CASE_ROWS, D), -800.0)
        for i in range(CASE_ROWS):
            logw[i, (7 * i + 3) % D] = 0.0
    elif pattern == "points":
        var = var.copy()
        for i in range(CASE_ROWS):
            var[i, i % 3::3] = 0.0
    elif pattern == "nanrow":
        var = var.copy()
        var[1, D // 2] = np.nan
        nan_rows = (1,)
    for a in (mean, var, logw, y):
        a.setflags(write=False)
    return dict(mean=mean, var=var, logw=logw, y=y, nan_rows=nan_rows)


def ref_pattern(pattern):
    """the pattern whose rows are the reference of `pattern`'s rows that are not NaN (nanrow: the random case, untouched beside row 1)"""
    return "random" if pattern == "nanrow" else pattern


@functools.lru_cache(maxsize=None)
def case_row(D, pattern, i, with_y=True):
    c = case(D, ref_pattern(pattern))
    return Row(c["mean"][i], c["var"][i], c["logw"][i], c["y"][i] if with_y else None)


@functools.lru_cache(maxsize=None)
def case_moments(D, pattern, i, with_y=True):
    return case_row(D, pattern, i, with_y).moments()


@functools.lru_cache(maxsize=None)
def case_pit(D, pattern, i):
    return case_row(D, pattern, i).pit()


@functools.lru_cache(maxsize=None)
def case_quantile_ok(D, pattern, i, t, p, width):
    return quantile_ok(case_row(D, pattern, i), t, p, width)


def check_case(D, pattern, rows, got, p_lo, p_hi, with_y=True):
    """the five outputs `got` (dict of mean, sd, pit, lower, upper; rows values each) of the first `rows` rows of case(D, pattern) against the
    reference: the largest |error| / bound met per output (every one asserted <= GATE), the quantiles by their residual"""
    c = case(D, pattern)
    cw = bracket_c(p_lo, p_hi)
    worst = dict(mean=0.0, sd=0.0, pit=0.0, quantile=0.0)
    for i in range(rows):
        if i in c["nan_rows"]:
            assert all(math.isnan(got[k][i]) for k in ("mean", "sd", "lower", "upper")) and (not with_y or math.isnan(got["pit"][i])), (D, pattern, i)
            continue
        mo = case_moments(D, pattern, i, with_y)
        single_point = D == 1 and c["var"][i, 0] == 0.0
        if not single_point:
            assert mo["sd2"] >= SD_FLOOR * mo["e2"], ("the case breaks the sd floor", D, pattern, i)      # (about the inputs)
        for k in ("mean", "sd"):
            if k == "sd" and single_point:
                assert got["sd"][i] == 0.0
                continue
            r = abs(got[k][i] - mo[k]) / mo["tol_" + k]
            assert math.isfinite(got[k][i]) and r <= GATE, (D, pattern, i, k, got[k][i], mo[k], r)
            worst[k] = max(worst[k], r)
        if with_y:
            ref, tol = case_pit(D, pattern, i)
            r = abs(got["pit"][i] - ref) / tol if tol > 0 else (0.0 if got["pit"][i] == ref else math.inf)
            assert r <= GATE, (D, pattern, i, "pit", got["pit"][i], ref, r)
            worst["pit"] = max(worst["pit"], r)
        width = bracket_width(c["mean"][i], c["var"][i], cw)
        for k, p in (("lower", p_lo), ("upper", p_hi)):
            ok, viol = case_quantile_ok(D, pattern, i, float(got[k][i]), p, width)
            assert ok, (D, pattern, i, k, got[k][i], viol)
            worst["quantile"] = max(worst["quantile"], viol)
    return worst


def numpy_bounds(mean, var, logw, y=None):
    """the first-order bounds of mean, sd and pit (rows,) of a rows x D case with every quantity taken from a float64 evaluation instead of
    mpmath (for shapes where mpmath is too slow: the comparison of two float64 evaluations against each other, each within its own gate)"""
    m, v, lw = (np.asarray(a, dtype=np.float64) for a in (mean, var, logw))
    D = m.shape[1]
    w = np.exp(lw)
    k = (D + 8) * U
    with np.errstate(all="ignore"):
        if y is not None:
            yv = np.asarray(y, dtype=np.float64).reshape(-1)
            r = yv[:, None] - m
            mu = yv - np.sum(w * r, axis=1)
            tol_mean = k * np.sum(w * np.abs(r), axis=1) + U * np.abs(yv)
        else:
            mu = np.sum(w * m, axis=1)
            tol_mean = k * np.sum(w * np.abs(m), axis=1)
        e2 = np.sum(w * (v + m * m), axis=1)
        sd = np.sqrt(np.fmax(e2 - mu * mu, 0.0))
        tol_sd = (k * e2 + 2 * np.abs(mu) * tol_mean + U * mu * mu) / (2 * sd)
        out = dict(tol_mean=tol_mean, tol_sd=tol_sd, sd2=sd * sd, e2=e2)
        if y is not None:
            z = r / np.sqrt(v)
            ph = np.where(v == 0, (r >= 0).astype(np.float64), 0.5 * np.vectorize(math.erfc)(-z / math.sqrt(2.0)))
            a2 = np.where(v == 0, -4.0, 0.5 * z * z)
            out["tol_pit"] = U * np.sum(w * (a2 + 4) * ph, axis=1) + k * np.sum(w * ph, axis=1)
    return out


def numpy_cdf(t, mean, var, logw):
    """(F(t), its first-order bound) of one row from a float64 evaluation (see numpy_bounds)"""
    m, v, lw = (np.asarray(a, dtype=np.float64).reshape(-1) for a in (mean, var, logw))
    w = np.exp(lw)
    with np.errstate(all="ignore"):
        z = (t - m) / np.sqrt(v)
        ph = np.where(v == 0, (t >= m).astype(np.float64), 0.5 * np.vectorize(math.erfc)(-z / math.sqrt(2.0)))
        a2 = np.where(v == 0, -4.0, 0.5 * z * z)
    F = float(np.sum(w * ph))
    return F, U * float(np.sum(w * (a2 + 4) * ph)) + (m.size + 8) * U * F
