"""CPU tests of bnr_host_gig_attempts (ABI 14): the index of the rejection attempt that the GIG draw of update_D! (gibbs.jl:454-458, gig.jl) accepts.  It must be the loop of
bnr_host_gig: replaying the attempts 0 ... k of a draw in Python -- the variates of counter {it, 21 (SITE_D_GIG), elem, attempt} from bnr_host_uniform2 through the
acceptance tests of gig.jl for lambda = 1/2 -- refuses every attempt below the reported index, accepts that one, and gives bnr_host_gig's value."""
import ctypes as C
import math
import os
import re

import numpy as np

import bnr_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SITE_D_GIG = 21
MAX_ATTEMPTS = 100000


def _mode(omega):                                   # gig.jl:170-176 for lambda = 1/2
    return omega / (math.sqrt(0.25 + omega * omega) + 0.5)


def _replay(L, seed, chi, psi, it, elem, upto):
    """(index of the first accepted attempt among 0 ... upto or None, its value, the sampler) of GIG(1/2, chi, psi), restated from gig.jl"""
    lam = 0.5
    alpha, omega = math.sqrt(chi / psi), math.sqrt(psi * chi)
    u2 = (C.c_double * 2)()
    if omega > 0.2:                                 # gig.jl:27-33 with lambda = 1/2: ratio of uniforms, shifted by the mode for omega > 3
        t, s = 0.5 * (lam - 1.0), 0.25 * omega
        xm = _mode(omega)
        nc = t * math.log(xm) - s * (xm + 1.0 / xm)
        if omega > 3.0:
            a = -(2.0 * (lam + 1.0) / omega + xm)
            b = 2.0 * (lam - 1.0) * xm / omega - 1.0
            p = b - a * a / 3.0
            qq = 2.0 * a * a * a / 27.0 - a * b / 3.0 + xm
            fi = math.acos(-qq / (2.0 * math.sqrt(-p * p * p / 27.0)))
            fak = 2.0 * math.sqrt(-p / 3.0)
            y1 = fak * math.cos(fi / 3.0) - a / 3.0
            y2 = fak * math.cos(fi / 3.0 + 4.0 / 3.0 * math.pi) - a / 3.0
            uhi = (y1 - xm) * math.exp(t * math.log(y1) - s * (y1 + 1.0 / y1) - nc)
            ulo = (y2 - xm) * math.exp(t * math.log(y2) - s * (y2 + 1.0 / y2) - nc)
            xoff = xm
        else:
            ym = ((lam + 1.0) + math.sqrt((lam + 1.0) * (lam + 1.0) + omega * omega)) / omega
            uhi = math.exp(0.5 * (lam + 1.0) * math.log(ym) - s * (ym + 1.0 / ym) - nc)
            ulo, xoff = 0.0, 0.0
        for k in range(upto + 1):
            L.bnr_host_uniform2(seed, it, SITE_D_GIG, elem, k, u2)
            ru, rv = u2[0], u2[1]
            X = (ulo + ru * (uhi - ulo)) / rv + xoff
            if X > 0.0 and math.log(rv) <= t * math.log(X) - s * (X + 1.0 / X) - nc:
                return k, alpha * X, 2
        return None, None, 2
    # gig_concave, gig.jl:102-168, lambda = 1/2
    xm = _mode(omega)
    x0 = omega / (1.0 - lam)
    k0 = math.exp((lam - 1.0) * math.log(xm) - 0.5 * omega * (xm + 1.0 / xm))
    A0 = k0 * x0
    x0l = math.sqrt(x0)
    if x0 >= 2.0 / omega:
        k1, A1 = 0.0, 0.0
        k2 = 1.0 / x0l
        A2 = k2 * 2.0 * math.exp(-omega * x0 / 2.0) / omega
    else:
        k1 = math.exp(-omega)
        twl = math.sqrt(2.0 / omega)
        A1 = k1 / lam * (twl - x0l)
        k2 = 1.0 / twl
        A2 = k2 * 2.0 * math.exp(-1.0) / omega
    Atot = A0 + A1 + A2
    for k in range(upto + 1):
        L.bnr_host_uniform2(seed, it, SITE_D_GIG, elem, k, u2)
        ru, rv = u2[0], u2[1]
        Vv = Atot * ru
        if Vv <= A0:
            X, hx = x0 * Vv / A0, k0
        else:
            Vv -= A0
            if Vv <= A1:
                r = x0l + (lam / k1 * Vv)
                X, hx = r * r, k1 / r
            else:
                Vv -= A1
                a = x0 if x0 > 2.0 / omega else 2.0 / omega
                X = -2.0 / omega * math.log(math.exp(-omega / 2.0 * a) - omega / (2.0 * k2) * Vv)
                hx = k2 * math.exp(-omega / 2.0 * X)
        if math.log(rv * hx) <= (lam - 1.0) * math.log(X) - omega / 2.0 * (X + 1.0 / X):
            return k, alpha * X, 3
    return None, None, 3


def test_abi_14_declares_the_helper():
    hdr = open(os.path.join(ROOT, "include", "bnr_hip.h")).read()
    assert int(re.search(r"#define BNR_ABI_VERSION (\d+)", hdr).group(1)) >= 14 and bnr_amd.lib().bnr_abi_version() >= 14
    assert "bnr_host_gig_attempts" in hdr and "bnr_host_gig_attempts" in bnr_amd.EXPORTS


def test_accepted_attempt_is_the_one_bnr_host_gig_takes():
    L = bnr_amd.lib()
    rng = np.random.default_rng(14)
    seed, seen, deepest = 90210, {2: 0, 3: 0}, 0
    for e in range(600):
        # omega = sqrt(chi psi) on both sides of 0.2 (concave below, ratio of uniforms above) and of 3 (shifted ratio of uniforms)
        omega, alpha = 10 ** rng.uniform(-4, 1.5), 10 ** rng.uniform(-3, 3)
        chi, psi = omega * alpha, omega / alpha
        it = 2 + e % 7
        k = L.bnr_host_gig_attempts(seed, 0.5, chi, psi, it, e)
        assert 0 <= k < MAX_ATTEMPTS
        got, val, kind = _replay(L, seed, chi, psi, it, e, k)
        assert got == k, (e, chi, psi, k, got)                      # every attempt below k refused, attempt k accepted
        want = L.bnr_host_gig(seed, 0.5, chi, psi, it, e)
        assert abs(val - want) <= 1e-12 * abs(want), (e, val, want)
        assert kind == (2 if math.sqrt(psi * chi) > 0.2 else 3)
        seen[kind] += 1
        deepest = max(deepest, k)
    assert min(seen.values()) > 100 and deepest >= 4, (seen, deepest)


def test_draws_without_a_rejection_loop_report_minus_one():
    L = bnr_amd.lib()
    assert L.bnr_host_gig_attempts(5, 0.5, 0.0, 1.0, 3, 0) == -1         # chi ~ 0: Gamma (gig.jl:14-20)
    assert L.bnr_host_gig_attempts(5, 0.5, 1.0, 1e-300, 3, 0) == -1      # psi ~ 0: inverse Gamma (gig.jl:21-26)
    assert L.bnr_host_gig_attempts(5, 0.5, float("nan"), 1.0, 3, 0) == -1
