"""Phi^-1 by mpmath at 40 digits, a yardstick that shares no code with bnr_ndtri (Wichura's AS 241) or with scipy's Cephes routine: Newton's
iteration z <- z - (Phi(z) - p) / phi(z) on mpmath's ncdf, for tests/test_sort_edges_host.py and tests/test_sort_edges_gpu.py.

The start is scipy's double, which only saves iterations: the fixed point is the root of mpmath's own ncdf.  A step dz from a point within
|dz| of the root leaves an error of about |z| dz^2 / 2 (Newton on a function with Phi'' / Phi' = -z), so the iteration stops behind the first
step with |dz| <= 1e-12 |z|: the result is then good to about 1e-22 relative, six digits more than the 1e-16 errors it measures."""
import mpmath as mp
import numpy as np
from scipy.special import ndtri

DPS = 40
E_AS = 7.29e-16         # the largest relative error of bnr_host_ndtri (AS 241) against phi_inv, measured by tests/test_sort_edges_host.py
DEVICE_ULPS = 16.0      # what tests/test_rank_diag_gpu.py grants the device's log and sqrt against the host's: 4 x K_PHI


def phi_inv(p):
    """Phi^-1(p) as an mpf, p a double in (0, 1) taken exactly"""
    with mp.workdps(DPS):
        pm = mp.mpf(float(p))
        z = mp.mpf(float(ndtri(float(p))))
        for _ in range(8):
            dz = (mp.ncdf(z) - pm) / mp.npdf(z)
            z -= dz
            if abs(dz) <= mp.mpf("1e-12") * abs(z) or z == 0:
                return z
    raise ArithmeticError("Newton's iteration for Phi^-1(%r) did not settle" % p)


def rel_errors(p, z):
    """|z_i - Phi^-1(p_i)| / |Phi^-1(p_i)| as doubles (0 where both are 0)"""
    out = np.zeros(len(p))
    with mp.workdps(DPS):
        for i, (pi, zi) in enumerate(zip(np.asarray(p, dtype=np.float64).tolist(), np.asarray(z, dtype=np.float64).tolist())):
            ref = phi_inv(pi)
            out[i] = float(abs(mp.mpf(zi) - ref) / abs(ref)) if ref != 0 else (0.0 if zi == 0.0 else np.inf)
    return out


def bound_ratios(p, z, e_as, ulps):
    """|z_i - Phi^-1(p_i)| over the allowance 2 e_as |ref| + ulps spacing(ref)"""
    out = np.zeros(len(p))
    with mp.workdps(DPS):
        for i, (pi, zi) in enumerate(zip(np.asarray(p, dtype=np.float64).tolist(), np.asarray(z, dtype=np.float64).tolist())):
            ref = phi_inv(pi)
            allow = 2.0 * e_as * abs(ref) + ulps * mp.mpf(float(np.spacing(abs(float(ref)))))
            out[i] = float(abs(mp.mpf(zi) - ref) / allow) if allow != 0 else (0.0 if zi == 0.0 else np.inf)
    return out
