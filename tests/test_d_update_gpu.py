"""GPU tests of update_D! -- S_e ~ GIG(1/2, chi_e = (gamma_e - W_e)^2 / tau2, psi = theta_prev), the draw of k_backproj -- against the
extended-precision reference of tests/gig_ref.py (run with -m gpu on an MI355X): on every edge whose decisions (kind, region of the hat,
accept / reject of every attempt) are decided, |S_dev - S*| <= the a-priori bound of the device's float64 error, which also pins the accepted
attempt; the undecided edges are counted and must stay few, and for omega in [1e-8, 3e3] a bound is below 1e-10 S* or the edge counts as
skipped too.

The hook update("D", 2, IT) runs the X pass (W) and k_backproj with flags = 2 on crafted rows (gig_ref.craft_D): omega log-uniform over
[1e-8, 3e3], a tenth of the edges up to 1e8, both sides of 0.2, 3 and chi = 10 eps, chi = 0, |W| up to 10 |gamma - W|; a second load with
theta_prev = 1e-300 sends every edge with chi >= 10 eps through the inverse-Gamma draw.  The largest error / bound per kind is printed (pytest -s)."""
import ctypes as C
import glob

import numpy as np
import pytest

import bnr_amd
import gig_ref as gr
import sweep_ref as sr
from oracle import bnr_oracle as bo
from test_backproj_packed_retry_gpu import _draw_inputs, _kinds

pytestmark = pytest.mark.gpu
IT = 2
SKIP_FRACTION = 0.05          # as tests/test_sweep_stages_gpu.py

WORST = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    print("\nupdate_D, largest error/bound:", {k: "%.3g" % v for k, v in sorted(WORST.items())})


def _kfd_compute_units():
    """the compute units of the GPU nodes as the kernel driver lists them (simd_count / simd_per_cu of the KFD topology)"""
    out = set()
    for f in glob.glob("/sys/class/kfd/kfd/topology/nodes/*/properties"):
        try:
            p = dict(ln.split()[:2] for ln in open(f) if len(ln.split()) >= 2)
        except OSError:
            continue
        if int(p.get("simd_count", 0)) > 0 and int(p.get("simd_per_cu", 0)) > 0:
            out.add(int(p["simd_count"]) // int(p["simd_per_cu"]))
    return out


def _compute_units(device=0):
    """the device property launch_backproj sizes its launch by (multiProcessorCount), asked of the HIP runtime the library is bound to.  The
    attribute is named by its number in hip_runtime_api.h, so the answer is held against the driver's own count: a number that meant another
    attribute would not pass for a CU count"""
    bnr_amd.lib()
    path = sorted({ln.split()[-1] for ln in open("/proc/self/maps") if "libamdhip64" in ln})[0]
    v = C.c_int(0)
    rc = C.CDLL(path).hipDeviceGetAttribute(C.byref(v), 63, device)          # hipDeviceAttributeMultiprocessorCount
    assert rc == 0, rc
    kfd = _kfd_compute_units()
    assert 16 <= v.value <= 1024 and v.value % 4 == 0 and (not kfd or v.value in kfd), (v.value, kfd)
    return v.value


def _row(t, j):
    return {k: t[k][j] for k in bo.COLUMNS}


def _check(ch, t, V, var, what):
    """one update_D! of row 2 from the loaded table t: the kinds of the fetched row"""
    ch.load(t)
    ch.update("D", 2, IT)
    g = ch.fetch()
    for k in bo.COLUMNS:
        if k != "S":
            assert np.array_equal(g[k][:2], t[k][:2]), k                    # the hook writes S of row 2 and nothing else
    assert np.array_equal(g["S"][0], t["S"][0])
    ref = gr.S_ref(_row(t, 0), _row(t, 1), V, var, IT)
    worst, skipped, bad = gr.check_S(g["S"][1], ref)
    q = ref["S"].size
    print("%s: %s, %d of %d edges skipped" % (what, {k: "%.3g" % v for k, v in worst.items()}, skipped, q))
    assert bad == 0, (what, bad)
    for k, v in worst.items():
        WORST[k] = max(WORST.get(k, 0.0), v)
        assert v <= 1.0, (what, k, v)
    assert skipped <= SKIP_FRACTION * q, (what, skipped, q)                  # (none of 3 edges, at most 3 of 66)
    assert ch.counters()["sampler_cap"] == 0
    return _kinds(*_draw_inputs(g, 1, V))


# n, V, R, theta_prev, kinds the grid is built for, more than two workgroups per compute unit
#   (12, 2, 1): 3 edges, one partial workgroup; (12, 11, 2): 66 edges, 32 + 32 + 2; at theta_prev = 2.3 omega < 7e-8 is chi < 10 eps: the Gamma draw
#   (8, 200, 2): 629 workgroups of 32 edges, more than twice the compute units: launch_backproj passes nslot = 2 -- one drawing wave, both samplers back to
#   back, the drawing wave rotating with the workgroup
CASES = [(12, 2, 1, 0.01, {2, 3}, False), (12, 11, 2, 2.3, {0, 2, 3}, False), (8, 23, 11, 0.01, {0, 2, 3}, False), (8, 200, 2, 0.01, {0, 2, 3}, True)]


@pytest.mark.parametrize("n,V,R,theta,kinds,many", CASES)
def test_update_D_on_crafted_rows_matches_the_reference(gpu, n, V, R, theta, kinds, many):
    q = V * (V + 1) // 2
    if many:
        ncu = _compute_units()
        assert 0 < ncu and (q + 31) // 32 > 2 * ncu, (q, ncu)
    X, y, _ = bnr_amd.make_synthetic(n, V, R, seed=V + 7 * R)
    seed = 700 + V
    ch = bnr_amd.Chain(X, y, R, 3, seed, 1, device=0, nu=max(10, R + 2))
    var = sr.Variates(bnr_amd.lib(), seed + 1)
    ch.init_prior()
    t = ch.fetch()
    info = gr.craft_D(t, V, R, 5 + V, theta)
    with np.errstate(divide="ignore"):
        built = _kinds(info["omega"] ** 2 / theta, theta)
    got = _check(ch, t, V, var, "n=%d V=%d R=%d" % (n, V, R))
    assert np.array_equal(got, built) and set(got.tolist()) == kinds, (np.bincount(got), np.bincount(built))
    if q > 3:
        assert (info["omega"][got == 2] > 3.0).any() and (info["omega"][got == 2] <= 3.0).any()          # the ratio of uniforms with and without the shift
    t["theta"][0] = 1e-300
    got = _check(ch, t, V, var, "n=%d V=%d R=%d, theta_prev = 1e-300" % (n, V, R))
    assert np.array_equal(got, np.where(built == 0, 0, 1)), np.bincount(got)
    ch.close()
