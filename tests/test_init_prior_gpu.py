"""GPU test of k_init_prior against the independent reference of tests/rng_ref.py (run with -m gpu on an MI355X): the prior row of
initialize_variables! (gibbs.jl:191-224), every column within its a-priori bound of the device's float64 error.  The kernel writes variates
into the table raw -- u is R V normals, S is q logarithms, xi is V coins -- so this is also the direct check of the device's Philox, unit
map, log, sin / cos, sqrt and pow against LIBM_ULPS, and of its Gamma sampler, Dirichlet rows, Bartlett factor, triangular inverse, T' T and
edge_W.  One launch of one workgroup per chain; the reference of a case is computed once (rng_ref.init_ref caches it) and shared with
tests/test_rng_ref_host.py, which holds the oracle's prior row to it on the CPU and requires that no decision of these cases is too close to call.

Cases (V, R, nu, eta), n = 8 (the prior row does not depend on X and y): rng_ref.CASES -- the smallest, with the eta reset and the boost path
of the Gamma sampler (shape 1/2); the reference's defaults; V = 65; 3 R = 96 Gamma lanes and R^2 = 1024 > 256 threads, shapes from 1024 down
to 1/2; q = 180 300 with R V = 19 200, every loop of the kernel wrapping many times.

Largest error / bound per column over the five cases and both chains, measured on an MI355X (pytest -s prints them):
    device:  S 0.375 (1.1 u of the value), pi 0.153, M 0.066, u 0.523 (3.7 u), gamma 0.134; no decision too close to call, no sampler cap
    oracle (tests/test_rng_ref_host.py, CPU, glibc):  S 0.334 (1.0 u), pi 0.153, M 0.066, u 0.523 (3.7 u), gamma 0.134
so the device's log stays within 1.1 of the LIBM_ULPS = 2 u it is allowed, its normals within 3.7 of the 7 u that follow from LIBM_ULPS (the
VARIATE_ULPS = 8 the stage references assume), and pow, sqrt and the Gamma sampler inside the propagated bounds of pi and M.
bench.py --gpus 1 --steps 2000 --warmup 200, three runs each, alternating: parent 23 027 / 23 095 / 23 099 it/s, with bnr_unit's clamp
23 061 / 23 053 / 22 977 -- the median 23 053 inside the parent's spread."""
import numpy as np
import pytest

import bnr_amd
import rng_ref as rr
from oracle import bnr_oracle as bo
from test_sweep_stages_gpu import SKIP_FRACTION

pytestmark = pytest.mark.gpu

WORST = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    print("\nprior row on the device, largest error/bound ([u]: in rounding units of the value):", {k: "%.3g" % v for k, v in sorted(WORST.items())})


def _bits(t, j):
    return {k: np.ascontiguousarray(t[k][j]).view(np.uint64).copy() for k in bo.COLUMNS}


def _check(ch, key, V, R, nu, eta, what):
    ref = rr.init_ref(V, R, eta, nu, key)
    t = ch.fetch()
    got = {k: t[k][0] for k in bo.COLUMNS}
    worst, checked, skipped = rr.check_init(got, ref)
    units = rr.raw_units(got, ref)
    print("\n%s V=%d R=%d nu=%g eta=%g, largest error/bound:" % (what, V, R, nu, eta), {k: "%.3g" % v for k, v in worst.items() if k not in rr.EQUAL},
          "; in u of the value:", {k: "%.2f" % v for k, v in units.items()},
          "; %d of %d lambda / pi / chi decisions too close to call" % (skipped, checked))
    for k, v in list(worst.items()) + [(k + " [u]", v) for k, v in units.items()]:
        WORST[k] = max(WORST.get(k, 0.0), v)
    assert max(worst.values()) <= 1.0, worst
    assert skipped <= SKIP_FRACTION * checked, (skipped, checked)
    assert ch.counters()["sampler_cap"] == 0 and ch.iter == 1
    return t


@pytest.mark.parametrize("case", range(len(rr.CASES)))
def test_prior_row_matches_the_independent_reference(gpu, case):
    V, R, nu, eta = rr.CASES[case]
    seed = rr.case_seed(case)
    q = V * (V + 1) // 2
    rng = np.random.default_rng(100 + case)
    X, y = rng.standard_normal((8, q)), rng.standard_normal(8)
    ch = bnr_amd.Chain(X, y, R, 3, seed, rr.CHAIN_ID, device=0, nu=nu, eta=eta)
    # a table loaded beforehand: the launch writes row 1 and nothing else
    before = ch.fetch()
    for k in bo.COLUMNS:
        before[k][...] = rng.standard_normal(before[k].shape)
    ch.load(before)
    ch.init_prior()
    t = _check(ch, (seed + rr.CHAIN_ID) % 2 ** 64, V, R, nu, eta, "chain %d" % rr.CHAIN_ID)
    for j in (1, 2):
        for k in bo.COLUMNS:
            assert np.array_equal(_bits(t, j)[k], _bits(before, j)[k]), ("row %d changed" % (j + 1), k)
    # again: the same bits
    ch.init_prior()
    t2 = ch.fetch()
    for j in range(3):
        for k in bo.COLUMNS:
            assert np.array_equal(_bits(t2, j)[k], _bits(t, j)[k]), ("second init_prior, row %d" % (j + 1), k)
    assert ch.counters()["sampler_cap"] == 0 and ch.iter == 1
    # another chain of the fit: its key is seed + chain id, the sum carrying into the key's high word
    assert (seed + rr.LIKE_ID) >> 32 == (seed >> 32) + 1
    like = bnr_amd.Chain.like(ch, seed, rr.LIKE_ID)
    like.init_prior()
    _check(like, (seed + rr.LIKE_ID) % 2 ** 64, V, R, nu, eta, "chain %d (create_like)" % rr.LIKE_ID)
    like.close()
    ch.close()
