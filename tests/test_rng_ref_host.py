"""CPU tests of the draw-site variates against the independent reference of tests/rng_ref.py: Philox-4x32-10 (Random123's known answers; random
counters), the word-to-uniform map, the normal and the Gamma sampler of the library's host copy (bnr_host_*), their distributions, and the
oracle's prior row against init_ref -- the reference that tests/test_init_prior_gpu.py holds the device to.  Every comparison is shown to have
power: the same check with a mutated reference (swapped multipliers, nine rounds, no key bump, d = a - 0.3, boost exponent a, reversed
acceptance, cosine without the quadrant's sign) must fail.

The finding: before bnr_unit, the uniform of a word whose top 53 bits are all ones was ((2^53 - 1) + 1/2) 2^-53, which float64 rounds to 1.0 --
outside the documented open interval, and log(1) = 0 makes an initial S_e zero.  test_unit_map_is_the_exact_grid_and_open asserts 0 < u < 1 on
that word; it fails on the bare formula (asserted there too, on the reference's clamp=False) and passes with bnr_unit, which changes no other
word.

Measured here with glibc (pytest -s prints them; u = 2^-53): bnr_host_normal at most 4.0 of its 7 u on 1e5 draws; the long-double normal within
2^-62.6 of mpmath; bnr_host_gamma at most 0.34 of its propagated bound -- errors of 5 to 86 u of the value, the large ones where 1 + c x is
small, which the propagation covers and a flat budget would not --, the reference's accepted attempt (at most the third) on all 18 000 draws,
none skipped; KS p-values 0.21 ... 0.89; the oracle's prior row at most 0.52 of its bound (u: 3.7 u; S: 1.0 u; pi 0.15, M 0.066, gamma 0.13).
"""
import ctypes as C

import numpy as np
import pytest
from scipy import stats

import bnr_amd
import rng_ref as rr
from oracle import bnr_oracle as bo
from sweep_ref import LD, U, f64
from test_oracle_golden import P_MIN

KAT = [      # Random123 kat_vectors, philox4x32 10: counter, key, expected
    ([0, 0, 0, 0], [0, 0], [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]),
    ([0xffffffff] * 4, [0xffffffff] * 2, [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]),
    ([0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344], [0xa4093822, 0x299f31d0], [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1]),
]
PHILOX_MUTATIONS = [dict(swap_multipliers=True), dict(rounds=9), dict(bump_key=False)]
GAMMA_SHAPES = [0.05, 0.5, 1.0, 2.5, 130.5, 2e4]
SEED, IT, SITE = 77, 1, 5


def _lib_philox(L, c, k):
    out = (C.c_uint32 * 4)()
    L.bnr_host_philox((C.c_uint32 * 4)(*c), (C.c_uint32 * 2)(*k), out)
    return list(out)


def test_philox_known_answers():
    L = bnr_amd.lib()
    for c, k, want in KAT:
        assert [int(v) for v in rr.philox4x32(c, k)] == want
        assert _lib_philox(L, c, k) == want
        assert bo.philox(c, k) == want
        for mut in PHILOX_MUTATIONS:
            assert [int(v) for v in rr.philox4x32(c, k, **mut)] != want, mut


def _random_counters(n):
    """it, site, elem, att, seed, chain id: the edges of the 32-bit fields, seeds with the high word set, seed + chain id carrying into it"""
    rng = np.random.default_rng(11)
    edge = np.array([0, 2 ** 31, 0xFFFFFFFF], dtype=np.uint64)
    f = [np.where(rng.random(n) < 0.3, edge[rng.integers(0, 3, n)], rng.integers(0, 2 ** 32, n, dtype=np.uint64)) for _ in range(3)]
    site = rng.integers(0, 64, n, dtype=np.uint64)
    seed = rng.integers(0, 2 ** 64, n, dtype=np.uint64)
    kind = rng.integers(0, 4, n)
    seed = np.where(kind == 1, seed & np.uint64(0xFFFFFFFF), seed)                                    # high word clear
    chain = rng.integers(1, 9, n).astype(np.uint64)
    seed = np.where(kind == 2, (seed | np.uint64(0xFFFFFFFF)) - chain + np.uint64(1), seed)           # seed + chain carries into the high word
    seed = np.where(kind == 3, np.uint64(2 ** 64 - 1) - chain + np.uint64(1) + (seed & np.uint64(1)), seed)   # ... and wraps at 2^64
    return f[0], site, f[1], f[2], seed, chain


def test_philox_on_random_counters_and_keys():
    L = bnr_amd.lib()
    n = 10 ** 4
    it, site, elem, att, seed, chain = _random_counters(n)
    key = seed + chain                                                                                # uint64: mod 2^64
    assert np.any((seed >> np.uint64(32)) != (key >> np.uint64(32))) and np.any(key < chain)
    a, b = rr.words(key, it, site, elem, att)
    got = np.array([_lib_philox(L, (int(it[i]), int(site[i]), int(elem[i]), int(att[i])), (int(key[i]) & 0xFFFFFFFF, int(key[i]) >> 32))
                    for i in range(n)], dtype=np.uint64)
    assert np.array_equal(got[:, 0] | (got[:, 1] << np.uint64(32)), a) and np.array_equal(got[:, 2] | (got[:, 3] << np.uint64(32)), b)
    # the key of a draw is seed + chain id split into its two words: the uniforms of the library (which adds nothing itself) and of the oracle
    u2 = (C.c_double * 2)()
    ua, ub = rr.unit(a), rr.unit(b)
    for i in range(0, n, 10):
        L.bnr_host_uniform2(int(key[i]), int(it[i]), int(site[i]), int(elem[i]), int(att[i]), u2)
        assert (u2[0], u2[1]) == (ua[i], ub[i]) == bo.uniform2(int(key[i]), int(it[i]), int(site[i]), int(elem[i]), int(att[i]))
    for mut in PHILOX_MUTATIONS:
        am, bm = rr.words(key, it, site, elem, att, **mut)
        assert np.mean((am != a) & (bm != b)) > 0.99, mut


def test_unit_map_is_the_exact_grid_and_open():
    """0 < u < 1 on every word is the assertion that fails on the parent's formula (y = 2^53 - 1 gave exactly 1.0: rr.unit(clamp=False), the
    bare formula in float64, is asserted to do so); bnr_unit maps that y alone elsewhere, so the stream of every other word did not move."""
    L = bnr_amd.lib()
    ys = [0, 1, 2 ** 52 - 1, 2 ** 52, 2 ** 52 + 1, 2 ** 53 - 2, 2 ** 53 - 1]
    crafted = [y << 11 for y in ys] + [(y << 11) | 0x7FF for y in ys]
    for w in crafted:
        y = w >> 11
        want = (2 * y + 1) / 2 ** 54 if y < 2 ** 52 else (y + (y & 1)) / 2 ** 53                       # Python ints: exact quotients of a float64
        if want == 1.0:
            want = 1.0 - 2.0 ** -53
        for got in (L.bnr_host_unit(w), bo.unit(w), float(rr.unit(w))):
            assert got == want and 0.0 < got < 1.0, (hex(w), got)
    assert L.bnr_host_unit((2 ** 52) << 11) == 0.5                                                     # 1/2 itself is reachable
    bare = (float(2 ** 53 - 1) + 0.5) * 2.0 ** -53
    assert bare == 1.0 == float(rr.unit((2 ** 53 - 1) << 11, clamp=False))                             # the defect of the unclamped formula
    w = np.random.default_rng(3).integers(0, 2 ** 64, 10 ** 5, dtype=np.uint64)
    got = np.array([L.bnr_host_unit(int(v)) for v in w])
    assert np.array_equal(got, rr.unit(w)) and np.all((got > 0) & (got < 1))
    assert np.array_equal(got, ((w >> np.uint64(11)).astype(np.float64) + 0.5) * 2.0 ** -53)          # the unchanged formula: no draw moved
    assert np.array_equal(got[:2000], [bo.unit(int(v)) for v in w[:2000]])


# ------------------------------------------------------------------------------------------------------------------ the normal
def _mp_normal(ua, ub):
    import mpmath
    with mpmath.workdps(40):
        return [mpmath.sqrt(-2 * mpmath.log(mpmath.mpf(float(a)))) * mpmath.cos(2 * mpmath.pi * mpmath.mpf(float(b))) for a, b in zip(ua, ub)]


def _mp_rel(z, ref):
    """|z - ref| / |ref| of long double z against mpmath values, the difference taken in mpmath; where z is exactly 0 (ub = 1/4, 3/4) the 40-digit
    value must be 0 to its own precision (2 pi is rounded there)"""
    import mpmath
    out = []
    with mpmath.workdps(40):
        for a, r in zip(z, ref):
            hi = float(a)
            am = mpmath.mpf(hi) + mpmath.mpf(float(a - LD(hi)))                                        # the long double, exactly
            if am == 0:
                out.append(0.0 if abs(r) < 1e-35 else np.inf)
            else:
                out.append(float(abs(am - r) / abs(r)))
    return np.array(out)


def _float64_normal(ua, ub):
    """the formula in float64 with numpy's libm, quadrant by quadrant"""
    x = 4.0 * ub
    qd = np.floor(x + 0.5)
    t = (x - qd) * (np.pi / 2)
    qi = qd.astype(np.int64) & 3
    return np.sqrt(-2.0 * np.log(ua)) * np.where(qi == 0, np.cos(t), np.where(qi == 1, -np.sin(t), np.where(qi == 2, -np.cos(t), np.sin(t))))


def test_normal_reference_on_crafted_pairs():
    """ub within 40 grid steps of 1/8, 1/4, 1/2, 3/4 and 1, ua at its smallest, at 0.3 and at its largest: the long-double reference equals a
    40-digit evaluation to 2^-60, is exactly 0 at ub = 1/4 and 3/4, and a float64 evaluation of the formula lies within the bound"""
    ub = []
    for target in (0.125, 0.25, 0.5, 0.75, 1.0):
        y0 = int(target * 2 ** 53)
        ub += [float(rr.unit(y << 11)) for y in range(max(0, y0 - 40), min(2 ** 53 - 1, y0 + 40) + 1)]
    ub = np.array(ub + [0.25, 0.75])          # the exact zeros (3/4 is on the grid, 1/4 lies between two of its points: given as it is)
    for ua in (2.0 ** -54, 0.3, 1.0 - 2.0 ** -53):
        uav = np.full(ub.size, ua)
        z, bound = rr.normal_ref(uav, ub)
        assert np.all(_mp_rel(z, _mp_normal(uav, ub)) <= 2.0 ** -60)
        for q in (0.25, 0.75):
            assert np.all(z[ub == q] == 0) and np.any(ub == q)
        err = np.abs(f64(np.asarray(_float64_normal(uav, ub), dtype=LD) - z))
        assert np.all(err <= bound), float(np.max(err / np.maximum(bound, 1e-300)))
        assert np.all(_float64_normal(uav, ub)[(ub == 0.25) | (ub == 0.75)] == 0)


def test_normal_reference_against_mpmath():
    e = np.arange(2000)
    ua, ub = rr.draw2(SEED, 3, 19, e)
    z, _ = rr.normal_ref(ua, ub)
    rel = _mp_rel(z, _mp_normal(ua, ub))
    print("\nlong-double normal against mpmath at 40 digits: largest relative difference 2^%.1f" % np.log2(max(rel.max(), 1e-30)))
    assert rel.max() <= 2.0 ** -60


def _host_normals(n, seed=SEED, it=3, site=19):
    L = bnr_amd.lib()
    return np.array([L.bnr_host_normal(seed, it, site, e, 0) for e in range(n)])


def test_host_normal_within_its_bound():
    n = 10 ** 5
    got = _host_normals(n)
    z, bound = rr.normal(SEED, 3, 19, np.arange(n))
    err = np.abs(f64(np.asarray(got, dtype=LD) - z))
    print("\nbnr_host_normal: largest error %.2f u of the value (bound %.1f u)" % (float(np.max(err / (U * np.abs(f64(z))))), rr.NORMAL_ULPS))
    assert np.all(err <= bound)
    assert np.array_equal(got[:500], [bo.normal(SEED, 3, 19, e, 0) for e in range(500)])
    zm, bm = rr.normal(SEED, 3, 19, np.arange(n), quadrant_sign=False)                                # the mutation must be seen
    assert np.mean(np.abs(f64(np.asarray(got, dtype=LD) - zm)) > bm) > 0.3


# ------------------------------------------------------------------------------------------------------------------ the Gamma sampler
def _host_gammas(shape, n, seed=SEED, it=IT, site=SITE):
    L = bnr_amd.lib()
    return np.array([L.bnr_host_gamma(seed, shape, it, site, e) for e in range(n)])


def _gamma_check(shape, n, **mutation):
    """bnr_host_gamma on n elements against gamma_ref: (draws outside their bound or on another attempt than the reference's, skipped draws,
    largest error / bound, largest error in u of the value, deepest accepted attempt).  The library's attempt is the one whose candidate
    d v^3 boost lies nearest to its value (candidates of different attempts are unrelated numbers)."""
    got = _host_gammas(shape, n)
    cand = []
    val, bound, att, robust = rr.gamma_ref(rr.VE(LD(shape)), SEED, IT, SITE, np.arange(n), candidates=cand, **mutation)
    skipped = ~robust | rr.vacuous(val, bound)
    # the attempt whose candidate d v^3 boost is nearest to the library's value
    best, best_d = np.full(n, -1), np.full(n, np.inf)
    for t, pos, v in cand:
        d = np.abs(v - got[pos])
        closer = d < best_d[pos]
        best[pos[closer]], best_d[pos[closer]] = t, d[closer]
    err = np.abs(f64(np.asarray(got, dtype=LD) - val))
    ok = ~skipped
    bad = ok & ((err > bound) | (best != att))
    with np.errstate(divide="ignore", invalid="ignore"):
        r = float(np.max(np.where(ok & (err > 0), err / bound, 0.0)))
        ulps = float(np.max(np.where(ok, err / (U * np.abs(f64(val))), 0.0)))
    return int(bad.sum()), int(skipped.sum()), r, ulps, int(att.max())


@pytest.mark.parametrize("shape", GAMMA_SHAPES)
def test_host_gamma_within_its_bound_on_the_same_attempt(shape):
    bad, skipped, r, ulps, deepest = _gamma_check(shape, 3000)
    print("\nbnr_host_gamma shape %g: largest error / bound %.3g (%.1f u), deepest accepted attempt %d" % (shape, r, ulps, deepest))
    assert skipped == 0, "no draw may be skipped"
    assert bad == 0


@pytest.mark.parametrize("shape,mutation", [(2.5, dict(d_offset=0.3)), (130.5, dict(d_offset=0.3)), (0.5, dict(boost_inverse=False)),
                                            (0.05, dict(boost_inverse=False)), (2.5, dict(accept_reversed=True)), (0.5, dict(accept_reversed=True))])
def test_gamma_comparison_sees_a_mutated_sampler(shape, mutation):
    bad, skipped, _r, _u, _d = _gamma_check(shape, 300, **mutation)
    assert bad > 30, (mutation, bad, skipped)


def test_gamma_and_normal_distributions():
    """KS of the library's draws against their distributions (fixed seeds: the floor of the other calibration tests)"""
    ps = {}
    for shape in GAMMA_SHAPES:
        ps["Gamma(%g)" % shape] = stats.kstest(_host_gammas(shape, 20000, it=2), "gamma", args=(shape,)).pvalue
    ps["normal"] = stats.kstest(_host_normals(60000, it=4), "norm").pvalue
    print("\nKS p-values:", {k: "%.3g" % v for k, v in ps.items()})
    assert min(ps.values()) > P_MIN, ps


# ------------------------------------------------------------------------------------------------------------------ the prior row
@pytest.mark.parametrize("case", range(len(rr.CASES)))
def test_oracle_prior_row_matches_init_ref(case):
    V, R, nu, eta = rr.CASES[case]
    seed = rr.case_seed(case)
    q = V * (V + 1) // 2
    rng = np.random.default_rng(case)
    X, y = rng.standard_normal((8, q)), rng.standard_normal(8)
    for chain in (rr.CHAIN_ID, rr.LIKE_ID):
        o = bo.Oracle(X, y, R, 2, seed, chain=chain, eta=eta, nu=nu)
        o.init_prior()
        assert o.status == 0
        ref = rr.init_ref(V, R, eta, nu, (seed + chain) % 2 ** 64)
        got = {k: o.t[k][0] for k in bo.COLUMNS}
        worst, checked, skipped = rr.check_init(got, ref)
        print("\noracle prior row V=%d R=%d nu=%g eta=%g chain %d, largest error/bound:" % (V, R, nu, eta, chain),
              {k: "%.3g" % v for k, v in worst.items() if k not in rr.EQUAL}, "; in u of the value:", {k: "%.2f" % v for k, v in rr.raw_units(got, ref).items()})
        assert skipped == 0 and ref["lam_robust"].all() and ref["pi_robust"].all() and ref["second_order_ok"]
        assert max(worst.values()) <= 1.0, worst
