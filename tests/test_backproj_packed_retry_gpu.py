"""GPU tests of k_backproj64's draw (run with -m gpu on an MI355X): one rejection sampler per drawing wave, attempt 0 of every edge in its own lane, then the rejected
edges' further attempts packed over the wave's 64 lanes.  The draw is the first accepted attempt of bnr_gig (gig.jl), so gamma, S and the per-chunk partial sums must be
bitwise the tables of k_backproj (wide_backproj = 0): for a chain alone and as a member of a group of three, from graphs and eagerly, with the sums inside the launch and as
a launch of their own.  Which sampler an edge takes and which attempt it accepts is restated on the host (bnr_host_gig_attempts) from the fetched rows and asserted, so
that the cases provably reach the paths they are meant for."""
import numpy as np
import pytest

import bnr_amd
from oracle import bnr_oracle as bo

pytestmark = pytest.mark.gpu

VARIANTS = (("32 edges per workgroup", {"wide_backproj": 0}), ("64 edges", {"wide_backproj": 1}), ("64 edges, eager", {"wide_backproj": 1, "graph": 0}),
            ("64 edges, sums split off", {"wide_backproj": 1, "split_sums": 1}), ("64 edges, sums inside", {"wide_backproj": 1, "split_sums": 0}))
EPS10 = 2.220446049250313e-16 * 10.0


def _inputs(n, V, R, binary):
    if binary:
        rng = np.random.default_rng(5)
        return bnr_amd.XInput(np.asfortranarray(rng.random((n, V * (V + 1) // 2)) < 0.5), False), rng.normal(size=n)
    X, y, _ = bnr_amd.make_synthetic(n, V, R, seed=11)
    return X, y


def _draw_inputs(t, i, V):
    """chi and psi of update_D! (gibbs.jl:454-458) for 0-based row i of table t: chi_e = (gamma_e - W_e)^2 / tau2 with W = the lower triangle of u' Lambda u (this row's u,
    the row before's Lambda), psi = the row before's theta; edges in the order of bnr_host_edge_index"""
    el = np.array([l for k in range(V) for l in range(k, V)])
    ek = np.array([k for k in range(V) for l in range(k, V)])
    u, lam = t["u"][i], t["lam"][i - 1][:, 0]
    W = np.einsum("r,re,re->e", lam, u[:, el], u[:, ek])
    g = t["gamma"][i][:, 0] - W
    return g * g / t["tau2"][i, 0, 0], float(t["theta"][i - 1, 0, 0])


def _kinds(chi, psi):
    """bnr_gig_kind for lambda = 1/2: 0 chi ~ 0, 1 psi ~ 0, 2 ratio of uniforms (sqrt(psi chi) > 0.2), 3 concave"""
    omega = np.sqrt(psi * chi)
    return np.where(chi < EPS10, 0, np.where(psi < EPS10, 1, np.where(omega > 0.2, 2, np.where(omega > 0.0, 3, 4))))


def _chain_set(X, y, R, tot, seed, binary, opts, hyper):
    ch = bnr_amd.Chain(X, y, R, tot, seed, 1, **hyper)
    mates = [bnr_amd.Chain.like(ch, seed, c, tot) for c in (2, 3)]
    solo = bnr_amd.Chain.like(ch, seed, 1, tot)
    for c in [ch, solo] + mates:
        c.init_prior()
        if binary:
            c.set_option("gram_i8", 0)
    g = bnr_amd.Group([mates[0], ch, mates[1]])
    for k, v in opts.items():
        g.set_option(k, v)
        solo.set_option(k, v)
    return ch, mates, solo, g


def _tables(X, y, R, seed, rows, binary=False, theta=None, **hyper):
    """{variant: (the group member's table, the table of the same chain alone)}: rows 2 ... `rows`, then -- theta given -- one more sweep from row `rows` with that theta"""
    tot = rows + (1 if theta is not None else 0)
    tabs = {}
    for name, opts in VARIANTS:
        ch, mates, solo, g = _chain_set(X, y, R, tot, seed, binary, opts, hyper)
        g.run(2, rows, rows)
        solo.run(2, rows, rows)
        if theta is not None:
            for c in [ch, solo] + mates:
                t = c.fetch()
                t["theta"][rows - 1] = theta
                c.load(t, rows, rows)
            g.run(tot, tot, tot)
            solo.run(tot, tot, tot)
        tabs[name] = (ch.fetch(), solo.fetch())
        for c in (ch, solo):
            assert c.counters()["chol_fail"] == 0 and c.counters()["sampler_cap"] == 0
        g.close()
        for c in [ch, solo] + mates:
            c.close()
    return tabs


def _assert_bitwise(tabs, what):
    base = tabs["32 edges per workgroup"]
    assert np.isfinite(base[1]["S"]).all() and (base[1]["S"] > 0).all(), what
    for name, (grp, alone) in tabs.items():
        for k in bo.COLUMNS:
            assert np.array_equal(grp[k], base[0][k]), (what, name, "group", k)
            assert np.array_equal(alone[k], base[1][k]), (what, name, "alone", k)
            assert np.array_equal(grp[k], alone[k]), (what, name, "group vs alone", k)


# (n, V, R, byte image, edges in the last workgroup of 64, workgroups): a fit that is one workgroup; workgroups of 64 edges followed by one of 62, 14, 20, 2, 33, 32 and 1
SHAPES = [(70, 19, 5, False, 62, 3), (64, 7, 2, False, 28, 1), (130, 12, 3, False, 14, 2), (40, 23, 11, False, 20, 5), (64, 12, 2, True, 14, 2), (40, 11, 2, False, 2, 2),
          (32, 62, 2, False, 33, 31), (32, 63, 2, False, 32, 32), (24, 126, 2, False, 1, 126)]


@pytest.mark.parametrize("n,V,R,binary,last,nwg", SHAPES)
def test_tables_are_bitwise_those_of_k_backproj(gpu, n, V, R, binary, last, nwg):
    """rows 2 ... 6 of the chain's own trajectory (both samplers, mixed inside the workgroups), then one sweep from theta = 1e-300: psi < 10 eps sends every edge through
    the draw without a rejection loop (gig.jl:21-26) in both kernels"""
    q = V * (V + 1) // 2
    assert q == 64 * (nwg - 1) + last
    X, y = _inputs(n, V, R, binary)
    tabs = _tables(X, y, R, 3, 6, binary, theta=1e-300, **(dict(nu=R + 2) if R > 8 else {}))
    _assert_bitwise(tabs, (n, V, R))
    alone = tabs["32 edges per workgroup"][1]
    seen = set()
    for i in range(1, 6):
        chi, psi = _draw_inputs(alone, i, V)
        seen |= set(_kinds(chi, psi).tolist())
    assert seen <= {0, 2, 3} and seen & {2, 3}, seen
    chi, psi = _draw_inputs(alone, 6, V)
    assert psi == 1e-300 and np.isin(_kinds(chi, psi), (0, 1)).all()


@pytest.mark.parametrize("which", ["ratio of uniforms", "concave", "mixed"])
@pytest.mark.parametrize("n,V,R", [(70, 19, 5), (40, 11, 2)])
def test_sampler_kinds_by_loaded_theta(gpu, n, V, R, which):
    """a theta loaded into row 4 decides the samplers of row 5 (omega = sqrt(theta chi): concave up to 0.2, ratio of uniforms above): every edge of the fit on one sampler
    -- the other drawing wave of every workgroup has nothing to do --, and both inside the first workgroup.  gamma, tau2 and u of row 5 do not depend on row 4's theta, so
    a probe chain gives chi; the kinds are then asserted on the rows that the compared chains really wrote."""
    X, y = _inputs(n, V, R, False)
    probe = bnr_amd.Chain(X, y, R, 5, 3, 1)
    probe.init_prior()
    probe.set_option("wide_backproj", 0)
    probe.run(2, 5, 5)
    chi, _ = _draw_inputs(probe.fetch(), 4, V)
    probe.close()
    theta = {"ratio of uniforms": 0.16 / chi.min(), "concave": 0.01 / chi.max(), "mixed": 0.04 / np.median(chi[:64])}[which]      # omega >= 0.4, <= 0.1, 0.2 at the median
    tabs = _tables(X, y, R, 3, 4, theta=theta)
    _assert_bitwise(tabs, (n, V, R, which))
    chi, psi = _draw_inputs(tabs["32 edges per workgroup"][1], 4, V)
    kinds = _kinds(chi, psi)
    assert psi == theta
    if which == "mixed":
        assert min((kinds[:64] == 2).sum(), (kinds[:64] == 3).sum()) >= 8 and set(kinds.tolist()) == {2, 3}, np.bincount(kinds[:64])
    else:
        assert (kinds == (2 if which == "ratio of uniforms" else 3)).all(), np.bincount(kinds)


def _round_sizes(att):
    """the attempts per edge A of the retry rounds of one drawing wave whose edges accept at the attempts `att` (bnr_bp_draw's deal: A = the largest power of two <= 64 / m, at
    most 16, for m open edges; the edges still open after a round advance by A)"""
    a, base, out = att[att > 0], 1, []
    while len(a):
        m = len(a)
        A = 16 if m <= 4 else 8 if m <= 8 else 4 if m <= 16 else 2 if m <= 32 else 1
        out.append(A)
        a, base = a[a >= base + A], base + A
    return out


def test_packed_retry_rounds(gpu):
    """the retry machinery, on states found on the CPU (the oracle's trajectory of this seed, searched with bnr_host_gig_attempts) and asserted here on the fetched rows:
    row 27, first workgroup: more than 32 of its ratio-of-uniforms edges have attempt 0 refused -- more open edges than half a wave, the round with one attempt per edge
    (A = 1); row 11: an edge of another workgroup is accepted only at attempt 5 or later; over the rows, every retry round size A = 16, 8, 4, 2, 1 occurs (the deal of
    bnr_bp_draw restated on the accepted attempts).
    The host restatement is checked against the table first: bnr_host_gig on the recomputed chi gives the fetched S."""
    n, V, R, seed, rows = 40, 23, 3, 543, 27
    X, y = _inputs(n, V, R, False)
    tabs = _tables(X, y, R, seed, rows)
    _assert_bitwise(tabs, (n, V, R, seed))
    t = tabs["32 edges per workgroup"][1]
    L = bnr_amd.lib()
    most_open, deepest, sizes = {}, {}, set()
    for i in range(1, rows):                               # 0-based row i was written by iteration i + 1 of stream seed + chain id
        chi, psi = _draw_inputs(t, i, V)
        kinds = _kinds(chi, psi)
        assert set(kinds.tolist()) <= {2, 3}
        att = np.array([L.bnr_host_gig_attempts(seed + 1, 0.5, float(c), psi, i + 1, e) for e, c in enumerate(chi)])
        S = np.array([L.bnr_host_gig(seed + 1, 0.5, float(c), psi, i + 1, e) for e, c in enumerate(chi)])
        assert np.allclose(S, t["S"][i][:, 0], rtol=1e-9, atol=0.0), i
        assert (att >= 0).all() and att.max() < 100000
        for w in range(0, len(chi), 64):
            for kd in (2, 3):
                most_open[(i + 1, w // 64, kd)] = int(((att[w:w + 64] > 0) & (kinds[w:w + 64] == kd)).sum())
                sizes |= set(_round_sizes(att[w:w + 64][kinds[w:w + 64] == kd]))
        deepest[i + 1] = (int(att.max()), int(att.argmax()) // 64)
    assert most_open[(27, 0, 2)] > 32, most_open[(27, 0, 2)]
    assert deepest[11][0] >= 5 and deepest[11][1] != 0, deepest[11]
    assert sizes == {16, 8, 4, 2, 1}, sizes
