"""GPU tests of the `xi_weights` model option (run with -m gpu on an MI355X): with xi_weights = reference the device samples xi with
the reference's own weight arithmetic (gibbs.jl:349-360: w = w_top / (w_bot + w_top) from two dense (V-1)-dim pdfs, NaN -> fair coin)
and must give the CPU oracle's tables in its reference weight mode (pdf_mode = 0) -- also at sizes where those weights under/overflow,
which the default log-space weights never do.  Tolerance as in test_gpu_parity.py: every column within RTOL = 1e-6, xi and lambda
exactly equal."""
import numpy as np
import pytest

import bnr_amd
from oracle import bnr_oracle as bo

pytestmark = pytest.mark.gpu
RTOL, ATOL = 1e-6, 1e-9
SEED = 20240501


def assert_tables_close(got, ref, what=""):
    for k in bo.COLUMNS:
        a, b = got[k], ref[k]
        assert a.shape == b.shape, (what, k, a.shape, b.shape)
        assert np.all(np.isfinite(a)), (what, k, "non-finite")
        if k in ("xi", "lam"):
            assert np.array_equal(a, b), (what, k, "discrete column differs", np.argwhere(a != b)[:8].tolist())
        else:
            err = np.abs(a - b) / (ATOL / RTOL + np.abs(b))
            assert err.max() < RTOL, (what, k, float(err.max()))


def assert_bitwise(a, b, what=""):
    for k in bo.COLUMNS:
        assert np.array_equal(a[k], b[k], equal_nan=True), (what, k)


def oracle_run(X, y, R, tot, seed, chain=1):
    o = bo.Oracle(X, y, R, tot, seed, chain=chain, pdf_mode=0)
    o.init_prior()
    o.run(2, tot, tot)
    return o


def lone_run(X, y, R, tot, seed, chain, xi_weights):
    ch = bnr_amd.Chain(X, y, R, tot, seed, chain, device=0, xi_weights=xi_weights)
    ch.init_prior()
    ch.run(2, tot, tot)
    t, c = ch.fetch(), ch.counters()
    ch.close()
    return t, c


# ------------------------------------------------------------------------------------------------------------------------
# Crafted rows (the pattern of test_gpu_parity.py's failure-path tests): a state row is loaded with bnr_chain_load, the update_u_xi! hook
# runs on it once, and xi, u and the counters are the oracle's (pdf_mode = 0).  Exact powers of two keep the branch taken independent of
# rounding: S = 1, tau2 = 1, lambda = 1, M = I, gamma = 64 (or 16) on every edge.
def _crafted(V, R, xi_weights, u, gamma, Delta, seed=5):
    X, y, _ = bnr_amd.make_synthetic(12, V, R, seed=77)
    ch = bnr_amd.Chain(X, y, R, 3, seed, 1, device=0, xi_weights=xi_weights)
    o = bo.Oracle(X, y, R, 3, seed, chain=1, pdf_mode=0 if xi_weights == "reference" else 1)
    ch.init_prior()
    o.init_prior()
    t = o.t
    t["u"][0] = u; t["lam"][0] = 1.0; t["S"][0] = 1.0; t["gamma"][0] = gamma; t["xi"][0] = 1.0; t["Delta"][0] = Delta
    t["M"][0] = np.eye(R)
    t["tau2"][1] = 1.0
    ch.load(t, 1, 2)
    ch.update("u_xi", 2, 2)
    o.update("u_xi", 1, 2)
    g, c = ch.fetch(2, 2), ch.counters()
    ch.close()
    assert int(o.o.status) == 0 and c["chol_fail"] == 0
    assert np.array_equal(g["xi"][0], t["xi"][1]), (xi_weights, g["xi"][0].ravel(), t["xi"][1].ravel())
    assert np.allclose(g["u"][0], t["u"][1], rtol=RTOL, atol=ATOL) and np.isfinite(g["u"][0]).all()
    assert c["nan_w"] == int(o.o.nan_w_events)
    return g["xi"][0].ravel().copy(), c["nan_w"]


def test_crafted_both_densities_underflow_every_node_takes_the_coin(gpu):
    """u = 0: both (V-1)-dim log densities are -1/2 (V-1)(log 2 pi + 4096) ~ -65 600: w_top = w_bot = 0, w = NaN, every node flips the coin
    from the XI draw site.  Delta = 1/4, so that the log-space weight (w = 3/4: a draw against 1/4, not 1/2) gives another xi row."""
    V, R = 33, 2
    xi_ref, nan_ref = _crafted(V, R, "reference", 0.0, 64.0, 0.25)
    assert nan_ref == V
    xi_log, nan_log = _crafted(V, R, "log", 0.0, 64.0, 0.25)
    assert nan_log == 0
    assert not np.array_equal(xi_ref, xi_log)                   # non-vacuity: the two modes sample differently on these rows


def test_crafted_only_w_top_underflows(gpu):
    """R = 1, u = 1, gamma = 16, V = 17 (m = 16 neighbours): l_top = -1/2 (16 log 2 pi + 4096) ~ -2063, l_bot = -1/2 (16 log 2 pi + log 17
    + 16 * 256 / 17) ~ -137: w_top = 0 < w_bot, w = 0, xi = 1 for every node without a draw (no NaN)."""
    V, R = 17, 1
    xi, nan_w = _crafted(V, R, "reference", 1.0, 16.0, 0.5)
    assert nan_w == 0 and np.all(xi == 1.0)


def test_crafted_delta_one(gpu):
    """Delta = 1 as in Julia: w_top = 0 * pdf_top = 0; with w_bot > 0 w = 0 and xi = 1 (both modes), with both densities underflowing
    0 / 0 = NaN and the coin (the log-space weight is exp(-Inf) -> w = 0: xi = 1 without a draw)."""
    V = 17
    xi, nan_w = _crafted(V, 1, "reference", 1.0, 16.0, 1.0)
    assert nan_w == 0 and np.all(xi == 1.0)
    xi, nan_w = _crafted(V, 1, "log", 1.0, 16.0, 1.0)
    assert nan_w == 0 and np.all(xi == 1.0)
    xi, nan_w = _crafted(33, 2, "reference", 0.0, 64.0, 1.0)
    assert nan_w == 33 and 0 < xi.sum() < 33
    xi, nan_w = _crafted(33, 2, "log", 0.0, 64.0, 1.0)
    assert nan_w == 0 and np.all(xi == 1.0)


# ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cfg4():
    """BASELINE configs[4]'s size (n = 500, V = 300, R = 10), 4 rows: every node update after the first sweep takes the reference's coin"""
    n, V, R, tot = 500, 300, 10, 4
    X, y, _ = bnr_amd.make_synthetic(n, V, R, seed=SEED)
    return X, y, R, tot, {c: oracle_run(X, y, R, tot, SEED, chain=c) for c in (1, 2, 3)}


def test_configs4_size_matches_the_reference_weights(gpu, cfg4):
    X, y, R, tot, ors = cfg4
    o = ors[1]
    assert int(o.o.nan_w_events) > 0                            # the regime this option exists for
    t, c = lone_run(X, y, R, tot, SEED, 1, "reference")
    assert_tables_close(t, o.t, "configs[4] size, one chain")
    assert c["nan_w"] == int(o.o.nan_w_events) and c["chol_fail"] == 0 and c["sampler_cap"] == 0
    tl, cl = lone_run(X, y, R, tot, SEED, 1, "log")
    assert cl["nan_w"] == 0 and not np.array_equal(tl["xi"], t["xi"])   # the default samples another xi here


def test_configs4_size_group_matches_the_reference_weights(gpu, cfg4):
    X, y, R, tot, ors = cfg4
    chains = [bnr_amd.Chain(X, y, R, tot, SEED, 1, device=0, xi_weights="reference")]
    chains += [bnr_amd.Chain.like(chains[0], SEED, c, tot) for c in (2, 3)]
    assert all(ch.xi_weights == "reference" for ch in chains)
    for ch in chains:
        ch.init_prior()
    g = bnr_amd.Group(chains)
    g.run(2, tot, tot)
    for c, ch in zip((1, 2, 3), chains):
        assert_tables_close(ch.fetch(), ors[c].t, "configs[4] size, group member %d" % c)
        assert ch.counters()["nan_w"] == int(ors[c].o.nan_w_events) > 0
    g.close()
    for ch in chains:
        ch.close()


def test_mixed_regime_per_sweep_nan_counts(gpu):
    """n = 500, V = 200, R = 7, 8 rows: after the first sweep part of the nodes take the coin and the rest draw with an interior w -- both
    branches of update_xi in one launch.  Sweep by sweep, the NaN count is the oracle's."""
    n, V, R, tot = 500, 200, 7, 8
    X, y, _ = bnr_amd.make_synthetic(n, V, R, seed=SEED)
    o = bo.Oracle(X, y, R, tot, SEED, chain=1, pdf_mode=0)
    ch = bnr_amd.Chain(X, y, R, tot, SEED, 1, device=0, xi_weights="reference")
    o.init_prior()
    ch.init_prior()
    per_o, per_g = [], []
    for j in range(2, tot + 1):
        o.run(j, tot, j)
        ch.run(j, tot, j)
        per_o.append(int(o.o.nan_w_events))
        per_g.append(ch.counters()["nan_w"])
    assert per_g == per_o, (per_g, per_o)
    steps = np.diff([0] + per_o)
    assert ((steps > 0) & (steps < V)).any(), steps             # sweeps in which NaN coins and interior weights meet
    assert_tables_close(ch.fetch(), o.t, "n=500 V=200 R=7")
    ch.close()


def test_headline_shape_modes_agree(gpu):
    """n = 500, V = 100, R = 7, 20 rows: no weight under/overflows here, the two modes give the same tables bit for bit, and the oracle's"""
    n, V, R, tot = 500, 100, 7, 20
    X, y, _ = bnr_amd.make_synthetic(n, V, R, seed=SEED)
    o = oracle_run(X, y, R, tot, SEED)
    assert int(o.o.nan_w_events) == 0
    tr, cr = lone_run(X, y, R, tot, SEED, 1, "reference")
    tl, cl = lone_run(X, y, R, tot, SEED, 1, "log")
    assert cr["nan_w"] == cl["nan_w"] == 0
    assert_bitwise(tr, tl, "reference vs log")
    assert_tables_close(tr, o.t, "headline shape, reference")
    assert_tables_close(tl, o.t, "headline shape, log")


# ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def v200():
    """4 chains at n = 500, V = 200, R = 7, 6 rows, each run alone in both modes"""
    n, V, R, tot = 500, 200, 7, 6
    X, y, _ = bnr_amd.make_synthetic(n, V, R, seed=SEED)
    alone = {(c, m): lone_run(X, y, R, tot, SEED, c, m)[0] for c in (1, 2, 3, 4) for m in ("log", "reference")}
    return X, y, R, tot, alone


def _group_of(X, y, R, tot, modes):
    chains = [bnr_amd.Chain(X, y, R, tot, SEED, 1, device=0, xi_weights=modes[0])]
    for c, m in zip(range(2, len(modes) + 1), modes[1:]):
        ch = bnr_amd.Chain.like(chains[0], SEED, c, tot)
        assert ch.xi_weights == modes[0]                        # inherited from the donor ...
        if m != modes[0]:
            ch.set_option("xi_weights", m)                      # ... and set per member
        chains.append(ch)
    for ch in chains:
        ch.init_prior()
    return chains, bnr_amd.Group(chains)


def test_group_in_reference_mode_is_bitwise_its_lone_runs(gpu, v200):
    X, y, R, tot, alone = v200
    assert not np.array_equal(alone[(1, "reference")]["xi"], alone[(1, "log")]["xi"])
    chains, g = _group_of(X, y, R, tot, ["reference"] * 4)
    g.run(2, tot, tot)
    for c, ch in enumerate(chains, 1):
        assert_bitwise(ch.fetch(), alone[(c, "reference")], "group of 4, member %d" % c)
    g.close()
    for ch in chains:
        ch.close()


def test_mixed_group_is_bitwise_its_lone_runs(gpu, v200):
    X, y, R, tot, alone = v200
    modes = ["log", "log", "reference", "reference"]
    chains, g = _group_of(X, y, R, tot, modes)
    g.run(2, tot, tot)
    for c, (ch, m) in enumerate(zip(chains, modes), 1):
        assert_bitwise(ch.fetch(), alone[(c, m)], "mixed group, member %d (%s)" % (c, m))
    g.close()
    for ch in chains:
        ch.close()


def test_switching_a_member_takes_effect_from_the_next_sweep(gpu, v200):
    """set_option("xi_weights") on a group member between two run calls: the member's later sweeps use the new weights (its graphs and the
    group's descriptor copy are rebuilt), bitwise like a lone chain switched at the same point; the other member is untouched"""
    X, y, R, tot, alone = v200
    chains, g = _group_of(X, y, R, tot, ["reference", "reference"])
    g.run(2, tot, 3)
    chains[1].set_option("xi_weights", "log")
    assert chains[1].xi_weights == "log" and chains[0].xi_weights == "reference"
    g.run(4, tot, tot)
    solo = {}
    for c in (1, 2):                                            # the same two run calls, alone
        ch = bnr_amd.Chain(X, y, R, tot, SEED, c, device=0, xi_weights="reference")
        ch.init_prior()
        ch.run(2, tot, 3)
        if c == 2:
            ch.set_option("xi_weights", "log")
        ch.run(4, tot, tot)
        solo[c] = ch.fetch()
        ch.close()
    t1, t2 = chains[0].fetch(), chains[1].fetch()
    assert_bitwise(t2, solo[2], "switched member vs switched lone chain")
    assert_bitwise(t1, solo[1], "untouched member vs lone chain")
    first = {k: t2[k][:3] for k in bo.COLUMNS}
    assert_tables_close(first, {k: alone[(2, "reference")][k][:3] for k in bo.COLUMNS}, "rows before the switch")
    assert not np.array_equal(t2["xi"][3:], alone[(2, "reference")]["xi"][3:])     # the switch did take effect
    with pytest.raises(bnr_amd.BnrError) as e:
        chains[0].set_option("xi_weights", 2)
    assert e.value.code == 1
    g.close()
    for ch in chains:
        ch.close()


# ------------------------------------------------------------------------------------------------------------------------
def test_fit_with_reference_weights_matches_the_oracle(gpu, tmp_path):
    """Fit!(..., xi_weights="reference") end to end at n = 100, V = 300, R = 10, where the reference's weights are NaN after the first
    sweep: chain 1's table is the oracle's in pdf_mode = 0 (and not the log-space one).  psrf_cutoff = Inf: no top-up round (the PSRF of xi
    is Inf here, every chain's xi being constant within each half of the 4-sample window)"""
    n, V, R, nburn, nsamp, seed = 100, 300, 10, 3, 4, SEED               # (the PSRF needs nsamp >= 4)
    X, y, _ = bnr_amd.make_synthetic(n, V, R, seed=SEED)
    r = bnr_amd.Fit(X, y, R, nburn=nburn, nsamples=nsamp, psrf_cutoff=np.inf, x_transform=False, suppress_timer=True, num_chains=2,
                    seed=seed, filename=str(tmp_path / "parameters.log"), xi_weights="reference")
    txt = (tmp_path / "parameters.log").read_text()
    assert "xi_weights" not in txt and "seed=%d" % seed in txt
    tot = nburn + nsamp
    o = bo.Oracle(X, y, R, tot, seed, chain=1, pdf_mode=0)
    o.init_prior()
    o.run(2, nburn, tot)
    assert int(o.o.nan_w_events) > 0
    got = {k: r.state[k] for k in bo.COLUMNS}
    assert_tables_close(got, o.t, "Fit xi_weights=reference, chain 1")
    o1 = bo.Oracle(X, y, R, tot, seed, chain=1, pdf_mode=1)
    o1.init_prior()
    o1.run(2, nburn, tot)
    assert not np.array_equal(o1.t["xi"], got["xi"])
