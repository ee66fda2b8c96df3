"""GPU tests of the node, tau2, M, inv(M), theta, mu, Delta, Lambda and pi stages against the extended-precision references of
tests/sweep_ref.py (run with -m gpu on an MI355X): every entry within its a-priori bound of the device's float64 error, every xi / lambda
decision equal to the exact one unless the uniform lies within the bound of its boundary (those are counted, and must stay few).
In whole sweeps the S stage (update_D!, tests/gig_ref.py) is checked the same way, from k_backproj and -- wide_backproj = 1 -- k_backproj64.

Crafted rows (Chain.load) run one hook at a time on the lone-chain instantiation; short runs and gibbs_step check whole sweeps stage by stage
(inv(M) of the scalar tail, the pre-drawn tau2, the two-workgroup tail), alone and as the middle member of a lockstep group of three.
The largest error / bound ratio per stage is printed (pytest -s)."""
import numpy as np
import pytest

import bnr_amd
import gig_ref as gr
import sweep_ref as sr
from oracle import bnr_oracle as bo
from test_backproj_packed_retry_gpu import _draw_inputs, _kinds

pytestmark = pytest.mark.gpu
IT = 2
SKIP_FRACTION = 0.05          # decisions too close to call, of all checked: more than this and the band could be hiding an error
XG_SWEEP_REL = 1e-10          # in a sweep X gamma comes out of the gamma solve's identity (k_solve_a4): allowance, see _sweep_rows

WORST = {}


def _note(stage, r):
    WORST[stage] = max(WORST.get(stage, 0.0), r)
    assert r <= 1.0, (stage, r)


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    print("\nsweep stages, largest error/bound:", {k: "%.3g" % v for k, v in sorted(WORST.items())})


def _row(t, j):
    return {k: t[k][j] for k in bo.COLUMNS}


def _scal(t, k, j):
    return float(t[k][j].ravel()[0])


def _nodes(V, rng):
    if V <= 130:
        return None
    return np.unique(np.r_[0, 1, V // 2, V - 2, V - 1, rng.choice(V, 11, replace=False)])


class Skips:
    """decisions too close to call, counted per group of stages: the xi / lambda decisions together, the edges of the S stage on their own (q
    edges per row would otherwise widen what the few xi / lambda decisions may skip)"""

    def __init__(self):
        self.count = {}

    def add(self, n, s, group="decisions"):
        c = self.count.setdefault(group, [0, 0])
        c[0] += n
        c[1] += s

    def check(self, what):
        for group, (n, skipped) in self.count.items():
            print("%s: %d of %d %s too close to call" % (what, skipped, n, group))
            assert skipped <= (max(1, SKIP_FRACTION * n) if group == "decisions" else SKIP_FRACTION * n), (what, group, skipped, n)


# ------------------------------------------------------------------------------------------------------------------ crafted rows, one hook each
# n, V, R, tau2, Delta, S spread (decades from 1e-12), kappa(M), zeros in lambda.  kappa(M) stays where the componentwise first-order
# bound of inv(M) holds (sweep_ref.second_order_ok): a larger kappa needs a bound that keeps the structure of inv(M)'s error
CASES = [
    (12, 2, 1, 1.0, 0.5, 0, 1.0, False),
    (447, 3, 2, 1e-8, 1e-12, 18, 1e4, True),
    (448, 64, 7, 1.0, 0.5, 18, 1e4, True),          # V - 1 = 63 staged nodes: one LDS chunk; nblk_bp = 65
    (449, 65, 10, 1e6, 1 - 1e-12, 6, 1e2, False),   # 64 staged: exactly one chunk; npair = 65 > 64 sums
    (1, 66, 11, 1.0, 0.5, 18, 1e3, True),           # two chunks; R = 11: two sum slots per lane
    (12, 129, 20, 1.0, 0.5, 3, 1e3, False),         # 3R + 2 = 62: the one-pass Gamma path of k_tail
    (12, 61, 21, 1.0, 0.5, 18, 1e3, True),          # R = 21: the looped path; q mod 1792 = 99; nblk_bp = 59
    (12, 68, 32, 1.0, 0.5, 3, 10.0, False),         # q mod 1792 = 554
    (20, 75, 2, 1.0, 0.5, 18, 1e5, True),           # 1058
    (20, 81, 3, 1e-8, 0.5, 6, 1e4, False),          # 1529
    (12, 63, 4, 1.0, 0.5, 6, 1e2, True),            # nblk_bp = 63
    (8, 480, 32, 1.0, 0.5, 3, 1e2, False),          # R V = 15 360: u still in LDS
    (8, 600, 32, 1.0, 0.5, 3, 1e2, True),           # R V = 19 200: k_tail reads u from the row; q = 180 300
]


def _craft(t, R, V, tau2, Delta, spread, kappa, lam_zero, rng):
    q = V * (V + 1) // 2
    if spread:
        t["S"][0, :, 0] = 10.0 ** rng.uniform(-12, -12 + spread, q)
    Q, _ = np.linalg.qr(rng.standard_normal((R, R)))
    M = (Q * np.logspace(0, -np.log10(kappa), R)) @ Q.T * 3.0
    t["M"][0] = (M + M.T) / 2
    if lam_zero and R > 1:
        t["lam"][0, ::2, 0] = 0.0
    t["Delta"][0] = Delta
    for k in bo.COLUMNS:
        t[k][1] = t[k][0]
    t["tau2"][1] = tau2


@pytest.mark.parametrize("n,V,R,tau2,Delta,spread,kappa,lam_zero", CASES)
def test_hooks_on_crafted_rows_match_the_references(gpu, n, V, R, tau2, Delta, spread, kappa, lam_zero):
    rng = np.random.default_rng(1000 + V + R)
    nu = max(10, R + 2)
    X, y, _ = bnr_amd.make_synthetic(n, V, R, seed=V + 7 * R)
    seed = 600 + V
    ch = bnr_amd.Chain(X, y, R, 3, seed, 1, device=0, nu=nu)
    var = sr.Variates(bnr_amd.lib(), seed + 1)
    el, ek = sr.edge_nodes(V)
    ch.init_prior()
    t = ch.fetch()
    _craft(t, R, V, tau2, Delta, spread, kappa, lam_zero, rng)
    ch.load(t)
    skips = Skips()

    # tau2 (refresh_carried: the carried sums of row 1 and inv(M) by the tail's route, then k_node mode 1)
    ch.update("tau2", 2, IT)
    g = ch.fetch()
    t2, e, rr, e_rr, sq, e_sq = sr.tau2_ref(_row(t, 0), X, y, V, var, IT, el, ek)
    sc = ch.debug_copy(5, 8)
    _note("rr", sr.check(sc[0], rr, e_rr))
    _note("sig_q", sr.check(sc[1], sq, e_sq))
    _note("tau2", sr.check(_scal(g, "tau2", 1), t2, e))
    Mi, ldM, eMi, eldM = sr.inv_M_ref(t["M"][0], "tri")
    dm = ch.debug_copy(4, R * R + 1)
    _note("inv(M)", sr.check(dm[:R * R].reshape(R, R, order="F"), Mi, eMi))
    _note("logdet M", sr.check(dm[R * R], ldM, eldM))

    # u, xi (k_node mode 2 | 4: inv(M) by the hook's own solves) at the crafted tau2
    g["tau2"][1] = tau2
    ch.load(g)
    ch.update("u_xi", 2, IT)
    t, g = g, ch.fetch()
    nr = sr.node_ref(_row(t, 0), tau2, var, IT, nodes=_nodes(V, rng))
    r, bad, sk = sr.check_node(g["u"][1], g["xi"][1], nr)
    assert bad == 0, ("xi", bad)
    skips.add(len(nr["nodes"]), sk)
    _note("u", r)

    # theta (sum S of row 2 from the back-projection's partials), Delta, M, mu, Lambda, pi: each from the table before its hook
    for name in ("theta", "Delta", "M", "mu", "Lambda", "pi"):
        t = g
        ch.update(name, 2, IT)
        g = ch.fetch()
        c = _row(t, 1)
        if name == "theta":
            _note("theta", sr.check(_scal(g, "theta", 1), *sr.theta_ref(c, V, 1.0, 1.0, var, IT)))
        elif name == "Delta":
            _note("Delta", sr.check(_scal(g, "Delta", 1), *sr.Delta_ref(c, V, 1.0, 1.0, var, IT)))
        elif name == "M":
            M, eM, _, _ = sr.M_ref(c, nu, var, IT)
            _note("M", sr.check(g["M"][1], M, eM))
        elif name == "mu":
            _note("mu", sr.check(_scal(g, "mu", 1), *sr.mu_ref(c, X, y, var, IT)))
        elif name == "Lambda":
            ll, ell, sS, e_sS = sr.lambda_sums_ref(c, t["lam"][0], el, ek)
            ps = ch.debug_copy(6, ((V * (V + 1) // 2 + 31) // 32) * (1 + 3 * R)).reshape(-1, 1 + 3 * R)
            tot = ps.astype(sr.LD).sum(axis=0)
            _note("sum S", sr.check(np.float64(tot[0]), sS, e_sS + sr.gamma_m(ps.shape[0]) * float(sS)))
            _note("Lambda sums", sr.check(sr.f64(tot[1:]).reshape(R, 3), ll, ell + sr.gamma_m(ps.shape[0]) * np.abs(sr.f64(ll))))
            lam, rob = sr.lambda_ref(ll, ell, t["pi"][0], var, IT)
            assert np.array_equal(lam[rob], g["lam"][1].ravel()[rob]), (lam, g["lam"][1].ravel())
            skips.add(R, int(np.sum(~rob)))
        else:
            _note("pi", sr.check(g["pi"][1], *sr.pi_ref(c, 1.01, var, IT)))
    c = ch.counters()
    assert c["chol_fail"] == 0 and c["sampler_cap"] == 0
    skips.check("n=%d V=%d R=%d" % (n, V, R))
    ch.close()


# ------------------------------------------------------------------------------------------------------------------ whole sweeps
def _sweep_rows(g, X, y, R, V, nu, var, rows, skips):
    """every stage of rows j (0-based, iteration id j + 1) from row j - 1 of the same table.  Here the node update reads inv(M) from the
    scalar tail (the triangular-inverse route), tau2 is pre-drawn by the tail, and X gamma in rr and mu is the gamma solve's
    X W + tau X sz + tau (b - a4) rather than a product with the stored gamma: that vector is checked against exact references by
    tests/test_gamma_linalg_gpu.py; here it gets an allowance of XG_SWEEP_REL (|X| |gamma| + |y|) per row."""
    el, ek = sr.edge_nodes(V)
    Xa = np.abs(X)
    for j in rows:
        it = j + 1
        p, c = _row(g, j - 1), _row(g, j)
        t2, e, rr, e_rr, sq, e_sq = sr.tau2_ref(p, X, y, V, var, it, el, ek)
        ex = XG_SWEEP_REL * (Xa @ np.abs(p["gamma"].ravel()) + np.abs(y))
        res = np.abs(sr.f64(np.asarray(y, dtype=sr.LD) - sr.LD(_scal(g, "mu", j - 1)) - sr.xgamma(X, p["gamma"])[0]))
        e += sr.SAFETY * float(np.sum(res * ex)) / var.gamma(X.shape[0] / 2.0 + V * (V + 1) / 4.0, it, sr.SITE_TAU2, 0)   # (2 |r| dr) / 2 / G
        _note("tau2 (sweep)", sr.check(_scal(g, "tau2", j), t2, e))
        Mi = sr.inv_M_ref(g["M"][j - 1], "tri")
        nr = sr.node_ref(p, _scal(g, "tau2", j), var, it, Minv=Mi)
        r, bad, sk = sr.check_node(g["u"][j], g["xi"][j], nr)
        assert bad == 0, ("xi", j, bad)
        skips.add(V, sk)
        _note("u (sweep)", r)
        _note("theta (sweep)", sr.check(_scal(g, "theta", j), *sr.theta_ref(c, V, 1.0, 1.0, var, it)))
        _note("Delta (sweep)", sr.check(_scal(g, "Delta", j), *sr.Delta_ref(c, V, 1.0, 1.0, var, it)))
        M, eM, _, _ = sr.M_ref(c, nu, var, it)
        _note("M (sweep)", sr.check(g["M"][j], M, eM))
        mu, e = sr.mu_ref(c, X, y, var, it)
        e += float(np.sum(XG_SWEEP_REL * (Xa @ np.abs(c["gamma"].ravel()) + np.abs(y)))) / X.shape[0]
        _note("mu (sweep)", sr.check(_scal(g, "mu", j), mu, e))
        ll, ell, _, _ = sr.lambda_sums_ref(c, g["lam"][j - 1], el, ek)
        lam, rob = sr.lambda_ref(ll, ell, g["pi"][j - 1], var, it)
        assert np.array_equal(lam[rob], g["lam"][j].ravel()[rob]), (j, lam, g["lam"][j].ravel())
        skips.add(R, int(np.sum(~rob)))
        _note("pi (sweep)", sr.check(g["pi"][j], *sr.pi_ref(c, 1.01, var, it)))
        # update_D!: row j's S from row j's gamma, u, tau2 and row j - 1's lambda and theta
        worst, skipped, bad = gr.check_S(c["S"], gr.S_ref(p, c, V, var, it))
        assert bad == 0, ("S", j, bad)
        skips.add(c["S"].size, skipped, "edges of S")
        for k, v in worst.items():
            _note(k + " (sweep)", v)


@pytest.mark.parametrize("n,V,R", [(40, 8, 3), (70, 19, 21), (30, 12, 7)])
def test_a_run_matches_the_references_stage_by_stage(gpu, n, V, R):
    tot, seed, nu = 6, 4242, max(10, R + 2)
    X, y, _ = bnr_amd.make_synthetic(n, V, R, seed=3 + V)
    ch = bnr_amd.Chain(X, y, R, tot, seed, 1, device=0, nu=nu)
    ch.init_prior()
    assert ch.run(2, tot, tot) == tot + 1
    g = ch.fetch()
    skips = Skips()
    _sweep_rows(g, X, y, R, V, nu, sr.Variates(bnr_amd.lib(), seed + 1), range(1, tot), skips)
    skips.check("run n=%d V=%d R=%d" % (n, V, R))
    assert ch.counters()["chol_fail"] == 0
    ch.close()


def test_gibbs_step_matches_the_references(gpu):
    n, V, R, seed, nu = 40, 9, 4, 99, 10
    X, y, _ = bnr_amd.make_synthetic(n, V, R, seed=5)
    ch = bnr_amd.Chain(X, y, R, 3, seed, 1, device=0)
    ch.init_prior()
    ch.gibbs_step(2, 2)
    g = ch.fetch()
    skips = Skips()
    _sweep_rows(g, X, y, R, V, nu, sr.Variates(bnr_amd.lib(), seed + 1), [1], skips)
    skips.check("gibbs_step")
    ch.close()


def test_middle_member_of_a_group_matches_the_references(gpu):
    """the lockstep-group instantiations (bnr_many) read their descriptors by chain index: member 1 of 3"""
    n, V, R, tot, nu = 60, 14, 5, 5, 10
    X, y, _ = bnr_amd.make_synthetic(n, V, R, seed=21)
    chains = [bnr_amd.Chain(X, y, R, tot, 300, 1, device=0)]
    chains += [bnr_amd.Chain.like(chains[0], 300, c, tot) for c in (2, 3)]
    for c in chains:
        c.init_prior()
    grp = bnr_amd.Group(chains)
    assert grp.run(2, tot, tot) == tot + 1
    skips = Skips()
    for m in (1, 2):
        _sweep_rows(chains[m].fetch(), X, y, R, V, nu, sr.Variates(bnr_amd.lib(), 300 + m + 1), range(1, tot), skips)
    skips.check("group")
    grp.close()
    for c in chains:
        c.close()


@pytest.mark.parametrize("ids", [(1,), (1, 2, 3)])
def test_sweeps_of_k_backproj64_match_the_references(gpu, ids):
    """wide_backproj = 1: a sweep's back-projection (flags 3 or 7) is k_backproj64 -- reachable no other way --, for a chain alone and for a lockstep group of three
    (its middle member is `mid`).  Rows 2 ... 4, then one more sweep from a theta loaded into row 4 that puts omega = 0.2 at the median of mid's first 64 edges of
    row 5: both drawing waves of its first workgroup have work (gamma, tau2 and u of row 5 do not depend on row 4's theta, so a probe chain gives chi)."""
    n, V, R, seed, rows, nu = 60, 14, 5, 300, 4, 10
    tot = rows + 1
    # launch_backproj keeps k_backproj where k_backproj64's LDS (a4 | 64 dots | u products R x 65 | terms (3R + 1) x 65, and the 13 312 bytes of
    # BNR_BP64_STATIC_LDS) passes 124 KB, and no counter tells which kernel ran: here n_pad = 64, (64 + 64 + 325 + 1040) x 8 + 13 312 = 25 256 bytes
    assert (-(-n // 64) * 64 + 64 + 65 * R + 65 * (3 * R + 1)) * 8 + (2 * 11 * 64 + 3 * 64) * 8 + 2 * 64 * 4 <= 124 * 1024
    X, y, _ = bnr_amd.make_synthetic(n, V, R, seed=21)
    chains = [bnr_amd.Chain(X, y, R, tot, seed, ids[0], device=0)]
    chains += [bnr_amd.Chain.like(chains[0], seed, c, tot) for c in ids[1:]]
    mid = len(ids) // 2
    probe = bnr_amd.Chain.like(chains[0], seed, ids[mid], tot)
    probe.init_prior()
    assert probe.run(2, tot, tot) == tot + 1
    chi, _ = _draw_inputs(probe.fetch(), tot - 1, V)
    probe.close()
    theta = 0.04 / np.median(chi[:64])
    for c in chains:
        c.init_prior()
    runner = bnr_amd.Group(chains) if len(chains) > 1 else chains[0]
    runner.set_option("wide_backproj", 1)
    assert runner.run(2, rows, rows) == rows + 1
    skips = Skips()
    checked = sorted({mid, len(ids) - 1})
    for m, c in enumerate(chains):
        t = c.fetch()
        if m in checked:
            _sweep_rows(t, X, y, R, V, nu, sr.Variates(bnr_amd.lib(), seed + ids[m]), range(1, rows), skips)
        t["theta"][rows - 1] = theta
        c.load(t, rows, rows)
    assert runner.run(tot, tot, tot) == tot + 1
    for m in checked:
        g = chains[m].fetch()
        _sweep_rows(g, X, y, R, V, nu, sr.Variates(bnr_amd.lib(), seed + ids[m]), [tot - 1], skips)
        assert chains[m].counters()["chol_fail"] == 0 and chains[m].counters()["sampler_cap"] == 0
        if m == mid:
            chi, psi = _draw_inputs(g, tot - 1, V)
            kinds = _kinds(chi, psi)[:64]
            assert psi == theta and min((kinds == 2).sum(), (kinds == 3).sum()) >= 8, np.bincount(kinds)
    skips.check("k_backproj64, %d chain(s)" % len(ids))
    if len(chains) > 1:
        runner.close()
    for c in chains:
        c.close()
