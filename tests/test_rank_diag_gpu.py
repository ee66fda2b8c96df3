"""GPU tests of the rank-normalised convergence diagnostics (ABI 12; run with -m gpu on an MI355X): the rank kernel alone
(bnr_amd.rank_normalize against scipy.stats.rankdata and bnr_host_ndtri), bnr_chains_rank_diag / bnr_chain_rank_diag against the package's
numpy restatement api._host_rank_diagnostics (itself pinned to an independent transcription of `posterior` by tests/test_rank_diag_host.py),
the bitwise properties, what the feature is for, the refusals and Fit(..., rank_diagnostics=True).

Chains as in test_diagnostics_gpu.py: three Chains of n = 8, V = 16, R = 2 with 640-row tables, never run; tables come in by Chain.load.

K_PHI: the largest gap between the device's z and bnr_host_ndtri((r - 3/8) / (S + 1/4)) over every row of the rank-kernel cases was measured as
4 ulp (at S = 4097; 0 ulp at every other length: host and device share the arithmetic bit for bit but for the one log and the one sqrt of the tails); the test allows 4 x that, the
procedure of test_noise_counter_layout_and_ulp_gap."""
import numpy as np
import pytest
from scipy.stats import rankdata

import bnr_amd
import diag_ref as dr
import rank_diag_cases as rc
import rank_diag_ref as rr
from bnr_amd import _capi, api
from oracle import bnr_oracle as bo

pytestmark = pytest.mark.gpu
K_PHI = 4.0                                            # ulp, measured on an MI355X (see the module docstring)
WORST = {}
ROW_LENGTHS = (1, 2, 3, 63, 64, 65, 255, 256, 257, 1280, 4097)


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    print("\nrank diagnostics, largest gaps:", {k: "%.3g" % v for k, v in sorted(WORST.items())})


@pytest.fixture(scope="module")
def chains(gpu):
    X, y, _ = bnr_amd.make_synthetic(dr.N, dr.V, dr.R, seed=3)
    cs = [bnr_amd.Chain(X, y, dr.R, dr.TOT, 99, 1, device=gpu)]
    cs += [bnr_amd.Chain.like(cs[0], 99, c) for c in (2, 3)]
    yield cs
    for c in cs:
        c.close()


def _load(chains, tabs):
    for ch, t in zip(chains, tabs):
        ch.load(t)


def _device(chains, first, nsamp, lag):
    return rc.as_dict(api.device_rank_diagnostics(chains, first - 1, nsamp, lag))


# ------------------------------------------------------------------------------------------------------------------ the rank kernel alone
def _rows(S, seed=7):
    rng = np.random.default_rng([seed, S])
    x = rng.standard_normal(S)
    i = np.arange(S, dtype=np.float64)
    return np.stack([x, np.full(S, -1.5), (rng.random(S) < 0.3).astype(np.float64), np.clip(rng.standard_normal(S), -1.2, 1.2),
                     dr.special_column("denormal", S, 0, rng), dr.special_column("inf_both", S, 0, rng), -2.0 + 3.5 * i / S, 5.0 - 0.25 * i])


def _check_rows(M, gpu):
    S = M.shape[1]
    out = bnr_amd.rank_normalize(M, device=gpu)
    want = np.stack([rankdata(r, method="average") for r in M])
    assert np.array_equal(out["ranks"], want), S
    assert np.array_equal(out["ranks"] * 2, np.round(out["ranks"] * 2))
    ref = _capi.host_ndtri((want - 0.375) / (S + 0.25))
    gap = float(np.max(np.abs(out["z"] - ref) / np.spacing(np.abs(ref))))
    WORST["z ulp"] = max(WORST.get("z ulp", 0.0), gap)
    print("rank kernel S = %d: z within %.3g ulp of bnr_host_ndtri" % (S, gap))
    assert gap <= 4 * K_PHI, (S, gap)
    return out


@pytest.mark.parametrize("S", ROW_LENGTHS)
def test_rank_kernel_against_rankdata(gpu, S):
    M = _rows(S)
    out = _check_rows(M, gpu)
    # each output alone (the other pointer NULL) is the same bits
    r_only, none = _capi.rank_normalize_raw(M, gpu, z=False)
    none2, z_only = _capi.rank_normalize_raw(M, gpu, ranks=False)
    assert none is None and none2 is None and np.array_equal(r_only, out["ranks"]) and np.array_equal(z_only, out["z"])


def test_rank_kernel_indices_past_16_bits(gpu):
    rng = np.random.default_rng(70001)
    _check_rows(np.clip(rng.standard_normal((1, 70001)), -1.2, 1.2), gpu)


def test_rank_kernel_nan_rows(gpu):
    M = np.random.default_rng(11).standard_normal((3, 257))
    M[0, 3] = dr.NAN_POS
    M[2, 256] = dr.NAN_NEG
    out = bnr_amd.rank_normalize(M, device=gpu)
    for k in ("ranks", "z"):
        assert np.isnan(out[k][0]).all() and np.isnan(out[k][2]).all() and not np.isnan(out[k][1]).any(), k
    assert np.array_equal(out["ranks"][1], rankdata(M[1]))
    v = bnr_amd.rank_normalize(M[1], device=gpu)                        # a vector is one row
    assert v["ranks"].shape == (257,) and np.array_equal(v["ranks"], out["ranks"][1]) and np.array_equal(v["z"], out["z"][1])
    for bad in (np.zeros((0, 4)), np.zeros((2, 0)), np.zeros((2, 2, 2))):
        with pytest.raises(ValueError):
            _capi.rank_normalize_raw(bad, gpu)


# ------------------------------------------------------------------------------------------------------------------ device against the restatement
@pytest.mark.parametrize("first,nsamp,lag", rc.WINDOWS)
def test_device_against_the_restatement(chains, first, nsamp, lag):
    _load(chains, rc.tables())
    for nch in (3, 1):
        got = _device(chains[:nch], first, nsamp, lag)
        wins = rc.windows_of(rc.tables()[:nch], first, nsamp)
        gaps = rc.compare(got, rc.host(nch, first, nsamp, lag), wins, (nch, first, nsamp, lag))
        print("device against restatement, %d chain(s), window %s:" % (nch, (first, nsamp, lag)), {k: "%.2g" % v for k, v in gaps.items()})
        for k, v in gaps.items():
            WORST[k] = max(WORST.get(k, 0.0), v)
    d = api.device_rank_diagnostics(chains, first - 1, nsamp, lag)
    assert (d.chains, d.draws, d.max_lag) == (3, 6 * (nsamp // 2), lag) and d.rhat_gamma.shape == (dr.Q,) and d.rhat_xi.shape == (dr.V,)


def test_default_lag_and_partial_requests(chains):
    _load(chains, rc.tables())
    d = api.device_rank_diagnostics(chains, 0, 640)
    assert d.max_lag == 160
    full = _capi.pooled_rank_diag(chains, 1, 640, 160)
    for i, f in enumerate(_capi.RANK_DIAG_FIELDS):                      # one output alone: the same bits, everything else not requested
        one = _capi.pooled_rank_diag(chains, 1, 640, 160, fields=(f,))
        assert all(o is None for j, o in enumerate(one) if j != i)
        assert np.array_equal(one[i], full[i], equal_nan=True), f
    assert np.array_equal(d.full("rhat"), np.fmax(full[0], full[1]), equal_nan=True)


# ------------------------------------------------------------------------------------------------------------------ bitwise properties
def test_bitwise_properties(chains):
    tabs = [dict(t) for t in rc.tables()]
    for t in tabs:
        t["gamma"] = t["gamma"].copy()
        t["gamma"][:, 9, 0] = t["gamma"][:, 0, 0] ** 3                  # column 9 is the cube of column 0
    _load(chains, tabs)
    first, nsamp, lag = 38, 601, 150
    before = [ch.fetch() for ch in chains]
    iters = [ch.iter for ch in chains]
    base = _capi.pooled_rank_diag(chains, first, nsamp, lag)
    again = _capi.pooled_rank_diag(chains, first, nsamp, lag)
    for a, b in zip(base, again):
        assert np.array_equal(a, b, equal_nan=True)
    for blk in (1, 7, 0):
        chains[0].set_option("rank_block_cols", blk)
        for a, b in zip(base, _capi.pooled_rank_diag(chains, first, nsamp, lag)):
            assert np.array_equal(a, b, equal_nan=True), blk
    one = chains[1].rank_diag(first, nsamp, lag)
    for a, b in zip(one, _capi.pooled_rank_diag([chains[1]], first, nsamp, lag)):
        assert np.array_equal(a, b, equal_nan=True)
    f = dict(zip(_capi.RANK_DIAG_FIELDS, base))
    for k in ("rhat_bulk", "ess_bulk", "ess_tail"):
        assert f[k][0] == f[k][9] and not np.isnan(f[k][0]), k
    assert f["ess_mean"][0] != f["ess_mean"][9]
    for ch, b, it in zip(chains, before, iters):                         # nothing of any chain is written
        after = ch.fetch()
        assert ch.iter == it
        for k in b:
            assert np.array_equal(b[k].view(np.uint64), after[k].view(np.uint64)), k


# ------------------------------------------------------------------------------------------------------------------ what the feature is for
SCALE_SEED = 4


def scale_tables(seed=SCALE_SEED):
    """gamma_0: N(0, 1) in two chains and N(0, 9) in the third; gamma_1: the same built on Cauchy draws; everything else the crafted tables"""
    tabs = []
    for c, t in enumerate(rc.tables()):
        t = dict(t)
        t["gamma"] = t["gamma"].copy()
        rng = np.random.default_rng([seed, c])
        s = 3.0 if c == 2 else 1.0
        t["gamma"][:, 0, 0] = s * rng.standard_normal(dr.TOT)
        t["gamma"][:, 1, 0] = s * rng.standard_cauchy(dr.TOT)
        tabs.append(t)
    return tabs


def test_scale_differences_show_in_the_tail_rhat(chains):
    tabs = scale_tables()
    gam = np.stack([t["gamma"][:, :2, 0] for t in tabs], axis=2)
    assert bo.rhat(gam)[0] < 1.05                                        # (the seed: checked on the CPU with the oracle and rank_diag_ref)
    want = rr.diagnostics_all([dr.window(t, 1, dr.TOT)[:, :2] for t in tabs], 160)
    assert want["rhat_tail"][0] > 1.05 and np.isfinite(want["rhat_bulk"][1])
    _load(chains, tabs)
    rg, _rx = _capi.rhat(chains, 3, None, 0, dr.TOT)
    assert rg[0] < 1.05                                                  # the classic split-R-hat does not see the third chain's scale
    d = api.device_rank_diagnostics(chains, 0, dr.TOT)
    print("N(0,1) x 2 + N(0,9): classic rhat %.4f, rhat_bulk %.4f, rhat_tail %.4f; Cauchy: classic %.4f, rhat_bulk %.4f, rhat_tail %.4f"
          % (rg[0], d.rhat_bulk_gamma[0], d.rhat_tail_gamma[0], rg[1], d.rhat_bulk_gamma[1], d.rhat_tail_gamma[1]))
    assert d.rhat_tail_gamma[0] > 1.05 and d.rhat_gamma[0] == d.rhat_tail_gamma[0]
    assert np.isfinite(d.rhat_bulk_gamma[1]) and np.isfinite(d.ess_bulk_gamma[1])
    assert d.rhat_tail_gamma[0] == pytest.approx(want["rhat_tail"][0], rel=rc.RTOL)
    assert d.rhat_bulk_gamma[1] == pytest.approx(want["rhat_bulk"][1], rel=rc.RTOL)


# ------------------------------------------------------------------------------------------------------------------ refusals
def test_refusals(chains):
    _load(chains, rc.tables())
    bad = [dict(first_row=1, nsamp=7, max_lag=2), dict(first_row=1, nsamp=640, max_lag=1), dict(first_row=1, nsamp=640, max_lag=321),
           dict(first_row=600, nsamp=100, max_lag=10), dict(first_row=0, nsamp=100, max_lag=10)]
    for kw in bad:
        for call in (lambda: _capi.pooled_rank_diag(chains, **kw), lambda: chains[0].rank_diag(**kw)):
            with pytest.raises(bnr_amd.BnrError) as e:
                call()
            assert e.value.code == _capi.BNR_ERR_BAD_ARG, kw
    for call in (lambda: _capi.pooled_rank_diag([chains[0], chains[1], chains[0]], 1, 640, 160), lambda: _capi.pooled_rank_diag(chains, 1, 640, 160, fields=()),
                 lambda: chains[0].rank_diag(1, 640, 160, fields=())):
        with pytest.raises(bnr_amd.BnrError) as e:
            call()
        assert e.value.code == _capi.BNR_ERR_BAD_ARG
    with pytest.raises(ValueError):
        api.device_rank_diagnostics(chains, 0, 640, 400)


# ------------------------------------------------------------------------------------------------------------------ Fit
def test_fit_fills_rank_diag(gpu, tmp_path):
    X, y, _ = bnr_amd.make_synthetic(8, 16, 2, seed=5)
    kw = dict(nburn=40, nsamples=80, num_chains=3, seed=17, x_transform=False, suppress_timer=True, psrf_cutoff=np.inf, return_state=False,
              filename=str(tmp_path / "parameters.log"), device=gpu)
    res = bnr_amd.Fit(X, y, 2, rank_diagnostics=True, **kw)
    d = res.rank_diag
    assert d is not None and d.chains == 3 and d.draws == 240 and d.max_lag == 20 and res.state is None
    assert d.rhat_gamma.shape == (136,) and d.ess_tail_xi.shape == (16,) and np.isfinite(d.rhat_gamma).all() and np.all(d.ess_bulk_gamma > 0)
    assert bnr_amd.RankDiagnose(res) is d
    assert bnr_amd.Fit(X, y, 2, rank_diagnostics=True, ess_max_lag=10, **kw).rank_diag.max_lag == 10
    assert bnr_amd.Fit(X, y, 2, rank_diagnostics=False, **kw).rank_diag is None
