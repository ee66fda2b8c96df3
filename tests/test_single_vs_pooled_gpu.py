"""GPU test (run with -m gpu on an MI355X) that every single-chain analysis call is its pooled twin on a list of one chain, bit for bit, at the
C entry points (bnr_chain_* forwards to bnr_chains_*) and in the ctypes layer (Chain.<call> and pooled_<call> share one body): summary,
predict for a model matrix and for adjacency matrices, loglik_stats, loo, loo_predict, rank_diag, hdi, inclusion, and device_summary
against device_summary_pooled.  Compared on the fields both return; NaNs compare by their bits.

The shape of smoke(): make_synthetic(40, 8, 3), two chains of 64 rows run to the end, window 17 .. 64 (nsamp = 48, max_lag = 12)."""
import numpy as np
import pytest

import bnr_amd
from bnr_amd import _capi

pytestmark = pytest.mark.gpu
N, V, R, TOT, SEED = 40, 8, 3, 64, 4242
FIRST, NSAMP, MAX_LAG = 17, 48, 12
K_LO, K_HI = 3, 46
M_NEW = 9                                       # new rows: fewer than a 32-row tile


@pytest.fixture(scope="module")
def chains(gpu):
    X, y, _ = bnr_amd.make_synthetic(N, V, R, seed=7)
    cs = [bnr_amd.Chain(X, y, R, TOT, SEED, 1, device=gpu)]
    cs.append(bnr_amd.Chain.like(cs[0], SEED, 2))
    for ch in cs:
        ch.init_prior()
        ch.run(2, TOT, TOT)
    yield cs
    for ch in cs:
        ch.close()


@pytest.fixture(scope="module")
def new_rows():
    Xn, yn, _ = bnr_amd.make_synthetic(M_NEW, V, R, seed=8)
    return Xn, yn


def _bits(a):
    if a is None or isinstance(a, int):
        return a
    return np.ascontiguousarray(a).tobytes()


def _same(one, pooled, what):
    assert len(one) <= len(pooled), what
    for j, (a, b) in enumerate(zip(one, pooled)):
        assert (a is None) == (b is None) and _bits(a) == _bits(b), (what, j)
        assert a is None or isinstance(a, int) or (a.shape == b.shape and a.dtype == b.dtype), (what, j)


def test_summary(chains):
    for ch in chains:
        _same(ch.summary(FIRST, NSAMP, K_LO, K_HI), _capi.pooled_summary([ch], FIRST, NSAMP, K_LO, K_HI), "summary")
        one, pooled = bnr_amd.device_summary(ch, FIRST - 1, NSAMP, 90), bnr_amd.device_summary_pooled([ch], FIRST - 1, NSAMP, 90)
        assert sorted(one) == sorted(pooled) and one["interval"] == pooled["interval"] == 90
        for k in ("estimate", "lower_bound", "upper_bound", "probability"):
            assert _bits(one[k]) == _bits(pooled[k]), k


def test_predict_and_predict_from_matrices(chains, new_rows):
    Xn, yn = new_rows
    mats = [bnr_amd.create_lower_tri(Xn[i], V) for i in range(M_NEW)]
    for ch in chains:
        for X, xt in ((Xn, False), (Xn.astype(np.float32), False), (mats, True)):
            for y in (yn, None):
                one = ch.predict(X, FIRST, NSAMP, K_LO, K_HI, y=y, x_transform=xt)
                pooled = _capi.pooled_predict([ch], X, FIRST, NSAMP, K_LO, K_HI, y=y, x_transform=xt)
                assert len(one) == 5 and len(pooled) == 8 and pooled[5:] == (None, None, None)
                _same(one, pooled, ("predict", xt, y is None))
                assert (one[3] is None) == (y is None)


def test_loglik_stats_loo_and_loo_predict(chains):
    for ch in chains:
        one = ch.loglik_stats(FIRST, NSAMP)
        assert len(one) == 2
        _same(one, _capi.pooled_loglik_stats([ch], FIRST, NSAMP), "loglik_stats")
        for r_eff in (None, 0.6):
            _same(ch.loo(FIRST, NSAMP, r_eff), _capi.pooled_loo([ch], FIRST, NSAMP, r_eff), ("loo", r_eff))
            one = ch.loo_predict(FIRST, NSAMP, r_eff, 0.05, 0.95)
            assert len(one) == len(_capi.LOO_PREDICT_FIELDS) and all(a is not None and a.shape == (N,) for a in one)
            _same(one, _capi.pooled_loo_predict([ch], FIRST, NSAMP, r_eff, 0.05, 0.95), ("loo_predict", r_eff))


def test_rank_diag_hdi_and_inclusion(chains):
    for ch in chains:
        one = ch.rank_diag(FIRST, NSAMP, MAX_LAG)
        assert all(a is not None and a.shape == (ch.q + ch.V,) for a in one)
        _same(one, _capi.pooled_rank_diag([ch], FIRST, NSAMP, MAX_LAG), "rank_diag")
        some = ("rhat_bulk", "ess_tail")
        _same(ch.rank_diag(FIRST, NSAMP, MAX_LAG, some), _capi.pooled_rank_diag([ch], FIRST, NSAMP, MAX_LAG, some), "rank_diag, two fields")
        one = ch.hdi(FIRST, NSAMP, (0.5, 0.9))
        assert one[0].shape == (2, ch.q + ch.V)
        _same(one, _capi.pooled_hdi([ch], FIRST, NSAMP, (0.5, 0.9)), "hdi")
        _same(ch.hdi(FIRST, NSAMP, (), ("median", "p_pos")), _capi.pooled_hdi([ch], FIRST, NSAMP, (), ("median", "p_pos")), "hdi, no level")
        for which in (0, 1):
            one = ch.inclusion(FIRST, NSAMP, which, 5)
            assert one[3] >= 1 and one[5][0] >= 1
            _same(one, _capi.pooled_inclusion([ch], FIRST, NSAMP, which, 5), ("inclusion", which))


def test_refusals_read_the_same(chains):
    """the single-chain entry points keep their own messages: the row window, and the order statistics against nsamp"""
    ch = chains[0]
    for call in (lambda: ch.summary(FIRST, NSAMP + 1, K_LO, K_HI), lambda: ch.rank_diag(FIRST + 1, NSAMP, MAX_LAG), lambda: ch.loo(0, NSAMP)):
        with pytest.raises(_capi.BnrError, match="row window outside the table"):
            call()
    with pytest.raises(_capi.BnrError, match="order statistics must be between 1 and nsamp"):
        ch.summary(FIRST, NSAMP, K_LO, NSAMP + 1)
    with pytest.raises(_capi.BnrError, match="order statistics must be between 1 and nsamp"):
        ch.predict(np.zeros((1, ch.q)), FIRST, NSAMP, 0, K_HI)
    with pytest.raises(_capi.BnrError, match="order statistics must be between 1 and nchains \\* nsamp"):
        _capi.stacked_summary([ch], [1.0], FIRST, NSAMP, K_LO, NSAMP + 1)
