"""Launch 0 of the one-panel factorization with the reduction of the Gram's K-split partial tiles inside (fuse_reduce, bnr_reduce_parts in
csrc/bnr_kernels.h) against the unchanged separate pass (fuse_reduce = 0: k_gram_reduce, Y = I written up front).  Run with -m gpu on an MI355X.

A reduction workgroup of launch 0 sums 1, 2 or 4 eighths of a partial tile (reduce_epw; 0 = the host's rule; a chain alone always runs 1, whatever
the option says -- its cases still go through all settings), all slices of a batch in flight: 8 slices per batch, 4 when it holds four eighths.  So the K splits here are 1, 3 (inside one batch at every width), 7 (two batches of 4, one of 8),
10 and 13 (two batches of 8; three and four of 4), at n_pad = 64 (one tile, two panels), 128 (three tiles) and 256 (ten tiles), for a chain alone, a
group of three and a group of nine (which takes k_chol_step<bnr_many> at every step).

Every case runs the same chains from the same prior four or five times -- separate pass, then reduce_epw 0, 1, 2, 4 -- two consecutive sweeps each,
WITHOUT re-creating the chains: each run starts on the E the run before left behind (L and Y = L^-T), and the second sweep of a run on the first
sweep's, so equal bits also say that nothing reads a block before its first touch of the sweep.  Required per member:
  * every column of the table rows of both sweeps bitwise equal to the separate pass's;
  * E after the second sweep bitwise equal on the matrix part from column 32 on (the lower 64 x 64 tiles: all that any kernel ever writes there;
    the first 32 columns differ by design -- launch 0's panel workgroups keep the unfactored diagonal block to themselves) and on the block-upper
    triangle of Y (linalg_ref.block_upper_Y);
  * the run returns without error -- a reduction stamp that is not this sweep's counts into counters[8], which fails the run ("stream ordering
    violated") --, and no factorization failure is counted."""
import numpy as np
import pytest

import bnr_amd
import linalg_ref as lr
from oracle import bnr_oracle as bo

pytestmark = pytest.mark.gpu
SHAPES = [  # n, V, the K split bnr_host_gram_plan gives at 256 compute units
    (40, 8, 1), (100, 12, 1), (100, 30, 7), (100, 40, 13), (200, 20, 3), (200, 36, 10)]
R, SEED = 3, 5


def _ksplit(n, V, ncu=256):
    plan = (bnr_amd._capi.C.c_int32 * 4)()
    bnr_amd._capi.check(bnr_amd._capi.lib().bnr_host_gram_plan(n, V, ncu, plan))
    return plan[0]


def _snapshot(chains):
    out = []
    for ch in chains:
        assert ch.counters()["chol_fail"] == 0
        n_pad = ch.debug_dims()["n_pad"]
        ld = 2 * n_pad + 32
        E = ch.debug_copy(0, ld * n_pad)
        M = E.reshape(n_pad, ld).T[:n_pad, :]                       # matrix part, [row, column]
        t = np.arange(n_pad) // 64
        written = (t[:, None] >= t[None, :]) & (np.arange(n_pad)[None, :] >= 32)
        out.append((ch.fetch(2, 3), np.where(written, M, 0.0), lr.block_upper_Y(E, n_pad, ld)))
    return out


def _same(got, want, what):
    for m, ((tg, Mg, Yg), (tw, Mw, Yw)) in enumerate(zip(got, want)):
        for k in bo.COLUMNS:
            assert np.array_equal(tg[k], tw[k]), (what, "member", m, "column", k)
        assert np.array_equal(Mg.view(np.uint64), Mw.view(np.uint64)), (what, "member", m, "E, matrix part from column 32 on")
        assert np.array_equal(Yg.view(np.uint64), Yw.view(np.uint64)), (what, "member", m, "Y, block upper triangle")


def _modes(n, V, nchains, modes):
    """the same chains from the same prior under every option set of `modes`, two sweeps each; one snapshot per mode"""
    X, y, _ = bnr_amd.make_synthetic(n, V, R, seed=SEED)
    chains = [bnr_amd.Chain(X, y, R, 4, SEED, 1)]
    chains += [bnr_amd.Chain.like(chains[0], SEED, c, 4) for c in range(2, nchains + 1)]
    runner = bnr_amd.Group(chains[1:] + chains[:1]) if nchains > 1 else chains[0]
    snaps = []
    try:
        for opts in modes:
            for ch in chains:
                ch.init_prior()
            for k, v in opts.items():
                runner.set_option(k, v)
            # counters[8] == 0, asserted through the status: counters() hands out the first 8 words only, and status_of (csrc/bnr_hip.hip) turns counters[8] > 0
            # of ANY member into BNR_ERR_HIP "stream ordering violated", which run raises as BnrError
            runner.run(2, 3, 3)
            snaps.append(_snapshot(chains))
    finally:
        if nchains > 1:
            runner.close()
        for ch in chains:
            ch.close()
    return snaps


@pytest.mark.parametrize("nchains", [1, 3, 9])
@pytest.mark.parametrize("n,V,ks", SHAPES)
def test_reduction_inside_launch_0_equals_the_separate_pass(gpu, n, V, ks, nchains):
    assert _ksplit(n, V) == ks, (n, V, _ksplit(n, V))
    modes = [{"factor_variant": 0, "fuse_reduce": 0}] + [{"fuse_reduce": 1, "reduce_epw": e} for e in (0, 1, 2, 4)]
    snaps = _modes(n, V, nchains, modes)
    for opts, got in zip(modes[1:], snaps[1:]):
        _same(got, snaps[0], (n, V, nchains, opts))


def test_reduction_inside_launch_0_issued_eagerly(gpu):
    """graph = 0: the same launches issued one by one instead of replayed from a captured graph (three tiles, two batches of slices, a group of three)"""
    modes = [{"factor_variant": 0, "fuse_reduce": 0, "graph": 0}] + [{"fuse_reduce": 1, "reduce_epw": e} for e in (0, 1, 2, 4)]
    snaps = _modes(100, 40, 3, modes)
    for opts, got in zip(modes[1:], snaps[1:]):
        _same(got, snaps[0], ("eager", opts))


def test_reduce_epw_takes_only_its_four_values(gpu):
    X, y, _ = bnr_amd.make_synthetic(40, 8, R, seed=SEED)
    ch = bnr_amd.Chain(X, y, R, 4, SEED, 1)
    try:
        for bad in (-1, 3, 8):
            with pytest.raises(bnr_amd.BnrError, match="reduce_epw"):
                ch.set_option("reduce_epw", bad)
    finally:
        ch.close()
