"""k_gram8's staging (two register sets, batch b + 2 loaded at the top of batch b) at the shapes where its loops begin and end.

A K-group's loop runs two batches of 8 columns per trip, with an odd batch behind the trips, and loads two batches ahead without a clamp.  The
cases take every way through it:
  n = 70  (n_pad 128: two diagonal tiles and one full tile -- full blocks, diagonal blocks and the dead blocks of the diagonal tiles all run)
  n = 190 (n_pad 192: six tiles)
  V = 5, 7, 9, 10: one K slice of 16, 32, 48, 64 columns = 1, 2, 3, 4 batches per K-group -- no trip at all, one trip, one trip + the odd batch, two trips
  V = 37: q = 703 in several K slices, the last one with a single column of padding (q_pad - q = 1 with 11 slices)
  V = 31 in 31 slices and V = 63 in 7 slices (BNR_GRAM_KSPLIT): q = q_pad exactly (496 = 31 x 16, 2016 = 7 x 288), so the last K slice ends where X and S
  end and everything its last batches load ahead comes from the zeros behind them; one batch per K-group, and 18 (nine trips).  No V up to
  1000 has q = q_pad at these n_pad under the split the library chooses by itself, hence the forced split for these two.
(the batches per K-group and q_pad are asserted from debug_dims where they do not depend on the card's number of compute units.)

Every case runs three rows (two sweeps) for chains 1, 2, 3 alone and as one lockstep group, with gram_variant 8 (k_gram8<bnr_one> / <bnr_many>)
and 16 (k_gram, 16-column batches, the same summation order).  Asserted:
  - all counters zero in every run;
  - the partial tiles of the last Gram (debug_copy(3)) are bitwise equal under variants 8 and 16, alone and in the group;
  - every member of the group is bitwise the chain alone: partial tiles and the whole table;
  - the partial tiles summed are the exact Gram X diag(S) X' (tests/linalg_ref.py; S = the row the last sweep read) within
    gamma_m (|X| S |X|'), m = q + ksplit + 4: any order of the f64 FMAs, the K-groups and the slices (the bound of tests/test_gamma_linalg_gpu.py),
    and the pad rows are zero."""
import os

import numpy as np
import pytest

import bnr_amd
from oracle import bnr_oracle as bo
import linalg_ref as lr

pytestmark = pytest.mark.gpu
TOT, R, SEED = 3, 2, 23
CASES = [  # n, V, forced K split (None: the library's), batches per K-group (None: depends on the card)
    (70, 5, None, 1), (70, 7, None, 2), (70, 9, None, 3), (70, 10, None, 4), (190, 9, None, 3), (190, 10, None, 4),
    (70, 37, None, None), (70, 31, 31, 1), (190, 63, 7, 18),
]
_DONE = {}


class Case:
    def __init__(self, n, V, ksplit, nbatch):
        self.n, self.V, self.ksplit, self.nbatch = n, V, ksplit, nbatch
        self.q = V * (V + 1) // 2
        rng = np.random.default_rng(1000 * n + V)
        self.X = np.asfortranarray(rng.integers(-128, 129, size=(n, self.q)) / 16.0)     # dyadic: linalg_ref's Gram of it is exact
        self.y = rng.normal(size=n) * 2.0
        self.alone = {}                                                                   # (chain id, variant) -> (partial tiles, table, dims)

    def chains(self, ids):
        old = os.environ.get("BNR_GRAM_KSPLIT")
        if self.ksplit:
            os.environ["BNR_GRAM_KSPLIT"] = str(self.ksplit)                              # read when a chain is created
        try:
            out = [bnr_amd.Chain(bnr_amd.XInput(self.X, False), self.y, R, TOT, SEED, ids[0])]
            out += [bnr_amd.Chain.like(out[0], SEED, c) for c in ids[1:]]
        finally:
            if self.ksplit:
                if old is None:
                    del os.environ["BNR_GRAM_KSPLIT"]
                else:
                    os.environ["BNR_GRAM_KSPLIT"] = old
        for ch in out:
            ch.init_prior()
        return out

    def check_dims(self, dm):
        assert dm["n_pad"] == 64 * ((self.n + 63) // 64)
        per_group = dm["q_pad"] // dm["ksplit"] // 16
        print("n=%d V=%d q=%d: q_pad=%d ksplit=%d, %d batches per K-group" % (self.n, self.V, self.q, dm["q_pad"], dm["ksplit"], per_group))
        if self.nbatch is not None:
            assert per_group == self.nbatch, (dm, self.nbatch)
        if self.ksplit:
            assert dm["ksplit"] == self.ksplit and dm["q_pad"] == self.q, dm
        elif self.nbatch is None:
            assert dm["ksplit"] > 1, dm

    def lone(self, cid, variant):
        if (cid, variant) not in self.alone:
            ch, = self.chains([cid])
            ch.set_option("gram_variant", variant)
            assert ch.run(2, TOT, TOT) == TOT + 1
            zero_counters(ch, (self.n, self.V, cid, variant, "alone"))
            dm = ch.debug_dims()
            self.check_dims(dm)
            self.alone[(cid, variant)] = (partials(ch, dm), ch.fetch(), dm)
            ch.close()
        return self.alone[(cid, variant)]


def case(*key):
    if key not in _DONE:
        _DONE[key] = Case(*key)
    return _DONE[key]


def partials(ch, dm):
    return ch.debug_copy(3, dm["ksplit"] * (dm["ntile"] * (dm["ntile"] + 1) // 2) * 4096)


def zero_counters(ch, what):
    c = ch.counters()
    assert c["jitter"] == 0 and c["nan_w"] == 0 and c["sampler_cap"] == 0 and c["chol_fail"] == 0 and not any(c["where"]), (what, c)


def within_the_exact_gram(cs, P, table, dm, what):
    n, ks, nt = cs.n, dm["ksplit"], dm["ntile"]
    S = table["S"][TOT - 2, :, 0]                                          # the last sweep (row TOT) reads S of row TOT - 1
    G = lr.tiles_to_lower(lr.sum_partials_ld(P.reshape(ks, -1, 4096)), nt)
    assert not np.any(G[n:]), (what, "pad rows of the Gram are not zero")
    low = np.tril(np.ones((n, n), dtype=bool))
    Gs, Ge = lr.exact_gram(cs.X, S)
    r = lr.check_gram_f64(np.where(low, G[:n, :n], 0), np.where(low, Gs, 0), Ge, lr.abs_gram(cs.X, S), cs.q + ks + 4)
    print("ratio gram_f64 %.3e  %s" % (r, what))
    assert r < 1.0, (what, r)


@pytest.mark.parametrize("n,V,ksplit,nbatch", CASES)
def test_a_chain_alone(gpu, n, V, ksplit, nbatch):
    cs = case(n, V, ksplit, nbatch)
    for cid in (1, 2, 3):
        P8, t8, dm = cs.lone(cid, 8)
        P16, t16, _ = cs.lone(cid, 16)
        what = "n=%d V=%d chain %d alone" % (n, V, cid)
        assert np.array_equal(P8, P16), (what, "partial tiles of k_gram8<bnr_one> against k_gram<bnr_one, 2>")
        for k in bo.COLUMNS:
            assert np.array_equal(t8[k], t16[k]), (what, k)
        within_the_exact_gram(cs, P8, t8, dm, what)


@pytest.mark.parametrize("n,V,ksplit,nbatch", CASES)
def test_a_group_of_three(gpu, n, V, ksplit, nbatch):
    cs = case(n, V, ksplit, nbatch)
    ids = (1, 2, 3)
    got = {}
    for variant in (8, 16):
        chains = cs.chains(ids)
        g = bnr_amd.Group(chains)
        g.set_option("gram_variant", variant)
        assert g.run(2, TOT, TOT) == TOT + 1
        for cid, ch in zip(ids, chains):
            zero_counters(ch, (n, V, cid, variant, "group"))
            dm = ch.debug_dims()
            cs.check_dims(dm)
            got[(cid, variant)] = (partials(ch, dm), ch.fetch(), dm)
        g.close()
        for ch in chains:
            ch.close()
    for cid in ids:
        what = "n=%d V=%d chain %d in a group of three" % (n, V, cid)
        P8, t8, dm = got[(cid, 8)]
        assert np.array_equal(P8, got[(cid, 16)][0]), (what, "partial tiles of k_gram8<bnr_many> against k_gram<bnr_many, 2>")
        Pa, ta, _ = cs.lone(cid, 8)
        assert np.array_equal(P8, Pa), (what, "partial tiles against the chain alone")
        for k in bo.COLUMNS:
            assert np.array_equal(t8[k], ta[k]), (what, k, "against the chain alone")
            assert np.array_equal(got[(cid, 16)][1][k], ta[k]), (what, k, "variant 16 against the chain alone")
        within_the_exact_gram(cs, P8, t8, dm, what)
