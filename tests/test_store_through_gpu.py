"""The sweep's cross-launch outputs written through the L2 (BNR_STORE_THROUGH, csrc/bnr_kernels.h) change no bit of any table.  Run with -m gpu on an MI355X.

tests/golden/store_through_digests.json holds, per case, member and table column, the SHA-256 (first 16 hex digits, the digest of tools/table_digest.py
taken per column) of four sweeps from the prior, recorded from the build BEFORE any store was changed (python tests/test_store_through_gpu.py --record).
The cases are the smallest shapes that reach every changed store:
  one            n = 100, V = 30, R = 3, a chain alone: k_chol_step<bnr_one>, the small-block update role, one eighth per reduction workgroup
  g3_epw4/_epw1  n = 200, V = 50, R = 5 as a group of 3: k_chol_step<bnr_few> at steps p >= 2, the super-block update role, reduce_epw 4 and 1
  g9             the same shape as a group of 9: k_chol_step<bnr_many> at every step
  g3_bool_i8     the same shape with a Bool model matrix and gram_i8 on: k_sdigits and k_gram_i8's epilogue
  g3_wide        a group of 3 with wide_backproj = 1: k_backproj64
  g3_sep_reduce  fuse_reduce = 0: k_gram_reduce writes E and Y = I
Required: every column's digest equals the recorded one; every member of a group is bitwise the chain run alone; no failure counter moves."""
import hashlib
import json
import os
import sys

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "store_through_digests.json")
SEED, SWEEPS = 11, 4
CASES = {
    "one": dict(n=100, V=30, R=3, chains=1, binary=False, opts={"reduce_epw": 1}),
    "g3_epw4": dict(n=200, V=50, R=5, chains=3, binary=False, opts={"reduce_epw": 4}),
    "g3_epw1": dict(n=200, V=50, R=5, chains=3, binary=False, opts={"reduce_epw": 1}),
    "g9": dict(n=200, V=50, R=5, chains=9, binary=False, opts={}),
    "g3_bool_i8": dict(n=200, V=50, R=5, chains=3, binary=True, opts={}),
    "g3_wide": dict(n=200, V=50, R=5, chains=3, binary=False, opts={"wide_backproj": 1}),
    "g3_sep_reduce": dict(n=200, V=50, R=5, chains=3, binary=False, opts={"factor_variant": 0, "fuse_reduce": 0}),
}


def _data(case):
    import bnr_amd
    if case["binary"]:
        rng = np.random.default_rng(5)
        q = case["V"] * (case["V"] + 1) // 2
        return bnr_amd.XInput(np.asfortranarray(rng.random((case["n"], q)) < 0.5), False), rng.normal(size=case["n"])
    X, y, _ = bnr_amd.make_synthetic(case["n"], case["V"], case["R"], seed=SEED)
    return X, y


def _run(case, X, y, ids, opts):
    """the chains `ids` (one: alone; several: one lockstep group) for SWEEPS sweeps from the prior: per chain (table, counters before, counters after)"""
    import bnr_amd
    tot = SWEEPS + 1
    chains = [bnr_amd.Chain(X, y, case["R"], tot, SEED, ids[0])]
    chains += [bnr_amd.Chain.like(chains[0], SEED, c, tot) for c in ids[1:]]
    runner = bnr_amd.Group(chains) if len(chains) > 1 else chains[0]
    try:
        for ch in chains:
            ch.init_prior()
            if case["binary"]:
                ch.set_option("gram_i8", 1)
        for k, v in opts.items():
            runner.set_option(k, v)
        before = [ch.counters() for ch in chains]
        runner.run(2, tot, tot)
        return [(ch.fetch(), b, ch.counters()) for ch, b in zip(chains, before)]
    finally:
        if len(chains) > 1:
            runner.close()
        for ch in chains:
            ch.close()


def _digests(table):
    return {k: hashlib.sha256(np.ascontiguousarray(table[k]).tobytes()).hexdigest()[:16] for k in sorted(table)}


def _case_digests(name):
    case = CASES[name]
    X, y = _data(case)
    ids = list(range(1, case["chains"] + 1))
    return case, X, y, ids, _run(case, X, y, ids, case["opts"])


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_tables_are_bitwise_those_of_the_plain_stores(gpu, name):
    with open(GOLDEN) as f:
        want = json.load(f)[name]
    case, X, y, ids, got = _case_digests(name)
    assert len(want) == len(got)
    for m, (table, before, after) in enumerate(got):
        assert before == after, (name, "member", m, "a failure counter moved", before, after)
        d = _digests(table)
        assert sorted(d) == sorted(want[m]), (name, "member", m, "columns")
        for k in sorted(d):
            assert d[k] == want[m][k], (name, "member", m, "column", k)
    if len(ids) > 1:
        for m, c in enumerate(ids):
            (alone, before, after), = _run(case, X, y, [c], {k: v for k, v in case["opts"].items() if k != "reduce_epw"})
            assert before == after, (name, "chain", c, "alone: a failure counter moved", before, after)
            for k in sorted(alone):
                assert np.array_equal(np.ascontiguousarray(alone[k]).view(np.uint8), np.ascontiguousarray(got[m][0][k]).view(np.uint8)), (name, "member", m, "column", k, "differs from the chain alone")


if __name__ == "__main__":
    if sys.argv[1:2] != ["--record"]:
        sys.exit("usage: python tests/test_store_through_gpu.py --record [FILE]   (with the build whose tables are the reference)")
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    path = sys.argv[2] if len(sys.argv) > 2 else GOLDEN
    out = {name: [_digests(t) for t, _, _ in _case_digests(name)[4]] for name in sorted(CASES)}
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("recorded", path, {k: len(v) for k, v in out.items()})
