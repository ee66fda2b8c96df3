"""Lockstep groups of more than eight chains (run with -m gpu on an MI355X).

bnr_group_create takes up to 1024 chains and a fit puts all the chains of a GPU into one group, but every other group in the suite has 2, 3, 5
or 8 members.  From nine members on the sweep runs code that no smaller group reaches: k_chol_step<bnr_many> at the panel steps p >= 2 (groups
of 2..8 get the by-value bnr_few argument there), the second and later batches of eight members in k_xpass_group / k_xpass_group2 (a short last
batch takes the low arms of bnr_xg_dispatch), the chain / slot decoding of the one-dimensional grids (gr % nchains, (gr / nchains) * 8 + gx)
with a chain count that is coprime with 8, the host's choices that depend on the member count (room, freecu and spw of launch_chol, `wide` of
launch_gram, many_rounds and nslot of launch_backproj), and the status words of the members behind the eighth.

For every group here (N members, chain ids 1..N in an order of the test's choosing):
  1. every member's table equals, column by column and bit for bit, the table of the same chain id run alone in a fresh Chain (on the same Gram
     pipe and in the same factorization family: those, and only those, are allowed to differ by rounding);
  2. the chains with ids 1, 9 and N, and the members at positions 0, 8 and N - 1, agree with the CPU oracle (test_gpu_parity's tolerance);
  3. no member counts a failed factorization or a NaN W.

No counter tells which kernel ran, so the dispatch rules of launch_chol, launch_gram, launch_xpass and launch_backproj (bnr_hip.hip) are restated
below (chol_plan, gram_plan, xpass_plan, backproj_plan); every test asserts from the restatement, before the device run, that its shape reaches
the branch it is there for, and prints what it reached.  The shapes were chosen for the MI355X's 256 compute units: on a card with another count
the tests skip, with that reason and no other.  tests/test_host_cpu.py holds the same expectations at 256 units without a GPU."""
import numpy as np
import pytest

import bnr_amd
import linalg_ref as lr
from oracle import bnr_oracle as bo
from test_gamma_linalg_gpu import _pivot_case, _plain_split, _run_case, _set_S0, _spw_per_launch, binary_X
from test_gpu_parity import assert_tables_close

pytestmark = pytest.mark.gpu
NCU = 256                                     # the compute units the shapes below were worked out for
SIZES = (9, 12, 16, 17)                       # last batches of 1, 4, 8, 1 members in the X pass; 9 and 17 are coprime with the 8 of the task maps
HOW = {9: "swap", 12: "up", 16: "up", 17: "down"}


# ------------------------------------------------------------------------------------------------------------------ the launch rules, restated
def n_pad_of(n):
    return 64 * ((n + 63) // 64)


def chol_plan(nb, n, cap, fv, ncu=NCU):
    """launch_chol: one dict per launch -- arg (the descriptor argument: bnr_one, bnr_few by value, bnr_many), form (reduce: launch 0 of the
    one-panel family; block: one 32 x 32 block per workgroup; super: 64 x 64 super blocks), spw, freecu.  spw comes from _spw_per_launch."""
    n_pad = n_pad_of(n)
    nbk = n_pad // 32
    many = "bnr_one" if nb == 1 else "bnr_many"
    if fv in (2, 3) or (fv < 0 and n_pad >= 1024):
        spw = _spw_per_launch(nb, nbk, cap, 3, ncu) if fv != 2 else None
        assert fv != 2 or nb * nbk >= ncu or nbk > 24, "variant 2 is restated only where spw = 1 (no CU left free)"
        return [dict(p=P, arg=many, form="super", spw=spw[P] if spw else 1, freecu=ncu - nb * nbk) for P in range(nbk // 2)]
    spw = _spw_per_launch(nb, nbk, cap, 0, ncu)
    few = 2 <= nb <= 8
    out = [dict(p=0, arg=many, form="reduce", spw=1, freecu=ncu - nb * (nbk + 1))]
    for p in range(1, nbk):
        s = spw[p - 1]
        out.append(dict(p=p, arg="bnr_few" if (few and p >= 2) else many, form="block" if s is None else "super", spw=1 if s is None else s,
                        freecu=ncu - nb * (nbk + 1)))
    return out


def gram_plan(nb, n, V, variant=0, i8=False, ncu=NCU):
    """launch_gram: the kernel, the K split (before the window guard, which acts at tens of thousands of columns only) and the grid"""
    nt = n_pad_of(n) // 64
    ntl, ks = nt * (nt + 1) // 2, _plain_split(n, V, ncu)
    if i8 and variant == 0:
        kernel = "k_gram_i8"
    else:
        wide = variant == 16 if variant else nb * ntl * ks <= 2 * ncu
        kernel = "k_gram<2>" if wide else "k_gram8"
    return dict(kernel=kernel, ksplit=ks, tasks=ntl * ks, grid=8 * ((ntl * ks + 7) // 8) * nb)


def xpass_plan(nb, n, V, group_xpass=-1, shares_x=True):
    """launch_xpass (which = 3, a sweep's X pass) and chain_build's column partition"""
    n_pad, q = n_pad_of(n), V * (V + 1) // 2
    nblk = max(min((q + 31) // 32, 256), (q + 255) // 256)
    chunk = (q + nblk - 1) // nblk
    nblk = (q + chunk - 1) // chunk
    big_x = n_pad * q * 8 >= 8 << 20
    grouped = (group_xpass == 1 or (group_xpass < 0 and big_x)) and nb >= 2 and shares_x and 16 * chunk * 8 <= 48 * 1024
    kernel = ("k_xpass_group2" if chunk > 64 else "k_xpass_group") if grouped else "k_xpass"
    slices = (n_pad + 255) // 256
    return dict(kernel=kernel, chunk_x=chunk, nblk_x=nblk, slices=slices, last_slice=n_pad - 256 * (slices - 1), last_chunk=q - chunk * (nblk - 1),
                batches=[min(8, nb - cb) for cb in range(0, nb, 8)] if grouped else None, grid=nblk * slices if grouped else 8 * ((nblk + 7) // 8) * nb)


def backproj_plan(nb, n, V, R, wide_backproj=-1, ncu=NCU):
    """launch_backproj of a sweep (flags & 3 == 3)"""
    q = V * (V + 1) // 2
    nblk = (q + 31) // 32
    lds64 = (n_pad_of(n) + 64 + R * 65 + (3 * R + 1) * 65) * 8 + (2 * 11 * 64 + 3 * 64) * 8 + 2 * 64 * 4
    many_rounds = nb * nblk > ncu if nb > 1 else nb * nblk >= 8 * ncu
    if lds64 <= 124 * 1024 and (wide_backproj == 1 or (wide_backproj < 0 and many_rounds)):
        return dict(kernel="k_backproj64", nslot=None, chunks=nb * nblk, grid=8 * (((nblk + 1) // 2 + 7) // 8) * nb)
    return dict(kernel="k_backproj", nslot=8 if nb * nblk <= 2 * ncu else 2, chunks=nb * nblk, grid=8 * ((nblk + 7) // 8) * nb)


# ---- what each shape of the issue is there for (asserted at 256 units by tests/test_host_cpu.py, and on the card before every device run)
def expect_chol_one_panel(ncu=NCU):
    """case 1: every step p >= 2 of a group of nine or more takes bnr_many; both update forms; spw 4 at cap 4; no CU left free"""
    a = chol_plan(9, 100, 4, 0, ncu)
    assert [s["form"] for s in a] == ["reduce", "block", "block", "block"] and all(s["arg"] == "bnr_many" for s in a), a
    b = chol_plan(9, 370, 4, 0, ncu)
    forms = [s["form"] for s in b if s["p"] >= 2]
    assert b[2]["form"] == "super" and "block" in forms and "super" in forms and forms[-1] == "block", forms
    assert all(s["arg"] == "bnr_many" for s in b) and any(s["arg"] == "bnr_few" for s in chol_plan(8, 370, 4, 0, ncu))
    c1, c4 = chol_plan(16, 370, 1, 0, ncu), chol_plan(16, 370, 4, 0, ncu)
    assert c4[5]["freecu"] == ncu - 16 * 13 > 0 and c4[5]["spw"] == 4 and max(s["spw"] for s in c1) == 1, (c1, c4)
    d = chol_plan(17, 470, 4, 0, ncu)
    assert d[0]["freecu"] < 0 and all(s["spw"] == 1 for s in d) and "super" in [s["form"] for s in d], d
    return dict(n100=[s["form"] for s in a], n370=[s["form"] for s in b], spw_cap4=[s["spw"] for s in c4], freecu_17x470=d[0]["freecu"])


def expect_chol_two_panel(ncu=NCU):
    """case 2: sixteen chains of 22 panels leave no CU free (spw = 1 whatever the cap)"""
    out = {}
    for fv in (2, 3):
        p = chol_plan(16, 700, 4, fv, ncu)
        assert len(p) == 11 and p[0]["freecu"] < 0 and all(s["spw"] == 1 and s["arg"] == "bnr_many" for s in p), p
        out[fv] = p[0]["freecu"]
    return out


def expect_xpass(ncu=NCU):
    """case 3: short chunks -> k_xpass_group with a short last row slice, chunks of 65 columns -> k_xpass_group2; last batches of 1, 4, 8, 1"""
    out = {}
    for nb in SIZES:
        a, b = xpass_plan(nb, 370, 12, 1), xpass_plan(nb, 40, 181, 1)
        assert a["kernel"] == "k_xpass_group" and a["chunk_x"] <= 64 and a["slices"] == 2 and a["last_slice"] < 256, a
        assert b["kernel"] == "k_xpass_group2" and b["chunk_x"] == 65 and b["last_chunk"] < 65, b
        assert a["batches"] == b["batches"] and len(a["batches"]) >= 2 and a["batches"][-1] == {9: 1, 12: 4, 16: 8, 17: 1}[nb], a
        assert xpass_plan(nb, 370, 12, 0)["kernel"] == xpass_plan(nb, 40, 181, 0)["kernel"] == "k_xpass"
        out[nb] = (a["kernel"], a["chunk_x"], b["kernel"], b["chunk_x"], a["batches"])
    return out


GRAM_SHAPES = ((130, 12), (470, 12))          # the second: 36 tiles, where the default kernel flips between nine and seventeen chains


def expect_gram(ncu=NCU):
    """case 4: both f64 kernels by force, the i8 kernel, and a default that flips with the member count"""
    out = {}
    for n, V in GRAM_SHAPES:
        for nb in (9, 17):
            assert gram_plan(nb, n, V, 8, ncu=ncu)["kernel"] == "k_gram8" and gram_plan(nb, n, V, 16, ncu=ncu)["kernel"] == "k_gram<2>"
            assert gram_plan(nb, n, V, 0, True, ncu)["kernel"] == "k_gram_i8"
            g = gram_plan(nb, n, V, ncu=ncu)
            assert g["grid"] % nb == 0 and g["grid"] // 8 // nb >= 1
            out[(n, nb)] = g["kernel"]
    assert out[(130, 9)] == out[(130, 17)] == out[(470, 9)] == "k_gram<2>" and out[(470, 17)] == "k_gram8", out
    return out


BP_SHAPES = ((60, 45, 3), (60, 20, 3))        # 33 and 7 chunks of 32 edges per chain


def expect_backproj(ncu=NCU):
    """case 5: the default is k_backproj64 at 9 x 33 chunks and k_backproj at 7 chunks per chain; k_backproj runs with both nslot values"""
    out = {}
    for n, V, R in BP_SHAPES:
        for nb in (9, 17):
            assert backproj_plan(nb, n, V, R, 1, ncu)["kernel"] == "k_backproj64"
            out[(V, nb)] = (backproj_plan(nb, n, V, R, -1, ncu)["kernel"], backproj_plan(nb, n, V, R, 0, ncu)["nslot"])
    assert out[(45, 9)] == ("k_backproj64", 8) and out[(45, 17)] == ("k_backproj64", 2), out
    assert out[(20, 9)] == out[(20, 17)] == ("k_backproj", 8), out
    return out


# ------------------------------------------------------------------------------------------------------------------ problems and their references
def _units():
    """the card's compute units; the one reason to skip"""
    from test_d_update_gpu import _compute_units
    ncu = _compute_units()
    if ncu != NCU:
        pytest.skip("the shapes were chosen for %d compute units, this card has %d" % (NCU, ncu))
    return ncu


class Problem:
    """one data set; the tables of its chains run alone and of the oracle are computed once per chain id and shared (never changed)"""

    def __init__(self, n, V, R, tot, kind="f64", gram_i8=None, fv=None, seed=40):
        # fv: the factorization the chains alone run.  The one-panel and the two-panel family sum in two orders and agree to rounding only; bitwise
        # equality holds inside a family, whatever the schedule and the group (test_gpu_parity.test_factorization_variants_are_bitwise_equal)
        self.n, self.V, self.R, self.tot, self.kind, self.gram_i8, self.fv, self.seed = n, V, R, tot, kind, gram_i8, fv, seed
        rng = np.random.default_rng(7 * n + V)
        if kind == "bool":
            self.X = binary_X(rng, n, V * (V + 1) // 2)
            self.y = rng.normal(size=n) * 2.0
        else:
            self.X, self.y, _ = bnr_amd.make_synthetic(n, V, R, seed=7 * n + V)
        self.alone, self.partials, self.oracle = {}, {}, {}

    def chain(self, cid, donor=None):
        ch = bnr_amd.Chain.like(donor, self.seed, cid, self.tot) if donor is not None else bnr_amd.Chain(bnr_amd.XInput(self.X, False), self.y, self.R, self.tot, self.seed, cid)
        if self.gram_i8 is not None:
            ch.set_option("gram_i8", self.gram_i8)
        ch.init_prior()
        return ch

    def lone(self, cid, partials=False):
        if cid not in self.alone or (partials and cid not in self.partials):
            ch = self.chain(cid)
            if self.fv is not None:
                ch.set_option("factor_variant", self.fv)
            assert ch.run(2, self.tot, self.tot) == self.tot + 1
            c = ch.counters()
            assert c["chol_fail"] == 0 and c["nan_w"] == 0, (cid, c)
            self.alone[cid] = ch.fetch()
            if partials:
                self.partials[cid] = _partials(ch)
            ch.close()
        return self.alone[cid]

    def ref(self, cid):
        if cid not in self.oracle:
            o = bo.Oracle(np.asfortranarray(self.X, dtype=np.float64), self.y, self.R, self.tot, self.seed, chain=cid, pdf_mode=1)
            o.init_prior()
            o.run(2, self.tot, self.tot)
            self.oracle[cid] = o.t
        return self.oracle[cid]


_PROBLEMS = {}


def problem(*key, **kw):
    k = key + tuple(sorted(kw.items()))
    if k not in _PROBLEMS:
        _PROBLEMS[k] = Problem(*key, **kw)
    return _PROBLEMS[k]


def _partials(ch):
    dm = ch.debug_dims()
    return ch.debug_copy(3, dm["ksplit"] * (dm["ntile"] * (dm["ntile"] + 1) // 2) * 4096)


def order_of(N, how):
    """chain ids in member order: `up` 1..N; `down` N..1 (chain 1 is the last member, chain N the first); `swap` 1..N with chains 1 and 9 exchanged"""
    ids = list(range(1, N + 1))
    if how == "down":
        return ids[::-1]
    if how == "swap":                           # chain 1 sits at position 8, chain 9 at position 0
        ids[0], ids[8] = ids[8], ids[0]
    return ids


def run_group(pb, ids, opts, partials_of=None):
    """the tables of a lockstep group of the chains `ids` (in that order) after rows 2..tot; every member's counters are checked"""
    chains = [pb.chain(ids[0])]
    chains += [pb.chain(c, chains[0]) for c in ids[1:]]
    g = bnr_amd.Group(chains)
    for k, v in opts.items():
        g.set_option(k, v)
    assert g.run(2, pb.tot, pb.tot) == pb.tot + 1
    info = dict(i8=g.last_timing(4)[0], ksplit=chains[0].debug_dims()["ksplit"])
    tabs = {}
    for cid, ch in zip(ids, chains):
        c = ch.counters()
        assert c["chol_fail"] == 0 and c["nan_w"] == 0, (cid, opts, c)
        tabs[cid] = ch.fetch()
    if partials_of is not None:
        info["partials"] = _partials(chains[ids.index(partials_of)])
    g.close()
    for ch in chains:
        ch.close()
    return tabs, info


def same_tables(a, b, what):
    for k in bo.COLUMNS:
        assert np.array_equal(a[k], b[k]), (what, k)


def common(pb, ids, tabs, what):
    """the three assertions of the module docstring (the counters: run_group)"""
    N = len(ids)
    assert sorted(ids) == list(range(1, N + 1)) and N > 8
    for cid in ids:
        same_tables(tabs[cid], pb.lone(cid), (what, "chain", cid, "at position", ids.index(cid), "against the chain alone"))
    for cid in sorted({1, 9, N, ids[0], ids[8], ids[N - 1]}):
        assert_tables_close(tabs[cid], pb.ref(cid), what="%s chain %d (position %d) vs oracle" % (what, cid, ids.index(cid)))


def group_case(pb, N, how, opts, what, partials=False):
    ids = order_of(N, how)
    tabs, info = run_group(pb, ids, opts, partials_of=N if partials else None)
    if partials:
        pb.lone(N, partials=True)
    common(pb, ids, tabs, "%s N=%d %s %s" % (what, N, how, opts))
    if partials:
        assert np.array_equal(info["partials"], pb.partials[N]), (what, N, opts, "partial Gram tiles of chain %d" % N)
    return tabs, info


# ------------------------------------------------------------------------------------------------------------------ case 1: one panel per launch
@pytest.mark.parametrize("N,n,V,how", [(9, 100, 5, "up"), (9, 370, 8, "down"), (12, 370, 8, "swap"), (17, 470, 8, "up")])
def test_one_panel_factorization_of_large_groups(gpu, N, n, V, how):
    ncu = _units()
    print("restated, one-panel factorization:", expect_chol_one_panel(ncu))
    plan = chol_plan(N, n, 4, 0, ncu)
    assert all(s["arg"] == "bnr_many" for s in plan)
    print("N=%d n=%d:" % (N, n), [(s["p"], s["form"], s["spw"]) for s in plan])
    group_case(problem(n, V, 2, 4), N, how, {"factor_variant": 0}, "one panel n=%d" % n)


def test_spw_cap_of_sixteen_chains_never_changes_the_tables(gpu):
    ncu = _units()
    c1, c4 = chol_plan(16, 370, 1, 0, ncu), chol_plan(16, 370, 4, 0, ncu)
    print("restated spw, cap 1:", [s["spw"] for s in c1], "cap 4:", [s["spw"] for s in c4], "freecu", c4[1]["freecu"])
    assert max(s["spw"] for s in c4) == 4 and max(s["spw"] for s in c1) == 1 and c4[1]["freecu"] > 0
    pb = problem(370, 8, 2, 4)
    t1, _ = group_case(pb, 16, "up", {"factor_variant": 0, "spw_cap": 1}, "spw_cap")
    t4, _ = group_case(pb, 16, "up", {"factor_variant": 0, "spw_cap": 4}, "spw_cap")
    for cid in t1:
        same_tables(t4[cid], t1[cid], ("spw_cap 4 against 1, chain", cid))


def test_gamma_stages_of_the_ninth_member_against_exact_references(gpu):
    """the Gram, b, the solve, Y' A Y - I and gamma of the last of nine members (chain 1 at position 8), from the group sweep and the hook"""
    ncu = _units()
    forms = [s["form"] for s in chol_plan(9, 370, 4, 0, ncu) if s["p"] >= 2]
    assert "block" in forms and "super" in forms, forms
    _run_case(370, 8, 2, "dyadic", "prior", {"factor_variant": 0}, group=9)


# ------------------------------------------------------------------------------------------------------------------ case 2: two panels per launch
@pytest.mark.parametrize("fv", [2, 3])
def test_two_panel_factorization_of_sixteen_chains(gpu, fv):
    ncu = _units()
    print("restated, two-panel family: freecu", expect_chol_two_panel(ncu))
    group_case(problem(700, 8, 2, 3, fv=2), 16, "down", {"factor_variant": fv}, "two panels")       # (the chains alone: variant 2 for both)


# ------------------------------------------------------------------------------------------------------------------ case 3: the X pass
@pytest.mark.parametrize("kind", ["f64", "bool"])
@pytest.mark.parametrize("n,V", [(370, 12), (40, 181)])
@pytest.mark.parametrize("N", SIZES)
def test_x_pass_of_large_groups(gpu, N, n, V, kind):
    """group_xpass = 1 (one workgroup per column chunk and row slice for all members, eight at a time) and 0 (the per-chain kernel's task map);
    f64 X, and a Bool X whose X pass reads the byte image (gram_i8 = 0: the Gram stays on the f64 pipe)"""
    _units()
    how = HOW[N]
    print("restated, X pass:", expect_xpass()[N], xpass_plan(N, n, V, 1), xpass_plan(N, n, V, 0)["grid"])
    pb = problem(n, V, 2, 3, kind=kind, gram_i8=0 if kind == "bool" else None)
    t1, i1 = group_case(pb, N, how, {"group_xpass": 1}, "X pass %s n=%d V=%d" % (kind, n, V))
    t0, _ = group_case(pb, N, how, {"group_xpass": 0}, "X pass %s n=%d V=%d" % (kind, n, V))
    assert i1["i8"] == 0
    for cid in t1:
        same_tables(t1[cid], t0[cid], ("group_xpass 1 against 0, chain", cid))


# ------------------------------------------------------------------------------------------------------------------ case 4: the Gram
@pytest.mark.parametrize("N", [9, 17])
@pytest.mark.parametrize("n,V", GRAM_SHAPES)
def test_gram_of_large_groups(gpu, N, n, V):
    ncu = _units()
    print("restated, Gram default:", expect_gram(ncu))
    pb = problem(n, V, 3, 3)
    for variant in (8, 16, 0):
        plan = gram_plan(N, n, V, variant, ncu=ncu)
        _, info = group_case(pb, N, "down" if variant else "up", {"gram_variant": variant}, "Gram n=%d" % n, partials=True)
        assert info["ksplit"] == plan["ksplit"] and info["i8"] == 0, (info["ksplit"], plan)
        print("N=%d n=%d gram_variant=%d:" % (N, n, variant), plan)
    pb8 = problem(n, V, 3, 3, kind="bool", gram_i8=1)                  # (switched on: at this size the library's default is the f64 pipe)
    _, info = group_case(pb8, N, "swap", {}, "i8 Gram n=%d" % n, partials=True)
    assert info["i8"] == 1


# ------------------------------------------------------------------------------------------------------------------ case 5: the back-projection
@pytest.mark.parametrize("N", [9, 17])
@pytest.mark.parametrize("n,V,R", BP_SHAPES)
def test_back_projection_of_large_groups(gpu, N, n, V, R):
    ncu = _units()
    print("restated, back-projection (default kernel, k_backproj's nslot):", expect_backproj(ncu))
    pb = problem(n, V, R, 4)
    ref = None
    for opts in ({"wide_backproj": 1}, {"wide_backproj": 0}, {"split_sums": 0}, {}):
        print("N=%d V=%d %s:" % (N, V, opts), backproj_plan(N, n, V, R, opts.get("wide_backproj", -1), ncu))
        tabs, _ = group_case(pb, N, "swap" if opts else "down", opts, "back-projection V=%d" % V)
        ref = ref or tabs
        for cid in tabs:
            same_tables(tabs[cid], ref[cid], (opts, "against wide_backproj = 1, chain", cid))


# ------------------------------------------------------------------------------------------------------------------ case 6: status behind the eighth member
@pytest.mark.parametrize("fv", [0, 3])
@pytest.mark.parametrize("pos", [8, 9])
def test_a_failed_factorization_of_a_member_behind_the_eighth(gpu, fv, pos):
    """the reference's PosDefException path in a group of ten: the member at position 8 / 9 has the -1 pivot; the run reports status 3, that
    member counts one failure at G + I, the nine others none"""
    n, r, N = 256, 100, 10
    bad = _pivot_case(n, r, fv)
    mates = [bnr_amd.Chain.like(bad, 3, c) for c in range(2, N + 1)]
    for m in mates:
        m.init_prior()
    _set_S0(bad, -2.0)
    members = mates[:pos] + [bad] + mates[pos:]
    assert members[pos] is bad and len(members) == N
    g = bnr_amd.Group(members)
    g.set_option("factor_variant", fv)
    with pytest.raises(bnr_amd.BnrError) as e:
        g.run(2, 2, 2)
    assert e.value.code == 3, str(e.value)
    for i, m in enumerate(members):
        c = m.counters()
        if m is bad:
            assert c["chol_fail"] == 1 and c["where"] == [0, 0, 0, 1], (fv, pos, c)
        else:
            assert c["chol_fail"] == 0 and c["where"] == [0, 0, 0, 0], (fv, pos, i, c)
    g.close()
    for m in members:
        m.close()


# ------------------------------------------------------------------------------------------------------------------ case 7: a fit of nine chains
def test_fit_of_nine_chains_on_one_device(gpu):
    """generate_samples / Fit with num_chains = 9: the chains of the device form one lockstep group; every chain's trace is bitwise that of the chain
    run alone, and the pooled summaries over the nine windows are returned (their estimate: the mean of the pooled draws)"""
    n, V, R, nburn, nsamp, seed, N = 40, 8, 2, 20, 30, 77, 9
    tot = nburn + nsamp
    X, y, _ = bnr_amd.make_synthetic(n, V, R, seed=19)
    kw = dict(psrf_cutoff=np.inf, x_transform=False, suppress_timer=True, num_chains=N, seed=seed, pool_chains=True, summary_interval=95)
    keep = []
    res = bnr_amd.generate_samples(X, y, R, nburn=nburn, nsamp=nsamp, maxburn=nburn, _keep=keep, **kw)
    cs = keep[0]
    assert cs.group is not None and sorted(cs.chains) == list(range(1, N + 1))
    tabs = {c: cs.chains[c].fetch() for c in cs.chains}
    for c in cs.chains:
        k = cs.chains[c].counters()
        assert k["chol_fail"] == 0 and k["nan_w"] == 0, (c, k)
    cs.close()
    for c in range(1, N + 1):
        ch = bnr_amd.Chain(X, y, R, tot, seed, c)
        ch.init_prior()
        assert ch.run(2, nburn, tot) == tot + 1
        same_tables(tabs[c], ch.fetch(), ("fit chain", c, "against the chain alone"))
        ch.close()
    fit = bnr_amd.Fit(X, y, R, nburn=nburn, nsamples=nsamp, filename=None, **kw)
    for r in (res, fit):
        assert r.stat_chains == N and r.burn_in == nburn and r.sampled == nsamp
        assert np.array_equal(r.state["gamma"], tabs[1]["gamma"]) and np.array_equal(r.state["xi"], tabs[1]["xi"])
        g = np.concatenate([tabs[c]["gamma"][nburn:, :, 0] for c in range(1, N + 1)])
        x = np.concatenate([tabs[c]["xi"][nburn:, :, 0] for c in range(1, N + 1)])
        S = g.shape[0]
        assert S == N * nsamp
        s = r.summary_device
        # a sum of S doubles in any order and one division: gamma_(S + 1) of the mean of the magnitudes
        assert np.all(np.abs(np.ravel(s["estimate"]) - g.mean(axis=0)) <= lr.gamma_m(S + 4) * np.abs(g).mean(axis=0) + 1e-300)
        assert np.all(np.abs(np.ravel(s["probability"]) - x.mean(axis=0)) <= lr.gamma_m(S + 4) * x.mean(axis=0))
        assert np.all(np.ravel(s["lower_bound"]) <= np.ravel(s["upper_bound"])) and np.all(np.isfinite(np.ravel(s["lower_bound"])))
