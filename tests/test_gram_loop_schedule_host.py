"""The K loops of k_gram8 as the compiler emitted them, read from the built library (tools/gram_loop_sched.py; no GPU).

bnr_gram8_task loads batch b + 2 at the top of batch b and stores it to LDS between the two k-steps of batch b + 1.  What is asserted, for
k_gram8<bnr_one> and k_gram8<bnr_many>, is that the compiled loops keep that:
  - the kernel descriptor: at most 80 VGPRs, no scratch, 32 768 bytes of LDS (three 512-thread workgroups per CU, six waves per SIMD);
  - three K loops (full block, diagonal block, dead block of a diagonal tile), and in each that holds MFMAs every 16-byte load of X is
    followed by at least 8 MFMAs of its wave before the first instruction that reads what it loaded (one batch of a full block: the
    latency a wave hides by itself);
  - in every K loop no such load is waited for by an s_waitcnt vmcnt(0) that stands behind an s_barrier with no MFMA in between (the
    whole workgroup would sit out a memory round trip there).
Skips without the LLVM tools or the built library."""
import importlib.util
import os

import pytest

import code_objects as co

KERNELS = ("k_gram8<bnr_one>", "k_gram8<bnr_many>")


@pytest.fixture(scope="module")
def sched(tmp_path_factory):
    if not co.have_tools():
        pytest.skip("the LLVM tools of ROCm are not installed")
    if not os.path.exists(co.LIB):
        pytest.skip("the library is not built")
    spec = importlib.util.spec_from_file_location("gram_loop_sched", os.path.join(co.ROOT, "tools", "gram_loop_sched.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    assert tool.KERNELS == KERNELS
    return tool.analyse(tmp_path_factory.mktemp("gram_loop_sched"))


@pytest.mark.parametrize("kernel", KERNELS)
def test_the_compiled_k_loops_keep_the_written_prefetch_distance(sched, kernel):
    r = sched[kernel]
    assert r["resources"]["vgprs"] <= 80 and r["resources"]["scratch"] == 0 and r["resources"]["lds"] == 32768, (kernel, r["resources"])
    loops = r["loops"]
    assert len(loops) == 3 and sorted(lp["mfma"] for lp in loops) == [0, 12, 16], (kernel, [(hex(lp["start"]), lp["mfma"]) for lp in loops])
    for lp in loops:
        assert len(lp["rows"]) == 4, (kernel, hex(lp["start"]))         # two batches per trip, an I and a J panel each
        for row in lp["rows"]:
            where = (kernel, "loop +0x%x" % lp["start"], "load +0x%x" % (row["load"].addr - lp["base"]))
            assert row["consumer"] is not None and row["wait"] is not None, where
            print(where, "MFMAs to the first reader:", row["mfma"], "wait: vmcnt(%d)" % row["wait"].vmcnt, "behind a barrier:", row["stall"])
    for lp in loops:
        if lp["mfma"]:
            short = [(hex(row["load"].addr - lp["base"]), row["mfma"]) for row in lp["rows"] if row["mfma"] < 8]
            assert not short, (kernel, "loop +0x%x" % lp["start"], "loads fewer than 8 MFMAs ahead of their first reader", short)
    for lp in loops:
        stalls = [hex(row["load"].addr - lp["base"]) for row in lp["rows"] if row["stall"]]
        assert not stalls, (kernel, "loop +0x%x" % lp["start"], "s_waitcnt vmcnt(0) directly behind s_barrier for the loads at", stalls)
