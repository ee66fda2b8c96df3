"""The store forms of the sweep's cross-launch outputs in the built gfx950 code object (BNR_STORE_THROUGH, csrc/bnr_kernels.h), and the registers of the kernels
that must not grow.  No GPU: the library's sweep code object is disassembled.  A check of vector store forms and register counts only.

Per site bit and kernel: with the bit set the kernel holds the store as a write-through one (global_/flat_store_dwordx2 or _dwordx4 with sc1), with the bit
cleared as a plain one.  Where the site's stores are the kernel's only stores of that width, the other form must be absent as well; k_chol_step holds two sites
of the same width (the update roles and the swept block), so there only presence is asked unless both bits agree.
Registers: k_gram8 at most 80 VGPRs (three workgroups of 512 per CU), the three k_chol_step at most 128 (four workgroups of 256), none of them nor k_backproj64
with scratch."""
import os
import re
import subprocess

import pytest

import code_objects as co

HEADER = os.path.join(co.CSRC, "bnr_kernels.h")
MAKEFILE = os.path.join(co.CSRC, "Makefile")
pytestmark = pytest.mark.skipif(not (co.have_tools() and os.path.exists(os.path.join(co.LLVM, "llvm-objdump")) and os.path.exists(co.LIB)),
                                reason="needs the built libbnr_hip.so and ROCm's clang-offload-bundler / llvm-objdump")
# (site, kernel name up to its template arguments, store mnemonic, these are the kernel's only stores of that width)
SITES = [
    ("GRAM", "k_gram", "global_store_dwordx2", True), ("GRAM", "k_gram8", "global_store_dwordx2", True), ("GRAM", "k_gram_i8", "global_store_dwordx2", True),
    ("LAUNCH0", "k_gram_reduce", "global_store_dwordx4", True), ("LAUNCH0", "k_chol_step<bnr_one>", "global_store_dwordx4", True),
    ("LAUNCH0", "k_chol_step<bnr_many>", "global_store_dwordx4", True),
    ("UPDATE", "k_chol_step", "global_store_dwordx2", False), ("PANEL", "k_chol_step", "global_store_dwordx2", False),
    ("RHS", "k_rhs", "global_store_dwordx2", True), ("RHS", "k_solve_w", "global_store_dwordx2", False), ("RHS", "k_solve_a4", "global_store_dwordx2", True),
    ("XPASS", "k_xpass", "global_store_dwordx2", False), ("XPASS", "k_xpass_group", "flat_store_dwordx2", True), ("XPASS", "k_xpass_group2", "flat_store_dwordx2", True),
    ("BACKPROJ", "k_backproj", "global_store_dwordx2", True), ("BACKPROJ", "k_backproj64", "global_store_dwordx2", True),
]


def _default_mask():
    src = open(HEADER).read()
    bits = {name: int(v) for name, v in re.findall(r"\bBNR_ST_(\w+) = (\d+)", src)}
    assert sorted(bits.values()) == [1, 2, 4, 8, 16, 32, 64], bits
    m = re.search(r"-DBNR_STORE_THROUGH=(\S+)", open(MAKEFILE).read())
    expr = m.group(1) if m else re.search(r"#ifndef BNR_STORE_THROUGH\s*\n#define BNR_STORE_THROUGH ([^\n/]+)", src).group(1)
    assert re.fullmatch(r"[\w\s|()]+", expr), expr
    mask = eval(re.sub(r"BNR_ST_(\w+)", lambda g: str(bits[g.group(1)]), expr), {"__builtins__": {}})
    return bits, mask


@pytest.fixture(scope="module")
def sweep(tmp_path_factory):
    """the sweep's code object: {demangled kernel: its disassembly}, {demangled kernel: (VGPRs, scratch bytes)}"""
    tmp = tmp_path_factory.mktemp("store_through")
    co.code_objects(tmp)                                   # leaves co<i>.o, one per bundle
    for f in sorted(os.listdir(tmp)):
        if not re.fullmatch(r"co\d+\.o", f):
            continue
        path = str(tmp / f)
        dis = subprocess.run([os.path.join(co.LLVM, "llvm-objdump"), "-d", "--mcpu=gfx950", path], check=True, stdout=subprocess.PIPE, text=True).stdout
        if "k_chol_step" not in dis:
            continue
        body, cur = {}, None
        for line in dis.splitlines():
            m = re.match(r"[0-9a-f]+ <(\S+)>:", line)
            if m:
                cur = m.group(1)
                body[cur] = []
            elif cur:
                body[cur].append(line)
        notes = subprocess.run([os.path.join(co.LLVM, "llvm-readelf"), "--notes", path], check=True, stdout=subprocess.PIPE, text=True).stdout
        res = {}
        for blk in re.split(r"\n\s*- \.agpr_count:", notes)[1:]:
            name, vg, sc = re.search(r"\.name:\s+(\S+)", blk), re.search(r"\.vgpr_count:\s+(\d+)", blk), re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk)
            res[name.group(1)] = (int(vg.group(1)), int(sc.group(1)))
        names = list(body)
        plain = subprocess.run(["c++filt"], input="\n".join(names), check=True, stdout=subprocess.PIPE, text=True).stdout.splitlines()
        short = {n: re.sub(r"^void |\(.*$", "", p) for n, p in zip(names, plain)}
        return {short[n]: body[n] for n in names}, {short[n]: res[n] for n in names if n in res}
    pytest.fail("no code object with k_chol_step in the library")


def _count(lines, mnemonic):
    through = sum(1 for ln in lines if re.search(r"\b%s\b" % mnemonic, ln) and re.search(r"\bsc1\b", ln))
    plain = sum(1 for ln in lines if re.search(r"\b%s\b" % mnemonic, ln) and not re.search(r"\bsc1\b", ln))
    return through, plain


def test_every_site_has_the_store_form_its_bit_asks_for(sweep):
    body, _ = sweep
    bits, mask = _default_mask()
    groups = {}                                            # (kernel instantiation, mnemonic) -> [site bits set?], only
    for site, kern, mnem, only in SITES:
        inst = [k for k in body if k == kern or k.startswith(kern + "<")]
        assert inst, ("no instantiation of", kern)
        for k in inst:
            g = groups.setdefault((k, mnem), [[], True])
            g[0].append(bool(mask & bits[site]))
            g[1] = g[1] and only
    for (k, mnem), (on, only) in sorted(groups.items()):
        through, plain = _count(body[k], mnem)
        if all(on):
            assert through >= 1, (k, mnem, "no write-through store although the bit is set", through, plain)
            if only:
                assert plain == 0, (k, mnem, "a plain store is left although the bit is set", through, plain)
        elif not any(on):
            assert plain >= 1 and through == 0, (k, mnem, "a write-through store although the bit is cleared", through, plain)
        else:
            assert through >= 1 and plain >= 1, (k, mnem, "two sites with different bits: both forms must be there", through, plain)


def test_registers_and_scratch_stay_where_they_were(sweep):
    _, res = sweep
    seen = 0
    for k, (vgpr, scratch) in res.items():
        if k.startswith("k_gram8<"):
            assert vgpr <= 80 and scratch == 0, (k, vgpr, scratch)
            seen += 1
        elif k.startswith("k_chol_step<"):
            assert vgpr <= 128 and scratch == 0, (k, vgpr, scratch)
            seen += 1
        elif k.startswith("k_backproj64<"):
            assert scratch == 0, (k, vgpr, scratch)
            seen += 1
    assert seen == 7, sorted(res)
