"""What the compiler made of the K loops of k_gram8<bnr_one> and k_gram8<bnr_many>, read from the BUILT library (no GPU): tools/gram_loop_sched.py [library]

The sweep's gfx950 code object is unbundled as tests/code_objects.py does it, the two kernels are disassembled, and every loop (a backward branch and
its target) that holds a 16-byte load of X -- buffer_load_dwordx4 into registers, or a load straight into LDS -- is a K loop.  One row per such load:
  mfma   the v_mfma instructions between the load and the first instruction that READS what it loaded (for a load into LDS: the s_waitcnt that
         covers it), following the loop round its back edge -- the MFMAs of the wave that hide the load's latency
  wait   the first s_waitcnt whose vmcnt covers the load (loads return in order: vmcnt(N) covers it once at most N younger ones are in flight)
  stall  "yes" when that wait is vmcnt(0) with no MFMA between the last s_barrier and it: the whole workgroup then sits out a memory round trip
         right behind a barrier, with nothing of its own to issue
and per kernel the registers, scratch and LDS of its kernel descriptor.  tests/test_gram_loop_schedule_host.py asserts on the same rows."""
import os
import re
import struct
import subprocess
import sys
import tempfile
import pathlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import code_objects as co

KERNELS = ("k_gram8<bnr_one>", "k_gram8<bnr_many>")


def sweep_object(tmp_path, lib=None):
    """path of the sweep's unbundled code object (tests/code_objects.py leaves one co<i>.o per bundle in tmp_path)"""
    if lib:
        co.LIB = lib
    cos = co.code_objects(tmp_path)
    idx = [i for i, c in enumerate(cos) if any(k.startswith("k_chol_step") for k in c)]
    assert len(idx) == 1, idx
    return str(tmp_path / ("co%d.o" % idx[0]))


def symbols(obj):
    """{demangled name: (mangled name, value, section index)} of the object's symbols"""
    syms = subprocess.run([os.path.join(co.LLVM, "llvm-readelf"), "-sW", obj], check=True, stdout=subprocess.PIPE, text=True).stdout
    rows = [m.groups() for m in (re.match(r"\s*\d+:\s+([0-9a-f]+)\s+\d+\s+\S+\s+\S+\s+\S+\s+(\S+)\s+(\S+)", ln) for ln in syms.splitlines()) if m]
    dem = subprocess.run(["c++filt"], input="\n".join(r[2] for r in rows), check=True, stdout=subprocess.PIPE, text=True).stdout.splitlines()
    return {d: (r[2], int(r[0], 16), r[1]) for d, r in zip(dem, rows)}


def mangled_name(syms, kernel):
    name = [d for d in syms if re.match(r"(void )?" + re.escape(kernel) + r"\(.*\)$", d)]
    assert len(name) == 1, (kernel, name)
    return syms[name[0]][0]


def descriptor(obj, syms, kernel):
    """VGPRs (as allocated: the granule of 8 of the unified file), scratch and LDS bytes from the kernel descriptor <kernel>.kd"""
    by_mangled = {m: (v, x) for m, v, x in syms.values()}
    value, shndx = by_mangled[mangled_name(syms, kernel) + ".kd"]
    secs = subprocess.run([os.path.join(co.LLVM, "llvm-readelf"), "-SW", obj], check=True, stdout=subprocess.PIPE, text=True).stdout
    for ln in secs.splitlines():
        m = re.match(r"\s*\[\s*(\d+)\]\s+\S+\s+\S+\s+([0-9a-f]+)\s+([0-9a-f]+)\s", ln)
        if m and m.group(1) == shndx:
            addr, off = int(m.group(2), 16), int(m.group(3), 16)
            break
    else:
        raise AssertionError("section %s of %s.kd not found" % (shndx, kernel))
    kd = open(obj, "rb").read()[off + value - addr: off + value - addr + 64]
    lds, scratch = struct.unpack_from("<II", kd, 0)
    rsrc1, = struct.unpack_from("<I", kd, 48)
    return {"vgprs": ((rsrc1 & 63) + 1) * 8, "scratch": scratch, "lds": lds}


def regs(operand):
    """the VGPR numbers an operand names"""
    m = re.fullmatch(r"v\[(\d+):(\d+)\]", operand)
    if m:
        return set(range(int(m.group(1)), int(m.group(2)) + 1))
    m = re.fullmatch(r"v(\d+)", operand)
    return {int(m.group(1))} if m else set()


class Inst:
    def __init__(self, addr, text):
        self.addr, self.text = addr, text
        self.op, _, rest = text.partition(" ")
        self.args = [a.strip() for a in rest.split(",")] if rest.strip() else []
        self.args = [a.split(" ")[0] for a in self.args]
        store = re.match(r"(ds_write|buffer_store|global_store|scratch_store|flat_store)", self.op)
        self.lds_load = bool(re.match(r"(buffer|global)_load", self.op)) and (" lds" in text or "_lds_" in self.op)
        srcs = self.args if (store or self.lds_load) else self.args[1:]
        self.writes = set() if (store or self.lds_load or not self.args) else regs(self.args[0])
        self.reads = set().union(*[regs(a) for a in srcs]) if srcs else set()
        self.vmem = bool(re.match(r"(buffer|global|flat|scratch)_(load|store|atomic)", self.op))
        self.x_load = self.op == "buffer_load_dwordx4" or (self.lds_load and ("dwordx4" in self.op or "b128" in self.op))
        m = re.search(r"vmcnt\((\d+)\)", text) if self.op == "s_waitcnt" else None
        self.vmcnt = int(m.group(1)) if m else None
        self.mfma = self.op.startswith("v_mfma")


def disassemble(obj, mangled):
    """(instructions, {index of a branch: index of its target}) of one kernel"""
    out = subprocess.run([os.path.join(co.LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn", "--disassemble-symbols=" + mangled, obj],
                         check=True, stdout=subprocess.PIPE, text=True).stdout
    insts, targets, base = [], {}, None
    for ln in out.splitlines():
        m = re.match(r"([0-9a-f]+) <" + re.escape(mangled) + r">:", ln)
        if m:
            base = int(m.group(1), 16)
            continue
        m = re.match(r"\s+(\S.*?)\s*//\s*([0-9A-Fa-f]+):(.*)$", ln)
        if not m or base is None:
            continue
        inst = Inst(int(m.group(2), 16), m.group(1))
        t = re.search(r"<" + re.escape(mangled) + r"(?:\+0x([0-9a-f]+))?>", m.group(3))
        if t and (inst.op.startswith("s_cbranch") or inst.op == "s_branch"):
            targets[len(insts)] = base + int(t.group(1) or "0", 16)
        insts.append(inst)
    at = {i.addr: n for n, i in enumerate(insts)}
    return insts, {n: at[a] for n, a in targets.items() if a in at}, base


def k_loops(insts, branches):
    """[(first, last)] instruction index ranges of the innermost loops that hold an X load"""
    loops = sorted((t, n) for n, t in branches.items() if t <= n)
    loops = [l for l in loops if not any(o != l and l[0] <= o[0] and o[1] <= l[1] for o in loops)]
    return [l for l in loops if any(i.x_load for i in insts[l[0]:l[1] + 1])]


def loop_rows(insts, first, last):
    body = insts[first:last + 1]
    n = len(body)
    rows = []
    for k, ld in enumerate(body):
        if not ld.x_load:
            continue
        order = [body[(k + 1 + d) % n] for d in range(n)]         # one whole trip behind the load, the load itself last
        mfma = younger = 0
        consumer = wait = None
        wait_pos = None
        for d, i in enumerate(order):
            if wait is None and i.vmcnt is not None and i.vmcnt <= younger:
                wait, wait_pos = i, (k + 1 + d) % n
                if ld.lds_load:
                    consumer = i
            if consumer is None and not ld.lds_load and (i.reads & ld.writes):
                consumer = i
            if consumer is not None and wait is not None:
                break
            if consumer is None:
                if i.writes & ld.writes and i is not ld:
                    break                                           # overwritten unread
                mfma += i.mfma
            younger += i.vmem
        stall = False
        if wait is not None and wait.vmcnt == 0:
            for d in range(1, n + 1):                               # back from the wait: a barrier before any MFMA?
                i = body[(wait_pos - d) % n]
                if i.mfma:
                    break
                if i.op == "s_barrier":
                    stall = True
                    break
        rows.append({"load": ld, "consumer": consumer, "mfma": mfma if consumer is not None else None, "wait": wait, "stall": stall})
    return rows


def analyse(tmp_path, lib=None):
    """{kernel: {"resources": {...}, "loops": [{"start": byte offset in the kernel, "mfma": MFMAs per trip, "rows": [...]}]}}"""
    obj = sweep_object(pathlib.Path(tmp_path), lib)
    syms = symbols(obj)
    out = {}
    for kernel in KERNELS:
        insts, branches, base = disassemble(obj, mangled_name(syms, kernel))
        loops = []
        for first, last in k_loops(insts, branches):
            loops.append({"start": insts[first].addr - base, "mfma": sum(i.mfma for i in insts[first:last + 1]), "rows": loop_rows(insts, first, last), "base": base})
        out[kernel] = {"resources": descriptor(obj, syms, kernel), "loops": loops}
    return out


def main():
    lib = sys.argv[1] if len(sys.argv) > 1 else None
    if not co.have_tools():
        sys.exit("the LLVM tools of ROCm are not installed")
    with tempfile.TemporaryDirectory() as tmp:
        res = analyse(tmp, lib)
    print("library: %s" % (lib or co.LIB))
    for kernel, r in res.items():
        print("%s: %d VGPRs, %d bytes of scratch, %d bytes of LDS" % (kernel, r["resources"]["vgprs"], r["resources"]["scratch"], r["resources"]["lds"]))
        for lp in r["loops"]:
            print("  K loop at +0x%x, %d MFMAs per trip" % (lp["start"], lp["mfma"]))
            print("    %-8s %-22s %-12s %-34s %5s  %-10s %s" % ("at", "load", "into", "first reader", "mfma", "wait", "stall"))
            for row in lp["rows"]:
                ld, c, w = row["load"], row["consumer"], row["wait"]
                print("    +0x%-5x %-22s %-12s %-34s %5s  %-10s %s" % (
                    ld.addr - lp["base"], ld.op, "LDS" if ld.lds_load else ld.args[0],
                    "(none)" if c is None else "+0x%x %s" % (c.addr - lp["base"], c.op),
                    "-" if row["mfma"] is None else row["mfma"], "-" if w is None else "vmcnt(%d)" % w.vmcnt, "yes" if row["stall"] else "no"))


if __name__ == "__main__":
    main()
