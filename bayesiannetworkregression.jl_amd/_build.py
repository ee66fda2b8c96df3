"""Build libbnr_hip.so and the six marginal libraries beside it (hipcc, gfx950) in-tree."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
LIB = os.environ.get("BNR_HIP_LIB") or os.path.join(HERE, "libbnr_hip.so")     # BNR_HIP_LIB: another build of the library (the sanitizer build of tools/sanitize_cpu.sh; julia/BNRHip.jl honours the same variable)
# the marginal libraries by short name (include/bnr_<short>.h): each a library and a code object of its own, linked against libbnr_hip.so beside it
MARGINAL_LIBS = {short: os.path.join(HERE, "libbnr_%s.so" % short) for short in ("mloo", "medge", "mpred", "mcheck", "mstack", "mcov")}
MLOO_LIB, MEDGE_LIB, MPRED_LIB, MCHECK_LIB, MSTACK_LIB, MCOV_LIB = MARGINAL_LIBS.values()


def build(force=False, verbose=False):
    if os.environ.get("BNR_HIP_LIB"):
        return LIB
    csrc = os.path.join(HERE, "csrc")
    cmd = ["make", "-j%d" % (2 + len(MARGINAL_LIBS)), "-C", csrc] + (["-B"] if force else [])     # the translation units side by side: libbnr_hip.so's two and one per marginal library
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if verbose or r.returncode:
        print(r.stdout)
    if r.returncode:
        raise RuntimeError("building %s failed" % " / ".join(["libbnr_hip.so"] + [os.path.basename(p) for p in MARGINAL_LIBS.values()]))
    return LIB
