"""Build libbnr_hip.so, libbnr_mloo.so, libbnr_medge.so, libbnr_mpred.so, libbnr_mcheck.so, libbnr_mstack.so and libbnr_mcov.so (hipcc, gfx950) in-tree."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
LIB = os.environ.get("BNR_HIP_LIB") or os.path.join(HERE, "libbnr_hip.so")     # BNR_HIP_LIB: another build of the library (the sanitizer build of tools/sanitize_cpu.sh; julia/BNRHip.jl honours the same variable)
MLOO_LIB = os.path.join(HERE, "libbnr_mloo.so")                              # marginal PSIS-LOO: a library of its own, linked against libbnr_hip.so beside it
MEDGE_LIB = os.path.join(HERE, "libbnr_medge.so")                            # Rao-Blackwellised edge summaries: a third library, built and linked like libbnr_mloo.so
MPRED_LIB = os.path.join(HERE, "libbnr_mpred.so")                            # Rao-Blackwellised prediction of new rows: a fourth library, built and linked like libbnr_medge.so
MCHECK_LIB = os.path.join(HERE, "libbnr_mcheck.so")                          # LOO predictive checks under the marginal PSIS weights: a fifth library, built and linked like libbnr_mpred.so
MSTACK_LIB = os.path.join(HERE, "libbnr_mstack.so")                          # chain stacking on the marginal PSIS-LOO: a sixth library, built and linked like libbnr_mcheck.so
MCOV_LIB = os.path.join(HERE, "libbnr_mcov.so")                              # Rao-Blackwellised covariance of the edge coefficients: a seventh library, built and linked like libbnr_medge.so


def build(force=False, verbose=False):
    if os.environ.get("BNR_HIP_LIB"):
        return LIB
    csrc = os.path.join(HERE, "csrc")
    cmd = ["make", "-j8", "-C", csrc] + (["-B"] if force else [])          # eight translation units, side by side
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if verbose or r.returncode:
        print(r.stdout)
    if r.returncode:
        raise RuntimeError("building libbnr_hip.so / libbnr_mloo.so / libbnr_medge.so / libbnr_mpred.so / libbnr_mcheck.so / libbnr_mstack.so / libbnr_mcov.so failed")
    return LIB
