"""The gfx950 code objects inside the built libbnr_hip.so, for the tests that pin which kernel lives where.  The library is linked from two
translation units -- csrc/bnr_hip.hip (the sweep) and csrc/bnr_analysis.hip (the posterior analysis) -- so its .hip_fatbin section holds two
offload bundles back to back; clang-offload-bundler only unbundles the first of an input, hence the split at the bundles' magic string."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "bayesiannetworkregression.jl_amd", "libbnr_hip.so")
LLVM = "/opt/rocm/lib/llvm/bin"
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"
CSRC = os.path.join(ROOT, "bayesiannetworkregression.jl_amd", "csrc")
# The manifest: every kernel instantiation of the two code objects, as c++filt prints them -- csrc/bnr_kernels.h in the sweep's, csrc/bnr_analysis_kernels.h
# in the analysis one.  test_host_cpu.py asserts both whole; a kernel added to either header is added here.
SWEEP = frozenset((
    "k_node<bnr_one>", "k_node<bnr_many>", "k_xpass<bnr_one>", "k_xpass<bnr_many>", "k_xpass_group", "k_xpass_group2<0>",
    "k_gram<bnr_one, 2>", "k_gram<bnr_one, 4>", "k_gram<bnr_many, 2>", "k_gram<bnr_many, 4>", "k_gram8<bnr_one>", "k_gram8<bnr_many>",
    "k_x_mask", "k_sdigits<bnr_one, 7>", "k_sdigits<bnr_one, 8>", "k_sdigits<bnr_many, 7>", "k_sdigits<bnr_many, 8>",
    "k_gram_i8<bnr_one, 7>", "k_gram_i8<bnr_one, 8>", "k_gram_i8<bnr_many, 7>", "k_gram_i8<bnr_many, 8>", "k_gram_reduce<bnr_one>", "k_gram_reduce<bnr_many>",
    "k_chol_step<bnr_one>", "k_chol_step<bnr_few>", "k_chol_step<bnr_many>", "k_chol_step2<bnr_one>", "k_chol_step2<bnr_many>",
    "k_rhs<bnr_one>", "k_rhs<bnr_many>", "k_solve_w<bnr_one>", "k_solve_w<bnr_many>", "k_solve_a4<bnr_one>", "k_solve_a4<bnr_many>",
    "k_backproj<bnr_one>", "k_backproj<bnr_many>", "k_backproj64<bnr_one>", "k_backproj64<bnr_many>",
    "k_tail<bnr_one, true>", "k_tail<bnr_one, false>", "k_tail<bnr_many, true>", "k_tail<bnr_many, false>",
    "k_advance", "k_scatter_plans", "k_nop", "k_gather_counters", "k_setbase", "k_init_prior",
    "k_x_convert<double>", "k_x_convert<float>", "k_x_convert<int>", "k_x_convert<long>", "k_x_convert<unsigned char>", "k_fetch_cols", "k_load_cols",
    "k_rhat_stats", "k_summary", "k_acov", "k_wsummary<10>", "k_wsummary<8>"))   # (trace statistics; the analysis launches them through csrc/bnr_internal.h)
ANALYSIS = frozenset((
    "k_predict<2>", "k_predict<1>", "k_pred_loglik", "k_pred_pit", "k_pred_noise", "k_psis<0>", "k_psis<1>",
    "k_psis_w<0>", "k_psis_w<1>", "k_inv_sd", "k_loo_moments", "k_loo_quantile", "k_rank", "k_fold", "k_hdi",
    "k_incl_pack", "k_incl_joint", "k_incl_group", "k_cov<2>", "k_cov<4>", "k_cov_finish"))


def declared_kernels(header):
    """the names of the __global__ functions that csrc/<header> declares"""
    src = open(os.path.join(CSRC, header)).read()
    return set(re.findall(r"__global__\s+(?:__launch_bounds__\([^)]*\)\s+)?void\s+(k_\w+)\s*\(", src))


def have_tools():
    return os.path.exists(os.path.join(LLVM, "clang-offload-bundler"))


def code_objects(tmp_path):
    """one {demangled kernel name: (address, size)} per gfx950 code object of LIB, in the order of the bundles"""
    fat = str(tmp_path / "fat.bin")
    subprocess.run(["objcopy", "-O", "binary", "--only-section=.hip_fatbin", LIB, fat], check=True)
    blob = open(fat, "rb").read()
    starts = [m.start() for m in re.finditer(re.escape(MAGIC), blob)]
    out = []
    for i, (a, b) in enumerate(zip(starts, starts[1:] + [len(blob)])):
        piece, co = str(tmp_path / ("bundle%d.bin" % i)), str(tmp_path / ("co%d.o" % i))
        open(piece, "wb").write(blob[a:b])
        subprocess.run([os.path.join(LLVM, "clang-offload-bundler"), "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--input=" + piece, "--output=" + co,
                        "--unbundle"], check=True)
        syms = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "-sW", co], check=True, stdout=subprocess.PIPE, text=True).stdout
        names = subprocess.run(["c++filt"], input=syms, check=True, stdout=subprocess.PIPE, text=True).stdout
        kernels = {}
        for line in names.splitlines():
            m = re.match(r"\s*\d+:\s+([0-9a-f]+)\s+(\d+)\s+FUNC\s+\S+\s+\S+\s+\S+\s+(?:void )?(k_\w+(?:<[^>]*>)?)", line)
            if m:
                kernels[m.group(3)] = (int(m.group(1), 16), int(m.group(2)))
        out.append(kernels)
    return out


def sweep_and_analysis(tmp_path):
    """(the sweep's code object, the analysis one): exactly two, told apart by where k_chol_step lives"""
    cos = code_objects(tmp_path)
    assert len(cos) == 2, [sorted(c)[:3] for c in cos]
    sweep = [c for c in cos if any(k.startswith("k_chol_step") for k in c)]
    assert len(sweep) == 1
    return sweep[0], [c for c in cos if c is not sweep[0]][0]
