// bnr_mcheck_rows.h -- the host code that libbnr_mcheck.so (bnr_mcheck.hip) and libbnr_mstack.so (bnr_mstack.hip) share: the outputs of a
// mixture call and their checks (mix_out, mix_check) and the two row kernels of bnr_mcheck_kernels.h on staged matrices (mix_rows).  No kernel
// of its own.  Internal: included by those two translation units after bnr_mcheck_kernels.h and bnr_mloo_job.h, each into its own library and
// code object; every name here has internal linkage.
#pragma once
#include "bnr_mcheck_kernels.h"
#include "bnr_mloo_job.h"

namespace {
struct mix_out { double *mean, *sd, *pit, *lower, *upper; };

// the checks of a mixture's arguments that need no shapes; c: the bracket's half-width in sds
const char *mix_check(const mix_out &o, bool has_y, double p_lo, double p_hi, double &c)
{
    c = 1.0;
    if (o.pit && !has_y) return "pit needs y";
    if (o.lower || o.upper) {
        if (!(p_lo > 0.0 && p_lo < p_hi && p_hi < 1.0)) return "need 0 < p_lo < p_hi < 1";
        c = bracket_halfwidth(p_lo, p_hi);
    }
    return nullptr;
}

// The rest of a mixture call once its matrices M, V, Wt, Isd (rows x D, a row's components contiguous) are allocated: the outputs' device
// slots, then stage() -- the caller's launch that fills the staged matrices --, k_mcheck_moments and (for the bounds) k_mcheck_quantile over the
// rows in chunks of MCHECK_ROWS_PER_LAUNCH, and the outputs asked for to the host; the stream is synchronised on return.  yd: rows, NULL: none.
template <typename Stage>
int mix_rows(call_guard &g, int rows, int D, const double *M, const double *V, const double *Wt, const double *Isd, const double *yd, double c,
             double p_lo, double p_hi, const mix_out &o, Stage stage)
{
    int rc;
    double *out = nullptr, *brk = nullptr;
    int *flag = nullptr;
    if ((rc = g.alloc(&out, (size_t)5 * rows))) return rc;
    if ((rc = g.alloc(&flag, (size_t)rows))) return rc;
    const bool bounds = o.lower || o.upper;
    if (bounds && (rc = g.alloc(&brk, (size_t)2 * rows))) return rc;
    double *host[5] = {o.mean, o.sd, o.pit, o.lower, o.upper}, *dev[5];
    for (int f = 0; f < 5; ++f) dev[f] = host[f] ? out + (size_t)f * rows : nullptr;
    stage();
    for (int i0 = 0; i0 < rows; i0 += MCHECK_ROWS_PER_LAUNCH) {
        const int nr = std::min(MCHECK_ROWS_PER_LAUNCH, rows - i0);
        hipLaunchKernelGGL(k_mcheck_moments, dim3(nr), dim3(256), 0, g.st, M, V, Wt, Isd, yd, D, i0, c, dev[0], dev[1], dev[2], brk, flag);
        if (bounds)
            hipLaunchKernelGGL(k_mcheck_quantile, dim3(nr, 2), dim3(256), 0, g.st, M, Wt, Isd, D, i0, (const double *)brk, (const int *)flag, p_lo, p_hi,
                               dev[3], dev[4]);
    }
    HIPCHK(hipGetLastError());
    for (int f = 0; f < 5; ++f)
        if (host[f]) HIPCHK(hipMemcpyAsync(host[f], dev[f], sizeof(double) * (size_t)rows, hipMemcpyDeviceToHost, g.st));
    HIPCHK(hipStreamSynchronize(g.st));
    HIPCHK(hipGetLastError());
    return BNR_OK;
}
}   // namespace
