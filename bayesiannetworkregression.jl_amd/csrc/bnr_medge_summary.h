// bnr_medge_summary.h -- the host driver of k_medge_summary that libbnr_medge.so (bnr_medge.hip), libbnr_mpred.so (bnr_mpred.hip) and
// libbnr_mcov.so (bnr_mcov.hip) share: the checks of a summary's arguments, the chain weights, the launch and the way an item-major device
// matrix reaches the host (fetch_transposed) and a draw-major host matrix the device (upload_transposed).  Internal: included by those
// translation units after bnr_medge_kernels.h and bnr_mloo_job.h, each into its own library and code object; every name here has internal
// linkage (the way bnr_mloo_job.h was split off bnr_mloo.hip).
#pragma once
#include "bnr_medge_kernels.h"
#include "bnr_mloo_job.h"

namespace {
// an edge-major device matrix (q x D) to the host as D x q
int fetch_transposed(call_guard &g, const double *dev, int q, int D, double *out)
{
    std::vector<double> t((size_t)q * (size_t)D);
    HIPCHK(hipMemcpyAsync(t.data(), dev, sizeof(double) * t.size(), hipMemcpyDeviceToHost, g.st));
    HIPCHK(hipStreamSynchronize(g.st));
    for (int s = 0; s < D; ++s)
        for (int e = 0; e < q; ++e) out[(size_t)s * q + e] = t[(size_t)e * D + s];
    return BNR_OK;
}

// a host (D x q) matrix, a draw's q values contiguous, to the device as q x D
int upload_transposed(call_guard &g, const double *src, int q, int D, double **dev)
{
    std::vector<double> t((size_t)q * (size_t)D);
    for (int s = 0; s < D; ++s)
        for (int e = 0; e < q; ++e) t[(size_t)e * D + s] = src[(size_t)s * q + e];
    int rc;
    if ((rc = g.upload(dev, t.data(), t.size()))) return rc;
    HIPCHK(hipStreamSynchronize(g.st));                                  // (t leaves scope)
    return BNR_OK;
}

struct summary_out { double *mean, *sd, *var_within, *p_pos, *p_neg, *lower, *upper; };

// the checks of a summary's arguments that do not need the shapes; c: the bracket's half-width in sds
int summary_check(const summary_out &o, double p_lo, double p_hi, double &c)
{
    if (!o.mean && !o.sd && !o.var_within && !o.p_pos && !o.p_neg && !o.lower && !o.upper) return fail(BNR_ERR_BAD_ARG, "ask for at least one summary");
    if ((o.lower == nullptr) != (o.upper == nullptr)) return fail(BNR_ERR_BAD_ARG, "lower and upper come together");
    c = 1.0;
    if (o.lower) {
        if (!(p_lo > 0.0 && p_lo < p_hi && p_hi < 1.0)) return fail(BNR_ERR_BAD_ARG, "need 0 < p_lo < p_hi < 1");
        c = bracket_halfwidth(p_lo, p_hi);
    }
    return BNR_OK;
}

// the chain weights of a summary: as given after weight_check, or 1 / K each
int summary_weights(const double *weights, int K, std::vector<double> &w)
{
    w.assign((size_t)K, 1.0 / (double)K);
    if (!weights) return BNR_OK;
    if (K > 32) return fail(BNR_ERR_BAD_ARG, "need 1 <= nchains <= 32 for a weighted call");
    if (const char *msg = weight_check(weights, K)) return fail(BNR_ERR_BAD_ARG, msg);
    w.assign(weights, weights + K);
    return BNR_OK;
}

// k_medge_summary on the edge-major device matrices Md, Vd (q x K nd) and its results to the host
int summary_run(call_guard &g, int q, int K, int nd, const double *Md, const double *Vd, const std::vector<double> &w, double c, double p_lo, double p_hi,
                const summary_out &o)
{
    int rc;
    double *wd = nullptr, *out = nullptr;
    if ((rc = g.upload(&wd, w.data(), (size_t)K))) return rc;
    if ((rc = g.alloc(&out, (size_t)7 * q))) return rc;
    double *host[7] = {o.mean, o.sd, o.var_within, o.p_pos, o.p_neg, o.lower, o.upper}, *dev[7];
    for (int f = 0; f < 7; ++f) dev[f] = host[f] ? out + (size_t)f * q : nullptr;
    hipLaunchKernelGGL(k_medge_summary, dim3((q + 3) / 4), dim3(256), 0, g.st, Md, Vd, (long long)K * nd, q, K, nd, (const double *)wd, c, p_lo, p_hi, dev[0],
                       dev[1], dev[2], dev[3], dev[4], dev[5], dev[6]);
    HIPCHK(hipGetLastError());
    for (int f = 0; f < 7; ++f)
        if (host[f]) HIPCHK(hipMemcpyAsync(host[f], dev[f], sizeof(double) * (size_t)q, hipMemcpyDeviceToHost, g.st));
    HIPCHK(hipStreamSynchronize(g.st));
    HIPCHK(hipGetLastError());
    return BNR_OK;
}
}   // namespace
