// bnr_medge.hip -- libbnr_medge.so behind include/bnr_medge.h: Rao-Blackwellised summaries of the edge coefficients, gamma integrated out on the
// device.  A library and a gfx950 code object of its own: the four kernels of bnr_mloo_kernels.h (by #include, through the driver shared with
// the other marginal libraries, bnr_mloo_job.h: it opens the job of either form and runs its batches) plus k_medge_proj and k_medge_summary
// (bnr_medge_kernels.h); the summary's host driver and the transposing copies are bnr_medge_summary.h, shared with libbnr_mpred.so and
// libbnr_mcov.so.  It reaches a chain through bnr_chain_device_view and leaves its messages with bnr_set_last_error -- exported calls of
// libbnr_hip.so, nothing of bnr_internal.h.
// Linked with bnr_medge.map: only the functions of the header are exported, so that neither this library nor libbnr_mloo.so, loaded into one
// process, can bind the other's kernel handles or host stubs.
#include "../../include/bnr_medge.h"
#include "bnr_medge_kernels.h"
#include "bnr_mloo_job.h"
#include "bnr_medge_summary.h"

namespace {
// m and v of every draw of the job, edge-major on the device (Md, Vd: q x ndraws), by k_medge_proj behind every batch's k_mloo_factor; resid and var
// stay on the device
int gamma_job(call_guard &g, mloo_job &job, double *Md, double *Vd, mloo_out &out)
{
    job.want_ll = false; job.want_resid = true; job.want_var = true;
    const long long D = job.ndraws;
    mloo_hook hook = [&](const mloo_batch &bt) -> int {
        hipLaunchKernelGGL(k_medge_proj, dim3((job.q + MEDGE_EB - 1) / MEDGE_EB, (bt.nb + MEDGE_DB - 1) / MEDGE_DB), dim3(256), 0, g.st, job.X, job.ldx,
                           job.n, bt.np, job.q, bt.G, (long long)bt.mat, bt.Sp, bt.Wbuf, bt.tau2, bt.resid, bt.var, bt.bad, bt.s0, D, bt.nb, Md, Vd);
        HIPCHK(hipGetLastError());
        return BNR_OK;
    };
    return run_job(g, job, out, hook);
}
}   // namespace

int bnr_medge_abi_version(void) { return BNR_MEDGE_ABI_VERSION; }

int bnr_medge_set_option(const char *name, int64_t value) { return set_batch_draws("medge", name, value); }

int bnr_marginal_gamma(int32_t device, int32_t n, int32_t q, int32_t ndraws, const double *X, const double *y, const double *tau2, const double *mu,
                       const double *S, const double *W, double *m, double *v, int32_t *n_bad)
{
    if (!X || !y || !tau2 || !mu || !S) return fail(BNR_ERR_BAD_ARG, "NULL argument");
    if (!m && !v) return fail(BNR_ERR_BAD_ARG, "ask for m or v");
    call_guard g;
    mloo_job job;
    int rc;
    if ((rc = open_raw_job(g, job, device, n, q, ndraws, X, y, tau2, mu, S, W))) return rc;
    double *Md = nullptr, *Vd = nullptr;
    if ((rc = g.alloc(&Md, (size_t)q * (size_t)ndraws))) return rc;
    if ((rc = g.alloc(&Vd, (size_t)q * (size_t)ndraws))) return rc;
    mloo_out out;
    if ((rc = gamma_job(g, job, Md, Vd, out))) return rc;
    if (m && (rc = fetch_transposed(g, Md, q, ndraws, m))) return rc;
    if (v && (rc = fetch_transposed(g, Vd, q, ndraws, v))) return rc;
    if (n_bad) *n_bad = count_bad(out.bad);
    return BNR_OK;
}

int bnr_mixture_summary(int32_t device, int32_t q, int32_t K, int32_t nd, const double *m, const double *v, const double *weights, double p_lo,
                        double p_hi, double *mean, double *sd, double *var_within, double *p_pos, double *p_neg, double *lower, double *upper)
{
    if (!m || !v) return fail(BNR_ERR_BAD_ARG, "NULL argument");
    if (q < 1 || K < 1 || nd < 1) return fail(BNR_ERR_BAD_ARG, "need q >= 1 edges, K >= 1 chains and nd >= 1 draws per chain");
    if ((long long)K * nd > 0x7FFFFFFFll) return fail(BNR_ERR_BAD_ARG, "more than 2^31 - 1 pooled draws");
    const summary_out o{mean, sd, var_within, p_pos, p_neg, lower, upper};
    double c;
    int rc;
    if ((rc = summary_check(o, p_lo, p_hi, c))) return rc;
    std::vector<double> w;
    if ((rc = summary_weights(weights, K, w))) return rc;
    call_guard g;
    if ((rc = g.open(device))) return rc;
    double *Md = nullptr, *Vd = nullptr;
    if ((rc = upload_transposed(g, m, q, K * nd, &Md))) return rc;
    if ((rc = upload_transposed(g, v, q, K * nd, &Vd))) return rc;
    return summary_run(g, q, K, nd, Md, Vd, w, c, p_lo, p_hi, o);
}

int bnr_chains_marginal_edges(bnr_chain *const *chains, int32_t nchains, const double *weights, int32_t first_row, int32_t nsamp, int32_t thin,
                              double p_lo, double p_hi, double *mean, double *sd, double *var_within, double *p_pos, double *p_neg, double *lower,
                              double *upper, double *m, double *v, int32_t *n_bad)
{
    if (!chains) return fail(BNR_ERR_BAD_ARG, "NULL argument");
    int rc, nd;
    if ((rc = check_chain_list(chains, nchains, thin))) return rc;
    const summary_out o{mean, sd, var_within, p_pos, p_neg, lower, upper};
    double c;
    if ((rc = summary_check(o, p_lo, p_hi, c))) return rc;
    std::vector<double> w;
    if ((rc = summary_weights(weights, nchains, w))) return rc;
    call_guard g;
    mloo_job job;
    if ((rc = open_chain_job(g, job, chains, nchains, first_row, nsamp, thin, nd))) return rc;
    const int q = job.q, D = job.ndraws;
    double *Md = nullptr, *Vd = nullptr;
    if ((rc = g.alloc(&Md, (size_t)q * (size_t)D))) return rc;
    if ((rc = g.alloc(&Vd, (size_t)q * (size_t)D))) return rc;
    mloo_out out;
    if ((rc = gamma_job(g, job, Md, Vd, out))) return rc;
    if ((rc = summary_run(g, q, nchains, nd, Md, Vd, w, c, p_lo, p_hi, o))) return rc;
    if (m && (rc = fetch_transposed(g, Md, q, D, m))) return rc;
    if (v && (rc = fetch_transposed(g, Vd, q, D, v))) return rc;
    if (n_bad) *n_bad = count_bad(out.bad);
    return BNR_OK;
}
