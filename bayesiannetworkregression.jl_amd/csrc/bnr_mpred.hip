// bnr_mpred.hip -- libbnr_mpred.so behind include/bnr_mpred.h: Rao-Blackwellised prediction of new rows, gamma integrated out on the device.
// A library and a gfx950 code object of its own: the four kernels of bnr_mloo_kernels.h and the two of bnr_medge_kernels.h (by #include, through
// the drivers shared with the other marginal libraries: bnr_mloo_job.h opens the job of either form and runs its batches, bnr_medge_summary.h
// (libbnr_medge.so's and libbnr_mcov.so's too) holds the summary and the transposing copies; k_medge_proj rides along unused) plus the four of
// bnr_mpred_kernels.h.  It reaches a chain through bnr_chain_device_view and leaves its messages with bnr_set_last_error -- exported
// calls of libbnr_hip.so, nothing of bnr_internal.h.  Linked with bnr_mpred.map: only the functions of the header are exported.
#include "../../include/bnr_mpred.h"
#include "bnr_mpred_kernels.h"
#include "bnr_mloo_job.h"
#include "bnr_medge_summary.h"

namespace {
std::atomic<long long> opt_block_rows{0};               // "mpred_block_rows" (0: automatic)

// mean, var and var + tau2 of every draw of the job for the new rows Xn (m x q column-major on the device), row-major per new row on the device
// (Md, Vd, Pd: m x ndraws; resid and var stay there too), behind every batch's k_mloo_factor: k_mpred_rhs once per batch, then k_mpred_cross and k_mpred_proj per block of rows
int predict_job(call_guard &g, mloo_job &job, const double *Xn, int m, double *Md, double *Vd, double *Pd, mloo_out &out)
{
    job.want_ll = false; job.want_resid = true; job.want_var = true;
    const long long D = job.ndraws;
    double *a = nullptr, *dq = nullptr, *C = nullptr;
    int MB = 0;                                         // new rows per block; a draw's block of C: np x round_up(MB, MLOO_TILE) doubles
    size_t cstride = 0;
    mloo_hook hook = [&](const mloo_batch &bt) -> int {
        int rc;
        if (!C) {                                       // (the first batch is the largest of the call)
            const long long mp = round_up(m, MLOO_TILE);
            long long mbp = ((long long)1 << 27) / ((long long)bt.nb * bt.np) / MLOO_TILE * MLOO_TILE;
            mbp = std::max<long long>(MLOO_TILE, std::min<long long>(mbp, mp));
            const long long o = opt_block_rows.load();
            MB = (int)std::min<long long>(o > 0 ? o : mbp, m);
            cstride = (size_t)bt.np * (size_t)round_up(MB, MLOO_TILE);
            if ((rc = g.alloc(&a, (size_t)bt.nb * (size_t)m))) return rc;
            if ((rc = g.alloc(&dq, (size_t)bt.nb * (size_t)m))) return rc;
            if ((rc = g.alloc(&C, (size_t)bt.nb * cstride))) return rc;
        }
        hipLaunchKernelGGL(k_mpred_rhs, dim3((m + 255) / 256, (bt.nb + MPRED_RB - 1) / MPRED_RB), dim3(256), 0, g.st, Xn, m, m, job.q, bt.Sp, bt.Wbuf, bt.nb,
                           a, dq);
        const int nt = bt.np / MLOO_TILE;
        for (int j0 = 0; j0 < m; j0 += MB) {
            const int mblk = std::min(MB, m - j0), ntj = (mblk + MLOO_TILE - 1) / MLOO_TILE;
            hipLaunchKernelGGL(k_mpred_cross, dim3(nt * ntj, (bt.nb + MLOO_DB - 1) / MLOO_DB), dim3(256), 0, g.st, job.X, job.ldx, job.n, job.q, Xn, m, j0,
                               mblk, bt.Sp, bt.nb, C, bt.np, (long long)cstride);
            hipLaunchKernelGGL(k_mpred_proj, dim3((mblk + MPRED_JB - 1) / MPRED_JB, bt.nb), dim3(256), 0, g.st, (const double *)C, (long long)cstride, job.n,
                               bt.np, j0, mblk, m, bt.G, (long long)bt.mat, (const double *)a, (const double *)dq, bt.tau2, bt.mu, bt.resid, bt.var,
                               bt.bad, bt.s0, D, Md, Vd, Pd);
        }
        HIPCHK(hipGetLastError());
        return BNR_OK;
    };
    return run_job(g, job, out, hook);
}

// k_mpred_score on the row-major device matrices Md, Pd (m x K nd) and its results to the host
int score_run(call_guard &g, int m, int K, int nd, const double *Md, const double *Pd, const double *yd, const std::vector<double> &w, double *lpd,
              double *pit)
{
    int rc;
    double *wd = nullptr, *out = nullptr;
    if ((rc = g.upload(&wd, w.data(), (size_t)K))) return rc;
    if ((rc = g.alloc(&out, (size_t)2 * m))) return rc;
    double *dl = lpd ? out : nullptr, *dp = pit ? out + m : nullptr;
    hipLaunchKernelGGL(k_mpred_score, dim3((m + 3) / 4), dim3(256), 0, g.st, Md, Pd, (long long)K * nd, m, K, nd, (const double *)wd, yd, dl, dp);
    HIPCHK(hipGetLastError());
    if (lpd) HIPCHK(hipMemcpyAsync(lpd, dl, sizeof(double) * (size_t)m, hipMemcpyDeviceToHost, g.st));
    if (pit) HIPCHK(hipMemcpyAsync(pit, dp, sizeof(double) * (size_t)m, hipMemcpyDeviceToHost, g.st));
    HIPCHK(hipStreamSynchronize(g.st));
    HIPCHK(hipGetLastError());
    return BNR_OK;
}
}   // namespace

int bnr_mpred_abi_version(void) { return BNR_MPRED_ABI_VERSION; }

int bnr_mpred_set_option(const char *name, int64_t value)
{
    if (name && std::string(name) == "mpred_block_rows") {
        if (value < 0 || value > 0x7FFFFFFFll) return fail(BNR_ERR_BAD_ARG, "mpred_block_rows must be >= 0 and < 2^31");
        opt_block_rows.store(value);
        return BNR_OK;
    }
    return set_batch_draws("mpred", name, value);
}

int bnr_marginal_predict(int32_t device, int32_t n, int32_t q, int32_t m, int32_t ndraws, const double *X, const double *y, const double *Xnew,
                         const double *tau2, const double *mu, const double *S, const double *W, double *mean, double *var, int32_t *n_bad)
{
    if (!X || !y || !Xnew || !tau2 || !mu || !S) return fail(BNR_ERR_BAD_ARG, "NULL argument");
    if (!mean && !var) return fail(BNR_ERR_BAD_ARG, "ask for mean or var");
    call_guard g;
    mloo_job job;
    int rc;
    if ((rc = open_raw_job(g, job, device, n, q, ndraws, X, y, tau2, mu, S, W, m < 1 ? "need m >= 1 new rows" : nullptr))) return rc;
    double *Xn = nullptr, *Md = nullptr, *Vd = nullptr, *Pd = nullptr;
    if ((rc = g.upload(&Xn, Xnew, (size_t)m * (size_t)q))) return rc;
    if ((rc = g.alloc(&Md, (size_t)m * (size_t)ndraws))) return rc;
    if ((rc = g.alloc(&Vd, (size_t)m * (size_t)ndraws))) return rc;
    if ((rc = g.alloc(&Pd, (size_t)m * (size_t)ndraws))) return rc;
    mloo_out out;
    if ((rc = predict_job(g, job, Xn, m, Md, Vd, Pd, out))) return rc;
    if (mean && (rc = fetch_transposed(g, Md, m, ndraws, mean))) return rc;
    if (var && (rc = fetch_transposed(g, Vd, m, ndraws, var))) return rc;
    if (n_bad) *n_bad = count_bad(out.bad);
    return BNR_OK;
}

int bnr_mixture_score(int32_t device, int32_t m, int32_t K, int32_t nd, const double *mean, const double *vobs, const double *y,
                      const double *weights, double *lpd, double *pit)
{
    if (!mean || !vobs || !y) return fail(BNR_ERR_BAD_ARG, "NULL argument");
    if (!lpd && !pit) return fail(BNR_ERR_BAD_ARG, "ask for lpd or pit");
    if (m < 1 || K < 1 || nd < 1) return fail(BNR_ERR_BAD_ARG, "need m >= 1 rows, K >= 1 chains and nd >= 1 draws per chain");
    if ((long long)K * nd > 0x7FFFFFFFll) return fail(BNR_ERR_BAD_ARG, "more than 2^31 - 1 pooled draws");
    int rc;
    std::vector<double> w;
    if ((rc = summary_weights(weights, K, w))) return rc;
    call_guard g;
    if ((rc = g.open(device))) return rc;
    const int D = K * nd;
    double *Md = nullptr, *Pd = nullptr, *yd = nullptr;
    if ((rc = upload_transposed(g, mean, m, D, &Md))) return rc;
    if ((rc = upload_transposed(g, vobs, m, D, &Pd))) return rc;
    if ((rc = g.upload(&yd, y, (size_t)m))) return rc;
    return score_run(g, m, K, nd, Md, Pd, yd, w, lpd, pit);
}

int bnr_chains_marginal_predict(bnr_chain *const *chains, int32_t nchains, const double *weights, int32_t first_row, int32_t nsamp, int32_t thin,
                                const double *Xnew, int32_t m, const double *ynew, double p_lo, double p_hi, double *mean, double *sd,
                                double *var_within, double *lower, double *upper, double *pred_sd, double *pred_lower, double *pred_upper,
                                double *lpd, double *pit, double *dmean, double *dvar, int32_t *n_bad)
{
    if (!chains || !Xnew) return fail(BNR_ERR_BAD_ARG, "NULL argument");
    int rc, nd;
    if ((rc = check_chain_list(chains, nchains, thin, m < 1 ? "need m >= 1 new rows" : nullptr))) return rc;
    const summary_out oe{mean, sd, var_within, nullptr, nullptr, lower, upper}, op{nullptr, pred_sd, nullptr, nullptr, nullptr, pred_lower, pred_upper};
    const bool want_e = mean || sd || var_within || lower || upper, want_p = pred_sd || pred_lower || pred_upper;
    if (!want_e && !want_p && !lpd && !pit && !dmean && !dvar) return fail(BNR_ERR_BAD_ARG, "ask for at least one output");
    if ((lpd || pit) && !ynew) return fail(BNR_ERR_BAD_ARG, "lpd and pit need ynew");
    double ce = 1.0, cp = 1.0;
    if (want_e && (rc = summary_check(oe, p_lo, p_hi, ce))) return rc;
    if (want_p && (rc = summary_check(op, p_lo, p_hi, cp))) return rc;
    std::vector<double> w;
    if ((rc = summary_weights(weights, nchains, w))) return rc;
    call_guard g;
    mloo_job job;
    if ((rc = open_chain_job(g, job, chains, nchains, first_row, nsamp, thin, nd))) return rc;
    const int q = job.q, D = job.ndraws;
    double *Xn = nullptr, *yd = nullptr, *Md = nullptr, *Vd = nullptr, *Pd = nullptr;
    if ((rc = g.upload(&Xn, Xnew, (size_t)m * (size_t)q))) return rc;
    if (ynew && (rc = g.upload(&yd, ynew, (size_t)m))) return rc;
    if ((rc = g.alloc(&Md, (size_t)m * (size_t)D))) return rc;
    if ((rc = g.alloc(&Vd, (size_t)m * (size_t)D))) return rc;
    if ((rc = g.alloc(&Pd, (size_t)m * (size_t)D))) return rc;
    mloo_out out;
    if ((rc = predict_job(g, job, Xn, m, Md, Vd, Pd, out))) return rc;
    if (want_e && (rc = summary_run(g, m, nchains, nd, Md, Vd, w, ce, p_lo, p_hi, oe))) return rc;
    if (want_p && (rc = summary_run(g, m, nchains, nd, Md, Pd, w, cp, p_lo, p_hi, op))) return rc;
    if ((lpd || pit) && (rc = score_run(g, m, nchains, nd, Md, Pd, yd, w, lpd, pit))) return rc;
    if (dmean && (rc = fetch_transposed(g, Md, m, D, dmean))) return rc;
    if (dvar && (rc = fetch_transposed(g, Vd, m, D, dvar))) return rc;
    if (n_bad) *n_bad = count_bad(out.bad);
    return BNR_OK;
}
