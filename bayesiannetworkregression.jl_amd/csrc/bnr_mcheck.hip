// bnr_mcheck.hip -- libbnr_mcheck.so behind include/bnr_mcheck.h: the leave-one-out predictive checks of the training rows under the marginal
// PSIS weights, on the device.  A library and a gfx950 code object of its own: the four kernels of bnr_mloo_kernels.h (by #include, through
// bnr_mloo_job.h, the driver shared with the other marginal libraries: open_chain_job, run_job without a hook, and mloo_out, which leaves
// loglik, resid and var on the device) plus the three of bnr_mcheck_kernels.h; the outputs' checks and the launch loop of the two row kernels
// are bnr_mcheck_rows.h, shared with libbnr_mstack.so.  It reaches a chain through bnr_chain_device_view, runs PSIS through bnr_psis_weights and
// leaves its messages with bnr_set_last_error -- exported calls of libbnr_hip.so, nothing of bnr_internal.h.  Linked with bnr_mcheck.map: only
// the functions of the header are exported.
#include "../../include/bnr_mcheck.h"
#include "bnr_mcheck_kernels.h"
#include "bnr_mloo_job.h"
#include "bnr_mcheck_rows.h"

namespace {
// The three kernels on the device matrices A, V, LW (rows x D, a row's draws contiguous) and yd (rows, NULL: none), and the outputs asked for
// to the host.  a_is_resid: A holds resid = y - m (the chain form; it needs yd), else m itself.
int mix_run(call_guard &g, int rows, int D, const double *A, bool a_is_resid, const double *V, const double *LW, const double *yd, double c,
            double p_lo, double p_hi, const mix_out &o)
{
    int rc;
    const size_t total = (size_t)rows * (size_t)D;
    double *Wt = nullptr, *Isd = nullptr, *Mo = nullptr;
    if ((rc = g.alloc(&Wt, total))) return rc;
    if ((rc = g.alloc(&Isd, total))) return rc;
    if (a_is_resid && (rc = g.alloc(&Mo, total))) return rc;
    const unsigned sblocks = (unsigned)std::min<size_t>((total + 255) / 256, (size_t)1 << 16);
    return mix_rows(g, rows, D, a_is_resid ? Mo : A, V, Wt, Isd, yd, c, p_lo, p_hi, o, [&] {
        hipLaunchKernelGGL(k_mcheck_stage, dim3(sblocks), dim3(256), 0, g.st, LW, V, A, yd, (long long)total, D, Wt, Isd, Mo);
    });
}
}   // namespace

int bnr_mcheck_abi_version(void) { return BNR_MCHECK_ABI_VERSION; }

int bnr_mcheck_set_option(const char *name, int64_t value) { return set_batch_draws("mcheck", name, value); }

int bnr_weighted_mixture(int32_t device, int32_t rows, int32_t ndraws, const double *mean, const double *var, const double *logw, const double *y,
                         double p_lo, double p_hi, double *out_mean, double *out_sd, double *out_pit, double *out_lower, double *out_upper)
{
    if (!mean || !var || !logw) return fail(BNR_ERR_BAD_ARG, "NULL argument");
    const mix_out o{out_mean, out_sd, out_pit, out_lower, out_upper};
    if (!out_mean && !out_sd && !out_pit && !out_lower && !out_upper) return fail(BNR_ERR_BAD_ARG, "ask for at least one output");
    if (rows < 1 || ndraws < 1) return fail(BNR_ERR_BAD_ARG, "need rows >= 1 and ndraws >= 1");
    if ((long long)rows * ndraws > 0x7FFFFFFFll) return fail(BNR_ERR_BAD_ARG, "rows x ndraws must stay below 2^31");
    double c;
    if (const char *msg = mix_check(o, y != nullptr, p_lo, p_hi, c)) return fail(BNR_ERR_BAD_ARG, msg);
    call_guard g;
    int rc;
    if ((rc = g.open(device))) return rc;
    const size_t total = (size_t)rows * (size_t)ndraws;
    double *Md = nullptr, *Vd = nullptr, *Ld = nullptr, *yd = nullptr;
    if ((rc = g.upload(&Md, mean, total))) return rc;
    if ((rc = g.upload(&Vd, var, total))) return rc;
    if ((rc = g.upload(&Ld, logw, total))) return rc;
    if (y && (rc = g.upload(&yd, y, (size_t)rows))) return rc;
    return mix_run(g, rows, ndraws, Md, false, Vd, Ld, yd, c, p_lo, p_hi, o);
}

int bnr_chains_marginal_loo_predict(bnr_chain *const *chains, int32_t nchains, int32_t first_row, int32_t nsamp, int32_t thin, const double *r_eff,
                                    double p_lo, double p_hi, double *elpd_loo, double *pareto_k, double *loo_mean, double *loo_sd, double *loo_pit,
                                    double *loo_lower, double *loo_upper, double *logml, double *loglik, int32_t *n_bad)
{
    if (!chains || !elpd_loo || !pareto_k) return fail(BNR_ERR_BAD_ARG, "NULL argument");
    const mix_out o{loo_mean, loo_sd, loo_pit, loo_lower, loo_upper};
    const bool checks = loo_mean || loo_sd || loo_pit || loo_lower || loo_upper;
    double c;
    const char *also = mix_check(o, true, p_lo, p_hi, c);
    call_guard g;
    mloo_job job;
    int rc, nd;
    if ((rc = check_chain_list(chains, nchains, thin, also))) return rc;
    if ((rc = open_chain_job(g, job, chains, nchains, first_row, nsamp, thin, nd))) return rc;
    job.want_ll = true; job.want_resid = checks; job.want_var = checks;
    mloo_out out;
    if ((rc = run_job(g, job, out))) return rc;
    const int n = job.n, D = job.ndraws;
    const size_t nout = (size_t)n * (size_t)D;
    std::vector<double> ll(nout), lw(nout);
    if ((rc = g.fetch(ll.data(), out.loglik, nout))) return rc;
    if ((rc = bnr_psis_weights(job.v.device, n, D, ll.data(), r_eff, lw.data(), elpd_loo, pareto_k))) return rc;
    if (checks) {
        HIPCHK(hipSetDevice(job.v.device));
        double *Ld = nullptr;
        if ((rc = g.upload(&Ld, (const double *)lw.data(), nout))) return rc;
        if ((rc = mix_run(g, n, D, out.resid, true, out.var, Ld, job.v.y, c, p_lo, p_hi, o))) return rc;
    }
    if ((rc = g.fetch(logml, out.logml, (size_t)D))) return rc;
    if (loglik) std::copy(ll.begin(), ll.end(), loglik);
    if (n_bad) *n_bad = count_bad(out.bad);
    return BNR_OK;
}
