// bnr_mloo.hip -- libbnr_mloo.so behind include/bnr_mloo.h: marginal PSIS-LOO, the edge coefficients integrated out on the device, over the
// kernels of bnr_mloo_kernels.h.  A library and a gfx950 code object of its own: libbnr_hip.so's two stay what they are.  It reaches a chain
// through bnr_chain_device_view, runs PSIS through bnr_psis_weights and leaves its messages with bnr_set_last_error -- the exported calls of
// libbnr_hip.so, nothing of bnr_internal.h.
// The driver of a call (call_guard, mloo_job, open_chain_job / open_raw_job, run_job) is bnr_mloo_job.h, shared with the five other marginal
// libraries; this library passes run_job no hook and fetches loglik, resid, var and logml as its outputs need them.
#include "bnr_mloo_job.h"

int bnr_mloo_abi_version(void) { return BNR_MLOO_ABI_VERSION; }

int bnr_mloo_set_option(const char *name, int64_t value) { return set_batch_draws("mloo", name, value); }

int bnr_marginal_loglik(int32_t device, int32_t n, int32_t q, int32_t ndraws, const double *X, const double *y, const double *tau2, const double *mu,
                        const double *S, const double *W, double *loglik, double *resid, double *var, double *logml, int32_t *n_bad)
{
    if (!X || !y || !tau2 || !mu || !S) return fail(BNR_ERR_BAD_ARG, "NULL argument");
    if (!loglik && !resid && !var) return fail(BNR_ERR_BAD_ARG, "ask for loglik, resid or var");
    call_guard g;
    mloo_job job;
    int rc;
    if ((rc = open_raw_job(g, job, device, n, q, ndraws, X, y, tau2, mu, S, W))) return rc;
    job.want_ll = loglik != nullptr; job.want_resid = resid != nullptr; job.want_var = var != nullptr;
    mloo_out out;
    if ((rc = run_job(g, job, out))) return rc;
    const size_t nout = (size_t)n * (size_t)ndraws;
    if ((rc = g.fetch(loglik, out.loglik, nout))) return rc;
    if ((rc = g.fetch(resid, out.resid, nout))) return rc;
    if ((rc = g.fetch(var, out.var, nout))) return rc;
    if ((rc = g.fetch(logml, out.logml, (size_t)ndraws))) return rc;
    if (n_bad) *n_bad = count_bad(out.bad);
    return BNR_OK;
}

int bnr_chains_marginal_loo(bnr_chain *const *chains, int32_t nchains, int32_t first_row, int32_t nsamp, int32_t thin, const double *r_eff,
                            double *elpd_loo, double *pareto_k, double *loo_mean, double *loo_sd, double *logml, double *loglik, int32_t *n_bad)
{
    if (!chains || !elpd_loo || !pareto_k) return fail(BNR_ERR_BAD_ARG, "NULL argument");
    call_guard g;
    mloo_job job;
    int rc, nd;
    if ((rc = check_chain_list(chains, nchains, thin))) return rc;
    if ((rc = open_chain_job(g, job, chains, nchains, first_row, nsamp, thin, nd))) return rc;
    job.want_ll = true; job.want_resid = loo_mean || loo_sd; job.want_var = loo_sd != nullptr;
    mloo_out out;
    if ((rc = run_job(g, job, out))) return rc;
    const int n = job.n, D = job.ndraws;
    const size_t nout = (size_t)n * (size_t)D;
    std::vector<double> ll(nout), rs(job.want_resid ? nout : 0), vr(job.want_var ? nout : 0), yh(n), lw(nout);
    if ((rc = g.fetch(ll.data(), out.loglik, nout))) return rc;
    if (job.want_resid && (rc = g.fetch(rs.data(), out.resid, nout))) return rc;
    if (job.want_var && (rc = g.fetch(vr.data(), out.var, nout))) return rc;
    if ((rc = g.fetch(yh.data(), job.v.y, (size_t)n))) return rc;
    if ((rc = bnr_psis_weights(job.v.device, n, D, ll.data(), r_eff, lw.data(), elpd_loo, pareto_k))) return rc;
    if (loo_mean || loo_sd) {
        for (int i = 0; i < n; ++i) {
            const double *w = lw.data() + (size_t)i * D, *ri = rs.data() + (size_t)i * D, *vi = loo_sd ? vr.data() + (size_t)i * D : nullptr;
            double a = 0.0, b = 0.0;
            for (int s = 0; s < D; ++s) {
                const double ws = std::exp(w[s]);
                a = a + ws * ri[s];
                if (vi) { const double ms = yh[i] - ri[s]; b = b + ws * (vi[s] + ms * ms); }
            }
            const double mean = yh[i] - a;
            if (loo_mean) loo_mean[i] = mean;
            if (loo_sd) loo_sd[i] = std::sqrt(b - mean * mean);
        }
    }
    if ((rc = g.fetch(logml, out.logml, (size_t)D))) return rc;
    if (loglik) std::copy(ll.begin(), ll.end(), loglik);
    if (n_bad) *n_bad = count_bad(out.bad);
    return BNR_OK;
}
