// bnr_mloo.hip -- libbnr_mloo.so behind include/bnr_mloo.h: marginal PSIS-LOO, the edge coefficients integrated out on the device, over the
// kernels of bnr_mloo_kernels.h.  A library and a gfx950 code object of its own: libbnr_hip.so's two stay what they are.  It reaches a chain
// through bnr_chain_device_view, runs PSIS through bnr_psis_weights and leaves its messages with bnr_set_last_error -- the exported calls of
// libbnr_hip.so, nothing of bnr_internal.h.
// The driver of a call (call_guard, mloo_job, run_job) is bnr_mloo_job.h, shared with libbnr_medge.so; this library passes run_job no hook.
#include "bnr_mloo_job.h"

int bnr_mloo_abi_version(void) { return BNR_MLOO_ABI_VERSION; }

int bnr_mloo_set_option(const char *name, int64_t value)
{
    if (!name) return fail(BNR_ERR_BAD_ARG, "NULL argument");
    if (std::string(name) == "mloo_batch_draws") {
        if (value < 0) return fail(BNR_ERR_BAD_ARG, "mloo_batch_draws must be >= 0");
        opt_batch_draws.store(value);
        return BNR_OK;
    }
    return fail(BNR_ERR_BAD_ARG, std::string("unknown option ") + name);
}

int bnr_marginal_loglik(int32_t device, int32_t n, int32_t q, int32_t ndraws, const double *X, const double *y, const double *tau2, const double *mu,
                        const double *S, const double *W, double *loglik, double *resid, double *var, double *logml, int32_t *n_bad)
{
    if (!X || !y || !tau2 || !mu || !S) return fail(BNR_ERR_BAD_ARG, "NULL argument");
    if (!loglik && !resid && !var) return fail(BNR_ERR_BAD_ARG, "ask for loglik, resid or var");
    if (n < 1 || q < 1 || ndraws < 1) return fail(BNR_ERR_BAD_ARG, "need n >= 1 rows, q >= 1 edges and ndraws >= 1 draws");
    if (n > BNR_MLOO_MAX_N) return fail(BNR_ERR_BAD_ARG, "n > 2048 is not supported by this version");
    call_guard g;
    int rc;
    if ((rc = g.open(device))) return rc;
    mloo_job job;
    job.n = n; job.q = q; job.ndraws = ndraws; job.ldx = n;
    double *Xd = nullptr, *yd = nullptr;
    if ((rc = g.upload(&Xd, X, (size_t)n * (size_t)q))) return rc;
    if ((rc = g.upload(&yd, y, (size_t)n))) return rc;
    if ((rc = g.upload(&job.tau2, tau2, (size_t)ndraws))) return rc;
    if ((rc = g.upload(&job.mu, mu, (size_t)ndraws))) return rc;
    job.X = Xd; job.y = yd; job.hS = S; job.hW = W; job.has_w = W != nullptr;
    job.want_ll = loglik != nullptr; job.want_resid = resid != nullptr; job.want_var = var != nullptr;
    std::vector<double> ll, rs, vr, lm;
    std::vector<int> bad;
    if ((rc = run_job(g, job, ll, rs, vr, lm, bad))) return rc;
    const size_t nout = (size_t)n * (size_t)ndraws;
    if (loglik) std::copy(ll.begin(), ll.begin() + nout, loglik);
    if (resid) std::copy(rs.begin(), rs.begin() + nout, resid);
    if (var) std::copy(vr.begin(), vr.begin() + nout, var);
    if (logml) std::copy(lm.begin(), lm.end(), logml);
    if (n_bad) { int nb = 0; for (int f : bad) nb += f != 0; *n_bad = nb; }
    return BNR_OK;
}

int bnr_chains_marginal_loo(bnr_chain *const *chains, int32_t nchains, int32_t first_row, int32_t nsamp, int32_t thin, const double *r_eff,
                            double *elpd_loo, double *pareto_k, double *loo_mean, double *loo_sd, double *logml, double *loglik, int32_t *n_bad)
{
    if (!chains || !elpd_loo || !pareto_k) return fail(BNR_ERR_BAD_ARG, "NULL argument");
    if (nchains < 1) return fail(BNR_ERR_BAD_ARG, "need nchains >= 1");
    if (thin < 1) return fail(BNR_ERR_BAD_ARG, "need thin >= 1");
    for (int i = 0; i < nchains; ++i) {
        if (!chains[i]) return fail(BNR_ERR_BAD_ARG, "NULL chain");
        for (int k = 0; k < i; ++k) if (chains[k] == chains[i]) return fail(BNR_ERR_BAD_ARG, "chain listed twice");
    }
    std::vector<bnr_chain_view> v(nchains);
    int rc;
    for (int i = 0; i < nchains; ++i) {
        if ((rc = bnr_chain_device_view(chains[i], &v[i]))) return rc;
        if (v[i].device != v[0].device || v[i].n != v[0].n || v[i].V != v[0].V || v[i].R != v[0].R || v[i].rowlen != v[0].rowlen)
            return fail(BNR_ERR_BAD_ARG, "pooled chains must live on one device and have equal n, V, R");
    }
    for (int i = 0; i < nchains; ++i)
        if (first_row < 1 || nsamp < 1 || (long long)first_row + nsamp - 1 > v[i].tot) return fail(BNR_ERR_BAD_ARG, "row window outside the table");
    const int nd = (nsamp + thin - 1) / thin;
    if ((long long)nchains * nd > 0x7FFFFFFFll) return fail(BNR_ERR_BAD_ARG, "more than 2^31 - 1 pooled draws");
    const int n = v[0].n, D = nchains * nd;
    if (n > BNR_MLOO_MAX_N) return fail(BNR_ERR_BAD_ARG, "n > 2048 is not supported by this version");
    call_guard g;
    if ((rc = g.open(v[0].device))) return rc;
    mloo_job job;
    job.n = n; job.q = v[0].q; job.ndraws = D; job.ldx = v[0].ldx; job.X = v[0].X; job.y = v[0].y; job.v = v[0];
    job.chain_form = true; job.has_w = true;
    job.want_ll = true; job.want_resid = loo_mean || loo_sd; job.want_var = loo_sd != nullptr;
    std::vector<const double *> hrow(D);
    for (int k = 0; k < nchains; ++k)
        for (int j = 0; j < nd; ++j) hrow[(size_t)k * nd + j] = v[k].trace + ((size_t)(first_row - 1) + (size_t)j * thin) * (size_t)v[k].rowlen;
    const double **rowp = nullptr;
    if ((rc = g.upload(&rowp, hrow.data(), (size_t)D))) return rc;
    HIPCHK(hipStreamSynchronize(g.st));
    job.rowp = rowp; job.hrow = hrow.data();
    if ((rc = g.alloc(&job.tau2, (size_t)D))) return rc;
    if ((rc = g.alloc(&job.mu, (size_t)D))) return rc;
    std::vector<double> ll, rs, vr, lm, yh(n);
    std::vector<int> bad;
    if ((rc = run_job(g, job, ll, rs, vr, lm, bad))) return rc;
    HIPCHK(hipMemcpy(yh.data(), v[0].y, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost));
    std::vector<double> lw((size_t)n * (size_t)D);
    if ((rc = bnr_psis_weights(v[0].device, n, D, ll.data(), r_eff, lw.data(), elpd_loo, pareto_k))) return rc;
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
    if (logml) std::copy(lm.begin(), lm.end(), logml);
    if (loglik) std::copy(ll.begin(), ll.end(), loglik);
    if (n_bad) { int nb = 0; for (int f : bad) nb += f != 0; *n_bad = nb; }
    return BNR_OK;
}
