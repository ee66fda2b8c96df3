// bnr_medge.hip -- libbnr_medge.so behind include/bnr_medge.h: Rao-Blackwellised summaries of the edge coefficients, gamma integrated out on the
// device.  A library and a gfx950 code object of its own: the four kernels of bnr_mloo_kernels.h (by #include, through the driver shared with
// libbnr_mloo.so, bnr_mloo_job.h) plus k_medge_proj and k_medge_summary (bnr_medge_kernels.h); the summary's host driver is bnr_medge_summary.h,
// shared with libbnr_mpred.so.  It reaches a chain through bnr_chain_device_view and leaves its messages with bnr_set_last_error -- exported calls
// of libbnr_hip.so, nothing of bnr_internal.h.
// Linked with bnr_medge.map: only the functions of the header are exported, so that neither this library nor libbnr_mloo.so, loaded into one
// process, can bind the other's kernel handles or host stubs.
#include "../../include/bnr_medge.h"
#include "bnr_medge_kernels.h"
#include "bnr_mloo_job.h"
#include "bnr_medge_summary.h"

namespace {
// m and v of every draw of the job, edge-major on the device (Md, Vd: q x ndraws), by k_medge_proj behind every batch's k_mloo_factor
int gamma_job(call_guard &g, mloo_job &job, double *Md, double *Vd, std::vector<int> &bad)
{
    job.want_ll = false; job.want_resid = true; job.want_var = true;
    std::vector<double> ll, rs, vr, lm;
    const long long D = job.ndraws;
    mloo_hook hook = [&](const mloo_batch &bt) -> int {
        hipLaunchKernelGGL(k_medge_proj, dim3((job.q + MEDGE_EB - 1) / MEDGE_EB, (bt.nb + MEDGE_DB - 1) / MEDGE_DB), dim3(256), 0, g.st, job.X, job.ldx,
                           job.n, bt.np, job.q, bt.G, (long long)bt.mat, bt.Sp, bt.Wbuf, bt.tau2, bt.resid, bt.var, bt.bad, bt.s0, D, bt.nb, Md, Vd);
        HIPCHK(hipGetLastError());
        return BNR_OK;
    };
    return run_job(g, job, ll, rs, vr, lm, bad, hook);
}
}   // namespace

int bnr_medge_abi_version(void) { return BNR_MEDGE_ABI_VERSION; }

int bnr_medge_set_option(const char *name, int64_t value)
{
    if (!name) return fail(BNR_ERR_BAD_ARG, "NULL argument");
    if (std::string(name) == "medge_batch_draws") {
        if (value < 0) return fail(BNR_ERR_BAD_ARG, "medge_batch_draws must be >= 0");
        opt_batch_draws.store(value);
        return BNR_OK;
    }
    return fail(BNR_ERR_BAD_ARG, std::string("unknown option ") + name);
}

int bnr_marginal_gamma(int32_t device, int32_t n, int32_t q, int32_t ndraws, const double *X, const double *y, const double *tau2, const double *mu,
                       const double *S, const double *W, double *m, double *v, int32_t *n_bad)
{
    if (!X || !y || !tau2 || !mu || !S) return fail(BNR_ERR_BAD_ARG, "NULL argument");
    if (!m && !v) return fail(BNR_ERR_BAD_ARG, "ask for m or v");
    if (n < 1 || q < 1 || ndraws < 1) return fail(BNR_ERR_BAD_ARG, "need n >= 1 rows, q >= 1 edges and ndraws >= 1 draws");
    if (n > BNR_MLOO_MAX_N) return fail(BNR_ERR_BAD_ARG, "n > 2048 is not supported by this version");
    call_guard g;
    int rc;
    if ((rc = g.open(device))) return rc;
    mloo_job job;
    job.n = n; job.q = q; job.ndraws = ndraws; job.ldx = n;
    double *Xd = nullptr, *yd = nullptr, *Md = nullptr, *Vd = nullptr;
    if ((rc = g.upload(&Xd, X, (size_t)n * (size_t)q))) return rc;
    if ((rc = g.upload(&yd, y, (size_t)n))) return rc;
    if ((rc = g.upload(&job.tau2, tau2, (size_t)ndraws))) return rc;
    if ((rc = g.upload(&job.mu, mu, (size_t)ndraws))) return rc;
    if ((rc = g.alloc(&Md, (size_t)q * (size_t)ndraws))) return rc;
    if ((rc = g.alloc(&Vd, (size_t)q * (size_t)ndraws))) return rc;
    job.X = Xd; job.y = yd; job.hS = S; job.hW = W; job.has_w = W != nullptr;
    std::vector<int> bad;
    if ((rc = gamma_job(g, job, Md, Vd, bad))) return rc;
    if (m && (rc = fetch_transposed(g, Md, q, ndraws, m))) return rc;
    if (v && (rc = fetch_transposed(g, Vd, q, ndraws, v))) return rc;
    if (n_bad) { int nb = 0; for (int f : bad) nb += f != 0; *n_bad = nb; }
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
    const int D = K * nd;
    std::vector<double> t((size_t)q * (size_t)D);
    double *Md = nullptr, *Vd = nullptr;
    for (int s = 0; s < D; ++s)
        for (int e = 0; e < q; ++e) t[(size_t)e * D + s] = m[(size_t)s * q + e];
    if ((rc = g.upload(&Md, t.data(), t.size()))) return rc;
    HIPCHK(hipStreamSynchronize(g.st));                                  // (t is reused)
    for (int s = 0; s < D; ++s)
        for (int e = 0; e < q; ++e) t[(size_t)e * D + s] = v[(size_t)s * q + e];
    if ((rc = g.upload(&Vd, t.data(), t.size()))) return rc;
    HIPCHK(hipStreamSynchronize(g.st));
    return summary_run(g, q, K, nd, Md, Vd, w, c, p_lo, p_hi, o);
}

int bnr_chains_marginal_edges(bnr_chain *const *chains, int32_t nchains, const double *weights, int32_t first_row, int32_t nsamp, int32_t thin,
                              double p_lo, double p_hi, double *mean, double *sd, double *var_within, double *p_pos, double *p_neg, double *lower,
                              double *upper, double *m, double *v, int32_t *n_bad)
{
    if (!chains) return fail(BNR_ERR_BAD_ARG, "NULL argument");
    if (nchains < 1) return fail(BNR_ERR_BAD_ARG, "need nchains >= 1");
    if (thin < 1) return fail(BNR_ERR_BAD_ARG, "need thin >= 1");
    for (int i = 0; i < nchains; ++i) {
        if (!chains[i]) return fail(BNR_ERR_BAD_ARG, "NULL chain");
        for (int k = 0; k < i; ++k) if (chains[k] == chains[i]) return fail(BNR_ERR_BAD_ARG, "chain listed twice");
    }
    const summary_out o{mean, sd, var_within, p_pos, p_neg, lower, upper};
    double c;
    int rc;
    if ((rc = summary_check(o, p_lo, p_hi, c))) return rc;
    std::vector<double> w;
    if ((rc = summary_weights(weights, nchains, w))) return rc;
    std::vector<bnr_chain_view> vw(nchains);
    for (int i = 0; i < nchains; ++i) {
        if ((rc = bnr_chain_device_view(chains[i], &vw[i]))) return rc;
        if (vw[i].device != vw[0].device || vw[i].n != vw[0].n || vw[i].V != vw[0].V || vw[i].R != vw[0].R || vw[i].rowlen != vw[0].rowlen)
            return fail(BNR_ERR_BAD_ARG, "pooled chains must live on one device and have equal n, V, R");
    }
    for (int i = 0; i < nchains; ++i)
        if (first_row < 1 || nsamp < 1 || (long long)first_row + nsamp - 1 > vw[i].tot) return fail(BNR_ERR_BAD_ARG, "row window outside the table");
    const int nd = (nsamp + thin - 1) / thin;
    if ((long long)nchains * nd > 0x7FFFFFFFll) return fail(BNR_ERR_BAD_ARG, "more than 2^31 - 1 pooled draws");
    const int n = vw[0].n, q = vw[0].q, D = nchains * nd;
    if (n > BNR_MLOO_MAX_N) return fail(BNR_ERR_BAD_ARG, "n > 2048 is not supported by this version");
    call_guard g;
    if ((rc = g.open(vw[0].device))) return rc;
    mloo_job job;
    job.n = n; job.q = q; job.ndraws = D; job.ldx = vw[0].ldx; job.X = vw[0].X; job.y = vw[0].y; job.v = vw[0];
    job.chain_form = true; job.has_w = true;
    std::vector<const double *> hrow(D);
    for (int k = 0; k < nchains; ++k)
        for (int j = 0; j < nd; ++j) hrow[(size_t)k * nd + j] = vw[k].trace + ((size_t)(first_row - 1) + (size_t)j * thin) * (size_t)vw[k].rowlen;
    const double **rowp = nullptr;
    if ((rc = g.upload(&rowp, hrow.data(), (size_t)D))) return rc;
    HIPCHK(hipStreamSynchronize(g.st));
    job.rowp = rowp; job.hrow = hrow.data();
    if ((rc = g.alloc(&job.tau2, (size_t)D))) return rc;
    if ((rc = g.alloc(&job.mu, (size_t)D))) return rc;
    double *Md = nullptr, *Vd = nullptr;
    if ((rc = g.alloc(&Md, (size_t)q * (size_t)D))) return rc;
    if ((rc = g.alloc(&Vd, (size_t)q * (size_t)D))) return rc;
    std::vector<int> bad;
    if ((rc = gamma_job(g, job, Md, Vd, bad))) return rc;
    if ((rc = summary_run(g, q, nchains, nd, Md, Vd, w, c, p_lo, p_hi, o))) return rc;
    if (m && (rc = fetch_transposed(g, Md, q, D, m))) return rc;
    if (v && (rc = fetch_transposed(g, Vd, q, D, v))) return rc;
    if (n_bad) { int nb = 0; for (int f : bad) nb += f != 0; *n_bad = nb; }
    return BNR_OK;
}
