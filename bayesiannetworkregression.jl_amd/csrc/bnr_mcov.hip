// bnr_mcov.hip -- libbnr_mcov.so behind include/bnr_mcov.h: the Rao-Blackwellised covariance of the edge coefficients, gamma integrated out on the
// device.  A library and a gfx950 code object of its own: the four kernels of bnr_mloo_kernels.h and the two of bnr_medge_kernels.h (by #include,
// through the driver shared with the other marginal libraries, bnr_mloo_job.h, and the summary's helpers, bnr_medge_summary.h) plus the four of
// bnr_mcov_kernels.h.  It reaches a chain through bnr_chain_device_view and leaves its messages with bnr_set_last_error -- exported calls of
// libbnr_hip.so, nothing of bnr_internal.h.
// Linked with bnr_mcov.map: only the functions of the header are exported, so that neither this library nor another marginal library, loaded into
// one process, can bind the other's kernel handles or host stubs.
#include "../../include/bnr_mcov.h"
#include "bnr_mcov_kernels.h"
#include "bnr_mloo_job.h"
#include "bnr_medge_summary.h"

namespace {
// the column list of a call over q edges: cols as given (every index in 0 .. q - 1), or 0 .. q - 1 for NULL -- bnr_chains_cov's rules and messages
int cov_cols(int32_t ncols, const int32_t *cols, int q, std::vector<int32_t> &out)
{
    if (ncols < 1) return fail(BNR_ERR_BAD_ARG, "need ncols >= 1 columns");
    if (!cols && ncols != q) return fail(BNR_ERR_BAD_ARG, "cols == NULL means every column: ncols must be " + std::to_string(q));
    out.resize(ncols);
    for (int p = 0; p < ncols; ++p) {
        out[p] = cols ? cols[p] : p;
        if (out[p] < 0 || out[p] >= q) return fail(BNR_ERR_BAD_ARG, "column index outside 0 .. " + std::to_string(q - 1));
    }
    return BNR_OK;
}

struct cov_out { double *mean, *cov, *within, *m, *v; int32_t *n_bad; };

// Everything behind an opened job of K chains of nd draws.  Per batch of run_job, behind its k_mloo_factor: sub-batches of as many draws as keep
// the panel T' near 1 GiB, each a k_mcov_proj and then one k_mcov_gram per chain that has draws in it (a launch never crosses a chain: it
// continues that chain's accumulators).  Behind the batches: k_medge_summary for mean and the diagonal's sums, k_mcov_center, the between Gram of
// every chain, k_mcov_finish.
int cov_job(call_guard &g, mloo_job &job, int K, int nd, const std::vector<double> &w, const std::vector<int32_t> &hc, const cov_out &o)
{
    job.want_ll = false; job.want_resid = true; job.want_var = true;
    const int n = job.n, nc = (int)hc.size(), cp = round_up(nc, 16), rs = round_up(n, 16);
    const long long D = job.ndraws;
    const size_t nt = (size_t)(nc + MCOV_T - 1) / MCOV_T, ntp = nt * (nt + 1) / 2, gs = ntp * (size_t)(MCOV_T * MCOV_T);
    if (ntp > 0x7FFFFFFFull) return fail(BNR_ERR_BAD_ARG, "more than 2^31 - 1 tile pairs");
    const size_t draw = (size_t)rs * (size_t)cp;                         // doubles of T' per draw
    const long long SB = std::max<long long>(1, std::min<long long>(D, (long long)(((size_t)1 << 30) / (draw * sizeof(double)))));
    int rc;
    int *colsd = nullptr;
    double *Md = nullptr, *Vd = nullptr, *Dd = nullptr, *Tp = nullptr, *Gw = nullptr, *Gb = nullptr, *Cd = nullptr, *wd = nullptr, *sm = nullptr,
           *outd = nullptr;
    if ((rc = g.upload(&colsd, (const int *)hc.data(), (size_t)nc))) return rc;
    if ((rc = g.upload(&wd, w.data(), (size_t)K))) return rc;
    HIPCHK(hipStreamSynchronize(g.st));
    if ((rc = g.alloc(&Md, (size_t)nc * (size_t)D))) return rc;
    if ((rc = g.alloc(&Vd, (size_t)nc * (size_t)D))) return rc;
    if ((rc = g.alloc(&Dd, (size_t)nc * (size_t)D))) return rc;
    if ((rc = g.alloc(&Tp, (size_t)SB * draw))) return rc;
    if ((rc = g.alloc(&Gw, (size_t)K * gs))) return rc;
    if ((rc = g.alloc(&Gb, (size_t)K * gs))) return rc;
    if ((rc = g.alloc(&Cd, (size_t)D * (size_t)cp))) return rc;
    if ((rc = g.alloc(&sm, (size_t)2 * nc))) return rc;
    if ((rc = g.alloc(&outd, (size_t)2 * (size_t)nc * (size_t)nc))) return rc;
    HIPCHK(hipMemsetAsync(Gw, 0, sizeof(double) * (size_t)K * gs, g.st));
    HIPCHK(hipMemsetAsync(Gb, 0, sizeof(double) * (size_t)K * gs, g.st));
    mloo_hook hook = [&](const mloo_batch &bt) -> int {
        for (long long o0 = 0; o0 < bt.nb; o0 += SB) {
            const int nsb = (int)std::min<long long>(SB, bt.nb - o0);
            hipLaunchKernelGGL(k_mcov_proj, dim3((nc + MEDGE_EB - 1) / MEDGE_EB, (nsb + MEDGE_DB - 1) / MEDGE_DB), dim3(256), 0, g.st, job.X, job.ldx, n,
                               bt.np, job.q, (const int *)colsd, nc, cp, rs, bt.G + (size_t)o0 * bt.mat, (long long)bt.mat, bt.Sp + o0,
                               bt.Wbuf ? bt.Wbuf + (size_t)o0 * (size_t)job.q : nullptr, bt.tau2 + o0, bt.resid, bt.var, bt.bad, bt.s0 + (int)o0, D, nsb, Md,
                               Vd, Dd, Tp);
            const long long s_lo = (long long)bt.s0 + o0, s_hi = s_lo + nsb;
            for (long long s = s_lo; s < s_hi;) {
                const long long k = s / nd, e = std::min<long long>((k + 1) * nd, s_hi);
                hipLaunchKernelGGL(k_mcov_gram, dim3((unsigned)ntp), dim3(256), 0, g.st, (const double *)(Tp + (size_t)(s - s_lo) * draw), (long long)cp,
                                   (e - s) * (long long)rs, cp, Gw + (size_t)k * gs);
                s = e;
            }
            HIPCHK(hipGetLastError());
        }
        return BNR_OK;
    };
    mloo_out out;
    if ((rc = run_job(g, job, out, hook))) return rc;
    const int nbad = count_bad(out.bad);
    // mean and the diagonal's sums: k_medge_summary's mean of (m, tau2 S) and its var_within
    hipLaunchKernelGGL(k_medge_summary, dim3((nc + 3) / 4), dim3(256), 0, g.st, (const double *)Md, (const double *)Dd, D, nc, K, nd, (const double *)wd, 1.0,
                       0.025, 0.975, sm, (double *)nullptr, sm + nc, (double *)nullptr, (double *)nullptr, (double *)nullptr, (double *)nullptr);
    hipLaunchKernelGGL(k_mcov_center, dim3((unsigned)((D + 31) / 32), (cp + 31) / 32), dim3(256), 0, g.st, (const double *)Md, D, D, (const double *)sm, nc, cp, Cd);
    for (int k = 0; k < K; ++k)
        hipLaunchKernelGGL(k_mcov_gram, dim3((unsigned)ntp), dim3(256), 0, g.st, (const double *)(Cd + (size_t)k * (size_t)nd * (size_t)cp), (long long)cp,
                           (long long)nd, cp, Gb + (size_t)k * gs);
    double *wid = outd, *cvd = outd + (size_t)nc * (size_t)nc;
    hipLaunchKernelGGL(k_mcov_finish, dim3((nc + 255) / 256, std::min(nc, 65535)), dim3(256), 0, g.st, (const double *)Gw, (const double *)Gb, (long long)gs, K,
                       nd, (const double *)wd, (const double *)(sm + nc), (const int *)colsd, nc, nbad > 0 ? 1 : 0, wid, cvd);
    HIPCHK(hipGetLastError());
    if ((rc = g.fetch(o.mean, (const double *)sm, (size_t)nc))) return rc;
    if ((rc = g.fetch(o.within, (const double *)wid, (size_t)nc * (size_t)nc))) return rc;
    if ((rc = g.fetch(o.cov, (const double *)cvd, (size_t)nc * (size_t)nc))) return rc;
    if (o.m && (rc = fetch_transposed(g, Md, nc, (int)D, o.m))) return rc;
    if (o.v && (rc = fetch_transposed(g, Vd, nc, (int)D, o.v))) return rc;
    HIPCHK(hipStreamSynchronize(g.st));
    HIPCHK(hipGetLastError());
    if (o.n_bad) *o.n_bad = nbad;
    return BNR_OK;
}
}   // namespace

int bnr_mcov_abi_version(void) { return BNR_MCOV_ABI_VERSION; }

int bnr_mcov_set_option(const char *name, int64_t value) { return set_batch_draws("mcov", name, value); }

int bnr_marginal_gamma_cov(int32_t device, int32_t n, int32_t q, int32_t K, int32_t nd, const double *X, const double *y, const double *tau2,
                           const double *mu, const double *S, const double *W, const double *weights, int32_t ncols, const int32_t *cols,
                           double *mean, double *cov, double *within, double *m, double *v, int32_t *n_bad)
{
    if (!X || !y || !tau2 || !mu || !S) return fail(BNR_ERR_BAD_ARG, "NULL argument");
    if (!mean && !cov && !within) return fail(BNR_ERR_BAD_ARG, "ask for mean, cov or within");
    if (K < 1 || nd < 1) return fail(BNR_ERR_BAD_ARG, "need K >= 1 chains and nd >= 1 draws per chain");
    if ((long long)K * nd > 0x7FFFFFFFll) return fail(BNR_ERR_BAD_ARG, "more than 2^31 - 1 pooled draws");
    if (n < 1 || q < 1) return fail(BNR_ERR_BAD_ARG, "need n >= 1 rows, q >= 1 edges and ndraws >= 1 draws");
    int rc;
    std::vector<double> w;
    if ((rc = summary_weights(weights, K, w))) return rc;
    std::vector<int32_t> hc;
    if ((rc = cov_cols(ncols, cols, q, hc))) return rc;
    call_guard g;
    mloo_job job;
    if ((rc = open_raw_job(g, job, device, n, q, K * nd, X, y, tau2, mu, S, W))) return rc;
    return cov_job(g, job, K, nd, w, hc, cov_out{mean, cov, within, m, v, n_bad});
}

int bnr_chains_marginal_edge_cov(bnr_chain *const *chains, int32_t nchains, const double *weights, int32_t first_row, int32_t nsamp, int32_t thin,
                                 int32_t ncols, const int32_t *cols, double *mean, double *cov, double *within, double *m, double *v,
                                 int32_t *n_bad)
{
    if (!chains) return fail(BNR_ERR_BAD_ARG, "NULL argument");
    if (!mean && !cov && !within) return fail(BNR_ERR_BAD_ARG, "ask for mean, cov or within");
    int rc, nd;
    if ((rc = check_chain_list(chains, nchains, thin))) return rc;
    std::vector<double> w;
    if ((rc = summary_weights(weights, nchains, w))) return rc;
    bnr_chain_view v0;
    if ((rc = bnr_chain_device_view(chains[0], &v0))) return rc;
    std::vector<int32_t> hc;
    if ((rc = cov_cols(ncols, cols, v0.q, hc))) return rc;
    call_guard g;
    mloo_job job;
    if ((rc = open_chain_job(g, job, chains, nchains, first_row, nsamp, thin, nd))) return rc;
    return cov_job(g, job, nchains, nd, w, hc, cov_out{mean, cov, within, m, v, n_bad});
}
