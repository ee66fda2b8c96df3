// bnr_mstack.hip -- libbnr_mstack.so behind include/bnr_mstack.h: chain stacking on the marginal PSIS-LOO of every chain from one pass over the
// pooled draws, and the leave-one-out predictive checks of the stacked mixture, on the device.  A library and a gfx950 code object of its own: the
// four kernels of bnr_mloo_kernels.h (by #include, through bnr_mloo_job.h, the driver shared with the other marginal libraries: open_chain_job,
// run_job without a hook, and mloo_out, which leaves loglik, resid and var on the device), the kernels of bnr_mcheck_kernels.h (by #include;
// k_mcheck_moments and k_mcheck_quantile are launched through bnr_mcheck_rows.h, the host code shared with libbnr_mcheck.so; k_mcheck_stage is
// only carried along) and k_mstack_stage of bnr_mstack_kernels.h.  It reaches a chain through bnr_chain_device_view, runs PSIS through
// bnr_psis_weights and the solver through bnr_stacking_weights, and leaves its messages with bnr_set_last_error -- exported calls of
// libbnr_hip.so, nothing of bnr_internal.h.  Linked with bnr_mstack.map: only the functions of the header are exported.
#include "../../include/bnr_mstack.h"
#include "bnr_mcheck_kernels.h"
#include "bnr_mstack_kernels.h"
#include "bnr_mloo_job.h"
#include "bnr_mcheck_rows.h"

#include <cstring>

namespace {
// log sum_{k: w_k > 0} w_k exp(v_k) with the largest such v_k taken out, k ascending (v: stride ldv) -- bnr_chains_stack's
double wlse(const double *v, size_t ldv, const double *w, int K)
{
    double M = -INFINITY;
    for (int k = 0; k < K; ++k) if (w[k] > 0.0) M = std::max(M, v[k * ldv]);
    double s = 0.0;
    for (int k = 0; k < K; ++k) if (w[k] > 0.0) s += w[k] * exp(v[k * ldv] - M);
    return M + log(s);
}

// The stacked mixture of the device matrices A, V, LW (rows x K nd, a row's components contiguous, chain k's in columns k nd ..) under the host
// weights w[K] (checked), yd (rows, NULL: none), and the outputs asked for to the host: k_mstack_stage into the compacted rows x D+ matrices, then
// the two row kernels of bnr_mcheck_kernels.h in the launch loop of bnr_mcheck_rows.h.  a_is_resid: A holds resid = y - m (the chain form; it
// needs yd), else m itself.
int stack_run(call_guard &g, int rows, int K, int nd, const double *w, const double *A, bool a_is_resid, const double *V, const double *LW,
              const double *yd, double c, double p_lo, double p_hi, const mix_out &o)
{
    int rc;
    std::vector<int> csel;
    std::vector<double> wsel;
    for (int k = 0; k < K; ++k)
        if (w[k] > 0.0) { csel.push_back(k); wsel.push_back(w[k]); }
    const int Kp = (int)csel.size(), D = K * nd, Dp = Kp * nd;
    const size_t total = (size_t)rows * (size_t)Dp;
    int *cd = nullptr;
    double *wd = nullptr, *Wt = nullptr, *Isd = nullptr, *Mo = nullptr, *Vo = nullptr;
    if ((rc = g.upload(&cd, (const int *)csel.data(), (size_t)Kp))) return rc;
    if ((rc = g.upload(&wd, (const double *)wsel.data(), (size_t)Kp))) return rc;
    HIPCHK(hipStreamSynchronize(g.st));
    if ((rc = g.alloc(&Wt, total))) return rc;
    if ((rc = g.alloc(&Isd, total))) return rc;
    if ((rc = g.alloc(&Mo, total))) return rc;
    if (Kp < K && (rc = g.alloc(&Vo, total))) return rc;
    const unsigned strips = (unsigned)((Dp + MSTACK_STRIP - 1) / MSTACK_STRIP);
    const unsigned gy = (unsigned)std::min<long long>(rows, std::max<long long>(1, std::min<long long>(65535, ((long long)1 << 16) / strips)));
    return mix_rows(g, rows, Dp, Mo, Vo ? Vo : V, Wt, Isd, yd, c, p_lo, p_hi, o, [&] {
        hipLaunchKernelGGL(k_mstack_stage, dim3(strips, gy), dim3(256), 0, g.st, LW, V, A, a_is_resid ? yd : nullptr, rows, D, Dp, nd, (const int *)cd,
                           (const double *)wd, Wt, Isd, Mo, Vo);
    });
}
}   // namespace

int bnr_mstack_abi_version(void) { return BNR_MSTACK_ABI_VERSION; }

int bnr_mstack_set_option(const char *name, int64_t value) { return set_batch_draws("mstack", name, value); }

int bnr_stacked_mixture(int32_t device, int32_t rows, int32_t K, int32_t nd, const double *mean, const double *var, const double *logw,
                        const double *weights, const double *y, double p_lo, double p_hi, double *out_mean, double *out_sd, double *out_pit,
                        double *out_lower, double *out_upper)
{
    if (!mean || !var || !logw || !weights) return fail(BNR_ERR_BAD_ARG, "NULL argument");
    const mix_out o{out_mean, out_sd, out_pit, out_lower, out_upper};
    if (!out_mean && !out_sd && !out_pit && !out_lower && !out_upper) return fail(BNR_ERR_BAD_ARG, "ask for at least one output");
    if (K < 1 || K > BNR_STACK_MAX_CHAINS) return fail(BNR_ERR_BAD_ARG, "need 1 <= nchains <= 32");
    if (rows < 1 || nd < 1) return fail(BNR_ERR_BAD_ARG, "need rows >= 1 and ndraws >= 1");
    if ((long long)rows * K * nd > 0x7FFFFFFFll) return fail(BNR_ERR_BAD_ARG, "rows x ndraws must stay below 2^31");
    double c;
    if (const char *msg = mix_check(o, y != nullptr, p_lo, p_hi, c)) return fail(BNR_ERR_BAD_ARG, msg);
    if (const char *msg = weight_check(weights, K)) return fail(BNR_ERR_BAD_ARG, msg);
    call_guard g;
    int rc;
    if ((rc = g.open(device))) return rc;
    const size_t total = (size_t)rows * (size_t)K * (size_t)nd;
    double *Md = nullptr, *Vd = nullptr, *Ld = nullptr, *yd = nullptr;
    if ((rc = g.upload(&Md, mean, total))) return rc;
    if ((rc = g.upload(&Vd, var, total))) return rc;
    if ((rc = g.upload(&Ld, logw, total))) return rc;
    if (y && (rc = g.upload(&yd, y, (size_t)rows))) return rc;
    return stack_run(g, rows, K, nd, weights, Md, false, Vd, Ld, yd, c, p_lo, p_hi, o);
}

int bnr_chains_marginal_stack(bnr_chain *const *chains, int32_t nchains, int32_t first_row, int32_t nsamp, int32_t thin, const double *r_eff,
                              const double *fixed_weights, int32_t max_iter, double gap_tol, double p_lo, double p_hi, double *weights,
                              double *elpd_chain, double *pareto_k_chain, double *elpd_stack, double *gap, int32_t *iters, double *loo_mean,
                              double *loo_sd, double *loo_pit, double *loo_lower, double *loo_upper, double *logml, int32_t *n_bad)
{
    if (!chains || !weights || !elpd_chain || !pareto_k_chain) return fail(BNR_ERR_BAD_ARG, "NULL argument");
    const mix_out o{loo_mean, loo_sd, loo_pit, loo_lower, loo_upper};
    const bool checks = loo_mean || loo_sd || loo_pit || loo_lower || loo_upper;
    call_guard g;
    mloo_job job;
    int rc, nd;
    if ((rc = check_chain_list(chains, nchains, thin))) return rc;
    if ((rc = open_chain_job(g, job, chains, nchains, first_row, nsamp, thin, nd))) return rc;
    if (nchains > BNR_STACK_MAX_CHAINS) return fail(BNR_ERR_BAD_ARG, "need 1 <= nchains <= 32");
    if (max_iter < 1) return fail(BNR_ERR_BAD_ARG, "need max_iter >= 1");
    if (!std::isfinite(gap_tol) || !(gap_tol > 0.0)) return fail(BNR_ERR_BAD_ARG, "gap_tol must be positive and finite");
    const int K = nchains;
    if (fixed_weights)
        if (const char *msg = weight_check(fixed_weights, K)) return fail(BNR_ERR_BAD_ARG, msg);
    double c;
    if (const char *msg = mix_check(o, true, p_lo, p_hi, c)) return fail(BNR_ERR_BAD_ARG, msg);
    job.want_ll = true; job.want_resid = checks; job.want_var = checks;
    mloo_out out;
    if ((rc = run_job(g, job, out))) return rc;
    const int n = job.n, D = job.ndraws;
    const size_t nout = (size_t)n * (size_t)D, nk = (size_t)n * (size_t)nd;
    // every chain's own PSIS on its n x nd slice of the pooled loglik; the normalised log weights back into the pooled layout
    std::vector<double> ll(nout), lw(checks ? nout : 0), llk(nk), lwk(nk);
    if ((rc = g.fetch(ll.data(), out.loglik, nout))) return rc;
    for (int k = 0; k < K; ++k) {
        for (int i = 0; i < n; ++i) memcpy(llk.data() + (size_t)i * nd, ll.data() + (size_t)i * D + (size_t)k * nd, sizeof(double) * (size_t)nd);
        if ((rc = bnr_psis_weights(job.v.device, n, nd, llk.data(), r_eff, lwk.data(), elpd_chain + (size_t)k * n, pareto_k_chain + (size_t)k * n)))
            return rc;
        if (checks)
            for (int i = 0; i < n; ++i) memcpy(lw.data() + (size_t)i * D + (size_t)k * nd, lwk.data() + (size_t)i * nd, sizeof(double) * (size_t)nd);
    }
    // the weights: given, or the solver's on the rows that are finite in every chain (bnr_chains_stack)
    std::vector<double> lp;
    std::vector<char> used(n, 1);
    for (int i = 0; i < n; ++i) {
        for (int k = 0; k < K; ++k) if (!std::isfinite(elpd_chain[(size_t)k * n + i])) used[i] = 0;
        if (used[i]) for (int k = 0; k < K; ++k) lp.push_back(elpd_chain[(size_t)k * n + i]);
    }
    const int nu = (int)(lp.size() / K);
    double gp = NAN;
    int32_t it = 0;
    if (fixed_weights) memcpy(weights, fixed_weights, sizeof(double) * (size_t)K);
    else if (nu < 1) for (int k = 0; k < K; ++k) weights[k] = 1.0 / K;
    else if ((rc = bnr_stacking_weights(nu, K, lp.data(), max_iter, gap_tol, weights, nullptr, &gp, &it))) return rc;
    if (elpd_stack) for (int i = 0; i < n; ++i) elpd_stack[i] = used[i] ? wlse(elpd_chain + i, (size_t)n, weights, K) : NAN;
    if (gap) *gap = gp;
    if (iters) *iters = it;
    if (checks) {
        HIPCHK(hipSetDevice(job.v.device));
        double *Ld = nullptr;
        if ((rc = g.upload(&Ld, (const double *)lw.data(), nout))) return rc;
        if ((rc = stack_run(g, n, K, nd, weights, out.resid, true, out.var, Ld, job.v.y, c, p_lo, p_hi, o))) return rc;
    }
    if ((rc = g.fetch(logml, out.logml, (size_t)D))) return rc;
    if (n_bad) *n_bad = count_bad(out.bad);
    return BNR_OK;
}
