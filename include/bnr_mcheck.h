/*
 * bnr_mcheck.h -- C ABI of libbnr_mcheck.so: the leave-one-out predictive checks of the training rows under the MARGINAL PSIS weights of
 * libbnr_mloo.so (include/bnr_mloo.h), for the Bayesian network regression of libbnr_hip.so (include/bnr_hip.h).  An ADDITION to the reference.
 * A fifth library beside libbnr_hip.so, libbnr_mloo.so, libbnr_medge.so and libbnr_mpred.so, with a gfx950 code object of its own that holds the
 * four kernels of libbnr_mloo.so and three more (csrc/bnr_mcheck_kernels.h); linked against libbnr_hip.so, it reads the chains through
 * bnr_chain_device_view and runs PSIS through bnr_psis_weights.  It exports the bnr_* functions below and nothing else.
 *
 * With the edge coefficients integrated out, row i of draw s has resid_is = y_i - E[y_i | y_-i, phi_s] and var_is = Var[y_i | y_-i, phi_s]
 * (bnr_mloo.h), and the leave-one-out predictive distribution of y_i is the mixture of normals
 *     sum_s w_is N(m_is, var_is),   m_is = y_i - resid_is,   w_is = exp(lw_is),   sd_is = sqrt(var_is)
 * under the normalised PSIS weights of the ratios 1 / p(y_i | y_-i, phi_s).  Per row:
 *     mean  = y_i - sum_s w_is resid_is                         (without y, raw form only: sum_s w_is m_is)
 *     sd    = sqrt(max(sum_s w_is (var_is + m_is^2) - mean^2, 0))
 *     pit   = sum_s w_is Phi(resid_is / sd_is),                 Phi(z) = erfc(-z / sqrt 2) / 2
 *     lower, upper = the p_lo- and p_hi-quantile of F_i(t) = sum_s w_is Phi((t - m_is) / sd_is)
 * In the raw form m is given and resid_is stands for y_i - m_is; in the chain form m_is = y_i - resid_is is rounded once and resid_is is taken
 * back from it in the same way, so that the two forms agree bit for bit on the same m.  Every division by sd_is is a product with 1 / sd_is,
 * rounded once per element and call; pit is F_i(y_i) bit for bit.
 * The quantile search is bnr_chains_loo_predict's bisection: the bracket [min_s(m_is - c sd_is), max_s(m_is + c sd_is)] with c the first of
 * 1, 1.5, 2, ... such that Phi(-c) < min(p_lo, 1 - p_hi) / 2; F(mid) < p moves the lower end, anything else the upper one; halved until the
 * bracket is no wider than 2^-40 of the first one, at most 64 times; the midpoint.
 * var_is = 0 is the point mass at m_is: Phi becomes [t >= m_is].
 * A row is NaN in all five outputs if it holds a NaN or negative var, a NaN mean or a log weight that is not finite; a NaN y makes mean, sd and
 * pit NaN (they are formed through y) and leaves the bounds.
 *
 * Summation order.  Every sum over the draws of a row is formed like this: partial sum t (t = 0 .. 255) adds the terms of draws t, t + 256,
 * t + 512, ... in that order from 0.0; the 256 partial sums are then added as a tree, partial t taking partial t + 128, then t + 64, 32, 16, 8,
 * 4, 2 and 1.  The order is fixed by D alone.  No output of a row depends on the other rows, on the grid, on the batch ("mcheck_batch_draws"), on
 * which outputs were asked for or on the call, bit for bit.
 *
 * Conventions: those of bnr_mloo.h.  Every pointer is a host pointer; a status other than BNR_OK leaves its message in bnr_last_error().
 * DESIGN.md section 8.
 */
#ifndef BNR_MCHECK_H
#define BNR_MCHECK_H

#include "bnr_mloo.h"

#ifdef __cplusplus
extern "C" {
#endif

#define BNR_MCHECK_ABI_VERSION 1

int bnr_mcheck_abi_version(void);

/* The kernels alone, on a caller's matrices: mean, var, logw rows x ndraws with a row's draws contiguous, logw the normalised log weights
 * (bnr_psis_weights' log_weights, or any other); y[rows] nullable (then no pit: asking for one is refused).  out_mean, out_sd, out_pit, out_lower,
 * out_upper: rows doubles each, every one nullable but not all of them.  Checks: rows, ndraws >= 1; rows ndraws < 2^31; 0 < p_lo < p_hi < 1
 * (read only where a bound is asked for); the device. */
int bnr_weighted_mixture(int32_t device, int32_t rows, int32_t ndraws, const double *mean, const double *var, const double *logw, const double *y,
                         double p_lo, double p_hi, double *out_mean, double *out_sd, double *out_pit, double *out_lower, double *out_upper);

/* The chain form: the draws, the checks and the refusals of bnr_chains_marginal_loo (same order, same messages; a bad p_lo / p_hi is refused
 * behind thin).  loglik, resid and var of every draw stay on the device; loglik goes to the host and through bnr_psis_weights as in that call, so
 * elpd_loo[n] and pareto_k[n] are that call's on the same chains, bit for bit; the normalised log weights go back to the device and the kernels
 * run on the resident resid, var and y.  loo_mean, loo_sd, loo_pit, loo_lower, loo_upper: n doubles each, every one nullable (with none of them
 * the call is bnr_chains_marginal_loo without its moments); only those n-vectors come back from the kernels.  logml[D], loglik (n x D) and n_bad
 * are nullable.  A bad draw is NaN in every row, so every row is NaN in the five outputs while n_bad > 0; pareto_k keeps bnr_psis_weights'
 * convention.  Nothing of any chain is written: tables, iteration counters, RNG and event counters stay as they were; a pending
 * bnr_chain_run_async is waited for. */
int bnr_chains_marginal_loo_predict(bnr_chain *const *chains, int32_t nchains, int32_t first_row, int32_t nsamp, int32_t thin, const double *r_eff,
                                    double p_lo, double p_hi, double *elpd_loo, double *pareto_k, double *loo_mean, double *loo_sd, double *loo_pit,
                                    double *loo_lower, double *loo_upper, double *logml, double *loglik, int32_t *n_bad);

/* "mcheck_batch_draws": draws per device batch of the factorizations (0 = automatic: the batch's matrices stay within about 1 GiB).
 * Performance only. */
int bnr_mcheck_set_option(const char *name, int64_t value);

#ifdef __cplusplus
}
#endif
#endif /* BNR_MCHECK_H */
