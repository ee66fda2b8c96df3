/*
 * bnr_mpred.h -- C ABI of libbnr_mpred.so: Rao-Blackwellised prediction of new rows for the Bayesian network regression of libbnr_hip.so
 * (include/bnr_hip.h), gamma integrated out on the device.  An ADDITION to the reference.  A fourth library beside libbnr_hip.so, libbnr_mloo.so
 * (include/bnr_mloo.h) and libbnr_medge.so (include/bnr_medge.h), with a gfx950 code object of its own that holds the six kernels of that library
 * and four more; linked against libbnr_hip.so, it reads the chains through bnr_chain_device_view.  It exports the bnr_* functions below and
 * nothing else.
 *
 * Given phi = (tau2, mu, u, lambda, S) of a table row, with D = diag S, A = I_n + X D X^T = L L^T, M = L^-1, r = y - mu - X W, g = A^-1 r and
 * new rows X* (m x q), row j = x*_j:
 *     C   = X D X*^T                       (n x m, the cross Gram of the draw)
 *     a_j = sum_e x*_je W_e,   d_j = sum_e (x*_je S_e) x*_je,   h_j = sum_i C_ij g_i,   t_j = ||M C_j||^2
 *     eta*_j | phi, y ~ N(mean_j, var_j),  mean_j = (mu + a_j) + h_j,   var_j = tau2 max(d_j - t_j, 0)
 *     y*_j   | phi, y ~ N(mean_j, var_j + tau2)
 * so the posterior of the mean response of row j is the mixture sum_s omega_s N(mean_sj, var_sj) over the draws s of phi and the predictive
 * distribution of a new observation the same mixture with var + tau2: neither carries the within-draw noise of gamma, and no predictive noise has
 * to be drawn (there is no seed).
 *
 * Conventions: those of bnr_medge.h.  Every pointer is a host pointer; a status other than BNR_OK leaves its message in bnr_last_error().
 * Limits (BNR_ERR_BAD_ARG beyond): n <= BNR_MLOO_MAX_N, m >= 1.  X is n x q and X* is m x q, both column-major without padding.
 * A draw whose S, tau2 or mu is not finite, or whose factorization meets a pivot that is not > 0, is flagged by the factor kernel: its mean and
 * var are NaN and it is counted in n_bad; it is no error, and no other draw changes a bit -- but every summary and score of a call whose
 * n_bad > 0 is NaN, because a new row with a NaN in any draw is NaN in every summary.
 * No mean or var of a draw depends on the batch ("mpred_batch_draws"), on the block of new rows ("mpred_block_rows"), on the other draws or new
 * rows of the call, on thin or on the call, bit for bit: the order of every sum is fixed by (n, q) alone (csrc/bnr_mpred_kernels.h).
 * DESIGN.md section 8.
 */
#ifndef BNR_MPRED_H
#define BNR_MPRED_H

#include "bnr_medge.h"

#ifdef __cplusplus
extern "C" {
#endif

#define BNR_MPRED_ABI_VERSION 1

int bnr_mpred_abi_version(void);

/* The linear algebra alone, on a caller's matrices: the inputs of bnr_marginal_gamma plus Xnew (m x q column-major).  mean, var: ndraws x m with
 * a draw's m values contiguous, each nullable but not both; n_bad nullable.  Checks: those of bnr_marginal_gamma, and m >= 1. */
int bnr_marginal_predict(int32_t device, int32_t n, int32_t q, int32_t m, int32_t ndraws, const double *X, const double *y, const double *Xnew,
                         const double *tau2, const double *mu, const double *S, const double *W, double *mean, double *var, int32_t *n_bad);

/* The score of m observed responses y[m] under m mixtures of normals, on a caller's (K nd) x m matrices mean, vobs (a draw's m values
 * contiguous, chain k's draws in rows k nd ..): omega_s = w_k / nd.  weights[K]: as in bnr_mixture_summary.  lpd, pit: m doubles each, nullable
 * but not both.  Chain sums and statistics in bnr_mixture_summary's order.
 *     l_s = -(log 2 pi + log vobs) / 2 - (((y - mean) (y - mean)) / vobs) / 2
 *     lpd = mx + log sum_k (chain sum of exp(l_s - mx) / nd) w_k,  mx = max l_s, both over the chains with w_k > 0 only
 *     pit = sum_k (chain sum of Phi((y - mean) / sqrt vobs) / nd) w_k,  Phi(z) = erfc(z (-1 / sqrt 2)) / 2, over all chains
 * A component with vobs = 0 is the point mass at mean: Phi -> [y >= mean]; it adds nothing to lpd unless y == mean, where lpd = +inf; a row
 * whose weighted components are all point masses elsewhere has lpd = -inf.  A row with a NaN y, a NaN mean or vobs in any draw (of any chain,
 * whatever its weight) or a vobs < 0 is NaN in lpd and pit. */
int bnr_mixture_score(int32_t device, int32_t m, int32_t K, int32_t nd, const double *mean, const double *vobs, const double *y,
                      const double *weights, double *lpd, double *pit);

/* The chain form: the draws and checks of bnr_chains_marginal_edges; Xnew m x q column-major (q the chains' V (V + 1) / 2 edges), ynew[m]
 * nullable.  The per-draw mean, var and var + tau2 stay on the device (row-major per new row); outputs, m doubles each, every one nullable but
 * not all of them:
 *     mean, sd, var_within, lower, upper   bnr_mixture_summary of (mean, var): the posterior of the mean response eta*_j
 *     pred_sd, pred_lower, pred_upper      the sd, lower and upper of bnr_mixture_summary of (mean, var + tau2): a new observation y*_j
 *     lpd, pit                             bnr_mixture_score of (mean, var + tau2) at ynew; they need ynew
 *     dmean, dvar                          the per-draw matrices (D x m, a draw's m values contiguous), only if asked for
 * lower and upper come together, pred_lower and pred_upper too; both pairs need 0 < p_lo < p_hi < 1.  The summaries are bnr_mixture_summary's
 * and bnr_mixture_score's on those matrices with K = nchains, bit for bit.  n_bad nullable.  Nothing of any chain is written: tables, iteration
 * counters, RNG and event counters stay as they were; a pending bnr_chain_run_async is waited for. */
int bnr_chains_marginal_predict(bnr_chain *const *chains, int32_t nchains, const double *weights, int32_t first_row, int32_t nsamp, int32_t thin,
                                const double *Xnew, int32_t m, const double *ynew, double p_lo, double p_hi, double *mean, double *sd,
                                double *var_within, double *lower, double *upper, double *pred_sd, double *pred_lower, double *pred_upper,
                                double *lpd, double *pit, double *dmean, double *dvar, int32_t *n_bad);

/* "mpred_batch_draws": draws per device batch (0 = automatic: the batch's factors stay within about 1 GiB).  "mpred_block_rows": new rows per
 * block of the cross Gram (0 = automatic: the batch's blocks of C stay within about 1 GiB).  Performance only. */
int bnr_mpred_set_option(const char *name, int64_t value);

#ifdef __cplusplus
}
#endif
#endif /* BNR_MPRED_H */
