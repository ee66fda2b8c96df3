/*
 * bnr_medge.h -- C ABI of libbnr_medge.so: Rao-Blackwellised summaries of the edge coefficients of the Bayesian network regression of
 * libbnr_hip.so (include/bnr_hip.h), gamma integrated out on the device.  An ADDITION to the reference.  A third library beside libbnr_hip.so and
 * libbnr_mloo.so (include/bnr_mloo.h), with a gfx950 code object of its own that holds the four kernels of marginal PSIS-LOO and two more; linked
 * against libbnr_hip.so, it reads the chains through bnr_chain_device_view.  It exports the bnr_* functions below and nothing else.
 *
 * Given phi = (tau2, mu, u, lambda, S) of a table row the edge coefficients are Gaussian in closed form (the distribution update_gamma! draws
 * from, gibbs.jl:420-436).  With D = diag S, A = I_n + X D X^T = L L^T, r = y - mu - X W, g = A^-1 r and x_e = column e of X:
 *     gamma | phi, y ~ N(m, tau2 (D - D X^T A^-1 X D))
 *     m_e = W_e + S_e p_e,                     p_e = sum_i x_ie g_i
 *     v_e = (tau2 S_e) max(1 - S_e t_e, 0),    t_e = x_e^T A^-1 x_e = ||L^-1 x_e||^2
 * so the posterior of gamma_e is the mixture sum_s omega_s N(m_se, v_se) over the draws s of phi: its moments, its CDF and its sign
 * probabilities carry none of the within-draw noise of gamma (law of total expectation / variance).
 *
 * Conventions: those of bnr_mloo.h.  Every pointer is a host pointer; a status other than BNR_OK leaves its message in bnr_last_error().
 * Limits (BNR_ERR_BAD_ARG beyond): n <= BNR_MLOO_MAX_N.
 * A draw whose S, tau2 or mu is not finite, or whose factorization meets a pivot that is not > 0, is flagged by the factor kernel: its m and v
 * are NaN and it is counted in n_bad (bnr_mloo.h's convention); it is no error, and no other draw changes a bit -- but every summary of a
 * call whose n_bad > 0 is NaN, because an edge with a NaN m or v in any draw is NaN in every summary.
 * No m or v of a draw depends on the batch ("medge_batch_draws"), on the other draws or edges of the call, on thin or on the call, bit for bit:
 * the order of every sum is fixed by (n, q) alone (csrc/bnr_medge_kernels.h).  DESIGN.md section 8.
 */
#ifndef BNR_MEDGE_H
#define BNR_MEDGE_H

#include "bnr_mloo.h"

#ifdef __cplusplus
extern "C" {
#endif

#define BNR_MEDGE_ABI_VERSION 1

int bnr_medge_abi_version(void);

/* The linear algebra alone, on a caller's matrices: the inputs of bnr_marginal_loglik (X n x q column-major, y[n], tau2[ndraws], mu[ndraws], S
 * and W ndraws x q with a draw's q values contiguous, W NULL: 0).  m, v: ndraws x q with a draw's q values contiguous, each nullable but not
 * both; n_bad nullable.  Checks: those of bnr_marginal_loglik. */
int bnr_marginal_gamma(int32_t device, int32_t n, int32_t q, int32_t ndraws, const double *X, const double *y, const double *tau2, const double *mu,
                       const double *S, const double *W, double *m, double *v, int32_t *n_bad);

/* The summary of q mixtures of normals on a caller's (K nd) x q matrices m, v (a draw's q values contiguous, chain k's draws in rows k nd ..):
 * omega_s = w_k / nd.  weights[K]: nullable (1 / K each); checked as bnr_chains_wsummary checks them (1 <= K <= 32, finite, >= 0, one > 0,
 * |sum - 1| <= 1e-9) and used as given.  Every output holds q doubles and is nullable, but not all of them; lower and upper come together and
 * need 0 < p_lo < p_hi < 1.
 * A chain sum: the terms of the chain's draws j = l, l + 64, l + 128, ... are added in that order from 0.0 into partial sum l (l = 0 .. 63), then
 * the partial sums pairwise: l with l + 32 (l < 32), then with l + 16, 8, 4, 2, 1 -- an order fixed by nd alone.  A statistic: the chain sums
 * divided by nd, multiplied by w_k and added with k ascending from 0.0.  Every product and sum is rounded on its own.
 *     mean       = sum omega m
 *     sd         = sqrt(max(sum omega (v + m m) - mean mean, 0))
 *     var_within = sum omega v: the part of the variance that Rao-Blackwellisation removes from the estimator
 *     p_pos      = sum omega erfc((m / sqrt v) (-1 / sqrt 2)) / 2
 *     p_neg      = sum omega erfc((m / sqrt v) (+1 / sqrt 2)) / 2, summed on its own: a tail of 1e-200 keeps its relative precision
 *     lower, upper: the p_lo- and p_hi-quantile of F(t) = sum omega Phi((t - m) / sqrt v), Phi(z) = erfc(z (-1 / sqrt 2)) / 2, found as
 *                   bnr_chains_loo_predict finds its mixture quantiles: bisection from [min (m - c sqrt v), max (m + c sqrt v)] over all draws,
 *                   c the first of 1, 1.5, 2, ... with Phi(-c) < min(p_lo, 1 - p_hi) / 2; F(mid) < p moves the lower end, anything else the
 *                   upper one; down to 2^-40 of the bracket (at most 64 halvings); the midpoint.
 * A component with v = 0 is the point mass at m: Phi -> [t >= m], p_pos -> [m > 0], p_neg -> [m < 0].  An edge with a NaN m or v in any draw is
 * NaN in every output. */
int bnr_mixture_summary(int32_t device, int32_t q, int32_t K, int32_t nd, const double *m, const double *v, const double *weights, double p_lo,
                        double p_hi, double *mean, double *sd, double *var_within, double *p_pos, double *p_neg, double *lower, double *upper);

/* The chain form: the draws of bnr_chains_marginal_loo -- rows first_row + j thin (1-based), j = 0 .. nd - 1, nd = ceil(nsamp / thin), of every
 * chain listed, chain k's first in order k, D = nchains nd, W formed on the device from u and lambda of the same row -- with the checks of that
 * call and, for weights (nullable), those of bnr_mixture_summary.  m and v stay on the device (edge-major); the summaries are
 * bnr_mixture_summary's on those matrices with K = nchains, bit for bit.  m, v (D x q, a draw's q values contiguous; nullable) reach the host only
 * if asked for.  The summary outputs as in bnr_mixture_summary (not all NULL); n_bad nullable: while n_bad > 0 every summary is NaN.
 * Nothing of any chain is written: tables, iteration counters, RNG and event counters stay as they were; a pending bnr_chain_run_async is
 * waited for. */
int bnr_chains_marginal_edges(bnr_chain *const *chains, int32_t nchains, const double *weights, int32_t first_row, int32_t nsamp, int32_t thin,
                              double p_lo, double p_hi, double *mean, double *sd, double *var_within, double *p_pos, double *p_neg, double *lower,
                              double *upper, double *m, double *v, int32_t *n_bad);

/* "medge_batch_draws": draws per device batch (0 = automatic: the batch's matrices stay within about 1 GiB).  Performance only. */
int bnr_medge_set_option(const char *name, int64_t value);

#ifdef __cplusplus
}
#endif
#endif /* BNR_MEDGE_H */
