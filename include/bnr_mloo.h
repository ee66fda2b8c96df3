/*
 * bnr_mloo.h -- C ABI of libbnr_mloo.so: marginal PSIS-LOO for the Bayesian network regression of libbnr_hip.so (include/bnr_hip.h), the
 * edge coefficients integrated out on the device (integrated importance sampling: Vehtari, Mononen, Tolvanen, Sivula & Winther 2016, JMLR 17).
 * An ADDITION to the reference.  A library of its own beside libbnr_hip.so -- its kernels are one gfx950 code object, the two of libbnr_hip.so
 * stay what they are -- linked against it: it reads the chains through bnr_chain_device_view and runs PSIS through bnr_psis_weights.
 *
 * Given phi = (tau2, mu, u, lambda, S) the edge coefficients are Gaussian, gamma ~ N(W, tau2 diag S), W_e = sum_t lambda_t u_{t,k(e)} u_{t,l(e)},
 * and integrate out in closed form:  y | phi ~ N(mu 1 + X W, tau2 A),  A = I_n + X diag(S) X^T  (the matrix update_gamma! factorises,
 * gibbs.jl:434).  With A = L L^T, r = y - mu - X W, g = A^-1 r, c_i = (A^-1)_ii:
 *     resid_i  = y_i - E[y_i | y_-i, phi] = g_i / c_i
 *     var_i    = Var[y_i | y_-i, phi]     = tau2 / c_i
 *     loglik_i = log p(y_i | y_-i, phi)   = -(log 2 pi + log var_i) / 2 - (resid_i^2 / var_i) / 2
 *     logml    = log p(y | phi)           = -(n / 2) log(2 pi tau2) - sum_j log L_jj - (||L^-1 r||^2 / tau2) / 2
 * and p(phi | y_-i) is proportional to p(phi | y) / p(y_i | y_-i, phi): the n x S matrix loglik goes through PSIS as the conditional one does.
 *
 * Conventions: those of bnr_hip.h.  Every pointer is a host pointer; a status other than BNR_OK leaves its message in bnr_last_error().
 * Limits (BNR_ERR_BAD_ARG beyond): n <= 2048 in this version.
 * A draw whose S, tau2 or mu is not finite, or whose factorization meets a pivot that is not > 0, is NaN in all of its outputs and is counted
 * in n_bad; it is no error, and no other draw changes a bit.  No output of a draw depends on the batch ("mloo_batch_draws"), on the other
 * draws of the call, on thin or on the call, bit for bit.  DESIGN.md section 8.
 */
#ifndef BNR_MLOO_H
#define BNR_MLOO_H

#include "bnr_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define BNR_MLOO_ABI_VERSION 1
#define BNR_MLOO_MAX_N 2048

int bnr_mloo_abi_version(void);

/* The linear algebra alone, on a caller's matrices: X n x q column-major, y[n], tau2[ndraws], mu[ndraws], S and W ndraws x q with a draw's q
 * values contiguous (W NULL: 0).  loglik, resid, var: n x ndraws with a row's draws contiguous, each nullable but not all three; logml[ndraws]
 * and n_bad nullable.  Checks: n, q, ndraws >= 1, n <= BNR_MLOO_MAX_N, the device. */
int bnr_marginal_loglik(int32_t device, int32_t n, int32_t q, int32_t ndraws, const double *X, const double *y, const double *tau2,
                        const double *mu, const double *S, const double *W, double *loglik, double *resid, double *var, double *logml,
                        int32_t *n_bad);

/* Marginal PSIS-LOO of the training rows over rows first_row + j thin (1-based), j = 0 .. ceil(nsamp / thin) - 1, of every chain listed: D =
 * nchains ceil(nsamp / thin) draws, chain k's first in order k.  The chains are equally shaped, live on one device and share X and y (the
 * first chain's are used); thin >= 1 and the window checks of bnr_chains_summary.  W is formed on the device from u and lambda of the same
 * row, in the order the sweep uses.  loglik (n x D, nullable) is handed to bnr_psis_weights: elpd_loo[n] and pareto_k[n] are that call's
 * results on that matrix, bit for bit (r_eff: n values or NULL), a row holding a NaN following its convention.  With its normalised weights
 * w_is, every sum in draw order from 0.0:
 *     loo_mean[i] = y_i - sum_s w_is resid_is
 *     loo_sd[i]   = sqrt(sum_s w_is (var_is + m_is^2) - loo_mean[i]^2),  m_is = y_i - resid_is
 * logml[D], loo_mean, loo_sd, loglik and n_bad are nullable.  Nothing of any chain is written: tables, iteration counters, RNG and event
 * counters stay as they were; a pending bnr_chain_run_async is waited for. */
int bnr_chains_marginal_loo(bnr_chain *const *chains, int32_t nchains, int32_t first_row, int32_t nsamp, int32_t thin, const double *r_eff,
                            double *elpd_loo, double *pareto_k, double *loo_mean, double *loo_sd, double *logml, double *loglik, int32_t *n_bad);

/* "mloo_batch_draws": draws per device batch (0 = automatic: the batch's matrices stay within about 1 GiB).  Performance only. */
int bnr_mloo_set_option(const char *name, int64_t value);

#ifdef __cplusplus
}
#endif
#endif /* BNR_MLOO_H */
