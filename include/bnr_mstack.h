/*
 * bnr_mstack.h -- C ABI of libbnr_mstack.so: chain stacking on the MARGINAL PSIS-LOO of every chain (include/bnr_mloo.h), from one pass over the
 * pooled draws, with the leave-one-out predictive checks (include/bnr_mcheck.h) of the stacked mixture; for the Bayesian network regression of
 * libbnr_hip.so (include/bnr_hip.h).  An ADDITION to the reference.  A sixth library beside libbnr_hip.so, libbnr_mloo.so, libbnr_medge.so,
 * libbnr_mpred.so and libbnr_mcheck.so, with a gfx950 code object of its own that holds the four kernels of libbnr_mloo.so, the two row kernels
 * of libbnr_mcheck.so and one more (csrc/bnr_mstack_kernels.h); linked against libbnr_hip.so, it reads the chains through bnr_chain_device_view,
 * runs PSIS through bnr_psis_weights and the solver through bnr_stacking_weights.  It exports the bnr_* functions below and nothing else.
 *
 * Chains are k = 0 .. K - 1.  Each has nd = ceil(nsamp / thin) draws; chain k's draws are columns k nd .. (k + 1) nd - 1 of the pooled n x (K nd)
 * matrices loglik, resid and var of bnr_chains_marginal_loo (one Gram and one factorization per draw, once).
 *   Per-chain LOO.  bnr_psis_weights on chain k's n x nd slice of loglik (the tail length comes from nd; r_eff NULL or n values, the same for
 *     every chain) gives elpd_chain[k][i], pareto_k_chain[k][i] and the normalised log weights lw_kis.  Row k is bit for bit what
 *     bnr_chains_marginal_loo(&chains[k], 1, ...) returns: no output of a draw depends on the other draws of a call.
 *   Weights.  bnr_stacking_weights on the transposed elpd_chain over the rows that are finite in every chain.  No row left: every weight 1 / K,
 *     *gap NaN, *iters 0 (bnr_chains_stack's convention).  fixed_weights[K] (nullable) skips the solver: checked like bnr_chains_wsummary's weights
 *     (finite, >= 0, one > 0, |sum - 1| <= 1e-9) and used as given; *gap is then NaN and *iters 0.
 *   Stacked score.  elpd_stack_i = M_i + log sum_{k: w_k > 0} w_k exp(elpd_ki - M_i), M_i the largest elpd_ki among the chains with w_k > 0, k
 *     ascending (bnr_chains_stack's formula); NaN for a row left out.
 *   Stacked LOO predictive of row i.  The mixture  sum_{k: w_k > 0} sum_s (w_k exp(lw_kis)) N(y_i - resid_kis, var_kis).  The weight of a
 *     component is the product w_k exp(lw_kis), rounded once; NaN where lw_kis is not finite.  Chains with w_k = 0 are dropped and their columns
 *     are not read: the mixture has D+ = K+ nd components, K+ the chains with w_k > 0, in chain order and then draw order.  mean, sd, pit, lower
 *     and upper are then bnr_mcheck.h's definitions on those D+ components: the summation order (fixed by D+ alone), the bracket over the retained
 *     components, the bisection, the point masses and the NaN conventions.
 * Bit for bit: with w = e_k the five outputs are bnr_chains_marginal_loo_predict(&chains[k], 1, ...)'s; with K = 1 (w = 1) the raw form is
 * bnr_weighted_mixture.  No output of a row depends on the other rows, on the batch ("mstack_batch_draws"), on which outputs were asked for or on
 * the call.
 * A bad draw (n_bad > 0) is NaN in every row of its chain: no row is left, the weights are 1 / K and all five checks are NaN.
 *
 * Conventions: those of bnr_mloo.h.  Every pointer is a host pointer; a status other than BNR_OK leaves its message in bnr_last_error().
 * DESIGN.md section 8.
 */
#ifndef BNR_MSTACK_H
#define BNR_MSTACK_H

#include "bnr_mcheck.h"

#ifdef __cplusplus
extern "C" {
#endif

#define BNR_MSTACK_ABI_VERSION 1

int bnr_mstack_abi_version(void);

/* The kernels alone, on a caller's matrices: mean, var, logw rows x (K nd) with a row's components contiguous, chain k's in columns k nd ..
 * (k + 1) nd - 1; logw the normalised log weights within every chain; weights[K] the chain weights (bnr_chains_wsummary's checks, 1 <= K <=
 * BNR_STACK_MAX_CHAINS); y[rows] nullable (then no pit: asking for one is refused).  out_mean, out_sd, out_pit, out_lower, out_upper: rows doubles
 * each, every one nullable but not all of them.  Checks (bnr_weighted_mixture's, same messages): rows, K nd >= 1 with nd >= 1; rows K nd < 2^31;
 * 0 < p_lo < p_hi < 1 (read only where a bound is asked for); the weights; the device. */
int bnr_stacked_mixture(int32_t device, int32_t rows, int32_t K, int32_t nd, const double *mean, const double *var, const double *logw,
                        const double *weights, const double *y, double p_lo, double p_hi, double *out_mean, double *out_sd, double *out_pit,
                        double *out_lower, double *out_upper);

/* The chain form: the draws, the checks and the refusals of bnr_chains_marginal_loo (same order, same messages); after them 1 <= nchains <=
 * BNR_STACK_MAX_CHAINS, max_iter >= 1 and gap_tol positive and finite (bnr_stacking_weights'), the checks of fixed_weights, and p_lo / p_hi only
 * where a bound is asked for.  weights[K], elpd_chain and pareto_k_chain (K x n, row k chain k's) are required; elpd_stack[n], gap, iters, loo_mean,
 * loo_sd, loo_pit, loo_lower, loo_upper (n each), logml[K nd] and n_bad are nullable.  One run over all chains leaves loglik, resid and var on the
 * device; loglik goes to the host, is repacked per chain and through K calls of bnr_psis_weights; the solver runs on the host; the log weights go
 * back to the device and the kernels run on the resident resid, var and y; only n-vectors come back from the checks.  Nothing of any chain is
 * written: tables, iteration counters, RNG and event counters stay as they were; a pending bnr_chain_run_async is waited for. */
int bnr_chains_marginal_stack(bnr_chain *const *chains, int32_t nchains, int32_t first_row, int32_t nsamp, int32_t thin, const double *r_eff,
                              const double *fixed_weights, int32_t max_iter, double gap_tol, double p_lo, double p_hi, double *weights,
                              double *elpd_chain, double *pareto_k_chain, double *elpd_stack, double *gap, int32_t *iters, double *loo_mean,
                              double *loo_sd, double *loo_pit, double *loo_lower, double *loo_upper, double *logml, int32_t *n_bad);

/* "mstack_batch_draws": draws per device batch of the factorizations (0 = automatic: the batch's matrices stay within about 1 GiB).
 * Performance only. */
int bnr_mstack_set_option(const char *name, int64_t value);

#ifdef __cplusplus
}
#endif
#endif /* BNR_MSTACK_H */
