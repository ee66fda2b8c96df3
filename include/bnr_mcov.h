/*
 * bnr_mcov.h -- C ABI of libbnr_mcov.so: the Rao-Blackwellised covariance of the edge coefficients of the Bayesian network regression of
 * libbnr_hip.so (include/bnr_hip.h), gamma integrated out on the device.  An ADDITION to the reference.  A seventh library beside libbnr_hip.so
 * and the five other marginal libraries, with a gfx950 code object of its own that holds the four kernels of marginal PSIS-LOO, k_medge_proj and
 * k_medge_summary of libbnr_medge.so (include/bnr_medge.h) and four more; linked against libbnr_hip.so, it reads the chains through
 * bnr_chain_device_view.  It exports the bnr_* functions below and nothing else.
 *
 * Given phi = (tau2, mu, u, lambda, S) of a table row the whole vector of edge coefficients is Gaussian in closed form (bnr_medge.h): with
 * D = diag S, A = I_n + X D X^T = L L^T and T = L^-1 X
 *     gamma | phi, y ~ N(m, tau2 (D - D X^T A^-1 X D)),        (X^T A^-1 X)_ab = t[a, b] = sum_i T_ia T_ib
 * so the posterior of gamma is the mixture of those normals over the draws s of phi, and by the law of total covariance
 *     cov = within + between
 *     within[a, b]  = sum_s omega_s tau2_s (S_sa [a == b] - S_sa S_sb t_s[a, b])         ([a == b]: the two columns are the same EDGE)
 *     between[a, b] = sum_s omega_s (m_sa - mean_a)(m_sb - mean_b),      mean = sum_s omega_s m_s
 * `within` carries none of the within-draw noise of the gamma draws that bnr_chains_cov (bnr_hip.h) estimates it from.
 *
 * Conventions: those of bnr_medge.h.  Every pointer is a host pointer; a status other than BNR_OK leaves its message in bnr_last_error().
 * Columns: cols[ncols] holds 0-based edge indices, in any order, repeats allowed; NULL means all q edges in order, and ncols must then be q
 * (bnr_chains_cov's rules and refusals).  Draws and weights: bnr_chains_marginal_edges' -- chain k's nd draws come first in order k, D = K nd,
 * omega_s = w_k / nd; weights[K] nullable (1 / K each), checked as bnr_mixture_summary checks them and used as given.
 * Limits (BNR_ERR_BAD_ARG beyond): n <= BNR_MLOO_MAX_N, ncols >= 1, every index in 0 .. q - 1.  Every size is computed in size_t; a buffer that
 * does not fit on the device is BNR_ERR_HIP.
 *
 * Outputs.  mean[ncols]: bnr_mixture_summary's mean of those columns, bit for bit.  within, cov[ncols x ncols]: row-major, both triangles;
 * [a, b] and [b, a] hold the same bits.  m, v (D x ncols, a draw's values contiguous): bnr_marginal_gamma's m and v of the chosen columns, bit for
 * bit (v keeps that call's clamp at 0).  mean, cov and within are nullable, but not all three; m, v and n_bad are nullable.
 * The diagonal of within is NOT clamped: unlike v_e and var_within it may fall a rounding below 0 where the data determine a coefficient
 * (S_a t[a, a] -> 1); a reader who needs >= 0 clamps it.
 *
 * The rounding sequence of one entry (every product and every sum rounded on its own, -ffp-contract=off; csrc/bnr_mcov_kernels.h):
 *   1. per draw s and column a: T_sia = sum_j (L_s^-1)_ij x_ja, one f64 MFMA accumulator, j in steps of 4 from 0 up to the first multiple of 32
 *      past the diagonal of i's 16-row tile (k_medge_proj's order: m and v come out of the same accumulators); scale_sa = sqrt(tau2_s) * S_sa;
 *      T'_sia = scale_sa * T_sia.  tau2 and S enter here and nowhere else in the off-diagonal terms.
 *   2. Gw_k[a, b] = sum over the draws s of chain k, ascending, and inside a draw over the rows i = 0 .. rs - 1 ascending (rs = n rounded up to
 *      16; T' of a row >= n is 0.0) of T'_sia T'_sib: one f64 MFMA accumulator from 0.0 for the whole chain, rows in steps of 4, inside a step
 *      the MFMA's own order.  The entry is computed once, for the larger of the two positions first; a product does not depend on the order of
 *      its factors.
 *   3. dg_a = sum_k (chain sum of tau2_s * S_sa / nd) w_k and mean_a = sum_k (chain sum of m_sa / nd) w_k, bnr_mixture_summary's chain sums
 *      and order (k ascending from 0.0).
 *   4. Gb_k[a, b] = sum over the draws s of chain k, ascending in steps of 4, of (m_sa - mean_a)(m_sb - mean_b): centred before the product, as
 *      bnr_chains_cov centres; one f64 MFMA accumulator from 0.0.
 *   5. gw = sum_k (Gw_k[a, b] / nd) w_k, gb = sum_k (Gb_k[a, b] / nd) w_k, k ascending from 0.0;
 *      within[a, b] = (cols[a] == cols[b] ? dg_a : 0.0) - gw;   cov[a, b] = within[a, b] + gb.
 * The order of every sum is fixed by (n, K, nd) alone: an entry does not depend on the batch ("mcov_batch_draws"), on the internal sub-batches,
 * on the grid, on which other columns were asked for, on the place of a or b in cols, or on the call, bit for bit.
 *
 * A draw whose S, tau2 or mu is not finite, or whose factorization meets a pivot that is not > 0, is flagged by the factor kernel and counted in
 * n_bad (bnr_medge.h's convention): its rows of m and v are NaN, and while n_bad > 0 every entry of mean, cov and within is NaN.  It is no error.
 * DESIGN.md section 8, "Rao-Blackwellised covariance of the edge coefficients".
 */
#ifndef BNR_MCOV_H
#define BNR_MCOV_H

#include "bnr_medge.h"

#ifdef __cplusplus
extern "C" {
#endif

#define BNR_MCOV_ABI_VERSION 1

int bnr_mcov_abi_version(void);

/* The raw form, on a caller's matrices: the inputs of bnr_marginal_gamma (X n x q column-major, y[n], tau2[D], mu[D], S and W D x q with a draw's
 * q values contiguous, W NULL: 0) for D = K nd draws, chain k's in rows k nd .. .  Checks: K >= 1, nd >= 1, K nd < 2^31, those of
 * bnr_marginal_gamma, the weights, the columns.  K = nd = 1 gives the conditional covariance of one draw: cov == within, between == 0. */
int bnr_marginal_gamma_cov(int32_t device, int32_t n, int32_t q, int32_t K, int32_t nd, const double *X, const double *y, const double *tau2,
                           const double *mu, const double *S, const double *W, const double *weights, int32_t ncols, const int32_t *cols,
                           double *mean, double *cov, double *within, double *m, double *v, int32_t *n_bad);

/* The chain form: the draws of bnr_chains_marginal_edges -- rows first_row + j thin (1-based), j = 0 .. nd - 1, nd = ceil(nsamp / thin), of every
 * chain listed, W formed on the device from u and lambda of the same row.  Checks, in this order: the chain list (bnr_chains_marginal_edges'),
 * the weights, the columns, the window.  The results are bnr_marginal_gamma_cov's on the fetched draws with K = nchains, bit for bit.
 * Nothing of any chain is written: tables, iteration counters, RNG and event counters stay as they were; a pending bnr_chain_run_async is
 * waited for. */
int bnr_chains_marginal_edge_cov(bnr_chain *const *chains, int32_t nchains, const double *weights, int32_t first_row, int32_t nsamp, int32_t thin,
                                 int32_t ncols, const int32_t *cols, double *mean, double *cov, double *within, double *m, double *v,
                                 int32_t *n_bad);

/* "mcov_batch_draws": draws per device batch of the factorization (0 = automatic: the batch's matrices stay within about 1 GiB).  Performance
 * only. */
int bnr_mcov_set_option(const char *name, int64_t value);

#ifdef __cplusplus
}
#endif
#endif /* BNR_MCOV_H */
