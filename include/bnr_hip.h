/*
 * bnr_hip.h -- C ABI of libbnr_hip.so: the MI355X (gfx950) implementation of the Gibbs hot path of
 * BayesianNetworkRegression.jl (reference: src/gibbs.jl + src/gig.jl + src/convergence.jl).
 *
 * The reference is pure Julia and has no FFI seam; this header IS the seam a maintainer would bind with
 * `ccall` (julia/BNRHip.jl) and that the Python host mirror binds with ctypes
 * (bayesiannetworkregression.jl_amd/_capi.py).  Every entry point names the reference code it replaces.
 *
 * Conventions
 *   - plain C types only; no exceptions cross the ABI; every call returns an int status (BNR_OK == 0);
 *     bnr_last_error() gives a thread-local message for the last non-zero status.
 *   - all floating point data is IEEE double, as in the reference (gibbs.jl:835-841).
 *   - host matrices are COLUMN-MAJOR (Julia `Matrix` memory): X is n x q with q = V(V+1)/2 columns in the
 *     column-wise lower-triangle order of utils.jl:50-55.
 *   - state tables handed to bnr_chain_fetch/bnr_chain_load use the reference layout
 *     Array{Float64,3}(tot_save,d1,d2), column-major, ITERATION INDEX FASTEST.
 *   - row/iteration indices are 1-based exactly as in run! (gibbs.jl:849-864) unless stated otherwise.
 *   - a handle is used by one host thread at a time; different handles may be driven concurrently.
 *   - the caller keeps ownership of every host buffer; the library owns all device memory of a chain until
 *     bnr_chain_destroy.
 */
#ifndef BNR_HIP_H
#define BNR_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BNR_ABI_VERSION 19  /* 2: + bnr_chain_create_like, bnr_group_*, bnr_chain_summary; 3: + bnr_*_prepare; 4: + bnr_comm_*, bnr_rhat;
                               5: + bnr_chain_create_typed, bnr_chain_create_from_matrices, bnr_device_synchronize; 6: + bnr_comm_info;
                               7: + option "xi_weights", bnr_host_xi_weight; 8: + bnr_chain_predict, bnr_chain_predict_from_matrices,
                               bnr_chain_loglik_stats, option "predict_block_rows"; 9: + bnr_chain_loo, bnr_psis_loo;
                               10: + bnr_chains_summary, bnr_chains_predict, bnr_chains_predict_from_matrices, bnr_chains_loglik_stats, bnr_chains_loo,
                               bnr_host_pred_noise, option "summary_block_cols"; 11: + bnr_chain_loo_predict, bnr_chains_loo_predict,
                               bnr_psis_weights; 12: + bnr_chain_rank_diag, bnr_chains_rank_diag, bnr_rank_normalize, bnr_host_ndtri,
                               option "rank_block_cols"; 13: + bnr_chain_hdi, bnr_chains_hdi, bnr_hdi;
                               14: + bnr_host_gig_attempts; 15: + bnr_chain_inclusion, bnr_chains_inclusion,
                               bnr_inclusion; 16: + bnr_stacking_weights, bnr_chains_stack, bnr_chains_wsummary, bnr_chains_wpredict,
                               bnr_wquantile; 17: + bnr_chain_cov, bnr_chains_cov, bnr_cov, option "cov_block_cols";
                               18: + bnr_chain_device_view, bnr_set_last_error; 19: + bnr_host_unit (all additive) */

enum {
    BNR_OK = 0,
    BNR_ERR_BAD_ARG = 1,
    BNR_ERR_HIP = 2,          /* a HIP runtime call failed (no device, out of memory, launch failure ...) */
    BNR_ERR_CHOLESKY = 3,     /* Cholesky failed after the jitter ladder (the reference rethrows: gibbs.jl:337-343) */
    BNR_ERR_SAMPLER_CAP = 4   /* a rejection sampler hit its attempt cap: returned ONCE, by the call in which it happened; the rows were written with
                               * the samplers' fall-backs, the table stays valid, later calls on the chain are not failed for it (the counter
                               * of bnr_chain_counters keeps the total).  The reference's rejection loops are unbounded and never raise here. */
};

typedef struct bnr_chain bnr_chain;   /* opaque: one Gibbs chain resident on one GPU */

/* hyper-parameters of Fit!/generate_samples! (gibbs.jl:725-727, 897-899) */
typedef struct {
    double eta, zeta, iota, aDelta, bDelta, nu;
} bnr_hyper;

/* progress callback: called from the calling host thread every prog_freq iterations
 * (the reference's `put!(channel,true)`, gibbs.jl:854-856).  `done` = iterations completed in this call. */
typedef void (*bnr_progress_cb)(void *user, int64_t done);

int bnr_abi_version(void);
const char *bnr_last_error(void);
int bnr_device_count(int *count);
int bnr_device_synchronize(int32_t device);          /* hipDeviceSynchronize on `device` (hosts that hold no HIP binding of their own) */
int bnr_runtime_version(int *version);               /* hipRuntimeGetVersion of the HIP runtime the library is bound to */

/* Allocate a chain: copies X (n x q col-major) and y to HBM, allocates the tot_save-row state table and all
 * work space on `device`.  Replaces the allocation half of initialize_and_run! (gibbs.jl:822-841).
 * The RNG stream is keyed by seed + chain_id (the reference's Xoshiro(seed+c), gibbs.jl:928).
 * Limits (BNR_ERR_BAD_ARG otherwise): 1 <= R <= 32, V >= 2, n <= 14000 (LDS budgets of single-workgroup kernels; round 5: R*V is no longer limited --
 * beyond 15360 the scalar tail reads u from the table row instead of staging it in LDS). */
int bnr_chain_create(int32_t n, int32_t V, int32_t R, const double *X, const double *y, const bnr_hyper *hyper,
                     uint64_t seed, int32_t chain_id, int32_t device, int32_t tot_save, bnr_chain **out);
/* The same with the model matrix in the caller's own element type -- the reference builds X_new as Matrix{eltype(T)} (gibbs.jl:917:
 * Bool for 0/1 adjacency data, Int, Float64 ...) -- uploaded as it is (a Bool/UInt8 matrix is 1/8 of the PCIe traffic) and converted
 * to the f64 device layout by a kernel.  X: n x q column-major elements of x_dtype. */
enum { BNR_F64 = 0, BNR_U8 = 1 /* Julia Bool / UInt8 */, BNR_I32 = 2, BNR_I64 = 3 /* Julia Int */, BNR_F32 = 4 };
int bnr_chain_create_typed(int32_t n, int32_t V, int32_t R, const void *X, int32_t x_dtype, const double *y, const bnr_hyper *hyper,
                           uint64_t seed, int32_t chain_id, int32_t device, int32_t tot_save, bnr_chain **out);
/* ... and straight from the vector of n adjacency matrices (x_transform = true: setup_X!, gibbs.jl:239-247, runs on the device):
 * A[i] points at a V x V column-major matrix of x_dtype; row i of the model matrix is lower_triangle(A[i]) (utils.jl:40-57: the
 * column-wise lower triangle including the diagonal, reading A[i][l, k] for l >= k -- the matrices need not be symmetric). */
int bnr_chain_create_from_matrices(int32_t n, int32_t V, int32_t R, const void *const *A, int32_t x_dtype, const double *y,
                                   const bnr_hyper *hyper, uint64_t seed, int32_t chain_id, int32_t device, int32_t tot_save,
                                   bnr_chain **out);
/* Another chain of the same fit on the same device: same X, y, sizes, hyper-parameters and model options as `donor`, own seed /
 * chain id, own table and work space.  The read-only device inputs (X, y, index maps) are SHARED with the donor, not
 * copied -- the reference hands the same X, y to every pmap worker (gibbs.jl:946-948) -- and live until the last chain
 * using them is destroyed. */
int bnr_chain_create_like(const bnr_chain *donor, uint64_t seed, int32_t chain_id, int32_t tot_save, bnr_chain **out);
int bnr_chain_destroy(bnr_chain *chain);

/* initialize_variables! (gibbs.jl:191-224): draws row 1 from the priors; sets the iteration counter to 1. */
int bnr_chain_init_prior(bnr_chain *chain);

/* run! (gibbs.jl:849-864): for i in first_index:total { gibbs_sample!(row j); purge ring }.
 * purge_burn <= 0 means `nothing`.  Synchronous.  *next_row (optional) receives the row index j the next
 * call would write.  cb may be NULL. */
int bnr_chain_run(bnr_chain *chain, int32_t first_index, int32_t nburn, int32_t total, int32_t purge_burn,
                  int32_t prog_freq, bnr_progress_cb cb, void *user, int32_t *next_row);
/* same, but only enqueues the work on the chain's stream(s); pair with bnr_chain_sync.  Lets several chains
 * that share one GPU overlap (the reference runs chains concurrently under pmap, gibbs.jl:946). */
int bnr_chain_run_async(bnr_chain *chain, int32_t first_index, int32_t nburn, int32_t total, int32_t purge_burn);
int bnr_chain_sync(bnr_chain *chain, int32_t *next_row);
/* Optional: build everything the run loop replays (the captured hipGraphs of graph_k sweeps and of one sweep) now, so that the
 * first bnr_chain_run / bnr_group_run call is already steady state.  run! has no counterpart (gibbs.jl:849-864 just loops);
 * calling it is never required -- the first run call does the same lazily -- and never changes results. */
int bnr_chain_prepare(bnr_chain *chain);

/* Lockstep group: the chains one `pmap` call of generate_samples! hands to the workers (gibbs.jl:946-948, 989-1000)
 * when several of them live on ONE GPU.  All members (equal n, V, R and table length, same device) advance together:
 * bnr_group_run is run! (gibbs.jl:849-864) for every member with the same (first_index, nburn, total, purge_burn),
 * each kernel of a sweep being launched once for the whole group.  Members stay independent chains (own seed + chain
 * id, own table); their tables are bitwise what bnr_chain_run would have produced for each of them alone.  The group
 * does not own its members; destroying a member dissolves the group (its handle stays valid until bnr_group_destroy,
 * bnr_group_run then fails).  cb ticks like chain 1's callback. */
typedef struct bnr_group bnr_group;
int bnr_group_create(bnr_chain *const *chains, int32_t nchains, bnr_group **out);
int bnr_group_destroy(bnr_group *group);
int bnr_group_run(bnr_group *group, int32_t first_index, int32_t nburn, int32_t total, int32_t purge_burn,
                  int32_t prog_freq, bnr_progress_cb cb, void *user, int32_t *next_row);
/* options "graph", "graph_k", "overlap", "profiling" as for bnr_chain_set_option / bnr_chain_set_profiling; timings as
 * bnr_chain_last_timing (which = 1: one k_gram launch covers all members) */
int bnr_group_prepare(bnr_group *group);   /* as bnr_chain_prepare */
int bnr_group_set_option(bnr_group *group, const char *name, int64_t value);
int bnr_group_last_timing(bnr_group *group, int32_t which, double *avg_us, int64_t *launches);

/* gibbs_sample!(state, row, ...) (gibbs.jl:663-677) for one row, and the ten update_*! functions in sweep
 * order (gibbs.jl:267-636): test hooks mirroring test/init-tests.jl:76,96-124.  `row` is 1-based (>= 2);
 * `iter` is the global iteration id that keys the RNG counter for this row. */
int bnr_gibbs_step(bnr_chain *chain, int32_t row, int64_t iter);
int bnr_update_tau2(bnr_chain *chain, int32_t row, int64_t iter);
int bnr_update_u_xi(bnr_chain *chain, int32_t row, int64_t iter);
int bnr_update_gamma(bnr_chain *chain, int32_t row, int64_t iter);
int bnr_update_D(bnr_chain *chain, int32_t row, int64_t iter);
int bnr_update_theta(bnr_chain *chain, int32_t row, int64_t iter);
int bnr_update_Delta(bnr_chain *chain, int32_t row, int64_t iter);
int bnr_update_M(bnr_chain *chain, int32_t row, int64_t iter);
int bnr_update_mu(bnr_chain *chain, int32_t row, int64_t iter);
int bnr_update_Lambda(bnr_chain *chain, int32_t row, int64_t iter);
int bnr_update_pi(bnr_chain *chain, int32_t row, int64_t iter);

/* iteration counter (global id of the last drawn row; init row = 1) */
int bnr_chain_get_iter(bnr_chain *chain, int64_t *iter);
int bnr_chain_set_iter(bnr_chain *chain, int64_t iter);

/* Copy rows first_row..last_row (1-based, inclusive) of the device table into / out of host arrays laid out as
 * the reference's state Table: 11 live columns tau2(.,1,1) u(.,R,V) xi(.,V,1) gamma(.,q,1) S(.,q,1) theta Delta
 * M(.,R,R) mu lam(.,R,1) pi(.,R,3), each Array{Float64,3}(host_tot,d1,d2).  Host row = device row + host_row_offset.
 * The 3 dead columns of the reference (Sigma^-1, invC, mu_t: allocated, never written, utils.jl:72-84) are the
 * caller's business.  Any column pointer may be NULL (skipped). */
int bnr_chain_fetch(bnr_chain *chain, int32_t first_row, int32_t last_row, int32_t host_tot, int32_t host_row_offset,
                    double *tau2, double *u, double *xi, double *gamma, double *S, double *theta, double *Delta,
                    double *M, double *mu, double *lam, double *pi);
int bnr_chain_load(bnr_chain *chain, int32_t first_row, int32_t last_row, int32_t host_tot, int32_t host_row_offset,
                   const double *tau2, const double *u, const double *xi, const double *gamma, const double *S,
                   const double *theta, const double *Delta, const double *M, const double *mu, const double *lam,
                   const double *pi);

/* copy_table!(table, to, from) for `count` consecutive rows on the device (utils.jl:72-84; used by the
 * continuation loops gibbs.jl:991-993, 1172).  Overlap-safe. */
int bnr_chain_move_rows(bnr_chain *chain, int32_t to_row, int32_t from_row, int32_t count);
/* Re-allocate the device table with new_tot rows, keeping rows 1..min(old,new) (generate_samples_dbl!
 * allocates a new table per round, gibbs.jl:1164-1172). */
int bnr_chain_resize(bnr_chain *chain, int32_t new_tot);

/* split-Rhat, first half of rhat() (convergence.jl:4-65) done on the device for ONE chain: for every parameter
 * p of gamma (q) then xi (V) over rows first_row..first_row+nsamp-1, the mean and the corrected variance of the
 * first floor(nsamp/2) and the last floor(nsamp/2) samples.  stats (host): 4*(q+V) doubles, laid out
 * [mean_h0(q+V) | var_h0(q+V) | mean_h1(q+V) | var_h1(q+V)].  This is the per-chain message that is
 * all-gathered across ranks (RCCL via torch.distributed in the host layer). */
int bnr_chain_rhat_stats(bnr_chain *chain, int32_t first_row, int32_t nsamp, double *stats);
/* Summary(results) (gibbs.jl:1214-1250) computed on the device over rows first_row .. first_row+nsamp-1 of this chain's
 * table: mean_gamma[q] = posterior mean of every edge coefficient, lower[q] / upper[q] = the k_lo-th / k_hi-th smallest
 * sample of every edge (1-based; the reference takes sort(gamma)[round(nsamp*lower_bound)] and [round(nsamp*upper_bound)]),
 * prob_xi[V] = posterior mean of xi.  Exact selection; only 3q + V doubles cross PCIe.  Rounding to `digits` is the caller's. */
int bnr_chain_summary(bnr_chain *chain, int32_t first_row, int32_t nsamp, int32_t k_lo, int32_t k_hi,
                      double *mean_gamma, double *lower, double *upper, double *prob_xi);

/* Posterior prediction -- an ADDITION to the reference (y = mu + X gamma + eps, eps ~ N(0, tau2): gibbs.jl:270, 432, 566).
 * posterior of the mean response mu + x.gamma of m new rows over rows first_row..first_row+nsamp-1 of this chain; X: m x q column-major in
 * x_dtype (as bnr_chain_create_typed) or m V x V matrices (as bnr_chain_create_from_matrices); y (nullable): observed responses of the rows
 * -> lpd / pwaic (NULL when y is NULL)
 *   mean[m]           posterior mean of eta_s = mu_s + x.gamma_s over the draws s of the window
 *   lower[m], upper[m] the k_lo-th / k_hi-th smallest eta_s (1-based; exact selection, as bnr_chain_summary).  A credible interval of the MEAN
 *                     response, not a predictive interval for a new observation (that adds eps ~ N(0, tau2_s): pred_lower / pred_upper of bnr_chains_predict).
 *   lpd[m]            log (1/nsamp) sum_s N(y_i | eta_is, tau2_s): the pointwise log predictive density (log-mean-exp, no overflow)
 *   pwaic[m]          the sample variance (ddof 1) over s of log N(y_i | eta_is, tau2_s): the pointwise WAIC penalty
 * Computed on the device (k_predict: f64 MFMA GEMM over the trace rows; k_summary; k_pred_loglik) in blocks of rows (tunable
 * "predict_block_rows"); only 5 m doubles cross PCIe back.  The table, the iteration counter, the RNG and the counters are not touched; the
 * chain may be a member of a group.  BNR_ERR_BAD_ARG: a NULL output, a pending asynchronous run, a window outside the table, ranks outside
 * 1..nsamp, m < 1, an unknown x_dtype. */
int bnr_chain_predict(bnr_chain *chain, int32_t first_row, int32_t nsamp, int32_t m, const void *X, int32_t x_dtype, const double *y,
                      int32_t k_lo, int32_t k_hi, double *mean, double *lower, double *upper, double *lpd, double *pwaic);
int bnr_chain_predict_from_matrices(bnr_chain *chain, int32_t first_row, int32_t nsamp, int32_t m, const void *const *A, int32_t x_dtype,
                      const double *y, int32_t k_lo, int32_t k_hi, double *mean, double *lower, double *upper, double *lpd, double *pwaic);
/* pointwise log predictive density and WAIC penalty of the chain's own training rows (X, y already on the device): lpd[n], pwaic[n] */
int bnr_chain_loglik_stats(bnr_chain *chain, int32_t first_row, int32_t nsamp, double *lpd, double *pwaic);

/* PSIS-LOO -- an ADDITION to the reference: Pareto-smoothed importance-sampling leave-one-out cross-validation (Vehtari, Gelman & Gabry 2017)
 * as loo 2.x computes it, per row i over the draws s of the window with l_s = log N(y_i | mu_s + x_i.gamma_s, tau2_s): log ratios -l_s,
 * tail length M = ceil(min(0.2 nsamp, 3 sqrt(nsamp / r_eff_i))); with M >= 5 the M largest log weights are replaced by the quantiles of a
 * generalized Pareto fit (Zhang & Stephens 2009, weakly informative prior), then truncated at the largest raw weight.
 *   lpd[i]       log (1/nsamp) sum_s exp(l_s): bit for bit bnr_chain_loglik_stats's lpd (NULL: not returned)
 *   elpd_loo[i]  log sum_s w_s exp(l_s) / sum_s w_s over the smoothed weights w_s
 *   pareto_k[i]  the fitted shape k-hat after the prior adjustment (k M + 5) / (M + 10); +inf where no tail was fitted (M < 5, a constant
 *                tail, a NaN shape).  A row with a non-finite l gets elpd_loo NaN and pareto_k +inf (not an error).
 * r_eff: NULL (every r_eff_i = 1) or one relative efficiency per row.  Tails are sorted in LDS: M <= BNR_PSIS_MAX_TAIL (8192) per row; a
 * longer tail (0.2 nsamp and 3 sqrt(nsamp / r_eff_i) both above 8192) is refused with BNR_ERR_BAD_ARG, as is r_eff_i <= 0 or non-finite.  Results are bitwise the same for
 * every "predict_block_rows" and every call.  DESIGN.md section 8.
 * bnr_chain_loo: the chain's own n training rows over rows first_row..first_row+nsamp-1 (k_predict, then k_psis on the device); checks as
 *   bnr_chain_loglik_stats (NULL outputs, a pending asynchronous run, the window).  The table, the iteration counter, the RNG and the counters
 *   are not touched.
 * bnr_psis_loo: the same kernel on a caller's m x nsamp log-likelihood matrix (host, ROW-major: row i's nsamp draws contiguous) on `device`. */
int bnr_chain_loo(bnr_chain *chain, int32_t first_row, int32_t nsamp, const double *r_eff, double *lpd, double *elpd_loo, double *pareto_k);
int bnr_psis_loo(int32_t device, int32_t m, int32_t nsamp, const double *loglik, const double *r_eff, double *elpd_loo, double *pareto_k,
                 double *lpd);

/* Pooled chains -- an ADDITION to the reference (whose Results keeps states[1] only): the statistics above over the POOLED WINDOW of several
 * chains of one fit that live on one device.  The pooled window is the concatenation, in the order the chains are passed, of rows
 * first_row..first_row+nsamp-1 of each of the nchains chains: S = nchains * nsamp draws, pooled draw c * nsamp + s (0-based) = the s-th window
 * row of chains[c].  Ranks (k_lo, k_hi) are 1..S; the PSIS tail length comes from S (refused above BNR_PSIS_MAX_TAIL as for one chain).
 *   bnr_chains_summary       = bnr_chain_summary over the pooled window.  The (q + V) S staged doubles are processed in blocks of parameter
 *                              columns of about 1 GiB (tunable "summary_block_cols" of chains[0]); results do not depend on the block.
 *   bnr_chains_predict / _from_matrices = bnr_chain_predict / _from_matrices over the pooled window, plus three nullable outputs:
 *       pred_lower[m], pred_upper[m]  (both or neither) the k_lo-th / k_hi-th smallest draw of a NEW OBSERVATION y~_is = eta_is + sqrt(tau2_s) z_is:
 *                        a predictive interval, where lower / upper are a credible interval of the mean response.  z_is is counter-based:
 *                        bnr_host_normal(pred_seed, it = s (pooled draw index, 0-based), site = 40 (SITE_PRED), elem = i, att = 0) with i the
 *                        0-based index of the row IN THIS CALL'S m rows -- so the same row predicted at another position of another call gets
 *                        another draw, while the block size, the grid, the input format and earlier calls never change one.  The key is
 *                        pred_seed itself (no chain id is added).  Host mirror: bnr_host_pred_noise.
 *       pit[m]           (needs y) the probability integral transform of y_i under the posterior predictive, Rao-Blackwellised (no draws):
 *                        (1/S) sum_s Phi((y_i - eta_is) / sqrt(tau2_s)), Phi(z) = erfc(-z / sqrt 2) / 2.  Uniform on (0, 1) over rows when the
 *                        predictive distribution is calibrated.  (In-sample for training rows; the leave-one-out PIT: bnr_chains_loo_predict.)
 *   bnr_chains_loglik_stats  = bnr_chain_loglik_stats over the pooled window; pit[n] (nullable): the PIT of the training responses.
 *   bnr_chains_loo           = bnr_chain_loo over the pooled window.
 * All work runs eagerly on chains[0]'s stream after the library has waited for the other chains' streams; no table, iteration counter, RNG
 * state or counter of any chain is touched, and the chains may be members of a group.  BNR_ERR_BAD_ARG: chains NULL, nchains < 1, a NULL or
 * repeated chain, chains on different devices or of different n, V, R, a pending asynchronous run on ANY of them, a window outside any
 * chain's table, ranks outside 1..S, more than 2^31 - 1 pooled draws, only one of pred_lower / pred_upper, pit without y; otherwise the checks
 * of the single-chain call.  With nchains == 1 and pred_lower, pred_upper, pit NULL every result is bit for bit the single-chain function's.
 * DESIGN.md section 8. */
int bnr_chains_summary(bnr_chain *const *chains, int32_t nchains, int32_t first_row, int32_t nsamp, int32_t k_lo, int32_t k_hi,
                       double *mean_gamma, double *lower, double *upper, double *prob_xi);
int bnr_chains_predict(bnr_chain *const *chains, int32_t nchains, int32_t first_row, int32_t nsamp, int32_t m, const void *X, int32_t x_dtype,
                       const double *y, int32_t k_lo, int32_t k_hi, double *mean, double *lower, double *upper, double *lpd, double *pwaic,
                       uint64_t pred_seed, double *pred_lower, double *pred_upper, double *pit);
int bnr_chains_predict_from_matrices(bnr_chain *const *chains, int32_t nchains, int32_t first_row, int32_t nsamp, int32_t m, const void *const *A,
                       int32_t x_dtype, const double *y, int32_t k_lo, int32_t k_hi, double *mean, double *lower, double *upper, double *lpd,
                       double *pwaic, uint64_t pred_seed, double *pred_lower, double *pred_upper, double *pit);
int bnr_chains_loglik_stats(bnr_chain *const *chains, int32_t nchains, int32_t first_row, int32_t nsamp, double *lpd, double *pwaic, double *pit);
int bnr_chains_loo(bnr_chain *const *chains, int32_t nchains, int32_t first_row, int32_t nsamp, const double *r_eff, double *lpd,
                   double *elpd_loo, double *pareto_k);

/* LOO predictive checks (ABI 11) -- an ADDITION to the reference: the PSIS weights themselves and the leave-one-out posterior predictive of
 * every training row over the pooled window of nchains >= 1 chains (draws and checks as bnr_chains_loo).  For row i and pooled draw s, with
 * l_is = log N(y_i | eta_is, tau2_s) and lw_is the log weight of bnr_chain_loo after smoothing and truncation at 0:
 *   w_is = exp(lw_is - logsumexp_s lw_is)                                   loo's weights(normalize = TRUE)
 *   the tail = the M draws largest in the lexicographic order (lw, s) (what a stable ascending argsort of lw picks); position j of that
 *       order gets the j-th quantile of the fitted generalized Pareto.  The composite key has no ties, so every w_is is well defined;
 *       against bnr_chain_loo, whose tail order is (lw, l), elpd_loo and pareto_k can differ only by the order of tied terms.
 *   lpd[i], elpd_loo[i], pareto_k[i]   as bnr_chains_loo (lpd bit for bit), elpd_loo[i] = log sum_s w_is exp(l_is) from the weights above
 *   loo_mean[i]  = sum_s w_is eta_is
 *   loo_sd[i]    = sqrt(sum_s w_is (tau2_s + eta_is^2) - loo_mean[i]^2): the sd of a NEW OBSERVATION of row i under the LOO predictive, a
 *                  mixture moment (no random numbers)
 *   loo_pit[i]   = sum_s w_is Phi((y_i - eta_is) / sqrt(tau2_s)), Phi(z) = erfc(-z / sqrt 2) / 2: the leave-one-out PIT
 *   loo_lower[i], loo_upper[i] = the p_lo- and p_hi-quantile of the mixture CDF F_i(t) = sum_s w_is Phi((t - eta_is) / sqrt(tau2_s)), by
 *                  bisection from [min_s(eta_is - c sd_s), max_s(eta_is + c sd_s)] (Phi(-c) < min(p_lo, 1 - p_hi) / 2) down to 2^-40 of that
 *                  bracket; the midpoint is returned.  The Rao-Blackwellised counterpart of the PIT: no sort, and NOT loo's weighted sample
 *                  quantile (.wquant).
 * Every output is nullable (with only lpd / elpd_loo / pareto_k the call still runs the weights kernel).  A row with a non-finite l gets NaN in
 * every output but lpd (as bnr_chains_loo computes it) and pareto_k (+inf).  p_lo, p_hi are read only when a bound is requested:
 * BNR_ERR_BAD_ARG unless 0 < p_lo < p_hi < 1.  Otherwise the checks of bnr_chains_loo / bnr_chain_loo, the tail limit included: a tail entry
 * is 12 bytes in LDS here (16 there), so the longest tail stays BNR_PSIS_MAX_TAIL (8192) and nothing more is refused.  Rows are processed in
 * blocks of about 512 MiB of eta with the log weights beside them ("predict_block_rows" overrides); no result depends on the block, the grid
 * or the call, bit for bit.  Nothing of any chain is written: tables, iteration counters, RNG and counters stay untouched.
 * bnr_psis_weights: the companion of bnr_psis_loo for a caller's m x nsamp log-likelihood matrix (host, row-major): log_weights[m x nsamp]
 *   (row-major, required) = log w_is; elpd_loo[m], pareto_k[m] nullable.  DESIGN.md section 8. */
int bnr_chain_loo_predict(bnr_chain *chain, int32_t first_row, int32_t nsamp, const double *r_eff, double p_lo, double p_hi, double *lpd,
                          double *elpd_loo, double *pareto_k, double *loo_mean, double *loo_sd, double *loo_pit, double *loo_lower,
                          double *loo_upper);
int bnr_chains_loo_predict(bnr_chain *const *chains, int32_t nchains, int32_t first_row, int32_t nsamp, const double *r_eff, double p_lo,
                           double p_hi, double *lpd, double *elpd_loo, double *pareto_k, double *loo_mean, double *loo_sd, double *loo_pit,
                           double *loo_lower, double *loo_upper);
int bnr_psis_weights(int32_t device, int32_t m, int32_t nsamp, const double *loglik, const double *r_eff, double *log_weights, double *elpd_loo,
                     double *pareto_k);

/* Rank-normalised convergence diagnostics (ABI 12) -- an ADDITION to the reference: the R-hat, bulk / tail effective sample sizes and Monte
 * Carlo standard error of Vehtari, Gelman, Simpson, Carpenter, Buerkner (2021) as `posterior` 1.x computes them (rhat, ess_bulk, ess_tail,
 * ess_mean, mcse_mean), for every parameter in [gamma(q) | xi(V)] over the pooled window (rows first_row .. first_row+nsamp-1 of every chain,
 * in the order the chains are passed) of nchains >= 1 chains of one device.  Every window gives two split chains of h = nsamp / 2 rows
 * (rows [0, h) and [nsamp - h, nsamp): an odd window drops its middle row); only these S' = 2 nchains h draws are ranked.
 *   z = Phi^-1((r - 3/8) / (S' + 1/4)), r the average rank (ties share the mean of their positions; -0 ties with +0), Phi^-1: bnr_host_ndtri.
 *   rhat_bulk = split-R-hat of z, sqrt(((h-1)/h W + B) / W); rhat_tail the same for the z of |x - median| (the median: mean of the two middle
 *   order statistics).  The caller combines rhat = fmax(rhat_bulk, rhat_tail).
 *   ess_bulk = bnr_ess_from_stats' estimator (truncated at max_lag) on z; ess_tail = the smaller of that estimator on I(x <= x_(k)),
 *   k = floor((S'-1) prob) + 1, prob = 0.05 and 0.95 (NaN if either is); ess_mean the estimator on x; mcse_mean = sd / sqrt(ess_mean).
 * Each output holds q + V doubles, gamma first, and may be NULL (not all): what is not asked for is not computed.  A parameter with a
 * non-finite draw, or with all S' draws equal, is NaN in every output (not bnr_rhat's 1.0); rhat_tail is NaN where the folded draws are all
 * equal.  Checks: those of bnr_chains_summary, nsamp >= 8, 2 <= max_lag <= nsamp / 2.  Runs eagerly on chains[0]'s stream; the columns are
 * staged in blocks of about 1 GiB of draws (option "rank_block_cols" of chains[0] overrides); no result depends on the block, the grid or
 * the call, bit for bit, and bnr_chain_rank_diag is the pooled call with one chain.  Nothing of any chain is written.
 * bnr_rank_normalize: the average ranks and normal scores of every row of a caller's m x S matrix (host, row-major), each row on its own;
 *   ranks[m x S], z[m x S] nullable (not both).  +-Inf rank as numbers; a row that holds a NaN gets NaN everywhere.  DESIGN.md section 8. */
int bnr_chain_rank_diag(bnr_chain *chain, int32_t first_row, int32_t nsamp, int32_t max_lag, double *rhat_bulk, double *rhat_tail,
                        double *ess_bulk, double *ess_tail, double *ess_mean, double *mcse_mean);
int bnr_chains_rank_diag(bnr_chain *const *chains, int32_t nchains, int32_t first_row, int32_t nsamp, int32_t max_lag, double *rhat_bulk,
                         double *rhat_tail, double *ess_bulk, double *ess_tail, double *ess_mean, double *mcse_mean);
int bnr_rank_normalize(int32_t device, int32_t m, int32_t S, const double *x, double *ranks, double *z);

/* Highest-density intervals, the median and the sign probabilities (ABI 13) -- an ADDITION to the reference -- of every parameter in
 * [gamma(q) | xi(V)] over the pooled window of nchains >= 1 chains of one device: all S = nchains nsamp draws take part (no split halves).
 *   For each of the nprob <= 8 levels probs[k] in (0, 1): w = floor(probs[k] S) (computed in double; at most S - 1), and among the windows
 *   x_(j) .. x_(j+w), j = 0 .. S - w - 1, of the sorted draws the one of the smallest width x_(j+w) - x_(j) (one f64 subtraction), the smallest j
 *   among equal widths: lower = x_(j), upper = x_(j+w).  This is the HDI of a sample as ArviZ (_hdi) and R's HDInterval::hdi compute it
 *   (unimodal; first minimum).
 *   median = the mean of the two middle order statistics x_(S/2) and x_(S/2+1) (1-based; S = 1: the draw), as bnr_chains_rank_diag takes it.
 *   p_pos, p_neg = the shares of draws above and below zero (exact counts over S; -0 counts as zero); P(x = 0) = 1 - p_pos - p_neg.
 * lower and upper hold nprob (q + V) doubles, level k at offset k (q + V), gamma first; median, p_pos and p_neg hold q + V doubles.  Every
 * output may be NULL (not all of them); lower and upper come together, and without them nprob may be 0 and no window is searched.
 * A parameter with a NaN draw is NaN in every output; one with an infinite draw (and no NaN) is NaN in lower, upper and median, and its shares
 * are counted (+Inf above, -Inf below zero).  All draws equal: lower = upper = the draw.  -0 is reported as +0.
 * Checks: those of bnr_chains_summary, 0 <= nprob <= 8, every level in (0, 1), lower and upper both or neither, nprob >= 1 with them.  Runs
 * eagerly on chains[0]'s stream; the columns are staged in blocks of about 1 GiB of draws (option "rank_block_cols" of chains[0] overrides);
 * no result depends on the block, the grid, the outputs requested or the call, bit for bit, and bnr_chain_hdi is the pooled call with one
 * chain.  Nothing of any chain is written.
 * bnr_hdi: the same for every row of a caller's m x S matrix (host, row-major), each row on its own; lower and upper hold nprob m doubles,
 *   level k at offset k m.  DESIGN.md section 8. */
int bnr_chain_hdi(bnr_chain *chain, int32_t first_row, int32_t nsamp, int32_t nprob, const double *probs, double *lower, double *upper,
                  double *median, double *p_pos, double *p_neg);
int bnr_chains_hdi(bnr_chain *const *chains, int32_t nchains, int32_t first_row, int32_t nsamp, int32_t nprob, const double *probs, double *lower,
                   double *upper, double *median, double *p_pos, double *p_neg);
int bnr_hdi(int32_t device, int32_t m, int32_t S, const double *x, int32_t nprob, const double *probs, double *lower, double *upper, double *median,
            double *p_pos, double *p_neg);

/* The joint posterior of the indicators (ABI 15) -- an ADDITION to the reference: which nodes are selected together, how many, and which node
 * sets are the most probable, over the pooled window of nchains >= 1 chains of one device (S = nchains nsamp draws, chain by chain in the
 * order passed, as for bnr_chains_hdi).  One call works on the S x B matrix z of 0/1 indicators:
 *   which = 0: B = V, z_sv = (xi_v of draw s != 0), the node indicators;  which = 1: B = R, z_sr = (lambda_r of draw s != 0), the latent
 *   dimensions in use.  The indicator is the IEEE comparison x != 0.0: -0 is zero, and a NaN counts as included.
 *   The pattern of a draw is the integer P_s = sum_k z_sk 2^k, stored as W = ceil(B / 64) little-endian 64-bit words: bit k mod 64 of word
 *   k div 64 is indicator k, the unused high bits are 0.
 *   prob[B]           = #{s : z_sk} / S, the marginal inclusion probabilities (bit for bit bnr_chains_summary's prob_xi for which = 0);
 *   joint[B x B]      = #{s : z_sk and z_sl} / S at joint[k B + l], the full symmetric co-inclusion matrix; its diagonal equals prob;
 *   size_pmf[B + 1]   = #{s : popcount(P_s) = m} / S, m = 0 .. B: the distribution of the number of included indicators;
 *   n_distinct        = the number of distinct patterns among the S draws;
 *   top_sets[ntop W], top_count[ntop]: the ntop most frequent distinct patterns and their counts, by count descending, ties by the pattern
 *   as an integer ascending; entries past n_distinct are all-zero words with count 0.
 * Every output is an exact integer count, divided once by (double)S where a double is returned.  Every output may be NULL (not all of them):
 * what is not asked for is not computed; top_sets and top_count come together and need ntop >= 1.
 * Checks: those of bnr_chains_summary, which in {0, 1}, 0 <= ntop <= 256, top_sets and top_count both or neither, at most 4096 indicators.
 * Runs eagerly on chains[0]'s stream and reads the trace rows in place; no result depends on the grid, the outputs requested or the call, bit
 * for bit, and bnr_chain_inclusion is the pooled call with one chain.  Nothing of any chain is written.
 * bnr_inclusion: the same for a caller's S x B matrix of bytes (host, row-major; a byte != 0 is 1), S >= 1, B >= 1.  DESIGN.md section 8. */
int bnr_chain_inclusion(bnr_chain *chain, int32_t first_row, int32_t nsamp, int32_t which, int32_t ntop, double *prob, double *joint,
                        double *size_pmf, int64_t *n_distinct, uint64_t *top_sets, int64_t *top_count);
int bnr_chains_inclusion(bnr_chain *const *chains, int32_t nchains, int32_t first_row, int32_t nsamp, int32_t which, int32_t ntop, double *prob,
                         double *joint, double *size_pmf, int64_t *n_distinct, uint64_t *top_sets, int64_t *top_count);
int bnr_inclusion(int32_t device, int32_t S, int32_t B, const uint8_t *z, int32_t ntop, double *prob, double *joint, double *size_pmf,
                  int64_t *n_distinct, uint64_t *top_sets, int64_t *top_count);

/* Chain stacking (ABI 16) -- an ADDITION to the reference: posterior statistics of chains that do not mix, under chain weights chosen by
 * leave-one-out predictive performance (Yao, Vehtari & Gelman 2022, "Stacking for non-mixing Bayesian computations", JMLR 23).
 * bnr_stacking_weights (host code, no GPU): the weights on the simplex that maximise f(w) = (1 / n) sum_i log sum_k w_k exp(lpd_ik) for the
 *   n x K matrix lpd (row-major) of pointwise predictive log densities, by the multiplicative (EM) fixed point: p_ik = exp(lpd_ik - max_k lpd_ik),
 *   w = 1 / K, then g_k = (1 / n) sum_i p_ik / sum_j w_j p_ij and w <- w o g (divided by its sum, which is 1 up to rounding).  f is concave and
 *   sum_k w_k g_k = 1, so f(w*) - f(w) <= max_k g_k - 1 for every w* of the simplex: the iteration stops when that bound is <= gap_tol, or
 *   after max_iter updates (no error: the caller reads *gap).  *gap = the last max_k g_k - 1 (that of the weights returned), *objective = f(w)
 *   with the row maxima added back, *iters = the updates applied (objective, gap, iters nullable).  Every sum runs in index order.
 *   BNR_ERR_BAD_ARG: n < 1, K < 1 or K > BNR_STACK_MAX_CHAINS, a NaN or +Inf entry, a row that is -Inf in every chain, max_iter < 1, gap_tol not
 *   finite or <= 0.
 * bnr_chains_stack: row k of elpd_chain / pareto_k_chain (K x n, nullable) is bit for bit what bnr_chain_loo(chains[k], first_row, nsamp, r_eff)
 *   returns (the tail length comes from nsamp, not from K nsamp); weights[K] = bnr_stacking_weights of the transposed elpd_chain over the rows
 *   that are finite in every chain; elpd_stack[n] (nullable): elpd_stack_i = M_i + log sum_{k: w_k > 0} w_k exp(elpd_ki - M_i), M_i the largest
 *   elpd_ki among the chains with w_k > 0, k ascending; NaN for a row left out.  No row left: every weight 1 / K, *gap NaN, *iters 0.
 *   Checks: those of bnr_chains_loo, nchains <= BNR_STACK_MAX_CHAINS, max_iter and gap_tol as above.  The K LOO passes run one after the other,
 *   each on its chain's stream, behind the wait every pooled call makes for the other chains' streams.  Nothing of any chain is written.
 * The weighted statistics work on columns of S = K nsamp draws, chain k's window in rows k nsamp .. (k + 1) nsamp - 1 (kernel k_wsummary); every
 *   sum below runs k ascending from 0.0, every product and addition rounded on its own:
 *   mean = sum_k w_k m_k, m_k the mean of chain k's draws exactly as bnr_chain_summary computes it;
 *   the order statistic of a rank r in 1 .. S (the ranks bnr_chains_summary takes): with T = (double)r / (double)K and
 *   W(x) = sum_k w_k (double)#{draws of chain k whose key is <= the key of x} -- the key is the order of bnr_chains_summary: numbers by value,
 *   -0 below +0 -- the draw with the smallest key for which W(x) >= T; where no draw reaches T (round-off near r = S) the largest draw among
 *   the chains with w_k > 0.  With K a power of two and w_k = 1 / K this is bnr_chains_summary's order statistic bit for bit; with w = e_k it
 *   is chain k's ceil(T)-th smallest draw.  A column holding a NaN draw is NaN in every output; +-Inf are ordered as numbers.
 *   Weights: finite, >= 0, at least one > 0, |sum_k w_k - 1| <= 1e-9 (BNR_ERR_BAD_ARG otherwise); used as given, not renormalised.
 * bnr_chains_wsummary: bnr_chains_summary under the weights (same staging blocks, option "summary_block_cols", same checks, nchains <=
 *   BNR_STACK_MAX_CHAINS; bitwise independent of the block); prob_xi = the weighted mean of every xi column.
 * bnr_chains_wpredict: bnr_chains_predict for a model matrix under the weights: mean / lower / upper from the eta columns of the pooled
 *   prediction; lpd[i] (needs y) = M + log sum_{k: w_k > 0} w_k exp(lpd_ki - M), lpd_ki = bit for bit bnr_chain_predict's lpd of chain k, M the
 *   largest of them among the chains with w_k > 0; pred_lower / pred_upper (both or neither): the same order statistics of the columns after
 *   bnr_chains_predict's noise with pred_seed (bnr_host_pred_noise).  Rows in blocks ("predict_block_rows"); no result depends on the block.
 * bnr_wquantile: the kernel on the rows of a caller's m x (K nsamp) matrix (host, row-major), each row on its own, on a stream of its own;
 *   lower and upper are nullable as a pair, mean is nullable, not all three.  DESIGN.md section 8. */
#define BNR_STACK_MAX_CHAINS 32
int bnr_stacking_weights(int32_t n, int32_t K, const double *lpd, int32_t max_iter, double gap_tol, double *weights, double *objective, double *gap,
                         int32_t *iters);
int bnr_chains_stack(bnr_chain *const *chains, int32_t nchains, int32_t first_row, int32_t nsamp, const double *r_eff, int32_t max_iter, double gap_tol,
                     double *weights, double *elpd_chain, double *pareto_k_chain, double *elpd_stack, double *gap, int32_t *iters);
int bnr_chains_wsummary(bnr_chain *const *chains, int32_t nchains, const double *weights, int32_t first_row, int32_t nsamp, int32_t k_lo, int32_t k_hi,
                        double *mean_gamma, double *lower, double *upper, double *prob_xi);
int bnr_chains_wpredict(bnr_chain *const *chains, int32_t nchains, const double *weights, int32_t first_row, int32_t nsamp, int32_t m, const void *X,
                        int32_t x_dtype, const double *y, int32_t k_lo, int32_t k_hi, double *mean, double *lower, double *upper, double *lpd,
                        uint64_t pred_seed, double *pred_lower, double *pred_upper);
int bnr_wquantile(int32_t device, int32_t m, int32_t K, int32_t nsamp, const double *x, const double *weights, int32_t k_lo, int32_t k_hi, double *mean,
                  double *lower, double *upper);

/* Posterior covariance of the edge coefficients (ABI 17) -- an ADDITION to the reference: vcov(fit) for ncols chosen gamma columns over the pooled
 * window of nchains >= 1 chains of one device (S = nchains nsamp draws, chain by chain in the order passed, as for bnr_chains_summary), computed
 * on the device from the resident traces (kernel k_cov, v_mfma_f64_16x16x4_f64 with the draws as the K dimension); nothing of any chain is written.
 *   cols[ncols]: 0-based gamma indices, in any order, repeats allowed; NULL = 0 .. q - 1 and then ncols must be q.
 *   mean[ncols]: the centre c of every column -- weights NULL: bnr_chains_summary's mean_gamma of that column, bit for bit; with weights:
 *   bnr_chains_wsummary's.
 *   cov[ncols x ncols], row-major, both triangles: with G_k[a, b] = sum over chain k's window of (x_sa - c_a)(x_sb - c_b) -- the centre is
 *   subtracted from every draw before the product --
 *     weights NULL: cov[a, b] = (sum_k G_k[a, b]) / (S - 1), numpy's cov;
 *     with weights w: cov[a, b] = (sum_k w_k G_k[a, b]) / nsamp, the covariance of the mixture sum_k w_k P_k of the chains' empirical measures;
 *   k ascending from 0.0, every product and addition rounded on its own.  The order of every entry's sums is fixed by (nchains, nsamp) alone: an
 *   entry does not depend on the grid, on the column block (option "cov_block_cols" of chains[0]: the columns staged at a time for the centres
 *   and the columns of a Gram block; 0 = blocks whose temporaries stay near 1 GiB), on which other columns were asked for, or on the call, bit
 *   for bit; cov[a, b] and cov[b, a] are the same bits.  A column holding a NaN or +-Inf draw is NaN in its whole row and column of cov; every
 *   other entry is unaffected.
 * Checks (BNR_ERR_BAD_ARG): those of bnr_chains_summary's window, S < 2, ncols < 1, an index outside 0 .. q - 1, cols NULL with ncols != q; with
 * weights those of bnr_chains_wsummary (finite, >= 0, one > 0, |sum - 1| <= 1e-9, nchains <= BNR_STACK_MAX_CHAINS; used as given).  A buffer that
 * does not fit on the device is BNR_ERR_HIP.  Runs eagerly on chains[0]'s stream; bnr_chain_cov is the pooled call on a list of one.
 * bnr_cov: the same for a caller's (K nsamp) x m matrix x (host, row-major: draws x columns, chain k's draws in rows k nsamp ..; K >= 1,
 * nsamp >= 1, m >= 1, K nsamp >= 2), all m columns, on a stream of its own; the matrix is uploaded whole.  DESIGN.md section 8. */
int bnr_chain_cov(bnr_chain *chain, int32_t first_row, int32_t nsamp, int32_t ncols, const int32_t *cols, double *mean, double *cov);
int bnr_chains_cov(bnr_chain *const *chains, int32_t nchains, const double *weights, int32_t first_row, int32_t nsamp, int32_t ncols,
                   const int32_t *cols, double *mean, double *cov);
int bnr_cov(int32_t device, int32_t K, int32_t nsamp, int32_t m, const double *x, const double *weights, double *mean, double *cov);

/* The device side of a chain, for a companion library (ABI 18) -- libbnr_mloo.so (include/bnr_mloo.h) reads the chains' tables through it; no
 * kernel of this library is involved.  Row r (0-based) of the table starts at trace + r * rowlen doubles; inside a row tau2 is the double at
 * o_tau2, mu at o_mu, lambda_t at o_lam + t, u_{t,v} at o_u + t + R v, gamma_e at o_gamma + e, S_e at o_S + e.  X is column-major with leading
 * dimension ldx >= n_pad: rows n .. n_pad - 1 and columns q .. q_pad - 1 hold 0.0.  ek[e] / el[e]: the column node and the row node of edge e.
 * The pointers stay valid until the chain is destroyed or resized (bnr_chain_resize moves trace and changes tot); chains made with
 * bnr_chain_create_like share X, y, ek, el.  The call waits for whatever the chain's stream (and its group's) still holds -- a pending
 * bnr_chain_run_async included, which stays pending for bnr_chain_sync -- so what the pointers show is complete.  Nothing is written.
 * bnr_set_last_error: the companion library's way to leave its message where bnr_last_error() finds it; returns code. */
typedef struct bnr_chain_view {
    int32_t device;
    int32_t n, n_pad, V, R, q, q_pad, tot, rowlen;
    int32_t o_tau2, o_mu, o_lam, o_u, o_gamma, o_S;
    int32_t ldx;
    const double *X, *y;
    const int32_t *ek, *el;
    const double *trace;
} bnr_chain_view;
int bnr_chain_device_view(bnr_chain *chain, bnr_chain_view *out);
int bnr_set_last_error(int code, const char *msg);

/* Effective sample size -- an ADDITION to the reference (which only has split-Rhat; north-star item "Rhat/ESS check").
 * bnr_chain_ess_stats: this chain's message over rows first_row .. first_row+nsamp-1: for both halves of the window (the
 *   halves of split-Rhat) the mean, the variance and the autocovariances at lags 0..max_lag-1 of gamma (q) then xi (V):
 *   stats[half][2 + max_lag][q + V], computed on the device.
 * bnr_ess_from_stats: bulk ESS over the messages of all chains ([chain][half][2 + max_lag][nparams]) with the estimator of
 *   Stan / MCMCDiagnosticTools.ess (split chains, Geyer's initial positive and monotone sequence), truncated at max_lag;
 *   NaN for a constant parameter.  ess[nparams]. */
int bnr_chain_ess_stats(bnr_chain *chain, int32_t first_row, int32_t nsamp, int32_t max_lag, double *stats);
int bnr_ess_from_stats(const double *stats, int32_t nchains, int32_t nparams, int32_t nsamp, int32_t max_lag, double *ess);

/* The convergence check over ALL chains of a fit, wherever they live (return_psrf_VOI, gibbs.jl:771-789, over rhat(),
 * convergence.jl:4-65; the reference's master receives whole state tables from its pmap workers, gibbs.jl:946-957 -- here only
 * 4 (q + V) doubles per chain travel).  Chains c = 1..nchains_total are placed round-robin: rank r holds, in increasing c, the
 * chains with (c - 1) % world == r.  bnr_rhat reduces every local chain's window rows burn+1 .. burn+nsamp on the device,
 * all-gathers the messages through `comm`, and finishes the same rhat_xi[V] / rhat_gamma[q] on every rank.
 * comm == NULL: one process holds all chains.
 * A communicator is either RCCL (ncclAllGather over xGMI on the library's own communicator; librccl.so is bound at run time, so
 * single-GPU use needs no RCCL) -- rank 0 calls bnr_comm_unique_id and the host carries the 128 bytes to the other ranks by
 * whatever connects them already (Julia Distributed, torch.distributed's store, MPI), then every rank calls bnr_comm_create_rccl
 * (a collective call) -- or a callback the host implements (an all-gather of `count` doubles per rank into recv[world * count] in
 * rank order, returning 0; used by the gloo tests and by hosts that bring their own transport). */
typedef struct bnr_comm bnr_comm;
typedef struct { char bytes[128]; } bnr_unique_id;                       /* ncclUniqueId */
typedef int (*bnr_allgather_fn)(void *ctx, const double *send, double *recv, int64_t count);
int bnr_comm_unique_id(bnr_unique_id *id);
int bnr_comm_create_rccl(const bnr_unique_id *id, int32_t rank, int32_t world, int32_t device, bnr_comm **out);
int bnr_comm_create_callback(int32_t rank, int32_t world, bnr_allgather_fn fn, void *ctx, bnr_comm **out);
int bnr_comm_destroy(bnr_comm *comm);
int bnr_comm_allgather(bnr_comm *comm, const double *send, double *recv, int64_t count);   /* host buffers; comm NULL = copy */
/* What the transport itself reports (any out pointer may be NULL): kind 0 = no communicator (one rank), 1 = RCCL, 2 = host callback;
 * rank / world as given at creation; rccl_ranks / rccl_rank = ncclCommCount / ncclCommUserRank of the library's communicator (0 / -1
 * unless kind 1) -- the number of ranks RCCL really connected, which a multi-GPU run reports beside its throughput (the reference's
 * counterpart is nworkers() after addprocs, gibbs.jl:946-948). */
int bnr_comm_info(bnr_comm *comm, int32_t *kind, int32_t *rank, int32_t *world, int32_t *rccl_ranks, int32_t *rccl_rank);
int bnr_rhat(bnr_chain *const *chains, int32_t nchains_local, int32_t nchains_total, bnr_comm *comm, int32_t burn, int32_t nsamp,
             double *rhat_xi, double *rhat_gamma);

/* second half: combine nchains messages (host arrays, chain-major) into Rhat per parameter.  Pure host code.
 * rhat: q+V doubles (gamma first, then xi).  Replaces convergence.jl:49-61. */
int bnr_rhat_from_stats(const double *stats, int32_t nchains, int32_t nparams, int32_t nsamp, double *rhat);

/* event counters: out[0]=Cholesky jitter events, out[1]=NaN-weight events (node updates that took the fair coin of gibbs.jl:392-400; always 0
 * with the default log-space weights, which cannot under/overflow; see "xi_weights"),
 * out[2]=sampler attempt-cap events, out[3]=Cholesky hard failures, out[4..7] where they happened (node, Psi, M, G+I).  A failed factorization of
 * G + I counts ONE in out[3] and out[7] per chain and gamma update -- the reference's one PosDefException of gibbs.jl:434 -- whatever the
 * factorization variant, the number of panels that meet the bad pivot, or the group the chain runs in */
int bnr_chain_counters(bnr_chain *chain, int64_t out[8]);

/* kernel timing: average device time in microseconds of the kernels of the last bnr_chain_run call, measured
 * with HIP events on the chain's own stream.  which: 0 = whole iteration, 1 = Gram kernel (X diag(S) X');
 * (which = 3 / 4: is a byte image of X in use / does the Gram run on the i8 pipe, see bnr_chain_set_option.)
 * which = 2 reports how the last run call was issued: *launches = sweeps replayed from captured graphs, *avg_us = sweeps
 * launched eagerly (a steady-state run is all replay). */
int bnr_chain_set_profiling(bnr_chain *chain, int32_t enable);
int bnr_chain_last_timing(bnr_chain *chain, int32_t which, double *avg_us, int64_t *launches);

/* diagnostics: in-kernel cycle stamps of a -DBNR_STAMPS build (zeros otherwise) */
int bnr_chain_debug_read(bnr_chain *chain, uint64_t *out, int32_t count);
/* diagnostics: average duration of `reps` back-to-back launches of the Gram kernel on the chain's stream */
int bnr_chain_debug_time_gram(bnr_chain *chain, int32_t reps, double *avg_us);
/* diagnostics: copy an internal work buffer to the host (0 = factorization matrix E, 1 = rhs b, 2 = a4, 3 = Gram partials; the scalar branch's
 * carried state, count checked against the buffer's size (BNR_ERR_BAD_ARG beyond it):
 *   4 = inv(M) (R x R, column-major) then logdet M: R^2 + 1 doubles, as the next node update of a sweep reads them (written by update_M!'s
 *       workgroup of the scalar tail, or by the refresh of the carried sums after init, load or a hook);
 *   5 = the carried sums: [0] rr = |y - mu - X gamma|^2, [1] sig_q = sum_e ((gamma_e - W_e)^2 / 2) / S_e, [2] tau = sqrt(tau2),
 *       [3] the pre-drawn next tau2, [4] the iteration id it belongs to (-1: none), [5..7] unused: at most 8 doubles;
 *   6 = the back-projection's per-block partial sums [nblk_bp][1 + 3R] (nblk_bp = ceil(q / 32)): [0] sum of S over the block's edges,
 *       [1 + 3r + c] the log-likelihood sums of update_Lambda! with lambda_r set to (0, 1, -1)[c].) */
int bnr_chain_debug_copy(bnr_chain *chain, int32_t which, double *out, int64_t count);
/* diagnostics: internal sizes {n_pad, q_pad, ksplit (K slices = planes of Gram partials), ntile (64-row tiles), kcp, kslab, i8L (i8 Gram: padded K slice,
 * bytes per mask row, digit planes), rowlen (doubles per trace row on the device)}; the Gram partials of debug_copy(3) are [ksplit][ntile (ntile + 1) / 2][64 x 64],
 * tile (ti >= tj) at index ti (ti + 1) / 2 + tj, element (i, j) of a tile at [j * 64 + i] */
int bnr_chain_debug_dims(bnr_chain *chain, int32_t *out8);
/* timing experiments of round 4 (removed in round 5, tools/experiments/README.md): the entry point remains and returns BNR_ERR_BAD_ARG.  (flags bit 0 made the
 * kernels of the scalar branch return at once -- what the critical chain costs without company.) */
int bnr_debug_set_exp(int32_t device, int32_t flags);

/* model options (change results):
 *   "xi_weights" 0 (default): update_u_xi!'s inclusion weight in log space, w = 1 / (1 + exp(log w_bot - log w_top)) -- never under/overflows;
 *               1: the reference's own arithmetic (gibbs.jl:349-360): w_top = (1 - Delta) pdf_top, w_bot = Delta pdf_bot from the two (V-1)-dim
 *               log densities (same determinant lemma and Woodbury identity), w = w_top / (w_bot + w_top) with its under/overflow: w = 0 or 1
 *               without a draw where one density underflows, NaN -> fair coin (counted in bnr_chain_counters out[1]) where both do.  Residual
 *               differences from the reference's dense pdf: the lemma uses the jittered Sigma^-1 when the jitter ladder fired (out[0]); where the
 *               dense covariance is not positive definite the reference throws PosDefException, here the lemma's value is used.
 *               Takes effect from the next sweep (also on a group member); bnr_chain_create_like inherits the donor's setting.  Any other value:
 *               BNR_ERR_BAD_ARG.  Default: same tables bit for bit as without the option.
 * tunables (performance only; never change results):
 *   "graph"     1 (default): replay captured hipGraphs of graph_k sweeps; 0: launch every kernel eagerly
 *   "graph_k"   sweeps per captured graph (default 16; a ladder graph_k, graph_k / 2, ..., 1 is captured so that a batch of any length is pure replay)
 *   "overlap"   1 (default): scalar branch and Gram/factorization branch of a sweep on two streams; 0: one stream
 *   "gram_variant" 0 (default): the Gram kernel is chosen per launch (k_gram8 when the launch has more than two workgroups per CU,
 *               k_gram otherwise); 8 / 16 force one of them.  Both write the same partial tiles bit for bit.  (9..14: the persistent /
 *               resident experiments of rounds 3-4, removed from the tree in round 5 -- tools/experiments/README.md -- and refused by name.)
 *   "profiling" 1: record HIP events around every k_gram launch (forces eager launches), see bnr_chain_last_timing
 *   "factor_variant" -1 (default): chosen by size -- 0 below n_pad = 1024, 3 from there on; 0: right-looking factorization, one
 *               32-column panel per launch (k_gram_reduce + k_chol_step); 2: right-looking, two panels per launch (k_chol_step2); 3: 2 with
 *               the whole trailing matrix updated at every other launch only (K = 128); (1: left-looking k_chol_ll, 4: data-flow k_chol_df, 5: one workgroup per
 *               chain k_chol_small -- experiments of rounds 3-4, removed in round 5 and refused)
 *   "fuse_reduce" 1 / -1 (default): launch 0 of the one-panel factorization also sums the Gram's K-split partial tiles (no k_gram_reduce
 *               launch); 0: separate reduction pass
 *   "reduce_epw" 0 (default): how many eighths of a partial tile a reduction workgroup of that launch 0 sums is chosen per launch (4 where the launch is then one
 *               round of workgroups, else 1); 1, 2, 4 force it for a lockstep group (a chain alone always runs 1).  The same sums in the same order: bitwise
 *               the same tables.
 *   "group_xpass" -1 (default): a lockstep group whose members share the device copy of X (bnr_chain_create_like) runs ONE X pass
 *               for all members (k_xpass_group) when X has 8 MB or more per chain; 1: always; 0: one pass per member
 *   "split_sums" -1 (default): a chain run alone computes the back-projection's partial sums (update_theta!, update_Lambda!) in a launch of
 *               their own in front of the scalar tail, off the critical chain; 1: always; 0: inside the back-projection
 *   "spw_cap"   1..4 (default 1 since round 6: one block each beside the pipelined panel sweep; rounds 3-5: 4): super blocks per update workgroup of the factorization, at most
 *   "tail_after" / "node_after" (round 6): WHEN the scalar branch of a sweep (k_tail: theta, mu, Lambda, pi, the next tau2; k_node: tau2, u, xi; the X pass; k_rhs) starts
 *               relative to the Gram / factorization branch it runs beside.  "tail_after" 0: k_tail of the previous sweep waits for the Gram; -1: it starts as soon as the
 *               dispatcher lets it (rounds 1-5).  "node_after" p >= 0: k_node waits for launch number p of the factorization; -1: follows k_tail at once.  -2 (default):
 *               chosen from a size model -- ordered where the factorization is the longer chain by a margin (n = 500, V = 100; n = 2000), free-running for small n or
 *               large q.  Graph edges between the two branches; the tables do not depend on them.
 *   "wide_backproj" -1 (default): a lockstep group whose back-projection has more chunks of 32 edges than the GPU has CUs, and a chain alone with 8 x CUs or more,
 *               run k_backproj64 -- a workgroup owns 64 edges, two of its waves draw (one rejection sampler each, one edge per lane: attempt 0 of every edge, then the
 *               refused edges' further attempts packed over the wave; fewer instructions per edge); smaller launches keep k_backproj, whose draws have the shorter
 *               latency; 1: always; 0: never.  Bitwise the same tables.
 *   Experiments ("nop_fork", "pipeline", "gate_us", "linear", "linear_merge", "linear_debug", "group_backproj", "resv_mask", "crit_origin"; rounds 3-4,
 *               profiles/round*_experiments_notes.txt): all measured no faster, part of them polled device memory.  Removed from the tree in
 *               round 5 (tools/experiments/README.md): the library refuses them by name.  Their host scaffolding (streams, fields and
 *               predicates of the sweep's issue path) is gone too; what is left of them in csrc/ is listed in DESIGN.md, section 3.
 *   "predict_block_rows" (chains only) rows per block of bnr_chain_predict / bnr_chain_loglik_stats, whose work buffer holds rows x nsamp
 *               doubles; rounded up to whole 32-row tiles.  0 (default): as many rows as fit in about 1 GiB.  The results are bitwise the same
 *               for every value.
 *   "summary_block_cols" (chains only) parameter columns per staging block of bnr_chain_summary / bnr_chains_summary, whose buffer holds columns x S
 *               doubles.  0 (default): as many as fit in about 1 GiB.  The results are bitwise the same for every value.
 *   "cov_block_cols" (chains only) edge columns per block of bnr_chain_cov / bnr_chains_cov: the columns staged at a time for the centres (columns x S
 *               doubles) and the columns of a Gram block (nchains x columns^2 doubles).  0 (default): blocks of about 1 GiB each.  The results
 *               are bitwise the same for every value.
 *   "byte_x"   (chains only) 0: the X passes read the f64 matrix although a byte image of X exists; 1 (default): the byte image
 *               (kept when the model matrix came as Bool/UInt8, or as Int32/Int64 with every value in 0..255; docs/src/man/inputdata.md)
 *   "gram_i8"   (chains only; round 5) 1 (the default from n_pad^2 q >= 2.5e8 on, where it was measured faster -- n = 500, V = 100 and
 *               larger; smaller problems default to 0): the model matrix came integer-typed with every entry 0 or 1
 *               (the reference's adjacency data, docs/src/man/inputdata.md:5-10) -- its Gram X diag(S) X' (gibbs.jl:434) runs on the i8 matrix pipe:
 *               S as i8L = 7 or 8 planes of balanced base-256 digits under the exponent of its largest entry (k_sdigits), one exact i32 Gram per plane
 *               (k_gram_i8, v_mfma_i32_16x16x64_i8), recombined in f64.  |G_i8 - G_exact|_ij <= (X X')_ij 2^(e - 8 i8L + 1) <= 8 q 2^(-8 i8L) max S <= 1e-12 max |G| (S rounded to nearest: two-sided); the tables
 *               agree with the f64 Gram's to that size of perturbation (NOT bit for bit) and with the oracle to the same 1e-6 as everything
 *               else.  0: the f64 Gram also for a binary matrix.  A matrix that is not binary has no i8 path (setting 1 is refused).
 *               bnr_chain_last_timing(which = 4): *avg_us = 1 when the chain's (its group's) Gram runs on the i8 pipe, *launches = i8L.
 * All variants except "gram_i8" give the same tables bit for bit.  bnr_chain_last_timing(which = 3) says whether a byte image is in use. */
int bnr_chain_set_option(bnr_chain *chain, const char *name, int64_t value);

/* Host-side copies of the draw-site primitives (same source as the device functions), exported so that the
 * CPU test-suite can check the product's RNG contract against the oracle without a GPU. */
void bnr_host_philox(const uint32_t ctr[4], const uint32_t key[2], uint32_t out[4]);
/* the uniform of one 64-bit word (ABI 19), what both halves of bnr_host_uniform2 go through: ((w >> 11) + 1/2) 2^-53 in float64, strictly inside
 * (0, 1) -- odd multiples of 2^-54 below 1/2, multiples of 2^-52 from 1/2 upward (1/2 itself included), 1 - 2^-53 where the formula would round to 1 */
double bnr_host_unit(uint64_t w);
void bnr_host_uniform2(uint64_t seed, uint32_t it, uint32_t site, uint32_t elem, uint32_t att, double out[2]);
double bnr_host_normal(uint64_t seed, uint32_t it, uint32_t site, uint32_t elem, uint32_t att);
double bnr_host_gamma(uint64_t seed, double shape, uint32_t it, uint32_t site, uint32_t elem);
double bnr_host_gig(uint64_t seed, double lambda, double chi, double psi, uint32_t it, uint32_t elem);
/* the index of the rejection attempt that bnr_host_gig's draw accepts (the same loop): -1 for the draws without a rejection loop of their own
 * (chi ~ 0, psi ~ 0, invalid parameters), BNR_MAX_ATTEMPTS (100000) when the attempt cap is hit */
int32_t bnr_host_gig_attempts(uint64_t seed, double lambda, double chi, double psi, uint32_t it, uint32_t elem);
int32_t bnr_host_edge_index(int32_t V, int32_t l, int32_t k);   /* 0-based (l,k) -> 0-based e; utils.jl:50-55 */
/* the noise of bnr_chains_predict's predictive draws (the kernel's own function; no GPU needed): an ni x ns block, ROW-major,
 * out[(i - i0) * ns + (s - s0)] = bnr_host_normal(seed, s, 40 (SITE_PRED), i, 0) for rows i0 <= i < i0 + ni and pooled draws s0 <= s < s0 + ns */
void bnr_host_pred_noise(uint64_t seed, uint32_t s0, uint32_t ns, uint32_t i0, uint32_t ni, double *out);
/* Phi^-1 as k_rank evaluates it (Wichura's AS 241, PPND16); no GPU */
double bnr_host_ndtri(double p);
/* the node weight of option "xi_weights" = 1 (the kernel's own function): w = (1 - Delta) exp(lt) / (Delta exp(lb) + (1 - Delta) exp(lt)),
 * written literally (gibbs.jl:349-351), so 0, 1 and NaN arise where they arise in the reference */
double bnr_host_xi_weight(double lt, double lb, double Delta);
/* The K split the library would choose for the Gram  X diag(S) X'  of gibbs.jl:434 on a device with `ncu` compute units (no GPU needed):
 * out[0] = K slices, out[1] = columns per slice (padded), out[2] = q_pad, out[3] = MiB of X one K-group of a workgroup addresses through its
 * 2 GiB buffer window.  The split is raised beyond what fills the chip until that span fits the window (n up to the 14 000-row limit with any V
 * the device holds); BNR_ERR_BAD_ARG when no split of at most 4096 slices does. */
int bnr_host_gram_plan(int32_t n, int32_t V, int32_t ncu, int32_t out[4]);

#ifdef __cplusplus
}
#endif
#endif /* BNR_HIP_H */
