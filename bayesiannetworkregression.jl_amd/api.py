"""Host-side mirror of the reference's public and chain-driver API for the Gibbs hot path, over the C ABI.

SPDX-License-Identifier: GPL-2.0-or-later.  Provenance: `generate_samples` / `generate_samples_dbl` restate the schedule arithmetic of
BayesianNetworkRegression.jl (GPL-2.0; S. Ozminkowski, C. Solis-Lemus), src/gibbs.jl:955-1013 and 1119-1190 -- the `num2move` rules,
`tot_sze`, `first_index` and the messages -- because a drop-in for that API must walk the same rows; the rest is written for this repository.

Julia is not available in this image, so the thin host layer a Julia user would get from julia/BNRHip.jl
(ccall) is mirrored here in Python (ctypes) with the reference's names, argument meaning and defaults:

  Fit!                   gibbs.jl:725-751   -> Fit
  generate_samples!      gibbs.jl:897-1020  -> generate_samples
  generate_samples_dbl!  gibbs.jl:1051-1198 -> generate_samples_dbl
  initialize_and_run!    gibbs.jl:822-846   -> initialize_and_run
  run!                   gibbs.jl:849-864   -> run
  return_psrf_VOI        gibbs.jl:771-789   -> return_psrf_VOI
  Results / BNRSummary   gibbs.jl:23-43     -> Results / BNRSummary
  Summary                gibbs.jl:1214-1250 -> Summary
  (additions)                               -> Predict / BNRPrediction (posterior of the mean response of new rows), WAIC, LOO / psis_loo;
                                               pooled chains, predictive intervals and PIT: device_*_pooled, _host_pooled_*;
                                               LOO predictive checks: LOOPredict / LOOPredictive, psis_weights, device_loo_predict;
                                               rank-normalised R-hat / ESS / MCSE: RankDiagnose / RankDiagnostics, rank_normalize,
                                               device_rank_diagnostics, _host_rank_diagnostics
                                               highest-density intervals, sign probabilities, edge selection: EdgeSelect / EdgeSelection,
                                               hdi, device_edge_selection, _host_hdi
                                               joint posterior of the node indicators: NodeSets, inclusion, device_node_sets,
                                               _host_node_sets, _host_inclusion
                                               chain stacking for chains that do not mix: Stacking / ChainStacking, stacking_weights,
                                               wquantile, device_stack_chains, device_summary_stacked, device_predict_stacked, _host_*
                                               posterior covariance of the edge coefficients: EdgeCov, cov, device_edge_cov, _host_edge_cov
                                               marginal PSIS-LOO (edge coefficients integrated out): MarginalLOO, marginal_loglik,
                                               device_marginal_loo, _host_marginal_loglik
                                               marginal LOO predictive checks (PIT and intervals under the marginal weights):
                                               MarginalLOOPredict / MarginalLOOPredictive, weighted_mixture, device_marginal_loo_predict,
                                               _host_weighted_mixture, _host_marginal_loo_predict
                                               chain stacking on the marginal PSIS-LOO, one factorization pass: MarginalStack /
                                               MarginalStacking, stacked_mixture, device_marginal_stack, _host_stacked_mixture,
                                               _host_marginal_stack
  lower_triangle / create_lower_tri / setup_X!  utils.jl:17-57, gibbs.jl:239-247

All sampling runs on the GPU through libbnr_hip.so; this file holds only the schedule logic (chain fan-out,
PSRF-driven top-ups), the table layout and the post-processing that the reference also does on the host.
Chains are placed one (or several) per GPU; with torch.distributed initialised, chains are sharded over ranks and
the per-chain split-Rhat statistics are all-gathered (RCCL on GPUs, gloo on CPU tests).
"""
import dataclasses
import datetime
import inspect
import math
import random
import sys
from dataclasses import dataclass

import numpy as np

from . import _capi
from ._capi import Chain, Comm, Group, XInput, ess_from_stats, new_table, rhat_from_stats, xi_weights_code

CITATION = ("If you use BayesianNetworkRegression.jl, please cite:\n@article{Ozminkowski2022,\n"
            "author = {Ozminkowski, S. and Sol\\'{i}s-Lemus, C.},\nyear = {2022},\n"
            "title = {{Identifying microbial drivers in biological phenotypes with a Bayesian Network Regression model}},\n"
            "journal = {In preparation}\n}")


# ------------------------------------------------------------------------------------------ utils.jl
def lower_triangle(matrix):
    """utils.jl:40-57: column-wise lower triangle INCLUDING the diagonal; reads matrix[j,i], j>=i."""
    m = np.asarray(matrix)
    if m.shape[0] != m.shape[1]:
        raise ValueError("matrix must be square")
    V = m.shape[0]
    return np.concatenate([m[i:, i] for i in range(V)])


def create_lower_tri(vector, V):
    """utils.jl:17-27: inverse of lower_triangle (upper part zero)."""
    v = np.asarray(vector).reshape(-1)
    mat = np.zeros((V, V), dtype=v.dtype)
    i = 0
    for k in range(V):
        mat[k:, k] = v[i:i + V - k]
        i += V - k
    return mat


def setup_X(X, x_transform=True):
    """setup_X! (gibbs.jl:239-247) + the V,q bookkeeping of generate_samples! (907-918) -> (X_new n x q float64, V, q)."""
    if x_transform:
        V = np.asarray(X[0]).shape[0]
        q = V * (V + 1) // 2
        X_new = np.empty((len(X), q), dtype=np.float64, order="F")
        for i in range(len(X)):
            X_new[i, :] = lower_triangle(X[i])
    else:
        X_new = np.asfortranarray(X, dtype=np.float64)
        q = X_new.shape[1]
        V = int((-1 + math.sqrt(1 + 8 * q)) / 2)
    return X_new, V, q


# ------------------------------------------------------------------------------------------ output structs
@dataclass
class Results:
    """gibbs.jl:23-29.  state: dict of arrays (tot_save,d1,d2) in the reference layout (chain 1 only)."""
    state: dict
    rhatxi: np.ndarray
    rhatgamma: np.ndarray
    burn_in: int
    sampled: int
    summary_device: dict = None      # filled on request: Summary statistics computed on the GPU (see Summary)
    essxi: np.ndarray = None         # filled on request (ess_max_lag=...): bulk effective sample sizes over all chains
    essgamma: np.ndarray = None
    prediction: "BNRPrediction" = None   # filled on request (predict_X=...): posterior of the mean response of new rows, computed on the GPU (see Predict)
    waic: dict = None                # filled on request (waic=True): WAIC of the training rows from the GPU's pointwise numbers (see WAIC)
    loo: dict = None                 # filled on request (loo=True): PSIS-LOO of the training rows computed on the GPU (see LOO)
    loo_predictive: "LOOPredictive" = None   # filled on request (loo_predict=True): the LOO predictive checks of the training rows (see LOOPredict)
    rank_diag: "RankDiagnostics" = None   # filled on request (rank_diagnostics=True): rank-normalised R-hat, bulk / tail ESS and MCSE over every chain (see RankDiagnose)
    edge_selection: "EdgeSelection" = None   # filled on request (edge_selection=True): HDIs, sign probabilities and the selected edges over every chain (see EdgeSelect)
    node_sets: "NodeSets" = None     # filled on request (node_sets=True): co-inclusion, model size, the most probable node sets and the active dimensions over every chain (see NodeSets)
    stacking: "ChainStacking" = None   # filled on request (stack_chains=True): every chain's own PSIS-LOO, the stacking weights of the chains and the summaries under them (see Stacking)
    edge_cov: "EdgeCov" = None       # filled on request (edge_cov=...): the posterior covariance matrix of the edge coefficients over every chain (see EdgeCov)
    marginal_loo: dict = None        # filled on request (marginal_loo=True): PSIS-LOO with the edge coefficients integrated out, computed on the GPU (see MarginalLOO)
    marginal_edges: "MarginalEdges" = None   # filled on request (marginal_edges=True): the edge table with gamma integrated out, computed on the GPU (see MarginalEdges)
    stat_chains: int = None          # how many chains the device statistics above (summary_device, prediction, waic, loo, loo_predictive) cover: 1 (chain 1's window), or
                                     # every chain of the fit with pool_chains=True; None when the fit computed none
    marginal_prediction: "MarginalPrediction" = None   # filled on request (marginal_predict=True): the prediction of predict_X with gamma integrated out, computed on the GPU (see MarginalPredict)
    marginal_edge_cov: "MarginalEdgeCov" = None   # filled on request (marginal_edge_cov=...): the covariance of the edge coefficients with gamma integrated out, computed on the GPU (see MarginalEdgeCov)
    marginal_stacking: "MarginalStacking" = None   # filled on request (marginal_stack=True): the stacking weights of the chains from every chain's marginal PSIS-LOO and the LOO predictive checks of the stacked mixture (see MarginalStack)
    marginal_loo_predictive: "MarginalLOOPredictive" = None   # filled on request (marginal_loo_predict=True): the LOO predictive checks of the training rows under the marginal PSIS weights (see MarginalLOOPredict)


@dataclass
class BNRSummary:
    """gibbs.jl:39-43 (DataFrames replaced by dicts of columns)."""
    edge_coef: dict
    prob_nodes: dict
    ci_level: int

    def __str__(self):
        e, p = self.edge_coef, self.prob_nodes
        lines = ["", "Edge Coefficient Estimates (%d%% credible intervals)" % self.ci_level,
                 " node1 node2 estimate lower_bound upper_bound"]
        for i in range(len(e["node1"])):
            lines.append(" %5d %5d %8.3f %11.3f %11.3f" % (e["node1"][i], e["node2"][i], e["estimate"][i], e["lower_bound"][i], e["upper_bound"][i]))
        lines.append("Node Probabilities")
        lines += [" %.3f" % v for v in p["probability"]]
        return "\n".join(lines)


def _julia_round(x):
    """Julia's round(): half to even, like Python's round() on floats."""
    return int(round(x))


def _summary_ranks(nsamp, interval):
    """1-based positions in the sorted sample the reference reads (gibbs.jl:1224-1233)."""
    lower_bound = (100 - interval) / 200
    upper_bound = 1 - lower_bound
    lw, hi = _julia_round(nsamp * lower_bound), _julia_round(nsamp * upper_bound)
    if lw < 1 or hi > nsamp:
        # the reference indexes the sorted vector at 0 here and stops with a BoundsError
        raise IndexError("Summary: %d samples are too few for a %s%% interval" % (nsamp, interval))
    return lw, hi


def device_summary(chain, nburn, nsamp, interval=95):
    """Summary statistics of one chain's table computed on the GPU (bnr_chain_summary): only 3q + V numbers cross PCIe."""
    lw, hi = _summary_ranks(nsamp, interval)
    mean, lo, up, pxi = chain.summary(nburn + 1, nsamp, lw, hi)
    return dict(interval=interval, estimate=mean, lower_bound=lo, upper_bound=up, probability=pxi)


def Summary(results, interval=95, digits=3):
    """gibbs.jl:1214-1250.  Uses the statistics computed on the GPU when the fit carried them (summary_interval=...),
    otherwise sorts the fetched gamma trace on the host like the reference."""
    nburn, nsamp = results.burn_in, results.sampled
    total = nburn + nsamp
    dev = results.summary_device
    if dev is not None and dev["interval"] == interval:
        est, lo, up, pxi = dev["estimate"], dev["lower_bound"], dev["upper_bound"], dev["probability"]
    else:
        g = results.state["gamma"][nburn:total, :, 0]
        g_sorted = np.sort(g, axis=0)
        lw, hi = _summary_ranks(nsamp, interval)
        est, lo, up = g.mean(axis=0), g_sorted[lw - 1, :], g_sorted[hi - 1, :]
        pxi = results.state["xi"][nburn:total, :, 0].mean(axis=0)
    q = est.shape[0]
    V = int((-1 + math.sqrt(1 + 8 * q)) / 2)
    node1, node2 = [], []
    for k in range(1, V + 1):
        for l in range(k, V + 1):
            node1.append(k)
            node2.append(l)
    edge = dict(node1=np.array(node1), node2=np.array(node2), estimate=np.round(est, digits),
                lower_bound=np.round(lo, digits), upper_bound=np.round(up, digits))
    xi = dict(probability=np.round(pxi, digits))
    return BNRSummary(edge, xi, interval)


# ------------------------------------------------------------------------------------------ prediction and WAIC (additions to the reference)
@dataclass
class BNRPrediction:
    """Posterior of the mean response eta = mu + x.gamma of new rows (y = mu + X gamma + eps, gibbs.jl:270, 432, 566) over chain 1's window:
    estimate = posterior mean, lower_bound / upper_bound = the order statistics Summary uses for a ci_level% interval.  This is a credible
    interval of the MEAN response, not a predictive interval for a new observation (which would add eps ~ N(0, tau2)).  With observed
    responses: lpd = pointwise log predictive density log mean_s N(y_i | eta_is, tau2_s), elpd = its sum.
    With predict_observation (device_predict_pooled, Fit(..., predict_observation=True)): pred_lower_bound / pred_upper_bound = the same order
    statistics of draws of a NEW OBSERVATION eta_s + sqrt(tau2_s) z_s -- the ci_level% predictive interval -- and, with observed responses,
    pit = the probability integral transform mean_s Phi((y_i - eta_is) / sqrt(tau2_s)) of every y_i (uniform over rows when the predictive
    distribution is calibrated).  draws = the number of posterior draws behind the statistics (chains x window rows; None on the older paths)."""
    estimate: np.ndarray
    lower_bound: np.ndarray
    upper_bound: np.ndarray
    ci_level: int
    lpd: np.ndarray = None
    elpd: float = None
    pred_lower_bound: np.ndarray = None
    pred_upper_bound: np.ndarray = None
    pit: np.ndarray = None
    draws: int = None


def _prediction(mean, lo, hi, interval, lpd=None, digits=None, pred_lo=None, pred_hi=None, pit=None, draws=None):
    r = (lambda a: a) if digits is None else (lambda a: None if a is None else np.round(a, digits))
    return BNRPrediction(r(mean), r(lo), r(hi), interval, lpd, None if lpd is None else float(np.sum(lpd)), r(pred_lo), r(pred_hi), pit, draws)


def _new_rows(X_new, x_transform, q, y_new=None):
    """the new rows as an XInput (element type kept) after the checks every prediction path makes first: q columns, one y per row"""
    xi = X_new if isinstance(X_new, XInput) else XInput(X_new, x_transform)
    if xi.q != q:
        raise ValueError("the new rows have %d edge columns (V = %d), the fit %d" % (xi.q, xi.V, q))
    if y_new is not None and np.asarray(y_new).reshape(-1).shape[0] != xi.n:
        raise ValueError("y_new must have one entry per new row (%d), not %d" % (xi.n, np.asarray(y_new).size))
    return xi


def _dense_rows(xi):
    """an XInput as the n x q float64 matrix (host paths)"""
    if xi.from_matrices:
        return np.stack([lower_triangle(a) for a in xi.data]).astype(np.float64)
    return np.asarray(xi.data, dtype=np.float64)


def _host_eta(state, X, nburn, nsamp):
    """eta[i, s] = mu_s + X[i] . gamma_s over rows nburn+1 .. nburn+nsamp of a fetched table"""
    g = state["gamma"][nburn:nburn + nsamp, :, 0]
    mu = state["mu"][nburn:nburn + nsamp, 0, 0]
    return mu[None, :] + X @ g.T


def _host_loglik(state, X, y, nburn, nsamp):
    """ll[i, s] = log N(y_i | eta_is, tau2_s) over rows nburn+1 .. nburn+nsamp of a fetched table"""
    eta = _host_eta(state, X, nburn, nsamp)
    tau2 = state["tau2"][nburn:nburn + nsamp, 0, 0]
    return -0.5 * (math.log(2 * math.pi) + np.log(tau2))[None, :] - (np.asarray(y, dtype=np.float64).reshape(-1, 1) - eta) ** 2 / (2 * tau2[None, :])


def _host_pointwise(state, X, y, nburn, nsamp):
    """(lpd, pwaic) per row: log-mean-exp and the ddof-1 variance over the draws of log N(y_i | eta_is, tau2_s)"""
    ll = _host_loglik(state, X, y, nburn, nsamp)
    mx = ll.max(axis=1)
    return mx + np.log(np.mean(np.exp(ll - mx[:, None]), axis=1)), ll.var(axis=1, ddof=1)


def _waic_from_pointwise(lpd, pwaic):
    """WAIC as in Vehtari, Gelman & Gabry (2017) / ArviZ: elpd_waic = sum(lpd_i - p_waic_i), waic = -2 elpd_waic, se = sqrt(n Var_i(elpd_i))"""
    lpd, pwaic = np.asarray(lpd, dtype=np.float64), np.asarray(pwaic, dtype=np.float64)
    e = lpd - pwaic
    elpd = float(np.sum(e))
    return dict(elpd_waic=elpd, p_waic=float(np.sum(pwaic)), waic=-2.0 * elpd, se=float(math.sqrt(e.size * np.var(e))),
                lpd_i=lpd, p_waic_i=pwaic, elpd_waic_i=e)


def device_predict(chain, nburn, nsamp, X_new, y_new=None, interval=95, x_transform=False):
    """Predict's statistics for new rows computed on the GPU over rows nburn+1 .. nburn+nsamp of `chain` (bnr_chain_predict)."""
    xi = _new_rows(X_new, x_transform, chain.q, y_new)
    lw, hi = _summary_ranks(nsamp, interval)
    mean, lo, up, lpd, _pw = chain.predict(xi, nburn + 1, nsamp, lw, hi, y=y_new)
    return _prediction(mean, lo, up, interval, lpd)


def Predict(results, X_new=None, y_new=None, interval=95, x_transform=True, digits=None):
    """Posterior of the mean response mu + x.gamma of new rows over chain 1's sampled window (the rows Summary reads) -> BNRPrediction.
    X_new None: the prediction the fit computed on the GPU (Fit(..., predict_X=..., predict_y=..., predict_interval=...)).  X_new given: computed
    on the host from results.state (needs return_state=True); X_new in the fit's x_transform format (list of V x V matrices, or n x q)."""
    nburn, nsamp = results.burn_in, results.sampled
    if X_new is None:
        p = results.prediction
        if p is None:
            raise ValueError("the fit computed no prediction: pass X_new (with return_state=True) or fit with predict_X=...")
        if p.ci_level != interval:
            raise ValueError("the fit's prediction has a %s%% interval, not %s%%: pass X_new to recompute" % (p.ci_level, interval))
        return _prediction(p.estimate, p.lower_bound, p.upper_bound, p.ci_level, p.lpd, digits, p.pred_lower_bound, p.pred_upper_bound, p.pit, p.draws)
    if results.state is None:
        raise ValueError("Predict with X_new needs the state table (Fit(..., return_state=True)), or fit with predict_X=... to predict on the GPU")
    q = results.state["gamma"].shape[1]
    xi = _new_rows(X_new, x_transform, q, y_new)
    lw, hi = _summary_ranks(nsamp, interval)
    X = _dense_rows(xi)
    eta = _host_eta(results.state, X, nburn, nsamp)
    srt = np.sort(eta, axis=1)
    lpd = None if y_new is None else _host_pointwise(results.state, X, y_new, nburn, nsamp)[0]
    return _prediction(eta.mean(axis=1), srt[:, lw - 1], srt[:, hi - 1], interval, lpd, digits)


def WAIC(results, X=None, y=None, x_transform=True):
    """WAIC of the training rows over chain 1's sampled window (Vehtari, Gelman & Gabry 2017; names as ArviZ): dict with elpd_waic, p_waic,
    waic = -2 elpd_waic, se and the pointwise lpd_i, p_waic_i, elpd_waic_i.  Uses the GPU's numbers when the fit carried them (waic=True);
    otherwise the host formula over results.state with the training X, y passed in."""
    if results.waic is not None:
        return results.waic
    if results.state is None or X is None or y is None:
        raise ValueError("WAIC needs Fit(..., waic=True), or the state table (return_state=True) together with the training X and y")
    xi = _new_rows(X, x_transform, results.state["gamma"].shape[1], y)
    lpd, pw = _host_pointwise(results.state, _dense_rows(xi), y, results.burn_in, results.sampled)
    return _waic_from_pointwise(lpd, pw)


# ------------------------------------------------------------------------------------------ PSIS-LOO (an addition to the reference)
# The host restatement of what k_psis computes (include/bnr_hip.h, bnr_chain_loo), pinned to loo 2.x (psis.R, gpdfit.R):
# the fallback of LOO over a fetched table, and the yardstick of the GPU tests.
def _tail_length(S, r_eff):
    """loo's n_pareto: M = ceil(min(0.2 S, 3 sqrt(S / r_eff)))"""
    return int(math.ceil(min(0.2 * S, 3.0 * math.sqrt(S / r_eff))))


def _logsumexp(a):
    m = np.max(a)
    if not np.isfinite(m):
        return float(m)
    return float(m + np.log(np.sum(np.exp(a - m))))


def _gpdfit(x):
    """loo's gpdfit on ascending x: the generalized Pareto fit of Zhang & Stephens (2009) with the weakly informative prior -> (k, sigma);
    k is the shape after the prior adjustment (k M + 5) / (M + 10), +inf when it is NaN"""
    N = x.size
    mg = 30 + int(math.floor(math.sqrt(N)))
    jj = np.arange(1, mg + 1, dtype=np.float64)
    xstar = x[int(math.floor(N / 4 + 0.5)) - 1]
    with np.errstate(all="ignore"):
        theta = 1.0 / x[N - 1] + (1.0 - np.sqrt(mg / (jj - 0.5))) / 3.0 / xstar
        kk = np.log1p(-theta[:, None] * x[None, :]).mean(axis=1)
        l_theta = N * (np.log(-theta / kk) - kk - 1.0)
        jm = int(np.argmax(l_theta))                       # matrixStats' logSumExp: max + log1p(sum over the other points)
        lse = l_theta[jm] + np.log1p(np.sum(np.exp(np.delete(l_theta, jm) - l_theta[jm])))
        theta_hat = np.sum(theta * np.exp(l_theta - lse))
        k = np.mean(np.log1p(-theta_hat * x))
        sigma = -k / theta_hat
        k = k * N / (N + 10) + 10 * 0.5 / (N + 10)
    return (math.inf if math.isnan(k) else float(k)), float(sigma)


def _psis_row(ll, M):
    """loo's do_psis_i + pointwise_loo_calcs for one row of log-likelihood draws with tail length M -> (lpd, elpd_loo, pareto_k)"""
    S = ll.size
    with np.errstate(all="ignore"):
        mx = np.max(ll)
        lpd = float(mx + np.log(np.sum(np.exp(ll - mx)) / S))
    if not np.all(np.isfinite(ll)):
        return lpd, math.nan, math.inf
    r = -ll
    lw = r - np.max(r)
    k = math.inf
    if M >= 5:
        order = np.argsort(lw, kind="stable")
        tail = order[S - M:]
        lw_tail = lw[tail]
        if not abs(lw_tail[-1] - lw_tail[0]) < np.finfo(np.float64).eps / 100:
            ec = math.exp(lw[order[S - M - 1]])
            k, sigma = _gpdfit(np.exp(lw_tail) - ec)
            if math.isfinite(k):
                p = (np.arange(1, M + 1) - 0.5) / M
                with np.errstate(all="ignore"):
                    q = np.full(M, np.nan) if (math.isnan(sigma) or sigma <= 0) else sigma * np.expm1(-k * np.log1p(-p)) / k
                    lw[tail] = np.log(q + ec)
    lw = np.where(lw > 0, 0.0, lw)                         # truncation at the largest raw weight (a NaN stays NaN)
    return lpd, _logsumexp(lw + ll) - _logsumexp(lw), float(k)


def _psis_host(loglik, r_eff=None):
    """(lpd, elpd_loo, pareto_k) of every row of an m x S log-likelihood matrix, on the host"""
    ll = np.asarray(loglik, dtype=np.float64)
    if ll.ndim != 2 or ll.shape[0] < 1 or ll.shape[1] < 1:
        raise ValueError("loglik must be an m x S matrix (rows x draws) with m, S >= 1")
    m, S = ll.shape
    r = _capi.r_eff_array(r_eff, m)
    out = np.empty((3, m))
    for i in range(m):
        out[:, i] = _psis_row(ll[i], _tail_length(S, 1.0 if r is None else r[i]))
    return out[0], out[1], out[2]


def _loo_from_pointwise(lpd, elpd_i, pareto_k, S):
    """LOO totals with the conventions of WAIC: elpd_loo = sum elpd_i, p_loo = sum(lpd_i - elpd_i), looic = -2 elpd_loo,
    se = sqrt(n Var_i(elpd_i)) (ddof 0); the k-hat threshold min(1 - 1/log10(S), 0.7) of loo 2.x and the count of rows above it"""
    lpd, e, k = (np.asarray(a, dtype=np.float64) for a in (lpd, elpd_i, pareto_k))
    p = lpd - e
    elpd = float(np.sum(e))
    thr = -math.inf if S == 1 else min(1.0 - 1.0 / math.log10(S), 0.7)
    return dict(elpd_loo=elpd, p_loo=float(np.sum(p)), looic=-2.0 * elpd, se=float(math.sqrt(e.size * np.var(e))), elpd_loo_i=e,
                p_loo_i=p, lpd_i=lpd, pareto_k=k, khat_threshold=thr, n_high_k=int(np.sum(k > thr)))


def psis_loo(loglik, r_eff=None, device=None):
    """PSIS-LOO of an m x S log-likelihood matrix (rows x draws) on the GPU (bnr_psis_loo) -> the dict of LOO.  r_eff: None (1), a scalar,
    or one relative efficiency per row."""
    lpd, e, k = _capi.psis_loo_raw(loglik, r_eff, 0 if device is None else int(device))
    return _loo_from_pointwise(lpd, e, k, np.shape(loglik)[1])


def LOO(results, X=None, y=None, x_transform=True, r_eff=None):
    """PSIS-LOO cross-validation of the training rows over chain 1's sampled window (Vehtari, Gelman & Gabry 2017, as loo 2.x): dict with
    elpd_loo, p_loo, looic = -2 elpd_loo, se, the pointwise elpd_loo_i, p_loo_i, lpd_i, pareto_k, and khat_threshold / n_high_k (the rows
    whose estimate is not to be trusted).  Uses the GPU's numbers when the fit carried them (loo=True) and no r_eff is passed; otherwise the
    host restatement over results.state with the training X, y passed in."""
    if results.loo is not None and r_eff is None:
        return results.loo
    if results.state is None or X is None or y is None:
        raise ValueError("LOO needs Fit(..., loo=True), or the state table (return_state=True) together with the training X and y")
    xi = _new_rows(X, x_transform, results.state["gamma"].shape[1], y)
    ll = _host_loglik(results.state, _dense_rows(xi), y, results.burn_in, results.sampled)
    return _loo_from_pointwise(*_psis_host(ll, r_eff), results.sampled)


# ------------------------------------------------------------------------------------------ rank-normalised convergence diagnostics (additions)
# R-hat, bulk / tail effective sample size and MCSE of Vehtari, Gelman, Simpson, Carpenter, Buerkner (2021) as `posterior` 1.x computes them
# (rhat, ess_bulk, ess_tail, ess_mean, mcse_mean), over the pooled window of the chains of one device (include/bnr_hip.h, ABI 12).  One
# deviation: rhat = fmax(rhat_bulk, rhat_tail) is NaN only when both are -- binary xi columns often fold to a constant, and `posterior`'s max
# would turn the whole answer into NA there.  ESS figures equal `posterior`'s whenever Geyer's sequence ends before max_lag.
RANK_DIAG_FIELDS = _capi.RANK_DIAG_FIELDS


@dataclass
class RankDiagnostics:
    """Per parameter, gamma (q) and xi (V) apart: rhat = fmax(rhat_bulk, rhat_tail), rhat_bulk (split-R-hat of the normal scores z of the
    ranks), rhat_tail (the same for |x - median|), ess_bulk (on z), ess_tail (the smaller ESS of the 5 % and 95 % indicators), ess_mean (on x),
    mcse_mean = sd / sqrt(ess_mean).  draws: the ranked split-chain draws 2 chains (nsamp // 2); max_lag: where Geyer's sequence is cut.
    NaN throughout for a parameter with a non-finite draw or with all draws equal."""
    rhat_gamma: np.ndarray
    rhat_xi: np.ndarray
    rhat_bulk_gamma: np.ndarray
    rhat_bulk_xi: np.ndarray
    rhat_tail_gamma: np.ndarray
    rhat_tail_xi: np.ndarray
    ess_bulk_gamma: np.ndarray
    ess_bulk_xi: np.ndarray
    ess_tail_gamma: np.ndarray
    ess_tail_xi: np.ndarray
    ess_mean_gamma: np.ndarray
    ess_mean_xi: np.ndarray
    mcse_mean_gamma: np.ndarray
    mcse_mean_xi: np.ndarray
    draws: int
    chains: int
    max_lag: int

    def full(self, name):
        """field `name` ("rhat", or one of RANK_DIAG_FIELDS) of all q + V parameters, gamma first"""
        return np.concatenate([getattr(self, name + "_gamma"), getattr(self, name + "_xi")])


def _rank_lag(nsamp, max_lag):
    """the lag window of the rank diagnostics (default min(250, nsamp // 4), as ChainSet.ess) with the library's checks as ValueErrors"""
    nsamp = int(nsamp)
    max_lag = min(250, nsamp // 4) if max_lag is None else int(max_lag)
    if nsamp < 8:
        raise ValueError("the rank diagnostics need nsamp >= 8, not %d" % nsamp)
    if not (2 <= max_lag <= nsamp // 2):
        raise ValueError("need 2 <= max_lag <= nsamp // 2, not max_lag = %d with nsamp = %d" % (max_lag, nsamp))
    return max_lag


def _rank_diagnostics(q, fields, nchains, nsamp, max_lag):
    """RankDiagnostics from the six arrays of q + V values in the order of RANK_DIAG_FIELDS"""
    f = dict(zip(RANK_DIAG_FIELDS, fields))
    f["rhat"] = np.fmax(f["rhat_bulk"], f["rhat_tail"])
    kw = {}
    for k, v in f.items():
        kw[k + "_gamma"], kw[k + "_xi"] = v[:q].copy(), v[q:].copy()
    return RankDiagnostics(draws=2 * nchains * (nsamp // 2), chains=nchains, max_lag=max_lag, **kw)


def device_rank_diagnostics(chains, nburn, nsamp, max_lag=None):
    """The rank-normalised diagnostics over the pooled windows nburn+1 .. nburn+nsamp of live chains, on the device (bnr_chains_rank_diag): only
    6 (q + V) numbers leave the GPU's side of the call"""
    chains = list(chains)
    max_lag = _rank_lag(nsamp, max_lag)
    out = _capi.pooled_rank_diag(chains, nburn + 1, nsamp, max_lag)
    return _rank_diagnostics(chains[0].q, out, len(chains), nsamp, max_lag)


def _average_ranks(x):
    """average ranks (1-based; ties share the mean of their positions, -0 ties with +0) and the sorted values of a NaN-free vector"""
    n = x.size
    order = np.argsort(x, kind="stable")
    xs = x[order]
    head = np.ones(n, dtype=bool)
    head[1:] = xs[1:] != xs[:-1]
    starts = np.flatnonzero(head)
    ends = np.append(starts[1:], n)
    run = np.cumsum(head) - 1
    r = np.empty(n)
    r[order] = (starts[run] + ends[run] + 1) * 0.5
    return r, xs


def _z_scale(x):
    """the normal scores of the ranks of a NaN-free vector, Phi^-1 by the library's own routine (one call per distinct rank)"""
    r, xs = _average_ranks(x)
    ur, inv = np.unique(r, return_inverse=True)
    return _capi.host_ndtri((ur - 0.375) / (x.size + 0.25))[inv], xs


def _split_message(series, L):
    """k_acov's messages of series (m, h, P) -- m = 2 C split chains in the order chain 0 first half, chain 0 second half, chain 1 ... -- as
    bnr_ess_from_stats takes them: (C, 2 (2 + L) P), per half the mean, the variance (ddof 1) and the autocovariances at lags 0 .. L-1 (1 / h)"""
    m, h, P = series.shape
    out = np.empty((m, 2 + L, P))
    mean = series.mean(axis=1)
    c = series - mean[:, None, :]
    out[:, 0] = mean
    for t in range(L):
        out[:, 2 + t] = (c[:, :h - t] * c[:, t:]).sum(axis=1) / h
    out[:, 1] = out[:, 2] * h / (h - 1)
    return out.reshape(m // 2, 2 * (2 + L) * P)


def _split_rhat(msg, C, L, P, h):
    """sqrt(((h-1)/h W + B) / W) from the messages: W the mean of the 2 C variances, B the variance (ddof 1) of the 2 C means"""
    st = msg.reshape(2 * C, 2 + L, P)
    W = st[:, 1].mean(axis=0)
    B = st[:, 0].var(axis=0, ddof=1)
    with np.errstate(all="ignore"):
        return np.sqrt(((h - 1.0) / h * W + B) / W)


def _host_rank_diagnostics(tables, nburn, nsamp, max_lag=None):
    """device_rank_diagnostics restated in numpy over the fetched tables of the same chains (Phi^-1 through _capi.host_ndtri, Geyer's sequence
    through the library's host routine bnr_ess_from_stats): the fallback of users who hold the tables, and the yardstick of the GPU tests"""
    tables = list(tables)
    if not tables:
        raise ValueError("need at least one table")
    L = _rank_lag(nsamp, max_lag)
    C, h = len(tables), nsamp // 2
    q = tables[0]["gamma"].shape[1]
    halves = []
    for t in tables:
        w = np.concatenate([t["gamma"][nburn:nburn + nsamp, :, 0], t["xi"][nburn:nburn + nsamp, :, 0]], axis=1)
        halves += [w[:h], w[nsamp - h:]]
    X = np.stack(halves)                                 # (2 C, h, q + V)
    m, _, P = X.shape
    n = m * h
    flat = X.reshape(n, P)
    ok = np.isfinite(flat).all(axis=0) & (flat != flat[0]).any(axis=0)
    Z, F, I05, I95, XC = (np.zeros_like(flat) for _ in range(5))
    fold_ok = np.zeros(P, dtype=bool)
    k05, k95 = int(np.floor((n - 1) * 0.05)) + 1, int(np.floor((n - 1) * 0.95)) + 1
    for p in np.flatnonzero(ok):
        x = flat[:, p]
        Z[:, p], xs = _z_scale(x)
        I05[:, p], I95[:, p] = x <= xs[k05 - 1], x <= xs[k95 - 1]
        XC[:, p] = x - (xs[n // 2 - 1] + xs[n // 2]) / 2.0            # x about its median: ess_mean and mcse_mean are shift-invariant, and
        f = np.abs(XC[:, p])                                         # the split-chain means of a column like 1e8 + N(0, 1) keep their digits
        fold_ok[p] = np.isfinite(f).all() and (f != f[0]).any()
        if fold_ok[p]:
            F[:, p] = _z_scale(f)[0]
    shape = (m, h, P)
    mz, m05, m95, mx = (_split_message(a.reshape(shape), L) for a in (Z, I05, I95, XC))
    mf = _split_message(F.reshape(shape), 1)
    nan = np.full(P, np.nan)
    rhat_bulk = np.where(ok, _split_rhat(mz, C, L, P, h), nan)
    rhat_tail = np.where(ok & fold_ok, _split_rhat(mf, C, 1, P, h), nan)
    ess = [_capi.ess_from_stats(a, nsamp, L) for a in (mz, m05, m95, mx)]
    ess_bulk = np.where(ok, ess[0], nan)
    ess_tail = np.where(ok & ~np.isnan(ess[1]) & ~np.isnan(ess[2]), np.minimum(ess[1], ess[2]), nan)
    ess_mean = np.where(ok, ess[3], nan)
    sx = mx.reshape(m, 2 + L, P)
    mm = sx[:, 0].mean(axis=0)
    sd2 = ((h - 1.0) * sx[:, 1].sum(axis=0) + h * ((sx[:, 0] - mm) ** 2).sum(axis=0)) / (n - 1.0)
    with np.errstate(all="ignore"):
        mcse = np.where(ok, np.sqrt(sd2) / np.sqrt(ess_mean), nan)
    return _rank_diagnostics(q, (rhat_bulk, rhat_tail, ess_bulk, ess_tail, ess_mean, mcse), C, nsamp, L)


def rank_normalize(x, device=None):
    """Average ranks and normal scores of every row of an m x S matrix (rows x draws), each row ranked on its own, on the GPU
    (bnr_rank_normalize): dict with ranks (ties share the mean of their positions) and z = Phi^-1((ranks - 3/8) / (S + 1/4)).  +-Inf rank as
    numbers; a row that holds a NaN is NaN everywhere.  A vector is taken as one row."""
    a = np.asarray(x, dtype=np.float64)
    r, z = _capi.rank_normalize_raw(a.reshape(1, -1) if a.ndim == 1 else a, 0 if device is None else int(device))
    return dict(ranks=r.reshape(a.shape), z=z.reshape(a.shape))


def RankDiagnose(results, max_lag=None):
    """The rank-normalised diagnostics of a fit -> RankDiagnostics.  Uses the GPU's numbers when the fit carried them (rank_diagnostics=True:
    every chain of the fit), otherwise restates them on the host over results.state (needs return_state=True; chain 1 alone)."""
    if results.rank_diag is not None and (max_lag is None or int(max_lag) == results.rank_diag.max_lag):
        return results.rank_diag
    if results.state is None:
        raise ValueError("RankDiagnose needs Fit(..., rank_diagnostics=True), or the state table (return_state=True)")
    return _host_rank_diagnostics([results.state], results.burn_in, results.sampled, max_lag)


# ------------------------------------------------------------------------------------------ highest-density intervals and edge selection (additions)
# Per parameter over the pooled window of the chains of one device (include/bnr_hip.h, ABI 13): the highest-density interval of the sample as
# ArviZ's hdi and R's HDInterval::hdi compute it (the shortest window of floor(prob n) + 1 consecutive order statistics, the first among equal
# widths), the median, and the sign probabilities P(x > 0), P(x < 0) as exact shares of the draws.  From them the local false sign rate of every
# edge, lfsr = 1 - max(p_pos, p_neg) (Stephens 2017), and the largest set of edges whose mean lfsr -- the expected share of wrongly signed
# edges in the set -- stays within `fdr`.
def _host_hdi(x, probs):
    """bnr_hdi restated in numpy for the rows of an m x S matrix (a vector is one row): dict of lower / upper (nprob, m), median, p_pos, p_neg
    (m,).  The device's conventions: -0 counts and is reported as +0; a row with a NaN is NaN throughout; a row with an infinite draw is NaN in
    lower, upper and median.  The fallback over fetched tables and the yardstick of the GPU tests."""
    a = np.asarray(x, dtype=np.float64)
    a = a.reshape(1, -1) if a.ndim == 1 else a
    if a.ndim != 2 or a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError("x must be an m x S matrix (rows x draws) with m, S >= 1")
    pr = _capi.hdi_probs(probs)
    m, n = a.shape
    lower, upper = np.full((pr.size, m), np.nan), np.full((pr.size, m), np.nan)
    median, p_pos, p_neg = np.full(m, np.nan), np.full(m, np.nan), np.full(m, np.nan)
    for i in range(m):
        row = a[i]
        if np.isnan(row).any():
            continue
        p_pos[i], p_neg[i] = np.count_nonzero(row > 0) / n, np.count_nonzero(row < 0) / n
        if np.isinf(row).any():
            continue
        xs = np.sort(row + 0.0)                                      # (-0 + 0 = +0)
        median[i] = (xs[n // 2 - 1] + xs[n // 2]) / 2.0 if n >= 2 else xs[0]
        for k, prob in enumerate(pr):
            w = min(int(np.floor(prob * n)), n - 1)
            j = int(np.argmin(xs[w:] - xs[:n - w]))
            lower[k, i], upper[k, i] = xs[j], xs[j + w]
    return dict(lower=lower, upper=upper, median=median, p_pos=p_pos, p_neg=p_neg)


def hdi(x, prob=0.95, device=None):
    """Highest-density intervals of every row of an m x S matrix (rows x draws), each row on its own, on the GPU (bnr_hdi): dict with lower and
    upper (the shortest interval holding floor(prob S) + 1 consecutive order statistics: ArviZ's hdi for a unimodal sample), median, p_pos and
    p_neg (the shares of draws above and below zero).  prob: one level, or up to 8 -- lower / upper then get a leading axis of levels.  A row
    with a NaN is NaN throughout; one with an infinite draw is NaN in lower, upper and median.  A vector is taken as one row."""
    a = np.asarray(x, dtype=np.float64)
    out = dict(zip(_capi.HDI_FIELDS, _capi.hdi_raw(a.reshape(1, -1) if a.ndim == 1 else a, prob, 0 if device is None else int(device))))
    lead = () if np.ndim(prob) == 0 else (-1,)
    tail = a.shape[:-1]
    for k in ("lower", "upper"):
        out[k] = out[k].reshape(lead + tail)
    for k in ("median", "p_pos", "p_neg"):
        out[k] = out[k].reshape(tail)
    return out


@dataclass
class EdgeSelection:
    """Per edge (q, in Summary's order): node1, node2, estimate (the posterior median), hdi_lower / hdi_upper (the hdi_prob highest-density
    interval), p_pos / p_neg (the shares of draws above / below zero), lfsr = 1 - max(p_pos, p_neg) (the local false sign rate),
    hdi_excludes_zero, selected (the largest set of edges whose mean lfsr is at most fdr).  Per node (V): xi_estimate, xi_hdi_lower,
    xi_hdi_upper and prob_nodes (the share of draws with xi = 1).  expected_fsr: the mean lfsr of the selected edges (0 when none is); draws:
    the pooled draws per parameter."""
    node1: np.ndarray
    node2: np.ndarray
    estimate: np.ndarray
    hdi_lower: np.ndarray
    hdi_upper: np.ndarray
    p_pos: np.ndarray
    p_neg: np.ndarray
    lfsr: np.ndarray
    hdi_excludes_zero: np.ndarray
    selected: np.ndarray
    xi_estimate: np.ndarray
    xi_hdi_lower: np.ndarray
    xi_hdi_upper: np.ndarray
    prob_nodes: np.ndarray
    hdi_prob: float
    fdr: float
    n_selected: int
    expected_fsr: float
    chains: int
    draws: int


def _edge_levels(hdi_prob, fdr):
    """(hdi_prob, fdr) as floats; ValueError unless 0 < hdi_prob < 1 and 0 <= fdr <= 1"""
    hdi_prob, fdr = float(hdi_prob), float(fdr)
    if not (0.0 < hdi_prob < 1.0):
        raise ValueError("need 0 < hdi_prob < 1, not %r" % hdi_prob)
    if not (0.0 <= fdr <= 1.0):
        raise ValueError("need 0 <= fdr <= 1, not %r" % fdr)
    return hdi_prob, fdr


def _select_by_lfsr(lfsr, fdr):
    """(selected, expected_fsr): the edges in the order of their lfsr (stable: ties by edge index), the longest prefix whose running mean of
    lfsr is at most fdr; expected_fsr is that mean, 0.0 when nothing is selected.  An edge whose lfsr is NaN is never selected."""
    lfsr = np.asarray(lfsr, dtype=np.float64)
    sel = np.zeros(lfsr.size, dtype=bool)
    cand = np.flatnonzero(~np.isnan(lfsr))
    order = cand[np.argsort(lfsr[cand], kind="stable")]
    if order.size == 0:
        return sel, 0.0
    run = np.cumsum(lfsr[order]) / np.arange(1, order.size + 1)
    ok = np.flatnonzero(run <= fdr)
    if ok.size == 0:
        return sel, 0.0
    k = int(ok[-1]) + 1                                              # (the running mean of a sorted vector never decreases: a prefix)
    sel[order[:k]] = True
    return sel, float(run[k - 1])


def _edge_selection(q, fields, hdi_prob, fdr, nchains, draws):
    """EdgeSelection from the five arrays of HDI_FIELDS over q + V parameters at one level"""
    lower, upper, median, p_pos, p_neg = (np.asarray(f, dtype=np.float64).reshape(-1) for f in fields)
    V = lower.size - q
    node1 = np.concatenate([np.full(V - k + 1, k) for k in range(1, V + 1)])
    node2 = np.concatenate([np.arange(k, V + 1) for k in range(1, V + 1)])
    lfsr = 1.0 - np.maximum(p_pos[:q], p_neg[:q])                    # (NaN where the shares are)
    selected, efsr = _select_by_lfsr(lfsr, fdr)
    return EdgeSelection(node1=node1, node2=node2, estimate=median[:q].copy(), hdi_lower=lower[:q].copy(), hdi_upper=upper[:q].copy(),
                         p_pos=p_pos[:q].copy(), p_neg=p_neg[:q].copy(), lfsr=lfsr, hdi_excludes_zero=(lower[:q] > 0) | (upper[:q] < 0),
                         selected=selected, xi_estimate=median[q:].copy(), xi_hdi_lower=lower[q:].copy(), xi_hdi_upper=upper[q:].copy(),
                         prob_nodes=p_pos[q:].copy(), hdi_prob=hdi_prob, fdr=fdr, n_selected=int(selected.sum()), expected_fsr=efsr,
                         chains=nchains, draws=draws)


def device_edge_selection(chains, nburn, nsamp, hdi_prob=0.95, fdr=0.05):
    """The HDIs, sign probabilities and selected edges over the pooled windows nburn+1 .. nburn+nsamp of live chains, on the device
    (bnr_chains_hdi): only 5 (q + V) numbers leave the GPU's side of the call"""
    chains = list(chains)
    hdi_prob, fdr = _edge_levels(hdi_prob, fdr)
    out = _capi.pooled_hdi(chains, nburn + 1, nsamp, hdi_prob)
    return _edge_selection(chains[0].q, out, hdi_prob, fdr, len(chains), len(chains) * int(nsamp))


def _host_edge_selection(tables, nburn, nsamp, hdi_prob=0.95, fdr=0.05):
    """device_edge_selection restated in numpy over the fetched tables of the same chains (_host_hdi on the pooled windows)"""
    tables = list(tables)
    if not tables:
        raise ValueError("need at least one table")
    hdi_prob, fdr = _edge_levels(hdi_prob, fdr)
    q = tables[0]["gamma"].shape[1]
    w = np.concatenate([np.concatenate([t["gamma"][nburn:nburn + nsamp, :, 0], t["xi"][nburn:nburn + nsamp, :, 0]], axis=1) for t in tables], axis=0)
    h = _host_hdi(w.T, hdi_prob)
    return _edge_selection(q, [h[f] for f in _capi.HDI_FIELDS], hdi_prob, fdr, len(tables), w.shape[0])


def EdgeSelect(results, hdi_prob=None, fdr=None):
    """The edge selection of a fit -> EdgeSelection.  Uses the GPU's numbers when the fit carried them (edge_selection=True: every chain of
    the fit; another fdr re-applies the rule to them), otherwise restates them on the host over results.state (needs return_state=True; chain
    1 alone; defaults hdi_prob = 0.95, fdr = 0.05)."""
    es = results.edge_selection
    if es is not None and (hdi_prob is None or float(hdi_prob) == es.hdi_prob):
        if fdr is None or float(fdr) == es.fdr:
            return es
        _, fdr = _edge_levels(es.hdi_prob, fdr)
        selected, efsr = _select_by_lfsr(es.lfsr, fdr)
        return dataclasses.replace(es, fdr=fdr, selected=selected, n_selected=int(selected.sum()), expected_fsr=efsr)
    if results.state is None:
        raise ValueError("EdgeSelect needs Fit(..., edge_selection=True), or the state table (return_state=True)")
    return _host_edge_selection([results.state], results.burn_in, results.sampled, 0.95 if hdi_prob is None else hdi_prob, 0.05 if fdr is None else fdr)


# ------------------------------------------------------------------------------------------ joint posterior of the node indicators (additions)
# Over the pooled window of the chains of one device (include/bnr_hip.h, ABI 15), of the S x B matrix of indicators z (xi_v != 0 per node, or
# lambda_r != 0 per latent dimension): the marginal and pairwise inclusion shares, the distribution of the number of included indicators, the
# number of distinct rows and the most frequent ones.  Every number is an integer count, divided once by S; the indicator is x != 0, so -0 is
# excluded and a NaN counts as included.
def _host_inclusion(z, ntop):
    """bnr_inclusion restated in numpy for an S x B matrix (rows = draws; an entry != 0 is 1): dict of _capi.INCL_FIELDS -- prob (B,), joint
    (B, B), size_pmf (B + 1,), n_distinct, top_sets (ntop, W) uint64 words (bit k % 64 of word k // 64 is indicator k) and top_count (ntop,),
    most frequent first, ties by the row as an integer; zeros behind the n_distinct-th.  The fallback over fetched tables and the yardstick of
    the GPU tests."""
    a = np.asarray(z)
    if a.ndim != 2 or a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError("z must be an S x B matrix (draws x indicators) with S, B >= 1")
    ntop = int(ntop)
    if not 0 <= ntop <= 256:
        raise ValueError("need 0 <= ntop <= 256, not %d" % ntop)
    b = a != 0
    S, B = b.shape
    W = (B + 63) // 64
    zi = b.astype(np.int64)
    padded = np.zeros((S, 64 * W), dtype=np.uint8)
    padded[:, :B] = b
    words = np.packbits(padded, axis=1, bitorder="little").view("<u8").astype(np.uint64).reshape(S, W)
    uniq, counts = np.unique(words[:, ::-1], axis=0, return_counts=True)   # most significant word first: ascending as integers
    order = np.argsort(-counts, kind="stable")[:ntop]
    top_sets, top_count = np.zeros((ntop, W), dtype=np.uint64), np.zeros(ntop, dtype=np.int64)
    top_sets[:order.size] = uniq[order][:, ::-1]
    top_count[:order.size] = counts[order]
    return dict(prob=zi.sum(axis=0) / float(S), joint=(zi.T @ zi) / float(S), size_pmf=np.bincount(zi.sum(axis=1), minlength=B + 1) / float(S),
                n_distinct=int(uniq.shape[0]), top_sets=top_sets, top_count=top_count)


def inclusion(z, ntop=10, device=None):
    """The joint summary of any S x B matrix of 0/1 indicators (rows = draws), on the GPU (bnr_inclusion): dict with prob (B,), joint (B, B),
    size_pmf (B + 1,), n_distinct, and the ntop most frequent rows as top_sets (ntop, W) uint64 words -- bit k % 64 of word k // 64 is
    indicator k -- with their counts top_count (zeros behind the n_distinct-th).  ntop = 0: no rows are returned."""
    fields = _capi.INCL_FIELDS if int(ntop) else _capi.INCL_FIELDS[:4]
    out = dict(zip(_capi.INCL_FIELDS, _capi.inclusion_raw(z, ntop, 0 if device is None else int(device), fields=fields)))
    return {k: v for k, v in out.items() if v is not None}


def _set_members(words, B):
    """the 1-based indices (as the reference numbers nodes) of the bits set in the W words of a pattern"""
    w = np.asarray(words, dtype=np.uint64).reshape(-1)
    k = np.arange(B)
    return (np.flatnonzero((w[k // 64] >> (k % 64).astype(np.uint64)) & np.uint64(1)) + 1).astype(np.int64)


_NODE_SETS_FIELDS = ("prob_nodes", "co_inclusion", "size_pmf", "size_mean", "size_mode", "n_distinct", "top_sets", "top_prob", "map_model",
                     "median_model", "prob_active", "dim_pmf", "dim_mean", "chains", "draws")


class NodeSets:
    """The joint posterior of the node indicators of a fit.  Per node (V): prob_nodes (the share of draws with xi_v = 1), co_inclusion (V x V:
    the share of draws that select both nodes; its diagonal is prob_nodes).  size_pmf (V + 1: the distribution of the number of selected
    nodes), size_mean, size_mode.  n_distinct: the number of distinct node sets among the draws; top_sets: the most frequent ones, each an
    array of 1-based node indices (as the reference numbers nodes), most probable first, ties by the set as an integer with node 1 the lowest
    bit; top_prob: their shares of the draws; map_model = top_sets[0]; median_model: the nodes with prob_nodes > 0.5.  Per latent dimension
    (R): prob_active (the share of draws with lambda_r != 0), dim_pmf (R + 1: the distribution of the number of active dimensions, the
    "effective dimensionality"), dim_mean.  chains, draws: what was pooled.

    NodeSets(results, top_sets=None) is the accessor of a fit: the GPU's numbers when the fit carried them (node_sets=True: every chain of the
    fit; asking for more top sets than the fit kept is a ValueError, never another population), otherwise restated on the host over
    results.state (needs return_state=True; chain 1 alone; top_sets defaults to 10).  Without a Results, NodeSets(**fields) builds the record
    itself from exactly the fields above."""

    def __new__(cls, results=None, top_sets=None, **fields):
        if results is not None:
            return _node_sets_of(results, top_sets)
        return object.__new__(cls)

    def __init__(self, results=None, top_sets=None, **fields):
        if results is not None:                                          # (the accessor: __new__ returned a finished object)
            return
        fields["top_sets"] = top_sets                                    # (without a Results the keyword is the field of that name)
        if set(fields) != set(_NODE_SETS_FIELDS) or top_sets is None:
            raise TypeError("NodeSets takes a Results, or exactly the fields %r" % (_NODE_SETS_FIELDS,))
        self.__dict__.update(fields)

    def __repr__(self):
        return "NodeSets(chains=%d, draws=%d, n_distinct=%d, size_mean=%.3f, map_model=%s)" % (self.chains, self.draws, self.n_distinct, self.size_mean,
                                                                                               self.map_model.tolist())


def _node_sets_ntop(ntop):
    """the number of node sets a NodeSets reports: an int in 1 .. 256 (ValueError otherwise)"""
    if isinstance(ntop, bool) or int(ntop) != ntop or not 1 <= int(ntop) <= 256:
        raise ValueError("top_sets must be an integer between 1 and 256, not %r" % (ntop,))
    return int(ntop)


def _node_sets(xi, lam, nchains, draws):
    """NodeSets from the INCL_FIELDS of the node indicators (all six) and of the dimensions (prob, size_pmf)"""
    prob, joint, size_pmf, n_distinct, words, count = xi
    V = prob.size
    keep = min(int(n_distinct), count.size)
    tops = [_set_members(words[j], V) for j in range(keep)]
    return NodeSets(prob_nodes=prob, co_inclusion=joint, size_pmf=size_pmf, size_mean=float(np.arange(V + 1) @ size_pmf), size_mode=int(np.argmax(size_pmf)),
                    n_distinct=int(n_distinct), top_sets=tops, top_prob=count[:keep] / float(draws), map_model=tops[0],
                    median_model=(np.flatnonzero(prob > 0.5) + 1).astype(np.int64), prob_active=lam[0], dim_pmf=lam[2],
                    dim_mean=float(np.arange(lam[2].size) @ lam[2]), chains=nchains, draws=draws)


def device_node_sets(chains, nburn, nsamp, ntop=10):
    """The joint posterior of the node indicators and the active dimensions over the pooled windows nburn+1 .. nburn+nsamp of live chains, on
    the device (bnr_chains_inclusion, once for xi and once for lambda): V^2 + 2 V + R + ... numbers leave the GPU's side, not the traces"""
    chains = list(chains)
    ntop = _node_sets_ntop(ntop)
    xi = _capi.pooled_inclusion(chains, nburn + 1, nsamp, 0, ntop)
    lam = _capi.pooled_inclusion(chains, nburn + 1, nsamp, 1, 0, fields=("prob", "size_pmf"))
    return _node_sets(xi, lam, len(chains), len(chains) * int(nsamp))


def _host_node_sets(tables, nburn, nsamp, ntop=10):
    """device_node_sets restated in numpy over the fetched tables of the same chains (_host_inclusion on the pooled windows)"""
    tables = list(tables)
    if not tables:
        raise ValueError("need at least one table")
    ntop = _node_sets_ntop(ntop)
    zx = np.concatenate([t["xi"][nburn:nburn + nsamp, :, 0] for t in tables], axis=0)
    xi = _host_inclusion(zx, ntop)
    lam = _host_inclusion(np.concatenate([t["lam"][nburn:nburn + nsamp, :, 0] for t in tables], axis=0), 0)
    return _node_sets([xi[f] for f in _capi.INCL_FIELDS], [lam[f] for f in _capi.INCL_FIELDS], len(tables), zx.shape[0])


def _node_sets_of(results, top_sets=None):
    """NodeSets(results, top_sets): see NodeSets"""
    ns = results.node_sets
    if ns is not None:                                                   # what the fit carried, never another population in its place
        if top_sets is not None and _node_sets_ntop(top_sets) > len(ns.top_sets) and len(ns.top_sets) < ns.n_distinct:
            raise ValueError("top_sets=%d, but the fit kept its %d most probable node sets of %d: refit with Fit(..., node_sets=True, top_sets=%d)"
                             % (int(top_sets), len(ns.top_sets), ns.n_distinct, int(top_sets)))
        return ns
    if results.state is None:
        raise ValueError("NodeSets needs Fit(..., node_sets=True), or the state table (return_state=True)")
    return _host_node_sets([results.state], results.burn_in, results.sampled, 10 if top_sets is None else top_sets)


# ------------------------------------------------------------------------------------------ pooled chains, predictive intervals, PIT (additions)
# Statistics over the POOLED window of several chains of a fit (include/bnr_hip.h, bnr_chains_*): draw c nsamp + s is the s-th window row of the
# c-th chain.  The device_* functions take live Chain objects; the _host_pooled_* restatements take the fetched tables of the same chains: the
# fallback of users who hold the tables, and the yardstick of the GPU tests.  By construction they ARE the single-table formulas above applied
# to the row-concatenated windows (one table: to that table itself).
def _pool_tables(states, nburn, nsamp):
    """(table, nburn', S): the windows nburn+1 .. nburn+nsamp of the tables concatenated in order (columns gamma, mu, tau2, xi), as one table
    with nburn' = 0; a single table is passed through untouched"""
    states = list(states)
    if not states:
        raise ValueError("need at least one table")
    if len(states) == 1:
        return states[0], nburn, nsamp
    cat = {k: np.asfortranarray(np.concatenate([st[k][nburn:nburn + nsamp] for st in states], axis=0)) for k in ("gamma", "mu", "tau2", "xi")}
    return cat, 0, nsamp * len(states)


def _erfc(a):
    try:
        from scipy.special import erfc
        return erfc(a)
    except ImportError:
        return np.vectorize(math.erfc, otypes=[np.float64])(a)


def _host_pit(eta, tau2, y):
    """pit_i = mean_s Phi((y_i - eta_is) / sqrt(tau2_s)), Phi(z) = erfc(-z / sqrt 2) / 2"""
    z = (np.asarray(y, dtype=np.float64).reshape(-1, 1) - eta) / np.sqrt(tau2)[None, :]
    return np.mean(0.5 * _erfc(-z / math.sqrt(2.0)), axis=1)


def _host_pooled_summary(states, nburn, nsamp, interval=95):
    """device_summary_pooled's statistics from the fetched tables: the dict of device_summary"""
    t, nb, S = _pool_tables(states, nburn, nsamp)
    lw, hi = _summary_ranks(S, interval)
    g = t["gamma"][nb:nb + S, :, 0]
    srt = np.sort(g, axis=0)
    return dict(interval=interval, estimate=g.mean(axis=0), lower_bound=srt[lw - 1, :], upper_bound=srt[hi - 1, :],
                probability=t["xi"][nb:nb + S, :, 0].mean(axis=0))


def _host_pooled_predict(states, X_new, y_new=None, nburn=0, nsamp=None, interval=95, x_transform=False, pred_seed=None):
    """device_predict_pooled's BNRPrediction from the fetched tables.  pred_seed given: the predictive bounds from y~ = eta + sqrt(tau2) z with the
    device's own z (bnr_host_pred_noise) and, with y_new, the PIT."""
    t, nb, S = _pool_tables(states, nburn, nsamp)
    xi = _new_rows(X_new, x_transform, t["gamma"].shape[1], y_new)
    lw, hi = _summary_ranks(S, interval)
    X = _dense_rows(xi)
    eta = _host_eta(t, X, nb, S)
    srt = np.sort(eta, axis=1)
    lpd = None if y_new is None else _host_pointwise(t, X, y_new, nb, S)[0]
    plo = phi = pit = None
    if pred_seed is not None:
        tau2 = t["tau2"][nb:nb + S, 0, 0]
        ysrt = np.sort(eta + np.sqrt(tau2)[None, :] * _capi.host_pred_noise(pred_seed, 0, S, 0, xi.n), axis=1)
        plo, phi = ysrt[:, lw - 1], ysrt[:, hi - 1]
        if y_new is not None:
            pit = _host_pit(eta, tau2, y_new)
    return _prediction(eta.mean(axis=1), srt[:, lw - 1], srt[:, hi - 1], interval, lpd, None, plo, phi, pit, S)


def _host_pooled_pointwise(states, X, y, nburn, nsamp, x_transform=False):
    """(lpd, pwaic, pit) of the rows X, y over the pooled windows of the fetched tables"""
    t, nb, S = _pool_tables(states, nburn, nsamp)
    Xd = _dense_rows(_new_rows(X, x_transform, t["gamma"].shape[1], y))
    lpd, pw = _host_pointwise(t, Xd, y, nb, S)
    return lpd, pw, _host_pit(_host_eta(t, Xd, nb, S), t["tau2"][nb:nb + S, 0, 0], y)


def _host_pooled_waic(states, X, y, nburn, nsamp, x_transform=False):
    """WAIC's dict over the pooled windows of the fetched tables"""
    return _waic_from_pointwise(*_host_pooled_pointwise(states, X, y, nburn, nsamp, x_transform)[:2])


def _host_pooled_loo(states, X, y, nburn, nsamp, x_transform=False, r_eff=None):
    """LOO's dict over the pooled windows of the fetched tables"""
    t, nb, S = _pool_tables(states, nburn, nsamp)
    Xd = _dense_rows(_new_rows(X, x_transform, t["gamma"].shape[1], y))
    return _loo_from_pointwise(*_psis_host(_host_loglik(t, Xd, y, nb, S), r_eff), S)


def device_summary_pooled(chains, nburn, nsamp, interval=95):
    """device_summary over rows nburn+1 .. nburn+nsamp of ALL the chains listed, pooled (bnr_chains_summary)"""
    chains = list(chains)
    lw, hi = _summary_ranks(nsamp * len(chains), interval)
    mean, lo, up, pxi = _capi.pooled_summary(chains, nburn + 1, nsamp, lw, hi)
    return dict(interval=interval, estimate=mean, lower_bound=lo, upper_bound=up, probability=pxi)


def device_predict_pooled(chains, nburn, nsamp, X_new, y_new=None, interval=95, pred_seed=0, x_transform=False, predict_observation=True):
    """device_predict over rows nburn+1 .. nburn+nsamp of ALL the chains listed, pooled (bnr_chains_predict).  predict_observation adds the
    predictive interval of a new observation (noise keyed by pred_seed, the pooled draw and the row's index in X_new) and, with y_new, the PIT."""
    chains = list(chains)
    if not chains:
        raise ValueError("need at least one chain")
    xi = _new_rows(X_new, x_transform, chains[0].q, y_new)
    S = nsamp * len(chains)
    lw, hi = _summary_ranks(S, interval)
    mean, lo, up, lpd, _pw, plo, phi, pit = _capi.pooled_predict(chains, xi, nburn + 1, nsamp, lw, hi, y=y_new,
                                                                pred_seed=pred_seed if predict_observation else None,
                                                                pit=bool(predict_observation) and y_new is not None)
    return _prediction(mean, lo, up, interval, lpd, None, plo, phi, pit, S)


# ------------------------------------------------------------------------------------------ LOO predictive checks (an addition to the reference)
# The PSIS weights themselves and the leave-one-out posterior predictive of every training row (include/bnr_hip.h, bnr_chains_loo_predict;
# DESIGN.md section 8, "LOO predictive checks").  The host restatements are the fallback of LOOPredict over fetched tables and the yardstick of
# the GPU tests.
def _psis_weights_row(ll, M):
    """_psis_row with the weights kept -> (lpd, elpd_loo, pareto_k, lwn): lwn = the log weights after smoothing and truncation at 0, normalised
    (lw - logsumexp lw: loo's weights(normalize = TRUE, log = TRUE)); elpd_loo = log sum_s exp(lwn_s + l_s).  The tail is the M largest in
    (lw, draw index), position j of that order gets the j-th GPD quantile -- _psis_row's stable argsort.  A non-finite l: NaN weights."""
    S = ll.size
    with np.errstate(all="ignore"):
        mx = np.max(ll)
        lpd = float(mx + np.log(np.sum(np.exp(ll - mx)) / S))
    if not np.all(np.isfinite(ll)):
        return lpd, math.nan, math.inf, np.full(S, np.nan)
    r = -ll
    lw = r - np.max(r)
    k = math.inf
    if M >= 5:
        order = np.argsort(lw, kind="stable")
        tail = order[S - M:]
        lw_tail = lw[tail]
        if not abs(lw_tail[-1] - lw_tail[0]) < np.finfo(np.float64).eps / 100:
            ec = math.exp(lw[order[S - M - 1]])
            k, sigma = _gpdfit(np.exp(lw_tail) - ec)
            if math.isfinite(k):
                p = (np.arange(1, M + 1) - 0.5) / M
                with np.errstate(all="ignore"):
                    q = np.full(M, np.nan) if (math.isnan(sigma) or sigma <= 0) else sigma * np.expm1(-k * np.log1p(-p)) / k
                    lw[tail] = np.log(q + ec)
    lw = np.where(lw > 0, 0.0, lw)
    lz = _logsumexp(lw)
    return lpd, _logsumexp(lw + ll) - lz, float(k), lw - lz


def _psis_weights_host(loglik, r_eff=None):
    """(log_weights m x S, elpd_loo, pareto_k) of every row of an m x S log-likelihood matrix, on the host"""
    ll = np.asarray(loglik, dtype=np.float64)
    if ll.ndim != 2 or ll.shape[0] < 1 or ll.shape[1] < 1:
        raise ValueError("loglik must be an m x S matrix (rows x draws) with m, S >= 1")
    m, S = ll.shape
    r = _capi.r_eff_array(r_eff, m)
    lw, e, k = np.empty((m, S)), np.empty(m), np.empty(m)
    for i in range(m):
        _lpd, e[i], k[i], lw[i] = _psis_weights_row(ll[i], _tail_length(S, 1.0 if r is None else r[i]))
    return lw, e, k


def psis_weights(loglik, r_eff=None, device=None):
    """The PSIS weights of an m x S log-likelihood matrix (rows x draws) on the GPU (bnr_psis_weights): dict with log_weights (m x S, each row
    normalised: loo's weights(log = TRUE)), elpd_loo_i, pareto_k and khat_threshold / n_high_k.  r_eff as for psis_loo."""
    lw, e, k = _capi.psis_weights_raw(loglik, r_eff, 0 if device is None else int(device))
    S = lw.shape[1]
    thr = -math.inf if S == 1 else min(1.0 - 1.0 / math.log10(S), 0.7)
    return dict(log_weights=lw, elpd_loo_i=e, pareto_k=k, khat_threshold=thr, n_high_k=int(np.sum(k > thr)))


@dataclass
class LOOPredictive:
    """The leave-one-out posterior predictive of every training row, from the PSIS weights w_is over the `draws` posterior draws:
    loo_mean = sum_s w eta, loo_sd = the sd of a new observation of the row (sqrt(sum_s w (tau2 + eta^2) - loo_mean^2)), loo_pit =
    sum_s w Phi((y - eta) / sqrt(tau2)) (uniform over rows when the model is calibrated OUT of sample, which the in-sample PIT cannot show),
    loo_lower / loo_upper = the (1 - interval/100)/2- and 1 - (1 - interval/100)/2-quantile of the mixture CDF sum_s w Phi((t - eta) / sqrt(tau2))
    found by a bracketed root search -- the Rao-Blackwellised counterpart of the PIT, not loo's weighted sample quantile (.wquant).
    Totals over the rows with finite outputs: rmse_loo = sqrt(mean (y - loo_mean)^2), r2_loo = 1 - Var(y - loo_mean) / Var(y) (ddof 0),
    coverage = the share of y inside [loo_lower, loo_upper], ks = the Kolmogorov-Smirnov distance of loo_pit from U(0, 1); n_high_k = the
    rows whose pareto_k is above khat_threshold (their numbers are not to be trusted), as in LOO."""
    loo_mean: np.ndarray
    loo_sd: np.ndarray
    loo_pit: np.ndarray
    loo_lower: np.ndarray
    loo_upper: np.ndarray
    lpd_i: np.ndarray
    elpd_loo_i: np.ndarray
    pareto_k: np.ndarray
    rmse_loo: float
    r2_loo: float
    coverage: float
    ks: float
    interval: float
    draws: int
    khat_threshold: float
    n_high_k: int


def _loo_interval_probs(interval):
    p_lo = (1.0 - interval / 100.0) / 2.0
    return _capi.loo_probs(p_lo, 1.0 - p_lo)


def _ks_uniform(u):
    """the Kolmogorov-Smirnov distance of the sample u from U(0, 1)"""
    u = np.sort(np.asarray(u, dtype=np.float64))
    n = u.size
    if n == 0:
        return math.nan
    i = np.arange(1, n + 1)
    return float(max(np.max(i / n - u), np.max(u - (i - 1) / n)))


def _loo_predictive(y, lpd, elpd, k, mean, sd, pit, lower, upper, interval, S):
    """LOOPredictive from the pointwise arrays: the totals on the host over the rows whose outputs are all finite"""
    y = np.asarray(y, dtype=np.float64).reshape(-1)
    arrs = [np.asarray(a, dtype=np.float64) for a in (mean, sd, pit, lower, upper)]
    ok = np.all(np.isfinite(np.stack(arrs)), axis=0)
    res = (y - arrs[0])[ok]
    if res.size:
        rmse = float(math.sqrt(np.mean(res ** 2)))
        vy = float(np.var(y[ok]))
        r2 = 1.0 - float(np.var(res)) / vy if vy > 0 else math.nan
        cov = float(np.mean((y[ok] >= arrs[3][ok]) & (y[ok] <= arrs[4][ok])))
    else:
        rmse = r2 = cov = math.nan
    thr = -math.inf if S == 1 else min(1.0 - 1.0 / math.log10(S), 0.7)
    k = np.asarray(k, dtype=np.float64)
    return LOOPredictive(arrs[0], arrs[1], arrs[2], arrs[3], arrs[4], np.asarray(lpd, dtype=np.float64), np.asarray(elpd, dtype=np.float64), k,
                         rmse, r2, cov, _ks_uniform(arrs[2][ok]), interval, int(S), thr, int(np.sum(k > thr)))


def _loo_bracket_c(p_lo, p_hi):
    """the half-width of the quantile search's bracket in sds: the first c = 1, 1.5, 2, ... with Phi(-c) < min(p_lo, 1 - p_hi) / 2 (the library's loop)"""
    pm = 0.5 * min(p_lo, 1.0 - p_hi)
    c = 1.0
    while not 0.5 * math.erfc(c * 0.70710678118654752440) < pm and c < 40.0:
        c += 0.5
    return c


def _mixture_cdf(t, w, eta, sd):
    """F(t) = sum_s w_s Phi((t - eta_s) / sd_s)"""
    return float(np.sum(w * 0.5 * _erfc(-((t - eta) / sd) / math.sqrt(2.0))))


def _bisect_quantile(F, p, lo, hi):
    """the library's bisection: down to 2^-40 of the bracket, at most 64 halvings, the midpoint"""
    tol = (hi - lo) * 2.0 ** -40
    for _ in range(64):
        if not hi - lo > tol:
            break
        mid = 0.5 * (lo + hi)
        f = F(mid)
        if f != f:
            return math.nan
        if f < p:
            lo = mid
        else:
            hi = mid
    return 0.5 * (lo + hi)


def _mixture_quantile(p, w, eta, sd, c, solver=None):
    """the p-quantile of the mixture CDF from the bracket [min(eta - c sd), max(eta + c sd)] -> (t, bracket width): scipy.optimize.brentq when
    scipy is there (solver None) or asked for (solver="brentq"), else the library's bisection (solver="bisect")"""
    lo, hi = float(np.min(eta - c * sd)), float(np.max(eta + c * sd))
    width = hi - lo
    if not (np.all(np.isfinite(w)) and math.isfinite(width) and width > 0):
        return math.nan, width
    F = lambda t: _mixture_cdf(t, w, eta, sd)
    brentq = None
    if solver != "bisect":
        try:
            from scipy.optimize import brentq
        except ImportError:
            if solver == "brentq":
                raise
    if brentq is None:
        return _bisect_quantile(F, p, lo, hi), width
    return float(brentq(lambda t: F(t) - p, lo, hi, xtol=width * 2.0 ** -44, rtol=8.9e-16, maxiter=500)), width


def _loo_predict_rows(eta, tau2, y, lwn, p_lo, p_hi, solver=None):
    """(loo_mean, loo_sd, loo_pit, loo_lower, loo_upper, bracket width) per row from eta (n x S), tau2 (S), y (n) and the normalised log weights"""
    n = eta.shape[0]
    sd = np.sqrt(tau2)
    c = _loo_bracket_c(p_lo, p_hi)
    out = np.full((6, n), np.nan)
    for i in range(n):
        if not np.all(np.isfinite(lwn[i])):
            continue
        w = np.exp(lwn[i])
        m = float(np.sum(w * eta[i]))
        out[0, i] = m
        out[1, i] = math.sqrt(float(np.sum(w * (tau2 + eta[i] ** 2))) - m * m)
        out[2, i] = _mixture_cdf(y[i], w, eta[i], sd)
        out[3, i], out[5, i] = _mixture_quantile(p_lo, w, eta[i], sd, c, solver)
        out[4, i], _ = _mixture_quantile(p_hi, w, eta[i], sd, c, solver)
    return tuple(out)


def _host_loo_predict(states, X, y, nburn, nsamp, interval=95, x_transform=False, r_eff=None, solver=None):
    """device_loo_predict's LOOPredictive from the fetched tables of the chains, pooled in order"""
    t, nb, S = _pool_tables(states, nburn, nsamp)
    p_lo, p_hi = _loo_interval_probs(interval)
    Xd = _dense_rows(_new_rows(X, x_transform, t["gamma"].shape[1], y))
    yv = np.asarray(y, dtype=np.float64).reshape(-1)
    ll = _host_loglik(t, Xd, yv, nb, S)
    lpd = _psis_host(ll, r_eff)[0]
    lwn, e, k = _psis_weights_host(ll, r_eff)
    mean, sd, pit, lo, hi, _w = _loo_predict_rows(_host_eta(t, Xd, nb, S), t["tau2"][nb:nb + S, 0, 0], yv, lwn, p_lo, p_hi, solver)
    return _loo_predictive(yv, lpd, e, k, mean, sd, pit, lo, hi, interval, S)


def device_loo_predict(chains, y, nburn, nsamp, interval=95, r_eff=None):
    """The LOO predictive checks of the training rows over rows nburn+1 .. nburn+nsamp of ALL the chains listed, pooled, on the GPU
    (bnr_chains_loo_predict) -> LOOPredictive.  y: the training responses (for the totals; the device has its own copy)."""
    chains = list(chains)
    p_lo, p_hi = _loo_interval_probs(interval)
    lpd, e, k, mean, sd, pit, lo, hi = _capi.pooled_loo_predict(chains, nburn + 1, nsamp, r_eff, p_lo, p_hi)
    return _loo_predictive(y, lpd, e, k, mean, sd, pit, lo, hi, interval, nsamp * len(chains))


def LOOPredict(results, X=None, y=None, x_transform=True, r_eff=None, interval=None):
    """The LOO predictive checks of the training rows -> LOOPredictive.  Uses the GPU's numbers when the fit carried them (loo_predict=True), no
    r_eff is passed and the interval is the fit's; otherwise the host restatement over results.state (chain 1's window) with the training
    X, y passed in (interval default 95)."""
    lp = results.loo_predictive
    if lp is not None and r_eff is None and (interval is None or interval == lp.interval):
        return lp
    if results.state is None or X is None or y is None:
        raise ValueError("LOOPredict needs Fit(..., loo_predict=True), or the state table (return_state=True) together with the training X and y")
    return _host_loo_predict([results.state], X, y, results.burn_in, results.sampled, 95 if interval is None else interval, x_transform, r_eff)


# ------------------------------------------------------------------------------------------ chain stacking (an addition to the reference)
# Posterior statistics of chains that do not mix (Yao, Vehtari & Gelman 2022, "Stacking for non-mixing Bayesian computations", JMLR 23;
# include/bnr_hip.h, ABI 16; DESIGN.md section 8, "Chain stacking"): every chain's own PSIS-LOO pointwise predictive density, the chain weights
# on the simplex that maximise the leave-one-out log score of the mixture, and the summaries and predictions under those weights.  The _host_*
# functions restate the definitions in numpy over fetched tables: the fallback of Stacking and the yardstick of the tests.
STACK_MAX_CHAINS = _capi.STACK_MAX_CHAINS


@dataclass
class ChainStacking:
    """weights: the stacking weight of every chain (they sum to 1); elpd_chain: every chain's own PSIS-LOO elpd (K totals), elpd_chain_i /
    pareto_k: its pointwise values and Pareto k-hat (K x n), n_high_k: per chain the rows whose k-hat is above khat_threshold; elpd_stack: the
    leave-one-out log score of the weighted mixture summed over the rows used, elpd_stack_i pointwise (NaN for a row whose elpd is not finite in
    some chain: those rows are left out, n_used counts the rest), se = sqrt(n_used Var_i(elpd_stack_i)); elpd_uniform: the same score with
    every weight 1 / K (what pooling the chains amounts to); gap: the bound max_k g_k - 1 on the distance of the weights' objective from the
    optimum (per row), iterations: the updates the solver applied; summary: device_summary's dict under the weights, prediction: a BNRPrediction
    under the weights (where requested)."""
    weights: np.ndarray
    elpd_chain: np.ndarray
    elpd_chain_i: np.ndarray
    pareto_k: np.ndarray
    n_high_k: np.ndarray
    elpd_stack: float
    se: float
    elpd_uniform: float
    gap: float
    iterations: int
    elpd_stack_i: np.ndarray = None
    n_used: int = None
    khat_threshold: float = None
    chains: int = None
    draws: int = None
    summary: dict = None
    prediction: BNRPrediction = None
    edge_cov: "EdgeCov" = None       # the posterior covariance of the edge coefficients under the weights (Fit(..., edge_cov=..., stack_chains=True))
    marginal_edges: "MarginalEdges" = None   # the edge table with gamma integrated out under the weights (Fit(..., marginal_edges=True, stack_chains=True))


def _stack_solver_args(max_iter, gap_tol):
    max_iter, gap_tol = int(max_iter), float(gap_tol)
    if max_iter < 1:
        raise ValueError("max_iter must be >= 1")
    if not (math.isfinite(gap_tol) and gap_tol > 0):
        raise ValueError("gap_tol must be positive and finite")
    return max_iter, gap_tol


def stacking_weights(lpd, max_iter=100000, gap_tol=1e-9):
    """The stacking weights of K chains (or models) from the n x K matrix of their pointwise predictive log densities (bnr_stacking_weights;
    host code, no GPU): dict with weights, objective = (1/n) sum_i log sum_k w_k exp(lpd_ik), gap (objective is within gap of the optimum)
    and iterations."""
    max_iter, gap_tol = _stack_solver_args(max_iter, gap_tol)
    w, f, g, it = _capi.stacking_weights_raw(lpd, max_iter, gap_tol)
    return dict(weights=w, objective=f, gap=g, iterations=it)


def _host_stacking_weights(lpd, max_iter=100000, gap_tol=1e-9, dtype=np.float64):
    """bnr_stacking_weights restated in numpy (in `dtype`: the tests run it in long double): the dict of stacking_weights"""
    a = np.ascontiguousarray(lpd, dtype=dtype)
    if a.ndim != 2 or a.shape[0] < 1 or not 1 <= a.shape[1] <= STACK_MAX_CHAINS:
        raise ValueError("lpd must be an n x K matrix with n >= 1 and 1 <= K <= %d" % STACK_MAX_CHAINS)
    if np.isnan(a).any() or (a == np.inf).any() or (a.max(axis=1) == -np.inf).any():
        raise ValueError("lpd must hold no NaN, no +Inf and no row that is -Inf in every chain")
    max_iter, gap_tol = _stack_solver_args(max_iter, gap_tol)
    n, K = a.shape
    mx = a.max(axis=1)
    p = np.exp(a - mx[:, None])
    w = np.full(K, dtype(1) / dtype(K), dtype=dtype)
    it = 0
    while True:
        d = p @ w
        g = (p / d[:, None]).sum(axis=0) / n
        gap = g.max() - 1
        if gap <= gap_tol or it == max_iter:
            break
        w = w * g
        w = w / w.sum()
        it += 1
    return dict(weights=w, objective=(mx + np.log(d)).sum() / n, gap=gap, iterations=it)


def _order_key(x):
    """the order of the summaries as 64-bit keys (bnr_key_of): numbers by value with -0 below +0, every NaN on top"""
    x = np.ascontiguousarray(x, dtype=np.float64)
    u = x.view(np.uint64)
    top = np.uint64(1) << np.uint64(63)
    return np.where(np.isnan(x), ~np.uint64(0), np.where(u & top != 0, ~u, u | top))


def _order_key_inv(k):
    top = np.uint64(1) << np.uint64(63)
    k = np.ascontiguousarray(k, dtype=np.uint64)
    return np.where(k & top != 0, k & ~top, ~k).view(np.float64)


def _strided_mean(x):
    """the mean along the last axis as the summary kernels add it: 256 strided partial sums, an 8-level tree, one division"""
    x = np.asarray(x, dtype=np.float64)
    n = x.shape[-1]
    red = np.zeros(x.shape[:-1] + (256,))
    with np.errstate(all="ignore"):
        for i0 in range(0, n, 256):
            blk = x[..., i0:i0 + 256]
            red[..., :blk.shape[-1]] = red[..., :blk.shape[-1]] + blk
        w = 128
        while w > 0:
            red[..., :w] = red[..., :w] + red[..., w:2 * w]
            w //= 2
        return red[..., 0] / n


def _wquantile_args(x, weights, nchains):
    a = np.ascontiguousarray(x, dtype=np.float64)
    a = a[None, :] if a.ndim == 1 else a
    K = int(nchains)
    if a.ndim != 2 or a.shape[0] < 1 or not 1 <= K <= STACK_MAX_CHAINS or a.shape[1] < K or a.shape[1] % K:
        raise ValueError("x must be an m x (nchains * nsamp) matrix with m, nsamp >= 1 and 1 <= nchains <= %d" % STACK_MAX_CHAINS)
    w = np.ascontiguousarray(weights, dtype=np.float64).reshape(-1)
    if w.shape != (K,):
        raise ValueError("need one weight per chain (%d), not %d" % (K, w.size))
    if not (np.all(np.isfinite(w)) and np.all(w >= 0) and np.any(w > 0)):
        raise ValueError("weights must be finite and >= 0, one of them > 0")
    tot = 0.0
    for v in w:
        tot = tot + v
    if not abs(tot - 1.0) <= 1e-9:
        raise ValueError("weights must sum to 1 (within 1e-9), not %r" % tot)
    return a, w, K


def _host_wquantile(x, weights, nchains, k_lo, k_hi):
    """bnr_wquantile restated in numpy for the rows of an m x (K nsamp) matrix (chain k's draws in columns k nsamp ..): dict of mean, lower,
    upper (m,).  mean = sum_k w_k m_k (k ascending from 0.0); the statistic of rank r: T = r / K, W(x) = sum_k w_k #{draws of chain k with key
    <= key(x)} (k ascending from 0.0), the draw of the smallest key with W >= T, else the largest draw of the chains with w_k > 0; a row with
    a NaN is NaN throughout."""
    a, w, K = _wquantile_args(x, weights, nchains)
    m, S = a.shape
    ns = S // K
    for r in (k_lo, k_hi):
        if not 1 <= int(r) <= S:
            raise ValueError("order statistics must be between 1 and nchains * nsamp")
    seg = a.reshape(m, K, ns)
    with np.errstate(all="ignore"):
        mk = _strided_mean(seg)
        mean = np.zeros(m)
        for k in range(K):
            mean = mean + w[k] * mk[:, k]
    bad = np.isnan(a).any(axis=1)
    mean = np.where(bad, np.nan, mean)
    key = _order_key(a)
    order = np.argsort(key, axis=1, kind="stable")
    skey = np.take_along_axis(key, order, axis=1)
    chain = order // ns
    last = np.ones((m, S), dtype=bool)                               # the last position of every run of equal keys
    last[:, :-1] = skey[:, 1:] != skey[:, :-1]
    pos = np.where(last, np.arange(S)[None, :], S)
    run_end = np.minimum.accumulate(pos[:, ::-1], axis=1)[:, ::-1]   # ... for every position
    W = np.zeros((m, S))
    for k in range(K):
        c = np.take_along_axis(np.cumsum(chain == k, axis=1), run_end, axis=1)
        W = W + w[k] * c.astype(np.float64)
    pk = _order_key(np.where((w > 0)[None, :, None], seg, -np.inf).reshape(m, S)).max(axis=1)     # the largest key of the chains with w_k > 0
    out = {}
    for name, r in (("lower", k_lo), ("upper", k_hi)):
        T = np.float64(int(r)) / np.float64(K)
        hit = W >= T
        first = np.argmax(hit, axis=1)
        kk = np.where(hit.any(axis=1), skey[np.arange(m), first], pk)
        out[name] = np.where(bad, np.nan, _order_key_inv(kk))
    return dict(mean=mean, lower=out["lower"], upper=out["upper"])


def wquantile(x, weights, nchains, interval=95, device=None):
    """The weighted mean and the interval% order statistics of every row of an m x (nchains nsamp) matrix (rows x draws, chain k's draws in
    columns k nsamp .. (k + 1) nsamp - 1) under chain weights, on the GPU (bnr_wquantile): dict with mean, lower, upper (m,) and interval"""
    a, w, K = _wquantile_args(x, weights, nchains)
    lw, hi = _summary_ranks(a.shape[1], interval)
    mean, lo, up = _capi.wquantile_raw(a, w, K, lw, hi, 0 if device is None else int(device))
    return dict(mean=mean, lower=lo, upper=up, interval=interval)


def _weighted_lse(v, w):
    """log sum_{k: w_k > 0} w_k exp(v_k) along axis 0, the largest such v_k taken out, k ascending"""
    v, w = np.asarray(v, dtype=np.float64), np.asarray(w, dtype=np.float64)
    pos = w > 0
    with np.errstate(all="ignore"):
        M = np.max(v[pos], axis=0)
        s = np.zeros(v.shape[1:])
        for k in np.flatnonzero(pos):
            s = s + w[k] * np.exp(v[k] - M)
        return M + np.log(s)


def _stacking(weights, el, kh, gap, iterations, nsamp):
    """ChainStacking from the weights and the per-chain pointwise numbers (K x n)"""
    w, el, kh = np.asarray(weights, dtype=np.float64), np.asarray(el, dtype=np.float64), np.asarray(kh, dtype=np.float64)
    K = el.shape[0]
    used = np.isfinite(el).all(axis=0)
    es = np.full(el.shape[1], np.nan)
    eu = np.full(el.shape[1], np.nan)
    if used.any():
        es[used] = _weighted_lse(el[:, used], w)
        eu[used] = _weighted_lse(el[:, used], np.full(K, 1.0 / K))
    thr = -math.inf if nsamp == 1 else min(1.0 - 1.0 / math.log10(nsamp), 0.7)
    nu = int(used.sum())
    return ChainStacking(weights=w, elpd_chain=el.sum(axis=1), elpd_chain_i=el, pareto_k=kh, n_high_k=(kh > thr).sum(axis=1),
                         elpd_stack=float(np.sum(es[used])), se=float(math.sqrt(nu * np.var(es[used]))) if nu else math.nan,
                         elpd_uniform=float(np.sum(eu[used])), gap=float(gap), iterations=int(iterations), elpd_stack_i=es, n_used=nu,
                         khat_threshold=thr, chains=K, draws=K * int(nsamp))


def device_stack_chains(chains, nburn, nsamp, r_eff=None, max_iter=100000, gap_tol=1e-9):
    """Every chain's own PSIS-LOO over rows nburn+1 .. nburn+nsamp and the stacking weights of the chains, on the GPU (bnr_chains_stack)
    -> ChainStacking"""
    chains = list(chains)
    max_iter, gap_tol = _stack_solver_args(max_iter, gap_tol)
    w, el, kh, _es, gap, it = _capi.chains_stack(chains, nburn + 1, nsamp, r_eff, max_iter, gap_tol)
    return _stacking(w, el, kh, gap, it, nsamp)


def _host_stack_chains(tables, X, y, nburn, nsamp, x_transform=False, r_eff=None, max_iter=100000, gap_tol=1e-9):
    """device_stack_chains restated in numpy over the fetched tables of the same chains and the training X, y: _psis_host per chain, then
    _host_stacking_weights over the rows that are finite in every chain"""
    tables = list(tables)
    if not 1 <= len(tables) <= STACK_MAX_CHAINS:
        raise ValueError("need between 1 and %d tables" % STACK_MAX_CHAINS)
    Xd = _dense_rows(_new_rows(X, x_transform, tables[0]["gamma"].shape[1], y))
    el, kh = [], []
    for t in tables:
        _lpd, e, k = _psis_host(_host_loglik(t, Xd, y, nburn, nsamp), r_eff)
        el.append(e)
        kh.append(k)
    el, kh = np.array(el), np.array(kh)
    used = np.isfinite(el).all(axis=0)
    K = len(tables)
    if used.any():
        r = _host_stacking_weights(el[:, used].T, max_iter, gap_tol)
        w, gap, it = r["weights"], r["gap"], r["iterations"]
    else:
        w, gap, it = np.full(K, 1.0 / K), math.nan, 0
    return _stacking(w, el, kh, gap, it, nsamp)


def device_summary_stacked(chains, weights, nburn, nsamp, interval=95):
    """device_summary_pooled under chain weights (bnr_chains_wsummary): the same ranks of the K nsamp pooled draws, read off the weighted
    distribution"""
    chains = list(chains)
    lw, hi = _summary_ranks(nsamp * len(chains), interval)
    mean, lo, up, pxi = _capi.stacked_summary(chains, weights, nburn + 1, nsamp, lw, hi)
    return dict(interval=interval, estimate=mean, lower_bound=lo, upper_bound=up, probability=pxi, weights=np.array(weights, dtype=np.float64))


def _host_summary_stacked(tables, weights, nburn, nsamp, interval=95):
    """device_summary_stacked from the fetched tables (_host_wquantile on the windows side by side)"""
    tables = list(tables)
    K = len(tables)
    lw, hi = _summary_ranks(nsamp * K, interval)
    q = tables[0]["gamma"].shape[1]
    cols = np.concatenate([np.concatenate([t["gamma"][nburn:nburn + nsamp, :, 0], t["xi"][nburn:nburn + nsamp, :, 0]], axis=1) for t in tables], axis=0)
    h = _host_wquantile(cols.T, weights, K, lw, hi)
    return dict(interval=interval, estimate=h["mean"][:q], lower_bound=h["lower"][:q], upper_bound=h["upper"][:q], probability=h["mean"][q:],
                weights=np.array(weights, dtype=np.float64))


def _stacked_rows(X_new, x_transform, q, y_new):
    """the new rows of a stacked prediction as a model matrix (the entry point takes no adjacency matrices: they are vectorised here)"""
    xi = _new_rows(X_new, x_transform, q, y_new)
    return XInput(_dense_rows(xi), False) if xi.from_matrices else xi


def device_predict_stacked(chains, weights, nburn, nsamp, X_new, y_new=None, interval=95, pred_seed=0, predict_observation=True, x_transform=False):
    """device_predict_pooled under chain weights (bnr_chains_wpredict): the weighted mean and order statistics of the mean response, with y_new
    the lpd of the weighted mixture of the chains' predictive densities, with predict_observation the predictive bounds (the noise of
    device_predict_pooled); no PIT"""
    chains = list(chains)
    if not chains:
        raise ValueError("need at least one chain")
    xi = _stacked_rows(X_new, x_transform, chains[0].q, y_new)
    S = nsamp * len(chains)
    lw, hi = _summary_ranks(S, interval)
    mean, lo, up, lpd, plo, phi = _capi.stacked_predict(chains, weights, xi, nburn + 1, nsamp, lw, hi, y=y_new,
                                                        pred_seed=pred_seed if predict_observation else None)
    return _prediction(mean, lo, up, interval, lpd, None, plo, phi, None, S)


def _host_predict_stacked(tables, weights, X_new, y_new=None, nburn=0, nsamp=None, interval=95, x_transform=False, pred_seed=None, eta=None):
    """device_predict_stacked from the fetched tables.  eta: the m x (K nsamp) matrix of mean responses to work on instead of the float64
    product of the tables (the tests pass the device's own, or an exact one)."""
    tables = list(tables)
    K = len(tables)
    xi = _stacked_rows(X_new, x_transform, tables[0]["gamma"].shape[1], y_new)
    S = nsamp * K
    lw, hi = _summary_ranks(S, interval)
    X = _dense_rows(xi)
    if eta is None:
        eta = np.concatenate([_host_eta(t, X, nburn, nsamp) for t in tables], axis=1)
    h = _host_wquantile(eta, weights, K, lw, hi)
    lpd = None
    if y_new is not None:
        lpd = _weighted_lse(np.array([_host_pointwise(t, X, y_new, nburn, nsamp)[0] for t in tables]), weights)
    plo = phi = None
    if pred_seed is not None:
        tau2 = np.concatenate([t["tau2"][nburn:nburn + nsamp, 0, 0] for t in tables])
        hp = _host_wquantile(eta + np.sqrt(tau2)[None, :] * _capi.host_pred_noise(pred_seed, 0, S, 0, xi.n), weights, K, lw, hi)
        plo, phi = hp["lower"], hp["upper"]
    return _prediction(h["mean"], h["lower"], h["upper"], interval, lpd, None, plo, phi, None, S)


def Stacking(results, X=None, y=None, x_transform=True, tables=None, r_eff=None):
    """The chain stacking of a fit -> ChainStacking.  Uses the GPU's numbers when the fit carried them (stack_chains=True); otherwise restates
    them on the host (_host_stack_chains) over the fetched tables of the chains -- `tables`, or results.state where that is a list of tables --
    with the training X, y passed in."""
    if results.stacking is not None and r_eff is None:
        return results.stacking
    if tables is None and isinstance(results.state, (list, tuple)):
        tables = results.state
    if tables is None or len(tables) < 2 or X is None or y is None:
        raise ValueError("Stacking needs Fit(..., stack_chains=True), or the state tables of at least two chains together with the training X and y")
    return _host_stack_chains(tables, X, y, results.burn_in, results.sampled, x_transform, r_eff)


# ------------------------------------------------------------------------------------------ posterior covariance of the edge coefficients (ABI 17)
# vcov(fit): how the edge coefficients move together, over the pooled window of the chains of one device (include/bnr_hip.h, bnr_chains_cov).
# With c the mean Summary reports for a column -- under chain weights the stacked Summary's -- and G_k[a, b] = sum over chain k's window of
# (x_sa - c_a)(x_sb - c_b), cov = sum_k G_k / (S - 1) (numpy's cov), or sum_k w_k G_k / nsamp under weights (the covariance of the mixture of
# the chains' empirical measures); k ascending from 0.0.
_EDGE_COV_FIELDS = ("cols", "node1", "node2", "mean", "cov", "chains", "draws", "weights")


class EdgeCov:
    """The posterior covariance of edge coefficients.  cols: the 0-based edge indices covered (Summary's order), node1 / node2: their 1-based
    nodes; mean (m,): the posterior means (Summary's, or the stacked Summary's under weights); cov (m, m): the covariance matrix; chains, draws:
    what was pooled; weights: the chain weights, or None.  Derived on the host: sd, corr (NaN where an sd is 0), contrast(C) -- the mean and sd
    of the linear combinations C gamma --, top_pairs(n) -- the most correlated pairs.

    EdgeCov(results) is the accessor of a fit: the GPU's numbers when the fit carried them (edge_cov=...: every chain of the fit), otherwise
    restated on the host over results.state (needs return_state=True; chain 1 alone, every edge).  Without a Results, EdgeCov(**fields) builds
    the record itself from exactly the fields above."""

    def __new__(cls, results=None, **fields):
        if results is not None:
            return _edge_cov_of(results)
        return object.__new__(cls)

    def __init__(self, results=None, **fields):
        if results is not None:                                          # (the accessor: __new__ returned a finished object)
            return
        if set(fields) != set(_EDGE_COV_FIELDS):
            raise TypeError("EdgeCov takes a Results, or exactly the fields %r" % (_EDGE_COV_FIELDS,))
        self.__dict__.update(fields)

    def __repr__(self):
        return "EdgeCov(edges=%d, chains=%d, draws=%d%s)" % (self.cols.size, self.chains, self.draws, "" if self.weights is None else ", weighted")

    @property
    def sd(self):
        """the posterior standard deviations, sqrt(diag(cov))"""
        return np.sqrt(np.diag(self.cov))

    @property
    def corr(self):
        """the correlation matrix cov / (sd sd'); NaN in the row and column of an edge whose sd is 0"""
        sd = self.sd
        with np.errstate(all="ignore"):
            r = self.cov / np.outer(sd, sd)
        zero = sd == 0
        r[zero, :] = np.nan
        r[:, zero] = np.nan
        return r

    def contrast(self, C):
        """dict(mean, sd) of the linear combinations C gamma of the covered edges: C is (r, m) or (m,), a row per combination -- a node's total
        effect, a pathway, a difference of two edges.  mean = C mean, sd = sqrt(diag(C cov C'))"""
        C = np.atleast_2d(np.asarray(C, dtype=np.float64))
        if C.shape[1] != self.cols.size:
            raise ValueError("C must have one column per covered edge (%d), not %d" % (self.cols.size, C.shape[1]))
        with np.errstate(invalid="ignore"):
            return dict(mean=C @ self.mean, sd=np.sqrt(np.einsum("ia,ab,ib->i", C, self.cov, C)))

    def top_pairs(self, n=10):
        """the n pairs (a, b, corr), a < b positions in cols, of largest |corr|, ties by (a, b) ascending; pairs whose corr is NaN are left out"""
        r = self.corr
        a, b = np.triu_indices(r.shape[0], 1)
        v = r[a, b]
        keep = np.flatnonzero(~np.isnan(v))
        order = keep[np.argsort(-np.abs(v[keep]), kind="stable")][:max(int(n), 0)]
        return [(int(a[i]), int(b[i]), float(v[i])) for i in order]


def _edge_nodes(V, cols):
    """(node1, node2), 1-based, of the 0-based edge indices cols in Summary's order (node1 <= node2; utils.jl:40-57)"""
    node1 = np.concatenate([np.full(V - k + 1, k) for k in range(1, V + 1)])
    node2 = np.concatenate([np.arange(k, V + 1) for k in range(1, V + 1)])
    return node1[cols], node2[cols]


def _edge_cov_cols(edge_cov, V=None):
    """The edge_cov keyword of a fit as _finish takes it: None (off: False or None), "all" (True), or the 0-based edge indices as int32 -- from
    an array of indices, or from a list of 1-based (node1, node2) pairs through the edge index.  ValueError for anything else, for an empty list
    and (where V is known) for an index or a node out of range."""
    if edge_cov is None or edge_cov is False:
        return None
    if edge_cov is True:
        return "all"
    if isinstance(edge_cov, (str, bytes, dict)) or np.isscalar(edge_cov):
        raise ValueError("edge_cov must be True, an array of 0-based edge indices or a list of (node1, node2) pairs, not %r" % (edge_cov,))
    try:
        a = np.asarray(edge_cov)
    except Exception:
        a = np.empty(0, dtype=object)
    if a.dtype == object or a.dtype == np.bool_ or a.size < 1 or a.ndim not in (1, 2) or (a.ndim == 2 and a.shape[1] != 2) or not np.all(a == np.floor(a)):
        raise ValueError("edge_cov must be True, an array of 0-based edge indices or a list of (node1, node2) pairs, not %r" % (edge_cov,))
    a = a.astype(np.int64)
    if a.ndim == 2:
        lo, hi = a.min(axis=1), a.max(axis=1)
        if lo.min() < 1 or (V is not None and hi.max() > V):
            raise ValueError("edge_cov: nodes are numbered 1 .. V")
        if V is None:
            return np.ascontiguousarray(a, dtype=np.int32)                 # (the pairs, checked again with V)
        return np.ascontiguousarray((lo - 1) * V - (lo - 1) * (lo - 2) // 2 + (hi - lo), dtype=np.int32)
    if a.min() < 0 or (V is not None and a.max() >= V * (V + 1) // 2):
        raise ValueError("edge_cov: edge indices are 0-based, 0 .. q - 1")
    return np.ascontiguousarray(a, dtype=np.int32)


def _edge_cov(q, cols, mean, cov, nchains, draws, weights):
    V = int(round((-1 + math.sqrt(1 + 8 * q)) / 2))
    cols = np.arange(q, dtype=np.int64) if cols is None else np.asarray(cols, dtype=np.int64)
    n1, n2 = _edge_nodes(V, cols)
    return EdgeCov(cols=cols, node1=n1, node2=n2, mean=mean, cov=cov, chains=nchains, draws=draws,
                   weights=None if weights is None else np.array(weights, dtype=np.float64))


def device_edge_cov(chains, nburn, nsamp, cols=None, weights=None):
    """The posterior covariance of the edge coefficients `cols` (0-based indices; None: all q) over the pooled windows nburn+1 .. nburn+nsamp of
    live chains, on the device (bnr_chains_cov) -> EdgeCov: m + m^2 numbers leave the GPU's side, not the traces.  weights: chain weights (the
    stacking weights), for the covariance of the chains' mixture under them."""
    chains = list(chains)
    if not chains:
        raise ValueError("need at least one chain")
    ci = _capi.cov_cols(cols, chains[0].q)
    mean, cov = _capi.pooled_cov(chains, nburn + 1, nsamp, ci, weights)
    return _edge_cov(chains[0].q, ci, mean, cov, len(chains), len(chains) * int(nsamp), weights)


def _host_cov(seg, weights=None, dtype=np.float64):
    """(mean, cov) of K chains' draws seg (K, nsamp, m) as bnr_cov defines them: the centre is the Summary mean (_strided_mean over the pooled
    draws; under weights sum_k w_k m_k of the chains' own, k ascending from 0.0) in float64; the centred products and their sums in `dtype` (the
    tests run it in long double), chain by chain, then sum_k G_k / (S - 1), or sum_k w_k G_k / nsamp"""
    seg = np.asarray(seg, dtype=np.float64)
    K, ns, m = seg.shape
    with np.errstate(all="ignore"):
        if weights is None:
            c = _strided_mean(seg.reshape(K * ns, m).T)
        else:
            w = np.asarray(weights, dtype=np.float64)
            mk = _strided_mean(np.transpose(seg, (0, 2, 1)))               # (K, m)
            c = np.zeros(m)
            for k in range(K):
                c = c + w[k] * mk[k]
            c = np.where(np.isnan(seg).any(axis=(0, 1)), np.nan, c)
        tot = np.zeros((m, m), dtype=dtype)
        for k in range(K):
            d = seg[k].astype(dtype) - c.astype(dtype)[None, :]
            G = d.T @ d
            tot = tot + (G if weights is None else dtype(w[k]) * G)
        cov = tot / dtype(ns if weights is not None else K * ns - 1)
        bad = ~np.isfinite(c)
        cov[bad, :] = np.nan
        cov[:, bad] = np.nan
    return c, cov


def _host_edge_cov(tables, nburn, nsamp, cols=None, weights=None, dtype=np.float64):
    """device_edge_cov restated in numpy over the fetched tables of the same chains (_host_cov on their windows): the same definition, centres
    included"""
    tables = list(tables)
    if not tables:
        raise ValueError("need at least one table")
    if nsamp * len(tables) < 2:
        raise ValueError("a covariance needs at least 2 draws")
    q = tables[0]["gamma"].shape[1]
    ci = _capi.cov_cols(cols, q)
    if weights is not None:
        weights = _wquantile_args(np.zeros((1, len(tables))), weights, len(tables))[1]
    sel = slice(None) if ci is None else ci
    seg = np.stack([t["gamma"][nburn:nburn + nsamp, :, 0][:, sel] for t in tables])
    mean, cov = _host_cov(seg, weights, dtype)
    return _edge_cov(q, ci, mean, cov, len(tables), len(tables) * int(nsamp), weights)


def cov(draws, nchains=1, weights=None, device=None):
    """The mean and the covariance matrix of any (nchains nsamp) x m matrix of draws (rows = draws, chain k's in rows k nsamp ..), on the GPU
    (bnr_cov): dict with mean (m,) and cov (m, m); numpy's cov about the Summary mean, or with chain weights the covariance of the mixture"""
    mean, c = _capi.cov_raw(draws, nchains, weights, 0 if device is None else int(device))
    return dict(mean=mean, cov=c)


def _edge_cov_of(results):
    """EdgeCov(results): see EdgeCov"""
    if results.edge_cov is not None:
        return results.edge_cov
    if results.state is None:
        raise ValueError("EdgeCov needs Fit(..., edge_cov=True), or the state table (return_state=True)")
    return _host_edge_cov([results.state], results.burn_in, results.sampled)


# ------------------------------------------------------------------------------------------ marginal PSIS-LOO (an addition to the reference)
# PSIS-LOO with the edge coefficients integrated out (integrated importance sampling: Vehtari, Mononen, Tolvanen, Sivula & Winther 2016, JMLR 17;
# include/bnr_mloo.h, libbnr_mloo.so; DESIGN.md section 8, "Marginal PSIS-LOO").  Given phi = (tau2, mu, u, lambda, S) of a table row,
# y | phi ~ N(mu + X W, tau2 A) with A = I + X diag(S) X^T and W_e = sum_t lambda_t u_{t,k(e)} u_{t,l(e)}; the importance ratios
# 1 / p(y_i | y_-i, phi) have far thinner tails than the conditional ones of LOO, which condition on all q edge coefficients.  The _host_*
# functions restate the definitions in numpy: the fallback of MarginalLOO and the yardstick of the tests.
MLOO_MAX_N = _capi.MLOO_MAX_N


def _solve_lower(L, b):
    """L^-1 b for a lower triangular L: scipy's triangular solve where scipy is there, numpy's general solve otherwise"""
    try:
        from scipy.linalg import solve_triangular
    except ImportError:
        return np.linalg.solve(L, b)
    return solve_triangular(L, b, lower=True, check_finite=False)


def _host_marginal_terms(X, y, tau2, mu, S, W=None):
    """(loglik, resid, var (n x D), logml (D,), n_bad) of D draws for one n x q matrix X: the definitions of include/bnr_mloo.h in numpy, per draw
    np.linalg.cholesky of A = I + X diag(S) X^T, L^-1 by a triangular solve (its column norms give c), z = L^-1 r and g = L^-T z.  A draw whose
    S, tau2 or mu is not finite or whose A is not positive definite is NaN and counted"""
    X = np.asarray(X, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64).reshape(-1)
    n, q = X.shape
    tau2, mu = np.atleast_1d(np.asarray(tau2, dtype=np.float64)), np.atleast_1d(np.asarray(mu, dtype=np.float64))
    D = tau2.size
    S = np.asarray(S, dtype=np.float64).reshape(D, q)
    W = None if W is None else np.asarray(W, dtype=np.float64).reshape(D, q)
    ll, rs, vr, ml = np.full((n, D), np.nan), np.full((n, D), np.nan), np.full((n, D), np.nan), np.full(D, np.nan)
    n_bad = 0
    eye = np.eye(n)
    for s in range(D):
        ok = np.isfinite(tau2[s]) and np.isfinite(mu[s]) and np.all(np.isfinite(S[s]))
        L = None
        if ok:
            try:
                L = np.linalg.cholesky(eye + (X * S[s][None, :]) @ X.T)
            except np.linalg.LinAlgError:
                L = None
            if L is not None and not np.all(np.isfinite(L)):
                L = None
        if L is None:
            n_bad += 1
            continue
        r = y - mu[s] - (X @ W[s] if W is not None else 0.0)
        Li = _solve_lower(L, eye)
        c = np.sum(Li * Li, axis=0)
        z = _solve_lower(L, r)
        g = _solve_lower(L[::-1, ::-1].T, z[::-1])[::-1]       # L^T g = z, as a lower triangular solve of the reversed system
        rs[:, s] = g / c
        vr[:, s] = tau2[s] / c
        ll[:, s] = -0.5 * (math.log(2 * math.pi) + np.log(vr[:, s])) - 0.5 * rs[:, s] ** 2 / vr[:, s]
        ml[s] = -0.5 * n * math.log(2 * math.pi * tau2[s]) - np.sum(np.log(np.diag(L))) - 0.5 * float(z @ z) / tau2[s]
    return ll, rs, vr, ml, n_bad


def _edge_nodes_all(V):
    """(ek, el): the column node and the row node (l >= k) of every edge in the column-wise lower-triangle order of utils.jl:50-55"""
    ek = np.concatenate([np.full(V - k, k) for k in range(V)])
    el = np.concatenate([np.arange(k, V) for k in range(V)])
    return ek, el


def _host_marginal_draws(states, nburn, nsamp, thin):
    """(tau2, mu (D,), S, W (D, q)) of rows nburn + 1 + j thin, j = 0 .. ceil(nsamp / thin) - 1, of every fetched table in order: W_e =
    sum_t u_{t,l(e)} lambda_t u_{t,k(e)}, t ascending, from u and lambda of the same row"""
    thin, nd = _capi.mloo_thin_draws(nsamp, thin)
    t2, mu, S, W = [], [], [], []
    for st in states:
        rows = nburn + thin * np.arange(nd)
        u, lam = st["u"][rows], st["lam"][rows, :, 0]            # (nd, R, V), (nd, R)
        ek, el = _edge_nodes_all(u.shape[2])
        w = np.zeros((nd, ek.size))
        for t in range(u.shape[1]):
            w = w + u[:, t, :][:, el] * lam[:, t][:, None] * u[:, t, :][:, ek]
        t2.append(st["tau2"][rows, 0, 0]); mu.append(st["mu"][rows, 0, 0]); S.append(st["S"][rows, :, 0]); W.append(w)
    return np.concatenate(t2), np.concatenate(mu), np.concatenate(S), np.concatenate(W)


def _host_marginal_loglik(states, X, y, nburn, nsamp, thin=1):
    """(loglik, resid, var (n x D), logml (D,), n_bad) over rows nburn + 1 + j thin of the fetched tables `states` (chain k's draws first in
    order k) and the training X (n x q), y: bnr_chains_marginal_loo's three matrices restated in numpy (_host_marginal_terms)"""
    return _host_marginal_terms(X, y, *_host_marginal_draws(list(states), nburn, nsamp, thin))


def marginal_loglik(X, y, tau2, mu, S, W=None, device=None):
    """The marginal leave-one-out terms of D draws phi = (tau2, mu, S, W) for one n x q model matrix on the GPU (bnr_marginal_loglik): dict with
    loglik, resid, var (n x D: log p(y_i | y_-i, phi), y_i - E[y_i | y_-i, phi], Var[y_i | y_-i, phi]), logml (D,: log p(y | phi)) and n_bad
    (the draws that are NaN: S, tau2 or mu not finite, or A not positive definite).  tau2, mu: (D,); S, W: (D, q), W None = 0"""
    ll, rs, vr, ml, nb = _capi.marginal_loglik_raw(X, y, tau2, mu, S, W, 0 if device is None else int(device))
    return dict(loglik=ll, resid=rs, var=vr, logml=ml, n_bad=nb)


def _row_lme(ll):
    """log mean exp of every row of an m x S matrix (NaN for a row holding one)"""
    ll = np.asarray(ll, dtype=np.float64)
    mx = ll.max(axis=1)
    with np.errstate(invalid="ignore"):
        return mx + np.log(np.mean(np.exp(ll - mx[:, None]), axis=1))


def _marginal_loo(y, lpd, elpd, k, loo_mean, loo_sd, logml, thin, draws, n_bad):
    """the dict device_marginal_loo returns, from the pointwise numbers"""
    y = np.asarray(y, dtype=np.float64).reshape(-1)
    out = _loo_from_pointwise(lpd, elpd, k, draws)
    err = y - loo_mean
    sst = float(np.sum((y - y.mean()) ** 2))
    out.update(loo_mean=loo_mean, loo_sd=loo_sd, rmse_loo=float(math.sqrt(np.mean(err ** 2))),
               r2_loo=1.0 - float(np.sum(err ** 2)) / sst if sst > 0 else math.nan, logml=logml, thin=int(thin), draws=int(draws), n_bad=int(n_bad))
    return out


def device_marginal_loo(chains, nburn, nsamp, thin=1, r_eff=None, per_chain=False):
    """Marginal PSIS-LOO of the training rows over rows nburn + 1 + j thin (j = 0 .. ceil(nsamp / thin) - 1) of ALL the chains listed, pooled, on
    the GPU (bnr_chains_marginal_loo): the dict of LOO -- elpd_loo, p_loo, looic, se, elpd_loo_i, p_loo_i, lpd_i, pareto_k, khat_threshold,
    n_high_k, here of the ratios 1 / p(y_i | y_-i, phi) with the edge coefficients integrated out -- plus loo_mean / loo_sd (the LOO predictive
    mean and sd of every row), rmse_loo, r2_loo, logml (log p(y | phi) of every draw), thin, draws and n_bad.  per_chain=True adds elpd_chain
    and pareto_k_chain (K x n, one call per chain), which feed the chain stacking:

        r = device_marginal_loo(chains, nburn, nsamp, thin=10, per_chain=True)
        w = stacking_weights(r["elpd_chain"].T)["weights"]
    """
    chains = list(chains)
    thin, nd = _capi.mloo_thin_draws(nsamp, thin)
    el, kh, lm, ls, ml, ll, nb = _capi.chains_marginal_loo(chains, nburn + 1, nsamp, thin, r_eff, loglik=True)
    out = _marginal_loo(chains[0].y, _row_lme(ll), el, kh, lm, ls, ml, thin, nd * len(chains), nb)
    if per_chain:
        each = [_capi.chains_marginal_loo([c], nburn + 1, nsamp, thin, r_eff) for c in chains]
        out.update(elpd_chain=np.array([e[0] for e in each]), pareto_k_chain=np.array([e[1] for e in each]))
    return out


def _host_marginal_loo(states, X, y, nburn, nsamp, thin=1, r_eff=None):
    """device_marginal_loo restated in numpy over the fetched tables of the same chains and the training X (n x q), y"""
    states = list(states)
    thin, nd = _capi.mloo_thin_draws(nsamp, thin)
    y = np.asarray(y, dtype=np.float64).reshape(-1)
    ll, rs, vr, ml, nb = _host_marginal_loglik(states, X, y, nburn, nsamp, thin)
    lpd = _row_lme(ll)
    lwn, e, k = _psis_weights_host(ll, r_eff)
    w = np.exp(lwn)
    mean = y - np.sum(w * rs, axis=1)
    with np.errstate(invalid="ignore"):
        sd = np.sqrt(np.sum(w * (vr + (y[:, None] - rs) ** 2), axis=1) - mean ** 2)
    return _marginal_loo(y, lpd, e, k, mean, sd, ml, thin, nd * len(states), nb)


def MarginalLOO(results, X=None, y=None, x_transform=True):
    """Marginal PSIS-LOO of the training rows (see device_marginal_loo for the dict).  Uses the GPU's numbers when the fit carried them
    (marginal_loo=True); otherwise the host restatement over results.state (chain 1's window, every draw) with the training X, y passed in."""
    if results.marginal_loo is not None:
        return results.marginal_loo
    if results.state is None or X is None or y is None:
        raise ValueError("MarginalLOO needs Fit(..., marginal_loo=True), or the state table (return_state=True) together with the training X and y")
    xi = _new_rows(X, x_transform, results.state["gamma"].shape[1], y)
    return _host_marginal_loo([results.state], _dense_rows(xi), y, results.burn_in, results.sampled)


def _positive_int(option, value):
    """int(value); ValueError, naming the option, unless it is an integer >= 1"""
    if isinstance(value, bool) or int(value) != value or int(value) < 1:
        raise ValueError("%s must be an integer >= 1, not %r" % (option, value))
    return int(value)


def _marginal_loo_thin(nsamp, draws):
    """thin = ceil(nsamp / marginal_loo_draws); ValueError unless marginal_loo_draws is an integer >= 1"""
    return max(1, -(-int(nsamp) // _positive_int("marginal_loo_draws", draws)))


# ------------------------------------------------------------------------------------------ marginal LOO predictive checks (an addition to the reference)
# LOOPredict's checks under the marginal PSIS weights (include/bnr_mcheck.h, libbnr_mcheck.so; DESIGN.md section 8, "Marginal LOO predictive
# checks").  With gamma integrated out, the leave-one-out predictive distribution of y_i is the mixture sum_s w_is N(y_i - resid_is, var_is) under
# the weights of the ratios 1 / p(y_i | y_-i, phi_s): a weight and a variance per (row, draw).  The _host_* functions restate the definitions in
# numpy: the fallback of MarginalLOOPredict and the yardstick of the tests.
@dataclass
class MarginalLOOPredictive:
    """LOOPredictive (its fields, with its totals) under the marginal PSIS weights: the mixture of every row is sum_s w_is N(m_is, var_is) with
    m_is = y_i - resid_is and var_is = Var[y_i | y_-i, phi_s] (gamma integrated out), lpd_i / elpd_loo_i / pareto_k those of MarginalLOO.
    thin, chains, draws: what was pooled; n_bad: the draws that could not be factorised (every row is NaN while n_bad > 0); logml: log p(y | phi)
    of every draw; loo: the dict of MarginalLOO (device_marginal_loo) from the same call's arrays."""
    loo_mean: np.ndarray
    loo_sd: np.ndarray
    loo_pit: np.ndarray
    loo_lower: np.ndarray
    loo_upper: np.ndarray
    lpd_i: np.ndarray
    elpd_loo_i: np.ndarray
    pareto_k: np.ndarray
    rmse_loo: float
    r2_loo: float
    coverage: float
    ks: float
    interval: float
    draws: int
    khat_threshold: float
    n_high_k: int
    thin: int = None
    chains: int = None
    n_bad: int = None
    logml: np.ndarray = None
    loo: dict = None


def _host_weighted_mixture(mean, var, log_weights, y, p_lo, p_hi, solver=None):
    """bnr_weighted_mixture restated in numpy: (mean, sd, pit, lower, upper, bracket width) per row of the rows x D matrices mean, var and the
    normalised log weights; y (rows,) or None (then mean = sum w m and pit is NaN).  _loo_predict_rows with a sd per (row, draw); a row that holds
    a point mass (var = 0: Phi -> [t >= m]) goes through the library's bisection, the others through _mixture_quantile.  A row with a NaN or
    negative var, a NaN mean or a log weight that is not finite is NaN; a NaN y makes mean, sd and pit NaN."""
    lw = np.asarray(log_weights, dtype=np.float64)
    with np.errstate(all="ignore"):
        w = np.where(np.isfinite(lw), np.exp(lw), np.nan)
    return _host_mixture_rows(mean, var, w, y, p_lo, p_hi, solver)


def _host_mixture_rows(mean, var, w, y, p_lo, p_hi, solver=None):
    """_host_weighted_mixture's six rows for component weights given as they are (rows x D; a NaN weight marks a log weight that was not
    finite): the part it shares with _host_stacked_mixture"""
    m, v, wt = (np.ascontiguousarray(a, dtype=np.float64) for a in (mean, var, w))    # (row-major: numpy's sums do not depend on the caller's layout)
    rows = m.shape[0]
    yv = None if y is None else np.asarray(y, dtype=np.float64).reshape(-1)
    c = _loo_bracket_c(p_lo, p_hi)
    out = np.full((6, rows), np.nan)
    h = 0.70710678118654752440
    for i in range(rows):
        if np.any(np.isnan(wt[i])) or np.any(np.isnan(m[i])) or np.any(np.isnan(v[i])) or np.any(v[i] < 0):
            continue
        w, sd = wt[i], np.sqrt(v[i])
        point = v[i] == 0.0

        def F(t, w=w, mi=m[i], sd=sd, point=point):
            with np.errstate(all="ignore"):
                return float(np.sum(w * np.where(point, (t >= mi).astype(np.float64), 0.5 * _erfc(((t - mi) / sd) * -h))))
        if yv is not None and not math.isnan(yv[i]):
            mu = float(yv[i] - np.sum(w * (yv[i] - m[i])))
            out[2, i] = F(yv[i]) if point.any() else _mixture_cdf(yv[i], w, m[i], sd)
        elif yv is None:
            mu = float(np.sum(w * m[i]))
        else:
            mu = math.nan
        out[0, i] = mu
        out[1, i] = math.sqrt(max(float(np.sum(w * (v[i] + m[i] ** 2))) - mu * mu, 0.0)) if not math.isnan(mu) else math.nan
        if point.any():
            lo, hi = float(np.min(m[i] - c * sd)), float(np.max(m[i] + c * sd))
            out[5, i] = hi - lo
            out[3, i], out[4, i] = _bisect_quantile(F, p_lo, lo, hi), _bisect_quantile(F, p_hi, lo, hi)
        else:
            out[3, i], out[5, i] = _mixture_quantile(p_lo, w, m[i], sd, c, solver)
            out[4, i], _ = _mixture_quantile(p_hi, w, m[i], sd, c, solver)
    return tuple(out)


def weighted_mixture(mean, var, log_weights, y=None, interval=95, device=None):
    """The summary of one weighted mixture of normals per row, sum_s exp(log_weights_is) N(mean_is, var_is), of rows x D matrices on the GPU
    (bnr_weighted_mixture): dict with mean, sd, pit (= F_i(y_i); None without y), lower, upper (rows,) -- the central interval% interval -- and
    interval.  log_weights: normalised log weights, e.g. psis_weights(...)["log_weights"]."""
    p_lo, p_hi = _loo_interval_probs(interval)
    out = dict(zip(_capi.MCHECK_FIELDS, _capi.weighted_mixture_raw(mean, var, log_weights, y, p_lo, p_hi, 0 if device is None else int(device))))
    out["interval"] = interval
    return out


def _marginal_loo_predictive(y, lpd, elpd, k, mean, sd, pit, lower, upper, logml, interval, thin, nchains, draws, n_bad):
    """MarginalLOOPredictive from the pointwise arrays: _loo_predictive's totals, and MarginalLOO's dict from the same arrays"""
    lp = _loo_predictive(y, lpd, elpd, k, mean, sd, pit, lower, upper, interval, draws)
    with np.errstate(invalid="ignore"):
        loo = _marginal_loo(y, lpd, elpd, k, lp.loo_mean, lp.loo_sd, logml, thin, draws, n_bad)
    return MarginalLOOPredictive(**{f.name: getattr(lp, f.name) for f in dataclasses.fields(lp)}, thin=int(thin), chains=int(nchains), n_bad=int(n_bad),
                                 logml=logml, loo=loo)


def device_marginal_loo_predict(chains, nburn, nsamp, thin=1, interval=95, r_eff=None):
    """The LOO predictive checks of the training rows under the marginal PSIS weights over rows nburn + 1 + j thin (j = 0 .. ceil(nsamp / thin)
    - 1) of ALL the chains listed, pooled, on the GPU (bnr_chains_marginal_loo_predict) -> MarginalLOOPredictive.  One call: the factorizations of
    device_marginal_loo, PSIS on their loglik, and the mixture kernels on the device-resident resid and var; `loo` of the record is that
    function's dict (without per_chain)."""
    chains = list(chains)
    thin, nd = _capi.mloo_thin_draws(nsamp, thin)
    p_lo, p_hi = _loo_interval_probs(interval)
    el, kh, (mean, sd, pit, lo, hi), ml, ll, nb = _capi.chains_marginal_loo_predict(chains, nburn + 1, nsamp, thin, r_eff, p_lo, p_hi, loglik=True)
    return _marginal_loo_predictive(chains[0].y, _row_lme(ll), el, kh, mean, sd, pit, lo, hi, ml, interval, thin, len(chains), nd * len(chains), nb)


def _host_marginal_loo_predict(states, X, y, nburn, nsamp, thin=1, interval=95, r_eff=None):
    """device_marginal_loo_predict restated in numpy over the fetched tables of the same chains and the training X (n x q), y"""
    states = list(states)
    thin, nd = _capi.mloo_thin_draws(nsamp, thin)
    p_lo, p_hi = _loo_interval_probs(interval)
    y = np.asarray(y, dtype=np.float64).reshape(-1)
    ll, rs, vr, ml, nb = _host_marginal_loglik(states, X, y, nburn, nsamp, thin)
    lwn, e, k = _psis_weights_host(ll, r_eff)
    mean, sd, pit, lo, hi, _w = _host_weighted_mixture(y[:, None] - rs, vr, lwn, y, p_lo, p_hi)
    return _marginal_loo_predictive(y, _row_lme(ll), e, k, mean, sd, pit, lo, hi, ml, interval, thin, len(states), nd * len(states), nb)


def MarginalLOOPredict(results, X=None, y=None, x_transform=True, interval=None):
    """The LOO predictive checks of the training rows under the marginal PSIS weights -> MarginalLOOPredictive.  Uses the GPU's numbers when the
    fit carried them (marginal_loo_predict=True) and the interval is the fit's; otherwise the host restatement over results.state (chain 1's
    window, every draw) with the training X, y passed in (interval default 95)."""
    rec = results.marginal_loo_predictive
    if rec is not None and (interval is None or interval == rec.interval):
        return rec
    if results.state is None or X is None or y is None:
        raise ValueError("MarginalLOOPredict needs Fit(..., marginal_loo_predict=True), or the state table (return_state=True) together with the "
                         "training X and y")
    xi = _new_rows(X, x_transform, results.state["gamma"].shape[1], y)
    return _host_marginal_loo_predict([results.state], _dense_rows(xi), y, results.burn_in, results.sampled, 1, 95 if interval is None else interval)


# ------------------------------------------------------------------------------------------ chain stacking on the marginal PSIS-LOO (an addition to the reference)
# Stacking's weights from every chain's MARGINAL PSIS-LOO (gamma integrated out: importance ratios that PSIS can use), from one pass over the
# pooled draws, and MarginalLOOPredict's checks of the stacked mixture (include/bnr_mstack.h, libbnr_mstack.so; DESIGN.md section 8, "Chain
# stacking on the marginal LOO").  The _host_* functions restate the definitions in numpy: the fallback of MarginalStack and the yardstick of
# the tests.
@dataclass
class MarginalStacking:
    """ChainStacking's fields from every chain's marginal PSIS-LOO over its own nd = ceil(nsamp / thin) draws (weights, elpd_chain, elpd_chain_i,
    pareto_k, n_high_k, elpd_stack, se, elpd_uniform, gap, iterations, elpd_stack_i, n_used, khat_threshold, chains, draws = K nd), and the
    leave-one-out predictive checks of the stacked mixture sum_{k: w_k > 0} sum_s w_k w_kis N(y_i - resid_kis, var_kis): loo_mean, loo_sd,
    loo_pit, loo_lower, loo_upper (n,), coverage of the interval% interval, ks (the distance of the PITs from U(0, 1)), rmse_loo, r2_loo over the
    rows whose five checks are finite.  thin: what was pooled; n_bad: the draws that could not be factorised (every weight is 1 / K and every
    check NaN while n_bad > 0); logml: log p(y | phi) of every draw.  summary, prediction, edge_cov, marginal_edges, marginal_prediction: the
    fit's other requests under the weights (where requested)."""
    weights: np.ndarray
    elpd_chain: np.ndarray
    elpd_chain_i: np.ndarray
    pareto_k: np.ndarray
    n_high_k: np.ndarray
    elpd_stack: float
    se: float
    elpd_uniform: float
    gap: float
    iterations: int
    elpd_stack_i: np.ndarray
    n_used: int
    khat_threshold: float
    chains: int
    draws: int
    loo_mean: np.ndarray
    loo_sd: np.ndarray
    loo_pit: np.ndarray
    loo_lower: np.ndarray
    loo_upper: np.ndarray
    coverage: float
    ks: float
    rmse_loo: float
    r2_loo: float
    interval: float
    thin: int
    n_bad: int
    logml: np.ndarray = None
    summary: dict = None
    prediction: BNRPrediction = None
    edge_cov: "EdgeCov" = None
    marginal_edges: "MarginalEdges" = None
    marginal_prediction: "MarginalPrediction" = None


def _host_stacked_mixture(mean, var, log_weights, weights, nchains, y, p_lo, p_hi, solver=None):
    """bnr_stacked_mixture restated in numpy: _host_weighted_mixture's six rows for the rows x (nchains nd) matrices mean, var and the log weights
    normalised within every chain, under the chain weights: the columns of the chains with w_k > 0 side by side in chain order, every component's
    weight the product w_k exp(lw) (NaN where lw is not finite); the dropped chains' columns are not read"""
    m, v, lw = (np.asarray(a, dtype=np.float64) for a in (mean, var, log_weights))
    K = int(nchains)
    w = _capi.stack_weights_array(weights, K)
    if m.ndim != 2 or m.shape[1] % K or m.shape[1] < K:
        raise ValueError("mean must be a rows x (nchains * nd) matrix")
    nd = m.shape[1] // K
    keep = np.concatenate([np.arange(k * nd, (k + 1) * nd) for k in range(K) if w[k] > 0])
    wk = np.repeat(w[w > 0], nd)
    with np.errstate(all="ignore"):
        wt = np.where(np.isfinite(lw[:, keep]), wk[None, :] * np.exp(lw[:, keep]), np.nan)
    return _host_mixture_rows(m[:, keep], v[:, keep], wt, y, p_lo, p_hi, solver)


def stacked_mixture(mean, var, log_weights, weights, nchains, y=None, interval=95, device=None):
    """The summary of one stacked mixture of normals per row, sum_{k: w_k > 0} sum_s w_k exp(log_weights_iks) N(mean_iks, var_iks), of rows x
    (nchains nd) matrices (chain k's components in columns k nd .. (k + 1) nd - 1) on the GPU (bnr_stacked_mixture): dict with mean, sd, pit
    (= F_i(y_i); None without y), lower, upper (rows,) -- the central interval% interval --, interval and weights.  log_weights: the log weights
    normalised within every chain, e.g. psis_weights of every chain's slice."""
    p_lo, p_hi = _loo_interval_probs(interval)
    out = dict(zip(_capi.MCHECK_FIELDS, _capi.stacked_mixture_raw(mean, var, log_weights, weights, nchains, y, p_lo, p_hi,
                                                                  0 if device is None else int(device))))
    out.update(interval=interval, weights=np.array(weights, dtype=np.float64))
    return out


def _marginal_stacking(y, weights, el, kh, gap, iterations, nd, mean, sd, pit, lower, upper, logml, interval, thin, n_bad):
    """MarginalStacking from the weights, the per-chain pointwise numbers (K x n) and the checks of the stacked mixture: _stacking's totals with
    nd as the per-chain sample size, _loo_predictive's over the rows whose checks are finite"""
    st = _stacking(weights, el, kh, gap, iterations, nd)
    lp = _loo_predictive(y, st.elpd_stack_i, st.elpd_stack_i, np.zeros(0), mean, sd, pit, lower, upper, interval, st.draws)
    base = {f.name: getattr(st, f.name) for f in dataclasses.fields(st) if f.name in MarginalStacking.__dataclass_fields__ and f.name not in
            ("summary", "prediction", "edge_cov", "marginal_edges", "marginal_prediction")}
    return MarginalStacking(**base, loo_mean=lp.loo_mean, loo_sd=lp.loo_sd, loo_pit=lp.loo_pit, loo_lower=lp.loo_lower, loo_upper=lp.loo_upper,
                            coverage=lp.coverage, ks=lp.ks, rmse_loo=lp.rmse_loo, r2_loo=lp.r2_loo, interval=interval, thin=int(thin), n_bad=int(n_bad),
                            logml=logml)


def device_marginal_stack(chains, nburn, nsamp, thin=1, interval=95, r_eff=None, weights=None, max_iter=100000, gap_tol=1e-9):
    """Chain stacking on the marginal PSIS-LOO of every chain over rows nburn + 1 + j thin (j = 0 .. ceil(nsamp / thin) - 1), and the LOO
    predictive checks of the stacked mixture, on the GPU (bnr_chains_marginal_stack) -> MarginalStacking.  One call and one pass: the
    factorizations of device_marginal_loo over all chains at once, PSIS on every chain's slice of their loglik, the solver of stacking_weights
    on the host, and the mixture kernels on the device-resident resid and var.  weights: chain weights to use instead of the solver's."""
    chains = list(chains)
    thin, nd = _capi.mloo_thin_draws(nsamp, thin)
    p_lo, p_hi = _loo_interval_probs(interval)
    max_iter, gap_tol = _stack_solver_args(max_iter, gap_tol)
    w, el, kh, _es, gap, it, (mean, sd, pit, lo, hi), ml, nb = _capi.chains_marginal_stack(chains, nburn + 1, nsamp, thin, r_eff, weights, max_iter, gap_tol,
                                                                                           p_lo, p_hi)
    return _marginal_stacking(chains[0].y, w, el, kh, gap, it, nd, mean, sd, pit, lo, hi, ml, interval, thin, nb)


def _host_marginal_stack(states, X, y, nburn, nsamp, thin=1, interval=95, r_eff=None, weights=None, max_iter=100000, gap_tol=1e-9):
    """device_marginal_stack restated in numpy over the fetched tables of the same chains and the training X (n x q), y: _host_marginal_loglik
    once, _psis_weights_host on every chain's slice, _host_stacking_weights over the rows that are finite in every chain, _host_stacked_mixture"""
    states = list(states)
    K = len(states)
    if not 1 <= K <= STACK_MAX_CHAINS:
        raise ValueError("need between 1 and %d tables" % STACK_MAX_CHAINS)
    thin, nd = _capi.mloo_thin_draws(nsamp, thin)
    p_lo, p_hi = _loo_interval_probs(interval)
    max_iter, gap_tol = _stack_solver_args(max_iter, gap_tol)
    y = np.asarray(y, dtype=np.float64).reshape(-1)
    ll, rs, vr, ml, nb = _host_marginal_loglik(states, X, y, nburn, nsamp, thin)
    lwn, el, kh = np.empty_like(ll), [], []
    for k in range(K):
        lwn[:, k * nd:(k + 1) * nd], e, kk = _psis_weights_host(ll[:, k * nd:(k + 1) * nd], r_eff)
        el.append(e)
        kh.append(kk)
    el, kh = np.array(el), np.array(kh)
    used = np.isfinite(el).all(axis=0)
    if weights is not None:
        w, gap, it = _capi.stack_weights_array(weights, K), math.nan, 0
    elif used.any():
        r = _host_stacking_weights(el[:, used].T, max_iter, gap_tol)
        w, gap, it = r["weights"], r["gap"], r["iterations"]
    else:
        w, gap, it = np.full(K, 1.0 / K), math.nan, 0
    mean, sd, pit, lo, hi, _w = _host_stacked_mixture(y[:, None] - rs, vr, lwn, w, K, y, p_lo, p_hi)
    return _marginal_stacking(y, w, el, kh, gap, it, nd, mean, sd, pit, lo, hi, ml, interval, thin, nb)


def MarginalStack(results, X=None, y=None, tables=None, x_transform=True):
    """The chain stacking of a fit on the marginal PSIS-LOO -> MarginalStacking.  Uses the GPU's numbers when the fit carried them
    (marginal_stack=True); otherwise restates them on the host (_host_marginal_stack, every draw, interval 95) over the fetched tables of the
    chains -- `tables`, or results.state where that is a list of tables -- with the training X, y passed in."""
    if results.marginal_stacking is not None:
        return results.marginal_stacking
    if tables is None and isinstance(results.state, (list, tuple)):
        tables = results.state
    if tables is None or len(tables) < 2 or X is None or y is None:
        raise ValueError("MarginalStack needs Fit(..., marginal_stack=True), or the state tables of at least two chains together with the "
                         "training X and y")
    xi = _new_rows(X, x_transform, tables[0]["gamma"].shape[1], y)
    return _host_marginal_stack(tables, _dense_rows(xi), y, results.burn_in, results.sampled)


# ------------------------------------------------------------------------------------------ Rao-Blackwellised edge summaries (an addition to the reference)
# The edge table with gamma integrated out (include/bnr_medge.h, libbnr_medge.so; DESIGN.md section 8, "Rao-Blackwellised edge summaries").  Given
# phi = (tau2, mu, u, lambda, S) of a table row, gamma_e | phi, y ~ N(m_e, v_e) in closed form, so the posterior of gamma_e is the mixture of
# those normals over the draws of phi: its mean, sd, interval and sign probabilities carry none of the within-draw noise of the gamma draws.
# The _host_* functions restate the definitions in numpy: the fallback of MarginalEdges and the yardstick of the tests.
_MEDGE_FIELDS = ("node1", "node2", "estimate", "sd", "lower_bound", "upper_bound", "p_pos", "p_neg", "var_within", "interval", "chains", "draws", "thin",
                 "n_bad", "weights", "m", "v")


def _host_gamma_terms(X, y, tau2, mu, S, W=None):
    """(m, v (D x q), n_bad) of D draws for one n x q matrix X: the definitions of include/bnr_medge.h in numpy, per draw np.linalg.cholesky of
    A = I + X diag(S) X^T, T = L^-1 X by a triangular solve (t_e = its column norms squared), g = A^-1 r by two, p = X^T g, m = W + S p,
    v = (tau2 S) max(1 - S t, 0).  A draw whose S, tau2 or mu is not finite or whose A is not positive definite is NaN and counted"""
    X = np.asarray(X, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64).reshape(-1)
    n, q = X.shape
    tau2, mu = np.atleast_1d(np.asarray(tau2, dtype=np.float64)), np.atleast_1d(np.asarray(mu, dtype=np.float64))
    D = tau2.size
    S = np.asarray(S, dtype=np.float64).reshape(D, q)
    W = None if W is None else np.asarray(W, dtype=np.float64).reshape(D, q)
    m, v = np.full((D, q), np.nan), np.full((D, q), np.nan)
    n_bad = 0
    eye = np.eye(n)
    for s in range(D):
        ok = np.isfinite(tau2[s]) and np.isfinite(mu[s]) and np.all(np.isfinite(S[s]))
        L = None
        if ok:
            try:
                L = np.linalg.cholesky(eye + (X * S[s][None, :]) @ X.T)
            except np.linalg.LinAlgError:
                L = None
            if L is not None and not np.all(np.isfinite(L)):
                L = None
        if L is None:
            n_bad += 1
            continue
        r = y - mu[s] - (X @ W[s] if W is not None else 0.0)
        T = _solve_lower(L, X)
        t = np.sum(T * T, axis=0)
        z = _solve_lower(L, r)
        g = _solve_lower(L[::-1, ::-1].T, z[::-1])[::-1]       # L^T g = z, as a lower triangular solve of the reversed system
        m[s] = (W[s] if W is not None else 0.0) + S[s] * (X.T @ g)
        v[s] = (tau2[s] * S[s]) * np.fmax(1.0 - S[s] * t, 0.0)
    return m, v, n_bad


def _host_marginal_gamma(states, X, y, nburn, nsamp, thin=1):
    """(m, v (D x q), n_bad) over rows nburn + 1 + j thin of the fetched tables `states` (chain k's draws first in order k) and the training
    X (n x q), y: the two matrices of bnr_chains_marginal_edges restated in numpy (_host_gamma_terms)"""
    return _host_gamma_terms(X, y, *_host_marginal_draws(list(states), nburn, nsamp, thin))


def _medge_chain_sum(terms):
    """the chain sum of include/bnr_medge.h for every column of an nd x q matrix of terms: partial sum l (0 .. 63) takes rows l, l + 64, ... in
    order from 0.0; the partial sums are then added pairwise, l with l + 32, then 16, 8, 4, 2, 1"""
    nd, q = terms.shape
    rows = -(-nd // 64)
    pad = np.zeros((rows * 64, q))
    pad[:nd] = terms
    acc = np.zeros((64, q))
    for r in range(rows):
        acc = acc + pad[r * 64:(r + 1) * 64]
    off = 32
    while off:
        acc = acc[:off] + acc[off:2 * off]
        off //= 2
    return acc[0]


def _medge_stat(terms, K, w):
    """sum_k (chain sum of chain k's rows / nd) w_k, k ascending from 0.0"""
    nd = terms.shape[0] // K
    tot = np.zeros(terms.shape[1])
    for k in range(K):
        tot = tot + (_medge_chain_sum(terms[k * nd:(k + 1) * nd]) / float(nd)) * w[k]
    return tot


def _host_mixture_summary(m, v, nchains=1, weights=None, p_lo=0.025, p_hi=0.975):
    """bnr_mixture_summary restated in numpy with its summation order: dict of mean, sd, var_within, p_pos, p_neg, lower, upper (q,) for the
    (nchains nd) x q matrices m, v.  The quantiles by _bisect_quantile from the bracket of _loo_bracket_c; erfc is scipy's (or math's), so the
    three statistics that go through it agree with the device to rounding, the others bit for bit"""
    m, v = np.asarray(m, dtype=np.float64), np.asarray(v, dtype=np.float64)
    K = int(nchains)
    D, q = m.shape
    w = np.full(K, 1.0 / K) if weights is None else np.asarray(weights, dtype=np.float64).reshape(K)
    p_lo, p_hi = _capi.loo_probs(p_lo, p_hi)
    c = _loo_bracket_c(p_lo, p_hi)
    h = 0.70710678118654752440
    point = v == 0.0
    with np.errstate(all="ignore"):
        sd = np.sqrt(v)
        r = m / sd
        out = dict(mean=_medge_stat(m, K, w), var_within=_medge_stat(v, K, w))
        out["sd"] = np.sqrt(np.fmax(_medge_stat(v + m * m, K, w) - out["mean"] * out["mean"], 0.0))
        out["p_pos"] = _medge_stat(np.where(point, (m > 0).astype(np.float64), 0.5 * _erfc(r * -h)), K, w)
        out["p_neg"] = _medge_stat(np.where(point, (m < 0).astype(np.float64), 0.5 * _erfc(r * h)), K, w)
        lo, hi = np.min(m - c * sd, axis=0), np.max(m + c * sd, axis=0)
        lower, upper = np.full(q, np.nan), np.full(q, np.nan)
        nan = np.any(np.isnan(m) | np.isnan(v), axis=0)
        for e in range(q):
            if nan[e]:
                continue
            me, se, pe = m[:, e:e + 1], sd[:, e:e + 1], point[:, e:e + 1]

            def F(t, me=me, se=se, pe=pe):
                return float(_medge_stat(np.where(pe, (t >= me).astype(np.float64), 0.5 * _erfc(((t - me) / se) * -h)), K, w)[0])
            lower[e] = _bisect_quantile(F, p_lo, float(lo[e]), float(hi[e]))
            upper[e] = _bisect_quantile(F, p_hi, float(lo[e]), float(hi[e]))
    for k in ("mean", "sd", "var_within", "p_pos", "p_neg"):
        out[k] = np.where(nan, np.nan, out[k])
    out.update(lower=lower, upper=upper)
    return out


class MarginalEdges:
    """The edge table with gamma integrated out.  node1 / node2: the 1-based nodes of every edge (Summary's order); estimate, sd: the mean and
    standard deviation of the mixture sum_s omega_s N(m_se, v_se); lower_bound / upper_bound: its central interval% interval; p_pos / p_neg: its
    mass above / below 0, each summed on its own; var_within: sum_s omega_s v_se.  Derived: lfsr = min(p_pos, p_neg), rb_share = var_within /
    sd^2 -- the share of the posterior variance that Rao-Blackwellisation removes from the estimator's noise.  chains, draws, thin: what was
    pooled; n_bad: the draws that could not be factorised (every summary is NaN while n_bad > 0); weights: the chain weights, or None; m, v: the
    per-draw conditional means and variances (draws x q), or None.

    MarginalEdges(results, X, y) is the accessor of a fit: the GPU's numbers when the fit carried them (marginal_edges=True), otherwise restated
    on the host over results.state (needs return_state=True and the training X, y; chain 1's window, every draw).  Without a Results,
    MarginalEdges(**fields) builds the record itself from exactly the fields above."""

    def __new__(cls, results=None, X=None, y=None, x_transform=True, **fields):
        if results is not None:
            return _marginal_edges_of(results, X, y, x_transform)
        return object.__new__(cls)

    def __init__(self, results=None, X=None, y=None, x_transform=True, **fields):
        if results is not None:                                          # (the accessor: __new__ returned a finished object)
            return
        if set(fields) != set(_MEDGE_FIELDS):
            raise TypeError("MarginalEdges takes a Results, or exactly the fields %r" % (_MEDGE_FIELDS,))
        self.__dict__.update(fields)

    def __repr__(self):
        return "MarginalEdges(edges=%d, chains=%d, draws=%d%s)" % (self.estimate.size, self.chains, self.draws, "" if self.weights is None else ", weighted")

    @property
    def lfsr(self):
        """the local false sign rate min(p_pos, p_neg) of every edge"""
        return np.fmin(self.p_pos, self.p_neg) + 0.0 * (self.p_pos + self.p_neg)       # (NaN where either is)

    @property
    def rb_share(self):
        """var_within / sd^2 (NaN where sd is 0)"""
        with np.errstate(all="ignore"):
            return np.where(self.sd > 0, self.var_within / (self.sd * self.sd), np.nan)


def _marginal_edges(stats, m, v, interval, nchains, draws, thin, n_bad, weights):
    q = stats["mean"].size
    V = int(round((-1 + math.sqrt(1 + 8 * q)) / 2))
    if V * (V + 1) // 2 == q:
        n1, n2 = _edge_nodes(V, np.arange(q))
    else:                                                               # (a raw matrix whose columns are no lower triangle)
        n1 = n2 = np.arange(1, q + 1)
    return MarginalEdges(node1=n1, node2=n2, estimate=stats["mean"], sd=stats["sd"], lower_bound=stats["lower"], upper_bound=stats["upper"],
                         p_pos=stats["p_pos"], p_neg=stats["p_neg"], var_within=stats["var_within"], interval=interval, chains=int(nchains),
                         draws=int(draws), thin=int(thin), n_bad=int(n_bad), weights=None if weights is None else np.array(weights, dtype=np.float64),
                         m=m, v=v)


def marginal_gamma(X, y, tau2, mu, S, W=None, device=None):
    """The conditional posterior of every edge coefficient given each of D draws phi = (tau2, mu, S, W), for one n x q model matrix, on the GPU
    (bnr_marginal_gamma): dict with m, v (D x q: gamma_e | phi, y ~ N(m, v)) and n_bad (the draws that are NaN: S, tau2 or mu not finite, or A
    not positive definite).  tau2, mu: (D,); S, W: (D, q), W None = 0"""
    m, v, nb = _capi.marginal_gamma_raw(X, y, tau2, mu, S, W, 0 if device is None else int(device))
    return dict(m=m, v=v, n_bad=nb)


def mixture_summary(m, v, nchains=1, weights=None, interval=95, device=None):
    """The summary of the q mixtures of normals in the columns of the (nchains nd) x q matrices m, v (chain k's draws in rows k nd ..) on the GPU
    (bnr_mixture_summary): dict with mean, sd, var_within, p_pos, p_neg, lower, upper (q,) -- the central interval% interval.  weights: chain
    weights (default 1 / nchains each)"""
    p_lo, p_hi = _loo_interval_probs(interval)
    return dict(zip(_capi.MEDGE_SUMMARY_FIELDS, _capi.mixture_summary_raw(m, v, nchains, weights, p_lo, p_hi, 0 if device is None else int(device))))


def device_marginal_edges(chains, nburn, nsamp, thin=1, weights=None, interval=95, per_draw=False):
    """The edge table with gamma integrated out over rows nburn + 1 + j thin (j = 0 .. ceil(nsamp / thin) - 1) of ALL the chains listed, pooled
    (under `weights`, the chain weights, where given), on the GPU (bnr_chains_marginal_edges) -> MarginalEdges.  The per-draw m and v stay on the
    device unless per_draw=True asks for them."""
    chains = list(chains)
    thin, nd = _capi.mloo_thin_draws(nsamp, thin)
    p_lo, p_hi = _loo_interval_probs(interval)
    out, m, v, nb = _capi.chains_marginal_edges(chains, nburn + 1, nsamp, thin, weights, p_lo, p_hi, per_draw)
    return _marginal_edges(dict(zip(_capi.MEDGE_SUMMARY_FIELDS, out)), m, v, interval, len(chains), nd * len(chains), thin, nb, weights)


def _host_marginal_edges(states, X, y, nburn, nsamp, thin=1, weights=None, interval=95, per_draw=False):
    """device_marginal_edges restated in numpy over the fetched tables of the same chains and the training X (n x q), y"""
    states = list(states)
    thin, nd = _capi.mloo_thin_draws(nsamp, thin)
    p_lo, p_hi = _loo_interval_probs(interval)
    m, v, nb = _host_marginal_gamma(states, X, y, nburn, nsamp, thin)
    stats = _host_mixture_summary(m, v, len(states), weights, p_lo, p_hi)
    return _marginal_edges(stats, m if per_draw else None, v if per_draw else None, interval, len(states), nd * len(states), thin, nb, weights)


def _marginal_edges_of(results, X=None, y=None, x_transform=True):
    if results.marginal_edges is not None:
        return results.marginal_edges
    if results.state is None or X is None or y is None:
        raise ValueError("MarginalEdges needs Fit(..., marginal_edges=True), or the state table (return_state=True) together with the training X and y")
    xi = _new_rows(X, x_transform, results.state["gamma"].shape[1], y)
    return _host_marginal_edges([results.state], _dense_rows(xi), y, results.burn_in, results.sampled)


# ------------------------------------------------------------------------------------------ Rao-Blackwellised covariance of the edge coefficients (an addition to the reference)
# The covariance of the edge coefficients with gamma integrated out (include/bnr_mcov.h, libbnr_mcov.so; DESIGN.md section 8, "Rao-Blackwellised
# covariance of the edge coefficients").  Given phi of a table row the whole vector gamma is N(m, tau2 (D - D X^T A^-1 X D)), so the covariance
# of the mixture over the draws is within + between (law of total covariance): within = sum omega_s of the conditional covariances, between =
# the covariance of the conditional means.  EdgeCov estimates the same matrix from the gamma draws, within-draw noise included.  The _host_*
# functions restate the definitions in numpy: the fallback of MarginalEdgeCov and the yardstick of the tests.
_MEDGE_COV_FIELDS = ("cols", "node1", "node2", "mean", "cov", "within", "chains", "draws", "thin", "n_bad", "weights")


class MarginalEdgeCov(EdgeCov):
    """The posterior covariance of edge coefficients with gamma integrated out.  cols, node1 / node2, mean, cov, chains, draws, weights: as in
    EdgeCov, with mean and cov those of the mixture sum_s omega_s N(m_s, C_s) over the draws of phi; within (m, m): sum_s omega_s C_s, the part
    that is known in closed form given a draw (its diagonal is not clamped: it may fall a rounding below 0); thin: the row stride; n_bad: the
    draws that could not be factorised (mean, cov and within are NaN while n_bad > 0).  Derived on the host: EdgeCov's sd, corr, contrast(C)
    and top_pairs(n), between = cov - within, rb_share = diag(within) / diag(cov).

    MarginalEdgeCov(results, X, y) is the accessor of a fit: the GPU's numbers when the fit carried them (marginal_edge_cov=...), otherwise
    restated on the host over results.state (needs return_state=True and the training X, y; chain 1's window, every draw, every edge).  Without a
    Results, MarginalEdgeCov(**fields) builds the record itself from exactly the fields above."""

    def __new__(cls, results=None, X=None, y=None, x_transform=True, **fields):
        if results is not None:
            return _marginal_edge_cov_of(results, X, y, x_transform)
        return object.__new__(cls)

    def __init__(self, results=None, X=None, y=None, x_transform=True, **fields):
        if results is not None:                                          # (the accessor: __new__ returned a finished object)
            return
        if set(fields) != set(_MEDGE_COV_FIELDS):
            raise TypeError("MarginalEdgeCov takes a Results, or exactly the fields %r" % (_MEDGE_COV_FIELDS,))
        self.__dict__.update(fields)

    def __repr__(self):
        return "MarginalEdgeCov(edges=%d, chains=%d, draws=%d%s)" % (self.cols.size, self.chains, self.draws, "" if self.weights is None else ", weighted")

    @property
    def between(self):
        """cov - within: the covariance of the conditional means over the draws"""
        return self.cov - self.within

    @property
    def rb_share(self):
        """diag(within) / diag(cov) (NaN where the variance is not > 0): the share of every variance that is known in closed form"""
        dc, dw = np.diag(self.cov), np.diag(self.within)
        with np.errstate(all="ignore"):
            return np.where(dc > 0, dw / dc, np.nan)


def _marginal_edge_cov(q, cols, mean, cov, within, nchains, draws, thin, n_bad, weights):
    V = int(round((-1 + math.sqrt(1 + 8 * q)) / 2))
    cols = np.arange(q, dtype=np.int64) if cols is None else np.asarray(cols, dtype=np.int64)
    if V * (V + 1) // 2 == q:
        n1, n2 = _edge_nodes(V, cols)
    else:                                                               # (a raw matrix whose columns are no lower triangle)
        n1 = n2 = cols + 1
    return MarginalEdgeCov(cols=cols, node1=n1, node2=n2, mean=mean, cov=cov, within=within, chains=int(nchains), draws=int(draws), thin=int(thin),
                           n_bad=int(n_bad), weights=None if weights is None else np.array(weights, dtype=np.float64))


def _host_gamma_cov(X, y, tau2, mu, S, W=None, cols=None):
    """(m (c,), Cov (c, c)) of ONE draw phi = (tau2, mu, S, W) for the n x q matrix X, in numpy through the A^-1 form: with A = I + X D X^T,
    m = W + D X^T A^-1 (y - mu - X W) and Cov = tau2 (D - D X^T A^-1 X D), at the columns cols (None: all)"""
    X = np.asarray(X, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64).reshape(-1)
    n, q = X.shape
    S = np.asarray(S, dtype=np.float64).reshape(q)
    W = np.zeros(q) if W is None else np.asarray(W, dtype=np.float64).reshape(q)
    ci = _capi.cov_cols(cols, q)
    sel = np.arange(q) if ci is None else ci.astype(np.int64)
    A = np.eye(n) + (X * S[None, :]) @ X.T
    Xs = X[:, sel]
    AiX = np.linalg.solve(A, Xs)
    m = W[sel] + S[sel] * (Xs.T @ np.linalg.solve(A, y - float(mu) - X @ W))
    # (a repeated column: the diagonal term stands wherever the two edges are the same one)
    C = float(tau2) * (np.where(sel[:, None] == sel[None, :], S[sel][:, None], 0.0) - (S[sel][:, None] * (Xs.T @ AiX)) * S[sel][None, :])
    return m, C


def _host_gamma_cov_terms(X, y, tau2, mu, S, W, nchains, cols=None, weights=None, dtype=np.float64):
    """(mean, cov, within, m, v, n_bad) of bnr_marginal_gamma_cov restated in numpy with the header's orders: per draw the scaled panel
    T' = (sqrt(tau2) S) L^-1 X, the chains' Grams of T' and of m - mean over the draws in order (products and sums in `dtype`), the chain sums
    of _medge_stat for mean and the diagonal, k ascending"""
    X = np.asarray(X, dtype=np.float64)
    n, q = X.shape
    tau2 = np.atleast_1d(np.asarray(tau2, dtype=np.float64))
    D, K = tau2.size, int(nchains)
    nd = D // K
    S = np.asarray(S, dtype=np.float64).reshape(D, q)
    ci = _capi.cov_cols(cols, q)
    sel = np.arange(q) if ci is None else ci.astype(np.int64)
    c = sel.size
    w = np.full(K, 1.0 / K) if weights is None else np.asarray(weights, dtype=np.float64).reshape(K)
    m, v, n_bad = _host_gamma_terms(X, y, tau2, mu, S, W)
    m, v = m[:, sel], v[:, sel]
    nanm = np.full((c, c), np.nan)
    if n_bad:
        return np.full(c, np.nan), nanm, nanm.copy(), m, v, n_bad
    Xs, eye = X[:, sel], np.eye(n)
    Gw = np.zeros((K, c, c), dtype=dtype)
    for s in range(D):
        L = np.linalg.cholesky(eye + (X * S[s][None, :]) @ X.T)
        Tp = ((np.sqrt(tau2[s]) * S[s, sel])[None, :] * _solve_lower(L, Xs)).astype(dtype)
        Gw[s // nd] = Gw[s // nd] + Tp.T @ Tp
    mean = _medge_stat(m, K, w)
    dg = _medge_stat(tau2[:, None] * S[:, sel], K, w)
    Cm = (m - mean[None, :]).astype(dtype)
    gw, gb = np.zeros((c, c), dtype=dtype), np.zeros((c, c), dtype=dtype)
    for k in range(K):
        Ck = Cm[k * nd:(k + 1) * nd]
        gw = gw + (Gw[k] / dtype(nd)) * dtype(w[k])
        gb = gb + ((Ck.T @ Ck) / dtype(nd)) * dtype(w[k])
    within = np.where(sel[:, None] == sel[None, :], dg.astype(dtype)[:, None], dtype(0.0)) - gw
    return mean, within + gb, within, m, v, 0


def marginal_gamma_cov(X, y, tau2, mu, S, W=None, cols=None, nchains=1, weights=None, device=None):
    """The covariance of the edge coefficients `cols` (0-based; None: all q) of the mixture of the conditional normals of gamma given each of
    D = nchains nd draws phi = (tau2, mu, S, W) for one n x q model matrix, on the GPU (bnr_marginal_gamma_cov): dict with mean (c,), cov and
    within (c, c; cov = within + between), m, v (D x c: the per-draw conditional means and variances) and n_bad.  One draw gives its
    conditional covariance, cov == within."""
    mean, cov, within, m, v, nb = _capi.marginal_gamma_cov_raw(X, y, tau2, mu, S, W, cols, nchains, weights, 0 if device is None else int(device))
    return dict(mean=mean, cov=cov, within=within, m=m, v=v, n_bad=nb)


def device_marginal_edge_cov(chains, nburn, nsamp, thin=1, cols=None, weights=None, per_draw=False):
    """The covariance of the edge coefficients `cols` (0-based; None: all q) with gamma integrated out over rows nburn + 1 + j thin (j = 0 ..
    ceil(nsamp / thin) - 1) of ALL the chains listed, pooled (under `weights`, the chain weights -- the stacking weights -- where given), on the
    GPU (bnr_chains_marginal_edge_cov) -> MarginalEdgeCov.  per_draw=True returns (record, m, v) with the per-draw conditional means and
    variances of the chosen columns."""
    chains = list(chains)
    thin, nd = _capi.mloo_thin_draws(nsamp, thin)
    if not chains:
        raise ValueError("need at least one chain")
    ci = _capi.cov_cols(cols, chains[0].q)
    mean, cov, within, m, v, nb = _capi.chains_marginal_edge_cov(chains, nburn + 1, nsamp, thin, ci, weights, per_draw)
    rec = _marginal_edge_cov(chains[0].q, ci, mean, cov, within, len(chains), nd * len(chains), thin, nb, weights)
    return (rec, m, v) if per_draw else rec


def _host_marginal_edge_cov(states, X, y, nburn, nsamp, thin=1, cols=None, weights=None, dtype=np.float64):
    """device_marginal_edge_cov restated in numpy over the fetched tables of the same chains and the training X (n x q), y, with the orders of
    include/bnr_mcov.h (_host_gamma_cov_terms)"""
    states = list(states)
    thin, nd = _capi.mloo_thin_draws(nsamp, thin)
    X = np.asarray(X, dtype=np.float64)
    q = X.shape[1]
    ci = _capi.cov_cols(cols, q)
    mean, cov, within, _m, _v, nb = _host_gamma_cov_terms(X, y, *_host_marginal_draws(states, nburn, nsamp, thin), len(states), ci, weights, dtype)
    return _marginal_edge_cov(q, ci, mean, cov, within, len(states), nd * len(states), thin, nb, weights)


def _marginal_edge_cov_of(results, X=None, y=None, x_transform=True):
    if results.marginal_edge_cov is not None:
        return results.marginal_edge_cov
    if results.state is None or X is None or y is None:
        raise ValueError("MarginalEdgeCov needs Fit(..., marginal_edge_cov=True), or the state table (return_state=True) together with the training "
                         "X and y")
    xi = _new_rows(X, x_transform, results.state["gamma"].shape[1], y)
    return _host_marginal_edge_cov([results.state], _dense_rows(xi), y, results.burn_in, results.sampled)


# ------------------------------------------------------------------------------------------ Rao-Blackwellised prediction of new rows (an addition to the reference)
# The prediction of new rows with gamma integrated out (include/bnr_mpred.h, libbnr_mpred.so; DESIGN.md section 8, "Rao-Blackwellised prediction").
# Given phi = (tau2, mu, u, lambda, S) of a table row, the mean response of a new row x* is N(mean, var) in closed form, so its posterior is the
# mixture of those normals over the draws of phi and the predictive distribution of a new observation the same mixture with var + tau2: no
# within-draw noise of gamma, no predictive noise to draw.  The _host_* functions restate the definitions in numpy: the fallback of
# MarginalPredict and the yardstick of the tests.
_LOG_2PI = 1.8378770664093454835606594728112      # (MLOO_LOG_2PI of csrc/bnr_mloo_kernels.h)
_MPRED_FIELDS = ("estimate", "sd", "lower_bound", "upper_bound", "var_within", "pred_sd", "pred_lower_bound", "pred_upper_bound", "lpd", "elpd", "pit",
                 "interval", "chains", "draws", "thin", "n_bad", "weights", "mean", "var")


def _host_predict_terms(X, y, X_new, tau2, mu, S, W=None):
    """(mean, var (D x m), n_bad) of D draws for one n x q matrix X and the m x q new rows X_new: the definitions of include/bnr_mpred.h in numpy,
    per draw np.linalg.cholesky of A = I + X diag(S) X^T, C = (X S) X*^T, T = L^-1 C by a triangular solve (t_j = its column norms squared),
    g = A^-1 r by two, h = C^T g, a = X* W, d_j = sum_e (x*_je S_e) x*_je, mean = (mu + a) + h, var = tau2 max(d - t, 0).  A draw whose S, tau2
    or mu is not finite or whose A is not positive definite is NaN and counted"""
    X = np.asarray(X, dtype=np.float64)
    Xn = np.asarray(X_new, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64).reshape(-1)
    n, q = X.shape
    m = Xn.shape[0]
    tau2, mu = np.atleast_1d(np.asarray(tau2, dtype=np.float64)), np.atleast_1d(np.asarray(mu, dtype=np.float64))
    D = tau2.size
    S = np.asarray(S, dtype=np.float64).reshape(D, q)
    W = None if W is None else np.asarray(W, dtype=np.float64).reshape(D, q)
    mean, var = np.full((D, m), np.nan), np.full((D, m), np.nan)
    n_bad = 0
    eye = np.eye(n)
    for s in range(D):
        ok = np.isfinite(tau2[s]) and np.isfinite(mu[s]) and np.all(np.isfinite(S[s]))
        L = None
        if ok:
            XS = X * S[s][None, :]
            try:
                L = np.linalg.cholesky(eye + XS @ X.T)
            except np.linalg.LinAlgError:
                L = None
            if L is not None and not np.all(np.isfinite(L)):
                L = None
        if L is None:
            n_bad += 1
            continue
        r = y - mu[s] - (X @ W[s] if W is not None else 0.0)
        Cm = XS @ Xn.T
        T = _solve_lower(L, Cm)
        t = np.sum(T * T, axis=0)
        z = _solve_lower(L, r)
        g = _solve_lower(L[::-1, ::-1].T, z[::-1])[::-1]       # L^T g = z, as a lower triangular solve of the reversed system
        a = Xn @ W[s] if W is not None else 0.0
        d = np.sum((Xn * S[s][None, :]) * Xn, axis=1)
        mean[s] = (mu[s] + a) + Cm.T @ g
        var[s] = tau2[s] * np.fmax(d - t, 0.0)
    return mean, var, n_bad


def _host_mixture_score(mean, vobs, y, nchains=1, weights=None):
    """bnr_mixture_score restated in numpy with its summation order: dict of lpd, pit (m,) for the (nchains nd) x m matrices mean, vobs and the
    responses y (m,).  A component with vobs = 0 is the point mass at mean (pit: [y >= mean]; lpd: nothing unless y == mean, then +inf; -inf where
    every weighted component is a point mass elsewhere); a row with a NaN y, a NaN mean or vobs in any draw of any chain or a vobs < 0 is NaN in
    both.  pit agrees with the device bit for bit where no erfc is involved, otherwise to erfc's rounding; lpd to the rounding of exp and log"""
    me, vo = np.asarray(mean, dtype=np.float64), np.asarray(vobs, dtype=np.float64)
    K = int(nchains)
    D, m = me.shape
    nd = D // K
    yv = np.asarray(y, dtype=np.float64).reshape(m)
    w = np.full(K, 1.0 / K) if weights is None else np.asarray(weights, dtype=np.float64).reshape(K)
    h = 0.70710678118654752440
    with np.errstate(all="ignore"):
        dlt = yv[None, :] - me
        point = vo == 0.0
        l = np.where(point, np.where(dlt == 0.0, np.inf, -np.inf), -0.5 * (_LOG_2PI + np.log(vo)) - 0.5 * ((dlt * dlt) / vo))
        nan = np.isnan(yv) | np.any(np.isnan(me) | np.isnan(vo) | np.isnan(l), axis=0)
        pit = _medge_stat(np.where(point, (yv[None, :] >= me).astype(np.float64), 0.5 * _erfc((dlt / np.sqrt(vo)) * -h)), K, w)
        on = np.repeat(w > 0.0, nd)
        mx = np.max(np.where(np.isnan(l[on]), -np.inf, l[on]), axis=0)
        tot = np.zeros(m)
        fin = np.isfinite(mx)
        mxs = np.where(fin, mx, 0.0)
        for k in range(K):
            if w[k] > 0.0:
                lk = np.where(point[k * nd:(k + 1) * nd], -np.inf, l[k * nd:(k + 1) * nd])
                tot = tot + (_medge_chain_sum(np.exp(lk - mxs[None, :])) / float(nd)) * w[k]
        lpd = np.where(fin, mxs + np.log(tot), mx)
    return dict(lpd=np.where(nan, np.nan, lpd), pit=np.where(nan, np.nan, pit))


class MarginalPrediction:
    """The prediction of new rows with gamma integrated out.  estimate, sd: the mean and standard deviation of the mixture sum_s omega_s
    N(mean_sj, var_sj), the posterior of the mean response of every new row; lower_bound / upper_bound: its central interval% interval;
    var_within: sum_s omega_s var_sj; pred_sd, pred_lower_bound / pred_upper_bound: the same of the predictive distribution of a new observation,
    the mixture with var + tau2; lpd, pit: the log predictive density and the probability integral transform of the observed y_new under it (None
    without y_new), elpd: the sum of lpd.  Derived: rb_share = var_within / sd^2 -- the share of the posterior variance of the mean response that
    Rao-Blackwellisation removes from the estimator's noise.  chains, draws, thin: what was pooled; n_bad: the draws that could not be factorised
    (every summary is NaN while n_bad > 0); weights: the chain weights, or None; mean, var: the per-draw conditional means and variances (draws x
    m), or None.  MarginalPrediction(**fields) builds the record from exactly the fields above; MarginalPredict is the accessor of a fit."""

    def __init__(self, **fields):
        if set(fields) != set(_MPRED_FIELDS):
            raise TypeError("MarginalPrediction takes exactly the fields %r" % (_MPRED_FIELDS,))
        self.__dict__.update(fields)

    def __repr__(self):
        return "MarginalPrediction(rows=%d, chains=%d, draws=%d%s)" % (self.estimate.size, self.chains, self.draws, "" if self.weights is None else ", weighted")

    @property
    def rb_share(self):
        """var_within / sd^2 (NaN where sd is 0)"""
        with np.errstate(all="ignore"):
            return np.where(self.sd > 0, self.var_within / (self.sd * self.sd), np.nan)


def _marginal_prediction(stats, mean, var, interval, nchains, draws, thin, n_bad, weights):
    lpd = stats.get("lpd")
    return MarginalPrediction(estimate=stats["mean"], sd=stats["sd"], lower_bound=stats["lower"], upper_bound=stats["upper"], var_within=stats["var_within"],
                              pred_sd=stats["pred_sd"], pred_lower_bound=stats["pred_lower"], pred_upper_bound=stats["pred_upper"], lpd=lpd,
                              elpd=None if lpd is None else float(np.sum(lpd)), pit=stats.get("pit"), interval=interval, chains=int(nchains),
                              draws=int(draws), thin=int(thin), n_bad=int(n_bad), weights=None if weights is None else np.array(weights, dtype=np.float64),
                              mean=mean, var=var)


def marginal_predict_terms(X, y, X_new, tau2, mu, S, W=None, device=None):
    """The conditional posterior of the mean response of every row of X_new (m x q) given each of D draws phi = (tau2, mu, S, W), for one n x q
    model matrix, on the GPU (bnr_marginal_predict): dict with mean, var (D x m: eta*_j | phi, y ~ N(mean, var); a new observation has
    var + tau2) and n_bad.  tau2, mu: (D,); S, W: (D, q), W None = 0"""
    mean, var, nb = _capi.marginal_predict_raw(X, y, X_new, tau2, mu, S, W, 0 if device is None else int(device))
    return dict(mean=mean, var=var, n_bad=nb)


def mixture_score(mean, vobs, y, nchains=1, weights=None, device=None):
    """The log predictive density and the PIT of the responses y (m,) under the m mixtures of normals in the columns of the (nchains nd) x m
    matrices mean, vobs (chain k's draws in rows k nd ..) on the GPU (bnr_mixture_score): dict with lpd, pit (m,)"""
    lpd, pit = _capi.mixture_score_raw(mean, vobs, y, nchains, weights, 0 if device is None else int(device))
    return dict(lpd=lpd, pit=pit)


def device_marginal_predict(chains, nburn, nsamp, X_new, y_new=None, thin=1, weights=None, interval=95, per_draw=False, x_transform=False):
    """The prediction of the rows X_new (y_new: their observed responses, or None) with gamma integrated out over rows nburn + 1 + j thin
    (j = 0 .. ceil(nsamp / thin) - 1) of ALL the chains listed, pooled (under `weights`, the chain weights, where given), on the GPU
    (bnr_chains_marginal_predict) -> MarginalPrediction.  The per-draw mean and var stay on the device unless per_draw=True asks for them."""
    chains = list(chains)
    thin, nd = _capi.mloo_thin_draws(nsamp, thin)
    p_lo, p_hi = _loo_interval_probs(interval)
    xi = _new_rows(X_new, x_transform, chains[0].q, y_new)
    out, dm, dv, nb = _capi.chains_marginal_predict(chains, nburn + 1, nsamp, _dense_rows(xi), y_new, thin, weights, p_lo, p_hi, per_draw)
    return _marginal_prediction(dict(zip(_capi.MPRED_SUMMARY_FIELDS, out)), dm, dv, interval, len(chains), nd * len(chains), thin, nb, weights)


def _host_marginal_predict(states, X, y, X_new, y_new, nburn, nsamp, thin=1, weights=None, interval=95, per_draw=False):
    """device_marginal_predict restated in numpy over the fetched tables of the same chains, the training X (n x q), y and the dense new rows
    X_new (m x q)"""
    states = list(states)
    thin, nd = _capi.mloo_thin_draws(nsamp, thin)
    p_lo, p_hi = _loo_interval_probs(interval)
    t2, mu, S, W = _host_marginal_draws(states, nburn, nsamp, thin)
    mean, var, nb = _host_predict_terms(X, y, X_new, t2, mu, S, W)
    vobs = var + t2[:, None]
    K = len(states)
    eta = _host_mixture_summary(mean, var, K, weights, p_lo, p_hi)
    obs = _host_mixture_summary(mean, vobs, K, weights, p_lo, p_hi)
    stats = dict(mean=eta["mean"], sd=eta["sd"], var_within=eta["var_within"], lower=eta["lower"], upper=eta["upper"], pred_sd=obs["sd"],
                 pred_lower=obs["lower"], pred_upper=obs["upper"])
    if y_new is not None:
        stats.update(_host_mixture_score(mean, vobs, y_new, K, weights))
    return _marginal_prediction(stats, mean if per_draw else None, var if per_draw else None, interval, K, nd * K, thin, nb, weights)


def MarginalPredict(results, X=None, y=None, X_new=None, y_new=None, x_transform=True):
    """The accessor of a fit's prediction with gamma integrated out -> MarginalPrediction: the GPU's numbers when the fit carried them
    (marginal_predict=True), otherwise restated on the host over results.state (needs return_state=True, the training X, y and the new rows X_new;
    chain 1's window, every draw)."""
    if results.marginal_prediction is not None:
        return results.marginal_prediction
    if results.state is None or X is None or y is None or X_new is None:
        raise ValueError("MarginalPredict needs Fit(..., marginal_predict=True), or the state table (return_state=True) together with the training X, y "
                         "and the new rows")
    q = results.state["gamma"].shape[1]
    xi = _new_rows(X, x_transform, q, y)
    xn = _new_rows(X_new, x_transform, q, y_new)
    return _host_marginal_predict([results.state], _dense_rows(xi), y, _dense_rows(xn), y_new, results.burn_in, results.sampled)


# ------------------------------------------------------------------------------------------ chain placement
def _dist():
    """torch.distributed if THE CALLER has imported and initialised it, else None.  Never imports torch itself: a process group can only
    exist if the caller imported torch already, and importing it here would map the torch wheel's own libamdhip64 in front of
    libbnr_hip.so's (/opt/rocm) in a process that has not created a chain yet -- the load-order guard of _capi.lib() then refuses to run."""
    import sys
    dist = sys.modules.get("torch.distributed")
    try:
        if dist is not None and dist.is_available() and dist.is_initialized():
            return dist
    except Exception:
        pass
    return None


def _rank_world():
    d = _dist()
    return (d.get_rank(), d.get_world_size()) if d else (0, 1)


def local_chain_ids(num_chains):
    """Chains c = 1..num_chains are sharded round-robin over ranks (the reference's pmap, gibbs.jl:946)."""
    rank, world = _rank_world()
    return [c for c in range(1, num_chains + 1) if (c - 1) % world == rank]


def _default_device():
    import os
    return int(os.environ.get("LOCAL_RANK", "0")) if _dist() else 0


def shared_seed(seed, draw):
    """The ONE seed of a fit: the reference draws it once and keys chain c with seed + c (gibbs.jl:739, 928).  With chains
    sharded over torch.distributed ranks the draw happens on rank 0 and is broadcast -- independent draws per rank could put
    two chains on the same stream (s_a + c_a == s_b + c_b) and would make parameters.log's seed describe rank 0 only."""
    d = _dist()
    if seed is not None and d is None:
        return int(seed)
    value = int(draw()) if seed is None else int(seed)
    if d is None:
        return value
    import torch
    use_cuda = d.get_backend() == "nccl"
    dev = torch.device("cuda", torch.cuda.current_device()) if use_cuda else torch.device("cpu")
    t = torch.tensor([value], dtype=torch.int64, device=dev)
    d.broadcast(t, src=0)
    return int(t.item())


def make_comm(device=None, force=False):
    """The communicator of this fit for the library's own exchange (bnr_rhat): None without torch.distributed; with backend
    nccl an RCCL communicator OWNED BY THE LIBRARY (rank 0's unique id travels through torch.distributed's object broadcast
    -- the only thing torch is used for here); otherwise (gloo: CPU tests, one-GPU rehearsals) a callback communicator whose
    all-gather runs over torch.distributed."""
    d = _dist()
    if d is None or (d.get_world_size() == 1 and not force):
        return None
    import torch
    rank, world = d.get_rank(), d.get_world_size()
    if d.get_backend() == "nccl":
        box = [Comm.unique_id() if rank == 0 else None]
        d.broadcast_object_list(box, src=0)
        return Comm.rccl(box[0], rank, world, torch.cuda.current_device() if device is None else device)

    def gather(send):
        t = torch.from_numpy(send)
        out = [torch.empty_like(t) for _ in range(world)]
        d.all_gather(out, t)
        return torch.stack(out).numpy()
    return Comm.callback(rank, world, gather)


def allgather_stats(local_stats, num_chains, comm=None):
    """All-gather of per-chain messages of equal width (the ESS message; 4*(q+V) doubles for split-Rhat).  local_stats:
    {chain_id: array}.  Returns (num_chains, width) in chain order on every rank.  With a library communicator (make_comm)
    the exchange is bnr_comm_allgather (RCCL owned by the library, or the host callback); without one it falls back to
    torch.distributed's all_gather (RCCL on GPUs, gloo on CPU tests)."""
    d = _dist()
    width = len(next(iter(local_stats.values()))) if local_stats else 0
    if comm is not None:
        world = comm.world
        per_rank = (num_chains + world - 1) // world
        width = int(comm.allgather(np.array([float(width)])).max())
        buf = np.zeros((per_rank, width))
        for slot, c in enumerate(sorted(local_stats)):
            buf[slot] = local_stats[c]
        allv = comm.allgather(buf.reshape(-1)).reshape(world, per_rank, width)
        return np.stack([allv[(c - 1) % world, (c - 1) // world] for c in range(1, num_chains + 1)])
    if d is None:
        return np.stack([local_stats[c] for c in range(1, num_chains + 1)])
    import torch
    rank, world = _rank_world()
    per_rank = (num_chains + world - 1) // world
    wt = torch.tensor([width], dtype=torch.int64)
    use_cuda = d.get_backend() == "nccl"
    dev = torch.device("cuda", torch.cuda.current_device()) if use_cuda else torch.device("cpu")
    wt = wt.to(dev)
    d.all_reduce(wt, op=d.ReduceOp.MAX)
    width = int(wt.item())
    buf = torch.zeros(per_rank, width, dtype=torch.float64)
    for slot, c in enumerate(sorted(local_stats)):
        buf[slot] = torch.from_numpy(np.asarray(local_stats[c], dtype=np.float64))
    buf = buf.to(dev)
    out = [torch.empty_like(buf) for _ in range(world)]
    d.all_gather(out, buf)
    allv = torch.stack(out).cpu().numpy()          # (world, per_rank, width)
    res = np.empty((num_chains, width))
    for c in range(1, num_chains + 1):
        res[c - 1] = allv[(c - 1) % world, (c - 1) // world]
    return res


class ChainSet:
    """The chains of one fit that live on this rank's GPU.  xi_weights: the model option of every chain ("log" or "reference")."""

    def __init__(self, X_new, y, R, num_chains, tot_save, seed, hyper, device=None, xi_weights="log"):
        xi_weights_code(xi_weights)
        self.num_chains = num_chains
        self.ids = local_chain_ids(num_chains)
        dev = _default_device() if device is None else device
        self.chains = {}
        for c in self.ids:                                  # X, y are uploaded once per GPU and shared by its chains
            first = next(iter(self.chains.values()), None)
            self.chains[c] = (Chain(X_new, y, R, tot_save, seed, c, device=dev, xi_weights=xi_weights, **hyper) if first is None
                              else Chain.like(first, seed, c, tot_save))
        # several chains share this GPU: they advance in lockstep, one launch per kernel for all of them (the sequential
        # panel chain of the n x n factorization is paid once per sweep of the whole group)
        self.group = Group([self.chains[c] for c in self.ids]) if len(self.chains) > 1 else None
        self.V, self.q, self.R = (next(iter(self.chains.values())).V, next(iter(self.chains.values())).q, R) if self.chains else (None, None, R)
        if self.V is None:                                  # a rank without a chain still takes part in the exchanges
            self.q = X_new.q if isinstance(X_new, XInput) else int(np.asarray(X_new).shape[1])
            self.V = int((-1 + math.sqrt(1 + 8 * self.q)) / 2)
        self.comm = make_comm(dev)

    def init_prior(self):
        for ch in self.chains.values():
            ch.init_prior()

    def run(self, first_index, nburn, total, purge_burn, prog_freq=0, callback=None):
        """run! on every local chain (in lockstep when there are several).  The rank that holds chain 1 ticks the
        progress callback (gibbs.jl:854-856)."""
        cb = callback if 1 in self.ids else None

        def tolerant(call):
            # BNR_ERR_SAMPLER_CAP (4): a rejection sampler stopped at its attempt cap somewhere in this call.  Every row was written (with the
            # capped draw's last proposal) and the table stays valid; the reference has no cap and never raises here.  A fit of 50 000
            # iterations must not die of one such draw: warn once per call and go on -- counters()['sampler_cap'] keeps the total.
            try:
                call()
            except _capi.BnrError as e:
                if getattr(e, "code", None) == _capi.BNR_ERR_SAMPLER_CAP:
                    import warnings
                    warnings.warn("libbnr_hip: a rejection sampler hit its attempt cap during rows %d..%d (the rows were written; see counters()['sampler_cap'])" % (first_index, total), RuntimeWarning)
                else:
                    raise

        if self.group is not None:
            tolerant(lambda: self.group.run(first_index, nburn, total, purge_burn, prog_freq, cb))
        else:
            for c in self.ids:
                tolerant(lambda c=c: self.chains[c].run(first_index, nburn, total, purge_burn, prog_freq, cb if c == 1 else None))

    def rhat(self, first_row, nsamp):
        """split-Rhat over ALL chains of the fit for gamma (q) then xi (V) (return_psrf_VOI, gibbs.jl:771-789)."""
        return _capi.rhat([self.chains[c] for c in self.ids], self.num_chains, self.comm, first_row - 1, nsamp, self.V, self.q)

    def ess(self, first_row, nsamp, max_lag=None):
        """Bulk effective sample size over ALL chains of the fit for gamma (q) then xi (V) -- an addition to the reference
        (split chains + Geyer's sequence, as Stan / MCMCDiagnosticTools.ess); same exchange pattern as rhat()."""
        max_lag = min(250, nsamp // 4) if max_lag is None else max_lag
        local = {c: ch.ess_stats(first_row, nsamp, max_lag) for c, ch in self.chains.items()}
        allst = allgather_stats(local, self.num_chains, self.comm)
        e = ess_from_stats(allst, nsamp, max_lag)
        return e[:self.q], e[self.q:]

    @staticmethod
    def _V_from_width(npar):
        # npar = q + V = V(V+3)/2
        return int(round((-3 + math.sqrt(9 + 8 * npar)) / 2))

    def close(self):
        if self.group is not None:
            self.group.close()
        for ch in self.chains.values():
            ch.close()
        if self.comm is not None:
            self.comm.close()
            self.comm = None


# ------------------------------------------------------------------------------------------ chain driver
def initialize_and_run(X, y, c, total, V, R, eta, zeta, iota, aDelta, bDelta, nu, seed, prog_freq=0, purge_burn=None,
                       nsamp=None, callback=None, device=0):
    """initialize_and_run! (gibbs.jl:822-846) for ONE chain c; `seed` replaces the reference's rng argument
    (stream = seed + c).  Returns the Chain handle (the device-resident state table)."""
    tot_save = total if purge_burn is None else nsamp + purge_burn
    ch = Chain(X, y, R, tot_save, seed, c, device=device, eta=eta, zeta=zeta, iota=iota, aDelta=aDelta, bDelta=bDelta, nu=nu)
    ch.init_prior()
    nburn = total - nsamp
    run(ch, 2, nburn, total, purge_burn, prog_freq, callback if c == 1 else None)
    return ch


def run(chain, first_index, nburn, total, purge_burn=None, prog_freq=0, callback=None):
    """run! (gibbs.jl:849-864) on an existing chain."""
    return chain.run(first_index, nburn, total, purge_burn, prog_freq, callback)


def return_psrf_VOI(chainset, nburn, nsamp, fetch_state=True, summary_interval=None):
    """gibbs.jl:771-789: PSRF of gamma and xi over rows nburn+1..nburn+nsamp of every chain + chain 1's table.
    fetch_state=False leaves the table on the device (the top-up loops only look at the PSRF of the intermediate
    results); summary_interval=<credible level> adds the Summary statistics of chain 1 computed on the device."""
    rg, rx = chainset.rhat(nburn + 1, nsamp)
    state, dev = None, None
    if 1 in chainset.chains:
        ch = chainset.chains[1]
        if fetch_state:
            state = new_table(ch.tot, ch.V, ch.R, dead=True)
            ch.fetch(1, ch.tot, state)
        if summary_interval is not None:
            dev = device_summary(ch, nburn, nsamp, summary_interval)
    return Results(state, rx, rg, nburn, nsamp, dev)


@dataclass(frozen=True)
class _Requests:
    """What a fit computes behind the sampling, as _fit_requests checked it and _finish takes it"""
    return_state: bool
    summary_interval: float          # the credible level of the Summary statistics from the device, or None
    ess_max_lag: int                 # None: no ESS; 0: the default lag window
    predict: tuple                   # (new rows, their y or None, interval), or None
    waic: bool
    loo: bool
    loo_r_eff: object
    pool_chains: bool
    predict_observation: bool
    pred_seed: int                   # None: the fit's seed
    loo_predict: tuple               # (training y, interval), or None
    rank_diag: bool
    edge_sel: tuple                  # (hdi_prob, fdr), or None
    node_sets: int                   # the number of top node sets, or None
    stack: bool
    edge_cov: object = None          # None, "all", or the 0-based edge indices (int32)
    marginal_loo: int = None         # the draws per chain of the marginal PSIS-LOO (marginal_loo_draws), or None
    marginal_edges: tuple = None     # (the draws per chain of the Rao-Blackwellised edge table (marginal_edges_draws), interval), or None
    marginal_predict: int = None     # the draws per chain of the Rao-Blackwellised prediction of predict_X (marginal_predict_draws), or None
    marginal_loo_predict: tuple = None   # (the draws per chain of the marginal LOO predictive checks (marginal_loo_draws), interval), or None
    marginal_stack: tuple = None     # (the draws per chain of the stacking on the marginal PSIS-LOO (marginal_loo_draws), interval), or None
    marginal_edge_cov: tuple = None  # (the draws per chain (marginal_edges_draws), "all" or the 0-based edge indices) of the Rao-Blackwellised covariance, or None


def _one_rank(option):
    """the refusal of an option that reads every chain of the fit where the chains are spread over several ranks"""
    if _rank_world()[1] > 1:
        raise ValueError("%s needs every chain of the fit on one rank: the chains are spread over %d torch.distributed ranks" % (option, _rank_world()[1]))


def _marginal_request(option, draws_option, draws, X_new, *interval):
    """The four checks that the marginal options of a fit share, in this order -> the draws per chain: every chain on one rank, the draws per
    chain (draws_option names them in the refusal), the interval where the option takes one, at most MLOO_MAX_N training rows"""
    _one_rank(option)
    draws = _positive_int(draws_option, draws)
    for level in interval:
        _loo_interval_probs(level)
    if X_new is not None and X_new.n > MLOO_MAX_N:
        raise ValueError("%s takes at most %d training rows in this version, not %d" % (option, MLOO_MAX_N, X_new.n))
    return draws


def _fit_requests(y, num_chains, X_new=None, nsamp=None, x_transform=True, return_state=True, summary_interval=None, ess_max_lag=None, predict_X=None,
                  predict_y=None, predict_interval=95, waic=False, loo=False, loo_r_eff=None, pool_chains=False, predict_observation=False,
                  pred_seed=None, loo_predict=False, rank_diagnostics=False, edge_selection=False, hdi_prob=0.95, fdr=0.05, node_sets=False,
                  top_sets=10, stack_chains=False, edge_cov=False, marginal_loo=False, marginal_loo_draws=2000, marginal_edges=False,
                  marginal_edges_draws=2000, marginal_predict=False, marginal_predict_draws=2000, marginal_edge_cov=False, marginal_stack=False, marginal_loo_predict=False):
    """The options of a fit (Fit's keywords) checked before any sampling, in this order -> _Requests.  Fit itself calls it ahead of
    parameters.log for the refusals alone, without X_new and nsamp: what needs them -- the new rows, the lag window of the rank diagnostics,
    r_eff -- is then left to generate_samples / generate_samples_dbl."""
    pred = None
    if X_new is not None:
        if predict_X is None and predict_y is not None:
            raise ValueError("predict_y needs predict_X")
        if predict_X is not None:
            pred = (_new_rows(predict_X, x_transform, X_new.q, predict_y),
                    None if predict_y is None else np.asarray(predict_y, dtype=np.float64).reshape(-1), predict_interval)
    if predict_observation and predict_X is None:
        raise ValueError("predict_observation needs predict_X")
    if pool_chains:
        _one_rank("pool_chains")
    lp = None
    if loo_predict:
        _one_rank("loo_predict")
        _loo_interval_probs(predict_interval)
        lp = (np.asarray(y, dtype=np.float64).reshape(-1), predict_interval)
    if rank_diagnostics:
        _one_rank("rank_diagnostics")
        if nsamp is not None:
            _rank_lag(nsamp, ess_max_lag if ess_max_lag else None)
    es = ntop = None
    if edge_selection:
        _one_rank("edge_selection")
        es = _edge_levels(hdi_prob, fdr)
    if node_sets:
        _one_rank("node_sets")
        ntop = _node_sets_ntop(top_sets)
    if stack_chains:
        if int(num_chains) < 2:
            raise ValueError("stack_chains needs num_chains >= 2: one chain has nothing to be weighted against")
        if int(num_chains) > STACK_MAX_CHAINS:
            raise ValueError("stack_chains takes at most %d chains" % STACK_MAX_CHAINS)
        _one_rank("stack_chains")
    ec = _edge_cov_cols(edge_cov, None if X_new is None else X_new.V)
    if ec is not None:
        _one_rank("edge_cov")
    ml = me = mec = mp_ = mlp = mst = None
    if marginal_loo:
        ml = _marginal_request("marginal_loo", "marginal_loo_draws", marginal_loo_draws, X_new)
    if marginal_edges:
        me = (_marginal_request("marginal_edges", "marginal_edges_draws", marginal_edges_draws, X_new, predict_interval), predict_interval)
    mc = _edge_cov_cols(marginal_edge_cov, None if X_new is None else X_new.V)
    if mc is not None:
        mec = (_marginal_request("marginal_edge_cov", "marginal_edges_draws", marginal_edges_draws, X_new), mc)
    if marginal_predict:
        if predict_X is None:
            raise ValueError("marginal_predict needs predict_X")
        mp_ = _marginal_request("marginal_predict", "marginal_predict_draws", marginal_predict_draws, X_new, predict_interval)
    if marginal_loo_predict:
        mlp = (_marginal_request("marginal_loo_predict", "marginal_loo_draws", marginal_loo_draws, X_new, predict_interval), predict_interval)
    if marginal_stack:
        if int(num_chains) < 2:
            raise ValueError("marginal_stack needs num_chains >= 2: one chain has nothing to be weighted against")
        if int(num_chains) > STACK_MAX_CHAINS:
            raise ValueError("marginal_stack takes at most %d chains" % STACK_MAX_CHAINS)
        mst = (_marginal_request("marginal_stack", "marginal_loo_draws", marginal_loo_draws, X_new, predict_interval), predict_interval)
    if X_new is not None:
        _capi.r_eff_array(loo_r_eff, X_new.n)
    return _Requests(return_state, summary_interval, ess_max_lag, pred, bool(waic), bool(loo), loo_r_eff, bool(pool_chains), bool(predict_observation),
                     pred_seed, lp, bool(rank_diagnostics), es, ntop, bool(stack_chains), ec, ml, me, mp_, mlp, mst, marginal_edge_cov=mec)


def _weighted_trace_requests(rec, every, nb, ns, req, pred_seed):
    """the summary and the prediction of a fit's requests under the chain weights of the record `rec` (Results.stacking or
    Results.marginal_stacking), each set only when it was asked for"""
    if req.summary_interval is not None:
        rec.summary = device_summary_stacked(every, rec.weights, nb, ns, req.summary_interval)
    if req.predict is not None:
        rec.prediction = device_predict_stacked(every, rec.weights, nb, ns, *req.predict, pred_seed, predict_observation=req.predict_observation)


def _weighted_edge_requests(rec, every, nb, ns, req):
    """edge_cov, marginal_edges and marginal_predict of a fit's requests under the chain weights of the record `rec`, each set only when it was
    asked for"""
    if req.edge_cov is not None:
        rec.edge_cov = device_edge_cov(every, nb, ns, None if isinstance(req.edge_cov, str) else req.edge_cov, rec.weights)
    if req.marginal_edges is not None:
        rec.marginal_edges = device_marginal_edges(every, nb, ns, _marginal_loo_thin(ns, req.marginal_edges[0]), rec.weights, req.marginal_edges[1])
    if req.marginal_predict is not None:
        rec.marginal_prediction = device_marginal_predict(every, nb, ns, req.predict[0], req.predict[1], _marginal_loo_thin(ns, req.marginal_predict),
                                                          rec.weights, req.predict[2])


# The analysis options of a fit: _fit_requests' parameters after x_transform.  Fit, generate_samples and generate_samples_dbl repeat them in
# their signatures (the documentation; tests/test_finish_host.py holds the four lists equal) and hand them on as one dict.
_ANALYSIS_OPTIONS = tuple(inspect.signature(_fit_requests).parameters)
_ANALYSIS_OPTIONS = _ANALYSIS_OPTIONS[_ANALYSIS_OPTIONS.index("x_transform") + 1:]


def _analysis_options(local):
    """the analysis options of a fit out of the locals() of a function that takes them as keywords, for _fit_requests(..., **options)"""
    return {name: local[name] for name in _ANALYSIS_OPTIONS}


def _finish(chainset, res, req, seed):
    """The Results a fit returns, from its checked requests (_Requests; seed: the fit's, which keys the predictive noise unless pred_seed does).
    By default chain 1's table (states[1], gibbs.jl:788) and/or its Summary statistics, the prediction, WAIC and PSIS-LOO from the device over
    chain 1's window, through the single-chain calls.  pool_chains: those statistics over the pooled windows of all chains of the fit (one rank
    holds them all); predict_observation: through the pooled calls as well (over chain 1 alone unless pool_chains), which add the predictive
    bounds and the PITs.  loo_predict: the LOO predictive checks (Results.loo_predictive), and Results.loo from the same call.
    rank_diag: the rank-normalised diagnostics over every chain of the fit (Results.rank_diag; ess_max_lag, where positive, is their lag window).
    edge_sel: the HDIs, sign probabilities and selected edges over every chain of the fit (Results.edge_selection).
    node_sets: the joint posterior of the node indicators over every chain of the fit (Results.node_sets).
    stack: the chain stacking over every chain of the fit (Results.stacking), with summary_interval its summary and with predict its
    prediction under the weights; what pool_chains or the default return is not changed by it.
    edge_cov: the posterior covariance of the edge coefficients over every chain of the fit (Results.edge_cov), and with stack the one under
    the stacking weights (Stacking.edge_cov).
    marginal_edge_cov: the covariance of the edge coefficients with gamma integrated out (Results.marginal_edge_cov) over chain 1's window or,
    with pool_chains, every chain's.
    marginal_loo_predict: the LOO predictive checks under the marginal PSIS weights (Results.marginal_loo_predictive) over chain 1's window or,
    with pool_chains, every chain's; a call of its own, which reads and sets nothing of the stacking record.
    marginal_stack: the chain stacking on the marginal PSIS-LOO over every chain of the fit (Results.marginal_stacking), with summary_interval,
    predict, edge_cov, marginal_edges and marginal_predict those requests under its weights; a record of its own, which reads and sets nothing
    of Results.stacking or of what pool_chains or the default return."""
    nb, ns = res.burn_in, res.sampled
    every = [chainset.chains[c] for c in chainset.ids]
    pred_seed = seed if req.pred_seed is None else req.pred_seed
    if req.stack:
        res.stacking = device_stack_chains(every, nb, ns, req.loo_r_eff)
        _weighted_trace_requests(res.stacking, every, nb, ns, req, pred_seed)
    if req.edge_cov is not None:
        res.edge_cov = device_edge_cov(every, nb, ns, None if isinstance(req.edge_cov, str) else req.edge_cov)
    if req.stack:
        _weighted_edge_requests(res.stacking, every, nb, ns, req)
    if req.marginal_stack is not None:
        res.marginal_stacking = device_marginal_stack(every, nb, ns, _marginal_loo_thin(ns, req.marginal_stack[0]), req.marginal_stack[1], req.loo_r_eff)
        _weighted_trace_requests(res.marginal_stacking, every, nb, ns, req, pred_seed)
        _weighted_edge_requests(res.marginal_stacking, every, nb, ns, req)
    if req.node_sets is not None:
        res.node_sets = device_node_sets(every, nb, ns, req.node_sets)
    if req.edge_sel is not None:
        res.edge_selection = device_edge_selection(every, nb, ns, *req.edge_sel)
    if req.rank_diag:
        res.rank_diag = device_rank_diagnostics(every, nb, ns, req.ess_max_lag if req.ess_max_lag else None)
    if req.ess_max_lag is not None:                   # collective over ranks, like the PSRF
        res.essgamma, res.essxi = chainset.ess(nb + 1, ns, req.ess_max_lag if req.ess_max_lag > 0 else None)
    if 1 not in chainset.chains:
        return res
    ch = chainset.chains[1]
    pooled = req.pool_chains or req.predict_observation        # through the pooled calls: over every chain, or over chain 1 with their extras
    chains = every if req.pool_chains else [ch]
    S = ns * len(chains)
    if req.return_state:
        res.state = new_table(ch.tot, ch.V, ch.R, dead=True)
        ch.fetch(1, ch.tot, res.state)
    if req.summary_interval is not None:
        res.summary_device = (device_summary_pooled(chains, nb, ns, req.summary_interval) if pooled
                              else device_summary(ch, nb, ns, req.summary_interval))
    if req.predict is not None:
        res.prediction = (device_predict_pooled(chains, nb, ns, *req.predict, pred_seed, predict_observation=req.predict_observation) if pooled
                          else device_predict(ch, nb, ns, *req.predict))
    if req.waic and pooled:
        lpd, pw, pit = _capi.pooled_loglik_stats(chains, nb + 1, ns, pit=True)
        res.waic = dict(_waic_from_pointwise(lpd, pw), pit_i=pit)
    elif req.waic:
        res.waic = _waic_from_pointwise(*ch.loglik_stats(nb + 1, ns))
    if req.loo_predict is not None:                   # (implies loo: both from one call)
        lp = device_loo_predict(chains, req.loo_predict[0], nb, ns, req.loo_predict[1], req.loo_r_eff)
        res.loo_predictive = lp
        res.loo = _loo_from_pointwise(lp.lpd_i, lp.elpd_loo_i, lp.pareto_k, S)
    elif req.loo:
        res.loo = _loo_from_pointwise(*(_capi.pooled_loo(chains, nb + 1, ns, req.loo_r_eff) if pooled else ch.loo(nb + 1, ns, req.loo_r_eff)), S)
    if req.marginal_loo is not None:
        res.marginal_loo = device_marginal_loo(chains, nb, ns, _marginal_loo_thin(ns, req.marginal_loo), req.loo_r_eff)
    if req.marginal_edges is not None:
        res.marginal_edges = device_marginal_edges(chains, nb, ns, _marginal_loo_thin(ns, req.marginal_edges[0]), None, req.marginal_edges[1])
    if req.marginal_edge_cov is not None:
        res.marginal_edge_cov = device_marginal_edge_cov(chains, nb, ns, _marginal_loo_thin(ns, req.marginal_edge_cov[0]),
                                                         None if isinstance(req.marginal_edge_cov[1], str) else req.marginal_edge_cov[1])
    if req.marginal_predict is not None:
        res.marginal_prediction = device_marginal_predict(chains, nb, ns, req.predict[0], req.predict[1], _marginal_loo_thin(ns, req.marginal_predict), None,
                                                          req.predict[2])
    if req.marginal_loo_predict is not None:
        res.marginal_loo_predictive = device_marginal_loo_predict(chains, nb, ns, _marginal_loo_thin(ns, req.marginal_loo_predict[0]),
                                                                  req.marginal_loo_predict[1], req.loo_r_eff)
    if (req.summary_interval is not None or req.predict is not None or req.waic or req.loo or req.loo_predict is not None
            or req.marginal_loo is not None or req.marginal_edges is not None or req.marginal_loo_predict is not None):
        res.stat_chains = len(chains)
    return res


class _Progress:
    def __init__(self, total_ticks, enabled, start=0):
        self.n, self.total, self.enabled = start, max(total_ticks, 1), enabled

    def tick(self, _done=None):
        self.n += 1
        if self.enabled:
            sys.stderr.write("\rProgress: %3d%%" % min(100, int(100 * self.n / self.total)))
            sys.stderr.flush()

    def done(self):
        if self.enabled:
            sys.stderr.write("\n")


def _normalize_purge(purge_burn, nburn):
    """gibbs.jl:930-936."""
    if purge_burn is not None and purge_burn < nburn and purge_burn != 0:
        if nburn % purge_burn != 0:
            purge_burn = purge_burn - (nburn % purge_burn)
        return purge_burn
    return None


def generate_samples(X, y, R, eta=1.01, zeta=1.0, iota=1.0, aDelta=1.0, bDelta=1.0, nu=10, nburn=30000, nsamp=20000,
                     maxburn=50000, psrf_cutoff=1.2, x_transform=True, suppress_timer=False, num_chains=2, seed=None,
                     purge_burn=None, device=None, _keep=None, return_state=True, summary_interval=None, ess_max_lag=None,
                     xi_weights="log", predict_X=None, predict_y=None, predict_interval=95, waic=False, loo=False, loo_r_eff=None,
                     pool_chains=False, predict_observation=False, pred_seed=None, loo_predict=False, rank_diagnostics=False, edge_selection=False,
                     hdi_prob=0.95, fdr=0.05, node_sets=False, top_sets=10, stack_chains=False, edge_cov=False, marginal_loo=False,
                     marginal_loo_draws=2000, marginal_edges=False, marginal_edges_draws=2000,
                     marginal_predict=False, marginal_predict_draws=2000, marginal_edge_cov=False, marginal_stack=False, marginal_loo_predict=False):
    """generate_samples! (gibbs.jl:897-1020): "traditional" scheme with PSRF-driven top-up rounds.
    xi_weights="reference" samples xi with the reference's own weight arithmetic (include/bnr_hip.h, option "xi_weights")."""
    opts = _analysis_options(locals())
    xi_weights_code(xi_weights)
    if nu < R:
        pass                                       # the reference constructs an ArgumentError without throwing it (901-902)
    elif nu == R:
        print("Warning: ν==R may give poor accuracy. Consider increasing ν")
    X_new = XInput(X, x_transform)                 # X_new of gibbs.jl:907-918: element type kept, setup_X! runs on the device
    req = _fit_requests(y, num_chains, X_new, nsamp, x_transform, **opts)       # (checked before any sampling)
    y = np.asarray(y, dtype=np.float64)
    total = nburn + nsamp
    prog_freq = 1000
    if prog_freq >= nburn:
        prog_freq = 10
    seed_eff = shared_seed(seed, lambda: random.SystemRandom().randrange(1, 2**31))     # Xoshiro() when seed===nothing; one draw per fit
    purge_burn = _normalize_purge(purge_burn, nburn)
    tot_save = total if purge_burn is None else nsamp + purge_burn
    hyper = dict(eta=eta, zeta=zeta, iota=iota, aDelta=aDelta, bDelta=bDelta, nu=nu)
    cs = ChainSet(X_new, y, R, num_chains, tot_save, seed_eff, hyper, device, xi_weights)
    if _keep is not None:
        _keep.append(cs)
    p = _Progress((total - 1) // prog_freq, not suppress_timer)
    cs.init_prior()
    cs.run(2, nburn, total, purge_burn, prog_freq, p.tick)
    p.done()
    tot_generated = nburn + nsamp
    stt = purge_burn if purge_burn is not None else nburn
    res = return_psrf_VOI(cs, stt, nsamp, fetch_state=False)
    print("%d samples generated. Max PSRF XI: %.2f. Max PSRF Gamma: %.2f" % (tot_generated, res.rhatxi.max(), res.rhatgamma.max()), file=sys.stderr)
    while (res.rhatxi.max() > psrf_cutoff or res.rhatgamma.max() > psrf_cutoff) and tot_generated < (maxburn + nsamp):
        # we want to generate nburn more samples (gibbs.jl:963-974)
        if purge_burn is not None:
            num2move = 1 if nsamp + purge_burn <= nburn else nsamp + purge_burn - nburn
        else:
            num2move = total - nburn
        tot_sze = tot_save
        print("num2move: %d nburn: %d nsamp: %d purge_burn: %s" % (num2move, nburn, nsamp, purge_burn), file=sys.stderr)
        p = _Progress((tot_generated + nburn - 1) // prog_freq, not suppress_timer, start=tot_generated // prog_freq)
        for ch in cs.chains.values():
            ch.move_rows(1, tot_sze - num2move + 1, num2move)                     # copy_table! loop :991-993
        cs.run(num2move + 1, (nburn - nsamp + num2move) if nburn > nsamp else 0,
               (num2move + nburn) if num2move > 1 else nburn, purge_burn, prog_freq, p.tick)   # run! :997-999
        p.done()
        A = (num2move + nburn) if num2move > 1 else nburn
        B = num2move
        tot_generated = tot_generated + A - B
        res = return_psrf_VOI(cs, stt, nsamp, fetch_state=False)
        print("%d samples generated. Max PSRF XI: %.3f. Max PSRF Gamma: %.3f" % (tot_generated, res.rhatxi.max(), res.rhatgamma.max()), file=sys.stderr)
    print("R = %s nu=%s nburn= %d nsamp = %d" % (R, nu, nburn, nsamp))
    print("%d samples generated. Max PSRF XI: %.3f. Max PSRF Gamma: %.3f\n" % (tot_generated, res.rhatxi.max(), res.rhatgamma.max()))
    res = _finish(cs, res, req, seed_eff)
    if _keep is None:
        cs.close()
    return res


def generate_samples_dbl(X, y, R, eta=1.01, zeta=1.0, iota=1.0, aDelta=1.0, bDelta=1.0, nu=10, mingen=10000,
                         maxgen=100000, psrf_cutoff=1.01, x_transform=True, suppress_timer=False, num_chains=2,
                         seed=None, purge_burn=None, device=None, return_state=True, summary_interval=None, ess_max_lag=None,
                         xi_weights="log", predict_X=None, predict_y=None, predict_interval=95, waic=False, loo=False, loo_r_eff=None,
                         pool_chains=False, predict_observation=False, pred_seed=None, loo_predict=False, rank_diagnostics=False, edge_selection=False,
                         hdi_prob=0.95, fdr=0.05, node_sets=False, top_sets=10, stack_chains=False, edge_cov=False, marginal_loo=False,
                         marginal_loo_draws=2000, marginal_edges=False, marginal_edges_draws=2000,
                         marginal_predict=False, marginal_predict_draws=2000, marginal_edge_cov=False, marginal_stack=False, marginal_loo_predict=False):
    """generate_samples_dbl! (gibbs.jl:1051-1198): "doubling generation" scheme.  xi_weights as for generate_samples."""
    opts = _analysis_options(locals())
    xi_weights_code(xi_weights)
    if nu == R:
        print("Warning: ν==R may give poor accuracy. Consider increasing ν")
    nburn = _julia_round(mingen / 2)
    nsamp = mingen - nburn
    X_new = XInput(X, x_transform)
    req = _fit_requests(y, num_chains, X_new, nsamp, x_transform, **opts)       # (checked before any sampling)
    y = np.asarray(y, dtype=np.float64)
    total = nburn + nsamp
    prog_freq = 1000
    if prog_freq >= nburn:
        prog_freq = 10
    seed_eff = shared_seed(seed, lambda: random.SystemRandom().randrange(1, 2**31))
    purge_burn = _normalize_purge(purge_burn, nburn)
    tot_save = total if purge_burn is None else nsamp + purge_burn
    hyper = dict(eta=eta, zeta=zeta, iota=iota, aDelta=aDelta, bDelta=bDelta, nu=nu)
    cs = ChainSet(X_new, y, R, num_chains, tot_save, seed_eff, hyper, device, xi_weights)
    p = _Progress((total - 1) // prog_freq, not suppress_timer)
    cs.init_prior()
    cs.run(2, nburn, total, purge_burn, prog_freq, p.tick)
    p.done()
    tot_generated = nburn + nsamp
    tot_samples = nsamp
    stt = purge_burn if purge_burn is not None else nburn
    res = return_psrf_VOI(cs, stt, nsamp, fetch_state=False)
    print("%d samples generated. Max PSRF XI: %.3f. Max PSRF Gamma: %.3f" % (tot_generated, res.rhatxi.max(), res.rhatgamma.max()), file=sys.stderr)

    def _bad(r):
        return (r.rhatxi.max() > psrf_cutoff or r.rhatgamma.max() > psrf_cutoff or np.isnan(r.rhatxi.max()) or np.isnan(r.rhatgamma.max()))

    while _bad(res) and tot_generated < maxgen:
        halfburn = _julia_round(mingen / 2)
        num2move = tot_samples                       # gibbs.jl:1143
        tot_samples = tot_samples + halfburn
        nsamp = tot_samples
        tot_sze = tot_save
        tot_save = tot_samples + halfburn
        print("num2move: %d nburn: %d nsamp: %d tot_save: %d first_index: %d" % (num2move, nburn, nsamp, tot_save, num2move + 1), file=sys.stderr)
        p = _Progress((tot_save - 1) // prog_freq, not suppress_timer, start=_julia_round((num2move + 1) / prog_freq))
        for ch in cs.chains.values():
            # new table of tot_save rows + copy_table!(state, states[c], 1:num2move, tail)  (gibbs.jl:1164-1172)
            ch.move_rows(1, tot_sze - num2move + 1, num2move)
            ch.resize(tot_save)
        cs.run(num2move + 1, 0, tot_save, purge_burn, prog_freq, p.tick)           # run! :1176-1178
        p.done()
        tot_generated = tot_generated + mingen
        res = return_psrf_VOI(cs, stt, nsamp, fetch_state=False)
        print("%d samples generated. Max PSRF XI: %.3f. Max PSRF Gamma: %.3f" % (tot_generated, res.rhatxi.max(), res.rhatgamma.max()), file=sys.stderr)
    print("\nR = %s nu=%s nburn= %d nsamp = %d\n" % (R, nu, nburn, nsamp))
    print("%d samples generated. Max PSRF XI: %.4f. Max PSRF Gamma: %.4f" % (tot_generated, res.rhatxi.max(), res.rhatgamma.max()))
    res = _finish(cs, res, req, seed_eff)
    cs.close()
    return res


def Fit(X, y, R, eta=1.01, V=30, zeta=1.0, iota=1.0, aDelta=1.0, bDelta=1.0, nu=10, nburn=30000, nsamples=20000,
        mingen=0, maxgen=0, psrf_cutoff=1.01, x_transform=True, suppress_timer=False, num_chains=2, seed=None,
        purge_burn=None, filename="parameters.log", device=None, return_state=True, summary_interval=None, ess_max_lag=None,
        xi_weights="log", predict_X=None, predict_y=None, predict_interval=95, waic=False, loo=False, loo_r_eff=None,
        pool_chains=False, predict_observation=False, pred_seed=None, loo_predict=False, rank_diagnostics=False, edge_selection=False,
        hdi_prob=0.95, fdr=0.05, node_sets=False, top_sets=10, stack_chains=False, edge_cov=False, marginal_loo=False,
        marginal_loo_draws=2000, marginal_edges=False, marginal_edges_draws=2000,
        marginal_predict=False, marginal_predict_draws=2000, marginal_edge_cov=False, marginal_stack=False, marginal_loo_predict=False):
    """Fit! (gibbs.jl:725-751).  The `V` keyword is accepted and ignored, as in the reference.
    Extensions: summary_interval=95 computes Summary's statistics on the GPU (Results.summary_device);
    return_state=False then leaves the (large) state table on the device and frees it; ess_max_lag=0 (default lag
    window) or a lag count adds bulk effective sample sizes over all chains (Results.essgamma / essxi);
    xi_weights="reference" samples xi with the reference's own weight arithmetic, under/overflow included (the default "log" never
    under/overflows; include/bnr_hip.h, option "xi_weights"); predict_X (new rows in the x_transform format of X), predict_y (their observed
    responses, optional) and predict_interval compute the posterior of the mean response of those rows on the GPU (Results.prediction, see
    Predict), waic=True the WAIC of the training rows (Results.waic, see WAIC), loo=True their PSIS-LOO (Results.loo, see LOO; loo_r_eff: the
    relative efficiencies, a scalar or one per training row, default 1) -- over chain 1's window, as Summary.  pool_chains=True computes
    summary_interval, predict_X, waic and loo over the pooled windows of ALL chains of the fit instead (num_chains x nsamples draws; every chain
    must live on this rank; Results.stat_chains says how many were covered); predict_observation=True adds to the prediction the predictive
    interval of a new observation and, with predict_y, the PIT (BNRPrediction.pred_lower_bound / pred_upper_bound / pit), its noise keyed by
    pred_seed (default: the fit's seed).  loo_predict=True adds the LOO predictive checks of the training rows (Results.loo_predictive, see
    LOOPredict: PSIS-weighted mean, sd, PIT and a predict_interval% interval of every row, RMSE, R2, coverage); it implies loo (Results.loo comes
    from the same device call), honours pool_chains and loo_r_eff, and like pool_chains needs every chain of the fit on this rank.
    rank_diagnostics=True adds the rank-normalised R-hat, bulk / tail ESS and MCSE over every chain of the fit, computed on the GPU from the
    resident traces (Results.rank_diag, see RankDiagnose; ess_max_lag, where positive, is their lag window); every chain must live on this rank.
    edge_selection=True adds the hdi_prob highest-density interval, the median and the sign probabilities of every edge coefficient and node
    indicator, and the largest set of edges whose expected false sign rate stays within fdr, computed on the GPU from the resident traces over
    every chain of the fit (Results.edge_selection, see EdgeSelect); every chain must live on this rank.
    node_sets=True adds the joint posterior of the node indicators: the co-inclusion matrix, the distribution of the number of selected nodes,
    the top_sets most probable node sets (the first is the MAP model) and the distribution of the number of active latent dimensions, computed
    on the GPU from the resident traces over every chain of the fit (Results.node_sets, see NodeSets); every chain must live on this rank.
    stack_chains=True (num_chains >= 2, every chain on this rank) adds the chain stacking of Yao, Vehtari & Gelman (2022) for chains that do
    not mix: every chain's own PSIS-LOO, the chain weights that maximise the leave-one-out log score of the mixture, and -- with
    summary_interval / predict_X -- the Summary statistics and the prediction under those weights (Results.stacking, see Stacking); what
    pool_chains or the default return is unchanged.
    edge_cov=True (or an array of 0-based edge indices, or a list of 1-based (node1, node2) pairs) adds the posterior covariance matrix of
    those edge coefficients -- vcov(fit) -- computed on the GPU from the resident traces over every chain of the fit (Results.edge_cov, see
    EdgeCov: sd, corr, contrast(C) for intervals on linear combinations of edges, top_pairs); with stack_chains=True also the covariance under
    the stacking weights (Results.stacking.edge_cov); every chain must live on this rank.
    marginal_loo=True adds PSIS-LOO with the edge coefficients integrated out (Results.marginal_loo, see MarginalLOO and device_marginal_loo):
    the importance ratios 1 / p(y_i | y_-i, tau2, mu, u, lambda, S) instead of LOO's 1 / p(y_i | gamma, mu, tau2), whose Pareto k-hat is above
    the threshold on most rows where q >> n.  It uses every thin-th row of the window, thin = ceil(nsamples / marginal_loo_draws) (default 2000
    draws per chain), over chain 1's window or every chain's with pool_chains=True, honours loo_r_eff, needs every chain of the fit on this rank
    and at most 2048 training rows; what loo, loo_predict and stack_chains return is not changed by it.
    marginal_edges=True adds the edge table with gamma integrated out (Results.marginal_edges, see MarginalEdges and device_marginal_edges): mean,
    sd, the predict_interval% interval and the sign probabilities of every edge coefficient from the mixture of its conditional normals
    N(m_e, v_e | tau2, mu, u, lambda, S) over the draws, free of the within-draw noise of the gamma draws.  Draws, chains and limits as for
    marginal_loo (marginal_edges_draws, default 2000 per chain); with stack_chains=True also under the stacking weights over every chain
    (Results.stacking.marginal_edges).  Every other field of the Results is what it is without it.
    marginal_edge_cov=True (or an array of 0-based edge indices, or a list of 1-based (node1, node2) pairs, as edge_cov takes them) adds the
    covariance matrix of those edge coefficients with gamma integrated out (Results.marginal_edge_cov, see MarginalEdgeCov and
    device_marginal_edge_cov): edge_cov's matrix without the within-draw noise of the gamma draws, split into `within` and `between`, with
    EdgeCov's sd, corr, contrast(C) and top_pairs.  Draws (marginal_edges_draws), chains and limits as for marginal_edges; the covariance under
    stacking weights is device_marginal_edge_cov(chains, ..., weights=...).  Every other field of the Results is what it is without it.
    marginal_predict=True adds the prediction of predict_X with gamma integrated out (Results.marginal_prediction, see MarginalPrediction and
    device_marginal_predict): per new row the mean, sd and interval of the mixture of N(mean_j, var_j | tau2, mu, u, lambda, S) over the draws, the
    predictive sd and interval of a new observation and, with predict_y, lpd / elpd and the PIT -- no predictive noise is drawn, so pred_seed plays
    no part.  It needs predict_X; predict_y and predict_interval are used as given.  Draws, chains and limits as for marginal_loo
    (marginal_predict_draws, default 2000 per chain); with stack_chains=True also under the stacking weights over every chain
    (Results.stacking.marginal_prediction).  Every other field of the Results is what it is without it.
    marginal_loo_predict=True adds the LOO predictive checks of the training rows under the marginal PSIS weights (Results.marginal_loo_predictive,
    see MarginalLOOPredict and device_marginal_loo_predict): what loo_predict returns -- the leave-one-out mean, sd, PIT and predict_interval%
    interval of every row, RMSE, R2, coverage and the KS distance of the PITs -- from the weights of marginal_loo, which stay below the k-hat
    threshold where loo_predict's do not, with the kernels on the device-resident matrices; its field `loo` is the dict of marginal_loo from the
    same call.  Draws (marginal_loo_draws), chains, loo_r_eff and limits as for marginal_loo; marginal_loo=True beside it still makes its own
    call.  Every other field of the Results is what it is without it.
    marginal_stack=True adds the chain stacking on the marginal PSIS-LOO (Results.marginal_stacking, see MarginalStack and
    device_marginal_stack): stack_chains' weights, per-chain and stacked scores from every chain's marginal PSIS-LOO over its own
    marginal_loo_draws draws, all chains in one factorization pass, and the leave-one-out mean, sd, PIT and predict_interval% interval of the
    stacked mixture with their coverage and KS distance.  With summary_interval, predict_X, edge_cov, marginal_edges or marginal_predict the
    record also holds those under its weights.  It needs 2 to 32 chains on one rank and at most 2048 training rows; stack_chains=True beside
    it fills Results.stacking as before, independently.  Every other field of the Results is what it is without it.
    parameters.log keeps the reference's lines only."""
    opts = _analysis_options(locals())
    xi_weights_code(xi_weights)
    _fit_requests(y, num_chains, **opts)
    seed = shared_seed(seed, lambda: random.randrange(1, 55556))          # sample(1:55555) :739; drawn on rank 0, the same on every rank
    if _rank_world()[0] == 0 and filename:
        with open(filename, "w") as f:
            f.write("BayesianNetworkRegression.jl Fit! function\n")
            f.write(datetime.datetime.now().strftime("%Y-%m-%d %H:%M:%S.%f")[:-3] + "\n")
            f.write(CITATION)
            f.write("\n\nParameters:\n")
            f.write("R=%s, η=%s, ζ=%s, ι=%s, aΔ=%s, bΔ=%s, ν=%s, nburn=%s, nsamples=%s, \n" % (R, eta, zeta, iota, aDelta, bDelta, nu, nburn, nsamples))
            f.write("mingen=%s, maxgen=%s, psrf_cutoff=%s, \n" % (mingen, maxgen, psrf_cutoff))
            f.write("x_transform=%s, suppress_timer=%s, num_chains=%s, purge_burn=%s \n" % (str(x_transform).lower(), str(suppress_timer).lower(), num_chains, "nothing" if purge_burn is None else purge_burn))
            f.write("seed=%s" % seed)
    if mingen > 0 and maxgen > 0:
        return generate_samples_dbl(X, y, R, eta=eta, zeta=zeta, iota=iota, aDelta=aDelta, bDelta=bDelta, nu=nu, mingen=mingen,
                                    maxgen=maxgen, psrf_cutoff=psrf_cutoff, x_transform=x_transform, suppress_timer=suppress_timer,
                                    num_chains=num_chains, seed=seed, purge_burn=purge_burn, device=device, xi_weights=xi_weights, **opts)
    return generate_samples(X, y, R, eta=eta, zeta=zeta, iota=iota, aDelta=aDelta, bDelta=bDelta, nu=nu, nburn=nburn, nsamp=nsamples,
                            maxburn=nburn + nsamples, psrf_cutoff=psrf_cutoff, x_transform=x_transform,
                            suppress_timer=suppress_timer, num_chains=num_chains, seed=seed, purge_burn=purge_burn, device=device,
                            xi_weights=xi_weights, **opts)
