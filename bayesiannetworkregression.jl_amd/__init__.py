"""MI355X-native Gibbs hot path of BayesianNetworkRegression.jl behind the reference's Fit!/generate_samples! API.

Compute lives in libbnr_hip.so (hand-written gfx950 HIP kernels, C ABI in include/bnr_hip.h); this package is the
host-side mirror of the reference interface."""
from ._build import build, LIB, MLOO_LIB, MEDGE_LIB, MPRED_LIB, MCHECK_LIB, MSTACK_LIB, MCOV_LIB                                # noqa: F401
from ._capi import BnrError, Chain, Comm, Group, XInput, device_count, device_synchronize, runtime_version, ess_from_stats, new_table, rhat_from_stats, lib, mloo_lib, medge_lib, mpred_lib, mcheck_lib, mstack_lib, mcov_lib, EXPORTS   # noqa: F401
from .api import (BNRPrediction, BNRSummary, ChainSet, Fit, LOO, LOOPredict, LOOPredictive, Predict, Results, Summary, WAIC, create_lower_tri, device_predict,   # noqa: F401
                  device_summary, device_predict_pooled, device_summary_pooled, generate_samples, psis_loo, psis_weights, device_loo_predict,
                  generate_samples_dbl, initialize_and_run, lower_triangle, return_psrf_VOI, run, setup_X,
                  allgather_stats, local_chain_ids, make_comm, shared_seed, RankDiagnose, RankDiagnostics, device_rank_diagnostics, rank_normalize,
                  EdgeSelect, EdgeSelection, device_edge_selection, hdi, NodeSets, device_node_sets, inclusion,
                  Stacking, ChainStacking, stacking_weights, wquantile, device_stack_chains, device_summary_stacked, device_predict_stacked,
                  EdgeCov, cov, device_edge_cov, MarginalLOO, marginal_loglik, device_marginal_loo,
                  MarginalEdges, marginal_gamma, mixture_summary, device_marginal_edges,
                  MarginalEdgeCov, marginal_gamma_cov, device_marginal_edge_cov,
                  MarginalPredict, MarginalPrediction, marginal_predict_terms, mixture_score, device_marginal_predict,
                  MarginalLOOPredict, MarginalLOOPredictive, weighted_mixture, device_marginal_loo_predict,
                  MarginalStack, MarginalStacking, stacked_mixture, device_marginal_stack)
from .synthetic import make_synthetic                             # noqa: F401
