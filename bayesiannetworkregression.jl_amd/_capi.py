"""ctypes binding of include/bnr_hip.h (libbnr_hip.so).  No torch types cross this boundary.

The HIP library is the ONLY compute path of the package: if the shared object is missing or a call fails the
error is raised, never papered over with a CPU fallback."""
import ctypes as C
import functools
import os

import numpy as np

from ._build import LIB, MARGINAL_LIBS

BNR_OK, BNR_ERR_BAD_ARG, BNR_ERR_HIP, BNR_ERR_CHOLESKY, BNR_ERR_SAMPLER = 0, 1, 2, 3, 4
BNR_ERR_SAMPLER_CAP = BNR_ERR_SAMPLER
ERRORS = {1: "bad argument", 2: "HIP error", 3: "Cholesky failed after jitter", 4: "sampler attempt cap"}


class BnrError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("libbnr_hip: %s (status %d: %s)" % (msg, code, ERRORS.get(code, "?")))
        self.code = code


class Hyper(C.Structure):
    _fields_ = [(k, C.c_double) for k in ("eta", "zeta", "iota", "aDelta", "bDelta", "nu")]


PROGRESS_CB = C.CFUNCTYPE(None, C.c_void_p, C.c_int64)
ALLGATHER_CB = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_int64)


class UniqueId(C.Structure):
    _fields_ = [("bytes", C.c_char * 128)]


class ChainView(C.Structure):
    """bnr_chain_view of include/bnr_hip.h: the device side of a chain, for a companion library"""
    _fields_ = ([(k, C.c_int32) for k in ("device", "n", "n_pad", "V", "R", "q", "q_pad", "tot", "rowlen", "o_tau2", "o_mu", "o_lam", "o_u", "o_gamma",
                                          "o_S", "ldx")]
                + [(k, C.c_void_p) for k in ("X", "y", "ek", "el", "trace")])
_dp = C.c_void_p
_lib = None
_mloo = _medge = _mpred = _mcheck = _mstack = _mcov = None       # the marginal libraries once loaded (marginal_lib sets them)

_SIGS = {
    "bnr_abi_version": (C.c_int, []),
    "bnr_last_error": (C.c_char_p, []),
    "bnr_device_count": (C.c_int, [C.POINTER(C.c_int)]),
    "bnr_device_synchronize": (C.c_int, [C.c_int32]),
    "bnr_runtime_version": (C.c_int, [C.POINTER(C.c_int)]),
    "bnr_chain_create": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, _dp, _dp, C.POINTER(Hyper), C.c_uint64, C.c_int32,
                                   C.c_int32, C.c_int32, C.POINTER(C.c_void_p)]),
    "bnr_chain_create_typed": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, _dp, C.c_int32, _dp, C.POINTER(Hyper), C.c_uint64, C.c_int32,
                                         C.c_int32, C.c_int32, C.POINTER(C.c_void_p)]),
    "bnr_chain_create_from_matrices": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_void_p), C.c_int32, _dp, C.POINTER(Hyper),
                                                 C.c_uint64, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_void_p)]),
    "bnr_chain_create_like": (C.c_int, [C.c_void_p, C.c_uint64, C.c_int32, C.c_int32, C.POINTER(C.c_void_p)]),
    "bnr_chain_destroy": (C.c_int, [C.c_void_p]),
    "bnr_chain_init_prior": (C.c_int, [C.c_void_p]),
    "bnr_chain_run": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, PROGRESS_CB, C.c_void_p,
                                C.POINTER(C.c_int32)]),
    "bnr_chain_run_async": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    "bnr_chain_sync": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32)]),
    "bnr_chain_prepare": (C.c_int, [C.c_void_p]),
    "bnr_group_prepare": (C.c_int, [C.c_void_p]),
    "bnr_group_create": (C.c_int, [C.POINTER(C.c_void_p), C.c_int32, C.POINTER(C.c_void_p)]),
    "bnr_group_destroy": (C.c_int, [C.c_void_p]),
    "bnr_group_run": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, PROGRESS_CB, C.c_void_p,
                                C.POINTER(C.c_int32)]),
    "bnr_group_set_option": (C.c_int, [C.c_void_p, C.c_char_p, C.c_int64]),
    "bnr_group_last_timing": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(C.c_double), C.POINTER(C.c_int64)]),
    "bnr_gibbs_step": (C.c_int, [C.c_void_p, C.c_int32, C.c_int64]),
    "bnr_chain_get_iter": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64)]),
    "bnr_chain_set_iter": (C.c_int, [C.c_void_p, C.c_int64]),
    "bnr_chain_fetch": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32] + [_dp] * 11),
    "bnr_chain_load": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32] + [_dp] * 11),
    "bnr_chain_move_rows": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32]),
    "bnr_chain_resize": (C.c_int, [C.c_void_p, C.c_int32]),
    "bnr_chain_rhat_stats": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, _dp]),
    "bnr_chain_summary": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _dp, _dp, _dp, _dp]),
    "bnr_chain_predict": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, _dp, C.c_int32, _dp, C.c_int32, C.c_int32] + [_dp] * 5),
    "bnr_chain_predict_from_matrices": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_void_p), C.c_int32, _dp, C.c_int32,
                                                  C.c_int32] + [_dp] * 5),
    "bnr_chain_loglik_stats": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, _dp, _dp]),
    "bnr_chain_loo": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, _dp, _dp, _dp, _dp]),
    "bnr_psis_loo": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, _dp, _dp, _dp, _dp, _dp]),
    "bnr_chains_summary": (C.c_int, [C.POINTER(C.c_void_p), C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _dp, _dp, _dp, _dp]),
    "bnr_chains_predict": (C.c_int, [C.POINTER(C.c_void_p), C.c_int32, C.c_int32, C.c_int32, C.c_int32, _dp, C.c_int32, _dp, C.c_int32, C.c_int32]
                           + [_dp] * 5 + [C.c_uint64] + [_dp] * 3),
    "bnr_chains_predict_from_matrices": (C.c_int, [C.POINTER(C.c_void_p), C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_void_p), C.c_int32,
                                                   _dp, C.c_int32, C.c_int32] + [_dp] * 5 + [C.c_uint64] + [_dp] * 3),
    "bnr_chains_loglik_stats": (C.c_int, [C.POINTER(C.c_void_p), C.c_int32, C.c_int32, C.c_int32, _dp, _dp, _dp]),
    "bnr_chains_loo": (C.c_int, [C.POINTER(C.c_void_p), C.c_int32, C.c_int32, C.c_int32, _dp, _dp, _dp, _dp]),
    "bnr_chain_loo_predict": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, _dp, C.c_double, C.c_double] + [_dp] * 8),
    "bnr_chains_loo_predict": (C.c_int, [C.POINTER(C.c_void_p), C.c_int32, C.c_int32, C.c_int32, _dp, C.c_double, C.c_double] + [_dp] * 8),
    "bnr_psis_weights": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, _dp, _dp, _dp, _dp, _dp]),
    "bnr_chain_rank_diag": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32] + [_dp] * 6),
    "bnr_chains_rank_diag": (C.c_int, [C.POINTER(C.c_void_p), C.c_int32, C.c_int32, C.c_int32, C.c_int32] + [_dp] * 6),
    "bnr_rank_normalize": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, _dp, _dp, _dp]),
    "bnr_host_ndtri": (C.c_double, [C.c_double]),
    "bnr_chain_hdi": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, _dp] + [_dp] * 5),
    "bnr_chains_hdi": (C.c_int, [C.POINTER(C.c_void_p), C.c_int32, C.c_int32, C.c_int32, C.c_int32, _dp] + [_dp] * 5),
    "bnr_hdi": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, _dp, C.c_int32, _dp] + [_dp] * 5),
    "bnr_chain_inclusion": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32] + [_dp] * 6),
    "bnr_chains_inclusion": (C.c_int, [C.POINTER(C.c_void_p), C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32] + [_dp] * 6),
    "bnr_inclusion": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, _dp, C.c_int32] + [_dp] * 6),
    "bnr_stacking_weights": (C.c_int, [C.c_int32, C.c_int32, _dp, C.c_int32, C.c_double, _dp, C.POINTER(C.c_double), C.POINTER(C.c_double),
                                       C.POINTER(C.c_int32)]),
    "bnr_chains_stack": (C.c_int, [C.POINTER(C.c_void_p), C.c_int32, C.c_int32, C.c_int32, _dp, C.c_int32, C.c_double, _dp, _dp, _dp, _dp,
                                   C.POINTER(C.c_double), C.POINTER(C.c_int32)]),
    "bnr_chains_wsummary": (C.c_int, [C.POINTER(C.c_void_p), C.c_int32, _dp, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _dp, _dp, _dp, _dp]),
    "bnr_chains_wpredict": (C.c_int, [C.POINTER(C.c_void_p), C.c_int32, _dp, C.c_int32, C.c_int32, C.c_int32, _dp, C.c_int32, _dp, C.c_int32, C.c_int32]
                            + [_dp] * 4 + [C.c_uint64] + [_dp] * 2),
    "bnr_wquantile": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, _dp, _dp, C.c_int32, C.c_int32, _dp, _dp, _dp]),
    "bnr_chain_cov": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, _dp, _dp, _dp]),
    "bnr_chains_cov": (C.c_int, [C.POINTER(C.c_void_p), C.c_int32, _dp, C.c_int32, C.c_int32, C.c_int32, _dp, _dp, _dp]),
    "bnr_cov": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, _dp, _dp, _dp, _dp]),
    "bnr_chain_device_view": (C.c_int, [C.c_void_p, C.POINTER(ChainView)]),
    "bnr_set_last_error": (C.c_int, [C.c_int, C.c_char_p]),
    "bnr_comm_unique_id": (C.c_int, [C.POINTER(UniqueId)]),
    "bnr_comm_create_rccl": (C.c_int, [C.POINTER(UniqueId), C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_void_p)]),
    "bnr_comm_create_callback": (C.c_int, [C.c_int32, C.c_int32, ALLGATHER_CB, C.c_void_p, C.POINTER(C.c_void_p)]),
    "bnr_comm_destroy": (C.c_int, [C.c_void_p]),
    "bnr_comm_allgather": (C.c_int, [C.c_void_p, _dp, _dp, C.c_int64]),
    "bnr_comm_info": (C.c_int, [C.c_void_p] + [C.POINTER(C.c_int32)] * 5),
    "bnr_rhat": (C.c_int, [C.POINTER(C.c_void_p), C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, _dp, _dp]),
    "bnr_rhat_from_stats": (C.c_int, [_dp, C.c_int32, C.c_int32, C.c_int32, _dp]),
    "bnr_chain_ess_stats": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, _dp]),
    "bnr_ess_from_stats": (C.c_int, [_dp, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _dp]),
    "bnr_chain_counters": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64)]),
    "bnr_chain_set_profiling": (C.c_int, [C.c_void_p, C.c_int32]),
    "bnr_chain_last_timing": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(C.c_double), C.POINTER(C.c_int64)]),
    "bnr_chain_set_option": (C.c_int, [C.c_void_p, C.c_char_p, C.c_int64]),
    "bnr_chain_debug_read": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64), C.c_int32]),
    "bnr_chain_debug_copy": (C.c_int, [C.c_void_p, C.c_int32, _dp, C.c_int64]),
    "bnr_chain_debug_dims": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32)]),
    "bnr_chain_debug_time_gram": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(C.c_double)]),
    "bnr_debug_set_exp": (C.c_int, [C.c_int32, C.c_int32]),
    "bnr_host_philox": (None, [C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "bnr_host_unit": (C.c_double, [C.c_uint64]),
    "bnr_host_uniform2": (None, [C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_double)]),
    "bnr_host_normal": (C.c_double, [C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32]),
    "bnr_host_gamma": (C.c_double, [C.c_uint64, C.c_double, C.c_uint32, C.c_uint32, C.c_uint32]),
    "bnr_host_gig": (C.c_double, [C.c_uint64, C.c_double, C.c_double, C.c_double, C.c_uint32, C.c_uint32]),
    "bnr_host_gig_attempts": (C.c_int32, [C.c_uint64, C.c_double, C.c_double, C.c_double, C.c_uint32, C.c_uint32]),
    "bnr_host_edge_index": (C.c_int32, [C.c_int32, C.c_int32, C.c_int32]),
    "bnr_host_xi_weight": (C.c_double, [C.c_double, C.c_double, C.c_double]),
    "bnr_host_pred_noise": (None, [C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, _dp]),
    "bnr_host_gram_plan": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_int32)]),
}
for _u in ("tau2", "u_xi", "gamma", "D", "theta", "Delta", "M", "mu", "Lambda", "pi"):
    _SIGS["bnr_update_" + _u] = (C.c_int, [C.c_void_p, C.c_int32, C.c_int64])

EXPORTS = sorted(_SIGS)

# The six marginal libraries beside libbnr_hip.so, each linked against it, by short name: lib<short>.so (MARGINAL_LIBS of _build.py holds the
# paths, in this order) behind include/bnr_<short>.h, and the signatures of its exports
_ip = C.POINTER(C.c_int32)
_SET_OPTION = (C.c_int, [C.c_char_p, C.c_int64])
_MARGINAL_SIGS = {
    "mloo": {       # marginal PSIS-LOO
        "bnr_mloo_abi_version": (C.c_int, []),
        "bnr_marginal_loglik": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32] + [_dp] * 10 + [_ip]),
        "bnr_chains_marginal_loo": (C.c_int, [C.POINTER(C.c_void_p), C.c_int32, C.c_int32, C.c_int32, C.c_int32] + [_dp] * 7 + [_ip]),
        "bnr_mloo_set_option": _SET_OPTION,
    },
    "medge": {      # Rao-Blackwellised edge summaries
        "bnr_medge_abi_version": (C.c_int, []),
        "bnr_marginal_gamma": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32] + [_dp] * 8 + [_ip]),
        "bnr_mixture_summary": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32] + [_dp] * 3 + [C.c_double, C.c_double] + [_dp] * 7),
        "bnr_chains_marginal_edges": (C.c_int, [C.POINTER(C.c_void_p), C.c_int32, _dp, C.c_int32, C.c_int32, C.c_int32, C.c_double, C.c_double] + [_dp] * 9
                                      + [_ip]),
        "bnr_medge_set_option": _SET_OPTION,
    },
    "mpred": {      # Rao-Blackwellised prediction of new rows
        "bnr_mpred_abi_version": (C.c_int, []),
        "bnr_marginal_predict": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32] + [_dp] * 9 + [_ip]),
        "bnr_mixture_score": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32] + [_dp] * 6),
        "bnr_chains_marginal_predict": (C.c_int, [C.POINTER(C.c_void_p), C.c_int32, _dp, C.c_int32, C.c_int32, C.c_int32, _dp, C.c_int32, _dp, C.c_double,
                                                  C.c_double] + [_dp] * 12 + [_ip]),
        "bnr_mpred_set_option": _SET_OPTION,
    },
    "mcheck": {     # the LOO predictive checks under the marginal PSIS weights
        "bnr_mcheck_abi_version": (C.c_int, []),
        "bnr_weighted_mixture": (C.c_int, [C.c_int32, C.c_int32, C.c_int32] + [_dp] * 4 + [C.c_double, C.c_double] + [_dp] * 5),
        "bnr_chains_marginal_loo_predict": (C.c_int, [C.POINTER(C.c_void_p), C.c_int32, C.c_int32, C.c_int32, C.c_int32, _dp, C.c_double, C.c_double]
                                            + [_dp] * 9 + [_ip]),
        "bnr_mcheck_set_option": _SET_OPTION,
    },
    "mstack": {     # chain stacking on the marginal PSIS-LOO and the checks of the stacked mixture
        "bnr_mstack_abi_version": (C.c_int, []),
        "bnr_stacked_mixture": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32] + [_dp] * 5 + [C.c_double, C.c_double] + [_dp] * 5),
        "bnr_chains_marginal_stack": (C.c_int, [C.POINTER(C.c_void_p), C.c_int32, C.c_int32, C.c_int32, C.c_int32, _dp, _dp, C.c_int32, C.c_double, C.c_double,
                                                C.c_double] + [_dp] * 4 + [C.POINTER(C.c_double), _ip] + [_dp] * 6 + [_ip]),
        "bnr_mstack_set_option": _SET_OPTION,
    },
    "mcov": {       # the Rao-Blackwellised covariance of the edge coefficients
        "bnr_mcov_abi_version": (C.c_int, []),
        # device, n, q, K, nd | X, y, tau2, mu, S, W, weights | ncols, cols | mean, cov, within, m, v | n_bad
        "bnr_marginal_gamma_cov": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32] + [_dp] * 7 + [C.c_int32, _ip] + [_dp] * 5 + [_ip]),
        # chains, nchains, weights, first_row, nsamp, thin | ncols, cols | mean, cov, within, m, v | n_bad
        "bnr_chains_marginal_edge_cov": (C.c_int, [C.POINTER(C.c_void_p), C.c_int32, _dp, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _ip] + [_dp] * 5 + [_ip]),
        "bnr_mcov_set_option": _SET_OPTION,
    },
}
MLOO_LIB, MEDGE_LIB, MPRED_LIB, MCHECK_LIB, MSTACK_LIB, MCOV_LIB = MARGINAL_LIBS.values()
_MLOO_SIGS, _MEDGE_SIGS, _MPRED_SIGS, _MCHECK_SIGS, _MSTACK_SIGS, _MCOV_SIGS = (_MARGINAL_SIGS[short] for short in MARGINAL_LIBS)
MLOO_EXPORTS, MEDGE_EXPORTS, MPRED_EXPORTS, MCHECK_EXPORTS, MSTACK_EXPORTS, MCOV_EXPORTS = (sorted(_MARGINAL_SIGS[short]) for short in MARGINAL_LIBS)
MLOO_MAX_N = 2048


_foreign_hip = None      # set by lib(): why chains must not be created in this process (GPU-free entry points stay usable)


def _mapped(needle):
    """paths of the shared objects in this process whose name contains `needle` (from /proc/self/maps)"""
    out = []
    try:
        with open("/proc/self/maps") as f:
            for line in f:
                parts = line.split()
                if len(parts) >= 6 and needle in os.path.basename(parts[5]) and parts[5] not in out:
                    out.append(parts[5])
    except OSError:
        pass
    return out


def lib():
    """Load libbnr_hip.so; raises if it has not been built (run __graft_entry__.build())."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB):
            raise ImportError("libbnr_hip.so is missing at %s -- build it with `python -c 'import __graft_entry__ as g; "
                              "g.build()'` (hipcc --offload-arch=gfx950); there is no CPU fallback" % LIB)
        # Load order: the process serves every libamdhip64 user from the FIRST copy that was mapped.  A torch wheel carries its own
        # ROCm runtime; if it is already in the process, libbnr_hip.so would silently run on that one (its graph capture of the
        # two-branch sweep has only ever been validated on the runtime the library was built against, and round 2 saw captures
        # crash under the wheel's 7.0 runtime).  Refuse with a clear message instead (BNR_ALLOW_FOREIGN_HIP=1 overrides).
        before = _mapped("libamdhip64")
        L = C.CDLL(LIB)
        after = _mapped("libamdhip64")
        foreign = [p_ for p_ in before if not os.path.realpath(p_).startswith(os.path.realpath(os.environ.get("ROCM_PATH", "/opt/rocm")))]
        global _foreign_hip
        if foreign and after == before and not os.environ.get("BNR_ALLOW_FOREIGN_HIP"):
            _foreign_hip = ("libbnr_hip.so was loaded after another HIP runtime (%s) and is bound to it instead of %s/lib: load the library "
                            "(bnr_amd._capi.lib(), or create the chains) BEFORE importing torch, or set BNR_ALLOW_FOREIGN_HIP=1 to run on the "
                            "foreign runtime" % (", ".join(foreign), os.environ.get("ROCM_PATH", "/opt/rocm")))
        for name, (res, args) in _SIGS.items():
            f = getattr(L, name)
            f.restype = res
            f.argtypes = args
        _lib = L
    return _lib


def marginal_lib(short):
    """Load the marginal library lib<short>.so (once), after libbnr_hip.so, which it is linked against, and give its functions their
    signatures; raises if it has not been built"""
    g = globals()
    if g["_" + short] is None:
        lib()
        path = MARGINAL_LIBS[short]
        if not os.path.exists(path):
            raise ImportError("%s is missing at %s -- build it with `python -c 'import __graft_entry__ as g; g.build()'`; there is no CPU fallback"
                              % (os.path.basename(path), path))
        L = C.CDLL(path)
        for name, (res, args) in _MARGINAL_SIGS[short].items():
            f = getattr(L, name)
            f.restype = res
            f.argtypes = args
        g["_" + short] = L
    return g["_" + short]


mloo_lib, medge_lib, mpred_lib, mcheck_lib, mstack_lib, mcov_lib = (functools.partial(marginal_lib, short) for short in MARGINAL_LIBS)


def _device_marginal(short):
    """marginal_lib(short) for the calls that open a device, refused like _device_lib()"""
    _device_lib()
    return marginal_lib(short)


def _marginal_set_option(short, name, value):
    check(getattr(marginal_lib(short), "bnr_%s_set_option" % short)(name.encode(), int(value)))


mloo_set_option, medge_set_option, mpred_set_option, mcheck_set_option, mstack_set_option, mcov_set_option = (
    functools.partial(_marginal_set_option, short) for short in MARGINAL_LIBS)


def _device_lib():
    """lib() for the calls that open a device: refused where the library is bound to a foreign HIP runtime (see lib())"""
    L = lib()
    if _foreign_hip:
        raise BnrError(BNR_ERR_HIP, _foreign_hip)
    return L


def check(code):
    if code != BNR_OK:
        raise BnrError(code, lib().bnr_last_error().decode())


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


TABLE_COLUMNS = ["tau2", "u", "xi", "gamma", "S", "theta", "Delta", "M", "mu", "lam", "pi"]
DEAD_COLUMNS = ["Sigma_inv", "invC", "mu_t"]   # allocated, never written by the reference (gibbs.jl:840-841)


def table_shapes(V, R):
    q = V * (V + 1) // 2
    return dict(tau2=(1, 1), u=(R, V), xi=(V, 1), gamma=(q, 1), S=(q, 1), theta=(1, 1), Delta=(1, 1), M=(R, R),
                mu=(1, 1), lam=(R, 1), pi=(R, 3), Sigma_inv=(R, R), invC=(R, R), mu_t=(R, 1))


def new_table(tot, V, R, dead=True):
    """The reference's state Table: every column Array{Float64,3}(tot,d1,d2), iteration index fastest."""
    names = TABLE_COLUMNS + (DEAD_COLUMNS if dead else [])
    sh = table_shapes(V, R)
    return {k: np.zeros((tot,) + sh[k], dtype=np.float64, order="F") for k in names}


def device_count():
    n = C.c_int(0)
    check(lib().bnr_device_count(C.byref(n)))
    return n.value


def device_synchronize(device=0):
    check(lib().bnr_device_synchronize(int(device)))


def runtime_version():
    v = C.c_int(0)
    check(lib().bnr_runtime_version(C.byref(v)))
    return v.value


def r_eff_array(r_eff, m):
    """PSIS's relative efficiencies as m float64 values, or None for the library's default (1): a scalar is repeated; every value must be
    positive and finite (ValueError before any library call)"""
    if r_eff is None:
        return None
    r = np.asarray(r_eff, dtype=np.float64)
    r = np.full(m, float(r)) if r.ndim == 0 else np.ascontiguousarray(r.reshape(-1))
    if r.shape != (m,):
        raise ValueError("r_eff must be a scalar or have one entry per row (%d), not %d" % (m, r.size))
    if not np.all(np.isfinite(r) & (r > 0)):
        raise ValueError("r_eff must be positive and finite")
    return r


def _matrix(x, name):
    """a caller's m x S matrix (rows x draws) as contiguous float64; ValueError (before any library call) unless it is one with m, S >= 1"""
    a = np.ascontiguousarray(x, dtype=np.float64)
    if a.ndim != 2 or a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError("%s must be an m x S matrix (rows x draws) with m, S >= 1" % name)
    return a


def psis_loo_raw(loglik, r_eff=None, device=0):
    """(lpd, elpd_loo, pareto_k) of every row of an m x S log-likelihood matrix, PSIS on the device (bnr_psis_loo)"""
    ll = _matrix(loglik, "loglik")
    m, S = ll.shape
    r = r_eff_array(r_eff, m)
    lpd, elpd, k = np.empty(m), np.empty(m), np.empty(m)
    check(_device_lib().bnr_psis_loo(int(device), m, S, _ptr(ll), _ptr(r), _ptr(elpd), _ptr(k), _ptr(lpd)))
    return lpd, elpd, k


def psis_weights_raw(loglik, r_eff=None, device=0):
    """(log_weights m x S, elpd_loo, pareto_k): the normalised PSIS log weights of every row of an m x S log-likelihood matrix, on the device
    (bnr_psis_weights); a row with a non-finite entry gets NaN weights"""
    ll = _matrix(loglik, "loglik")
    m, S = ll.shape
    r = r_eff_array(r_eff, m)
    lw, elpd, k = np.empty((m, S)), np.empty(m), np.empty(m)
    check(_device_lib().bnr_psis_weights(int(device), m, S, _ptr(ll), _ptr(r), _ptr(lw), _ptr(elpd), _ptr(k)))
    return lw, elpd, k


def loo_probs(p_lo, p_hi):
    """the probabilities of the LOO predictive bounds as floats; ValueError (before any library call) unless 0 < p_lo < p_hi < 1"""
    p_lo, p_hi = float(p_lo), float(p_hi)
    if not (0.0 < p_lo < p_hi < 1.0):
        raise ValueError("need 0 < p_lo < p_hi < 1, not p_lo = %r, p_hi = %r" % (p_lo, p_hi))
    return p_lo, p_hi


LOO_PREDICT_FIELDS = ("lpd", "elpd_loo", "pareto_k", "loo_mean", "loo_sd", "loo_pit", "loo_lower", "loo_upper")


RANK_DIAG_FIELDS = ("rhat_bulk", "rhat_tail", "ess_bulk", "ess_tail", "ess_mean", "mcse_mean")


def host_ndtri(p):
    """Phi^-1 as the rank kernel evaluates it (bnr_host_ndtri: Wichura's AS 241, PPND16; no GPU), elementwise"""
    f = lib().bnr_host_ndtri
    a = np.asarray(p, dtype=np.float64)
    return np.array([f(v) for v in a.reshape(-1).tolist()], dtype=np.float64).reshape(a.shape)


def rank_normalize_raw(x, device=0, ranks=True, z=True):
    """(ranks, z) of every row of an m x S matrix, each row ranked on its own, on the device (bnr_rank_normalize): average ranks (ties share the
    mean of their positions) and z = Phi^-1((r - 3/8) / (S + 1/4)); the one not asked for is None"""
    a = _matrix(x, "x")
    if not (ranks or z):
        raise ValueError("ask for the ranks, z or both")
    m, S = a.shape
    r = np.empty((m, S)) if ranks else None
    zz = np.empty((m, S)) if z else None
    check(_device_lib().bnr_rank_normalize(int(device), m, S, _ptr(a), _ptr(r), _ptr(zz)))
    return r, zz


HDI_FIELDS = ("lower", "upper", "median", "p_pos", "p_neg")


def hdi_probs(probs):
    """the levels of an HDI call as a float64 vector (a scalar is one level); ValueError (before any library call) unless there are at most 8
    and every one lies in (0, 1)"""
    pr = np.ascontiguousarray(np.atleast_1d(np.asarray(probs, dtype=np.float64)).reshape(-1))
    if pr.size > 8:
        raise ValueError("at most 8 HDI levels in one call, not %d" % pr.size)
    if not np.all((pr > 0.0) & (pr < 1.0)):
        raise ValueError("every HDI level must lie in (0, 1), not %r" % (pr.tolist(),))
    return pr


def _hdi_outputs(pr, m, fields):
    """the five output arrays of an HDI call over m columns: lower / upper (nprob, m), median / p_pos / p_neg (m,); None where not in `fields`"""
    shapes = dict(lower=(pr.size, m), upper=(pr.size, m), median=(m,), p_pos=(m,), p_neg=(m,))
    return [np.empty(shapes[f]) if f in fields else None for f in HDI_FIELDS]


def hdi_raw(x, probs, device=0, fields=HDI_FIELDS):
    """The tuple HDI_FIELDS of every row of an m x S matrix, each row on its own, on the device (bnr_hdi): lower / upper (nprob, m) -- the
    highest-density interval of every level of `probs` --, the median, and the shares of draws above and below zero (m,); an entry not named
    in `fields` is not requested and comes back as None"""
    a = _matrix(x, "x")
    pr = hdi_probs(probs)
    m, S = a.shape
    out = _hdi_outputs(pr, m, fields)
    check(_device_lib().bnr_hdi(int(device), m, S, _ptr(a), pr.size, _ptr(pr), *[_ptr(o) for o in out]))
    return tuple(out)


INCL_FIELDS = ("prob", "joint", "size_pmf", "n_distinct", "top_sets", "top_count")


def _incl_outputs(B, ntop, fields):
    """(ntop, the six output arrays of an inclusion call over B indicators): prob (B,), joint (B, B), size_pmf (B + 1,), n_distinct (1,) int64,
    top_sets (ntop, W) uint64 with W = ceil(B / 64), top_count (ntop,) int64; None where not in `fields`.  ValueError (before any library
    call) for a field that does not exist, for no field at all, for ntop outside 0 .. 256 and for top_sets without top_count, the reverse,
    or either with ntop = 0"""
    fields = tuple(fields)
    ntop = int(ntop)
    unknown = [f for f in fields if f not in INCL_FIELDS]
    if unknown or not fields:
        raise ValueError("fields must name at least one of %r, not %r" % (INCL_FIELDS, fields))
    if not 0 <= ntop <= 256:
        raise ValueError("need 0 <= ntop <= 256, not %d" % ntop)
    if ("top_sets" in fields) != ("top_count" in fields):
        raise ValueError("top_sets and top_count come together")
    if "top_sets" in fields and ntop < 1:
        raise ValueError("top_sets and top_count need ntop >= 1")
    W = (B + 63) // 64
    make = dict(prob=lambda: np.empty(B), joint=lambda: np.empty((B, B)), size_pmf=lambda: np.empty(B + 1), n_distinct=lambda: np.zeros(1, dtype=np.int64),
                top_sets=lambda: np.zeros((ntop, W), dtype=np.uint64), top_count=lambda: np.zeros(ntop, dtype=np.int64))
    return ntop, [make[f]() if f in fields else None for f in INCL_FIELDS]


def _incl_result(out):
    """the outputs of an inclusion call as they are returned: n_distinct as an int"""
    return tuple(int(o[0]) if f == "n_distinct" and o is not None else o for f, o in zip(INCL_FIELDS, out))


def inclusion_raw(z, ntop, device=0, fields=INCL_FIELDS):
    """The tuple INCL_FIELDS of an S x B matrix of indicators (rows = draws; an entry != 0 is 1), on the device (bnr_inclusion): the marginal
    shares prob (B,), the co-inclusion shares joint (B, B), the distribution size_pmf (B + 1,) of the number of indicators that are 1 in a draw,
    the number n_distinct of distinct rows, and the ntop most frequent rows as top_sets (ntop, W) -- bit k % 64 of word k // 64 is indicator k
    -- with their counts top_count, most frequent first, ties by the row as an integer; an entry not named in `fields` is not requested and
    comes back as None"""
    a = np.asarray(z)
    if a.ndim != 2 or a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError("z must be an S x B matrix (draws x indicators) with S, B >= 1")
    a = np.ascontiguousarray(a != 0, dtype=np.uint8)
    S, B = a.shape
    ntop, out = _incl_outputs(B, ntop, fields)
    check(_device_lib().bnr_inclusion(int(device), S, B, _ptr(a), ntop, *[_ptr(o) for o in out]))
    return _incl_result(out)


X_DTYPES = {np.dtype(np.float64): 0, np.dtype(np.bool_): 1, np.dtype(np.uint8): 1, np.dtype(np.int32): 2, np.dtype(np.int64): 3,
            np.dtype(np.float32): 4}     # the enum of include/bnr_hip.h (BNR_F64, BNR_U8, BNR_I32, BNR_I64, BNR_F32)


class XInput:
    """The model input of a fit as the library takes it: the n x q matrix X_new in its own element type (gibbs.jl:917:
    Matrix{eltype(T)} -- Bool adjacency data stays one byte per entry until it is on the device), or, with x_transform=True, the
    list of n adjacency matrices themselves (setup_X!, gibbs.jl:239-247, then runs on the device).  Element types without a device
    converter are promoted to float64 here."""

    def __init__(self, X, x_transform=False):
        self.from_matrices = bool(x_transform)
        if x_transform:
            mats = [np.asarray(m) for m in X]
            V = mats[0].shape[0]
            if any(m.shape != (V, V) for m in mats):
                raise ValueError("every adjacency matrix must be V x V")
            dt = np.result_type(*mats)
            dt = dt if dt in X_DTYPES else np.dtype(np.float64)
            self.data = [np.asfortranarray(m, dtype=dt) for m in mats]
            self.n, self.V = len(mats), V
            self.q = V * (V + 1) // 2
        else:
            a = np.asarray(X)
            if a.ndim != 2:
                raise ValueError("X must be an n x q matrix")
            dt = a.dtype if a.dtype in X_DTYPES else np.dtype(np.float64)
            self.data = np.asfortranarray(a, dtype=dt)
            self.n, self.q = a.shape
            self.V = int(round((-1 + np.sqrt(1 + 8 * self.q)) / 2))
            if self.V * (self.V + 1) // 2 != self.q:
                raise ValueError("X must have V(V+1)/2 columns")
        self.dtype_code = X_DTYPES[dt]


XI_WEIGHTS = {"log": 0, "reference": 1}      # model option "xi_weights" of include/bnr_hip.h


def xi_weights_code(xi_weights):
    """the library's value of the `xi_weights` model option: "log" (default: log-space node weights) or "reference" (the reference's
    ratio of pdfs with its under/overflow, gibbs.jl:349-360); anything else is a ValueError, raised before any GPU call"""
    if not isinstance(xi_weights, str) or xi_weights not in XI_WEIGHTS:
        raise ValueError("xi_weights must be one of %s, not %r" % (", ".join(map(repr, XI_WEIGHTS)), xi_weights))
    return XI_WEIGHTS[xi_weights]


# ------------------------------------------------------------------------------------------ the analysis calls, each written once
# fn: the name of the library function of one chain (bnr_chain_*) or of a list of chains (bnr_chains_*), looked up on c0.L behind the checks
# that need no library; head: its leading handle arguments, (chain.h,) or (array of handles, their number) -- and then the weights of a
# stacked call; c0: the (first) chain, for the sizes.  Chain.<call> and pooled_<call> / stacked_<call> below are their callers.
def _summary(fn, head, c0, first_row, nsamp, k_lo, k_hi):
    mean, lo, hi, pxi = np.empty(c0.q), np.empty(c0.q), np.empty(c0.q), np.empty(c0.V)
    check(getattr(c0.L, fn)(*head, int(first_row), int(nsamp), int(k_lo), int(k_hi), _ptr(mean), _ptr(lo), _ptr(hi), _ptr(pxi)))
    return mean, lo, hi, pxi


def _predict(form, fn, fn_matrices, head, c0, X, first_row, nsamp, k_lo, k_hi, y, x_transform, pred_seed=None, pit=False):
    """(mean, lower, upper, lpd, pwaic, pred_lower, pred_upper, pit), None what was not asked for.  form: "chain" (no pred_seed and pit
    arguments), "pooled", or "stacked" (no pwaic and pit arguments, and no fn_matrices)"""
    xi = X if isinstance(X, XInput) else XInput(X, x_transform)
    if xi.from_matrices and fn_matrices is None:
        raise ValueError("the stacked prediction takes a model matrix (n x q), not adjacency matrices")
    if xi.q != c0.q:
        raise ValueError("the new rows have %d edge columns, the chain %d" % (xi.q, c0.q))
    m = xi.n
    yf = None
    if y is not None:
        yf = np.ascontiguousarray(y, dtype=np.float64).reshape(-1)
        if yf.shape != (m,):
            raise ValueError("y must have one entry per new row (%d), not %d" % (m, yf.size))
    if pit and yf is None:
        raise ValueError("the PIT needs the observed responses y")
    mean, lo, hi = np.empty(m), np.empty(m), np.empty(m)
    lpd = np.empty(m) if yf is not None else None
    pw = np.empty(m) if yf is not None and form != "stacked" else None
    plo, phi = (np.empty(m), np.empty(m)) if pred_seed is not None else (None, None)
    pt = np.empty(m) if pit else None
    tail = [_ptr(yf), int(k_lo), int(k_hi), _ptr(mean), _ptr(lo), _ptr(hi), _ptr(lpd)]
    if form != "stacked":
        tail.append(_ptr(pw))
    if form != "chain":
        tail += [C.c_uint64((0 if pred_seed is None else int(pred_seed)) & (2**64 - 1)), _ptr(plo), _ptr(phi)]
    if form == "pooled":
        tail.append(_ptr(pt))
    if xi.from_matrices:
        ptrs = (C.c_void_p * m)(*[a.ctypes.data for a in xi.data])
        check(getattr(c0.L, fn_matrices)(*head, int(first_row), int(nsamp), m, ptrs, xi.dtype_code, *tail))
    else:
        check(getattr(c0.L, fn)(*head, int(first_row), int(nsamp), m, _ptr(xi.data), xi.dtype_code, *tail))
    return mean, lo, hi, lpd, pw, plo, phi, pt


def _loglik_stats(fn, head, c0, first_row, nsamp, pit=None):
    """(lpd, pwaic, pit or None); pit=None: fn takes no such argument (bnr_chain_loglik_stats)"""
    lpd, pw = np.empty(c0.n), np.empty(c0.n)
    pt = np.empty(c0.n) if pit else None
    check(getattr(c0.L, fn)(*head, int(first_row), int(nsamp), _ptr(lpd), _ptr(pw), *(() if pit is None else (_ptr(pt),))))
    return lpd, pw, pt


def _loo(fn, head, c0, first_row, nsamp, r_eff):
    r = r_eff_array(r_eff, c0.n)
    lpd, elpd, k = np.empty(c0.n), np.empty(c0.n), np.empty(c0.n)
    check(getattr(c0.L, fn)(*head, int(first_row), int(nsamp), _ptr(r), _ptr(lpd), _ptr(elpd), _ptr(k)))
    return lpd, elpd, k


def _loo_predict(fn, head, c0, first_row, nsamp, r_eff, p_lo, p_hi, fields):
    r = r_eff_array(r_eff, c0.n)
    out = [np.empty(c0.n) if f in fields else None for f in LOO_PREDICT_FIELDS]
    check(getattr(c0.L, fn)(*head, int(first_row), int(nsamp), _ptr(r), p_lo, p_hi, *[_ptr(o) for o in out]))
    return tuple(out)


def _rank_diag(fn, head, c0, first_row, nsamp, max_lag, fields):
    fields = RANK_DIAG_FIELDS if fields is None else fields
    out = [np.empty(c0.q + c0.V) if f in fields else None for f in RANK_DIAG_FIELDS]
    check(getattr(c0.L, fn)(*head, int(first_row), int(nsamp), int(max_lag), *[_ptr(o) for o in out]))
    return tuple(out)


def _hdi(fn, head, c0, first_row, nsamp, probs, fields):
    pr = hdi_probs(probs)
    out = _hdi_outputs(pr, c0.q + c0.V, fields)
    check(getattr(c0.L, fn)(*head, int(first_row), int(nsamp), pr.size, _ptr(pr), *[_ptr(o) for o in out]))
    return tuple(out)


def _inclusion(fn, head, c0, first_row, nsamp, which, ntop, fields):
    ntop, out = _incl_outputs(c0.R if which == 1 else c0.V, ntop, fields)
    check(getattr(c0.L, fn)(*head, int(first_row), int(nsamp), int(which), ntop, *[_ptr(o) for o in out]))
    return _incl_result(out)


def cov_cols(cols, q):
    """the column list of a covariance call over q edges as int32, or None for every edge; ValueError (before any library call) for an empty
    list, a value that is no integer, or an index outside 0 .. q - 1"""
    if cols is None:
        return None
    a = np.asarray(cols)
    if a.ndim != 1 or a.size < 1 or a.dtype == np.bool_ or not (np.issubdtype(a.dtype, np.integer) or np.all(a == np.floor(a))):
        raise ValueError("cols must be a non-empty list of 0-based edge indices")
    a = a.astype(np.int64)
    if a.min() < 0 or a.max() >= q:
        raise ValueError("edge indices must lie in 0 .. %d" % (q - 1))
    return np.ascontiguousarray(a, dtype=np.int32)


def _cov(fn, head, c0, first_row, nsamp, cols):
    """(mean (ncols,), cov (ncols, ncols)) of the chosen gamma columns; head carries the weights (or None) of the pooled form behind the handles"""
    ci = cov_cols(cols, c0.q)
    m = c0.q if ci is None else ci.size
    mean, cov = np.empty(m), np.empty((m, m))
    check(getattr(c0.L, fn)(*head, int(first_row), int(nsamp), m, _ptr(ci), _ptr(mean), _ptr(cov)))
    return mean, cov


class Chain:
    """One Gibbs chain resident on one GPU (handle of include/bnr_hip.h).  xi_weights: "log" (default) or "reference" (model
    option "xi_weights": the reference's node weights with their under/overflow, see include/bnr_hip.h)."""

    def __init__(self, X, y, R, tot_save, seed, chain_id, device=0, eta=1.01, zeta=1.0, iota=1.0, aDelta=1.0,
                 bDelta=1.0, nu=10, xi_weights="log"):
        xw = xi_weights_code(xi_weights)
        xi = X if isinstance(X, XInput) else XInput(X)
        yf = np.ascontiguousarray(y, dtype=np.float64)
        n, q, V = xi.n, xi.q, xi.V
        if yf.shape != (n,):
            raise ValueError("y must have one entry per row of X")
        self.n, self.q, self.V, self.R, self.tot = n, q, V, int(R), int(tot_save)
        self.y = yf.copy()                                  # (the training responses, for the totals of the LOO calls)
        self.h = C.c_void_p()
        hy = Hyper(eta, zeta, iota, aDelta, bDelta, float(nu))
        self.L = _device_lib()
        common =(_ptr(yf), C.byref(hy), C.c_uint64(int(seed) & (2**64 - 1)), int(chain_id), int(device), int(tot_save), C.byref(self.h))
        if xi.from_matrices:
            ptrs = (C.c_void_p * n)(*[m.ctypes.data for m in xi.data])
            check(self.L.bnr_chain_create_from_matrices(n, V, int(R), ptrs, xi.dtype_code, *common))
        elif xi.dtype_code == 0:
            check(self.L.bnr_chain_create(n, V, int(R), _ptr(xi.data), *common))
        else:
            check(self.L.bnr_chain_create_typed(n, V, int(R), _ptr(xi.data), xi.dtype_code, *common))
        self.xi_weights = xi_weights
        if xw:
            self.set_option("xi_weights", xw)

    @classmethod
    def like(cls, donor, seed, chain_id, tot_save=None):
        """Another chain of the same fit (same X, y, hyper-parameters and xi_weights; device inputs shared with `donor`)."""
        self = cls.__new__(cls)
        self.n, self.q, self.V, self.R = donor.n, donor.q, donor.V, donor.R
        self.y = donor.y
        self.tot = int(donor.tot if tot_save is None else tot_save)
        self.h = C.c_void_p()
        self.L = donor.L
        check(self.L.bnr_chain_create_like(donor.h, C.c_uint64(int(seed) & (2**64 - 1)), int(chain_id), self.tot, C.byref(self.h)))
        self.xi_weights = donor.xi_weights                  # inherited by the library (bnr_chain_create_like)
        return self

    def close(self):
        h, self.h = getattr(self, "h", None), None          # (no ctypes call when the interpreter is shutting down: C may be gone)
        if h and h.value and getattr(self, "L", None) is not None:
            self.L.bnr_chain_destroy(h)

    __del__ = close

    def init_prior(self):
        check(self.L.bnr_chain_init_prior(self.h))

    def run(self, first_index, nburn, total, purge_burn=None, prog_freq=0, callback=None):
        nxt = C.c_int32(0)
        cb = PROGRESS_CB(lambda user, done: callback(done)) if callback else PROGRESS_CB()
        check(self.L.bnr_chain_run(self.h, first_index, nburn, total, purge_burn or 0, prog_freq if callback else 0, cb,
                                   None, C.byref(nxt)))
        return nxt.value

    def prepare(self):
        """Capture the hipGraphs the run loop replays now (otherwise done lazily by the first run call)."""
        check(self.L.bnr_chain_prepare(self.h))

    def run_async(self, first_index, nburn, total, purge_burn=None):
        check(self.L.bnr_chain_run_async(self.h, first_index, nburn, total, purge_burn or 0))

    def sync(self):
        nxt = C.c_int32(0)
        check(self.L.bnr_chain_sync(self.h, C.byref(nxt)))
        return nxt.value

    def gibbs_step(self, row, it):
        check(self.L.bnr_gibbs_step(self.h, row, it))

    def update(self, name, row, it):
        check(getattr(self.L, "bnr_update_" + name)(self.h, row, it))

    @property
    def iter(self):
        v = C.c_int64(0)
        check(self.L.bnr_chain_get_iter(self.h, C.byref(v)))
        return v.value

    @iter.setter
    def iter(self, v):
        check(self.L.bnr_chain_set_iter(self.h, int(v)))

    def fetch(self, first_row=1, last_row=None, table=None, host_row_offset=0):
        last_row = self.tot if last_row is None else last_row
        if table is None:
            table = new_table(last_row - first_row + 1, self.V, self.R, dead=False)
            host_row_offset = -(first_row - 1)
        tot = table["tau2"].shape[0]
        for k in TABLE_COLUMNS:
            a = table[k]
            assert a.dtype == np.float64 and a.flags.f_contiguous and a.shape[0] == tot, k
        check(self.L.bnr_chain_fetch(self.h, first_row, last_row, tot, host_row_offset, *[_ptr(table[k]) for k in TABLE_COLUMNS]))
        return table

    def load(self, table, first_row=1, last_row=None, host_row_offset=0):
        tot = table["tau2"].shape[0]
        last_row = min(self.tot, tot - host_row_offset) if last_row is None else last_row
        cols = []
        for k in TABLE_COLUMNS:
            a = table.get(k)
            if a is not None:
                a = np.asfortranarray(a, dtype=np.float64)
                assert a.shape[0] == tot, k
            cols.append(a)
        self._keep = cols
        check(self.L.bnr_chain_load(self.h, first_row, last_row, tot, host_row_offset, *[_ptr(a) for a in cols]))

    def move_rows(self, to_row, from_row, count):
        check(self.L.bnr_chain_move_rows(self.h, to_row, from_row, count))

    def resize(self, new_tot):
        check(self.L.bnr_chain_resize(self.h, new_tot))
        self.tot = int(new_tot)

    def rhat_stats(self, first_row, nsamp):
        out = np.empty(4 * (self.q + self.V))
        check(self.L.bnr_chain_rhat_stats(self.h, first_row, nsamp, _ptr(out)))
        return out

    def summary(self, first_row, nsamp, k_lo, k_hi):
        """(mean gamma, k_lo-th smallest, k_hi-th smallest per edge, mean xi per node) over the row window, on the device."""
        return _summary("bnr_chain_summary", (self.h,), self, first_row, nsamp, k_lo, k_hi)

    def predict(self, X, first_row, nsamp, k_lo, k_hi, y=None, x_transform=False):
        """Posterior of the mean response mu + x.gamma of new rows over the row window, on the device (bnr_chain_predict): (mean, k_lo-th
        smallest, k_hi-th smallest, lpd, pwaic) per row; lpd / pwaic are None without y.  X as for Chain(): an m x q matrix in its own element
        type, or (x_transform=True) a list of m V x V matrices."""
        return _predict("chain", "bnr_chain_predict", "bnr_chain_predict_from_matrices", (self.h,), self, X, first_row, nsamp, k_lo, k_hi, y,
                        x_transform)[:5]

    def loglik_stats(self, first_row, nsamp):
        """(lpd, pwaic) of the chain's own training rows over the row window, on the device (bnr_chain_loglik_stats)."""
        return _loglik_stats("bnr_chain_loglik_stats", (self.h,), self, first_row, nsamp)[:2]

    def loo(self, first_row, nsamp, r_eff=None):
        """(lpd, elpd_loo, pareto_k) of the chain's own training rows over the row window: PSIS-LOO on the device (bnr_chain_loo).
        r_eff: None (1), a scalar, or one relative efficiency per training row."""
        return _loo("bnr_chain_loo", (self.h,), self, first_row, nsamp, r_eff)

    def loo_predict(self, first_row, nsamp, r_eff=None, p_lo=0.025, p_hi=0.975):
        """The LOO predictive checks of the chain's own training rows over the row window, on the device (bnr_chain_loo_predict): the tuple
        LOO_PREDICT_FIELDS = (lpd, elpd_loo, pareto_k, loo_mean, loo_sd, loo_pit, loo_lower, loo_upper), one entry per row each."""
        return _loo_predict("bnr_chain_loo_predict", (self.h,), self, first_row, nsamp, r_eff, *loo_probs(p_lo, p_hi), LOO_PREDICT_FIELDS)

    def ess_stats(self, first_row, nsamp, max_lag):
        out = np.empty(2 * (2 + max_lag) * (self.q + self.V))
        check(self.L.bnr_chain_ess_stats(self.h, first_row, nsamp, max_lag, _ptr(out)))
        return out

    def rank_diag(self, first_row, nsamp, max_lag, fields=None):
        """The rank-normalised diagnostics of this chain's window, on the device (bnr_chain_rank_diag): the tuple RANK_DIAG_FIELDS, each q + V
        values (gamma first); an entry not named in `fields` is not requested and comes back as None"""
        return _rank_diag("bnr_chain_rank_diag", (self.h,), self, first_row, nsamp, max_lag, fields)

    def hdi(self, first_row, nsamp, probs, fields=HDI_FIELDS):
        """The highest-density intervals, medians and sign probabilities of this chain's window, on the device (bnr_chain_hdi): the tuple
        HDI_FIELDS over the q + V parameters (gamma first), lower / upper one row per level of `probs`; an entry not named in `fields` is not
        requested and comes back as None"""
        return _hdi("bnr_chain_hdi", (self.h,), self, first_row, nsamp, probs, fields)

    def inclusion(self, first_row, nsamp, which, ntop, fields=INCL_FIELDS):
        """The joint posterior of this chain's indicators over its window, on the device (bnr_chain_inclusion): the tuple INCL_FIELDS of the V
        node indicators xi (which = 0) or of the R dimensions lambda != 0 (which = 1), see inclusion_raw; an entry not named in `fields` is
        not requested and comes back as None"""
        return _inclusion("bnr_chain_inclusion", (self.h,), self, first_row, nsamp, which, ntop, fields)

    def cov(self, first_row, nsamp, cols=None):
        """(mean, cov) of this chain's edge coefficients over its window, on the device (bnr_chain_cov): the columns `cols` (0-based edge
        indices; None: all q), cov = numpy's cov of the draws about the Summary mean"""
        return _cov("bnr_chain_cov", (self.h,), self, first_row, nsamp, cols)

    def device_view(self):
        """bnr_chain_device_view: the sizes, row offsets and device pointers of this chain as a ChainView"""
        v = ChainView()
        check(self.L.bnr_chain_device_view(self.h, C.byref(v)))
        return v

    def counters(self):
        out = (C.c_int64 * 8)()
        check(self.L.bnr_chain_counters(self.h, out))
        return dict(jitter=out[0], nan_w=out[1], sampler_cap=out[2], chol_fail=out[3], where=list(out[4:8]))

    def set_profiling(self, on=True):
        check(self.L.bnr_chain_set_profiling(self.h, 1 if on else 0))

    def last_timing(self, which):
        us, n = C.c_double(0), C.c_int64(0)
        check(self.L.bnr_chain_last_timing(self.h, which, C.byref(us), C.byref(n)))
        return us.value, n.value

    def debug_read(self, count=1024):
        out = (C.c_uint64 * count)()
        check(self.L.bnr_chain_debug_read(self.h, out, count))
        return np.array(out[:], dtype=np.uint64)

    def debug_time_gram(self, reps=100):
        us = C.c_double(0)
        check(self.L.bnr_chain_debug_time_gram(self.h, reps, C.byref(us)))
        return us.value

    def debug_copy(self, which, count):
        out = np.empty(count)
        check(self.L.bnr_chain_debug_copy(self.h, which, _ptr(out), count))
        return out

    def debug_dims(self):
        out = (C.c_int32 * 8)()
        check(self.L.bnr_chain_debug_dims(self.h, out))
        return dict(zip(("n_pad", "q_pad", "ksplit", "ntile", "kcp", "kslab", "i8L", "rowlen"), [int(v) for v in out]))

    def debug_gram(self):
        """The (G) of the last Gram launch, lower triangle, summed over the K-split partial tiles on the host (diagnostics; n_pad x n_pad)."""
        dm = self.debug_dims()
        nt, ks = dm["ntile"], dm["ksplit"]
        ntl = nt * (nt + 1) // 2
        P = self.debug_copy(3, ks * ntl * 4096).reshape(ks, ntl, 64, 64).sum(axis=0)     # [tile][j][i]
        G = np.zeros((dm["n_pad"], dm["n_pad"]))
        for ti in range(nt):
            for tj in range(ti + 1):
                G[ti * 64:(ti + 1) * 64, tj * 64:(tj + 1) * 64] = P[ti * (ti + 1) // 2 + tj].T
        return np.tril(G)

    def set_option(self, name, value):
        if name == "xi_weights" and isinstance(value, str):
            value = xi_weights_code(value)
        check(self.L.bnr_chain_set_option(self.h, name.encode(), int(value)))
        if name == "xi_weights":
            self.xi_weights = {v: k for k, v in XI_WEIGHTS.items()}[int(value)]


class Group:
    """Lockstep group of equally shaped chains on one GPU (bnr_group_* of include/bnr_hip.h): one launch per kernel of a
    sweep for all members; every member's table is bitwise what it would be when run alone."""

    def __init__(self, chains):
        self.chains = list(chains)
        self.L = lib()
        self.h = C.c_void_p()
        arr = (C.c_void_p * len(self.chains))(*[ch.h for ch in self.chains])
        check(self.L.bnr_group_create(arr, len(self.chains), C.byref(self.h)))

    def close(self):
        h, self.h = getattr(self, "h", None), None
        if h and h.value and getattr(self, "L", None) is not None:
            self.L.bnr_group_destroy(h)

    __del__ = close

    def run(self, first_index, nburn, total, purge_burn=None, prog_freq=0, callback=None):
        nxt = C.c_int32(0)
        cb = PROGRESS_CB(lambda user, done: callback(done)) if callback else PROGRESS_CB()
        check(self.L.bnr_group_run(self.h, first_index, nburn, total, purge_burn or 0, prog_freq if callback else 0, cb,
                                   None, C.byref(nxt)))
        return nxt.value

    def prepare(self):
        check(self.L.bnr_group_prepare(self.h))

    def set_option(self, name, value):
        check(self.L.bnr_group_set_option(self.h, name.encode(), int(value)))

    def set_profiling(self, on=True):
        self.set_option("profiling", 1 if on else 0)

    def last_timing(self, which):
        us, n = C.c_double(0), C.c_int64(0)
        check(self.L.bnr_group_last_timing(self.h, which, C.byref(us), C.byref(n)))
        return us.value, n.value


# ------------------------------------------------------------------------------------------ pooled chains (bnr_chains_* of include/bnr_hip.h)
def _pooled(chains):
    """(the first chain, (the handles as a C array, their number)): the chains of one fit on one device whose windows are pooled, in this order"""
    chains = list(chains)
    if not chains:
        raise ValueError("need at least one chain")
    return chains[0], ((C.c_void_p * len(chains))(*[ch.h for ch in chains]), len(chains))


def host_pred_noise(seed, s0, ns, i0, ni):
    """the noise z of the predictive draws as the device draws it (bnr_host_pred_noise; no GPU): an (ni, ns) array, element [i - i0, s - s0] for
    row i of the call and pooled draw s"""
    out = np.empty((int(ni), int(ns)))
    lib().bnr_host_pred_noise(C.c_uint64(int(seed) & (2**64 - 1)), int(s0), int(ns), int(i0), int(ni), _ptr(out))
    return out


def pooled_summary(chains, first_row, nsamp, k_lo, k_hi):
    """Chain.summary over the pooled window of `chains` (bnr_chains_summary); ranks in 1 .. len(chains) * nsamp"""
    c0, head = _pooled(chains)
    return _summary("bnr_chains_summary", head, c0, first_row, nsamp, k_lo, k_hi)


def pooled_predict(chains, X, first_row, nsamp, k_lo, k_hi, y=None, x_transform=False, pred_seed=None, pit=False):
    """Chain.predict over the pooled window of `chains` (bnr_chains_predict / _from_matrices): (mean, lower, upper, lpd, pwaic, pred_lower,
    pred_upper, pit) per row.  pred_seed given: the k_lo-th / k_hi-th smallest draw of a new observation (None otherwise); pit=True (needs y):
    the PIT of the observed responses."""
    c0, head = _pooled(chains)
    return _predict("pooled", "bnr_chains_predict", "bnr_chains_predict_from_matrices", head, c0, X, first_row, nsamp, k_lo, k_hi, y, x_transform,
                    pred_seed, pit)


def pooled_loglik_stats(chains, first_row, nsamp, pit=False):
    """(lpd, pwaic, pit or None) of the training rows over the pooled window of `chains` (bnr_chains_loglik_stats)"""
    c0, head = _pooled(chains)
    return _loglik_stats("bnr_chains_loglik_stats", head, c0, first_row, nsamp, bool(pit))


def pooled_loo(chains, first_row, nsamp, r_eff=None):
    """(lpd, elpd_loo, pareto_k) of the training rows over the pooled window of `chains`: PSIS-LOO on the device (bnr_chains_loo)"""
    c0, head = _pooled(chains)
    return _loo("bnr_chains_loo", head, c0, first_row, nsamp, r_eff)


def pooled_loo_predict(chains, first_row, nsamp, r_eff=None, p_lo=0.025, p_hi=0.975, fields=LOO_PREDICT_FIELDS):
    """Chain.loo_predict over the pooled window of `chains` (bnr_chains_loo_predict): the tuple LOO_PREDICT_FIELDS; an entry not named in
    `fields` is not requested from the library and comes back as None"""
    p_lo, p_hi = loo_probs(p_lo, p_hi)
    c0, head = _pooled(chains)
    return _loo_predict("bnr_chains_loo_predict", head, c0, first_row, nsamp, r_eff, p_lo, p_hi, fields)


def pooled_rank_diag(chains, first_row, nsamp, max_lag, fields=None):
    """Chain.rank_diag over the pooled window of `chains` (bnr_chains_rank_diag): the tuple RANK_DIAG_FIELDS"""
    c0, head = _pooled(chains)
    return _rank_diag("bnr_chains_rank_diag", head, c0, first_row, nsamp, max_lag, fields)


def pooled_hdi(chains, first_row, nsamp, probs, fields=HDI_FIELDS):
    """Chain.hdi over the pooled window of `chains` (bnr_chains_hdi): the tuple HDI_FIELDS"""
    c0, head = _pooled(chains)
    return _hdi("bnr_chains_hdi", head, c0, first_row, nsamp, probs, fields)


def pooled_inclusion(chains, first_row, nsamp, which, ntop, fields=INCL_FIELDS):
    """Chain.inclusion over the pooled window of `chains` (bnr_chains_inclusion): the tuple INCL_FIELDS"""
    c0, head = _pooled(chains)
    return _inclusion("bnr_chains_inclusion", head, c0, first_row, nsamp, which, ntop, fields)


# ------------------------------------------------------------------------------------------ chain stacking (ABI 16)
STACK_MAX_CHAINS = 32
WQUANTILE_FIELDS = ("mean", "lower", "upper")


def stacking_weights_raw(lpd, max_iter=100000, gap_tol=1e-9):
    """(weights, objective, gap, iterations) of bnr_stacking_weights for an n x K matrix of pointwise predictive log densities (no GPU)"""
    a = np.ascontiguousarray(lpd, dtype=np.float64)
    if a.ndim != 2:
        raise ValueError("lpd must be an n x K matrix (rows x chains)")
    n, K = a.shape
    w = np.empty(max(K, 1))
    f, g, it = C.c_double(0.0), C.c_double(0.0), C.c_int32(0)
    check(lib().bnr_stacking_weights(n, K, _ptr(a), int(max_iter), float(gap_tol), _ptr(w), C.byref(f), C.byref(g), C.byref(it)))
    return w[:K], f.value, g.value, it.value


def stack_weights_array(weights, K):
    """chain weights as K float64 values (the library checks them)"""
    w = np.ascontiguousarray(weights, dtype=np.float64).reshape(-1)
    if w.shape != (K,):
        raise ValueError("need one weight per chain (%d), not %d" % (K, w.size))
    return w


def wquantile_raw(x, weights, nchains, k_lo, k_hi, device=0, fields=WQUANTILE_FIELDS):
    """(mean, lower, upper) of every row of an m x (K nsamp) matrix under chain weights, on the device (bnr_wquantile): chain k's draws in
    columns k nsamp .. (k + 1) nsamp - 1; an entry not named in `fields` is not requested and comes back as None"""
    a = np.ascontiguousarray(x, dtype=np.float64)
    K = int(nchains)
    if a.ndim != 2 or a.shape[0] < 1 or K < 1 or a.shape[1] < K or a.shape[1] % K:
        raise ValueError("x must be an m x (nchains * nsamp) matrix with m, nsamp >= 1")
    w = stack_weights_array(weights, K)
    m, S = a.shape
    out = [np.empty(m) if f in fields else None for f in WQUANTILE_FIELDS]
    check(_device_lib().bnr_wquantile(int(device), m, K, S // K, _ptr(a), _ptr(w), int(k_lo), int(k_hi), *[_ptr(o) for o in out]))
    return tuple(out)


def chains_stack(chains, first_row, nsamp, r_eff=None, max_iter=100000, gap_tol=1e-9):
    """(weights, elpd_chain K x n, pareto_k_chain K x n, elpd_stack n, gap, iterations): per-chain PSIS-LOO and the stacking weights
    (bnr_chains_stack)"""
    c0, (arr, K) = _pooled(chains)
    n = c0.n
    r = r_eff_array(r_eff, n)
    w, el, kh, es = np.empty(K), np.empty((K, n)), np.empty((K, n)), np.empty(n)
    g, it = C.c_double(0.0), C.c_int32(0)
    check(c0.L.bnr_chains_stack(arr, K, int(first_row), int(nsamp), _ptr(r), int(max_iter), float(gap_tol), _ptr(w), _ptr(el), _ptr(kh), _ptr(es),
                                C.byref(g), C.byref(it)))
    return w, el, kh, es, g.value, it.value


def stacked_summary(chains, weights, first_row, nsamp, k_lo, k_hi):
    """pooled_summary under chain weights (bnr_chains_wsummary)"""
    c0, head = _pooled(chains)
    w = stack_weights_array(weights, head[1])
    return _summary("bnr_chains_wsummary", head + (_ptr(w),), c0, first_row, nsamp, k_lo, k_hi)


def stacked_predict(chains, weights, X, first_row, nsamp, k_lo, k_hi, y=None, x_transform=False, pred_seed=None):
    """pooled_predict under chain weights for a model matrix (bnr_chains_wpredict): (mean, lower, upper, lpd, pred_lower, pred_upper) per row"""
    c0, head = _pooled(chains)
    w = stack_weights_array(weights, head[1])
    r = _predict("stacked", "bnr_chains_wpredict", None, head + (_ptr(w),), c0, X, first_row, nsamp, k_lo, k_hi, y, x_transform, pred_seed)
    return r[:4] + r[5:7]


# ------------------------------------------------------------------------------------------ posterior covariance of the edge coefficients (ABI 17)
def pooled_cov(chains, first_row, nsamp, cols=None, weights=None):
    """Chain.cov over the pooled window of `chains` (bnr_chains_cov); with weights the covariance of the chains' mixture under them"""
    c0, head = _pooled(chains)
    w = None if weights is None else stack_weights_array(weights, head[1])
    return _cov("bnr_chains_cov", head + (_ptr(w),), c0, first_row, nsamp, cols)


def cov_raw(x, nchains=1, weights=None, device=0):
    """(mean (m,), cov (m, m)) of a (nchains nsamp) x m matrix of draws (rows = draws, chain k's in rows k nsamp ..), on the device (bnr_cov)"""
    a = np.ascontiguousarray(x, dtype=np.float64)
    K = int(nchains)
    if a.ndim != 2 or K < 1 or a.shape[1] < 1 or a.shape[0] < max(K, 2) or a.shape[0] % K:
        raise ValueError("x must be a (nchains * nsamp) x m matrix (draws x columns) with at least 2 draws and m >= 1")
    w = None if weights is None else stack_weights_array(weights, K)
    S, m = a.shape
    mean, cov = np.empty(m), np.empty((m, m))
    check(_device_lib().bnr_cov(int(device), K, S // K, m, _ptr(a), _ptr(w), _ptr(mean), _ptr(cov)))
    return mean, cov


# ------------------------------------------------------------------------------------------ marginal PSIS-LOO (libbnr_mloo.so, include/bnr_mloo.h)
MLOO_FIELDS = ("loglik", "resid", "var", "logml")


def _phi_arrays(X, y, tau2, mu, S, W):
    """(Xf, yf, t2, mu, Sf, Wf, n, q, D): the model matrix (column-major) and D draws phi = (tau2, mu, S, W) of a raw marginal call as contiguous
    float64 arrays; ValueError for shapes that do not fit or n > 2048"""
    Xf = np.asfortranarray(X, dtype=np.float64)
    if Xf.ndim != 2 or Xf.shape[0] < 1 or Xf.shape[1] < 1:
        raise ValueError("X must be an n x q matrix with n, q >= 1")
    n, q = Xf.shape
    if n > MLOO_MAX_N:
        raise ValueError("n = %d: more than %d rows are not supported by this version" % (n, MLOO_MAX_N))
    yf = np.ascontiguousarray(y, dtype=np.float64).reshape(-1)
    t2 = np.ascontiguousarray(np.atleast_1d(np.asarray(tau2, dtype=np.float64))).reshape(-1)
    D = t2.size
    mu_ = np.ascontiguousarray(np.atleast_1d(np.asarray(mu, dtype=np.float64))).reshape(-1)
    Sf = np.ascontiguousarray(np.asarray(S, dtype=np.float64).reshape(-1, q))
    Wf = None if W is None else np.ascontiguousarray(np.asarray(W, dtype=np.float64).reshape(-1, q))
    if yf.shape != (n,) or D < 1 or mu_.shape != (D,) or Sf.shape != (D, q) or (Wf is not None and Wf.shape != (D, q)):
        raise ValueError("need y (n,), tau2 and mu (D,), S and W (D, q) for X (n, q)")
    return Xf, yf, t2, mu_, Sf, Wf, n, q, D


def marginal_loglik_raw(X, y, tau2, mu, S, W=None, device=0, fields=MLOO_FIELDS):
    """(loglik, resid, var (n x D each), logml (D,), n_bad) of D draws phi = (tau2, mu, S, W) for one n x q model matrix, the edge coefficients
    integrated out, on the device (bnr_marginal_loglik); an entry not named in `fields` is not requested and comes back as None.  ValueError
    (before any library call) for shapes that do not fit, n > 2048 or no matrix asked for"""
    Xf, yf, t2, m, Sf, Wf, n, q, D = _phi_arrays(X, y, tau2, mu, S, W)
    fields = tuple(fields)
    if [f for f in fields if f not in MLOO_FIELDS] or not set(fields) & {"loglik", "resid", "var"}:
        raise ValueError("fields must name loglik, resid or var (and logml), not %r" % (fields,))
    out = [np.empty((n, D)) if f in fields else None for f in MLOO_FIELDS[:3]] + [np.empty(D) if "logml" in fields else None]
    nb = C.c_int32(0)
    check(_device_marginal("mloo").bnr_marginal_loglik(int(device), n, q, D, _ptr(Xf), _ptr(yf), _ptr(t2), _ptr(m), _ptr(Sf), _ptr(Wf), *[_ptr(o) for o in out],
                                             C.byref(nb)))
    return tuple(out) + (nb.value,)


def mloo_thin_draws(nsamp, thin):
    """(thin, the draws per chain ceil(nsamp / thin)) of a marginal LOO call; ValueError unless thin >= 1 and nsamp >= 1"""
    nsamp, thin = int(nsamp), int(thin)
    if thin < 1 or nsamp < 1:
        raise ValueError("need thin >= 1 and nsamp >= 1, not thin = %d, nsamp = %d" % (thin, nsamp))
    return thin, (nsamp + thin - 1) // thin


def _pooled_window(chains, nsamp, thin):
    """(the first chain, the chain array, K, thin, the draws per chain) of a chain-form marginal call; ValueError for a bad window or n > 2048"""
    c0, (arr, K) = _pooled(chains)
    thin, nd = mloo_thin_draws(nsamp, thin)
    if c0.n > MLOO_MAX_N:
        raise ValueError("n = %d: more than %d rows are not supported by this version" % (c0.n, MLOO_MAX_N))
    return c0, arr, K, thin, nd


def chains_marginal_loo(chains, first_row, nsamp, thin=1, r_eff=None, loglik=False):
    """(elpd_loo, pareto_k, loo_mean, loo_sd (n,), logml (K draws,), loglik (n, K draws) or None, n_bad) over rows first_row + j thin of every
    chain listed (bnr_chains_marginal_loo)"""
    c0, arr, K, thin, nd = _pooled_window(chains, nsamp, thin)
    n, D = c0.n, K * nd
    r = r_eff_array(r_eff, n)
    el, kh, lm, ls, ml = np.empty(n), np.empty(n), np.empty(n), np.empty(n), np.empty(D)
    ll = np.empty((n, D)) if loglik else None
    nb = C.c_int32(0)
    check(_device_marginal("mloo").bnr_chains_marginal_loo(arr, K, int(first_row), int(nsamp), thin, _ptr(r), _ptr(el), _ptr(kh), _ptr(lm), _ptr(ls), _ptr(ml),
                                                 _ptr(ll), C.byref(nb)))
    return el, kh, lm, ls, ml, ll, nb.value


# ------------------------------------------------------------------------------------------ Rao-Blackwellised edge summaries (libbnr_medge.so, include/bnr_medge.h)
MEDGE_SUMMARY_FIELDS = ("mean", "sd", "var_within", "p_pos", "p_neg", "lower", "upper")


def marginal_gamma_raw(X, y, tau2, mu, S, W=None, device=0):
    """(m, v (D x q each), n_bad): the conditional mean and variance of every edge coefficient given each of D draws phi = (tau2, mu, S, W) for
    one n x q model matrix, on the device (bnr_marginal_gamma).  ValueError (before any library call) for shapes that do not fit or n > 2048"""
    Xf, yf, t2, mu_, Sf, Wf, n, q, D = _phi_arrays(X, y, tau2, mu, S, W)
    m, v = np.empty((D, q)), np.empty((D, q))
    nb = C.c_int32(0)
    check(_device_marginal("medge").bnr_marginal_gamma(int(device), n, q, D, _ptr(Xf), _ptr(yf), _ptr(t2), _ptr(mu_), _ptr(Sf), _ptr(Wf), _ptr(m), _ptr(v),
                                             C.byref(nb)))
    return m, v, nb.value


def _medge_outputs(q, fields):
    fields = tuple(fields)
    if not fields or [f for f in fields if f not in MEDGE_SUMMARY_FIELDS] or (("lower" in fields) != ("upper" in fields)):
        raise ValueError("fields must name some of %r, lower and upper together, not %r" % (MEDGE_SUMMARY_FIELDS, fields))
    return [np.empty(q) if f in fields else None for f in MEDGE_SUMMARY_FIELDS]


def mixture_summary_raw(m, v, nchains=1, weights=None, p_lo=0.025, p_hi=0.975, device=0, fields=MEDGE_SUMMARY_FIELDS):
    """the tuple MEDGE_SUMMARY_FIELDS (q values each) of the mixtures of normals in the columns of the (nchains nd) x q matrices m, v, on the
    device (bnr_mixture_summary); an entry not named in `fields` is not requested and comes back as None"""
    mf, vf = np.ascontiguousarray(m, dtype=np.float64), np.ascontiguousarray(v, dtype=np.float64)
    K = int(nchains)
    if mf.ndim != 2 or mf.shape != vf.shape or K < 1 or mf.shape[1] < 1 or mf.shape[0] < K or mf.shape[0] % K:
        raise ValueError("m and v must be (nchains * nd) x q matrices of one shape with nd, q >= 1")
    w = None if weights is None else stack_weights_array(weights, K)
    p_lo, p_hi = loo_probs(p_lo, p_hi)
    D, q = mf.shape
    out = _medge_outputs(q, fields)
    check(_device_marginal("medge").bnr_mixture_summary(int(device), q, K, D // K, _ptr(mf), _ptr(vf), _ptr(w), p_lo, p_hi, *[_ptr(o) for o in out]))
    return tuple(out)


def chains_marginal_edges(chains, first_row, nsamp, thin=1, weights=None, p_lo=0.025, p_hi=0.975, per_draw=False, fields=MEDGE_SUMMARY_FIELDS):
    """(the tuple MEDGE_SUMMARY_FIELDS (q,), m, v (K nd x q) or None, n_bad) over rows first_row + j thin of every chain listed
    (bnr_chains_marginal_edges)"""
    c0, arr, K, thin, nd = _pooled_window(chains, nsamp, thin)
    w = None if weights is None else stack_weights_array(weights, K)
    p_lo, p_hi = loo_probs(p_lo, p_hi)
    q = c0.q
    out = _medge_outputs(q, fields)
    m, v = (np.empty((K * nd, q)), np.empty((K * nd, q))) if per_draw else (None, None)
    nb = C.c_int32(0)
    check(_device_marginal("medge").bnr_chains_marginal_edges(arr, K, _ptr(w), int(first_row), int(nsamp), thin, p_lo, p_hi, *[_ptr(o) for o in out], _ptr(m),
                                                    _ptr(v), C.byref(nb)))
    return tuple(out), m, v, nb.value


# ------------------------------------------------------------------------------------------ Rao-Blackwellised covariance of the edge coefficients (libbnr_mcov.so, include/bnr_mcov.h)
def _mcov_outputs(D, m, per_draw):
    return np.empty(m), np.empty((m, m)), np.empty((m, m)), (np.empty((D, m)) if per_draw else None), (np.empty((D, m)) if per_draw else None)


def marginal_gamma_cov_raw(X, y, tau2, mu, S, W=None, cols=None, nchains=1, weights=None, device=0, per_draw=True):
    """(mean (c,), cov, within (c x c), m, v (D x c) or None, n_bad) of the columns `cols` (None: all q) of the mixture of the D = nchains nd
    conditional normals of gamma given phi = (tau2, mu, S, W), chain k's draws in rows k nd .., on the device (bnr_marginal_gamma_cov)"""
    Xf, yf, t2, mu_, Sf, Wf, n, q, D = _phi_arrays(X, y, tau2, mu, S, W)
    K = int(nchains)
    if K < 1 or D % K:
        raise ValueError("the %d draws do not split into %d chains" % (D, K))
    ci = cov_cols(cols, q)
    w = None if weights is None else stack_weights_array(weights, K)
    c = q if ci is None else ci.size
    mean, cov, within, m, v = _mcov_outputs(D, c, per_draw)
    nb = C.c_int32(0)
    check(_device_marginal("mcov").bnr_marginal_gamma_cov(int(device), n, q, K, D // K, _ptr(Xf), _ptr(yf), _ptr(t2), _ptr(mu_), _ptr(Sf), _ptr(Wf), _ptr(w), c,
                                                None if ci is None else ci.ctypes.data_as(_ip), _ptr(mean), _ptr(cov), _ptr(within), _ptr(m),
                                                _ptr(v), C.byref(nb)))
    return mean, cov, within, m, v, nb.value


def chains_marginal_edge_cov(chains, first_row, nsamp, thin=1, cols=None, weights=None, per_draw=False):
    """(mean (c,), cov, within (c x c), m, v (K nd x c) or None, n_bad) over rows first_row + j thin of every chain listed
    (bnr_chains_marginal_edge_cov)"""
    c0, arr, K, thin, nd = _pooled_window(chains, nsamp, thin)
    ci = cov_cols(cols, c0.q)
    w = None if weights is None else stack_weights_array(weights, K)
    c = c0.q if ci is None else ci.size
    mean, cov, within, m, v = _mcov_outputs(K * nd, c, per_draw)
    nb = C.c_int32(0)
    check(_device_marginal("mcov").bnr_chains_marginal_edge_cov(arr, K, _ptr(w), int(first_row), int(nsamp), thin, c, None if ci is None else ci.ctypes.data_as(_ip),
                                                      _ptr(mean), _ptr(cov), _ptr(within), _ptr(m), _ptr(v), C.byref(nb)))
    return mean, cov, within, m, v, nb.value


# ------------------------------------------------------------------------------------------ Rao-Blackwellised prediction of new rows (libbnr_mpred.so, include/bnr_mpred.h)
MPRED_SUMMARY_FIELDS = ("mean", "sd", "var_within", "lower", "upper", "pred_sd", "pred_lower", "pred_upper", "lpd", "pit")


def marginal_predict_raw(X, y, X_new, tau2, mu, S, W=None, device=0):
    """(mean, var (D x m each), n_bad): the conditional mean and variance of the mean response of every row of X_new (m x q) given each of D draws
    phi = (tau2, mu, S, W) for one n x q model matrix, on the device (bnr_marginal_predict).  ValueError (before any library call) for shapes
    that do not fit or n > 2048"""
    Xf, yf, t2, mu_, Sf, Wf, n, q, D = _phi_arrays(X, y, tau2, mu, S, W)
    Xn = np.asfortranarray(X_new, dtype=np.float64)
    if Xn.ndim != 2 or Xn.shape[0] < 1 or Xn.shape[1] != q:
        raise ValueError("X_new must be an m x q matrix with m >= 1 and the q columns of X")
    m = Xn.shape[0]
    mean, var = np.empty((D, m)), np.empty((D, m))
    nb = C.c_int32(0)
    check(_device_marginal("mpred").bnr_marginal_predict(int(device), n, q, m, D, _ptr(Xf), _ptr(yf), _ptr(Xn), _ptr(t2), _ptr(mu_), _ptr(Sf), _ptr(Wf),
                                               _ptr(mean), _ptr(var), C.byref(nb)))
    return mean, var, nb.value


def mixture_score_raw(mean, vobs, y, nchains=1, weights=None, device=0, fields=("lpd", "pit")):
    """(lpd, pit) (m values each) of the responses y under the mixtures of normals in the columns of the (nchains nd) x m matrices mean, vobs,
    on the device (bnr_mixture_score); an entry not named in `fields` is not requested and comes back as None"""
    mf, vf = np.ascontiguousarray(mean, dtype=np.float64), np.ascontiguousarray(vobs, dtype=np.float64)
    K = int(nchains)
    if mf.ndim != 2 or mf.shape != vf.shape or K < 1 or mf.shape[1] < 1 or mf.shape[0] < K or mf.shape[0] % K:
        raise ValueError("mean and vobs must be (nchains * nd) x m matrices of one shape with nd, m >= 1")
    D, m = mf.shape
    yf = np.ascontiguousarray(y, dtype=np.float64).reshape(-1)
    if yf.shape != (m,):
        raise ValueError("y must hold one response per column of mean")
    fields = tuple(fields)
    if not fields or [f for f in fields if f not in ("lpd", "pit")]:
        raise ValueError("fields must name lpd or pit, not %r" % (fields,))
    w = None if weights is None else stack_weights_array(weights, K)
    out = [np.empty(m) if f in fields else None for f in ("lpd", "pit")]
    check(_device_marginal("mpred").bnr_mixture_score(int(device), m, K, D // K, _ptr(mf), _ptr(vf), _ptr(yf), _ptr(w), _ptr(out[0]), _ptr(out[1])))
    return tuple(out)


def chains_marginal_predict(chains, first_row, nsamp, X_new, y_new=None, thin=1, weights=None, p_lo=0.025, p_hi=0.975, per_draw=False,
                            fields=None):
    """(the tuple MPRED_SUMMARY_FIELDS (m,) -- lpd and pit None without y_new --, mean, var (K nd x m) or None, n_bad) over rows first_row + j thin
    of every chain listed, for the rows of the dense m x q matrix X_new (bnr_chains_marginal_predict)"""
    c0, arr, K, thin, nd = _pooled_window(chains, nsamp, thin)
    q = c0.q
    Xn = np.asfortranarray(X_new, dtype=np.float64)
    if Xn.ndim != 2 or Xn.shape[0] < 1 or Xn.shape[1] != q:
        raise ValueError("X_new must be an m x q matrix with m >= 1 and q = %d columns" % q)
    m = Xn.shape[0]
    yn = None if y_new is None else np.ascontiguousarray(y_new, dtype=np.float64).reshape(-1)
    if yn is not None and yn.shape != (m,):
        raise ValueError("y_new must hold one response per row of X_new")
    w = None if weights is None else stack_weights_array(weights, K)
    p_lo, p_hi = loo_probs(p_lo, p_hi)
    if fields is None:
        fields = MPRED_SUMMARY_FIELDS if yn is not None else MPRED_SUMMARY_FIELDS[:8]
    fields = tuple(fields)
    if (not fields and not per_draw) or [f for f in fields if f not in MPRED_SUMMARY_FIELDS] or (("lower" in fields) != ("upper" in fields)) \
            or (("pred_lower" in fields) != ("pred_upper" in fields)) or (yn is None and set(fields) & {"lpd", "pit"}):
        raise ValueError("fields must name some of %r, lower and upper together, lpd and pit only with y_new, not %r" % (MPRED_SUMMARY_FIELDS, fields))
    out = [np.empty(m) if f in fields else None for f in MPRED_SUMMARY_FIELDS]
    dm, dv = (np.empty((K * nd, m)), np.empty((K * nd, m))) if per_draw else (None, None)
    nb = C.c_int32(0)
    check(_device_marginal("mpred").bnr_chains_marginal_predict(arr, K, _ptr(w), int(first_row), int(nsamp), thin, _ptr(Xn), m, _ptr(yn), p_lo, p_hi,
                                                      *[_ptr(o) for o in out], _ptr(dm), _ptr(dv), C.byref(nb)))
    return tuple(out), dm, dv, nb.value


# ------------------------------------------------------------------------------------------ marginal LOO predictive checks (libbnr_mcheck.so, include/bnr_mcheck.h)
MCHECK_FIELDS = ("mean", "sd", "pit", "lower", "upper")


def _mcheck_fields(fields, has_y):
    fields = tuple(fields)
    if not fields or [f for f in fields if f not in MCHECK_FIELDS] or ("pit" in fields and not has_y):
        raise ValueError("fields must name some of %r, pit only with y, not %r" % (MCHECK_FIELDS, fields))
    return fields


def weighted_mixture_raw(mean, var, log_weights, y=None, p_lo=0.025, p_hi=0.975, device=0, fields=None):
    """the tuple MCHECK_FIELDS (rows values each) of the weighted mixtures of normals in the rows of the rows x D matrices mean, var under the
    normalised log weights log_weights (rows x D), on the device (bnr_weighted_mixture); y (rows,) or None (then no pit); an entry not named in
    `fields` is not requested and comes back as None.  ValueError (before any library call) for shapes that do not fit or rows D >= 2^31"""
    shape = np.shape(mean)
    if len(shape) != 2 or np.shape(var) != shape or np.shape(log_weights) != shape:
        raise ValueError("mean, var and log_weights must be rows x D matrices of one shape")
    if shape[0] * shape[1] >= 2 ** 31:
        raise ValueError("rows x D must stay below 2^31, not %d x %d" % shape)
    mf = _matrix(mean, "mean")
    vf, lf = np.ascontiguousarray(var, dtype=np.float64), np.ascontiguousarray(log_weights, dtype=np.float64)
    rows, D = mf.shape
    yf = None if y is None else np.ascontiguousarray(y, dtype=np.float64).reshape(-1)
    if yf is not None and yf.shape != (rows,):
        raise ValueError("y must hold one response per row of mean")
    if fields is None:
        fields = MCHECK_FIELDS if yf is not None else ("mean", "sd", "lower", "upper")
    fields = _mcheck_fields(fields, yf is not None)
    if set(fields) & {"lower", "upper"}:
        p_lo, p_hi = loo_probs(p_lo, p_hi)
    out = [np.empty(rows) if f in fields else None for f in MCHECK_FIELDS]
    check(_device_marginal("mcheck").bnr_weighted_mixture(int(device), rows, D, _ptr(mf), _ptr(vf), _ptr(lf), _ptr(yf), float(p_lo), float(p_hi),
                                                *[_ptr(o) for o in out]))
    return tuple(out)


def chains_marginal_loo_predict(chains, first_row, nsamp, thin=1, r_eff=None, p_lo=0.025, p_hi=0.975, loglik=False, fields=MCHECK_FIELDS):
    """(elpd_loo, pareto_k (n,), the tuple MCHECK_FIELDS (n,: loo_mean, loo_sd, loo_pit, loo_lower, loo_upper; an entry not named in `fields` is
    not requested and comes back as None), logml (K draws,), loglik (n, K draws) or None, n_bad) over rows first_row + j thin of every chain
    listed (bnr_chains_marginal_loo_predict)"""
    c0, arr, K, thin, nd = _pooled_window(chains, nsamp, thin)
    n, D = c0.n, K * nd
    r = r_eff_array(r_eff, n)
    fields = tuple(fields)
    if [f for f in fields if f not in MCHECK_FIELDS]:
        raise ValueError("fields must name some of %r, not %r" % (MCHECK_FIELDS, fields))
    if set(fields) & {"lower", "upper"}:
        p_lo, p_hi = loo_probs(p_lo, p_hi)
    el, kh, ml = np.empty(n), np.empty(n), np.empty(D)
    out = [np.empty(n) if f in fields else None for f in MCHECK_FIELDS]
    ll = np.empty((n, D)) if loglik else None
    nb = C.c_int32(0)
    check(_device_marginal("mcheck").bnr_chains_marginal_loo_predict(arr, K, int(first_row), int(nsamp), thin, _ptr(r), float(p_lo), float(p_hi), _ptr(el),
                                                           _ptr(kh), *[_ptr(o) for o in out], _ptr(ml), _ptr(ll), C.byref(nb)))
    return el, kh, tuple(out), ml, ll, nb.value


# ------------------------------------------------------------------------------------------ chain stacking on the marginal PSIS-LOO (libbnr_mstack.so, include/bnr_mstack.h)
def stacked_mixture_raw(mean, var, log_weights, weights, nchains, y=None, p_lo=0.025, p_hi=0.975, device=0, fields=None):
    """the tuple MCHECK_FIELDS (rows values each) of the stacked mixtures of normals in the rows of the rows x (nchains nd) matrices mean, var
    (chain k's components in columns k nd .. (k + 1) nd - 1) under the chain weights `weights` and the log weights log_weights, normalised within
    every chain, on the device (bnr_stacked_mixture); y (rows,) or None (then no pit); an entry not named in `fields` is not requested and comes
    back as None.  ValueError (before any library call) for shapes that do not fit or rows D >= 2^31"""
    shape = np.shape(mean)
    K = int(nchains)
    if len(shape) != 2 or np.shape(var) != shape or np.shape(log_weights) != shape:
        raise ValueError("mean, var and log_weights must be rows x (nchains * nd) matrices of one shape")
    if K < 1 or shape[1] < K or shape[1] % K:
        raise ValueError("mean, var and log_weights must be rows x (nchains * nd) matrices with nd >= 1")
    if shape[0] * shape[1] >= 2 ** 31:
        raise ValueError("rows x D must stay below 2^31, not %d x %d" % shape)
    mf = _matrix(mean, "mean")
    vf, lf = np.ascontiguousarray(var, dtype=np.float64), np.ascontiguousarray(log_weights, dtype=np.float64)
    rows, D = mf.shape
    w = stack_weights_array(weights, K)
    yf = None if y is None else np.ascontiguousarray(y, dtype=np.float64).reshape(-1)
    if yf is not None and yf.shape != (rows,):
        raise ValueError("y must hold one response per row of mean")
    if fields is None:
        fields = MCHECK_FIELDS if yf is not None else ("mean", "sd", "lower", "upper")
    fields = _mcheck_fields(fields, yf is not None)
    if set(fields) & {"lower", "upper"}:
        p_lo, p_hi = loo_probs(p_lo, p_hi)
    out = [np.empty(rows) if f in fields else None for f in MCHECK_FIELDS]
    check(_device_marginal("mstack").bnr_stacked_mixture(int(device), rows, K, D // K, _ptr(mf), _ptr(vf), _ptr(lf), _ptr(w), _ptr(yf), float(p_lo),
                                               float(p_hi), *[_ptr(o) for o in out]))
    return tuple(out)


def chains_marginal_stack(chains, first_row, nsamp, thin=1, r_eff=None, weights=None, max_iter=100000, gap_tol=1e-9, p_lo=0.025, p_hi=0.975,
                          fields=MCHECK_FIELDS):
    """(weights (K,), elpd_chain, pareto_k_chain (K x n), elpd_stack (n,), gap, iterations, the tuple MCHECK_FIELDS (n,: loo_mean, loo_sd,
    loo_pit, loo_lower, loo_upper of the stacked mixture; an entry not named in `fields` is not requested and comes back as None), logml
    (K draws,), n_bad) over rows first_row + j thin of every chain listed (bnr_chains_marginal_stack); weights: chain weights to use instead of
    the solver's, or None"""
    c0, arr, K, thin, nd = _pooled_window(chains, nsamp, thin)
    n, D = c0.n, K * nd
    r = r_eff_array(r_eff, n)
    fw = None if weights is None else stack_weights_array(weights, K)
    fields = tuple(fields)
    if [f for f in fields if f not in MCHECK_FIELDS]:
        raise ValueError("fields must name some of %r, not %r" % (MCHECK_FIELDS, fields))
    if set(fields) & {"lower", "upper"}:
        p_lo, p_hi = loo_probs(p_lo, p_hi)
    w, el, kh, es, ml = np.empty(K), np.empty((K, n)), np.empty((K, n)), np.empty(n), np.empty(D)
    out = [np.empty(n) if f in fields else None for f in MCHECK_FIELDS]
    g, it, nb = C.c_double(0.0), C.c_int32(0), C.c_int32(0)
    check(_device_marginal("mstack").bnr_chains_marginal_stack(arr, K, int(first_row), int(nsamp), thin, _ptr(r), _ptr(fw), int(max_iter), float(gap_tol),
                                                     float(p_lo), float(p_hi), _ptr(w), _ptr(el), _ptr(kh), _ptr(es), C.byref(g), C.byref(it),
                                                     *[_ptr(o) for o in out], _ptr(ml), C.byref(nb)))
    return w, el, kh, es, g.value, it.value, tuple(out), ml, nb.value


class Comm:
    """The ranks of one fit (bnr_comm of include/bnr_hip.h): RCCL communicator owned by the library, or a host callback."""

    def __init__(self, handle, rank, world, keep=None):
        self.h, self.rank, self.world, self._keep, self.L = handle, rank, world, keep, lib()

    @staticmethod
    def unique_id():
        uid = UniqueId()
        check(lib().bnr_comm_unique_id(C.byref(uid)))
        return bytes(C.string_at(C.addressof(uid), 128))

    @classmethod
    def rccl(cls, unique_id, rank, world, device):
        """Collective: every rank calls it with rank 0's 128-byte id."""
        uid = UniqueId()
        C.memmove(C.addressof(uid), unique_id, 128)
        h = C.c_void_p()
        check(lib().bnr_comm_create_rccl(C.byref(uid), rank, world, device, C.byref(h)))
        return cls(h, rank, world)

    @classmethod
    def callback(cls, rank, world, allgather):
        """allgather(send: ndarray[count]) -> ndarray[world * count] in rank order (the host's own transport)."""
        def _cb(_ctx, send, recv, count):
            try:
                out = np.ascontiguousarray(allgather(np.ctypeslib.as_array(send, shape=(count,)).copy()), dtype=np.float64).reshape(-1)
                if out.size != world * count:
                    return 2
                C.memmove(recv, out.ctypes.data, 8 * out.size)
                return 0
            except Exception:                                                      # no exception may cross the ABI
                import traceback
                traceback.print_exc()
                return 1
        fn = ALLGATHER_CB(_cb)
        h = C.c_void_p()
        check(lib().bnr_comm_create_callback(rank, world, fn, None, C.byref(h)))
        return cls(h, rank, world, keep=fn)

    def allgather(self, send):
        s = np.ascontiguousarray(send, dtype=np.float64).reshape(-1)
        out = np.empty(self.world * s.size)
        check(self.L.bnr_comm_allgather(self.h, _ptr(s), _ptr(out), s.size))
        return out.reshape(self.world, s.size)

    def info(self):
        """bnr_comm_info: what the transport itself reports -- {'kind': 'rccl' | 'callback', 'rank', 'world', 'rccl_ranks' (ncclCommCount; 0 unless RCCL), 'rccl_rank'}."""
        v = [C.c_int32() for _ in range(5)]
        check(self.L.bnr_comm_info(self.h, *[C.byref(x) for x in v]))
        kind, rank, world, nr, ur = [x.value for x in v]
        return {"kind": {0: "none", 1: "rccl", 2: "callback"}[kind], "rank": rank, "world": world, "rccl_ranks": nr, "rccl_rank": ur}

    def close(self):
        h, self.h = getattr(self, "h", None), None
        if h and h.value and getattr(self, "L", None) is not None:
            self.L.bnr_comm_destroy(h)

    __del__ = close


def rhat(chains, nchains_total, comm, burn, nsamp, V=None, q=None):
    """bnr_rhat: split-Rhat of gamma and xi over ALL chains of the fit; `chains` = this rank's Chain objects in increasing
    chain id.  Returns (rhat_gamma[q], rhat_xi[V]).  V, q are needed on a rank that holds no chain."""
    if chains:
        V, q = chains[0].V, chains[0].q
    rx, rg = np.empty(V), np.empty(q)
    arr = (C.c_void_p * max(1, len(chains)))(*[ch.h for ch in chains])
    check(lib().bnr_rhat(arr, len(chains), nchains_total, comm.h if comm is not None else None, burn, nsamp, _ptr(rx), _ptr(rg)))
    return rg, rx


def ess_from_stats(stats, nsamp, max_lag):
    """Bulk effective sample size from the gathered per-chain messages (nchains, 2 * (2 + max_lag) * nparams)."""
    st = np.ascontiguousarray(stats, dtype=np.float64)
    nch = st.shape[0]
    npar = st.shape[1] // (2 * (2 + max_lag))
    out = np.empty(npar)
    check(lib().bnr_ess_from_stats(_ptr(st), nch, npar, nsamp, max_lag, _ptr(out)))
    return out


def rhat_from_stats(stats, nsamp):
    """stats: (nchains, 4*nparams) -> rhat (nparams,)   second half of convergence.jl:4-65."""
    s = np.ascontiguousarray(stats, dtype=np.float64)
    nchains, w = s.shape
    out = np.empty(w // 4)
    check(lib().bnr_rhat_from_stats(_ptr(s), nchains, w // 4, nsamp, _ptr(out)))
    return out
