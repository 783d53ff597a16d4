"""ctypes binding of the C ABI in include/autoreparam.h.

The shared library is the product: if it is missing or fails to load this module
raises -- there is no CPU fallback on the product path (the CPU restatement under
oracle/ is test infrastructure and is never imported from here).
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# ARP_LIB_PATH: timing experiments only (a variant built with ARP_HIPCC_FLAGS / ARP_BUILD_TAG); honoured under
# ARP_DEBUG=1 only and announced on stderr
LIB_PATH = os.path.join(_HERE, "libautoreparam_hip.so")
if os.environ.get("ARP_LIB_PATH"):
    import sys as _sys
    if os.environ.get("ARP_DEBUG") == "1":
        LIB_PATH = os.environ["ARP_LIB_PATH"]
        print("autoreparam_amd: DEBUG SWITCH ARP_LIB_PATH=%s is in effect (ARP_DEBUG=1)" % LIB_PATH, file=_sys.stderr, flush=True)
    else:
        print("autoreparam_amd: ARP_LIB_PATH IGNORED (experiment switch; set ARP_DEBUG=1 to enable it)", file=_sys.stderr, flush=True)

MODEL_EIGHT_SCHOOLS, MODEL_RADON, MODEL_GERMAN_CREDIT, MODEL_ELECTION, MODEL_RADON_STDDVS = 0, 1, 2, 3, 4
MODEL_NEALS_FUNNEL = 5
MODEL_ELECTRIC = 6
MODEL_TIME_SERIES = 7
ADAPT_NONE, ADAPT_DUAL, ADAPT_SIMPLE = 0, 1, 2
RNG_SLOTS = 16  # rng buffer is [C][16][4] uint32

_f32p = C.POINTER(C.c_float)
_i32p = C.POINTER(C.c_int32)


class Dataset(C.Structure):
    _fields_ = [("model", C.c_int32), ("n_obs", C.c_int32), ("n_groups", C.c_int32),
                ("n_features", C.c_int32),
                ("group_host", _i32p), ("u_host", _f32p), ("x_host", _f32p), ("x2_host", _f32p),
                ("y_host", _f32p), ("X_host", _f32p), ("group2_host", _i32p), ("group3_host", _i32p)]


class HmcConfig(C.Structure):
    _fields_ = [("n_chains", C.c_int32), ("n_leapfrog", C.c_int32), ("n_steps", C.c_int32),
                ("step_base", C.c_int64), ("chain_offset", C.c_int64), ("seed", C.c_uint64),
                ("adapt_kind", C.c_int32), ("n_adapt", C.c_int32),
                ("adapt_target", C.c_float), ("adapt_rate", C.c_float),
                ("n_burnin", C.c_int32), ("thin", C.c_int32), ("n_samples", C.c_int32),
                ("trace_centered", C.c_int32), ("lanes_per_chain", C.c_int32), ("stats_batch", C.c_int32),
                ("trace_chains", C.c_int32), ("reserved", C.c_int32)]


class HmcIO(C.Structure):
    _fields_ = [("q", C.c_void_p), ("grad", C.c_void_p), ("logp", C.c_void_p), ("adapt", C.c_void_p),
                ("rng", C.c_void_p), ("accept_count", C.c_void_p), ("eps0", C.c_void_p),
                ("trace", C.c_void_p), ("trace_accept", C.c_void_p), ("stats", C.c_void_p),
                ("rec_accept_count", C.c_void_p)]


class InterleavedIO(C.Structure):
    _fields_ = [("k0", HmcIO), ("adapt1", C.c_void_p), ("accept_count1", C.c_void_p),
                ("eps0_1", C.c_void_p), ("trace_accept1", C.c_void_p), ("rec_accept_count1", C.c_void_p)]


class ViConfig(C.Structure):
    _fields_ = [("n_lr", C.c_int32), ("n_steps", C.c_int32), ("n_mc", C.c_int32),
                ("learn_a", C.c_int32), ("tied_b", C.c_int32), ("a_prior", C.c_int32),
                ("seed", C.c_uint64)]


class ViIO(C.Structure):
    _fields_ = [("lr", C.c_void_p), ("loc", C.c_void_p), ("rho", C.c_void_p), ("w", C.c_void_p),
                ("wb", C.c_void_p), ("elbo", C.c_void_p), ("prior", C.c_void_p), ("a_group", C.c_void_p),
                ("b_group", C.c_void_p)]


# every symbol include/autoreparam.h declares
SYMBOLS = ["arp_version", "arp_last_error", "arp_model_create", "arp_model_destroy", "arp_model_dim",
           "arp_model_logp_const", "arp_model_set_param", "arp_model_set_option", "arp_logp_grad", "arp_transform",
           "arp_hmc_run", "arp_interleaved_run", "arp_model_check", "arp_vi_run", "arp_vi_geometry", "arp_vi_attempts", "arp_relay_geometry", "arp_relay_schedule", "arp_ess", "arp_ess_ws", "arp_ess_workspace_bytes",
           "arp_moments_workspace_bytes", "arp_split_moments", "arp_moments_fold",
           "arp_rank_workspace_bytes", "arp_rank_normalize",
           "arp_ess_multichain_workspace_bytes", "arp_ess_multichain",
           "arp_moments_fold_nested", "arp_nested_step_workspace_bytes", "arp_nested_step_sums",
           "arp_gram_workspace_bytes", "arp_gram_sums",
           "arp_pointwise_loglik", "arp_psis_workspace_bytes", "arp_psis_loo",
           "arp_psis_weights_workspace_bytes", "arp_psis_weights",
           "arp_vi_draws", "arp_vi_fold_workspace_bytes", "arp_vi_fold",
           "arp_predictive_workspace_bytes", "arp_predictive_check", "arp_group_predictive_check",
           "arp_group_loglik",
           "arp_weighted_moments_workspace_bytes", "arp_weighted_moments", "arp_affine_rows",
           "arp_loo_predictive_workspace_bytes", "arp_loo_predictive",
           "arp_loglik_total", "arp_element_order_workspace_bytes", "arp_element_order", "arp_cjs_sums",
           "arp_site_logprior", "arp_site_prior_draws", "arp_site_redraw", "arp_sbc_fold",
           "arp_adapt_probe", "arp_clock_probe", "arp_energy_probe",
           "arp_trajectory_probe", "arp_jump_workspace_bytes", "arp_jump_sums"]

_lib = None


def lib():
    """Load (once) and return the HIP engine; raises if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            "autoreparam_amd: %s is missing -- build it with `python -c 'import __graft_entry__ as g; "
            "g.build()'` (hipcc --offload-arch=gfx950). There is no CPU fallback." % LIB_PATH)
    L = C.CDLL(LIB_PATH)
    L.arp_version.restype = C.c_int
    L.arp_last_error.restype = C.c_char_p
    L.arp_model_create.argtypes = [C.POINTER(Dataset), C.POINTER(C.c_void_p)]
    L.arp_model_destroy.argtypes = [C.c_void_p]
    L.arp_model_dim.argtypes = [C.c_void_p]
    L.arp_model_logp_const.argtypes = [C.c_void_p, C.c_int]
    L.arp_model_logp_const.restype = C.c_double
    L.arp_model_set_param.argtypes = [C.c_void_p, C.c_int, _f32p, _f32p]
    L.arp_model_set_option.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p]
    L.arp_logp_grad.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                C.c_int, C.c_void_p]
    L.arp_transform.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    L.arp_energy_probe.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_void_p, C.c_uint64,
                                   C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    L.arp_energy_probe.restype = C.c_int
    L.arp_trajectory_probe.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_void_p, C.c_uint64,
                                       C.c_int64, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p]
    L.arp_trajectory_probe.restype = C.c_int
    L.arp_jump_workspace_bytes.argtypes = [C.c_int64, C.c_int32, C.c_int32]
    L.arp_jump_workspace_bytes.restype = C.c_int64
    L.arp_jump_sums.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p,
                                C.c_int64, C.c_void_p]
    L.arp_jump_sums.restype = C.c_int
    L.arp_hmc_run.argtypes = [C.c_void_p, C.c_int, C.POINTER(HmcConfig), C.POINTER(HmcIO), C.c_void_p]
    L.arp_interleaved_run.argtypes = [C.c_void_p, C.POINTER(HmcConfig), C.c_int,
                                      C.POINTER(InterleavedIO), C.c_void_p]
    L.arp_vi_run.argtypes = [C.c_void_p, C.c_int, C.POINTER(ViConfig), C.POINTER(ViIO), C.c_void_p]
    L.arp_vi_geometry.argtypes = [C.POINTER(C.c_int32)]
    L.arp_vi_attempts.argtypes = [C.POINTER(C.c_int32)]
    L.arp_relay_geometry.argtypes = [C.POINTER(C.c_int32)]
    L.arp_relay_schedule.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int32), C.c_int]
    L.arp_relay_schedule.restype = C.c_int
    L.arp_model_check.argtypes = [C.c_void_p]
    L.arp_ess.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p]
    L.arp_ess_ws.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
    L.arp_ess_ws.restype = C.c_int
    L.arp_ess_workspace_bytes.argtypes = [C.c_int64, C.c_int64]
    L.arp_ess_workspace_bytes.restype = C.c_int64
    L.arp_moments_workspace_bytes.argtypes = [C.c_int64, C.c_int64, C.c_int]
    L.arp_moments_workspace_bytes.restype = C.c_int64
    L.arp_split_moments.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_int, C.c_void_p, C.c_void_p,
                                    C.c_void_p, C.c_int64, C.c_void_p]
    L.arp_split_moments.restype = C.c_int
    L.arp_moments_fold.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p]
    L.arp_moments_fold.restype = C.c_int
    L.arp_rank_workspace_bytes.argtypes = [C.c_int64, C.c_int64, C.c_int32, C.c_int]
    L.arp_rank_workspace_bytes.restype = C.c_int64
    L.arp_rank_normalize.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.c_int64, C.c_int, C.c_void_p,
                                     C.c_void_p, C.c_void_p, C.POINTER(C.c_double), C.c_int32, C.c_void_p,
                                     C.c_void_p, C.c_int64, C.c_void_p]
    L.arp_rank_normalize.restype = C.c_int
    L.arp_ess_multichain_workspace_bytes.argtypes = [C.c_int64, C.c_int64, C.c_int32, C.c_int]
    L.arp_ess_multichain_workspace_bytes.restype = C.c_int64
    L.arp_ess_multichain.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.c_int64, C.c_int, C.c_void_p,
                                     C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p]
    L.arp_ess_multichain.restype = C.c_int
    L.arp_moments_fold_nested.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int64, C.c_void_p, C.c_void_p]
    L.arp_moments_fold_nested.restype = C.c_int
    L.arp_nested_step_workspace_bytes.argtypes = [C.c_int64, C.c_int64, C.c_int32, C.c_int64]
    L.arp_nested_step_workspace_bytes.restype = C.c_int64
    L.arp_nested_step_sums.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.c_int64, C.c_int64, C.c_void_p,
                                       C.c_void_p, C.c_int64, C.c_void_p]
    L.arp_nested_step_sums.restype = C.c_int
    L.arp_gram_workspace_bytes.argtypes = [C.c_int64, C.c_int64, C.c_int32]
    L.arp_gram_workspace_bytes.restype = C.c_int64
    L.arp_gram_sums.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.c_int64, C.c_void_p, C.c_void_p,
                                C.c_void_p, C.c_int64, C.c_void_p]
    L.arp_gram_sums.restype = C.c_int
    L.arp_pointwise_loglik.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.c_int64, C.c_int32, C.c_void_p,
                                       C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64,
                                       C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]
    L.arp_pointwise_loglik.restype = C.c_int
    L.arp_psis_workspace_bytes.argtypes = [C.c_int64, C.c_int64]
    L.arp_psis_workspace_bytes.restype = C.c_int64
    L.arp_psis_loo.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64,
                               C.c_void_p]
    L.arp_psis_loo.restype = C.c_int
    L.arp_predictive_workspace_bytes.argtypes = [C.c_int64, C.c_int64]
    L.arp_predictive_workspace_bytes.restype = C.c_int64
    L.arp_predictive_check.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.c_int64, C.c_int32, C.c_void_p,
                                       C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64,
                                       C.c_uint64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p,
                                       C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
    L.arp_predictive_check.restype = C.c_int
    L.arp_group_predictive_check.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.c_int64, C.c_int32, C.c_void_p,
                                             C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p,
                                             C.c_int64, C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_uint64, C.c_int64,
                                             C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.arp_group_predictive_check.restype = C.c_int
    L.arp_group_loglik.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p,
                                   C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64,
                                   C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int64] + [C.c_void_p] * 8 + [
        C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]
    L.arp_group_loglik.restype = C.c_int
    L.arp_weighted_moments_workspace_bytes.argtypes = [C.c_int64, C.c_int32, C.c_int64]
    L.arp_weighted_moments_workspace_bytes.restype = C.c_int64
    L.arp_weighted_moments.argtypes = [C.c_void_p, C.c_int64, C.c_int32, C.c_int64, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p,
                                       C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
    L.arp_weighted_moments.restype = C.c_int
    L.arp_affine_rows.argtypes = [C.c_void_p, C.c_int64, C.c_int32, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64,
                                  C.c_int32, C.c_void_p, C.c_void_p]
    L.arp_affine_rows.restype = C.c_int
    L.arp_loo_predictive_workspace_bytes.argtypes = [C.c_int64, C.c_int64]
    L.arp_loo_predictive_workspace_bytes.restype = C.c_int64
    L.arp_loo_predictive.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.c_int64, C.c_int32, C.c_void_p,
                                     C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64,
                                     C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
    L.arp_loo_predictive.restype = C.c_int
    L.arp_loglik_total.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p]
    L.arp_loglik_total.restype = C.c_int
    L.arp_element_order_workspace_bytes.argtypes = [C.c_int64, C.c_int64, C.c_int32]
    L.arp_element_order_workspace_bytes.restype = C.c_int64
    L.arp_element_order.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.c_int64, C.c_void_p, C.c_void_p,
                                    C.c_void_p, C.c_int64, C.c_void_p]
    L.arp_element_order.restype = C.c_int
    L.arp_cjs_sums.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p,
                               C.c_void_p, C.c_void_p]
    L.arp_cjs_sums.restype = C.c_int
    L.arp_site_logprior.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.c_int64] + [C.c_void_p] * 9 + [
        C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.arp_site_logprior.restype = C.c_int
    L.arp_site_prior_draws.argtypes = [C.c_int32] + [C.c_void_p] * 7 + [C.c_int64, C.c_uint64, C.c_int64, C.c_void_p, C.c_int64,
                                                                       C.c_void_p, C.c_void_p]
    L.arp_site_prior_draws.restype = C.c_int
    L.arp_site_redraw.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.c_int64] + [C.c_void_p] * 8 + [
        C.c_uint64, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
    L.arp_site_redraw.restype = C.c_int
    L.arp_sbc_fold.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.c_int64, C.c_int64, C.c_void_p, C.c_int64,
                               C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.arp_sbc_fold.restype = C.c_int
    L.arp_psis_weights_workspace_bytes.argtypes = [C.c_int64, C.c_int64]
    L.arp_psis_weights_workspace_bytes.restype = C.c_int64
    L.arp_psis_weights.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64,
                                   C.c_void_p, C.c_int64, C.c_void_p]
    L.arp_psis_weights.restype = C.c_int
    L.arp_vi_draws.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int64, C.c_uint64, C.c_int64, C.c_void_p, C.c_void_p,
                               C.c_int64, C.c_void_p, C.c_void_p]
    L.arp_vi_draws.restype = C.c_int
    L.arp_vi_fold_workspace_bytes.argtypes = [C.c_int64, C.c_int32]
    L.arp_vi_fold_workspace_bytes.restype = C.c_int64
    L.arp_vi_fold.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                              C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
    L.arp_vi_fold.restype = C.c_int
    L.arp_clock_probe.argtypes = [C.c_int, C.c_void_p, C.c_void_p]
    L.arp_adapt_probe.argtypes = [C.POINTER(HmcConfig), C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    _lib = L
    return L


def check(rc):
    if rc != 0:
        raise RuntimeError("autoreparam engine: " + lib().arp_last_error().decode("utf-8", "replace"))


def ptr(t):
    """The device pointer argument for tensor `t`; NULL for None."""
    return C.c_void_p(t.data_ptr() if t is not None else 0)


def stream():
    """The stream argument of an entry point: torch's current stream on the current device."""
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def host64(x):
    """A tensor (wherever it lives) or anything numpy reads, as float64 numpy."""
    import numpy as np
    import torch
    return np.asarray(x.cpu() if torch.is_tensor(x) else x, np.float64)


def call(device, fn, *args, workspace=None):
    """check(fn(*args, stream())) with `device` current.  workspace=need, for an entry point that ends in (workspace,
    workspace_bytes, stream): a uint8 tensor of `need` bytes on `device` is passed and lives until the call returns when
    need > 0, (NULL, 0) otherwise.  Launches only: nothing here waits for the device or copies."""
    import torch
    with torch.cuda.device(device):
        if workspace is not None:
            need = int(workspace)
            ws = torch.empty(need, dtype=torch.uint8, device=device) if need > 0 else None
            args += (ptr(ws), need)
        check(fn(*args, stream()))


def device_operand(t, dtype, shape, who, name, dims):
    """`t`, an optional device operand of `who`: None, or a contiguous `dtype` tensor of `shape` on the GPU (`dims`: the
    shape as the message spells it); raises ValueError otherwise."""
    import torch
    if t is not None and not (torch.is_tensor(t) and t.is_cuda and t.dtype == dtype and t.is_contiguous()
                              and tuple(t.shape) == tuple(shape)):
        raise ValueError("%s: %s must be a contiguous %s [%s] tensor on the GPU" % (who, name, str(dtype)[len("torch."):], dims))
    return t


def trace_view(trace, who):
    """(x, S, C, D, row_stride) of a float32 [S, C, D] device trace as the diagnostics kernels read it: rows of C * D
    adjacent floats, `row_stride` floats apart.  A contiguous trace and a leading or inner block of chains of a wider one
    ([S, i:j, D] of [S, K, D]: rows stay rows, further apart) are taken in place, x is trace; anything else is copied."""
    import torch
    if not (trace.is_cuda and trace.dtype == torch.float32 and trace.dim() == 3):
        raise ValueError(who + ": a float32 [S, C, D] trace on the GPU is required (there is no CPU fallback)")
    S, Cn, D = trace.shape
    in_place = trace.is_contiguous() or (trace.stride(2) == 1 and trace.stride(1) == D and S > 1)
    x = trace if in_place else trace.contiguous()
    return x, S, Cn, D, (x.stride(0) if S > 1 else Cn * D)
