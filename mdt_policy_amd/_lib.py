"""ctypes binding of libmdt_hip.so (include/mdt_hip.h, include/mdt_hip_ops.h).

The product path has NO fallback: if the HIP library cannot be loaded (or built with hipcc) every entry
point raises.  PyTorch-ROCm is only used by callers for device memory and streams; nothing here imports torch.
"""
from __future__ import annotations

import ctypes as C
import os
import threading

from . import build as _build

c_float_p = C.POINTER(C.c_float)


class MDTHipError(RuntimeError):
    def __init__(self, status: int, message: str):
        super().__init__(f"libmdt_hip status {status}: {message}")
        self.status = status


class MDTConfig(C.Structure):
    _fields_ = [(n, C.c_int32) for n in (
        "arch", "embed_dim", "n_heads", "n_enc_layers", "n_dec_layers", "action_dim", "obs_dim", "goal_dim",
        "n_obs_token", "goal_seq_len", "action_seq_len", "use_mlp_goal", "use_modality_encoder", "use_abs_pos_emb",
        "use_rot_embed", "use_ada_conditioning", "use_noise_encoder", "linear_output", "bias")] + [
        ("sigma_data", C.c_float), ("no_goal_conditioning", C.c_int32), ("proprio_dim", C.c_int32),
        ("use_proprio", C.c_int32)]


class GemmArgs(C.Structure):
    _fields_ = [
        ("A", C.c_void_p), ("lda", C.c_int64), ("Wp", C.c_void_p), ("bias", C.c_void_p), ("out", C.c_void_p),
        ("ldo", C.c_int64), ("M", C.c_int32), ("N", C.c_int32), ("K", C.c_int32), ("ln", C.c_int32),
        ("ln_w", C.c_void_p), ("ln_b", C.c_void_p), ("mod", C.c_void_p), ("mod_stride", C.c_int64),
        ("shift_off", C.c_int32), ("scale_off", C.c_int32), ("rows_per_sample", C.c_int32), ("act", C.c_int32),
        ("residual", C.c_int32), ("gate_off", C.c_int32), ("gin", C.c_int32), ("gout", C.c_int32),
        ("goff", C.c_int32), ("rowvec", C.c_void_p), ("batch", C.c_int32), ("bs_a", C.c_int64), ("bs_w", C.c_int64),
        ("bs_out", C.c_int64), ("aux", C.c_void_p), ("aux_mode", C.c_int32), ("a_parts", C.c_int32),
        ("a_part_stride", C.c_int64), ("a_merged", C.c_void_p), ("Wp_split", C.c_void_p), ("Wp_pair", C.c_void_p)]


class AttnArgs(C.Structure):
    _fields_ = [
        ("q", C.c_void_p), ("ldq", C.c_int64), ("k", C.c_void_p), ("v", C.c_void_p), ("ldkv", C.c_int64),
        ("out", C.c_void_p), ("ldo", C.c_int64), ("B", C.c_int32), ("H", C.c_int32), ("hd", C.c_int32),
        ("Tq", C.c_int32), ("Tk", C.c_int32), ("causal", C.c_int32), ("rope", C.c_int32)]


class XFoldArgs(C.Structure):
    _fields_ = [("kv", C.c_void_p), ("ldkv", C.c_int64), ("WqT_p", C.c_void_p), ("bq", C.c_void_p), ("Wo_p", C.c_void_p),
                ("U", C.c_void_p), ("Wf", C.c_void_p), ("c", C.c_void_p), ("B", C.c_int32), ("H", C.c_int32),
                ("hd", C.c_int32), ("D", C.c_int32), ("Te", C.c_int32)]


class XApplyArgs(C.Structure):
    _fields_ = [("y", C.c_void_p), ("ln_w", C.c_void_p), ("ln_b", C.c_void_p), ("U", C.c_void_p), ("Wf", C.c_void_p),
                ("c", C.c_void_p), ("bo", C.c_void_p), ("B", C.c_int32), ("H", C.c_int32), ("D", C.c_int32),
                ("Te", C.c_int32), ("Ta", C.c_int32), ("y_out", C.c_void_p)]


class HeadArgs(C.Structure):
    _fields_ = [
        ("y", C.c_void_p), ("ln_w", C.c_void_p), ("ln_b", C.c_void_p), ("Wp", C.c_void_p), ("bp", C.c_void_p),
        ("x", C.c_void_p), ("sigma", C.c_void_p), ("sigma_stride", C.c_int64), ("out", C.c_void_p),
        ("M", C.c_int32), ("D", C.c_int32), ("A", C.c_int32), ("rows_per_sample", C.c_int32), ("mode", C.c_int32),
        ("step", C.c_void_p), ("sigma_data", C.c_float), ("y_next", C.c_void_p), ("Wa", C.c_void_p),
        ("ba", C.c_void_p), ("no_ln", C.c_int32), ("y_parts", C.c_int32), ("y_part_stride", C.c_int64)]


class SamplerParams(C.Structure):
    """mdt_sampler_params (include/mdt_hip.h)."""
    _fields_ = [(n, C.c_float) for n in ("eta", "s_churn", "s_tmin", "s_tmax", "s_noise", "r")] + [("order", C.c_int32)]


SAMPLER_MAX_STEPS, SAMPLER_MAX_EVALS, SAMPLER_NREG = 64, 128, 10
# mdt_sampler_kind: gc_sampling function name (without "sample_") -> kind
SAMPLER_KIND = {"euler": 0, "euler_ancestral": 1, "heun": 2, "dpm_2": 3, "dpm_2_ancestral": 4, "lms": 5, "dpmpp_2s": 6,
                "dpmpp_2s_ancestral": 7, "dpmpp_2m": 8, "dpmpp_2_with_lms": 8, "dpmpp_sde": 9, "dpm_fast": 10}


class SamplerEval(C.Structure):
    """mdt_sampler_eval (include/mdt_hip.h): one denoiser evaluation of a sampler plan."""
    _fields_ = [("sigma", C.c_float), ("sigma_next", C.c_float), ("cx", C.c_float * SAMPLER_NREG),
                ("cy", C.c_float * (SAMPLER_NREG + 1)), ("push", C.c_int32), ("noise", C.c_int32 * 2), ("draws", C.c_int32),
                ("step", C.c_int32), ("t", C.c_float), ("ends_step", C.c_int32), ("begins_step", C.c_int32),
                ("pad", C.c_int32 * 1)]


class BrownianSource(C.Structure):
    """mdt_brownian_source (include/mdt_hip.h): the tree of a tree-noise dpmpp_sde call."""
    _fields_ = [("seeds", C.c_void_p), ("n_seeds", C.c_int32), ("pad", C.c_int32), ("lo", C.c_double), ("hi", C.c_double),
                ("tol", C.c_double)]


BROWNIAN_MAX_PAIRS = 64  # MDT_BROWNIAN_MAX_PAIRS


class SampleOpts(C.Structure):
    """mdt_sample_opts (include/mdt_hip.h): bounds, record, guidance, tree noise and pinned actions of mdt_sample_opt /
    mdt_sample_dev_opt / mdt_sample_ddim_opt / mdt_sample_ddim_dev_opt."""
    _fields_ = [("size", C.c_int32), ("cond_lambda", C.c_float), ("lo", C.c_void_p), ("hi", C.c_void_p), ("record", C.c_void_p),
                ("tree", C.POINTER(BrownianSource)), ("pin_known", C.c_void_p), ("pin_keep", C.c_void_p)]


class SelectSpec(C.Structure):
    """mdt_select_spec (include/mdt_hip.h): the score and the selection of mdt_sample_select / _dev_select / mdt_sample_ddim_select /
    _ddim_dev_select."""
    _fields_ = [("size", C.c_int32), ("sigmas_host", C.POINTER(C.c_float)), ("weights_host", C.POINTER(C.c_float)),
                ("n_levels", C.c_int32), ("noise", C.c_void_p), ("draws", C.c_int32), ("chunks", C.c_void_p),
                ("scores", C.c_void_p), ("index", C.c_void_p)]


class SamplerPlan(C.Structure):
    """mdt_sampler_plan_t (include/mdt_hip.h)."""
    _fields_ = [("n_evals", C.c_int32), ("n_noise", C.c_int32), ("y0_noise", C.c_int32), ("y0_cn", C.c_float),
                ("y0_draws", C.c_int32), ("pad", C.c_int32 * 3), ("e", SamplerEval * SAMPLER_MAX_EVALS)]


class DpmAdaptiveParams(C.Structure):
    """mdt_dpm_adaptive_params (include/mdt_hip.h)."""
    _fields_ = [("order", C.c_int32)] + [(n, C.c_double) for n in ("rtol", "atol", "h_init", "pcoeff", "icoeff", "dcoeff",
                                                                   "accept_safety")]


class DpmAdaptiveInfo(C.Structure):
    """mdt_dpm_adaptive_info (include/mdt_hip.h)."""
    _fields_ = [(n, C.c_int32) for n in ("steps", "nfe", "n_accept", "n_reject")]


class DpmControl(C.Structure):
    """mdt_dpm_control (include/mdt_hip.h): _StepControl's state."""
    _fields_ = [("h", C.c_double), ("w", C.c_double * 3), ("safety", C.c_double), ("eps", C.c_double),
                ("hist", C.c_double * 3), ("started", C.c_int32), ("pad", C.c_int32)]


DPM_REJECT, DPM_ACCEPT, DPM_STOP = 0, 1, 2


class LoglikParams(C.Structure):
    """mdt_loglik_params (include/mdt_hip_train.h)."""
    _fields_ = [("size", C.c_int32), ("probes", C.c_int32), ("rtol", C.c_double), ("atol", C.c_double),
                ("max_steps", C.c_int32), ("pad", C.c_int32)]


class LoglikInfo(C.Structure):
    """mdt_loglik_info (include/mdt_hip_train.h)."""
    _fields_ = [(n, C.c_int32) for n in ("fevals", "steps", "n_accept", "n_reject")]


class LnTrainArgs(C.Structure):
    _fields_ = [("x", C.c_void_p), ("w", C.c_void_p), ("b", C.c_void_p), ("mod", C.c_void_p), ("mod_stride", C.c_int64),
                ("shift_off", C.c_int32), ("scale_off", C.c_int32), ("rows_per_sample", C.c_int32),
                ("out", C.c_void_p), ("stats", C.c_void_p), ("M", C.c_int32), ("D", C.c_int32)]


class LnBwdArgs(C.Structure):
    _fields_ = [("x", C.c_void_p), ("stats", C.c_void_p), ("w", C.c_void_p), ("b", C.c_void_p), ("mod", C.c_void_p),
                ("mod_stride", C.c_int64), ("shift_off", C.c_int32), ("scale_off", C.c_int32),
                ("dh", C.c_void_p), ("ld_dh", C.c_int64), ("dx", C.c_void_p), ("accumulate", C.c_int32),
                ("d_mod", C.c_void_p), ("d_mod_stride", C.c_int64), ("pw", C.c_void_p), ("pb", C.c_void_p),
                ("B", C.c_int32), ("rows_per_sample", C.c_int32), ("D", C.c_int32), ("row_chunks", C.c_int32),
                ("accumulate_dmod", C.c_int32)]


class AttnBwdArgs(C.Structure):
    _fields_ = [("q", C.c_void_p), ("ldq", C.c_int64), ("k", C.c_void_p), ("v", C.c_void_p), ("ldkv", C.c_int64),
                ("d_out", C.c_void_p), ("ld_do", C.c_int64), ("dq", C.c_void_p), ("ld_dq", C.c_int64),
                ("dk", C.c_void_p), ("dv", C.c_void_p), ("ld_dkv", C.c_int64), ("accumulate_kv", C.c_int32),
                ("B", C.c_int32), ("H", C.c_int32), ("hd", C.c_int32), ("Tq", C.c_int32), ("Tk", C.c_int32),
                ("causal", C.c_int32), ("p", C.c_float), ("site", C.c_uint32), ("seed", C.c_uint64),
                ("rope", C.c_int32), ("rope_cos", C.c_void_p), ("rope_sin", C.c_void_p)]


class AttnTrainArgs(C.Structure):
    _fields_ = [("q", C.c_void_p), ("ldq", C.c_int64), ("k", C.c_void_p), ("v", C.c_void_p), ("ldkv", C.c_int64),
                ("out", C.c_void_p), ("ldo", C.c_int64), ("B", C.c_int32), ("H", C.c_int32), ("hd", C.c_int32),
                ("Tq", C.c_int32), ("Tk", C.c_int32), ("causal", C.c_int32), ("p", C.c_float), ("site", C.c_uint32),
                ("seed", C.c_uint64), ("rope", C.c_int32), ("rope_cos", C.c_void_p), ("rope_sin", C.c_void_p)]


class MergeArgs(C.Structure):
    _fields_ = [("x", C.c_void_p), ("a", C.c_void_p), ("gate", C.c_void_p), ("gate_stride", C.c_int64),
                ("out", C.c_void_p), ("dgate", C.c_void_p), ("dgate_stride", C.c_int64), ("B", C.c_int32),
                ("rows_per_sample", C.c_int32), ("D", C.c_int32), ("p", C.c_float), ("site", C.c_uint32),
                ("seed", C.c_uint64)]


class Dropout(C.Structure):
    """mirrors mdt_dropout (include/mdt_hip_train.h)"""
    _fields_ = [("attn_p", C.c_float), ("resid_p", C.c_float), ("mlp_p", C.c_float), ("embed_p", C.c_float),
                ("seed", C.c_uint64)]


class LinearBwdArgs(C.Structure):
    _fields_ = [("X", C.c_void_p), ("ldx", C.c_int64), ("dY", C.c_void_p), ("ldy", C.c_int64), ("Wt", C.c_void_p),
                ("dW", C.c_void_p), ("dbias", C.c_void_p), ("dX", C.c_void_p), ("ldxo", C.c_int64),
                ("accumulate_dw", C.c_int32), ("accumulate_dx", C.c_int32), ("M", C.c_int32), ("N", C.c_int32),
                ("K", C.c_int32), ("scratch", C.c_void_p), ("dx_act_u", C.c_void_p), ("dx_act", C.c_int32)]


class OptTensor(C.Structure):
    """mirrors mdt_opt_tensor (include/mdt_hip_train.h)"""
    _fields_ = [("p", C.c_void_p), ("g", C.c_void_p), ("m", C.c_void_p), ("v", C.c_void_p), ("ema", C.c_void_p),
                ("numel", C.c_int64)]


class ResamplerConfig(C.Structure):
    """mirrors mdt_resampler_config (include/mdt_resampler.h)"""
    _fields_ = [(n, C.c_int32) for n in ("dim", "depth", "dim_head", "heads", "num_latents", "num_time_embeds",
                                          "ff_mult", "activation")]


class MapPoolConfig(C.Structure):
    """mirrors mdt_map_pool_config (include/mdt_map_pool.h)"""
    _fields_ = [(n, C.c_int32) for n in ("n_latents", "embed_dim", "output_dim", "n_heads", "mlp_hidden")]


class InfoNCEArgs(C.Structure):
    """mirrors mdt_infonce_args (include/mdt_map_pool.h)"""
    _fields_ = [("image_features", C.c_void_p), ("lang_features", C.c_void_p), ("logit_scale", C.c_void_p),
                ("batch", C.c_int32), ("dim", C.c_int32), ("mode", C.c_int32), ("loss", C.c_void_p),
                ("d_image", C.c_void_p), ("d_lang", C.c_void_p), ("d_logit_scale", C.c_void_p), ("scratch", C.c_void_p)]


INFONCE_MODE = {"symmetric": 0, "img_to_text": 1, "text_to_img": 2}
ARCH = {"mdtv": 0, "mdt": 1}
MODALITY = {"vis": 0, "lang": 1}
ACT = {"none": 0, "gelu": 1, "mish": 2, "silu": 3, "swiglu": 4}
HEAD = {"denoised": 0, "ddim": 1, "raw": 2}
RAW_OUTPUT, RAW_INPUT, SIGMA_SCALAR = 1, 2, 4

# every symbol include/*.h declares: (name, restype, argtypes)
_VP, _I32, _I64, _F = C.c_void_p, C.c_int32, C.c_int64, C.c_float
SYMBOLS = [
    ("mdt_last_error", C.c_char_p, []),
    ("mdt_version", C.c_char_p, []),
    ("mdt_set_allocator", _I32, [_VP, _VP, _VP]),
    ("mdt_allocator_detach", _I32, []),
    ("mdt_create", _I32, [C.POINTER(MDTConfig), C.POINTER(_VP)]),
    ("mdt_destroy", _I32, [_VP]),
    ("mdt_param_count", _I64, [_VP]),
    ("mdt_param_name", C.c_char_p, [_VP, _I64]),
    ("mdt_param_numel", _I64, [_VP, _I64]),
    ("mdt_load_param", _I32, [_VP, C.c_char_p, _VP, _I64, _VP]),
    ("mdt_load_params", _I32, [_VP, _I32, C.POINTER(C.c_char_p), C.POINTER(C.c_void_p), C.POINTER(_I64), _VP]),
    ("mdt_reserve", _I32, [_VP, _I64]),
    ("mdt_ws_generation", _I64, [_VP]),
    ("mdt_encode", _I32, [_VP, _VP, _VP, _VP, _I32, _I32, _VP, _I64, _VP, _VP]),
    ("mdt_denoise_cached", _I32, [_VP, _VP, _VP, _I64, _I32, _VP, _VP]),
    ("mdt_forward", _I32, [_VP, _VP, _VP, _VP, _I32, _VP, _VP, _I64, _VP, _VP, _VP]),
    ("mdt_sample_ddim", _I32, [_VP, _VP, _VP, _VP, _I32, _VP, C.POINTER(C.c_float), _I32, _I64, _VP, _VP, _VP]),
    ("mdt_sample_ddim_dev", _I32, [_VP, _VP, _VP, _VP, _I32, _VP, _VP, _I32, _I64, _VP, _VP, _VP]),
    ("mdt_sample", _I32, [_VP, _VP, _VP, _VP, _I32, _VP, _I32, C.POINTER(SamplerParams), C.POINTER(C.c_float), _I32, _VP, _I32,
                          _I64, _VP, _VP, _VP]),
    ("mdt_sample_dev", _I32, [_VP, _VP, _VP, _VP, _I32, _VP, _I32, C.POINTER(SamplerParams), _VP, _I32, _VP, _I32, _I64, _VP,
                              _VP, _VP]),
    ("mdt_sample_opt", _I32, [_VP, _VP, _VP, _VP, _I32, _VP, _I32, C.POINTER(SamplerParams), C.POINTER(C.c_float), _I32, _VP, _I32,
                              _I64, _VP, _VP, C.POINTER(SampleOpts), _VP]),
    ("mdt_sample_dev_opt", _I32, [_VP, _VP, _VP, _VP, _I32, _VP, _I32, C.POINTER(SamplerParams), _VP, _I32, _VP, _I32, _I64, _VP,
                                  _VP, C.POINTER(SampleOpts), _VP]),
    ("mdt_sample_ddim_opt", _I32, [_VP, _VP, _VP, _VP, _I32, _VP, C.POINTER(C.c_float), _I32, _I64, _VP, _VP, C.POINTER(SampleOpts),
                                   _VP]),
    ("mdt_sample_ddim_dev_opt", _I32, [_VP, _VP, _VP, _VP, _I32, _VP, _VP, _I32, _I64, _VP, _VP, C.POINTER(SampleOpts), _VP]),
    # the *_opt calls with `candidates` chunks per observation, after `batch`
    ("mdt_sample_multi", _I32, [_VP, _VP, _VP, _VP, _I32, _VP, _I32, C.POINTER(SamplerParams), C.POINTER(C.c_float), _I32, _VP, _I32,
                                _I64, _I32, _VP, _VP, C.POINTER(SampleOpts), _VP]),
    ("mdt_sample_dev_multi", _I32, [_VP, _VP, _VP, _VP, _I32, _VP, _I32, C.POINTER(SamplerParams), _VP, _I32, _VP, _I32, _I64, _I32,
                                    _VP, _VP, C.POINTER(SampleOpts), _VP]),
    ("mdt_sample_ddim_multi", _I32, [_VP, _VP, _VP, _VP, _I32, _VP, C.POINTER(C.c_float), _I32, _I64, _I32, _VP, _VP,
                                     C.POINTER(SampleOpts), _VP]),
    ("mdt_sample_ddim_dev_multi", _I32, [_VP, _VP, _VP, _VP, _I32, _VP, _VP, _I32, _I64, _I32, _VP, _VP, C.POINTER(SampleOpts), _VP]),
    # chunks scored by their denoising error: host levels and weights (or NULL), device noise rows (n_levels, draws, Ta, A)
    ("mdt_denoising_score", _I32, [_VP, _VP, _VP, _VP, _I32, _VP, C.POINTER(C.c_float), C.POINTER(C.c_float), _I32, _VP, _I32, _I64,
                                   _I32, _VP, _VP, _VP]),
    # the *_multi calls with `out` = the best chunk per observation and the score / selection spec in front of `stream`
    ("mdt_sample_select", _I32, [_VP, _VP, _VP, _VP, _I32, _VP, _I32, C.POINTER(SamplerParams), C.POINTER(C.c_float), _I32, _VP, _I32,
                                 _I64, _I32, _VP, _VP, C.POINTER(SampleOpts), C.POINTER(SelectSpec), _VP]),
    ("mdt_sample_dev_select", _I32, [_VP, _VP, _VP, _VP, _I32, _VP, _I32, C.POINTER(SamplerParams), _VP, _I32, _VP, _I32, _I64, _I32,
                                     _VP, _VP, C.POINTER(SampleOpts), C.POINTER(SelectSpec), _VP]),
    ("mdt_sample_ddim_select", _I32, [_VP, _VP, _VP, _VP, _I32, _VP, C.POINTER(C.c_float), _I32, _I64, _I32, _VP, _VP,
                                      C.POINTER(SampleOpts), C.POINTER(SelectSpec), _VP]),
    ("mdt_sample_ddim_dev_select", _I32, [_VP, _VP, _VP, _VP, _I32, _VP, _VP, _I32, _I64, _I32, _VP, _VP, C.POINTER(SampleOpts),
                                          C.POINTER(SelectSpec), _VP]),
    ("mdt_sampler_plan", _I32, [_I32, C.POINTER(SamplerParams), C.POINTER(C.c_float), _I32, C.POINTER(SamplerPlan)]),
    ("mdt_sample_dpm_adaptive", _I32, [_VP, _VP, _VP, _VP, _I32, _VP, C.c_float, C.c_float, C.POINTER(DpmAdaptiveParams), _I64,
                                       _VP, _VP, C.POINTER(DpmAdaptiveInfo), _VP]),
    ("mdt_sample_ddim_guided", _I32, [_VP, _VP, _VP, _VP, _I32, _VP, C.POINTER(C.c_float), _I32, _I64, _VP, _VP, _F, _VP]),
    ("mdt_sample_ddim_dev_guided", _I32, [_VP, _VP, _VP, _VP, _I32, _VP, _VP, _I32, _I64, _VP, _VP, _F, _VP]),
    ("mdt_sample_guided", _I32, [_VP, _VP, _VP, _VP, _I32, _VP, _I32, C.POINTER(SamplerParams), C.POINTER(C.c_float), _I32, _VP,
                                 _I32, _I64, _VP, _VP, _F, _VP]),
    ("mdt_sample_dev_guided", _I32, [_VP, _VP, _VP, _VP, _I32, _VP, _I32, C.POINTER(SamplerParams), _VP, _I32, _VP, _I32, _I64,
                                     _VP, _VP, _F, _VP]),
    ("mdt_brownian_noise", _I32, [_VP, _I32, C.c_double, C.c_double, C.c_double, _VP, _I32, _I64, _I64, _VP, _VP]),
    ("mdt_brownian_noise_host", _I32, [_VP, _I32, C.c_double, C.c_double, C.c_double, _VP, _I32, _I64, _I64, _VP]),
    ("mdt_sample_sde_tree", _I32, [_VP, _VP, _VP, _VP, _I32, _VP, C.POINTER(SamplerParams), C.POINTER(C.c_float), _I32,
                                   C.POINTER(BrownianSource), _I64, _VP, _VP, _VP]),
    ("mdt_sample_sde_tree_dev", _I32, [_VP, _VP, _VP, _VP, _I32, _VP, C.POINTER(SamplerParams), _VP, _I32, C.POINTER(BrownianSource),
                                       _I64, _VP, _VP, _VP]),
    ("mdt_sample_sde_tree_guided", _I32, [_VP, _VP, _VP, _VP, _I32, _VP, C.POINTER(SamplerParams), C.POINTER(C.c_float), _I32,
                                          C.POINTER(BrownianSource), _I64, _VP, _VP, _F, _VP]),
    ("mdt_sample_sde_tree_dev_guided", _I32, [_VP, _VP, _VP, _VP, _I32, _VP, C.POINTER(SamplerParams), _VP, _I32,
                                              C.POINTER(BrownianSource), _I64, _VP, _VP, _F, _VP]),
    ("mdt_sample_dpm_adaptive_guided", _I32, [_VP, _VP, _VP, _VP, _I32, _VP, C.c_float, C.c_float, C.POINTER(DpmAdaptiveParams),
                                              _I64, _VP, _VP, _F, C.POINTER(DpmAdaptiveInfo), _VP]),
    ("mdt_dpm_control_init", _I32, [C.POINTER(DpmControl)] + [C.c_double] * 6),
    ("mdt_dpm_control_update", _I32, [C.POINTER(DpmControl), C.c_float, C.POINTER(C.c_int32)]),
    ("mdt_dpm_adaptive_plan", _I32, [_I32, C.c_float, C.c_float, C.POINTER(SamplerPlan)]),
    ("mdt_loss_fwd", _I32, [_VP, _VP, _VP, _VP, _I32, _VP, _VP, _VP, _I64, _VP, _VP, _VP, _VP]),
    ("mdt_flops_per_chunk", C.c_double, [_VP, _I32]),
    ("mdt_fnv1_32", C.c_uint32, [C.c_char_p, C.c_uint64, C.c_uint32]),
    ("mdt_op_packed_numel", _I64, [_I64, _I64]),
    ("mdt_op_pack_weight", _I32, [_VP, _I64, _I64, _VP, _I64, _I64, _VP]),
    ("mdt_op_pack_weight_glu", _I32, [_VP, _I64, _I64, _VP, _VP]),
    ("mdt_op_gemm", _I32, [C.POINTER(GemmArgs), _VP]),
    ("mdt_op_mlp", _I32, [C.POINTER(GemmArgs), C.POINTER(GemmArgs), _VP, _I64, C.POINTER(_I32), _VP]),
    ("mdt_op_pack_weight_split", _I32, [_VP, _I64, _I64, _VP, _VP]),
    ("mdt_op_pack_weight_split_rows", _I32, [_VP, _I64, _I64, _VP, _I64, _VP]),
    ("mdt_op_mlp_split", _I32, [C.POINTER(GemmArgs), C.POINTER(GemmArgs), _VP, _VP, _VP, _I64, C.POINTER(_I32), _VP]),
    ("mdt_op_pair_image_bytes", _I64, [_I64, _I64]),
    ("mdt_op_pack_weight_pair", _I32, [_VP, _I64, _I64, _VP, _I64, _VP]),
    ("mdt_op_pair_from_packed", _I32, [_VP, _I64, _I64, _VP, _VP]),
    ("mdt_op_mlp_pair", _I32, [C.POINTER(GemmArgs), C.POINTER(GemmArgs), _VP, _VP, _VP, _I64, C.POINTER(_I32), _VP]),
    ("mdt_op_gemm_ln_pair", _I32, [C.POINTER(GemmArgs), _VP]),
    ("mdt_op_attention", _I32, [C.POINTER(AttnArgs), _VP]),
    ("mdt_op_attn_proj", _I32, [C.POINTER(GemmArgs), _VP, _I64, _I32, _I32, _I32, _VP]),
    ("mdt_op_xattn_fold", _I32, [C.POINTER(XFoldArgs), _VP]),
    ("mdt_op_xattn_apply", _I32, [C.POINTER(XApplyArgs), _VP]),
    ("mdt_op_attn_xattn", _I32, [C.POINTER(GemmArgs), _VP, _I64, C.POINTER(XApplyArgs), _I32, _I32, _VP]),
    ("mdt_op_attn_xattn_pair", _I32, [C.POINTER(GemmArgs), _VP, _I64, C.POINTER(XApplyArgs), _I32, _I32, _VP]),
    ("mdt_op_xattn_gemm", _I32, [C.POINTER(XApplyArgs), C.POINTER(GemmArgs), _VP]),
    ("mdt_op_layernorm", _I32, [_VP, _VP, _VP, _VP, _I64, _I32, _VP]),
    ("mdt_op_head", _I32, [C.POINTER(HeadArgs), _VP]),
    ("mdt_op_action_embed", _I32, [_VP, _VP, _I64, _F, _VP, _VP, _VP, _I64, _I32, _I32, _I32, _VP]),
    # include/mdt_hip_debug.h (process-global test and measurement hooks)
    ("mdt_op_set_mlp_split", None, [_I32]),
    ("mdt_op_set_gemm_geometry", None, [_I32]),
    ("mdt_op_set_mlp_fuse_min", None, [_I32]),
    ("mdt_op_set_side_jobs", None, [_I32]),
    ("mdt_op_side_jobs_paired", _I64, []),
    ("mdt_op_set_mlp_skew", None, [_I32]),
    ("mdt_op_set_attn_wide_min", None, [_I32]),
    ("mdt_op_attention_shared", _I32, [C.POINTER(AttnArgs), _I32, _VP]),
    ("mdt_op_attention_prefix", _I32, [C.POINTER(AttnArgs), _I32, _I32, _VP]),
    ("mdt_op_attn_fwd_train_prefix", _I32, [C.POINTER(AttnTrainArgs), _I32, _VP]),
    ("mdt_op_attn_bwd_prefix", _I32, [C.POINTER(AttnBwdArgs), _I32, _VP]),
    ("mdt_op_attn_chunk_lds", _I64, [_I32, _I32, _I32, _I32]),
    ("mdt_op_map_attn_fwd", _I32, [_I32, _VP, _VP, _VP, _VP, _I64, _I32, _I32, _I32, _I32, _VP]),
    ("mdt_op_map_attn_bwd", _I32, [_I32, _VP, _VP, _VP, _VP, _VP, _VP, _I64, _I32, _I32, _I32, _I32, _VP]),
    ("mdt_op_map_attn_lds", _I64, [_I32, _I32, _I32, _I32, _I32]),
    ("mdt_op_trace_mlp", None, [_I32]),
    ("mdt_op_trace_mlp_read", _I32, [_VP, _I32]),
    ("mdt_op_trace_mlp_read_empty", _I32, [_VP, _I32]),
    ("mdt_op_clock_stamp", _I32, [_VP, _VP]),
    ("mdt_op_set_ws_split", None, [_I32]),
    ("mdt_op_set_tn_split", None, [_I32]),
    ("mdt_op_narrow_dw", _I32, [_VP, _VP, _I64, _VP, _I32, _I32, _I32, _I32, _I32, _VP]),
    ("mdt_op_narrow_out", _I32, [_VP, _I64, _VP, _VP, _I32, _I32, _I32, _VP]),
    ("mdt_op_narrow_dx", _I32, [_VP, _VP, _VP, _I32, _I32, _I32, _VP]),
    ("mdt_op_steer_seed", _I32, [_VP, _VP, _VP, _VP, _F, _F, _I64, _VP, _VP, _VP, _VP]),
    ("mdt_op_steer_step", _I32, [_VP, _VP, _VP, _VP, _F, _F, _F, _F, _F, _VP, _VP, _I32, _F, _I64, _I64, _VP, _VP, _VP]),
    ("mdt_op_steer_first", _I32, [_VP, _VP, _F, _F, _I64, _I64, _VP, _VP, _VP, _VP, _VP]),
    ("mdt_op_steer_plan", _I32, [C.POINTER(SamplerEval), _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _I64, _I64,
                                 _F, _F, _I32, _I32, _VP]),
    ("mdt_op_score_prep", _I32, [_VP, _VP, _VP, _I32, _I32, _I32, _I64, _I32, _I32, _I32, _F, _VP, _VP, _VP, _VP, _VP, _VP, _VP]),
    ("mdt_op_score_repeat", _I32, [_VP, _VP, _VP, _I64, _I32, _I32, _I32, _I32, _VP, _VP, _VP, _VP]),
    ("mdt_op_score_reduce", _I32, [_VP, _VP, _VP, _VP, _VP, _I64, _I32, _I32, _I32, _I32, _F, _VP, _VP]),
    ("mdt_op_score_select", _I32, [_VP, _VP, _I64, _I32, _I32, _VP, _VP, _VP]),
    # include/mdt_hip_train.h
    ("mdt_train_prepare", _I32, [_VP]),
    ("mdt_grad_numel", _I64, [_VP]),
    ("mdt_grad_offset", _I64, [_VP, _I64]),
    ("mdt_train_loss_fwd", _I32, [_VP, _VP, _VP, _VP, _I32, _VP, _VP, _VP, _I64, C.POINTER(Dropout), _VP, _VP, _VP,
                                  C.POINTER(_I32), _VP]),
    ("mdt_train_loss_bwd", _I32, [_VP, _I32, _VP, _VP, _VP, _VP, _VP, _VP, _VP]),
    ("mdt_train_loss_bwd_stages", _I32, [_VP]),
    ("mdt_train_loss_bwd_stage", _I32, [_VP, _I32, _I32, _VP, _VP, _VP, _VP, _VP, _VP, _VP]),
    ("mdt_train_param_stage", _I32, [_VP, _I64]),
    ("mdt_train_encode_fwd", _I32, [_VP, _VP, _VP, _VP, _I32, _I32, _VP, _I64, C.POINTER(Dropout), _VP, C.POINTER(_I32),
                                    _VP]),
    ("mdt_train_encode_bwd", _I32, [_VP, _I32, _VP, _VP, _VP, _VP, _VP, _VP]),
    ("mdt_tape_release", _I32, [_VP, _I32]),
    ("mdt_denoise_vjp", _I32, [_VP, _VP, _VP, _VP, _I32, _VP, _VP, _VP, _I64, _VP, _VP, _VP]),
    ("mdt_log_likelihood", _I32, [_VP, _VP, _VP, _VP, _I32, _VP, _VP, _F, _F, _I64, _I32, C.POINTER(LoglikParams), _VP, _VP, _VP,
                                  C.POINTER(LoglikInfo), _VP]),
    ("mdt_sample_ddim_steer", _I32, [_VP, _VP, _VP, _VP, _I32, _VP, _VP, _I32, _I64, _I32, _VP, _VP, _F, _VP, _VP, _VP, _VP, _VP]),
    ("mdt_sample_steer", _I32, [_VP, _VP, _VP, _VP, _I32, _VP, _I32, C.POINTER(SamplerParams), C.POINTER(C.c_float), _I32, _VP, _I32,
                                _I64, _I32, _VP, _VP, _F, _VP, _VP, _VP, _VP, _VP, _VP]),
    ("mdt_dopri5_h0", C.c_double, [C.c_double, C.c_double]),
    ("mdt_dopri5_h1", C.c_double, [C.c_double, C.c_double, C.c_double]),
    ("mdt_dopri5_next", C.c_double, [C.c_double, C.c_double, C.POINTER(_I32)]),
    ("mdt_train_denoise_fwd", _I32, [_VP, _VP, _VP, _VP, _I64, C.POINTER(Dropout), _VP, C.POINTER(_I32), _VP]),
    ("mdt_train_denoise_bwd", _I32, [_VP, _I32, _VP, _VP, _VP, _VP, _VP, _VP]),
    ("mdt_op_pack_weight_t", _I32, [_VP, _I64, _I64, _I64, _VP, _I64, _I64, _VP]),
    ("mdt_op_pack_many", _I32, [_I32, C.POINTER(C.c_void_p), C.POINTER(_I32), C.POINTER(_I32), C.POINTER(C.c_void_p),
                                C.POINTER(C.c_void_p), _VP]),
    ("mdt_op_ln_fwd_train", _I32, [C.POINTER(LnTrainArgs), _VP]),
    ("mdt_op_ln_bwd", _I32, [C.POINTER(LnBwdArgs), _VP]),
    ("mdt_op_attn_bwd", _I32, [C.POINTER(AttnBwdArgs), _VP]),
    ("mdt_op_act_fwd", _I32, [_VP, _VP, _I64, _I32, _VP]),
    ("mdt_op_act_bwd", _I32, [_VP, _VP, _VP, _I64, _I32, _VP]),
    ("mdt_op_attn_fwd_train", _I32, [C.POINTER(AttnTrainArgs), _VP]),
    ("mdt_op_merge_fwd", _I32, [C.POINTER(MergeArgs), _VP]),
    ("mdt_op_merge_bwd", _I32, [C.POINTER(MergeArgs), _VP]),
    ("mdt_op_merge_ln_fwd", _I32, [C.POINTER(MergeArgs), C.POINTER(LnTrainArgs), _VP]),
    ("mdt_op_ln_bwd_merge", _I32, [C.POINTER(LnBwdArgs), C.POINTER(MergeArgs), _VP]),
    ("mdt_op_colsum", _I32, [_VP, _I64, _I64, _I64, _VP, _I32, _VP]),
    ("mdt_op_linear_bwd", _I32, [C.POINTER(LinearBwdArgs), _VP]),
    ("mdt_op_linear_bwd_scratch", _I64, [_I64, _I64, _I64]),
    ("mdt_op_linear_bwd_scratch_exact", _I64, [_I64, _I64, _I64]),
    ("mdt_op_multi_adamw", _I32, [C.POINTER(OptTensor), _I32, _F, _F, _F, _F, _F, _I64, _VP]),
    ("mdt_op_multi_ema", _I32, [C.POINTER(OptTensor), _I32, _F, _VP]),
    ("mdt_op_multi_sumsq_scratch", _I64, [C.POINTER(OptTensor), _I32]),
    ("mdt_op_multi_sumsq", _I32, [C.POINTER(OptTensor), _I32, _I32, _VP, _VP, _I64, _VP]),
    ("mdt_op_multi_adamw_dev", _I32, [C.POINTER(OptTensor), _I32, _F, _F, _F, _F, _F, _VP, _VP, _VP, _VP, _F, _VP, _VP]),
    # include/mdt_resampler.h
    ("mdt_resampler_create", _I32, [C.POINTER(ResamplerConfig), C.POINTER(_VP)]),
    ("mdt_resampler_destroy", _I32, [_VP]),
    ("mdt_resampler_param_count", _I64, [_VP]),
    ("mdt_resampler_param_name", C.c_char_p, [_VP, _I64]),
    ("mdt_resampler_param_numel", _I64, [_VP, _I64]),
    ("mdt_resampler_load_param", _I32, [_VP, C.c_char_p, _VP, _I64, _VP]),
    ("mdt_resampler_forward", _I32, [_VP, _VP, _VP, _I64, _I32, _I32, _VP, _VP]),
    ("mdt_resampler_train_prepare", _I32, [_VP]),
    ("mdt_resampler_grad_numel", _I64, [_VP]),
    ("mdt_resampler_grad_offset", _I64, [_VP, _I64]),
    ("mdt_resampler_forward_train", _I32, [_VP, _VP, _VP, _I64, _I32, _I32, _VP, C.POINTER(_I32), _VP]),
    ("mdt_resampler_backward", _I32, [_VP, _I32, _VP, _VP, _VP, _VP]),
    ("mdt_resampler_tape_release", _I32, [_VP, _I32]),
    ("mdt_resampler_flops", C.c_double, [_VP, _I32, _I32]),
    # include/mdt_map_pool.h
    ("mdt_map_pool_create", _I32, [C.POINTER(MapPoolConfig), C.POINTER(_VP)]),
    ("mdt_map_pool_destroy", _I32, [_VP]),
    ("mdt_map_pool_param_count", _I64, [_VP]),
    ("mdt_map_pool_param_name", C.c_char_p, [_VP, _I64]),
    ("mdt_map_pool_param_numel", _I64, [_VP, _I64]),
    ("mdt_map_pool_load_param", _I32, [_VP, C.c_char_p, _VP, _I64, _VP]),
    ("mdt_map_pool_forward", _I32, [_VP, _VP, _I64, _I32, _VP, _VP]),
    ("mdt_map_pool_train_prepare", _I32, [_VP]),
    ("mdt_map_pool_grad_numel", _I64, [_VP]),
    ("mdt_map_pool_grad_offset", _I64, [_VP, _I64]),
    ("mdt_map_pool_forward_train", _I32, [_VP, _VP, _I64, _I32, _VP, C.POINTER(_I32), _VP]),
    ("mdt_map_pool_backward", _I32, [_VP, _I32, _VP, _VP, _VP, _VP]),
    ("mdt_map_pool_tape_release", _I32, [_VP, _I32]),
    # include/mdt_mae.h
    ("mdt_op_rms_fwd", _I32, [_VP, _VP, _VP, _I64, _I32, _F, _VP]),
    ("mdt_op_rms_bwd_scratch", _I64, [_I64, _I32]),
    ("mdt_op_rms_bwd", _I32, [_VP, _VP, _VP, _VP, _I32, _VP, _I32, _I64, _I32, _F, _VP, _VP]),
    ("mdt_op_rms_bwd_res", _I32, [_VP, _VP, _VP, _VP, _VP, _VP, _I32, _I64, _I32, _F, _VP, _VP]),
    ("mdt_op_scale_residual_fwd", _I32, [_VP, _VP, _VP, _VP, _I64, _I32, _VP]),
    ("mdt_op_scale_residual_bwd_scratch", _I64, [_I64, _I32]),
    ("mdt_op_scale_residual_bwd", _I32, [_VP, _VP, _VP, _VP, _VP, _I64, _I32, _VP, _VP]),
    ("mdt_op_scale_residual_rms_fwd", _I32, [_VP, _VP, _VP, _VP, _VP, _VP, _I64, _I32, _F, _VP]),
    ("mdt_op_scale_residual_rms_bwd_scratch", _I64, [_I64, _I32]),
    ("mdt_op_scale_residual_rms_bwd", _I32, [_VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _I64, _I32, _F, _VP, _VP]),
    ("mdt_op_swiglu_fwd", _I32, [_VP, _VP, _I64, _I32, _VP]),
    ("mdt_op_swiglu_bwd", _I32, [_VP, _VP, _VP, _I64, _I32, _VP]),
    ("mdt_op_attn_mid_fwd", _I32, [_VP, _I64, _VP, _I64, _I64, _I32, _I32, _I32, _F, _VP]),
    ("mdt_op_attn_mid_bwd", _I32, [_VP, _I64, _VP, _I64, _VP, _I64, _VP, _I64, _I64, _I32, _I32, _I32, _F, _VP]),
    ("mdt_op_attn_long_fwd", _I32, [_VP, _I64, _VP, _I64, _VP, _I64, _I32, _I32, _I32, _F, _VP]),
    ("mdt_op_attn_long_bwd_scratch", _I64, [_I64, _I32, _I32]),
    ("mdt_op_attn_long_bwd", _I32, [_VP, _I64, _VP, _I64, _VP, _VP, _I64, _VP, _I64, _I64, _I32, _I32, _I32, _F, _VP, _VP]),
    ("mdt_op_patch_mse_fwd", _I32, [_VP, _VP, _VP, _VP, _VP, _VP, _I64, _I32, _I32, _I32, _I32, _VP]),
    ("mdt_op_patch_mse_bwd", _I32, [_VP, _VP, _VP, _VP, _VP, _VP, _I64, _I32, _I32, _I32, _I32, _VP]),
    ("mdt_op_infonce_scratch", _I64, [_I64, _I64]),
    ("mdt_op_infonce", _I32, [C.POINTER(InfoNCEArgs), _VP]),
]

_lock = threading.Lock()
_lib = None


def library_path() -> str:
    return _build.LIB


def load() -> C.CDLL:
    """Load (building with hipcc if the in-tree .so is missing or stale).  Raises if neither is possible."""
    global _lib
    with _lock:
        if _lib is not None:
            return _lib
        path = _build.LIB
        override = os.environ.get("MDT_HIP_LIB")  # tuning A/B runs: an experimental build of the same sources
        if override:
            path = override
        elif not os.path.exists(path):
            # Only a MISSING library is built here (atomically); a stale one is rebuilt by __graft_entry__.build(),
            # never implicitly at import time -- N ranks importing at once must not race on the same file.
            try:
                path = _build.build_library()
            except Exception as e:  # no hipcc and no prebuilt library: there is nothing to run
                raise RuntimeError(
                    "libmdt_hip.so is missing and could not be built; the MDT hot path has no CPU/eager "
                    f"fallback ({e})") from e
        # torch FIRST: its wheels bundle their own libamdhip64 / HSA runtime.  If this library is loaded before torch (as
        # __graft_entry__.build() followed by smoke() in ONE process did), the process ends up with two HIP runtimes and the one
        # this library is bound to reports "no ROCm-capable device" at its first hipMalloc.
        try:
            import torch  # noqa: F401
        except ImportError:  # a torch-free client of the C ABI (tests/c_client) has only one runtime anyway
            pass
        lib = C.CDLL(path)
        for name, res, args in SYMBOLS:
            fn = getattr(lib, name)  # AttributeError if the library does not export a declared symbol
            fn.restype = res
            fn.argtypes = args
        _lib = lib
        return lib


def check(status: int) -> None:
    if status != 0:
        raise MDTHipError(status, load().mdt_last_error().decode("utf-8", "replace"))


def sampler_params(**kw) -> SamplerParams:
    """mdt_sampler_params with Python's defaults for every field not given (gc_sampling.py signatures)."""
    p = dict(eta=1., s_churn=0., s_tmin=0., s_tmax=float("inf"), s_noise=1., r=0.5, order=4)
    unknown = set(kw) - set(p)
    if unknown:
        raise TypeError(f"unknown sampler parameter(s) {sorted(unknown)}")
    p.update(kw)
    return SamplerParams(*(float(p[k]) for k in ("eta", "s_churn", "s_tmin", "s_tmax", "s_noise", "r")), int(p["order"]))


def sampler_plan(kind, sigmas, n_steps=None, **params) -> SamplerPlan:
    """mdt_sampler_plan: the plan mdt_sample builds for this sampler (a name of SAMPLER_KIND or an mdt_sampler_kind),
    parameter set and host schedule (n_steps + 1 levels; dpm_fast: {sigma_max, sigma_min} and ``n_steps`` evaluations),
    computed on the host."""
    kind = SAMPLER_KIND[kind] if isinstance(kind, str) else int(kind)
    sig = [float(v) for v in sigmas]
    arr = (C.c_float * len(sig))(*sig)
    plan = SamplerPlan()
    n = len(sig) - 1 if n_steps is None else int(n_steps)
    check(load().mdt_sampler_plan(kind, C.byref(sampler_params(**params)), arr, n, C.byref(plan)))
    return plan


def brownian_noise_host(seeds, lo, hi, tol, pairs, batch, per_row):
    """mdt_brownian_noise_host: a (len(pairs), batch, per_row) float32 numpy array of the tree's noise values for the (from, to)
    ``pairs``; ``seeds`` one int (the whole tensor) or ``batch`` ints (one tree per sample)."""
    import numpy as np
    sd = np.ascontiguousarray(np.asarray(seeds, dtype=np.uint64).reshape(-1))
    pr = np.ascontiguousarray(np.asarray(pairs, dtype=np.float64).reshape(-1, 2))
    out = np.empty((pr.shape[0], int(batch), int(per_row)), dtype=np.float32)
    check(load().mdt_brownian_noise_host(sd.ctypes.data, len(sd), float(lo), float(hi), float(tol), pr.ctypes.data, pr.shape[0],
                                         int(batch), int(per_row), out.ctypes.data))
    return out


def dpm_adaptive_params(order=3, rtol=0.05, atol=0.0078, h_init=0.05, pcoeff=0., icoeff=1., dcoeff=0.,
                        accept_safety=0.81) -> DpmAdaptiveParams:
    """mdt_dpm_adaptive_params with sample_dpm_adaptive's defaults."""
    return DpmAdaptiveParams(int(order), *(float(v) for v in (rtol, atol, h_init, pcoeff, icoeff, dcoeff, accept_safety)))


def dpm_adaptive_plan(order, s, t) -> SamplerPlan:
    """mdt_dpm_adaptive_plan: the evaluations of one attempted adaptive step from s to t (t = -ln sigma), on the host."""
    plan = SamplerPlan()
    check(load().mdt_dpm_adaptive_plan(int(order), float(s), float(t), C.byref(plan)))
    return plan


def loglik_params(probes=1, rtol=1e-4, atol=1e-4, max_steps=10000) -> LoglikParams:
    """mdt_loglik_params with log_likelihood's defaults."""
    return LoglikParams(C.sizeof(LoglikParams), int(probes), float(rtol), float(atol), int(max_steps), 0)


def dopri5_start(d0, d1):
    """mdt_dopri5_h0: the first guess of _dopri5's starting step."""
    return load().mdt_dopri5_h0(float(d0), float(d1))


def dopri5_start_refine(h0, d1, d2):
    """mdt_dopri5_h1: the starting step from the guess h0 and the probe evaluation's norm d2 (not yet divided by h0)."""
    return load().mdt_dopri5_h1(float(h0), float(d1), float(d2))


def dopri5_next(h, ratio):
    """mdt_dopri5_next: (the next step size, whether the attempt at ``h`` with scaled error ``ratio`` is accepted)."""
    acc = C.c_int32()
    return load().mdt_dopri5_next(float(h), float(ratio), C.byref(acc)), bool(acc.value)


class DpmController:
    """mdt_dpm_control_init / _update: the step-size controller mdt_sample_dpm_adaptive runs, on the host."""

    def __init__(self, h, pcoeff, icoeff, dcoeff, order, accept_safety):
        self.c = DpmControl()
        check(load().mdt_dpm_control_init(C.byref(self.c), h, pcoeff, icoeff, dcoeff, order, accept_safety))

    @property
    def h(self) -> float:
        return self.c.h

    def update(self, error) -> int:
        """DPM_ACCEPT, DPM_REJECT or DPM_STOP for the scaled error of the step just tried (taken as fp32)."""
        d = C.c_int32()
        check(load().mdt_dpm_control_update(C.byref(self.c), float(error), C.byref(d)))
        return d.value


def call(fn, *args) -> None:
    """``check(fn(*args))`` with one retry after ``torch.cuda.empty_cache()`` when a hipMalloc inside the library failed:
    weights, workspace and tapes are raw HIP allocations, so memory that torch's caching allocator holds but does not use
    looks exhausted to them although it is free."""
    status = fn(*args)
    if status != 0:
        msg = load().mdt_last_error().decode("utf-8", "replace")
        if "hipMalloc" in msg or "out of memory" in msg.lower():
            import torch
            torch.cuda.empty_cache()
            status = fn(*args)
            if status == 0:
                return
            msg = load().mdt_last_error().decode("utf-8", "replace")
        raise MDTHipError(status, msg)
