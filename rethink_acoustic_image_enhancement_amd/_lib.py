"""ctypes binding of libkdlae.so (the C ABI declared in include/kdlae.h).

The product path has no CPU fallback: if the shared library is missing or a call fails, a
RuntimeError is raised.  Build it with ``make -C rethink_acoustic_image_enhancement_amd/csrc``
(or ``python -c 'import __graft_entry__ as g; g.build()'``).
"""
from __future__ import annotations

import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# KDLAE_LIB overrides the library (kernel A/B builds under tools/); default: the in-tree build
LIB_PATH = os.environ.get("KDLAE_LIB") or os.path.join(_HERE, "libkdlae.so")

c_int, c_int64, c_double, c_void_p, c_char_p = (ctypes.c_int, ctypes.c_int64, ctypes.c_double,
                                                ctypes.c_void_p, ctypes.c_char_p)

ERRORS = {0: "OK", 1: "EINVAL_SHAPE", 2: "EINVAL_CONFIG", 3: "EHIP", 4: "EPARAM", 5: "ENOTIMPL",
          6: "ESTATE"}

# Every entry point include/kdlae.h declares (checked by tests/test_abi.py).
EXPORTS = (
    "kdlae_last_error", "kdlae_abi_version",
    "kdlae_t_create", "kdlae_t_create_restormer", "kdlae_t_destroy", "kdlae_t_num_params", "kdlae_t_param_info",
    "kdlae_t_set_param", "kdlae_t_commit_params", "kdlae_t_params_numel", "kdlae_t_prepare", "kdlae_t_pack_device",
    "kdlae_t_workspace_bytes", "kdlae_t_forward",
    "kdlae_t_rates_workspace_bytes", "kdlae_t_forward_rates", "kdlae_t_sr_workspace_bytes", "kdlae_t_forward_sr",
    "kdlae_rate_select",
    "kdlae_tile_plan", "kdlae_tile_gather", "kdlae_tile_blend", "kdlae_tile_blend_rates",
    "kdlae_tile_blend_w", "kdlae_tile_blend_rates_w",
    "kdlae_clip_plan", "kdlae_clip_gather", "kdlae_clip_blend", "kdlae_clip_blend_u8",
    "kdlae_stream_state_bytes", "kdlae_stream_reset", "kdlae_stream_push_u8", "kdlae_stream_push_f32",
    "kdlae_stream_advance",
    "kdlae_distill_expand_u8", "kdlae_distill_expand_f32", "kdlae_distill_collapse",
    "kdlae_t_probe_arm", "kdlae_t_probe_read",
    "kdlae_t_debug_tap_count", "kdlae_t_debug_tap_info", "kdlae_t_debug_taps", "kdlae_t_debug_sr_fold",
    "kdlae_s_create", "kdlae_s_destroy", "kdlae_s_num_params", "kdlae_s_param_info",
    "kdlae_s_set_param", "kdlae_s_commit_params", "kdlae_s_params_numel", "kdlae_s_prepare", "kdlae_s_pack_device",
    "kdlae_s_workspace_bytes", "kdlae_s_forward",
    "asdqe_create", "asdqe_destroy", "asdqe_num_params", "asdqe_param_info", "asdqe_set_param",
    "asdqe_commit_params", "asdqe_params_numel", "asdqe_prepare", "asdqe_pack_device", "asdqe_workspace_bytes", "asdqe_forward",
    "kdlae_padded_size", "kdlae_preprocess_u8", "kdlae_frames_preprocess_u8", "kdlae_postprocess_u8",
    "kdlae_tt_create", "kdlae_tt_create_restormer", "kdlae_tt_destroy", "kdlae_tt_num_params", "kdlae_tt_param_info", "kdlae_tt_num_floats",
    "kdlae_tt_workspace_bytes", "kdlae_tt_forward", "kdlae_tt_backward", "kdlae_tt_backward_marked",
    "kdlae_tt_mark_count", "kdlae_tt_mark_lo", "kdlae_tt_mark_wait", "kdlae_tt_mark_sync",
    "kdlae_tt_set_trainable", "kdlae_tt_is_trainable", "kdlae_tt_debug_backward_launches",
    "kdlae_train_l1sr_scratch_floats", "kdlae_train_l1sr", "kdlae_train_adamw_scratch_floats",
    "kdlae_train_clip_adamw", "kdlae_train_mixup", "kdlae_train_ema",
    "kdlae_st_create", "kdlae_st_destroy", "kdlae_st_num_params", "kdlae_st_param_info", "kdlae_st_num_floats",
    "kdlae_st_workspace_bytes", "kdlae_st_forward", "kdlae_st_backward",
    "kdlae_train_l1frames_scratch_floats", "kdlae_train_l1frames",
    "kdlae_train_l1sonar_scratch_floats", "kdlae_train_l1sonar",
    "kdlae_debug_tgemm",
    "kdlae_debug_gemm",
    "kdlae_debug_gemm_variant",
    "kdlae_debug_gram",
    "kdlae_debug_ln",
    "kdlae_debug_small_in",
    "asdqe_train_create", "asdqe_train_destroy", "asdqe_train_num_params", "asdqe_train_param_info",
    "asdqe_train_num_floats", "asdqe_train_num_stat_floats", "asdqe_train_workspace_bytes", "asdqe_train_forward",
    "asdqe_train_backward", "kdlae_train_mse",
    "kdlae_debug_bn",
    "kdlae_metric_scratch_bytes", "kdlae_metric_psnr",
    "kdlae_metric_ssim_scratch_bytes", "kdlae_metric_ssim",
    "kdlae_metric_niqe_scratch_bytes", "kdlae_metric_niqe",
    "kdlae_train_prepare", "kdlae_train_mask_frames",
    "kdlae_data_sample", "kdlae_data_count", "kdlae_data_finish",
    "kdlae_debug_train", "kdlae_debug_train_blocks", "kdlae_debug_train_s",
    "kdlae_debug_infer",
    "kdlae_debug_head_train",
)

# The entry points include/kdlae_ensemble.h declares (checked by tests/test_ensemble.py): a header and a tuple of
# their own, include/kdlae.h and EXPORTS stay as they are.
ENSEMBLE_EXPORTS = ("kdlae_ens_gather", "kdlae_ens_merge")


class TConfig(ctypes.Structure):
    """kdlae_t_config (include/kdlae.h) = KDLAE_teacher ctor kwargs (KDLAE_model.py:205-218)."""

    _fields_ = [
        ("inp_channels", c_int), ("out_channels", c_int), ("dim", c_int),
        ("num_blocks", c_int * 4), ("num_refinement_blocks", c_int), ("heads", c_int * 4),
        ("ffn_expansion_factor", c_double), ("bias", c_int), ("layernorm_biasfree", c_int),
        ("dual_pixel_task", c_int), ("static_train", c_int), ("params_cat", c_int),
    ]


class SConfig(ctypes.Structure):
    """kdlae_s_config (include/kdlae.h) = KDLAE_student ctor kwargs (KDLAE_model.py:341-342)."""

    _fields_ = [
        ("inp_channels", c_int), ("out_channels", c_int), ("residual", c_int), ("num_hidden", c_int),
        ("hidden_channels", c_int * 8), ("kernel_size", c_int),
    ]


class AConfig(ctypes.Structure):
    """asdqe_config (include/kdlae.h) = DenoiseRatePredictor ctor kwargs (ASDQE_model.py:127)."""

    _fields_ = [("in_channels", c_int), ("dim", c_int)]


class TrainRedDesc(ctypes.Structure):
    """kdlae_debug_train_red (include/kdlae.h)."""

    _fields_ = [("part", c_void_p), ("out", c_void_p), ("nblk", c_int), ("ncols", c_int), ("pstride", c_int),
                ("scale", ctypes.c_float)]


class TrainDesc(ctypes.Structure):
    """kdlae_debug_train_desc (include/kdlae.h): the C field `in` is `inp` here."""

    _fields_ = [("op", c_int), ("inp", c_void_p * 4), ("ldi", c_int * 4), ("w", c_void_p), ("bias", c_void_p),
                ("out", c_void_p * 4), ("ldo", c_int * 4), ("part", c_void_p), ("part_floats", c_int64),
                ("C", c_int), ("C2", c_int), ("heads", c_int), ("Bn", c_int), ("H", c_int), ("W", c_int),
                ("P", c_int64), ("flag", c_int), ("accumulate", c_int), ("zero_to", c_int),
                ("nblk", c_int), ("nseg", c_int), ("pstride", c_int), ("scale", ctypes.c_float),
                ("nred", c_int), ("red", TrainRedDesc * 8)]


class TrainSDesc(ctypes.Structure):
    """kdlae_debug_train_s_desc (include/kdlae.h): the C field `in` is `inp` here."""

    _fields_ = [("op", c_int), ("inp", c_void_p * 3), ("ldi", c_int * 3), ("bias", c_void_p),
                ("out", c_void_p), ("ldo", c_int),
                ("C", c_int), ("O", c_int), ("B", c_int), ("F", c_int), ("H", c_int), ("W", c_int),
                ("accumulate", c_int), ("dir", c_int)]


class InferDesc(ctypes.Structure):
    """kdlae_debug_infer_desc (include/kdlae.h): the C field `in` is `inp` here."""

    _fields_ = [("op", c_int), ("inp", c_void_p * 3), ("ldi", c_int * 3), ("w", c_void_p * 4),
                ("bias", c_void_p * 4), ("R", c_void_p), ("ldr", c_int),
                ("out", c_void_p * 2), ("ldo", c_int * 2), ("scratch", c_void_p), ("scratch_floats", c_int64),
                ("zeros", c_void_p),
                ("C", c_int), ("C2", c_int), ("heads", c_int), ("Bn", c_int), ("F", c_int), ("H", c_int), ("W", c_int),
                ("hidS", c_int), ("ln", c_int), ("nseg", c_int), ("seg_rows", c_int),
                ("ntiles", c_int), ("cin_pad", c_int), ("kt", c_int), ("ks", c_int), ("relu", c_int),
                ("out_mode", c_int), ("nout", c_int), ("use_wp3", c_int),
                ("out_nchw", c_int), ("wt", c_int), ("slots", c_int),
                ("M", c_int), ("N1", c_int), ("N2", c_int)]


class SmallInDesc(ctypes.Structure):
    """kdlae_debug_small_in_desc (include/kdlae.h): the C field `in` is `inp` here."""

    _fields_ = [("inp", c_void_p), ("sb", c_int64), ("sc", c_int64), ("sy", c_int64), ("sx", c_int64),
                ("st", c_int64), ("in_sub", c_void_p),
                ("Cin", c_int), ("Cout", c_int), ("dil", c_int), ("kt", c_int), ("F", c_int),
                ("w", c_void_p), ("bias", c_void_p), ("out", c_void_p), ("ldo", c_int),
                ("Bn", c_int), ("H", c_int), ("W", c_int), ("vh", c_int), ("vw", c_int), ("relu", c_int),
                ("wt", c_int)]


class BnDesc(ctypes.Structure):
    """kdlae_debug_bn_desc (include/kdlae.h)."""

    _fields_ = [("op", c_int), ("x", c_void_p), ("ldx", c_int), ("y", c_void_p), ("ldy", c_int),
                ("dy", c_void_p), ("ldd", c_int), ("out", c_void_p), ("ldo", c_int),
                ("mean", c_void_p), ("rstd", c_void_p), ("running_mean", c_void_p), ("running_var", c_void_p),
                ("momentum", ctypes.c_float), ("gamma", c_void_p), ("beta", c_void_p), ("dgamma", c_void_p),
                ("dbeta", c_void_p), ("C", c_int), ("P", c_int64), ("N", c_int), ("h", c_int), ("w", c_int),
                ("part", c_void_p), ("part_floats", c_int64),
                ("Hp", c_int), ("Wp", c_int), ("accumulate", c_int), ("scale", ctypes.c_float)]


class HeadTrainDesc(ctypes.Structure):
    """kdlae_debug_head_train_desc (include/kdlae.h)."""

    _fields_ = [("dir", c_int), ("partial", c_void_p), ("slots", c_int), ("C", c_int), ("inv_hw", ctypes.c_float),
                ("wo", c_void_p), ("bo", c_void_p), ("M", c_int),
                ("w1", c_void_p), ("b1", c_void_p), ("N1", c_int),
                ("w2", c_void_p), ("b2", c_void_p), ("N2", c_int),
                ("w3", c_void_p), ("b3", c_void_p), ("mask1", c_void_p), ("mask2", c_void_p),
                ("score", c_void_p), ("B", c_int), ("save", c_void_p), ("save_floats", c_int64),
                ("dscore", c_void_p),
                ("gwo", c_void_p), ("gbo", c_void_p), ("gw1", c_void_p), ("gb1", c_void_p),
                ("gw2", c_void_p), ("gb2", c_void_p), ("gw3", c_void_p), ("gb3", c_void_p)]


class PrepSeg(ctypes.Structure):
    """kdlae_prep_seg (include/kdlae.h): one tensor of a kdlae_train_prepare call."""

    _fields_ = [("src", c_void_p), ("dst", c_void_p),
                ("B_src", c_int), ("C", c_int), ("Hs", c_int), ("Ws", c_int), ("h", c_int), ("w", c_int),
                ("y0", c_int), ("x0", c_int), ("prob", ctypes.c_float), ("keep", c_void_p)]


class DataItem(ctypes.Structure):
    """kdlae_data_item (include/kdlae.h): one source image and one destination slot of a kdlae_data_sample call."""

    _fields_ = [("src", c_void_p), ("dst", c_void_p), ("z", c_void_p), ("counts", c_void_p), ("mean", c_void_p),
                ("std", c_void_p), ("sy", c_int64), ("sx", c_int64), ("sc", c_int64), ("count_n", c_int64),
                ("count_thr", c_double), ("loc", c_double), ("scale", c_double), ("div", c_double),
                ("src_u8", c_int), ("Hs", c_int), ("Ws", c_int), ("C", c_int),
                ("Hc", c_int), ("Wc", c_int), ("Hp", c_int), ("Wp", c_int), ("pad_mode", c_int),
                ("top", c_int), ("left", c_int), ("h", c_int), ("w", c_int),
                ("dihedral", c_int), ("reverse_c", c_int), ("noise", c_int), ("reserved", c_int)]


_lib = None


def lib() -> ctypes.CDLL:
    """Load libkdlae.so once; raise loudly if it is missing (no silent fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} is missing: the KDLAE HIP path has no CPU fallback. Build it with "
            "`make -C rethink_acoustic_image_enhancement_amd/csrc` (hipcc, gfx950).")
    L = ctypes.CDLL(LIB_PATH)
    L.kdlae_last_error.restype = c_char_p
    L.kdlae_abi_version.restype = c_int
    L.kdlae_t_create.argtypes = [ctypes.POINTER(TConfig), c_int, ctypes.POINTER(c_void_p)]
    L.kdlae_t_create_restormer.argtypes = L.kdlae_t_create.argtypes
    L.kdlae_t_destroy.argtypes = [c_void_p]
    L.kdlae_t_num_params.argtypes = [c_void_p]
    L.kdlae_t_param_info.argtypes = [c_void_p, c_int, ctypes.POINTER(c_char_p), ctypes.POINTER(c_int64)]
    L.kdlae_t_set_param.argtypes = [c_void_p, c_char_p, c_void_p, c_int64]
    L.kdlae_t_commit_params.argtypes = [c_void_p, c_void_p]
    for pre in ("kdlae_t", "kdlae_s", "asdqe"):
        getattr(L, pre + "_params_numel").argtypes = [c_void_p]
        getattr(L, pre + "_params_numel").restype = c_int64
        getattr(L, pre + "_pack_device").argtypes = [c_void_p, c_void_p, c_int64, c_void_p]
        getattr(L, pre + "_prepare").argtypes = [c_void_p]
    L.kdlae_t_workspace_bytes.argtypes = [c_void_p, c_int, c_int, c_int]
    L.kdlae_t_workspace_bytes.restype = c_int64
    L.kdlae_t_forward.argtypes = [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p,
                                  c_void_p, c_int64, c_void_p]
    L.kdlae_t_rates_workspace_bytes.argtypes = [c_void_p, c_int, c_int, c_int, c_int, c_int]
    L.kdlae_t_rates_workspace_bytes.restype = c_int64
    L.kdlae_t_forward_rates.argtypes = [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p,
                                        c_void_p, c_void_p, c_int64, c_void_p]
    L.kdlae_t_sr_workspace_bytes.argtypes = [c_void_p, c_int, c_int, c_int]
    L.kdlae_t_sr_workspace_bytes.restype = c_int64
    L.kdlae_t_forward_sr.argtypes = [c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_int64, c_void_p]
    L.kdlae_rate_select.argtypes = [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_int64, c_void_p, c_void_p,
                                    c_void_p]
    L.kdlae_tile_plan.argtypes = [c_int, c_int, c_int, c_int] + [ctypes.POINTER(c_int)] * 6
    L.kdlae_tile_gather.argtypes = [c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p,
                                    c_void_p]
    L.kdlae_tile_blend.argtypes = [c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p]
    L.kdlae_tile_blend_rates.argtypes = [c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int,
                                         c_void_p, c_void_p]
    L.kdlae_tile_blend_w.argtypes = [c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p,
                                     c_void_p, c_void_p]
    L.kdlae_tile_blend_rates_w.argtypes = [c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int,
                                           c_void_p, c_void_p, c_void_p, c_void_p]
    L.kdlae_clip_plan.argtypes = [c_int, c_int, c_int] + [ctypes.POINTER(c_int)] * 3
    L.kdlae_clip_gather.argtypes = [c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p,
                                    c_void_p]
    L.kdlae_clip_blend.argtypes = [c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p]
    L.kdlae_clip_blend_u8.argtypes = [c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p,
                                      c_void_p, c_void_p]
    L.kdlae_stream_state_bytes.argtypes = [c_int, c_int, c_int, c_int]
    L.kdlae_stream_state_bytes.restype = c_int64
    L.kdlae_stream_reset.argtypes = [c_void_p, c_void_p]
    L.kdlae_stream_push_u8.argtypes = [c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p,
                                       c_void_p]
    L.kdlae_stream_push_f32.argtypes = [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p]
    L.kdlae_stream_advance.argtypes = [c_void_p, c_void_p]
    L.kdlae_distill_expand_u8.argtypes = [c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p, c_int, c_int,
                                          c_void_p, c_void_p, c_void_p]
    L.kdlae_distill_expand_f32.argtypes = [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_int, c_int, c_void_p,
                                           c_void_p, c_void_p]
    L.kdlae_distill_collapse.argtypes = [c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int,
                                         c_void_p, c_int, c_void_p, c_int, c_void_p]
    L.kdlae_t_probe_arm.argtypes = [c_void_p, c_int, c_int]
    L.kdlae_t_probe_read.argtypes = [c_void_p, ctypes.POINTER(c_double), ctypes.POINTER(c_int64),
                                     ctypes.POINTER(c_double), ctypes.POINTER(c_double)]
    L.kdlae_t_debug_tap_count.argtypes = [c_void_p]
    L.kdlae_t_debug_tap_info.argtypes = [c_void_p, c_int, c_char_p, c_int, ctypes.POINTER(c_int),
                                         ctypes.POINTER(c_int), ctypes.POINTER(c_int)]
    L.kdlae_t_debug_taps.argtypes = [c_void_p, c_int, ctypes.POINTER(c_void_p)]
    L.kdlae_t_debug_sr_fold.argtypes = [c_void_p, c_void_p, c_int64, c_void_p]
    L.kdlae_t_debug_sr_fold.restype = c_int64
    L.kdlae_s_create.argtypes = [ctypes.POINTER(SConfig), c_int, ctypes.POINTER(c_void_p)]
    L.kdlae_s_destroy.argtypes = [c_void_p]
    L.kdlae_s_num_params.argtypes = [c_void_p]
    L.kdlae_s_param_info.argtypes = [c_void_p, c_int, ctypes.POINTER(c_char_p), ctypes.POINTER(c_int64)]
    L.kdlae_s_set_param.argtypes = [c_void_p, c_char_p, c_void_p, c_int64]
    L.kdlae_s_commit_params.argtypes = [c_void_p, c_void_p]
    L.kdlae_s_workspace_bytes.argtypes = [c_void_p, c_int, c_int, c_int, c_int]
    L.kdlae_s_workspace_bytes.restype = c_int64
    L.kdlae_s_forward.argtypes = [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_int64,
                                  c_void_p]
    L.asdqe_create.argtypes = [ctypes.POINTER(AConfig), c_int, ctypes.POINTER(c_void_p)]
    L.asdqe_destroy.argtypes = [c_void_p]
    L.asdqe_num_params.argtypes = [c_void_p]
    L.asdqe_param_info.argtypes = [c_void_p, c_int, ctypes.POINTER(c_char_p), ctypes.POINTER(c_int64)]
    L.asdqe_set_param.argtypes = [c_void_p, c_char_p, c_void_p, c_int64]
    L.asdqe_commit_params.argtypes = [c_void_p, c_void_p]
    L.asdqe_workspace_bytes.argtypes = [c_void_p, c_int, c_int, c_int]
    L.asdqe_workspace_bytes.restype = c_int64
    L.asdqe_forward.argtypes = [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p,
                                c_int64, c_void_p]
    L.kdlae_padded_size.argtypes = [c_int, c_int, c_int, ctypes.POINTER(c_int), ctypes.POINTER(c_int)]
    L.kdlae_padded_size.restype = None
    L.kdlae_preprocess_u8.argtypes = [c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p,
                                      c_void_p, c_void_p]
    L.kdlae_frames_preprocess_u8.argtypes = [c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p,
                                             c_void_p]
    L.kdlae_postprocess_u8.argtypes = [c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p, c_int,
                                       c_void_p, c_void_p]
    L.kdlae_tt_create.argtypes = [ctypes.POINTER(TConfig), c_int, ctypes.POINTER(c_void_p)]
    L.kdlae_tt_create_restormer.argtypes = L.kdlae_tt_create.argtypes
    L.kdlae_tt_destroy.argtypes = [c_void_p]
    L.kdlae_tt_num_params.argtypes = [c_void_p]
    L.kdlae_tt_param_info.argtypes = [c_void_p, c_int, ctypes.POINTER(c_char_p), ctypes.POINTER(c_int64),
                                      ctypes.POINTER(c_int64)]
    L.kdlae_tt_num_floats.argtypes = [c_void_p]
    L.kdlae_tt_num_floats.restype = c_int64
    L.kdlae_tt_workspace_bytes.argtypes = [c_void_p, c_int, c_int, c_int]
    L.kdlae_tt_workspace_bytes.restype = c_int64
    L.kdlae_tt_forward.argtypes = [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p,
                                   c_void_p, c_void_p, ctypes.c_size_t, c_void_p]
    L.kdlae_tt_backward.argtypes = [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, ctypes.c_size_t,
                                    c_void_p]
    L.kdlae_tt_backward_marked.argtypes = L.kdlae_tt_backward.argtypes
    L.kdlae_tt_mark_count.argtypes = [c_void_p]
    L.kdlae_tt_mark_lo.argtypes = [c_void_p, c_int]
    L.kdlae_tt_mark_lo.restype = c_int64
    L.kdlae_tt_mark_wait.argtypes = [c_void_p, c_int, c_void_p]
    L.kdlae_tt_mark_sync.argtypes = [c_void_p, c_int]
    L.kdlae_tt_set_trainable.argtypes = [c_void_p, c_void_p, c_int]
    L.kdlae_tt_is_trainable.argtypes = [c_void_p, c_int]
    L.kdlae_tt_debug_backward_launches.argtypes = [c_void_p]
    L.kdlae_tt_debug_backward_launches.restype = c_int64
    L.kdlae_train_l1sr_scratch_floats.argtypes = []
    L.kdlae_train_l1sr_scratch_floats.restype = c_int64
    L.kdlae_train_l1sr.argtypes = [c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_void_p, c_void_p,
                                   c_void_p, c_void_p, c_void_p]
    L.kdlae_train_adamw_scratch_floats.argtypes = []
    L.kdlae_train_adamw_scratch_floats.restype = c_int64
    c_float = ctypes.c_float
    L.kdlae_train_clip_adamw.argtypes = [c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_float, c_float,
                                         c_float, c_float, c_float, c_float, c_float, c_int, c_void_p, c_int, c_void_p,
                                         c_void_p]
    L.kdlae_train_mixup.argtypes = [c_void_p, c_void_p, c_int, c_int64, c_void_p, c_float, c_void_p]
    L.kdlae_train_ema.argtypes = [c_void_p, c_void_p, c_int64, c_float, c_void_p]
    L.kdlae_st_create.argtypes = [ctypes.POINTER(SConfig), c_int, ctypes.POINTER(c_void_p)]
    L.kdlae_st_destroy.argtypes = [c_void_p]
    L.kdlae_st_num_params.argtypes = [c_void_p]
    L.kdlae_st_param_info.argtypes = [c_void_p, c_int, ctypes.POINTER(c_char_p), ctypes.POINTER(c_int64),
                                      ctypes.POINTER(c_int64)]
    L.kdlae_st_num_floats.argtypes = [c_void_p]
    L.kdlae_st_num_floats.restype = c_int64
    L.kdlae_st_workspace_bytes.argtypes = [c_void_p, c_int, c_int, c_int, c_int]
    L.kdlae_st_workspace_bytes.restype = c_int64
    L.kdlae_st_forward.argtypes = [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p,
                                   c_int64, c_void_p]
    L.kdlae_st_backward.argtypes = [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_void_p]
    L.kdlae_train_l1frames_scratch_floats.argtypes = []
    L.kdlae_train_l1frames_scratch_floats.restype = c_int64
    L.kdlae_train_l1frames.argtypes = [c_void_p, c_void_p, c_int, c_int, c_int64, ctypes.c_float, ctypes.c_float,
                                       ctypes.c_float, c_int, c_void_p, c_void_p, c_void_p, c_void_p]
    L.kdlae_train_l1sonar_scratch_floats.argtypes = []
    L.kdlae_train_l1sonar_scratch_floats.restype = c_int64
    L.kdlae_train_l1sonar.argtypes = [c_void_p, c_void_p, c_int64, ctypes.c_float, ctypes.c_float, c_int, c_void_p,
                                      c_void_p, c_void_p, c_void_p, c_void_p]
    L.asdqe_train_create.argtypes = [ctypes.POINTER(AConfig), c_int, ctypes.POINTER(c_void_p)]
    L.asdqe_train_destroy.argtypes = [c_void_p]
    L.asdqe_train_num_params.argtypes = [c_void_p]
    L.asdqe_train_param_info.argtypes = [c_void_p, c_int, ctypes.POINTER(c_char_p), ctypes.POINTER(c_int64),
                                         ctypes.POINTER(c_int64)]
    L.asdqe_train_num_floats.argtypes = [c_void_p]
    L.asdqe_train_num_floats.restype = c_int64
    L.asdqe_train_num_stat_floats.argtypes = [c_void_p]
    L.asdqe_train_num_stat_floats.restype = c_int64
    L.asdqe_train_workspace_bytes.argtypes = [c_void_p, c_int, c_int, c_int]
    L.asdqe_train_workspace_bytes.restype = c_int64
    L.asdqe_train_forward.argtypes = [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int,
                                      c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_void_p]
    L.asdqe_train_backward.argtypes = [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_int64, c_void_p]
    L.kdlae_train_mse.argtypes = [c_void_p, c_void_p, c_int, ctypes.c_float, c_void_p, c_void_p, c_void_p]
    L.kdlae_debug_bn.argtypes = [c_void_p, c_void_p]
    L.kdlae_metric_scratch_bytes.argtypes = []
    L.kdlae_metric_scratch_bytes.restype = c_int64
    L.kdlae_metric_psnr.argtypes = [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int,
                                    c_int, c_int, c_void_p, c_void_p, c_void_p]
    L.kdlae_metric_ssim_scratch_bytes.argtypes = []
    L.kdlae_metric_ssim_scratch_bytes.restype = c_int64
    L.kdlae_metric_ssim.argtypes = [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int,
                                    c_int, c_int, c_int, c_void_p, c_void_p, c_void_p]
    L.kdlae_metric_niqe_scratch_bytes.argtypes = [c_int, c_int, c_int]
    L.kdlae_metric_niqe_scratch_bytes.restype = c_int64
    L.kdlae_metric_niqe.argtypes = [c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int,
                                    ctypes.POINTER(ctypes.c_double), c_void_p, c_void_p, c_void_p, c_void_p,
                                    c_int64, c_void_p]
    L.kdlae_train_prepare.argtypes = [ctypes.POINTER(PrepSeg), c_int, c_void_p, c_int, c_float, ctypes.c_uint64,
                                      ctypes.c_uint64, c_void_p]
    L.kdlae_train_mask_frames.argtypes = [c_void_p, c_void_p, c_int, c_int, c_int, c_int,
                                          ctypes.POINTER(c_float), c_int, c_float, c_void_p, ctypes.c_uint64,
                                          ctypes.c_uint64, c_void_p]
    L.kdlae_data_sample.argtypes = [ctypes.POINTER(DataItem), c_void_p, c_int, ctypes.c_uint64, ctypes.c_uint64,
                                    c_void_p]
    L.kdlae_data_count.argtypes = [c_void_p, c_int, c_int64, c_void_p, c_void_p]
    L.kdlae_data_finish.argtypes = [c_void_p, c_int, c_int, c_int64, c_void_p, c_double, c_float, c_void_p, c_void_p,
                                    c_void_p]
    L.kdlae_debug_tgemm.argtypes = [c_void_p, c_void_p]
    for f in ("kdlae_debug_gemm", "kdlae_debug_gram", "kdlae_debug_ln", "kdlae_debug_small_in",
              "kdlae_debug_train", "kdlae_debug_train_s", "kdlae_debug_infer", "kdlae_debug_head_train"):
        getattr(L, f).argtypes = [c_void_p, c_void_p]
    L.kdlae_debug_train_blocks.argtypes = [c_int, c_int64, c_int, c_int, c_int64]
    L.kdlae_debug_gemm_variant.argtypes = [c_int, c_int, ctypes.POINTER(c_int)]
    for name in ENSEMBLE_EXPORTS:   # (src, dst, N, C, H, W, mode_mask, stream)
        getattr(L, name).argtypes = [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p]
        getattr(L, name).restype = c_int
    for name in EXPORTS:
        if not name.endswith(("_last_error", "_abi_version", "_workspace_bytes", "_padded_size", "_num_floats",
                              "_scratch_floats", "_scratch_bytes", "_state_bytes", "_params_numel", "_mark_lo", "_num_stat_floats",
                              "_backward_launches")):
            getattr(L, name).restype = c_int
    _lib = L
    return L


def last_error() -> str:
    msg = lib().kdlae_last_error()
    return msg.decode() if msg else ""


def check(rc: int, what: str) -> None:
    if rc != 0:
        err = last_error()
        code = ERRORS.get(rc, str(rc))
        if rc == 5:
            raise NotImplementedError(f"{what}: {err}")
        raise RuntimeError(f"{what} failed ({code}): {err}")
