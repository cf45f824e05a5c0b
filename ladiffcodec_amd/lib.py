"""ctypes binding of libladiffcodec.so (the C ABI in include/ladiffcodec.h).

There is deliberately no fallback: if the shared library is missing or does not load, `load()` raises.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess
from typing import Optional

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libladiffcodec.so")
CSRC = os.path.join(_HERE, "csrc")

LDC_F32, LDC_BF16, LDC_BF16_W8 = 0, 1, 2
DTYPES = {"f32": LDC_F32, "bf16": LDC_BF16, "fp8": LDC_BF16_W8}
MODEL_MAIN, MODEL_COND = 0, 1
MAX_RATIOS = 8
STREAM_ENCODER, STREAM_DECODER = 0, 1

EXPORTS = [
    "ldc_last_error", "ldc_version", "ldc_create", "ldc_destroy", "ldc_reseed", "ldc_set_option", "ldc_quantize_e4m3", "ldc_set_weight", "ldc_finalize_weights",
    "ldc_seanet_encode", "ldc_seanet_decode", "ldc_rvq_encode", "ldc_rvq_decode", "ldc_get_cond",
    "ldc_cond_upsample", "ldc_unet_forward", "ldc_p_sample", "ldc_denoise", "ldc_p_sample_loop", "ldc_infilling", "ldc_output_normalise", "ldc_decode", "ldc_ddim_times", "ldc_ddim_sample", "ldc_decode_ddim", "ldc_decode_codes", "ldc_decode_codes_ddim",
    "ldc_dpm_schedule", "ldc_dpm_sample", "ldc_decode_dpm", "ldc_decode_codes_dpm", "ldc_decode_ragged_dpm",
    "ldc_window_layout", "ldc_window_layout_n", "ldc_window_parts", "ldc_unet_forward_windows", "ldc_denoise_windows", "ldc_ddim_sample_windows", "ldc_decode_windows", "ldc_decode_ddim_windows",
    "ldc_dpm_sample_windows", "ldc_decode_dpm_windows", "ldc_decode_codes_windows", "ldc_decode_codes_dpm_windows",
    "ldc_window_group_layout", "ldc_unet_forward_windows_group", "ldc_sample_windows_group", "ldc_decode_windows_group",
    "ldc_decode_ragged", "ldc_unet_forward_ragged", "ldc_get_cond_ragged", "ldc_decode_codes_ragged", "ldc_ac_encode_ragged", "ldc_ac_decode_ragged",
    "ldc_sample_seeded", "ldc_decode_seeded", "ldc_decode_codes_seeded",
    "ldc_unet_forward_items", "ldc_pool_create", "ldc_pool_destroy", "ldc_pool_admit", "ldc_pool_admit_ddim", "ldc_pool_admit_dpm", "ldc_pool_step", "ldc_pool_remaining", "ldc_pool_take", "ldc_pool_peek", "ldc_pool_evict",
    "ldc_stream_min_first", "ldc_stream_create", "ldc_stream_reset", "ldc_stream_destroy", "ldc_seanet_encode_stream", "ldc_seanet_decode_stream", "ldc_get_cond_stream",
    "ldc_sconv1d", "ldc_sconvtr1d", "ldc_slstm", "ldc_unet_debug_tap", "ldc_unet_step_cost", "ldc_profile_enable",
    "ldc_profile_read", "ldc_profile_read_classes", "ldc_conv_microbench", "ldc_conv_compare", "ldc_conv_compare_fp8", "ldc_ln_fold_compare", "ldc_gn_microbench", "ldc_host_stats", "ldc_graph_schedule", "ldc_stream_info", "ldc_clock_sample", "ldc_debug_raise_failure", "ldc_debug_attn_core", "ldc_debug_attention_block", "ldc_debug_resnet_block", "ldc_debug_sea_conv", "ldc_debug_sea_op", "ldc_debug_sync_count", "ldc_debug_lean_launches", "ldc_xcc_census", "ldc_timeline_enable", "ldc_timeline_read", "ldc_kstamps_enable", "ldc_kstamps_reset", "ldc_kstamps_read", "ldc_packed_bytes", "ldc_pack_codes", "ldc_unpack_codes",
    "ldc_ac_build_cdf", "ldc_ac_encode", "ldc_ac_decode", "ldc_train_q_sample", "ldc_train_num_timesteps", "ldc_train_predict_x_start", "ldc_train_neg_sdsdr", "ldc_train_l1_loss", "ldc_train_block_ws_floats",
    "ldc_train_block_forward", "ldc_train_block_backward", "ldc_train_layernorm_forward", "ldc_train_layernorm_backward", "ldc_train_adam_step", "ldc_train_adam_step_dev", "ldc_train_pointwise_forward", "ldc_train_pointwise_backward", "ldc_train_linattn_ws_floats", "ldc_train_linattn_forward", "ldc_train_linattn_backward", "ldc_train_conv_forward", "ldc_train_conv_backward", "ldc_train_join", "ldc_train_side_stream", "ldc_train_upsample2", "ldc_train_activation", "ldc_train_attn_ws_floats", "ldc_train_attn_forward", "ldc_train_attn_backward", "ldc_train_convtr_forward", "ldc_train_convtr_backward", "ldc_train_maxscale", "ldc_resample_out_len", "ldc_resample",
]


class LdcConfig(C.Structure):
    _fields_ = [
        ("compute_dtype", C.c_int32), ("rep_dims", C.c_int32), ("n_filters", C.c_int32),
        ("n_residual_layers", C.c_int32), ("lstm", C.c_int32), ("n_enc_ratios", C.c_int32),
        ("enc_ratios", C.c_int32 * MAX_RATIOS), ("diff_dims", C.c_int32), ("n_upsampling_ratios", C.c_int32),
        ("upsampling_ratios", C.c_int32 * MAX_RATIOS), ("unet_scale_cond", C.c_int32), ("unet_scale_x", C.c_int32),
        ("has_cond_model", C.c_int32), ("cond_bandwidth", C.c_float), ("max_batch", C.c_int32),
        ("max_latent_len", C.c_int32), ("noise_seed", C.c_uint64), ("final_activation", C.c_int32),
        ("reserved_", C.c_int32),
    ]


# --final_activation names -> LDC_ACT_* (include/ladiffcodec.h)
FINAL_ACTIVATIONS = {None: 0, "Identity": 0, "Tanh": 1, "Sigmoid": 2, "ELU": 3, "SiLU": 4, "GELU": 5, "ReLU": 6}


# LDC_E_* (include/ladiffcodec.h)
E_INVALID, E_STATE, E_MISSING, E_HIP, E_NOMEM = -1, -2, -3, -4, -5


class LdcError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"libladiffcodec error {code}: {msg}")
        self.code = code


_lib: Optional[C.CDLL] = None


def build(verbose: bool = False) -> str:
    """Compile the HIP sources for gfx950 (hipcc cross-compiles without a GPU)."""
    r = subprocess.run(["make", "-C", CSRC, "-j8"], capture_output=True, text=True)
    if verbose or r.returncode != 0:
        print(r.stdout[-4000:])
        print(r.stderr[-8000:])
    if r.returncode != 0:
        raise RuntimeError("building libladiffcodec.so failed")
    return LIB_PATH


def load() -> C.CDLL:
    global _lib
    if _lib is not None:
        return _lib
    path = os.environ.get("LDC_LIB_PATH", LIB_PATH)   # tuning aid: A/B two builds of the library on one GPU box
    if not os.path.exists(path):
        raise RuntimeError(f"{path} not found: run `python -c 'import __graft_entry__ as g; g.build()'` "
                           f"(or `make -C {CSRC}`). There is no CPU fallback.")
    lib = C.CDLL(path)
    vp, i32, i64p, fp = C.c_void_p, C.c_int, C.POINTER(C.c_int64), C.c_void_p
    lib.ldc_last_error.restype = C.c_char_p
    lib.ldc_version.restype = C.c_char_p
    lib.ldc_create.argtypes = [C.POINTER(LdcConfig), i32, C.POINTER(vp)]
    lib.ldc_destroy.argtypes = [vp]
    lib.ldc_reseed.argtypes = [vp, C.c_uint64]
    lib.ldc_quantize_e4m3.argtypes = [vp, C.c_int64, vp, vp]
    lib.ldc_set_weight.argtypes = [vp, i32, C.c_char_p, vp, i64p, i32]
    lib.ldc_finalize_weights.argtypes = [vp, i32]
    lib.ldc_seanet_encode.argtypes = [vp, i32, fp, i32, i32, fp, vp]
    lib.ldc_seanet_decode.argtypes = [vp, i32, fp, i32, i32, fp, vp]
    lib.ldc_rvq_encode.argtypes = [vp, fp, i32, i32, i32, vp, fp, vp]
    lib.ldc_rvq_decode.argtypes = [vp, vp, i32, i32, i32, fp, vp]
    lib.ldc_get_cond.argtypes = [vp, fp, i32, i32, C.c_float, fp, vp, vp]
    lib.ldc_cond_upsample.argtypes = [vp, fp, i32, i32, i32, fp, vp]
    lib.ldc_unet_forward.argtypes = [vp, fp, i32, fp, i32, i32, i32, fp, vp]
    lib.ldc_p_sample.argtypes = [vp, fp, i32, fp, fp, i32, i32, i32, vp]
    lib.ldc_denoise.argtypes = [vp, fp, fp, fp, i32, i32, i32, i32, vp]
    lib.ldc_p_sample_loop.argtypes = [vp, fp, fp, fp, i32, i32, i32, i32, vp]
    lib.ldc_infilling.argtypes = [vp, fp, fp, fp, i32, fp, C.c_float, i32, i32, i32, i32, vp]
    lib.ldc_output_normalise.argtypes = [vp, fp, i32, i32, i32, vp]
    lib.ldc_decode.argtypes = [vp, fp, i32, i32, i32, fp, i32, fp, fp, fp, vp, vp]
    lib.ldc_ddim_times.argtypes = [i32, i32, C.POINTER(C.c_int)]
    lib.ldc_graph_schedule.argtypes = [i32, i32, i32, i32, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]
    lib.ldc_ddim_sample.argtypes = [vp, fp, fp, fp, i32, i32, i32, C.c_float, i32, i32, i32, vp]
    lib.ldc_decode_ddim.argtypes = [vp, fp, i32, i32, i32, i32, C.c_float, fp, i32, fp, fp, fp, vp, vp]
    lib.ldc_decode_codes.argtypes = [vp, vp, vp, C.c_int64, i32, i32, i32, i32, i32, fp, i32, fp, fp, fp, vp]
    lib.ldc_decode_codes_ddim.argtypes = [vp, vp, vp, C.c_int64, i32, i32, i32, i32, i32, i32, C.c_float, fp, i32, fp, fp, fp, vp]
    lib.ldc_decode_ragged.argtypes = [vp, fp, C.POINTER(C.c_int32), i32, i32, i32, i32, C.c_float, fp, fp, fp, fp, vp, vp]
    lib.ldc_get_cond_ragged.argtypes = [vp, fp, C.POINTER(C.c_int32), i32, i32, C.c_float, fp, vp, vp]
    lib.ldc_decode_codes_ragged.argtypes = [vp, vp, vp, C.c_int64, i32, i32, i32, i32, C.POINTER(C.c_int32), i32, i32, C.c_float, fp, fp, fp, fp, vp]
    lib.ldc_dpm_schedule.argtypes = [fp, fp, i32, i32, i32, C.POINTER(C.c_int), C.POINTER(C.c_float)]
    lib.ldc_dpm_sample.argtypes = [vp, fp, fp, i32, i32, i32, i32, i32, vp]
    lib.ldc_decode_dpm.argtypes = [vp, fp, i32, i32, i32, i32, i32, fp, fp, fp, vp, vp]
    lib.ldc_decode_codes_dpm.argtypes = [vp, vp, vp, C.c_int64, i32, i32, i32, i32, i32, i32, i32, fp, fp, fp, vp]
    lib.ldc_decode_ragged_dpm.argtypes = [vp, fp, C.POINTER(C.c_int32), i32, i32, i32, i32, fp, fp, fp, vp, vp]
    lib.ldc_window_layout.argtypes = [i32, i32, i32, i32, C.POINTER(C.c_int), C.POINTER(C.c_float)]
    lib.ldc_window_layout_n.argtypes = [i32, i32, i32, i32, i32, C.POINTER(C.c_int), C.POINTER(C.c_float)]
    lib.ldc_window_parts.argtypes = [i32, i32, C.POINTER(C.c_int)]
    lib.ldc_unet_forward_windows.argtypes = [vp, fp, i32, fp, i32, i32, i32, i32, fp, vp]
    lib.ldc_denoise_windows.argtypes = [vp, fp, fp, fp, i32, i32, i32, i32, i32, vp]
    lib.ldc_ddim_sample_windows.argtypes = [vp, fp, fp, fp, i32, i32, C.c_float, i32, i32, i32, i32, vp]
    lib.ldc_decode_windows.argtypes = [vp, fp, i32, i32, fp, i32, i32, fp, fp, fp, vp, vp]
    lib.ldc_decode_ddim_windows.argtypes = [vp, fp, i32, i32, i32, C.c_float, fp, i32, i32, fp, fp, fp, vp, vp]
    lib.ldc_dpm_sample_windows.argtypes = [vp, fp, fp, i32, i32, i32, i32, i32, i32, vp]
    lib.ldc_decode_dpm_windows.argtypes = [vp, fp, i32, i32, i32, i32, i32, fp, fp, fp, vp, vp]
    lib.ldc_decode_codes_windows.argtypes = [vp, vp, vp, C.c_int64, i32, i32, i32, i32, i32, C.c_float, fp, i32, i32, fp, fp, fp, vp]
    lib.ldc_decode_codes_dpm_windows.argtypes = [vp, vp, vp, C.c_int64, i32, i32, i32, i32, i32, i32, i32, fp, fp, fp, vp]
    ip, u64p = C.POINTER(C.c_int), C.POINTER(C.c_uint64)
    lib.ldc_window_group_layout.argtypes = [i32, ip, i32, i32, i32, ip, ip, C.POINTER(C.c_float)]
    lib.ldc_unet_forward_windows_group.argtypes = [vp, fp, i32, fp, i32, ip, ip, i32, i32, fp, vp]
    lib.ldc_sample_windows_group.argtypes = [vp, fp, fp, i32, i32, i32, C.c_float, fp, u64p, i32, ip, ip, i32, i32, vp]
    lib.ldc_decode_windows_group.argtypes = [vp, fp, i32, ip, i32, i32, i32, C.c_float, fp, u64p, i32, i32, fp, fp, fp, vp, vp]
    lib.ldc_sample_seeded.argtypes = [vp, fp, fp, i32, i32, i32, C.c_float, u64p, i32, i32, i32, vp]
    lib.ldc_decode_seeded.argtypes = [vp, fp, C.POINTER(C.c_int32), i32, i32, i32, i32, i32, C.c_float, u64p, fp, fp, fp, vp, vp]
    lib.ldc_decode_codes_seeded.argtypes = [vp, vp, vp, C.c_int64, i32, i32, i32, i32, C.POINTER(C.c_int32), i32, i32, i32, C.c_float, u64p, fp, fp,
                                            fp, vp]
    lib.ldc_ac_encode_ragged.argtypes = [vp, vp, vp, vp, i32, i32, i32, i32, i32, vp, C.c_int64, vp, vp]
    lib.ldc_ac_decode_ragged.argtypes = [vp, vp, C.c_int64, vp, vp, vp, i32, i32, i32, i32, i32, vp, vp, vp]
    lib.ldc_unet_forward_ragged.argtypes = [vp, fp, i32, fp, C.POINTER(C.c_int32), i32, i32, i32, fp, vp]
    lib.ldc_unet_forward_items.argtypes = [vp, fp, C.POINTER(C.c_int32), fp, C.POINTER(C.c_int32), i32, i32, i32, fp, vp]
    lib.ldc_pool_create.argtypes = [vp, i32, i32, C.POINTER(vp)]
    lib.ldc_pool_destroy.argtypes = [vp]
    lib.ldc_pool_admit.argtypes = [vp, vp, i32, fp, fp, i32, i32, fp, C.c_uint64, vp]
    lib.ldc_pool_admit_ddim.argtypes = [vp, vp, i32, fp, fp, i32, i32, i32, C.c_float, fp, C.c_uint64, vp]
    lib.ldc_pool_admit_dpm.argtypes = [vp, vp, i32, fp, fp, i32, i32, i32, vp]
    lib.ldc_pool_step.argtypes = [vp, vp, i32, vp]
    lib.ldc_pool_remaining.argtypes = [vp, C.POINTER(C.c_int32)]
    lib.ldc_pool_take.argtypes = [vp, vp, i32, fp, vp]
    lib.ldc_pool_peek.argtypes = [vp, vp, i32, fp, vp]
    lib.ldc_pool_evict.argtypes = [vp, i32]
    lib.ldc_stream_min_first.argtypes = [C.POINTER(LdcConfig), i32, i32]
    lib.ldc_stream_create.argtypes = [vp, i32, i32, i32, C.POINTER(vp)]
    lib.ldc_stream_reset.argtypes = [vp, vp, vp]
    lib.ldc_stream_destroy.argtypes = [vp]
    lib.ldc_seanet_encode_stream.argtypes = [vp, vp, fp, i32, fp, vp]
    lib.ldc_seanet_decode_stream.argtypes = [vp, vp, fp, i32, fp, vp]
    lib.ldc_get_cond_stream.argtypes = [vp, vp, fp, i32, C.c_float, fp, vp, vp]
    lib.ldc_sconv1d.argtypes = [vp, fp, i32, i32, i32, vp, vp, i32, i32, i32, i32, i32, i32, fp, vp]
    lib.ldc_sconvtr1d.argtypes = [vp, fp, i32, i32, i32, vp, vp, i32, i32, i32, i32, fp, vp]
    lib.ldc_slstm.argtypes = [vp, fp, i32, i32, i32, C.POINTER(vp), i32, fp, vp]
    lib.ldc_unet_debug_tap.argtypes = [vp, C.c_char_p, fp, C.c_int64, vp]
    lib.ldc_unet_step_cost.argtypes = [vp, i32, i32, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    lib.ldc_profile_enable.argtypes = [vp, i32]
    lib.ldc_profile_read.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_int64), C.POINTER(C.c_double)]
    lib.ldc_profile_read_classes.argtypes = [vp, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_int64), C.POINTER(C.c_double), C.POINTER(C.c_double)]
    lib.ldc_set_option.argtypes = [vp, C.c_char_p, i32]
    lib.ldc_train_num_timesteps.argtypes = [vp]
    lib.ldc_train_predict_x_start.argtypes = [vp, vp, vp, vp, i32, i32, i32, vp, vp]
    lib.ldc_train_neg_sdsdr.argtypes = [vp, vp, vp, i32, C.c_int64, C.c_float, vp, vp]
    lib.ldc_host_stats.argtypes = [vp, i32, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_int64)]
    lib.ldc_stream_info.argtypes = [vp, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_int)]
    lib.ldc_clock_sample.argtypes = [vp, C.POINTER(C.c_uint64), vp]
    lib.ldc_xcc_census.argtypes = [vp, vp, i32, i32, vp]
    lib.ldc_conv_microbench.argtypes = [vp, i32, i32, i32, i32, i32, i32, i32, i32, i32, i32, C.POINTER(C.c_double)]
    lib.ldc_conv_compare.argtypes = [vp] + [i32] * 13 + [C.POINTER(C.c_double)] * 3
    lib.ldc_conv_compare_fp8.argtypes = [vp] + [i32] * 10 + [C.POINTER(C.c_double)] * 3
    lib.ldc_ln_fold_compare.argtypes = [vp, i32, i32, i32, i32, C.c_double, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    lib.ldc_debug_attn_core.argtypes = [vp, i32, fp, i32, i32, vp, vp, vp, fp, i32, fp, vp]
    lib.ldc_debug_attention_block.argtypes = [vp, C.c_char_p, fp, i32, i32, fp, vp]
    lib.ldc_debug_resnet_block.argtypes = [vp, C.c_char_p, fp, fp, i32, i32, i32, C.POINTER(i32), i32, C.POINTER(i32), i32, fp, fp, vp, fp, fp, C.POINTER(i32), vp]
    lib.ldc_debug_sea_conv.argtypes = [vp, fp, i32, i32, i32, vp, vp, i32, i32, i32, i32, i32, i32, i32, fp, fp, C.POINTER(i32), vp]
    lib.ldc_debug_sea_op.argtypes = [vp, i32, i32, i32, fp, i32, i32, fp, C.c_int64, C.POINTER(i32), vp]
    lib.ldc_timeline_enable.argtypes = [vp, i32]
    lib.ldc_timeline_read.argtypes = [vp, i32, i32, C.POINTER(C.c_uint64)]
    lib.ldc_kstamps_enable.argtypes = [vp, i32]
    lib.ldc_kstamps_reset.argtypes = [vp]
    lib.ldc_kstamps_read.argtypes = [vp, i32, i32, C.POINTER(i32), C.POINTER(C.c_uint64), C.c_char_p, i32, C.POINTER(i32)]
    lib.ldc_packed_bytes.argtypes = [i32, i32, i32]
    lib.ldc_pack_codes.argtypes = [vp, vp, i32, i32, i32, i32, vp, C.c_int64, vp]
    lib.ldc_unpack_codes.argtypes = [vp, vp, C.c_int64, i32, i32, i32, i32, vp, vp]
    lib.ldc_ac_build_cdf.argtypes = [vp, vp, i32, i32, i32, C.c_float, i32, vp, vp]
    lib.ldc_ac_encode.argtypes = [vp, vp, vp, i32, i32, i32, i32, i32, vp, C.c_int64, vp, vp]
    lib.ldc_ac_decode.argtypes = [vp, vp, C.c_int64, vp, vp, i32, i32, i32, i32, i32, vp, vp, vp]
    lib.ldc_train_q_sample.argtypes = [vp, fp, vp, fp, i32, i32, i32, fp, vp]
    lib.ldc_train_l1_loss.argtypes = [vp, fp, fp, vp, i32, i32, i32, fp, fp, vp]
    lib.ldc_train_block_ws_floats.argtypes = [i32, i32, i32, i32, i32]
    lib.ldc_train_block_forward.argtypes = [vp, fp, fp, fp, fp, fp, fp, i32, i32, i32, i32, i32, fp, fp, vp]
    lib.ldc_train_block_backward.argtypes = [vp, fp, fp, fp, fp, fp, i32, i32, i32, i32, i32, fp, fp, fp, fp, fp, fp, fp, vp]
    lib.ldc_train_layernorm_forward.argtypes = [vp, fp, fp, i32, i32, i32, fp, fp, vp]
    lib.ldc_train_layernorm_backward.argtypes = [vp, fp, fp, fp, fp, i32, i32, i32, fp, fp, vp]
    lib.ldc_train_pointwise_forward.argtypes = [vp, fp, fp, fp, i32, i32, i32, i32, i32, fp, vp]
    lib.ldc_train_pointwise_backward.argtypes = [vp, fp, fp, fp, i32, i32, i32, i32, i32, fp, fp, fp, vp]
    lib.ldc_train_linattn_ws_floats.argtypes = [i32, i32, i32, i32]
    lib.ldc_train_linattn_ws_floats.restype = C.c_int64
    lib.ldc_train_linattn_forward.argtypes = [vp, fp, i32, i32, i32, i32, fp, fp, vp]
    lib.ldc_train_linattn_backward.argtypes = [vp, fp, fp, i32, i32, i32, i32, fp, fp, vp]
    lib.ldc_train_conv_forward.argtypes = [vp, fp, fp, fp, i32, i32, i32, i32, i32, i32, i32, fp, vp]
    lib.ldc_train_conv_backward.argtypes = [vp, fp, fp, fp, i32, i32, i32, i32, i32, i32, i32, fp, fp, fp, vp]
    lib.ldc_train_join.argtypes = [vp, vp]
    lib.ldc_train_side_stream.argtypes = [vp, C.POINTER(C.c_void_p)]
    lib.ldc_train_upsample2.argtypes = [vp, fp, C.c_int64, i32, i32, fp, vp]
    lib.ldc_train_activation.argtypes = [vp, fp, fp, C.c_int64, i32, fp, vp]
    lib.ldc_train_attn_ws_floats.argtypes = [i32, i32, i32]
    lib.ldc_train_attn_forward.argtypes = [vp, fp, i32, i32, i32, i32, fp, fp, vp]
    lib.ldc_train_attn_backward.argtypes = [vp, fp, fp, i32, i32, i32, i32, fp, fp, vp]
    lib.ldc_train_convtr_forward.argtypes = [vp, fp, fp, fp, i32, i32, i32, i32, i32, fp, vp]
    lib.ldc_train_convtr_backward.argtypes = [vp, fp, fp, fp, i32, i32, i32, i32, i32, fp, fp, fp, vp]
    lib.ldc_train_maxscale.argtypes = [vp, fp, fp, i32, C.c_int64, fp, vp]
    lib.ldc_train_adam_step.argtypes = [vp, fp, fp, fp, fp, C.c_int64, i32, C.c_float, C.c_float, C.c_float, C.c_float, vp]
    lib.ldc_train_adam_step_dev.argtypes = [vp, fp, fp, fp, fp, C.c_int64, vp, C.c_float, C.c_float, C.c_float, C.c_float, vp]
    lib.ldc_resample_out_len.argtypes = [C.c_int64, i32, i32]
    lib.ldc_resample.argtypes = [vp, fp, i32, C.c_int64, i32, i32, fp, vp]
    # (LDC_LIB_PATH may name an older build for an A/B: a test hook it lacks is skipped, everything else must be there)
    optional = {"ldc_debug_lean_launches"} if "LDC_LIB_PATH" in os.environ else set()
    if hasattr(lib, "ldc_debug_lean_launches"):
        lib.ldc_debug_lean_launches.argtypes = [i32]
    lib.ldc_gn_microbench.argtypes = [vp, i32, i32, i32, i32, i32, i32, C.POINTER(C.c_double)]
    for name in EXPORTS:
        if name in optional and not hasattr(lib, name):
            continue
        fn = getattr(lib, name)
        if name in ("ldc_debug_sync_count", "ldc_debug_lean_launches", "ldc_packed_bytes", "ldc_train_block_ws_floats", "ldc_train_linattn_ws_floats", "ldc_train_attn_ws_floats", "ldc_resample_out_len"):
            fn.restype = C.c_int64
        elif name == "ldc_quantize_e4m3":
            fn.restype = None
        elif name not in ("ldc_last_error", "ldc_version"):
            fn.restype = C.c_int
    _lib = lib
    return lib


def ddim_times(t_start: int, n_steps: int):
    """The reference's DDIM timestep list (n_steps + 1 entries, the last -1): ldc_ddim_times, host-only."""
    out = (C.c_int * (int(n_steps) + 1))() if n_steps >= 0 else (C.c_int * 1)()
    check(load().ldc_ddim_times(int(t_start), int(n_steps), out))
    return list(out)


def window_layout(Ltot: int, Lw: int, overlap: int, up: int, max_windows: int = 32):
    """The coupled-windows layout of ldc_window_layout (host-only): -> (starts [W] list, weights [W, Lw'] float32), Lw' = min(Lw, Ltot).
    max_windows other than 32 (up to 128: the layouts of a call in batch parts, 32 windows per part) goes through ldc_window_layout_n;
    the engine's own calls take 32 windows."""
    import numpy as np
    lib = load()
    max_windows = int(max_windows)
    if max_windows == 32:
        def call(starts, weights):
            return lib.ldc_window_layout(int(Ltot), int(Lw), int(overlap), int(up), starts, weights)
    else:
        def call(starts, weights):
            return lib.ldc_window_layout_n(int(Ltot), int(Lw), int(overlap), int(up), max_windows, starts, weights)
    starts = (C.c_int * max(32, max_windows))()
    W = call(starts, None)
    if W < 0:
        check(W)
    lw = min(int(Lw), int(Ltot))
    weights = (C.c_float * (W * lw))()
    check(min(0, call(starts, weights)))
    return list(starts)[:W], np.array(weights, dtype=np.float32).reshape(W, lw)


def window_group_layout(Ltot, Lw: int, overlap: int, up: int):
    """The layout of a window group (ldc_window_group_layout, host-only): R recordings of Ltot[r] latent frames whose windows share one
    batch -> (w0 [R + 1] list: recording r's windows are the batch items w0[r] .. w0[r + 1] - 1, starts [W_sum] list in each recording's
    own frames, weights [W_sum, Lw] float32)."""
    import numpy as np
    lib = load()
    lens = [int(v) for v in Ltot]
    R = len(lens)
    arr = (C.c_int * max(1, R))(*lens)
    w0 = (C.c_int * (R + 1))()
    starts = (C.c_int * 32)()
    W = lib.ldc_window_group_layout(R, arr, int(Lw), int(overlap), int(up), w0, starts, None)
    if W < 0:
        check(W)
    weights = (C.c_float * (W * int(Lw)))()
    check(min(0, lib.ldc_window_group_layout(R, arr, int(Lw), int(overlap), int(up), w0, starts, weights)))
    return list(w0), list(starts)[:W], np.array(weights, dtype=np.float32).reshape(W, int(Lw))


def window_parts(W: int, parts: int):
    """W windows cut into min(parts, W) contiguous batch parts (ldc_window_parts, host-only): -> the P_eff + 1 range starts;
    part p holds the windows [first[p], first[p + 1])."""
    first = (C.c_int * (max(1, int(parts)) + 1))()
    p_eff = load().ldc_window_parts(int(W), int(parts), first)
    if p_eff < 0:
        check(p_eff)
    return list(first)[:p_eff + 1]


def dpm_schedule(sqrt_recip, sqrt_recipm1, t_start: int, n_steps: int):
    """The DPM-Solver++(2M) table of ldc_dpm_schedule (host-only) from the checkpoint's sqrt_recip_alphas_cumprod /
    sqrt_recipm1_alphas_cumprod tables: -> (t [n_steps] int32, coef [n_steps, 3] float32 rows (a, b0, b1))."""
    import numpy as np
    R = np.ascontiguousarray(np.asarray(sqrt_recip, dtype=np.float32))
    M = np.ascontiguousarray(np.asarray(sqrt_recipm1, dtype=np.float32))
    if R.ndim != 1 or R.shape != M.shape:
        raise ValueError("the two tables must be one-dimensional and of one length")
    n = max(int(n_steps), 1)
    t_out, coef = (C.c_int * n)(), (C.c_float * (3 * n))()
    check(load().ldc_dpm_schedule(R.ctypes.data, M.ctypes.data, int(R.shape[0]), int(t_start), int(n_steps), t_out, coef))
    return np.array(t_out, dtype=np.int32), np.array(coef, dtype=np.float32).reshape(n, 3)


def stream_min_first(cfg: LdcConfig, which: int, side: int) -> int:
    """Smallest first chunk of a stream session, in input units (samples for an encoder, latent frames for a decoder):
    ldc_stream_min_first, host-only."""
    n = load().ldc_stream_min_first(C.byref(cfg), int(which), int(side))
    if n < 0:
        check(n)
    return n


def check(rc: int) -> None:
    if rc != 0:
        raise LdcError(rc, load().ldc_last_error().decode("utf-8", "replace"))
