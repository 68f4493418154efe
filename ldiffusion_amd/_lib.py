"""ctypes binding of libldiff_hip.so (include/ldiff.h).  No fallback: if the shared object is
missing or cannot be loaded the import of any compute entry point raises.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libldiff_hip.so")
MAX_BLOCKS = 8

F32, F16, BF16 = 0, 1, 2


class UNetCfg(C.Structure):
    _fields_ = [("in_channels", C.c_int), ("out_channels", C.c_int), ("n_blocks", C.c_int),
                ("block_out_channels", C.c_int * MAX_BLOCKS), ("down_has_attn", C.c_int * MAX_BLOCKS),
                ("up_has_attn", C.c_int * MAX_BLOCKS), ("layers_per_block", C.c_int), ("heads", C.c_int),
                ("cross_attention_dim", C.c_int), ("norm_num_groups", C.c_int), ("norm_eps", C.c_float),
                ("flip_sin_to_cos", C.c_int), ("freq_shift", C.c_float)]


class VaeCfg(C.Structure):
    _fields_ = [("in_channels", C.c_int), ("out_channels", C.c_int), ("latent_channels", C.c_int), ("n_blocks", C.c_int),
                ("block_out_channels", C.c_int * MAX_BLOCKS), ("layers_per_block", C.c_int), ("norm_num_groups", C.c_int),
                ("scaling_factor", C.c_float)]


class TextEncCfg(C.Structure):
    _fields_ = [("vocab_size", C.c_int), ("hidden", C.c_int), ("intermediate", C.c_int), ("layers", C.c_int), ("heads", C.c_int),
                ("max_positions", C.c_int), ("act", C.c_int), ("ln_eps", C.c_float)]


class ConvArgs(C.Structure):
    _fields_ = [("x", C.c_void_p), ("x2", C.c_void_p), ("C1", C.c_int), ("C2", C.c_int),
                ("B", C.c_int), ("Hin", C.c_int), ("Win", C.c_int), ("Hout", C.c_int), ("Wout", C.c_int),
                ("ks", C.c_int), ("stride", C.c_int), ("pad_t", C.c_int), ("pad_l", C.c_int), ("ups", C.c_int),
                ("w", C.c_void_p), ("N", C.c_int), ("Nrows", C.c_int),
                ("gn_scale", C.c_void_p), ("gn_shift", C.c_void_p), ("silu_in", C.c_int),
                ("bias", C.c_void_p), ("temb", C.c_void_p), ("ld_temb", C.c_int),
                ("res", C.c_void_p), ("ld_res", C.c_int), ("y", C.c_void_p), ("ldy", C.c_int), ("out_f32", C.c_int), ("stats", C.c_void_p),
                ("geglu", C.c_int), ("ld1", C.c_int), ("ld2", C.c_int), ("res_lo", C.c_int), ("y_lo", C.c_int), ("short_runs", C.c_int),
                ("lo8_slab0", C.c_int), ("lo8_scale", C.c_void_p), ("gemm_df", C.c_int),
                ("sc_x", C.c_void_p), ("sc_C", C.c_int), ("sc_ld", C.c_int), ("sc_w", C.c_void_p), ("sc_bias", C.c_void_p), ("c3d_ups", C.c_int), ("n_real", C.c_int), ("splitk", C.c_int),
                ("out_shift", C.c_int), ("silu_out", C.c_int), ("cond_conv", C.c_int), ("lrelu_in", C.c_int), ("tconv", C.c_int), ("seg_conv", C.c_int),
                ("relu_out", C.c_int), ("cls_conv", C.c_int), ("bn_stats", C.c_void_p), ("fold_gn", C.c_int), ("act_out", C.c_int)]


class SegMetricsOut(C.Structure):
    _fields_ = [("num_classes", C.c_int), ("dice", C.c_float * 32), ("dice_mean", C.c_float), ("iou", C.c_double * 32), ("iou_skipped", C.c_int * 32),
                ("iou_mean", C.c_double), ("pa", C.c_double * 32), ("pa_mean", C.c_double), ("fw_iou", C.c_float), ("fw_iou_fg", C.c_float)]


class SegCase(C.Structure):     # ldiff_seg_case
    _fields_ = [("coef_off", C.c_int64), ("raw_off", C.c_int64), ("label_off", C.c_int64), ("H", C.c_int32), ("W", C.c_int32), ("stride", C.c_int32),
                ("label_stride", C.c_int32)]


class SegSample(C.Structure):   # ldiff_seg_sample
    _fields_ = [("m", C.c_float * 6), ("case_index", C.c_int32), ("copy", C.c_int32), ("noise_sigma", C.c_float), ("reserved", C.c_uint32),
                ("philox_offset", C.c_uint64)]


class SegChan(C.Structure):     # ldiff_seg_chan
    _fields_ = [("blur_sigma", C.c_float), ("brightness", C.c_float), ("contrast", C.c_float), ("lowres_zoom", C.c_float), ("gamma_inverted", C.c_float),
                ("gamma", C.c_float)]


WINDOW_MAX_TILES = 64           # LDIFF_WINDOW_MAX_TILES
CC_TILE_H, CC_TILE_W = 32, 32   # LDIFF_CC_TILE_H / _W: the tile of the connected-component kernels (tests straddle it)


class WindowTiles(C.Structure):  # ldiff_window_tiles
    _fields_ = [("n_tiles", C.c_int32), ("n_valid", C.c_int32), ("n_variants", C.c_int32), ("reserved", C.c_int32), ("variants", C.c_int32 * 4),
                ("y0", C.c_int32 * WINDOW_MAX_TILES), ("x0", C.c_int32 * WINDOW_MAX_TILES)]


# name -> (restype, argtypes); every symbol include/ldiff.h declares
P, I, F, I64, U64 = C.c_void_p, C.c_int, C.c_float, C.c_int64, C.c_uint64
SIGNATURES = {
    "ldiff_version": (I, []),
    "ldiff_last_error": (C.c_char_p, []),
    "ldiff_unet_create": (I, [C.POINTER(P), C.POINTER(UNetCfg), I]),
    "ldiff_unet_load": (I, [P, C.c_char_p, P, I, C.POINTER(I64), I]),
    "ldiff_unet_set_precision": (I, [P, I]),
    "ldiff_unet_set_plan_batch": (I, [P, I]),
    "ldiff_unet_set_graph": (I, [P, I]),
    "ldiff_unet_graph_replays": (I64, [P]),
    "ldiff_unet_graph_nodes": (I64, [P]),
    "ldiff_unet_missing": (I, [P]),
    "ldiff_unet_missing_name": (C.c_char_p, [P, I]),
    "ldiff_unet_set_context": (I, [P, P, I, I, P]),
    "ldiff_unet_forward": (I, [P, P, I, I, I, F, P, P]),
    "ldiff_unet_set_additional_residuals": (I, [P, C.POINTER(P), I, P]),
    "ldiff_unet_check_finite": (I, [P, P]),
    "ldiff_unet_destroy": (None, [P]),
    "ldiff_controlnet_create": (I, [C.POINTER(P), C.POINTER(UNetCfg), I, C.POINTER(I), I, I]),
    "ldiff_controlnet_load": (I, [P, C.c_char_p, P, I, C.POINTER(I64), I]),
    "ldiff_controlnet_missing": (I, [P]),
    "ldiff_controlnet_missing_name": (C.c_char_p, [P, I]),
    "ldiff_controlnet_set_precision": (I, [P, I]),
    "ldiff_controlnet_set_plan_batch": (I, [P, I]),
    "ldiff_controlnet_set_context": (I, [P, P, I, I, P]),
    "ldiff_controlnet_set_cond": (I, [P, P, I, I, I, P]),
    "ldiff_controlnet_forward": (I, [P, P, I, I, I, F, F, C.POINTER(P), I, P, P]),
    "ldiff_controlnet_check_finite": (I, [P, P]),
    "ldiff_controlnet_destroy": (None, [P]),
    "ldiff_unet_attach_controlnet": (I, [P, P, F]),
    "ldiff_segnet_create": (I, [C.POINTER(P), I, I, C.POINTER(I), C.POINTER(I), C.POINTER(I), C.POINTER(I), I, I]),
    "ldiff_segnet_load": (I, [P, C.c_char_p, P, I, C.POINTER(I64), I]),
    "ldiff_segnet_missing": (I, [P]),
    "ldiff_segnet_missing_name": (C.c_char_p, [P, I]),
    "ldiff_segnet_set_graph": (I, [P, I]),
    "ldiff_segnet_graph_replays": (I64, [P]),
    "ldiff_segnet_forward": (I, [P, P, I, I, I, P, I, P]),
    "ldiff_segnet_check_finite": (I, [P, P]),
    "ldiff_segnet_destroy": (None, [P]),
    "ldiff_resnet_create": (I, [C.POINTER(P), C.POINTER(I), I, I, I, I]),
    "ldiff_resnet_load": (I, [P, C.c_char_p, P, I, C.POINTER(I64), I]),
    "ldiff_resnet_missing": (I, [P]),
    "ldiff_resnet_missing_name": (C.c_char_p, [P, I]),
    "ldiff_resnet_set_graph": (I, [P, I]),
    "ldiff_resnet_graph_replays": (I64, [P]),
    "ldiff_resnet_forward": (I, [P, P, I, I, P, P, P]),
    "ldiff_resnet_set_train": (I, [P, I]),
    "ldiff_resnet_bn_channels": (I64, [P]),
    "ldiff_resnet_bn_entry": (I, [P, I, C.POINTER(C.c_char_p), C.POINTER(I64), C.POINTER(I)]),
    "ldiff_resnet_forward_train": (I, [P, P, I, I, P, P, P, P, P]),
    "ldiff_resnet_check_finite": (I, [P, P]),
    "ldiff_resnet_destroy": (None, [P]),
    "ldiff_textenc_create": (I, [C.POINTER(P), C.POINTER(TextEncCfg), I]),
    "ldiff_textenc_load": (I, [P, C.c_char_p, P, I, C.POINTER(I64), I]),
    "ldiff_textenc_missing": (I, [P]),
    "ldiff_textenc_missing_name": (C.c_char_p, [P, I]),
    "ldiff_textenc_set_graph": (I, [P, I]),
    "ldiff_textenc_graph_replays": (I64, [P]),
    "ldiff_textenc_graph_nodes": (I64, [P]),
    "ldiff_textenc_forward": (I, [P, C.POINTER(C.c_int32), I, I, I, P, I, P]),
    "ldiff_textenc_check_finite": (I, [P, P]),
    "ldiff_textenc_destroy": (None, [P]),
    "ldiff_op_text_attention": (I, [P, I, I, P, I, I, I, I, I, F, P]),
    "ldiff_vae_create": (I, [C.POINTER(P), C.POINTER(VaeCfg), I]),
    "ldiff_vae_load": (I, [P, C.c_char_p, P, I, C.POINTER(I64), I]),
    "ldiff_vae_set_precision": (I, [P, I, I]),
    "ldiff_vae_set_range_shift": (I, [P, I]),
    "ldiff_vae_set_plan_batch": (I, [P, I]),
    "ldiff_vae_missing": (I, [P]),
    "ldiff_vae_missing_name": (C.c_char_p, [P, I]),
    "ldiff_vae_encode": (I, [P, P, I, I, I, P, P]),
    "ldiff_vae_decode": (I, [P, P, I, I, I, F, P, P, P, P, I, I, P]),
    "ldiff_vae_check_finite": (I, [P, P]),
    "ldiff_vae_destroy": (None, [P]),
    "ldiff_pndm_step": (I, [C.POINTER(F), C.POINTER(P), I, P, I64, P]),
    "ldiff_pndm_alphas_cumprod": (I, [C.POINTER(F), I]),
    "ldiff_pndm_coeffs": (I, [F, F, C.POINTER(F), C.POINTER(F)]),
    "ldiff_laplace_add": (I, [P, F, P, U64, U64, P, I64, P]),
    "ldiff_argmax_u8": (I, [P, I, I, I, I, P, P]),
    "ldiff_confusion": (I, [P, I, P, I, P, P, I, I, I, I, P, P, P]),
    "ldiff_seg_metrics": (I, [C.POINTER(I64), I, C.POINTER(SegMetricsOut)]),
    "ldiff_probe_argmax_u8": (I, [P, I, I, I, I, P, P, F, I, P, P]),
    "ldiff_window_accumulate": (I, [P, P, P, P, I, I, I, I, I, I, I, I, P]),
    "ldiff_luma_float": (I, [P, P, I, I, I, P]),
    "ldiff_bilinear_resize": (I, [P, P, I, I, I, I, I, I, P]),
    "ldiff_op_resize_u8_ws_bytes": (I64, [I, I, I, I, I, I, I]),
    "ldiff_op_resize_u8": (I, [P, I, I, I, I, I, I, P, P, I, P, P, I, P, P, P, I64, P]),
    "ldiff_op_label_table_u8": (I, [P, P, I64, P, P]),
    "ldiff_op_gather_labels": (I, [P, I, I, I, P, I, P, P, P]),
    "ldiff_op_warmup_labels_supported": (I, [I, I, I, I]),
    "ldiff_op_warmup_labels": (I, [P, I, I, I, P, I, I, I, P, P]),
    "ldiff_op_warmup_images": (I, [P, I, I, I, P, I, P, P, P, I, P, P, I, I, I, P, P]),
    "ldiff_pipeline_create": (I, [C.POINTER(P), P, P]),
    "ldiff_pipeline_set_alphas_cumprod": (I, [P, C.POINTER(F), I]),
    "ldiff_pipeline_set_overlap": (I, [P, I]),
    "ldiff_pipeline_join": (I, [P, P]),
    "ldiff_sample": (I, [P, P, I, I, I, I, P, P, P, P]),
    "ldiff_pipeline_check_finite": (I, [P, P]),
    "ldiff_plms_timesteps": (I, [I, C.POINTER(I64), I]),
    "ldiff_pipeline_destroy": (None, [P]),
    "ldiff_op_conv": (I, [C.POINTER(ConvArgs), P]),
    "ldiff_op_conv_pb": (I, [C.POINTER(ConvArgs), I, P]),
    "ldiff_op_conv_stats_blocks": (I, [C.POINTER(ConvArgs)]),
    "ldiff_op_conv_bn_stats_blocks": (I, [C.POINTER(ConvArgs)]),
    "ldiff_op_bn_finalize": (I, [P, I, I, I64, P, P, P, P, P, I64, I64, P]),
    "ldiff_op_bn_apply": (I, [P, I64, I, P, P, P, P, P, I, P, P, P]),
    "ldiff_op_gn_finalize": (I, [P, I, I, P, I, I, I, I, I, F, P, P, P, P, P]),
    "ldiff_op_in_finalize": (I, [P, I, P, I, I, I, I, F, P, P, P, P, I, I, I, P]),
    "ldiff_op_maxpool3x3s2": (I, [P, P, I, I, I, I, P]),
    "ldiff_op_crop_resize_norm": (I, [P, I, I, P, I, P, I, C.POINTER(C.c_double), C.POINTER(C.c_double), P, P]),
    "ldiff_op_cls_head": (I, [P, I, I, I, I, P, P, I, P, P, P]),
    "ldiff_op_cls_head_feat": (I, [P, I, I, I, I, P, P, I, P, P, P, P]),
    "ldiff_op_attention": (I, [P, I, P, I, P, I, P, I, I, I, I, I, I, I64, I64, I64, F, P]),
    "ldiff_op_attention_pb": (I, [P, I, P, I, P, I, P, I, I, I, I, I, I, I64, I64, I64, F, I, P]),
    "ldiff_op_attention_prescaled": (I, [P, I, P, I, P, I, P, I, I, I, I, I, I, I64, I64, I64, P]),
    "ldiff_op_gn_stats": (I, [P, I, I, I, P, I, I, I, I, I, I, F, P, P, P, P, P]),
    "ldiff_op_gn_stats_pb": (I, [P, I, I, I, P, I, I, I, I, I, I, F, P, P, P, P, I, P]),
    "ldiff_op_layernorm": (I, [P, I, I, P, I, I, P, P, F, P]),
    "ldiff_op_ln_linear": (I, [P, I, I, I, I, P, P, F, P, I, I, P, I, P, I, I, F, P]),
    "ldiff_op_norm_apply": (I, [P, I, I, I, P, I, I, I, I, I, P, P, I, P, I, I, P]),
    "ldiff_op_dup_weights": (I, [P, P, I, I, I, I, I, I, P]),
    "ldiff_op_norm_apply_lo8": (I, [P, I, I, I, I, I, P, P, I, P, P]),
    "ldiff_op_lo8_weights": (I, [P, P, P, I, I, I, P]),
    "ldiff_op_geglu": (I, [P, P, I64, I, P]),
    "ldiff_op_nchw_to_nhwc": (I, [P, P, I, I, I, I, I, I, P]),
    "ldiff_op_im2col_t": (I, [P, P, I, I, I, I, I, I, I, I, I, I, I, P]),
    "ldiff_op_transpose": (I, [P, P, I, I, I, I, P]),
    "ldiff_op_colsum": (I, [P, P, I, I, I, P]),
    "ldiff_op_gn_train_fwd": (I, [P, P, P, P, P, P, I, I, I, I, F, I, P]),
    "ldiff_op_gn_train_bwd": (I, [P, P, P, P, P, P, P, P, P, I, I, I, I, I, P]),
    "ldiff_op_ln_bwd": (I, [P, P, P, P, P, P, I, I, F, P]),
    "ldiff_op_geglu_bwd": (I, [P, P, P, I64, I, P]),
    "ldiff_op_silu": (I, [P, P, I64, P]),
    "ldiff_op_silu_bwd": (I, [P, P, P, I64, P]),
    "ldiff_op_attention_bwd": (I, [P, I, P, I, P, I, P, I, P, P, P, I, I, I, I, I, I64, I64, I64, F, P]),
    "ldiff_op_adamw": (I, [P, P, P, P, I64, F, F, F, F, F, I, P]),
    "ldiff_op_pack_weight": (I, [P, P, I, I, I, I, I, I, P]),
    "ldiff_op_unpack_wgrad": (I, [P, P, I, I, I, I, I, P]),
    "ldiff_op_pack_weight_multi": (I, [P, P, I, I, P]),
    "ldiff_op_adamw_multi": (I, [P, P, P, I64, F, F, F, F, F, I, P]),
    "ldiff_op_infonce": (I, [P, I, I, I64, P, P, P, P, I, P, I, F, P, P, P]),
    "ldiff_op_in_train_ws_bytes": (I64, [I, I, I]),
    "ldiff_op_in_train_fwd": (I, [P, P, P, P, P, P, I, I, I, F, F, P, I64, P]),
    "ldiff_op_in_train_bwd": (I, [P, P, P, P, P, P, P, P, P, I, I, I, F, P, I64, P]),
    "ldiff_op_dice_ce_ws_bytes": (I64, [I, I64, I]),
    "ldiff_op_dice_ce": (I, [P, I, I, P, I, I, I64, I, F, F, F, P, P, P, I64, P]),
    "ldiff_op_dice_ce_stats": (I, [P, I, I, P, I, I, I64, I, P, P, I64, P]),
    "ldiff_op_dice_ce_from_sums": (I, [P, I, I, P, I, I, I64, I, F, F, F, P, P, I, P, P, P, I64, P]),
    "ldiff_op_dice_ce_ignore_ws_bytes": (I64, [I, I64, I]),
    "ldiff_op_dice_ce_ignore_nacc": (I, [I]),
    "ldiff_op_dice_ce_ignore": (I, [P, I, I, I, P, I, I, I64, I, F, F, F, P, P, P, I64, P]),
    "ldiff_op_dice_ce_ignore_stats": (I, [P, I, I, I, P, I, I, I64, I, P, P, I64, P]),
    "ldiff_op_dice_ce_ignore_from_sums": (I, [P, I, I, I, P, I, I, I64, I, F, F, F, P, P, P, P, I64, P]),
    "ldiff_op_dice_focal_ws_bytes": (I64, [I, I64, I]),
    "ldiff_op_dice_focal_nacc": (I, [I]),
    "ldiff_op_dice_focal": (I, [P, I, I, P, P, I, I, I, I, I64, I, F, F, F, P, P, P, I64, P]),
    "ldiff_op_dice_focal_stats": (I, [P, I, I, P, P, I, I, I, I, I64, I, P, P, I64, P]),
    "ldiff_op_dice_focal_from_sums": (I, [P, I, I, P, P, I, I, I, I, I64, I, F, F, F, P, P, I, P, P, P, I64, P]),
    "ldiff_op_region_counts_ws_bytes": (I64, [I, I64, I]),
    "ldiff_op_region_counts": (I, [P, I, I, P, P, I, I, I64, F, P, P, I64, P]),
    "ldiff_op_region_mask_u8": (I, [P, I, I, I, I, P, F, P, I, I, I, I, P]),
    "ldiff_op_keep_largest_component_ws_bytes": (I64, [I, I, I]),
    "ldiff_op_keep_largest_component": (I, [P, P, I, I, I, P, I, P, I64, P]),
    "ldiff_op_cc_label": (I, [P, I, I, I, P, P, P, P, I64, P]),
    "ldiff_op_bucket_pack": (I, [P, P, P, I64, P, P]),
    "ldiff_op_sumsq_ws_bytes": (I64, [I64]),
    "ldiff_op_sumsq": (I, [P, I64, P, P, I64, P]),
    "ldiff_op_sgd_nesterov_multi": (I, [P, P, P, I64, F, F, F, I, P, P, P]),
    "ldiff_op_conv_wgrad_ws_bytes": (I64, [I, I, I, I, I, I, I]),
    "ldiff_op_conv_wgrad": (I, [P, P, P, I, I, I, I, I, I, I, I, I, I, I, I, P, I64, P]),
    "ldiff_op_conv_wgrad_wide_ws_bytes": (I64, [I, I, I, I, I, I, I]),
    "ldiff_op_conv_wgrad_wide": (I, [P, P, P, I, I, I, I, I, I, I, I, I, I, I, I, P, I64, P]),
    "ldiff_op_colsum_slabs_ws_bytes": (I64, [I64, I]),
    "ldiff_op_colsum_slabs": (I, [P, P, I64, I, I, P, I64, P]),
    "ldiff_op_seg_sample": (I, [P, I64, P, I, P, I, I, I, I, I, P, P, P]),
    "ldiff_op_seg_intensity_ws_bytes": (I64, [I, I, I, I]),
    "ldiff_op_seg_intensity": (I, [P, P, P, I, I, I, I, P, U64, P, I64, P]),
    "ldiff_op_seg_intensity_lr_ws_bytes": (I64, [I, I, I, I]),
    "ldiff_op_seg_intensity_lr": (I, [P, P, P, I, I, I, I, P, U64, P, I64, P]),
    "ldiff_op_spline_prefilter": (I, [P, I, I, I, I, P]),
    "ldiff_op_case_bbox": (I, [P, I, I, I, I, I64, I64, P, P]),
    "ldiff_op_case_stats_ws_bytes": (I64, [I]),
    "ldiff_op_case_stats": (I, [P, I, I, I, I, I64, I64, I, I, I, I, P, P, I64, P]),
    "ldiff_op_case_counts": (I, [P, I, I, I64, I, I, I, I, I, P, P, P, P]),
    "ldiff_op_case_counts_classes": (I, [P, I, I, I64, I, I, I, I, I, I, P, P, P, P]),
    "ldiff_op_case_apply": (I, [P, I, I, I, I, I64, I64, P, I64, I, I, I, I, C.POINTER(F), C.POINTER(F), P, I64, C.POINTER(SegCase), I, P]),
    "ldiff_op_case_rank_to_coord": (I, [P, I, I, I64, I, I, I, I, I, P, P, I64, P, P, I, I, I64, I64, P, P]),
    "ldiff_op_window_gather": (I, [P, I, I, I, I64, I64, I, I, I, I, C.POINTER(WindowTiles), I, I, P, P]),
    "ldiff_op_window_accumulate_batch": (I, [P, P, P, P, I, I, I, I, I, C.POINTER(WindowTiles), I, P]),
    "ldiff_op_window_finish": (I, [P, P, I, I, I, I, I, I, I, I, P, P, I, I, I, I, P, P]),
    "ldiff_op_window_finish_ensemble": (I, [C.POINTER(P), I, P, I, I, I, I, I, I, I, I, P, P, I, I, I, I, P, P]),
    "ldiff_stream_create_cu_share": (I, [I, I, P]),
    "ldiff_stream_destroy": (I, [P]),
    "ldiff_vae_set_side_cu_share": (I, [P, I, I]),
    "ldiff_prof_enable": (I, [I]),
    "ldiff_prof_set_filter": (I, [C.c_char_p]),
    "ldiff_prof_collect": (I, [P, I]),
}


class ProfRow(C.Structure):
    _fields_ = [("name", C.c_char * 64), ("launches", C.c_int64), ("ms", C.c_double), ("flops", C.c_double), ("bytes", C.c_double)]


def prof_collect():
    """Rows of the live HIP-event profile: list of dict(name, launches, ms, flops, bytes)."""
    lib = load()
    rows = (ProfRow * 128)()
    n = lib.ldiff_prof_collect(C.cast(rows, C.c_void_p), 128)
    check(n if n < 0 else 0)
    return [dict(name=r.name.decode(), launches=r.launches, ms=r.ms, flops=r.flops, bytes=r.bytes) for r in rows[:min(n, 128)]]

_lib = None


def load() -> C.CDLL:
    """Load the HIP library (once).  Raises RuntimeError with a build hint when it is absent."""
    global _lib
    if _lib is not None:
        return _lib
    # torch first: it ships its own HIP runtime, and the library must bind to THAT copy -- loaded before torch, libldiff_hip.so pulls in
    # /opt/rocm's libamdhip64 and the process ends up with two runtimes, of which ours sees no device (seen as "no ROCm-capable device is
    # detected" from ldiff_vae_create when build() and smoke() ran in one process)
    import torch  # noqa: F401
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} not found: the gfx950 HIP extension is not built. Run `python -c \"import __graft_entry__ as g; g.build()\"` "
            "at the repo root (needs hipcc). There is no CPU fallback.")
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if the symbol is missing: fail loudly
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


class NonFiniteError(RuntimeError):
    """LDIFF_ERR_NONFINITE: an activation left fp16's range (or turned NaN) somewhere in a graph; the call's results are invalid
    (include/ldiff.h, "Non-finite detection")."""


def check(rc: int) -> None:
    """Map ldiff_status to the exceptions the reference raises: bad shapes -> ValueError, else RuntimeError."""
    if rc == 0:
        return
    msg = load().ldiff_last_error().decode("utf-8", "replace")
    if rc == -1:
        raise ValueError(msg)
    if rc == -4:
        raise NonFiniteError(f"ldiff error {rc}: {msg}")
    raise RuntimeError(f"ldiff error {rc}: {msg}")


def require_gpu():
    import torch
    if not torch.cuda.is_available():
        raise RuntimeError("ldiffusion_amd needs a ROCm GPU (gfx950); torch.cuda.is_available() is False and there is no CPU fallback")


def stream_ptr():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)
