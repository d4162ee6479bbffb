"""ctypes binding of libeavsr_hip.so (the C ABI declared in include/eavsr_hip.h).

There is no CPU path and no PyTorch fallback: if the shared object is missing or an entry
point is absent, the first use raises.  Build it with ``python -m eavsr_amd.build`` (or
``__graft_entry__.build()``).
"""
from __future__ import annotations

import ctypes as C
import os
import threading

_HERE = os.path.dirname(os.path.abspath(__file__))
# EAVSR_LIB_PATH: A/B builds of the same ABI (the lab flavour eavsr_amd/lib/libeavsr_lab.so among them; EAVSR_BUILD_LAB=1 picks that one)
LIB_PATH = os.environ.get("EAVSR_LIB_PATH") or os.path.join(
    _HERE, "lib", "libeavsr_lab.so" if os.environ.get("EAVSR_BUILD_LAB", "0") == "1" else "libeavsr_hip.so")

ABI_VERSION = 32
WARP_PAIR_BORDER = 0x10      # EAVSR_WARP_PAIR_BORDER: or-ed into outb_il8 of eavsr_flow_warp_pair_f32 (border padding)

p_f32 = C.c_void_p  # device pointers travel as integers
i32 = C.c_int32
i64 = C.c_int64
f32 = C.c_float
vp = C.c_void_p


class ConvDesc(C.Structure):
    """struct eavsr_conv2d_desc"""
    _fields_ = [
        ("src", vp * 5),
        ("src_c", i32 * 5),
        ("n_src", i32),
        ("ksize", i32),
        ("weight_packed", vp),
        ("bias", vp),
        ("residual", vp),
        ("out", vp),
        ("chan_partial", vp),
        ("n", i32), ("h", i32), ("w", i32), ("cin", i32), ("cout", i32),
        ("act", i32),
        ("slope", f32),
        ("ca_scale", vp),
        ("ca_x", vp),
        ("ca_out", vp),
        ("out_shuffle", i32),
        ("res_scale", vp),
        ("border_pieces", vp),
        ("border_stride", i32),
        ("sum_mul", vp),
    ]


# name -> (restype, argtypes); every symbol include/eavsr_hip.h declares
SIGNATURES = {
    "eavsr_abi_version": (C.c_int, []),
    "eavsr_version": (C.c_char_p, []),
    "eavsr_conv2d_desc_size": (C.c_size_t, []),
    "eavsr_lab_build": (C.c_int, []),
    "eavsr_last_error": (C.c_char_p, []),
    "eavsr_selftest_mfma_f32": (C.c_int, [vp, vp]),
    "eavsr_flow_warp_f32": (C.c_int, [vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, vp]),
    "eavsr_flow_warp_pair_f32": (C.c_int, [vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, vp]),
    "eavsr_flow_warp_single_f32": (C.c_int, [vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, vp]),
    "eavsr_dcnv2_f32": (C.c_int, [vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, vp]),
    "eavsr_dcnv2_generic_f32": (C.c_int, [vp] * 6 + [i32] * 15 + [vp]),
    "eavsr_dcn_weight_x9_bytes": (C.c_int64, [i32, i32]),
    "eavsr_pack_dcn_weight_x9": (C.c_int, [vp, vp, i32, i32, vp]),
    "eavsr_nchw_to_il8_f32": (C.c_int, [vp, vp, i32, i32, i32, i32, vp]),
    "eavsr_dcnv2_il_f32": (C.c_int, [vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, i32, vp]),
    "eavsr_dcn_weight_il2_bytes": (C.c_int64, [i32, i32]),
    "eavsr_pack_dcn_weight_il2": (C.c_int, [vp, vp, i32, i32, vp]),
    "eavsr_dcnv2_il2_f32": (C.c_int, [vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, i32, vp]),
    "eavsr_dcn_il16_weight_bytes": (C.c_int64, [i32, i32]),
    "eavsr_pack_dcn_il16_weight": (C.c_int, [vp, vp, i32, i32, i32, vp]),
    "eavsr_nchw_to_il8_h16": (C.c_int, [vp, vp, i32, i32, i32, i32, i32, vp]),
    "eavsr_dcnv2_il16": (C.c_int, [vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, i32, vp]),
    "eavsr_wino4_schedule": (C.c_int, []),
    "eavsr_conv3x3_wino4_border_pieces": (C.c_int, [i32, i32, C.POINTER(i32), C.POINTER(i32)]),
    "eavsr_ca_scale_pre_pieces": (C.c_int, [vp, vp, i32, vp, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, vp]),
    "eavsr_conv2d_f32": (C.c_int, [C.POINTER(ConvDesc), vp]),
    "eavsr_wino4_weight_elems": (C.c_int64, [i32, i32]),
    "eavsr_pack_conv_weight_wino4": (C.c_int, [vp, vp, i32, i32, vp]),
    "eavsr_conv3x3_wino4_tiles": (i32, [i32, i32]),
    "eavsr_conv3x3_wino4_f32": (C.c_int, [vp, vp, vp]),
    "eavsr_wgrad3_mode": (C.c_int, []),
    "eavsr_conv3x3_x6s_tiles": (i32, [i32, i32]),
    "eavsr_conv3x3_f32x6s": (C.c_int, [vp, vp, vp]),
    "eavsr_pack_conv_weight_wino5x5": (C.c_int, [vp, vp, i32, i32, vp]),
    "eavsr_conv5x5_wino_tiles": (i32, [i32, i32]),
    "eavsr_conv5x5_wino_f32": (C.c_int, [vp, vp, vp]),
    "eavsr_conv2d_ck": (i32, [i32]),
    "eavsr_conv2d_tile_rows": (i32, [i32, i32, i32, i32]),
    "eavsr_conv2d_tiles": (i32, [i32, i32, i32, i32]),
    "eavsr_route_batch": (i32, [i32]),
    "eavsr_packed_weight_elems": (i64, [i32, i32, i32]),
    "eavsr_pack_conv_weight_f32": (C.c_int, [vp, vp, i32, i32, i32, vp]),
    "eavsr_conv3x3_smallco_f32": (C.c_int, [vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, f32, vp]),
    "eavsr_smallco_packed_elems": (C.c_int64, [i32, i32]),
    "eavsr_pack_smallco_weight": (C.c_int, [vp, vp, i32, i32, vp]),
    "eavsr_conv3x3_smallco_lite_f32": (C.c_int, [vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, f32, vp]),
    "eavsr_conv_weight_x6_bytes": (C.c_size_t, [i32, i32, i32]),
    "eavsr_pack_conv_weight_x6": (C.c_int, [vp, vp, i32, i32, i32, vp]),
    "eavsr_pack_conv_weight_x6_dgrad": (C.c_int, [vp, vp, i32, i32, i32, vp]),
    "eavsr_pack_conv_weight_x6_multi": (C.c_int, [vp, vp, vp, i32, i32, i32, vp]),
    "eavsr_conv_f32x6_tiles_per_workgroup": (i32, [i32, i32, i32, i32, i32, i32]),
    "eavsr_conv_f32x6": (C.c_int, [vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, f32, i32, vp]),
    "eavsr_ca_scale_f32": (C.c_int, [vp, i32, i32, vp, vp, vp, vp, vp, i32, i32, i32, vp]),
    "eavsr_ca_scale_mean_f32": (C.c_int, [vp, i32, i32, vp, vp, vp, vp, vp, vp, i32, i32, i32, vp]),
    "eavsr_scale_residual_f32": (C.c_int, [vp, vp, vp, vp, i32, i32, i32, vp]),
    "eavsr_ca_tail_f32": (C.c_int, [vp, vp, i32, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, vp]),
    "eavsr_ca_tail_stats_f32": (C.c_int, [vp, vp, i32, vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, vp]),
    "eavsr_adapt_frontend_f32": (C.c_int, [vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, vp]),
    "eavsr_affine_offsets_f32": (C.c_int, [vp, vp, vp, i32, i32, i32, i32, vp]),
    "eavsr_resize_bilinear_ac_f32": (C.c_int, [vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, f32, vp]),
    "eavsr_pyramid_f32": (C.c_int, [vp, vp, vp, i32, i32, i32, vp]),
    "eavsr_add_f32": (C.c_int, [vp, vp, vp, vp, i64, vp]),
    "eavsr_normalize_f32": (C.c_int, [vp, vp, vp, vp, i32, i32, i32, vp]),
    "eavsr_avg_pool2_f32": (C.c_int, [vp, vp, i32, i32, i32, vp]),
    "eavsr_resize_bilinear_f32": (C.c_int, [vp, vp, i32, i32, i32, i32, i32, i32, i32, f32, f32, vp]),
    "eavsr_concat3_f32": (C.c_int, [vp, i32, vp, i32, vp, i32, vp, i32, i32, vp]),
    # backward entry points
    "eavsr_act_bwd_f32": (C.c_int, [vp, vp, vp, i64, i32, f32, vp]),
    "eavsr_plane_sum_f32": (C.c_int, [vp, vp, vp, i32, i32, f32, vp]),
    "eavsr_channel_sum_f32": (C.c_int, [vp, vp, i32, i32, i32, i32, vp]),
    "eavsr_channel_sum_multi_f32": (C.c_int, [vp, i32, vp, i32, i32, i32, i32, vp]),
    "eavsr_scale_residual_bwd_f32": (C.c_int, [vp, vp, vp, vp, i32, i32, i32, vp]),
    "eavsr_rcab_tail_bwd_f32": (C.c_int, [vp] * 13 + [i32] * 7 + [vp]),
    "eavsr_ca_mlp_bwd_f32": (C.c_int, [vp] * 11 + [i32, i32, i32, vp]),
    "eavsr_flow_warp_bwd_f32": (C.c_int, [vp] * 6 + [i32, i32, i32, i32, vp]),
    "eavsr_resize_bilinear_ac_bwd_f32": (C.c_int, [vp, vp, i32, i32, i32, i32, i32, i32, f32, vp]),
    "eavsr_pyramid_bwd_f32": (C.c_int, [vp, vp, vp, i32, i32, i32, vp]),
    "eavsr_affine_offsets_bwd_f32": (C.c_int, [vp, vp, vp, vp, i32, i32, i32, i32, vp]),
    "eavsr_conv_wgrad_blocks": (i32, [i32, i32, i32, i32]),
    "eavsr_conv_wgrad_f32": (C.c_int, [vp, vp, vp, vp] + [i32] * 11 + [vp]),
    "eavsr_conv_wgrad_multi_f32": (C.c_int, [vp, vp, i32, vp, vp] + [i32] * 11 + [vp]),
    "eavsr_conv_wgrad_span_f32": (C.c_int, [vp, vp, vp, vp] + [i32] * 9 + [vp]),
    "eavsr_conv_wgrad_bias_multi_f32": (C.c_int, [vp, vp, i32, vp, vp, vp] + [i32] * 11 + [vp]),
    "eavsr_dcnv2_bwd_grid": (i32, [i32, i32, i32]),
    "eavsr_dcnv2_bwd_workspace_floats": (C.c_int64, [i32, i32, i32]),
    "eavsr_dcnv2_bwd_f32": (C.c_int, [vp] * 10 + [i32] * 7 + [vp]),
    "eavsr_il8_to_nchw_f32": (C.c_int, [vp, vp, i32, i32, i32, i32, vp]),
    "eavsr_dcnv2_im2col_f32": (C.c_int, [vp, vp, vp, vp, i32, i32, i32, i32, i32, vp]),
    "eavsr_dcnv2_col2im_f32": (C.c_int, [vp] * 7 + [i32, i32, i32, i32, i32, vp]),
    "eavsr_gconv3x3_fwd_f32": (C.c_int, [vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, f32, vp]),
    "eavsr_gconv3x3_bwd_f32": (C.c_int, [vp] * 6 + [i32, i32, i32, i32, i32, vp]),
    "eavsr_gconv3x3_bwd_acc_f32": (C.c_int, [vp] * 6 + [i32, i32, i32, i32, i32, i32, vp]),
    # 16-bit backbone
    "eavsr_conv_h16_tiles": (i32, [i32, i32]),
    "eavsr_pack_conv3x3_c64_h16": (C.c_int, [vp, vp, i32, vp]),
    "eavsr_conv5x5_c64_h16_weight_bytes": (C.c_int64, []),
    "eavsr_pack_conv5x5_c64_h16": (C.c_int, [vp, vp, i32, i32, vp]),
    "eavsr_conv5x5_c64_h16": (C.c_int, [vp, vp, vp, vp, i32, i32, i32, i32, i32, vp]),
    "eavsr_conv_h16_partial_rows": (i32, [i32, i32, i32]),
    "eavsr_conv3x3_c64_h16": (C.c_int, [vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, vp]),
    "eavsr_conv3x3_c64_h16_res": (C.c_int, [vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, vp]),
    "eavsr_ca_scale_pre_f32": (C.c_int, [vp] * 11 + [i32, i32, i32, i32, vp]),
    "eavsr_ca_scale_pre_ws_floats": (C.c_int64, [i32]),
    "eavsr_ca_scale_pre_h16": (C.c_int, [vp] * 11 + [i32, i32, i32, i32, i32, vp]),
    "eavsr_conv_h16_border_pieces": (C.c_int, [i32, i32, C.POINTER(i32), C.POINTER(i32)]),
    "eavsr_conv3x3_c64_h16_b": (C.c_int, [vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, vp]),
    "eavsr_conv3x3_c64_h16_act": (C.c_int, [vp, vp, vp, vp, i32, i32, i32, i32, f32, i32, i32, vp]),
    "eavsr_conv3x3_c64to3_h16": (C.c_int, [vp, vp, vp, vp, vp, i32, i32, i32, i32, vp]),
    "eavsr_conv3x3_h16g_weight_bytes": (C.c_int64, [i32, i32]),
    "eavsr_pack_conv3x3_h16g": (C.c_int, [vp, vp, i32, i32, i32, vp]),
    "eavsr_conv3x3_h16g_f32": (C.c_int, [vp, i32, vp]),
    "eavsr_conv_weight_h16x1_bytes": (C.c_size_t, [i32, i32, i32]),
    "eavsr_pack_conv_weight_h16x1": (C.c_int, [vp, vp, i32, i32, i32, i32, vp]),
    "eavsr_conv_h16x1": (C.c_int, [vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, f32, i32, vp]),
    "eavsr_nchw_f32_to_nhwc_h16": (C.c_int, [vp, vp, i32, i32, i32, i32, vp]),
    "eavsr_nhwc_h16_to_nchw_f32": (C.c_int, [vp, vp, vp, i32, i32, i32, i32, vp]),
    "eavsr_scale_residual_h16": (C.c_int, [vp, vp, vp, vp, i32, i32, i32, i32, vp]),
    # PWC-Net of the late-training validity mask (ABI 31)
    "eavsr_pwc_conv3x3_weight_elems": (C.c_int64, [i32, i32]),
    "eavsr_pwc_pack_conv3x3_f32": (C.c_int, [vp, vp, i32, i32, vp]),
    "eavsr_pwc_conv3x3_f32": (C.c_int, [vp, i64, vp, vp, vp, i64] + [i32] * 8 + [f32, vp]),
    "eavsr_pwc_deconv4x4s2_f32": (C.c_int, [vp, i64, vp, vp, vp, i64, i32, i32, i32, i32, vp]),
    "eavsr_pwc_correlation_f32": (C.c_int, [vp, i64, vp, i64, vp, i64, i32, i32, i32, i32, vp]),
    "eavsr_pwc_backwarp_f32": (C.c_int, [vp, i64, vp, i64, vp, i64, vp] + [i32] * 6 + [f32, vp]),
    # the opt-in bf16 training mode (ABI 32)
    "eavsr_conv_weight_bf16x1_bytes": (C.c_size_t, [i32, i32, i32]),
    "eavsr_pack_conv_weight_bf16x1": (C.c_int, [vp, vp, i32, i32, i32, vp]),
    "eavsr_pack_conv_weight_bf16x1_dgrad": (C.c_int, [vp, vp, i32, i32, i32, vp]),
    "eavsr_pack_conv_weight_bf16x1_multi": (C.c_int, [vp, vp, vp, i32, i32, i32, vp]),
    "eavsr_conv3x3_bf16x1s": (C.c_int, [vp, vp, vp]),
    "eavsr_conv_wgrad_bias_multi_bf16": (C.c_int, [vp, vp, i32, vp, vp, vp] + [i32] * 11 + [vp]),
    # the opt-in deterministic training mode (csrc/det_scatter.hip; additions to ABI 32)
    "eavsr_resize_bilinear_ac_bwd_det_f32": (C.c_int, [vp, vp, i32, i32, i32, i32, i32, i32, f32, vp]),
    "eavsr_flow_warp_bwd_dx_det_workspace_floats": (C.c_int64, [i32, i32, i32]),
    "eavsr_flow_warp_bwd_dx_det_f32": (C.c_int, [vp] * 5 + [i32] * 4 + [vp]),
    "eavsr_dcnv2_col2im_dx_det_workspace_floats": (C.c_int64, [i32, i32, i32]),
    "eavsr_dcnv2_col2im_dx_det_f32": (C.c_int, [vp] * 5 + [i32] * 5 + [vp]),
    # per-frame PSNR / SSIM and the 8-bit frame (csrc/metrics.hip; additions to ABI 32)
    "eavsr_frame_metrics_partials": (i32, [i32, i32, i32, i32]),
    "eavsr_frame_metrics_f32": (C.c_int, [vp, vp, f32, i32, i32, i32, i32, vp, vp, vp, vp, vp]),
    "eavsr_rgb8_f32": (C.c_int, [vp, f32, i32, i32, i32, i32, vp, vp]),
    # temporal consistency of the report: warping error and tOF (csrc/temporal.hip; additions to ABI 32)
    "eavsr_temporal_metrics_partials": (i32, [i32, i32, i32, i32]),
    "eavsr_temporal_metrics_f32": (C.c_int, [vp, vp, vp, vp, f32, i32, i32, i32, i32, vp, vp, vp, vp, vp]),
    # NIQE, the report's no-reference column: block moments and the antialiased half-size resize (csrc/niqe.hip; additions to ABI 32)
    "eavsr_niqe_moments": (C.c_int, [vp, i32, f32] + [i32] * 9 + [C.POINTER(C.c_double), vp, vp, vp]),
    "eavsr_niqe_half_f64": (C.c_int, [vp, vp, vp, vp, i32, vp, vp, i32, vp, i32] + [i32] * 5 + [vp]),
    "eavsr_u8_to_f32": (C.c_int, [vp, vp, i32, i32, i32, i32, i32, vp]),
    # padded ingest of frames of any size, and of a window of them: one kernel family (csrc/ingest_pad.hip; additions to ABI 32)
    "eavsr_ingest_pad": (C.c_int, [vp, vp] + [i32] * 8 + [vp]),
    "eavsr_ingest_window": (C.c_int, [vp, vp] + [i32] * 12 + [vp]),
    # spatial tiling: weighted accumulation of SR tiles (csrc/blend.hip; addition to ABI 32)
    "eavsr_tile_blend_f32": (C.c_int, [vp] * 4 + [i32] * 9 + [i64] * 4 + [vp]),
    # self-ensemble inference: flips / transposes of LR frames, their inverses into the accumulator (csrc/blend.hip; additions to ABI 32)
    "eavsr_dihedral_f32": (C.c_int, [vp, vp] + [i32] * 5 + [vp]),
    "eavsr_blend_dihedral_f32": (C.c_int, [vp] * 4 + [i32] * 10 + [i64] * 4 + [vp]),
    # the 16-bit feature cache of the long-clip path: fp32 <-> fp16 / bf16 over a list of segments (csrc/cache16.hip; additions to ABI 32)
    "eavsr_cache16_max_segments": (C.c_int, []),
    "eavsr_pack16": (C.c_int, [vp, vp, vp, i32, i32, vp]),
    "eavsr_unpack16": (C.c_int, [vp, vp, vp, i32, i32, vp]),
    "eavsr_pack16_census": (C.c_int, [vp, vp, vp, i32, i32, vp, vp]),      # pack16 + the five counts of what the rounding did
    # the range census of the 16-bit backbone modes: stored words / fp32 values as rounded (csrc/range16.hip; additions to ABI 32)
    "eavsr_range16_words": (C.c_int, [vp, vp, i32, i32, vp, vp]),
    "eavsr_range16_as_rounded": (C.c_int, [vp, vp, i32, i32, vp, vp]),
    "eavsr_range16_stamp": (C.c_int, [vp, vp, C.c_uint64, vp]),
    # training batches from device-resident 8-bit frames (csrc/batch.hip; addition to ABI 32)
    "eavsr_gather_pairs_u8": (C.c_int, [vp] * 6 + [i32] * 9 + [vp]),
    # LR frames from full-size frames: cv2.resize INTER_CUBIC on bytes (csrc/resize_cubic.hip; addition to ABI 32)
    "eavsr_resize_cubic_u8": (C.c_int, [vp] * 6 + [i32] * 6 + [vp]),
    # the outgoing PNG file: scanline filters and a Huffman-only deflate coder (csrc/png.hip; additions to ABI 32)
    "eavsr_png_filter_u8": (C.c_int, [vp, vp, i32, i32, i32, i32, vp]),
    "eavsr_png_capacity": (C.c_int64, [i64, i64]),
    "eavsr_deflate_workspace_bytes": (C.c_int64, [i32, i64, i64]),
    "eavsr_deflate_huffman_u8": (C.c_int, [vp] * 5 + [i32, i64, i64, vp]),
    # the incoming PNG file: the scanline unfilter (csrc/png_decode.hip; addition to ABI 32)
    "eavsr_png_unfilter_u8": (C.c_int, [vp, vp, i32, i32, i32, i32, i32, vp]),
    # scene-cut statistics of 8-bit frames: luma histogram and frame-to-frame SAD (csrc/scene.hip; addition to ABI 32)
    "eavsr_frame_change_u8": (C.c_int, [vp, vp, vp, i32, i32, i32, i32, i32, vp]),
    # LPIPS (AlexNet), the report's third column (csrc/lpips.hip; additions to ABI 32)
    "eavsr_lpips_conv_weight_elems": (C.c_int64, [i32, i32, i32]),
    "eavsr_lpips_pack_conv_f32": (C.c_int, [vp, vp, i32, i32, i32, vp]),
    "eavsr_lpips_conv1_f32": (C.c_int, [vp, vp, f32, vp, vp, vp, vp, vp, i32, i32, i32, i32, vp]),
    "eavsr_lpips_conv_f32": (C.c_int, [vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, vp]),
    "eavsr_lpips_maxpool3s2_f32": (C.c_int, [vp, vp, i64, i32, i32, vp]),
    "eavsr_lpips_tap_partials": (i32, [i32, i32]),
    "eavsr_lpips_tap_f32": (C.c_int, [vp, vp, vp, vp, i32, i32, i32, i32, i32, vp]),
    # output at any target size: the antialiased bicubic resize of fp32 frames (csrc/resize_aa.hip; addition to ABI 32)
    "eavsr_resize_aa_f32": (C.c_int, [vp, i64, i64, i64, i32, i32, i32, i32, vp, vp, i32, vp, vp, i32, vp, vp, i32, i32, vp]),
}

# Entry points of the LAB build only (`python -m eavsr_amd.build --lab`; the header's EXPERIMENTAL section): bound when the
# library exports them, absent from a default build (ops raises LabBuildRequired for the modes that need them).
LAB_SIGNATURES = {
    "eavsr_conv3x3_f32x9": (C.c_int, [vp, vp, vp]),
    "eavsr_dcnv2_f32x9": (C.c_int, [vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, vp]),
    "eavsr_dcnv2_ws_f32": (C.c_int, [vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, i32, vp]),
    "eavsr_wino_weight_elems": (C.c_int64, [i32, i32]),
    "eavsr_pack_conv_weight_wino": (C.c_int, [vp, vp, i32, i32, vp]),
    "eavsr_conv3x3_wino_tiles": (i32, [i32, i32]),
    "eavsr_conv3x3_wino_f32": (C.c_int, [vp, vp, vp]),
    "eavsr_flow_level_f32": (C.c_int, [vp] * 11 + [i32, i32, i32, i32, vp]),
    "eavsr_rcab_h16_partial_rows": (i32, [i32, i32, i32]),
    "eavsr_rcab_convs_h16": (C.c_int, [vp] * 7 + [i32] * 4 + [vp]),
}

_lock = threading.Lock()
_lib = None


class NativeLibraryError(RuntimeError):
    pass


def load():
    """Load (once) and return the ctypes library with typed entry points."""
    global _lib
    if _lib is not None:
        return _lib
    with _lock:
        if _lib is not None:
            return _lib
        if not os.path.exists(LIB_PATH):
            raise NativeLibraryError(
                f"{LIB_PATH} is missing: the HIP extension has not been built "
                "(run `python -m eavsr_amd.build`). eavsr_amd has no CPU or PyTorch fallback.")
        try:
            lib = C.CDLL(LIB_PATH)
        except OSError as e:  # e.g. libamdhip64 not found
            raise NativeLibraryError(f"cannot load {LIB_PATH}: {e}") from e
        for name, (res, args) in SIGNATURES.items():
            try:
                fn = getattr(lib, name)
            except AttributeError as e:
                raise NativeLibraryError(f"{LIB_PATH} does not export {name}") from e
            fn.restype = res
            fn.argtypes = args
        if lib.eavsr_abi_version() != ABI_VERSION:
            raise NativeLibraryError(
                f"ABI mismatch: library {lib.eavsr_abi_version()} vs binding {ABI_VERSION}; rebuild")
        if lib.eavsr_conv2d_desc_size() != C.sizeof(ConvDesc):      # a descriptor that grew without an ABI bump
            raise NativeLibraryError(
                f"struct eavsr_conv2d_desc: library {lib.eavsr_conv2d_desc_size()} bytes vs binding {C.sizeof(ConvDesc)}; rebuild")
        if lib.eavsr_lab_build():
            for name, (res, args) in LAB_SIGNATURES.items():
                try:
                    fn = getattr(lib, name)
                except AttributeError as e:
                    raise NativeLibraryError(f"{LIB_PATH} says it is a lab build but does not export {name}") from e
                fn.restype = res
                fn.argtypes = args
        _lib = lib
    return _lib


def lab_build() -> bool:
    """True when the loaded library is the lab build (the retired schedules are there)"""
    return bool(load().eavsr_lab_build())


def check(code: int, what: str):
    if code != 0:
        msg = load().eavsr_last_error().decode(errors="replace")
        kind = "argument error" if code < 0 else "hipError"
        raise RuntimeError(f"{what} failed ({kind} {code}): {msg}")
