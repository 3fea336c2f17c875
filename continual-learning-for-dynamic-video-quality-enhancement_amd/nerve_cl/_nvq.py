"""ctypes binding of libnvq.so (include/nvq.h).

This is the only place that touches the C ABI.  There is no CPU or PyTorch fallback:
if the shared library is missing, or a tensor is not a contiguous fp32 HIP tensor, the
call raises.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Dict, Optional, Sequence

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("NVQ_LIB", os.path.join(os.path.dirname(_HERE), "libnvq.so"))

MATH_F32 = 0
MATH_BF16 = 1
MAX_T = 8

_lib = None

vp, ci, cl, cf, sz = C.c_void_p, C.c_int, C.c_long, C.c_float, C.c_size_t


class ConvDesc(C.Structure):
    _fields_ = [
        ("inp", vp), ("in_ld", ci), ("in_coff", ci), ("cin", ci),
        ("wpack", vp),
        ("bias", vp),
        ("out", vp), ("out_ld", ci), ("out_coff", ci), ("cout", ci),
        ("cout_store", ci),
        ("out2", vp), ("out2_ld", ci), ("out2_coff", ci),
        ("res", vp), ("res_ld", ci), ("res_coff", ci), ("res_cmax", ci),
        ("mask", vp), ("mask_ld", ci), ("mask_coff", ci), ("mask_c0", ci), ("mask_c1", ci),
        ("n", ci), ("h", ci), ("w", ci),
        ("ksize", ci),
        ("relu", ci),
        ("alpha", cf),
        ("accumulate", ci),
        ("math", ci),
        ("in_bf16", ci), ("out_bf16", ci), ("out2_bf16", ci), ("res_bf16", ci), ("mask_bf16", ci),
        ("bits", vp), ("bits_mode", ci), ("center_cin", ci), ("in_plane", C.c_uint),
        ("tile_rows", ci), ("bits_words", ci),
    ]


class DwEpilogue(C.Structure):
    _fields_ = [("add", vp), ("add_ld", ci), ("mask", vp), ("mask_ld", ci), ("mask_bf16", ci), ("add_bf16", ci)]


class CorrAddends(C.Structure):
    _fields_ = [("a", vp), ("a_ld", ci), ("a_coff", ci), ("b", vp), ("b_ld", ci), ("b_coff", ci)]


class BnInput(C.Structure):
    _fields_ = [("mean", vp), ("invstd", vp), ("gamma", vp), ("beta", vp), ("group_images", ci)]


class WgradDesc(C.Structure):
    _fields_ = [
        ("x", vp), ("x_ld", ci), ("x_coff", ci), ("cin", ci), ("cin_w", ci),
        ("dy", vp), ("dy_ld", ci), ("dy_coff", ci), ("cout", ci),
        ("dw", vp), ("dbias", vp),
        ("workspace", vp), ("workspace_bytes", sz),
        ("n", ci), ("h", ci), ("w", ci), ("ksize", ci),
        ("alpha", cf), ("accumulate", ci), ("math", ci),
        ("x_bf16", ci), ("dy_bf16", ci), ("x_plane", C.c_uint), ("variant", ci),
    ]


class WgradReduceJob(C.Structure):
    _fields_ = [
        ("part", vp), ("bias_part", vp), ("dw", vp), ("dbias", vp),
        ("nsplit", ci), ("nci", ci), ("nco", ci), ("taps", ci), ("cout", ci), ("cin_w", ci),
        ("alpha", cf), ("accumulate", ci),
    ]


LAYOUT_MAX_JOBS = 2 * MAX_T + 1
INJECT_MAX_SRC = 4


class GatherJob(C.Structure):
    _fields_ = [("src", vp), ("src_ld", ci), ("src_coff", ci), ("src_bf16", ci), ("dst", vp)]


class InjectJob(C.Structure):
    _fields_ = [("dst", vp), ("dst_ld", ci), ("dst_coff", ci), ("dst_bf16", ci), ("src", vp * INJECT_MAX_SRC)]


_IP = C.POINTER(ci)

# name -> (restype, argtypes); must list every symbol declared in include/nvq.h
SIGNATURES = {
    "nvq_version": (ci, []),
    "nvq_last_error": (C.c_char_p, []),
    "nvq_conv_pack_floats": (sz, [ci, ci, ci, ci]),
    "nvq_conv_pack": (ci, [vp, ci, ci, ci, ci, ci, ci, ci, vp, vp]),
    "nvq_conv_forward": (ci, [C.POINTER(ConvDesc), vp]),
    "nvq_rdb_tail_forward": (ci, [C.POINTER(ConvDesc), C.POINTER(ConvDesc), vp]),
    "nvq_rdb_backward_weights_floats": (sz, [ci]),
    "nvq_rdb_backward_weights": (ci, [vp, vp, vp, vp, vp, vp, ci, vp, vp]),
    "nvq_sizeof_conv_desc": (sz, []),
    "nvq_wgrad_workspace_bytes": (sz, []),
    "nvq_conv_wgrad": (ci, [C.POINTER(WgradDesc), vp]),
    "nvq_conv_wgrad_partial": (ci, [C.POINTER(WgradDesc), C.POINTER(WgradReduceJob), vp]),
    "nvq_wgrad_reduce_batch": (ci, [C.POINTER(WgradReduceJob), ci, vp]),
    "nvq_sizeof_wgrad_desc": (sz, []),
    "nvq_sizeof_wgrad_reduce_job": (sz, []),
    "nvq_conv_pack_batch": (ci, [vp, ci, ci, vp]),
    "nvq_head_forward": (ci, [vp, ci, ci, ci, ci, ci, _IP, ci, vp, vp, ci, vp, ci, ci, vp, ci, vp]),
    "nvq_head_wgrad": (ci, [vp, ci, ci, ci, ci, ci, _IP, ci, vp, ci, vp, ci, vp, ci, ci, vp, vp, vp, sz, ci, ci, vp]),
    "nvq_dwconv_forward": (ci, [vp, ci, vp, ci, vp, ci, ci, ci, ci, ci, ci, ci, vp, vp, vp]),
    "nvq_dwconv_wgrad": (ci, [vp, ci, vp, ci, ci, ci, ci, ci, vp, vp, sz, ci, ci, ci, vp, vp]),
    "nvq_bn_stats": (ci, [vp, ci, ci, ci, ci, ci, ci, cf, cf, _IP, vp, vp, vp, vp, vp, sz, ci, vp]),
    "nvq_bn_eval_stats": (ci, [vp, vp, ci, ci, cf, vp, vp, vp]),
    "nvq_bn_apply_relu": (ci, [vp, ci, ci, ci, ci, ci, ci, vp, vp, vp, vp, vp, ci, vp, ci, ci, ci, vp, ci, ci, ci, ci, ci, vp]),
    "nvq_bn_relu_backward": (ci, [vp, ci, vp, ci, ci, ci, ci, ci, ci, vp, vp, vp, vp, ci, vp, ci, vp, vp, vp, sz, ci, ci, ci, ci, vp]),
    "nvq_dwconv_backward": (ci, [vp, ci, vp, vp, ci, vp, vp, ci, vp, ci, ci, ci, vp, vp, vp, vp, vp, sz, vp]),
    "nvq_dwconv_backward_ex": (ci, [vp, ci, vp, vp, ci, vp, vp, ci, vp, ci, ci, ci, vp, vp, vp, vp, vp, sz, ci, vp]),
    "nvq_dwpw_forward": (ci, [vp, ci, vp, vp, vp, vp, ci, vp, ci, ci, ci, ci, ci, ci, cf, cf, _IP, vp, vp, vp, vp, vp, sz, vp]),
    "nvq_pw_bn_backward": (ci, [vp, ci, ci, vp, ci, vp, ci, ci, ci, ci, ci, vp, vp, vp, vp, ci, vp, vp, ci, vp, vp, vp, vp, vp, sz, vp]),
    "nvq_pw_bn_backward_ex": (ci, [vp, ci, ci, vp, ci, vp, ci, ci, ci, ci, ci, vp, vp, vp, vp, ci, vp, vp, ci, vp, vp, vp, vp, vp, sz, ci,
                                   vp]),
    "nvq_correlation_forward": (ci, [vp, ci, vp, ci, ci, ci, ci, ci, ci, vp, ci, ci, ci, ci, vp]),
    "nvq_correlation_backward": (ci, [ci, vp, ci, vp, ci, ci, ci, ci, ci, ci, vp, ci, ci, ci, ci, ci, ci, ci, vp, ci, vp, vp]),
    "nvq_warp_forward": (ci, [vp, ci, vp, ci, ci, ci, ci, ci, vp, ci, ci, ci, ci, vp]),
    "nvq_warp_backward": (ci, [vp, ci, ci, vp, ci, vp, ci, ci, ci, ci, ci, vp, ci, vp, ci, vp, sz, ci, ci, ci, ci, vp]),
    "nvq_warp_backward_workspace_bytes": (sz, [ci, ci, ci, ci]),
    "nvq_warp_backward_ex": (ci, [vp, ci, ci, vp, ci, vp, ci, ci, ci, ci, ci, vp, ci, vp, ci, vp, sz, ci, ci, ci, ci, ci, vp, sz,
                                  vp]),
    "nvq_tsum_blocks": (ci, [ci, ci]),
    "nvq_tsum_forward": (ci, [vp, ci, vp, ci, ci, ci, ci, ci, ci, vp, ci, vp, ci, vp, ci, ci, vp]),
    "nvq_tsum_backward": (ci, [vp, ci, vp, vp, ci, vp, ci, ci, ci, ci, ci, ci, vp, ci, vp, ci, ci, ci, ci, vp]),
    "nvq_cbam_channel": (ci, [vp, ci, ci, ci, ci, ci, vp, vp, vp, vp, vp, vp]),
    "nvq_cbam_pool": (ci, [vp, ci, vp, ci, ci, ci, ci, vp, vp, ci, vp]),
    "nvq_cbam_spatial_apply": (ci, [vp, ci, vp, vp, vp, ci, ci, ci, ci, vp, vp, ci, ci, ci, ci, vp]),
    "nvq_cbam_bwd_spatial_pre": (ci, [vp, ci, ci, vp, ci, vp, vp, ci, ci, ci, ci, vp, ci, vp]),
    "nvq_cbam_bwd_spatial_conv": (ci, [vp, vp, vp, ci, ci, ci, vp, vp, vp, sz, ci, vp]),
    "nvq_cbam_bwd_spatial_conv_ex": (ci, [vp, vp, vp, ci, ci, ci, vp, vp, vp, sz, ci, ci, vp]),
    "nvq_cbam_bwd_scale": (ci, [vp, ci, ci, vp, ci, vp, vp, vp, vp, ci, ci, ci, ci, vp, ci, vp, ci, vp]),
    "nvq_cbam_bwd_channel": (ci, [vp, ci, ci, ci, ci, ci, vp, vp, vp, vp, vp, vp, vp, vp, ci, vp]),
    "nvq_cbam_bwd_channel_ex": (ci, [vp, ci, ci, ci, ci, ci, vp, vp, vp, vp, vp, vp, vp, vp, ci, ci, vp]),
    "nvq_upsampler_tail_forward": (ci, [C.POINTER(ConvDesc), vp, ci, ci, ci, ci, vp, vp, vp]),
    "nvq_shuffle_bicubic_clamp": (ci, [vp, ci, vp, ci, ci, ci, ci, ci, ci, ci, vp, vp, vp]),
    "nvq_shuffle_clamp_backward": (ci, [vp, vp, ci, ci, ci, ci, ci, vp, ci, vp]),
    "nvq_bicubic_blend": (ci, [vp, vp, ci, ci, ci, ci, ci, ci, ci, cf, vp, vp]),
    "nvq_head_dgrad": (ci, [vp, ci, ci, vp, ci, vp, ci, ci, vp, ci, ci, ci, ci, ci, ci, _IP, ci, vp, ci, vp]),
    "nvq_bicubic_adjoint": (ci, [vp, vp, ci, ci, ci, ci, ci, ci, ci, cf, vp, ci, vp]),
    "nvq_head_dgrad_tc": (ci, [vp, ci, ci, vp, ci, ci, ci, ci, ci, ci, _IP, _IP, ci, ci, vp, ci, vp]),
    "nvq_stem7_dgrad": (ci, [vp, ci, ci, vp, ci, ci, ci, ci, vp, vp, ci, vp]),
    "nvq_mask_blend_backward_ex": (ci, [vp, vp, vp, ci, vp, ci, ci, ci, ci, vp, vp, vp, vp]),
    "nvq_nchw_to_nhwc": (ci, [vp, cl, ci, ci, ci, ci, vp, ci, ci, ci, vp]),
    "nvq_nhwc_to_nchw": (ci, [vp, ci, ci, ci, ci, ci, ci, vp, cl, vp]),
    "nvq_gather_nchw": (ci, [vp, ci, ci, ci, ci, ci, vp]),
    "nvq_inject_nchw": (ci, [vp, ci, ci, ci, ci, ci, vp]),
    "nvq_sizeof_gather_job": (sz, []),
    "nvq_sizeof_inject_job": (sz, []),
    "nvq_bn2_workspace_bytes": (sz, [ci]),
    "nvq_bn2_stats": (ci, [vp, ci, ci, cl, cf, cf, vp, vp, vp, vp, vp, sz, ci, vp]),
    "nvq_bn2_eval_stats": (ci, [vp, vp, ci, cf, vp, vp, vp]),
    "nvq_bn2_apply": (ci, [vp, ci, ci, cl, vp, vp, vp, vp, vp, ci, ci, vp, ci, ci, vp]),
    "nvq_bn2_backward": (ci, [vp, ci, vp, ci, ci, cl, vp, vp, vp, vp, vp, ci, ci, ci, vp, ci, vp, ci, vp, vp, vp, sz, ci, vp]),
    "nvq_bn2_backward_ex": (ci, [vp, ci, vp, ci, ci, cl, vp, vp, vp, vp, vp, ci, ci, ci, vp, ci, vp, ci, vp, vp, vp, sz, ci, ci, vp]),
    # synchronised BatchNorm: reduce / finish phases (fp64 sums in caller buffers)
    "nvq_bn_stats_reduce": (ci, [vp, ci, ci, ci, ci, ci, ci, vp, vp, sz, ci, vp]),
    "nvq_bn_stats_finish": (ci, [vp, ci, ci, cf, cf, _IP, vp, vp, vp, vp, vp]),
    "nvq_dwpw_forward_sums": (ci, [vp, ci, vp, vp, vp, vp, ci, vp, ci, ci, ci, ci, ci, vp, vp, sz, vp]),
    "nvq_bn_relu_backward_reduce": (ci, [vp, ci, vp, ci, ci, ci, ci, ci, ci, vp, vp, vp, vp, vp, vp, vp, vp, sz, ci, ci, ci, vp]),
    "nvq_bn_relu_backward_finish": (ci, [vp, ci, vp, ci, ci, ci, ci, ci, ci, vp, vp, vp, vp, vp, vp, vp, ci, ci, ci, ci, vp]),
    "nvq_pw_bn_backward_reduce": (ci, [vp, ci, ci, vp, ci, ci, ci, ci, ci, vp, vp, vp, vp, vp, vp, vp, vp, sz, vp]),
    "nvq_pw_bn_backward_finish": (ci, [vp, ci, ci, vp, ci, vp, ci, ci, ci, ci, ci, vp, vp, vp, vp, vp, vp, ci, vp, vp, vp, vp, sz,
                                       ci, vp]),
    "nvq_bn2_stats_reduce": (ci, [vp, ci, ci, cl, vp, vp, sz, ci, vp]),
    "nvq_bn2_stats_finish": (ci, [vp, ci, cf, cf, vp, vp, vp, vp, vp]),
    "nvq_bn2_backward_reduce": (ci, [vp, ci, vp, ci, ci, cl, vp, vp, vp, vp, vp, ci, ci, vp, ci, vp, vp, vp, vp, sz, ci, vp]),
    "nvq_bn2_backward_finish": (ci, [vp, ci, vp, ci, ci, cl, vp, vp, vp, vp, vp, ci, ci, vp, vp, vp, ci, ci, vp]),
    "nvq_maxpool_forward": (ci, [vp, ci, ci, ci, ci, ci, ci, ci, vp, vp, ci, vp]),
    "nvq_maxpool_backward": (ci, [vp, vp, ci, ci, ci, ci, ci, ci, ci, vp, ci, vp]),
    "nvq_subsample2": (ci, [vp, ci, ci, ci, ci, vp, ci, ci, vp]),
    "nvq_bilinear_resize": (ci, [vp, ci, ci, ci, ci, ci, ci, vp, ci, vp]),
    "nvq_convt_pack": (ci, [vp, ci, ci, vp, vp]),
    "nvq_convt_unpack_grad": (ci, [vp, ci, ci, vp, vp]),
    "nvq_depth_space2": (ci, [vp, vp, ci, ci, ci, ci, ci, ci, vp]),
    "nvq_cast_slice": (ci, [vp, ci, ci, ci, vp, ci, ci, ci, ci, cl, cf, ci, vp]),
    "nvq_tconv_relayout": (ci, [vp, vp, ci, ci, ci, vp]),
    "nvq_tconv_cat": (ci, [vp, ci, ci, ci, ci, ci, ci, vp, vp]),
    "nvq_tconv_grad_combine": (ci, [vp, vp, vp, ci, ci, ci, vp, vp]),
    "nvq_gap_blocks": (ci, [ci, ci]),
    "nvq_gap_partial": (ci, [vp, ci, ci, ci, ci, ci, vp, vp]),
    "nvq_add_image_channel": (ci, [vp, ci, ci, ci, ci, ci, vp, vp]),
    "nvq_tanh": (ci, [vp, vp, cl, vp, ci, vp]),
    "nvq_fusion_mix_forward": (ci, [vp, vp, ci, vp, ci, vp, ci, ci, cl, vp, vp, vp, vp]),
    "nvq_fusion_mix_backward": (ci, [vp, vp, vp, ci, cl, vp, ci, vp, ci, vp, ci, vp]),
    "nvq_mask_blend": (ci, [vp, vp, ci, vp, ci, ci, ci, ci, vp, vp]),
    "nvq_mask_blend_backward": (ci, [vp, vp, ci, ci, ci, ci, vp, ci, vp]),
    "nvq_stem7_forward": (ci, [vp, vp, ci, ci, ci, ci, vp, ci, ci, vp]),
    "nvq_stem7_wgrad": (ci, [vp, vp, ci, ci, ci, ci, ci, vp, vp, sz, ci, vp]),
    "nvq_pixel_shuffle": (ci, [vp, ci, ci, ci, ci, ci, ci, vp, ci, vp]),
    "nvq_mse_forward": (ci, [vp, vp, cl, vp, vp, sz, vp]),
    "nvq_mse_backward": (ci, [vp, vp, cl, vp, vp, vp]),
    "nvq_quality_sums": (ci, [vp, vp, ci, cl, vp, vp, sz, vp]),
    "nvq_pixel_loss_forward": (ci, [vp, vp, ci, cl, ci, cf, vp, vp, sz, vp]),
    "nvq_pixel_loss_backward": (ci, [vp, vp, ci, cl, ci, cf, vp, vp, vp]),
    "nvq_ssim_forward": (ci, [vp, vp, ci, ci, ci, ci, cf, ci, ci, vp, vp, sz, vp]),
    "nvq_ssim_backward": (ci, [vp, vp, ci, ci, ci, ci, cf, vp, ci, cf, vp, vp]),
    "nvq_avgpool2_pair": (ci, [vp, vp, ci, ci, ci, vp, vp, vp]),
    "nvq_msssim_workspace_bytes": (sz, [ci, ci, ci, ci]),
    "nvq_msssim_scale_forward": (ci, [vp, vp, ci, ci, ci, ci, ci, cf, vp, sz, vp]),
    "nvq_msssim_finalize": (ci, [vp, ci, ci, ci, ci, ci, vp, ci, ci, vp, vp, vp, vp]),
    "nvq_msssim_scale_backward": (ci, [vp, vp, ci, ci, ci, ci, ci, ci, cf, vp, vp, ci, cf, vp, vp, vp]),
    # distillation losses (csrc/distill.hip)
    "nvq_distill_forward": (ci, [vp, vp, vp, ci, cl, cf, cf, vp, vp, sz, vp]),
    "nvq_distill_backward": (ci, [vp, vp, vp, ci, cl, cf, cf, vp, vp, vp]),
    "nvq_cosine_distill_forward": (ci, [vp, vp, ci, ci, ci, cf, ci, vp, vp, sz, vp]),
    "nvq_cosine_distill_backward": (ci, [vp, vp, ci, ci, ci, cf, vp, ci, vp, vp]),
    "nvq_axpy_slice": (ci, [vp, ci, ci, vp, ci, ci, vp, ci, ci, ci, cl, cf, ci, ci, vp]),
    "nvq_colsum": (ci, [vp, ci, ci, ci, cl, cf, vp, vp, sz, ci, vp]),
    "nvq_ewc_penalty": (ci, [vp, vp, vp, cl, cf, vp, vp, sz, vp]),
    "nvq_ewc_penalty_grad": (ci, [vp, vp, vp, cl, cf, vp, vp, ci, vp]),
    "nvq_fisher_accumulate": (ci, [vp, cl, vp, vp]),
    "nvq_si_update": (ci, [vp, vp, cl, vp, vp, vp]),
    "nvq_si_consolidate": (ci, [vp, cl, cf, vp, vp, vp, vp]),
    # gradient projection (A-GEM) and global-norm clipping on flat buckets (csrc/bucket_ops.hip)
    "nvq_bucket_moments": (ci, [vp, vp, cl, vp, ci, ci, vp, sz, vp]),
    "nvq_bucket_project": (ci, [vp, vp, cl, vp, vp]),
    "nvq_bucket_clip": (ci, [vp, cl, vp, cf, vp, vp]),
    # Adam / AdamW with clipping and weight EMA on flat buffers (csrc/optim.hip)
    "nvq_adam_step": (ci, [vp, vp, vp, vp, vp, cl, cf, cf, cf, cf, cf, cf, cf, ci, cf, cf, cf, vp, cf, vp]),
    # device-resident episodic memory (csrc/replay.hip)
    "nvq_replay_store": (ci, [vp, vp, ci, cl, cl, ci, vp, vp, vp, vp, vp, vp, ci, ci, vp, vp, vp, vp, vp, ci, vp]),
    "nvq_replay_gather": (ci, [vp, vp, ci, ci, cl, cl, vp, ci, vp, vp, ci, vp, vp]),
    "nvq_replay_sample_weighted": (ci, [vp, vp, vp, ci, ci, cf, ci, vp, ci, vp, vp]),
    "nvq_replay_update_importance": (ci, [vp, ci, vp, vp, ci, cf, vp]),
    "nvq_replay_nearest": (ci, [vp, vp, vp, ci, ci, vp, vp, vp]),
    # drift detection (csrc/drift.hip)
    "nvq_rbf_gram_workspace_bytes": (sz, [ci, ci, ci]),
    "nvq_rbf_gram_sum": (ci, [vp, vp, vp, vp, ci, ci, ci, ci, ci, vp, ci, vp, vp, sz, vp]),
    "nvq_mmd_finish": (ci, [vp, ci, ci, cf, vp, vp, vp]),
    "nvq_psi_counts": (ci, [vp, cl, vp, ci, vp, vp]),
    "nvq_psi_finish": (ci, [vp, vp, ci, cl, cl, vp, vp, vp]),
    "nvq_cell_descriptor": (ci, [vp, ci, ci, ci, ci, ci, ci, vp, vp]),
    "nvq_metric_window_update": (ci, [vp, vp, vp, ci, cf, cf, vp, vp, vp]),
    # Kolmogorov-Smirnov drift test (csrc/ks.hip)
    "nvq_sort_columns": (ci, [vp, vp, ci, ci, ci, vp, vp]),
    "nvq_ks_statistic": (ci, [vp, vp, ci, ci, ci, vp, vp, vp]),
    "nvq_ks_pvalue": (ci, [vp, ci, ci, ci, vp, vp]),
    "nvq_ks_finish": (ci, [vp, ci, vp, vp, vp, vp]),
    # federated aggregation and differential privacy on flat buffers (csrc/federated.hip)
    "nvq_fed_workspace_bytes": (sz, [ci, cl]),
    "nvq_fed_delta_norms": (ci, [vp, cl, ci, vp, cl, vp, vp, sz, vp]),
    "nvq_fed_aggregate": (ci, [vp, cl, ci, vp, vp, vp, cf, cf, cf, cl, cl, cl, vp, vp]),
    "nvq_dp_segment_norms": (ci, [vp, vp, vp, ci, vp, ci, vp, vp, sz, vp]),
    "nvq_dp_clip_noise": (ci, [vp, vp, vp, ci, vp, ci, vp, cf, cf, cl, cl, vp]),
    "nvq_fed_gram_workspace_bytes": (sz, [ci, cl]),
    "nvq_fed_update_gram": (ci, [vp, cl, ci, vp, cl, vp, vp, sz, vp]),
    "nvq_cluster_gram_kmeans": (ci, [vp, ci, ci, vp, ci, vp, vp, vp, vp, vp]),
    "nvq_fed_aggregate_clusters": (ci, [vp, cl, ci, vp, ci, vp, cl, vp, vp, cf, cf, cf, cl, cl, cl, vp, cl, vp]),
    # Byzantine-robust aggregation: trimmed mean / median, Krum selection (csrc/robust.hip)
    "nvq_fed_trimmed_aggregate": (ci, [vp, cl, ci, vp, vp, ci, cf, cf, cl, cl, cl, vp, vp]),
    "nvq_fed_krum_select": (ci, [vp, ci, vp, ci, ci, vp, vp, vp, vp]),
    # federated optimisation: FedOpt server rules, the FedProx gradient (csrc/fedopt.hip)
    "nvq_fed_server_opt": (ci, [vp, cl, ci, vp, vp, vp, cf, ci, cf, cf, cf, cf, vp, vp, cf, cl, cl, cl, vp, vp]),
    "nvq_fed_prox_grad": (ci, [vp, vp, vp, cl, cf, vp]),
    # compressed client updates: top-k with error feedback, QSGD quantisation (csrc/compress.hip)
    "nvq_fed_compress_workspace_bytes": (sz, [ci, cl]),
    "nvq_fed_compress": (ci, [vp, cl, ci, vp, cl, cl, ci, vp, cl, vp, cl, cl, vp, vp, sz, vp]),
    # ABR agent: vectorised environment, fused act, GAE, PPO loss (csrc/abr.hip)
    "nvq_abr_env_reset": (ci, [vp, vp, vp, vp, ci, ci, cl, ci, vp]),
    "nvq_abr_env_step": (ci, [vp, vp, vp, _IP, ci, ci, ci, vp, cl, ci, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
    "nvq_abr_act_supported": (ci, [ci, _IP]),
    "nvq_abr_act": (ci, [vp, ci, ci, vp, _IP, vp, cl, ci, vp, vp, vp, vp, vp]),
    "nvq_abr_gae": (ci, [vp, vp, vp, vp, cf, cf, ci, ci, vp, vp, vp]),
    "nvq_abr_adv_stats": (ci, [vp, cl, vp, vp]),
    "nvq_ppo_loss_workspace_bytes": (sz, [cl]),
    "nvq_ppo_loss": (ci, [vp, vp, vp, vp, vp, vp, cl, _IP, ci, cf, cf, cf, vp, vp, vp, sz, vp]),
    # Gradient Episodic Memory: Gram of the references and the gradient, the QP, the projection (csrc/gem.hip)
    "nvq_gem_gram": (ci, [vp, cl, ci, vp, cl, vp, ci, vp, sz, vp]),
    "nvq_gem_solve": (ci, [vp, ci, cf, cf, ci, vp, vp, vp]),
    "nvq_gem_project": (ci, [vp, vp, cl, ci, cl, vp, vp]),
}


def lib():
    """Load libnvq.so once; raise loudly when it is absent (no fallback exists)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"libnvq.so not found at {LIB_PATH}: build it with "
                f"`python -c 'import __graft_entry__ as g; g.build()'` (hipcc --offload-arch=gfx950). "
                "nerve_cl has no CPU / PyTorch fallback for the super-resolution hot path.")
        l = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(l, name)
            fn.restype = res
            fn.argtypes = args
        assert l.nvq_sizeof_conv_desc() == C.sizeof(ConvDesc), "nvq_conv_desc layout mismatch"
        assert l.nvq_sizeof_wgrad_desc() == C.sizeof(WgradDesc), "nvq_wgrad_desc layout mismatch"
        assert l.nvq_sizeof_wgrad_reduce_job() == C.sizeof(WgradReduceJob), "nvq_wgrad_reduce_job layout mismatch"
        assert l.nvq_sizeof_gather_job() == C.sizeof(GatherJob), "nvq_gather_job layout mismatch"
        assert l.nvq_sizeof_inject_job() == C.sizeof(InjectJob), "nvq_inject_job layout mismatch"
        _lib = l
    return _lib


def check(rc: int, what: str) -> None:
    if rc != 0:
        raise RuntimeError(f"{what} failed (code {rc}): {lib().nvq_last_error().decode()}")


def stream() -> vp:
    return vp(torch.cuda.current_stream().cuda_stream)


def require_device(t: torch.Tensor, what: str = "tensor") -> None:
    if not t.is_cuda:
        raise RuntimeError(
            f"{what} lives on {t.device}: the nerve_cl super-resolution path runs only as HIP kernels "
            "on an AMD GPU (move the model and its inputs to 'cuda'); there is no CPU fallback.")


def device_guard(dev: torch.device):
    """Context that makes `dev` the current HIP device: libnvq launches on the CURRENT device's stream, so a tensor on
    cuda:1 must not be handed to a launch issued while cuda:0 is current."""
    import contextlib
    return torch.cuda.device(dev) if dev.type == "cuda" else contextlib.nullcontext()


def is_bf16(t: Optional[torch.Tensor]) -> int:
    return int(t is not None and t.dtype == torch.bfloat16)


def ptr(t: Optional[torch.Tensor], off: int = 0) -> Optional[int]:
    """Device address of element `off` of a contiguous fp32/int32/uint8 tensor (None passes NULL)."""
    if t is None:
        return None
    require_device(t)
    assert t.is_contiguous(), "libnvq needs contiguous tensors"
    return t.data_ptr() + off * t.element_size()


def int_array(vals: Sequence[int]):
    return (ci * len(vals))(*vals)


class Sl:
    """A channel slice of an NHWC activation buffer (fp32, or bf16 for conv-internal tensors):
    tensor [N,H,W,ld], channels [coff, coff+c); ld / coff count elements of the tensor's dtype."""

    __slots__ = ("t", "ld", "coff", "c", "plane")

    def __init__(self, t: torch.Tensor, c: Optional[int] = None, coff: int = 0, plane: int = 0):
        """plane != 0 (conv / weight-gradient INPUTS only): `t` is the leading tensor of a slice-planar buffer (CatBuf) and
        the c channels continue in the compact 32-channel planes behind it (nvq_conv_desc::in_plane)."""
        assert t.dtype in (torch.float32, torch.bfloat16) and t.dim() == 4 and t.is_contiguous()
        self.t, self.ld, self.coff, self.plane = t, t.shape[-1], coff, plane
        self.c = t.shape[-1] - coff if c is None else c
        assert self.coff + self.c <= self.ld or (plane and coff == 0)

    @property
    def n(self):
        return self.t.shape[0]

    @property
    def bf16(self) -> int:
        return int(self.t.dtype == torch.bfloat16)

    def images(self, lo: int, hi: int) -> "Sl":
        assert not self.plane
        return Sl(self.t[lo:hi], self.c, self.coff)

    def base(self) -> int:
        """address of channel `coff` of pixel 0"""
        return ptr(self.t, self.coff)


class CatBuf:
    """The buffer of one residual dense block: [x (F channels) | 32-channel slices ...] (forward: x, y_0 .. y_4; backward:
    gout, dy_4 .. dy_0).  Interleaved: one [N,H,W,ld] tensor, a slice = a channel range (torch.cat for free).  Slice-planar
    (planar=True, bf16): x and every slice are compact tensors of their own in one allocation, so a layer's 64-byte pixel
    rows fill whole 128-byte lines; the convs / weight gradients that read a channel prefix take it through `inp()`."""

    def __init__(self, dev, N: int, H: int, W: int, F: int, nslices: int, ld: int, dtype, planar: bool):
        self.F, self.planar = F, planar
        if planar:
            assert dtype == torch.bfloat16 and F in (32, 64, 128)
            npx = N * H * W
            self.plane = npx * 32
            self.flat = torch.empty((F // 32 + nslices) * self.plane, dtype=dtype, device=dev)
            self.lead = self.flat[:npx * F].view(N, H, W, F)
            self.slices = [self.flat[(F // 32 + j) * self.plane:(F // 32 + j + 1) * self.plane].view(N, H, W, 32)
                           for j in range(nslices)]
        else:
            self.t = torch.empty((N, H, W, ld), dtype=dtype, device=dev)

    def x(self) -> Sl:
        return Sl(self.lead) if self.planar else Sl(self.t, self.F, 0)

    def y(self, j: int) -> Sl:
        return Sl(self.slices[j]) if self.planar else Sl(self.t, 32, self.F + 32 * j)

    def inp(self, cin: int) -> Sl:
        return Sl(self.lead, cin, 0, plane=self.plane) if self.planar else Sl(self.t, cin, 0)


class KernelTimer:
    """HIP-event timing of individual launches on the current stream (bench.py only)."""

    def __init__(self):
        self.records = []          # (label, flops, bytes, ev0, ev1, shape)
        self.tags = []             # section tag of each record (TIMER_TAG at launch time)
        self.enabled = True

    def start(self):
        if not self.enabled:
            return None
        ev = torch.cuda.Event(enable_timing=True)
        ev.record()
        return ev

    def stop(self, ev0, label, flops, nbytes, shape=""):
        if ev0 is None:
            return
        ev1 = torch.cuda.Event(enable_timing=True)
        ev1.record()
        self.records.append((label, flops, nbytes, ev0, ev1, shape))
        self.tags.append(TIMER_TAG)

    def _durations(self):
        """ms per record.  An event pair brackets the launch on the stream, so when the GPU has caught up with the host the
        pair also contains the host's launch gap; such records (more than twice the median of their (label, shape) group)
        are counted at the group median.  Returns (durations, number of records replaced)."""
        raw = [e0.elapsed_time(e1) for _, _, _, e0, e1, _ in self.records]
        groups = {}
        for i, (label, _, _, _, _, shape) in enumerate(self.records):
            groups.setdefault((label, shape), []).append(i)
        fixed = 0
        for idx in groups.values():
            vals = sorted(raw[i] for i in idx)
            med = vals[len(vals) // 2]
            for i in idx:
                if raw[i] > 2.0 * med:
                    raw[i] = med
                    fixed += 1
        self.outliers = fixed
        return raw

    def summary(self):
        """{label: dict(launches, ms_total, flops, bytes)} (call after a device synchronize)."""
        out = {}
        dur = self._durations()
        for (label, fl, nb, _, _, _), ms in zip(self.records, dur):
            d = out.setdefault(label, dict(launches=0, ms_total=0.0, flops=0.0, bytes=0.0))
            d["launches"] += 1
            d["ms_total"] += ms
            d["flops"] += fl
            d["bytes"] += nb
        return out

    def by_tag(self):
        """{tag: dict(launches, ms_total, flops, bytes)} over the engine's section tags (e.g. "rdb")."""
        out = {}
        dur = self._durations()
        for (label, fl, nb, _, _, _), ms, tag in zip(self.records, dur, self.tags):
            d = out.setdefault(tag, dict(launches=0, ms_total=0.0, flops=0.0, bytes=0.0))
            d["launches"] += 1
            d["ms_total"] += ms
            d["flops"] += fl
            d["bytes"] += nb
        return out

    def by_shape(self):
        """{(label, shape): dict(...)} for the per-shape table of bench.py --detail."""
        out = {}
        dur = self._durations()
        for (label, fl, nb, _, _, shape), ms in zip(self.records, dur):
            d = out.setdefault((label, shape), dict(launches=0, ms_total=0.0, flops=0.0, bytes=0.0))
            d["launches"] += 1
            d["ms_total"] += ms
            d["flops"] += fl
            d["bytes"] += nb
        return out


TIMER: Optional[KernelTimer] = None
TIMER_TAG = ""     # set by the engine around a section (bench.py's per-section roofline)


def _nt(cout: int) -> int:
    return 16 if cout <= 16 else (32 if cout <= 32 else 64)


def wgrad_workspace_bytes() -> int:
    return int(lib().nvq_wgrad_workspace_bytes())


def pad4(c: int) -> int:
    return (c + 3) // 4 * 4


# ----------------------------------------------------------------------------- convolution
class PackJob(C.Structure):
    """nvq_pack_job"""
    _fields_ = [("w", vp), ("cout_w", ci), ("cin_w", ci), ("ksize", ci), ("transpose", ci), ("cin_store", ci),
                ("cout_keep", ci), ("wpack", vp)]


def conv_pack_many(reqs, math: int = MATH_F32) -> "list[torch.Tensor]":
    """conv_pack of every (w, transpose, cin_store, cout_keep) of `reqs` in one launch per 48 jobs (nvq_conv_pack_batch);
    the results are slices of one buffer."""
    if not reqs:
        return []
    sizes, ws = [], []
    for w, transpose, cin_store, cout_keep in reqs:
        cout_w, cin_w, k, _ = w.shape
        keep = (cin_w if cout_keep is None else cout_keep) if transpose else cout_w
        sizes.append((int(lib().nvq_conv_pack_floats(keep, cin_store, k, math)), keep))
        ws.append(w.contiguous())
    flat = torch.empty(sum((n + 3) // 4 * 4 for n, _ in sizes), dtype=torch.float32, device=ws[0].device)
    jobs = (PackJob * len(reqs))()
    outs, off = [], 0
    for i, ((w, transpose, cin_store, _), (n, keep)) in enumerate(zip(reqs, sizes)):
        out = flat[off:off + n]
        off += (n + 3) // 4 * 4
        cout_w, cin_w, k, _ = w.shape
        jobs[i] = PackJob(ptr(ws[i]), cout_w, cin_w, k, int(transpose), cin_store, keep if transpose else 0, ptr(out))
        outs.append(out)
    check(lib().nvq_conv_pack_batch(C.cast(jobs, vp), len(reqs), math, stream()), "nvq_conv_pack_batch")
    return outs


def conv_pack(w: torch.Tensor, transpose: bool, cin_store: int, cout_keep: Optional[int] = None,
              math: int = MATH_F32) -> torch.Tensor:
    """Pack a PyTorch conv weight [Cout, Cin, k, k] for nvq_conv_forward (mode-specific layout)."""
    cout_w, cin_w, k, _ = w.shape
    keep = (cin_w if cout_keep is None else cout_keep) if transpose else cout_w
    n = lib().nvq_conv_pack_floats(keep, cin_store, k, math)
    wp = torch.empty(n, dtype=torch.float32, device=w.device)
    check(lib().nvq_conv_pack(ptr(w.contiguous()), cout_w, cin_w, k, int(transpose), cin_store,
                              keep if transpose else 0, math, ptr(wp), stream()), "nvq_conv_pack")
    return wp


def _conv_desc(x: Sl, wpack: torch.Tensor, bias: Optional[torch.Tensor], out: Sl, ksize: int, *,
                 relu: bool = False, alpha: float = 1.0, accumulate: bool = False,
                 cout_store: Optional[int] = None, out2: Optional[Sl] = None,
                 res: Optional[Sl] = None, mask: Optional[Sl] = None, mask_c0: int = 0,
                 mask_c1: int = 0, math: int = MATH_F32, alg_cin: Optional[int] = None,
                 bits: Optional[torch.Tensor] = None, bits_mode: int = 0, center_cin: int = 0,
                 tile_rows: int = 0) -> ConvDesc:
    """bits: int32 [N,H,W] or [N,H,W,words] one-bit ReLU masks (see nvq_conv_desc): bits_mode 1 = write, 2 = read as the mask.
    center_cin: leading input channels whose weights are zero outside the centre tap (a hint, see nvq_conv_desc)."""
    n, h, w, _ = x.t.shape
    assert out.t.shape[:3] == x.t.shape[:3]
    d = ConvDesc()
    d.inp, d.in_ld, d.in_coff, d.cin = ptr(x.t), x.ld, x.coff, x.c
    d.wpack = ptr(wpack)
    d.bias = ptr(bias)
    d.out, d.out_ld, d.out_coff, d.cout = ptr(out.t), out.ld, out.coff, out.c
    d.cout_store = out.c if cout_store is None else cout_store
    if out2 is not None:
        d.out2, d.out2_ld, d.out2_coff = ptr(out2.t), out2.ld, out2.coff
    if res is not None:
        d.res, d.res_ld, d.res_coff, d.res_cmax = ptr(res.t), res.ld, res.coff, res.c
    if mask is not None:
        d.mask, d.mask_ld, d.mask_coff, d.mask_c0, d.mask_c1 = ptr(mask.t), mask.ld, mask.coff, mask_c0, mask_c1
    d.n, d.h, d.w, d.ksize = n, h, w, ksize
    d.relu, d.alpha, d.accumulate, d.math = int(relu), alpha, int(accumulate), math
    d.in_bf16, d.out_bf16 = x.bf16, out.bf16
    d.out2_bf16 = out2.bf16 if out2 is not None else 0
    d.res_bf16 = res.bf16 if res is not None else 0
    d.mask_bf16 = mask.bf16 if mask is not None else 0
    if bits_mode:
        assert bits is not None and bits.dtype == torch.int32 and tuple(bits.shape[:3]) == (n, h, w) and bits.is_contiguous()
        d.bits, d.bits_mode = ptr(bits), bits_mode
        d.bits_words = bits.shape[3] if bits.dim() == 4 else 1        # [N,H,W] (cout <= 32) or [N,H,W,ceil(cout / 32)]
    d.center_cin = center_cin
    d.in_plane = x.plane
    d.tile_rows = tile_rows
    return d


def conv_forward(x: Sl, wpack: torch.Tensor, bias: Optional[torch.Tensor], out: Sl, ksize: int, *,
                 relu: bool = False, alpha: float = 1.0, accumulate: bool = False,
                 cout_store: Optional[int] = None, out2: Optional[Sl] = None,
                 res: Optional[Sl] = None, mask: Optional[Sl] = None, mask_c0: int = 0,
                 mask_c1: int = 0, math: int = MATH_F32, alg_cin: Optional[int] = None,
                 bits: Optional[torch.Tensor] = None, bits_mode: int = 0, center_cin: int = 0, tile_rows: int = 0) -> None:
    n, h, w, _ = x.t.shape
    ev0 = TIMER.start() if TIMER is not None else None
    d = _conv_desc(x, wpack, bias, out, ksize, relu=relu, alpha=alpha, accumulate=accumulate, cout_store=cout_store,
                   out2=out2, res=res, mask=mask, mask_c0=mask_c0, mask_c1=mask_c1, math=math, bits=bits,
                   bits_mode=bits_mode, center_cin=center_cin, tile_rows=tile_rows)
    check(lib().nvq_conv_forward(C.byref(d), stream()), "nvq_conv_forward")
    if ev0 is not None:
        cin = x.c if alg_cin is None else alg_cin
        esz = lambda sl: 2.0 if sl.bf16 else 4.0   # noqa: E731  bytes per element
        nbytes = cin * esz(x) + out.c * esz(out) * (2 if accumulate else 1) \
            + (res.c * esz(res) if res is not None else 0) + (out2.c * esz(out2) if out2 is not None else 0) \
            + ((mask_c1 - mask_c0) * esz(mask) if mask is not None else 0) + (4 * (bits.shape[3] if bits is not None and bits.dim() == 4 else 1) if bits_mode else 0)
        TIMER.stop(ev0, f"conv_{'bf16' if math == MATH_BF16 else 'f32'}_kernel<{_nt(out.c) // 16},{ksize}>", 2.0 * n * h * w * (cin * ksize * ksize - center_cin * (ksize * ksize - 1)) * out.c,
                   n * h * w * nbytes, f"n{n} cin{x.c}{'h' if x.bf16 else ''} cout{out.c}{'h' if out.bf16 else ''}"
                   + (" acc" if accumulate else "")
                   + (" res" if res is not None else "") + (" mask" if mask is not None else "")
                   + (" bitsW" if bits_mode == 1 else " bitsR" if bits_mode == 2 else "")
                   + (f" ctr{center_cin}" if center_cin else ""))


def rdb_tail_forward(x: Sl, w3: torch.Tensor, b3, y4: Sl, wl: torch.Tensor, bl, out: Sl, *, alpha: float, res: Sl,
                     bits: Optional[torch.Tensor] = None, tile_rows: int = 0) -> None:
    """Last dense layer (3x3, x -> y4 = the next 32 channels of the same buffer, bias + ReLU) and the block's 1x1 fusion
    over [x | y4] (-> out = alpha * (lff + bias) + res) in one launch (nvq_rdb_tail_forward).  tile_rows = 4: the four-wave
    kernel instead of the eight-wave, two-role one (same results)."""
    n, h, w, _ = x.t.shape
    ev0 = TIMER.start() if TIMER is not None else None
    d3 = _conv_desc(x, w3, b3, y4, 3, relu=True, math=MATH_BF16, bits=bits, bits_mode=1 if bits is not None else 0,
                    tile_rows=tile_rows)
    xl = Sl(x.t, x.c + y4.c, x.coff, plane=x.plane)
    dl = _conv_desc(xl, wl, bl, out, 1, alpha=alpha, res=res, math=MATH_BF16)
    check(lib().nvq_rdb_tail_forward(C.byref(d3), C.byref(dl), stream()), "nvq_rdb_tail_forward")
    if ev0 is not None:
        esz = lambda sl: 2.0 if sl.bf16 else 4.0   # noqa: E731
        TIMER.stop(ev0, "rdb_tail_kernel", 2.0 * n * h * w * (x.c * y4.c * 9 + xl.c * out.c),
                   n * h * w * (x.c * 2.0 + y4.c * 2.0 + res.c * esz(res) + out.c * esz(out)),
                   f"n{n} cin{x.c}h -> 32 + lff {xl.c} -> {out.c}{'h' if out.bf16 else ''}")


def rdb_backward_weights(lff: torch.Tensor, ws: Sequence[torch.Tensor], F: int):
    """Combined 'mirror' weights of one dense block: returns ([Wb_4, Wb_3, Wb_2, Wb_1, Wb_0], Wb_x) as views
    of one buffer, PyTorch layout (see nvq_rdb_backward_weights)."""
    n = lib().nvq_rdb_backward_weights_floats(F)
    out = torch.empty(n, dtype=torch.float32, device=lff.device)
    check(lib().nvq_rdb_backward_weights(ptr(lff), *[ptr(w) for w in ws], F, ptr(out), stream()),
          "nvq_rdb_backward_weights")
    views, off = [], 0
    for t in range(5):
        k = 32 * (F + 32 * t) * 9
        views.append(out[off:off + k].view(32, F + 32 * t, 3, 3))
        off += k
    return views, out[off:].view(F, F + 160, 3, 3)


def conv_wgrad(x: Sl, cin_w: int, dy: Sl, dw: torch.Tensor, dbias: Optional[torch.Tensor],
               ws: torch.Tensor, ksize: int, *, alpha: float = 1.0, accumulate: bool = False,
               math: int = MATH_F32, variant: int = 0, defer: Optional[list] = None) -> None:
    """defer: a list -> only the weight-gradient kernel runs (nvq_conv_wgrad_partial); its reduce job is appended to the list
    and finished by wgrad_reduce_batch(list).  `ws` must then be this call's own until that batch has run."""
    n, h, w, _ = x.t.shape
    ev0 = TIMER.start() if TIMER is not None and defer is None else None
    d = WgradDesc()
    d.x, d.x_ld, d.x_coff, d.cin, d.cin_w = ptr(x.t), x.ld, x.coff, x.c, cin_w
    d.dy, d.dy_ld, d.dy_coff, d.cout = ptr(dy.t), dy.ld, dy.coff, dy.c
    d.dw, d.dbias = ptr(dw), ptr(dbias)
    d.workspace, d.workspace_bytes = ptr(ws), ws.numel() * ws.element_size()
    d.n, d.h, d.w, d.ksize = n, h, w, ksize
    d.alpha, d.accumulate, d.math = alpha, int(accumulate), math
    d.x_bf16, d.dy_bf16, d.x_plane = x.bf16, dy.bf16, x.plane
    d.variant = variant
    if defer is not None:
        job = WgradReduceJob()
        check(lib().nvq_conv_wgrad_partial(C.byref(d), C.byref(job), stream()), "nvq_conv_wgrad_partial")
        defer.append((job, (ws, dw, dbias)))               # (the tensors stay alive with the job)
        return
    check(lib().nvq_conv_wgrad(C.byref(d), stream()), "nvq_conv_wgrad")
    if ev0 is not None:
        TIMER.stop(ev0, f"wgrad_{'bf16' if math == MATH_BF16 else 'f32'}_kernel<{ksize}>", 2.0 * n * h * w * cin_w * dy.c * ksize * ksize,
                   n * h * w * (cin_w * (2.0 if x.bf16 else 4.0) + dy.c * (2.0 if dy.bf16 else 4.0)),
                   f"n{n} cin{cin_w}{'h' if x.bf16 else ''} cout{dy.c}{'h' if dy.bf16 else ''}")


def wgrad_reduce_batch(jobs: list) -> None:
    """Finish the weight gradients deferred into `jobs` (conv_wgrad(..., defer=jobs)): up to 16 reduces per launch."""
    if not jobs:
        return
    arr = (WgradReduceJob * len(jobs))(*[j for j, _ in jobs])
    check(lib().nvq_wgrad_reduce_batch(arr, len(jobs), stream()), "nvq_wgrad_reduce_batch")
    jobs.clear()


# ----------------------------------------------------------------------------- return_intermediate tensors
def _nhwc4(src: Sl):
    """(N, C, H, W) of an NHWC slice"""
    n, h, w, _ = src.t.shape
    return n, src.c, h, w


def gather_nchw(jobs: "Sequence[tuple[Sl, torch.Tensor]]") -> None:
    """dst = src as fp32 NCHW for every (src slice, dst [N,C,H,W] fp32) pair, one launch (nvq_gather_nchw; bit-exact)."""
    if not jobs:
        return
    shape = _nhwc4(jobs[0][0])
    arr = (GatherJob * len(jobs))()
    for a, (src, dst) in zip(arr, jobs):
        assert _nhwc4(src) == shape and not src.plane and dst.dtype == torch.float32 and tuple(dst.shape) == shape
        a.src, a.src_ld, a.src_coff, a.src_bf16, a.dst = ptr(src.t), src.ld, src.coff, src.bf16, ptr(dst)
    check(lib().nvq_gather_nchw(C.addressof(arr), len(jobs), *shape, stream()), "nvq_gather_nchw")


def inject_nchw(jobs: "Sequence[tuple[Sl, Sequence[Optional[torch.Tensor]]]]") -> None:
    """dst slice += src_0 + src_1 + ... (fp32 NCHW [N,C,H,W] each, None skipped) in that order, for every (dst slice, sources)
    pair, one launch (nvq_inject_nchw).  Jobs without a source are dropped; nothing runs when none is left."""
    jobs = [(d, list(ss)) for d, ss in jobs if any(x is not None for x in ss)]
    if not jobs:
        return
    shape = _nhwc4(jobs[0][0])
    arr = (InjectJob * len(jobs))()
    for a, (dst, srcs) in zip(arr, jobs):
        assert _nhwc4(dst) == shape and not dst.plane and len(srcs) <= INJECT_MAX_SRC
        a.dst, a.dst_ld, a.dst_coff, a.dst_bf16 = ptr(dst.t), dst.ld, dst.coff, dst.bf16
        for i, x in enumerate(srcs):
            if x is not None:
                assert x.dtype == torch.float32 and tuple(x.shape) == shape
                a.src[i] = ptr(x)
    check(lib().nvq_inject_nchw(C.addressof(arr), len(jobs), *shape, stream()), "nvq_inject_nchw")


# ----------------------------------------------------------------------------- feature extractor
def head_forward(frames: torch.Tensor, slots: Sequence[int], weight, bias, out: torch.Tensor,
                 img8: Optional[torch.Tensor] = None, math: int = MATH_F32) -> None:
    B, T, Cin, H, W = frames.shape
    F = weight.shape[0]
    assert img8 is None or (img8.dtype == torch.bfloat16 and tuple(img8.shape) == (len(slots) * B, H, W, 8))
    check(lib().nvq_head_forward(ptr(frames), B, T, Cin, H, W, int_array(slots), len(slots), ptr(weight),
                                 ptr(bias), F, ptr(out), out.shape[-1], is_bf16(out), ptr(img8), math, stream()),
          "nvq_head_forward")


def head_wgrad(frames, slots, dout: torch.Tensor, act: torch.Tensor, dweight, dbias, ws, accumulate=False,
               dout2: Optional[torch.Tensor] = None):
    B, T, Cin, H, W = frames.shape
    F = dweight.shape[0]
    check(lib().nvq_head_wgrad(ptr(frames), B, T, Cin, H, W, int_array(slots), len(slots), ptr(dout),
                               dout.shape[-1], ptr(dout2), dout2.shape[-1] if dout2 is not None else 0, ptr(act),
                               act.shape[-1], F, ptr(dweight), ptr(dbias), ptr(ws),
                               ws.numel() * 4, int(accumulate), is_bf16(act), stream()), "nvq_head_wgrad")


def _bn_input(bn) -> "Optional[BnInput]":
    """bn = (mean, invstd, gamma, beta, group_images) or None."""
    if bn is None:
        return None
    b = BnInput()
    b.mean, b.invstd, b.gamma, b.beta, b.group_images = ptr(bn[0]), ptr(bn[1]), ptr(bn[2]), ptr(bn[3]), int(bn[4])
    return b


def dwconv_bn_fusable(x: torch.Tensor, C: int) -> bool:
    """True when the depthwise kernels can evaluate relu(bn(x)) while staging x (bf16 tensor, C % 64 == 0)."""
    return x.dtype == torch.bfloat16 and C % 64 == 0


def dwconv_forward(x: torch.Tensor, weight, out: torch.Tensor, flip=False, bn=None,
                   add: Optional[torch.Tensor] = None, mask: Optional[torch.Tensor] = None):
    """add (fp32) / mask (fp32 or bf16), both [N,H,W,>=C]: out = (conv + add) where mask > 0 (64-channel bf16 kernels)."""
    N, H, W, ld = x.shape
    Cc = weight.shape[0]
    b = _bn_input(bn)
    e = None
    if add is not None or mask is not None:
        e = DwEpilogue()
        e.add, e.add_ld, e.add_bf16 = ptr(add), add.shape[-1] if add is not None else 0, is_bf16(add)
        e.mask, e.mask_ld, e.mask_bf16 = ptr(mask), mask.shape[-1] if mask is not None else 0, is_bf16(mask)
    check(lib().nvq_dwconv_forward(ptr(x), ld, ptr(weight), Cc, ptr(out), out.shape[-1], N, H, W, int(flip),
                                   is_bf16(x), is_bf16(out), C.byref(b) if b is not None else None,
                                   C.byref(e) if e is not None else None, stream()),
          "nvq_dwconv_forward")


def dwconv_wgrad(x: torch.Tensor, dy: torch.Tensor, dweight, ws, accumulate=False, bn=None):
    N, H, W, ld = x.shape
    Cc = dweight.shape[0]
    b = _bn_input(bn)
    check(lib().nvq_dwconv_wgrad(ptr(x), ld, ptr(dy), dy.shape[-1], Cc, N, H, W, ptr(dweight), ptr(ws),
                                 ws.numel() * 4, int(accumulate), is_bf16(x), is_bf16(dy),
                                 C.byref(b) if b is not None else None, stream()), "nvq_dwconv_wgrad")


def bn_stats(x: torch.Tensor, group_images: int, order: Sequence[int], mean, invstd, rmean, rvar, ws,
             eps=1e-5, momentum=0.1):
    N, H, W, ld = x.shape
    Cc = mean.shape[-1]
    check(lib().nvq_bn_stats(ptr(x), ld, Cc, N, group_images, H, W, eps, momentum, int_array(order), ptr(mean),
                             ptr(invstd), ptr(rmean), ptr(rvar), ptr(ws), ws.numel() * 4, is_bf16(x), stream()),
          "nvq_bn_stats")


def bn_eval_stats(rmean, rvar, G: int, mean, invstd, eps=1e-5):
    check(lib().nvq_bn_eval_stats(ptr(rmean), ptr(rvar), rmean.numel(), G, eps, ptr(mean), ptr(invstd), stream()),
          "nvq_bn_eval_stats")


def bn_apply_relu(x: torch.Tensor, group_images: int, mean, invstd, gamma, beta, res: Optional[torch.Tensor],
                  outA: Sl, split_images: int, outB: Optional[Sl] = None):
    N, H, W, ld = x.shape
    Cc = gamma.numel()
    check(lib().nvq_bn_apply_relu(ptr(x), ld, Cc, N, group_images, H, W, ptr(mean), ptr(invstd), ptr(gamma),
                                  ptr(beta), ptr(res), res.shape[-1] if res is not None else 0, ptr(outA.t),
                                  outA.ld, outA.coff, split_images, ptr(outB.t) if outB else None,
                                  outB.ld if outB else 0, outB.coff if outB else 0, is_bf16(x), outA.bf16, is_bf16(res),
                                  stream()),
          "nvq_bn_apply_relu")


def bn_relu_backward(dy: torch.Tensor, x: torch.Tensor, group_images: int, mean, invstd, gamma, beta,
                     training: bool, dx: torch.Tensor, dgamma, dbeta, ws, accumulate=False):
    N, H, W, ld = x.shape
    Cc = gamma.numel()
    check(lib().nvq_bn_relu_backward(ptr(dy), dy.shape[-1], ptr(x), ld, Cc, N, group_images, H, W, ptr(mean),
                                     ptr(invstd), ptr(gamma), ptr(beta), int(training), ptr(dx), dx.shape[-1],
                                     ptr(dgamma), ptr(dbeta), ptr(ws), ws.numel() * 4, int(accumulate), is_bf16(dy),
                                     is_bf16(x), is_bf16(dx), stream()),
          "nvq_bn_relu_backward")


def dwconv_backward(x: torch.Tensor, bn, dy: torch.Tensor, weight: torch.Tensor, dx: torch.Tensor, dweight, ws,
                    add: Optional[torch.Tensor] = None, mask: Optional[torch.Tensor] = None, bn_sums=None, bn_dgamma=None,
                    bn_dbeta=None) -> None:
    """Input and weight gradient of a 64-channel depthwise 3x3 conv from one staged tile (bf16 mode): see nvq_dwconv_backward.
    bn = (mean, invstd, gamma, beta, group_images): the conv was fed relu(bn(x)); add (fp32) / mask (bf16): dx = (dx + add)
    where mask > 0.  bn_sums [G, 2, 64] (+ bn_dgamma, bn_dbeta [64]): also return the backward sums of that BatchNorm (its input is
    x, the gradient of its activation is dx) - pw_bn_backward(..., sums_in=bn_sums) then skips its reduce pass.
    dweight None (a frozen depthwise weight): dx alone, nvq_dwconv_backward_ex(NVQ_NO_WGRAD)."""
    N, H, W, ld = x.shape
    assert x.dtype == dy.dtype == dx.dtype == torch.bfloat16 and weight.shape[0] == 64
    b = _bn_input(bn)
    e = None
    if add is not None or mask is not None:
        e = DwEpilogue()
        e.add, e.add_ld, e.add_bf16 = ptr(add), add.shape[-1] if add is not None else 0, is_bf16(add)
        e.mask, e.mask_ld, e.mask_bf16 = ptr(mask), mask.shape[-1] if mask is not None else 0, is_bf16(mask)
    args = (ptr(x), ld, C.byref(b) if b is not None else None, ptr(dy), dy.shape[-1], ptr(weight.contiguous()), ptr(dx),
            dx.shape[-1], C.byref(e) if e is not None else None, N, H, W, ptr(dweight), ptr(bn_sums), ptr(bn_dgamma),
            ptr(bn_dbeta), ptr(ws), ws.numel() * 4)
    if dweight is None:
        check(lib().nvq_dwconv_backward_ex(*args, NO_WGRAD, stream()), "nvq_dwconv_backward_ex")
        return
    check(lib().nvq_dwconv_backward(*args, stream()), "nvq_dwconv_backward")


def dwpw_forward(x: torch.Tensor, bn, dw_weight: torch.Tensor, pw_weight: torch.Tensor, d: torch.Tensor, p: torch.Tensor,
                 group_images: int, order: Optional[Sequence[int]], mean, invstd, rmean, rvar, ws, eps=1e-5,
                 momentum=0.1) -> None:
    """depthwise 3x3 -> pointwise 1x1 -> BatchNorm statistics in one pass (bf16 mode, 64 channels): see nvq_dwpw_forward.
    bn = (mean, invstd, gamma, beta, group_images) of the previous layer or None; order None: no statistics (eval mode)."""
    N, H, W, ld = x.shape
    assert x.dtype == d.dtype == p.dtype == torch.bfloat16 and tuple(pw_weight.shape[:2]) == (64, 64)
    b = _bn_input(bn)
    stats = order is not None
    ev0 = TIMER.start() if TIMER is not None else None
    check(lib().nvq_dwpw_forward(ptr(x), ld, C.byref(b) if b is not None else None, ptr(dw_weight.contiguous()),
                                 ptr(pw_weight.contiguous()), ptr(d), d.shape[-1], ptr(p), p.shape[-1], N, group_images, H, W,
                                 int(stats), eps, momentum, int_array(order) if stats else None, ptr(mean) if stats else None,
                                 ptr(invstd) if stats else None, ptr(rmean) if stats else None, ptr(rvar) if stats else None,
                                 ptr(ws), ws.numel() * 4, stream()), "nvq_dwpw_forward")
    if ev0 is not None:
        npx = N * H * W
        TIMER.stop(ev0, "dwpw_fwd_kernel", 2.0 * npx * 64 * (64 + 9), npx * 64 * 2.0 * 3, f"n{N} 64->64")


def pw_bn_backward(dy: torch.Tensor, p: torch.Tensor, d: torch.Tensor, group_images: int, mean, invstd, gamma, beta,
                   training: bool, weight: torch.Tensor, dd: torch.Tensor, dgamma, dbeta, dweight, ws, sums_in=None,
                   recompute: bool = False) -> None:
    """Backward of pointwise conv -> BatchNorm -> ReLU in one pass (bf16 mode, 64 channels): see nvq_pw_bn_backward.
    dweight None (a frozen pointwise weight) and / or dgamma, dbeta None (a frozen BatchNorm affine): nvq_pw_bn_backward_ex,
    dd is the same either way.  recompute: p is dwpw_forward's output on this d and this weight (NVQ_PW_RECOMPUTE) - the
    pass behind the BatchNorm sums forms it again from d instead of reading it (the library does so with a bf16 dy and a
    weight gradient; any other call reads p)."""
    N, H, W, _ = p.shape
    assert p.dtype == d.dtype == dd.dtype == torch.bfloat16 and tuple(weight.shape[:2]) == (64, 64)
    ev0 = TIMER.start() if TIMER is not None else None
    args = (ptr(dy), dy.shape[-1], is_bf16(dy), ptr(p), p.shape[-1], ptr(d), d.shape[-1], N, group_images, H, W, ptr(mean),
            ptr(invstd), ptr(gamma), ptr(beta), int(training), ptr(weight.contiguous()), ptr(dd), dd.shape[-1], ptr(dgamma),
            ptr(dbeta), ptr(dweight), ptr(sums_in), ptr(ws), ws.numel() * 4)
    if dweight is None or dgamma is None or dbeta is None or recompute:
        flags = (NO_WGRAD if dweight is None else 0) | (PW_RECOMPUTE if recompute else 0)
        check(lib().nvq_pw_bn_backward_ex(*args, flags, stream()), "nvq_pw_bn_backward_ex")
    else:
        check(lib().nvq_pw_bn_backward(*args, stream()), "nvq_pw_bn_backward")
    if ev0 is not None:
        npx = N * H * W
        TIMER.stop(ev0, "pw_bn_bwd_kernel", 2.0 * npx * 64 * 64 * 2,
                   npx * 64 * (2.0 * (1 if recompute and dweight is not None and is_bf16(dy) else 2)
                               + (2 if is_bf16(dy) else 4) * 2 + 2), f"n{N} 64->64 {'h' if is_bf16(dy) else 'f'}")


# ----------------------------------------------------------------------------- synchronised BatchNorm (reduce / finish)
# Forward stats buffers: fp64 [G * 2 * C + G] = {sum x, sum x^2} per (group, channel), then the G pixel counts; backward sums:
# fp64 [G * 2 * C] = {sum g, sum g xhat}.  The caller all-reduces them between the two phases (see include/nvq.h).
def new_bn_stats(dev, G: int, Cc: int) -> torch.Tensor:
    return torch.empty(G * 2 * Cc + G, dtype=torch.float64, device=dev)


def bn_counts(stats: torch.Tensor, G: int, Cc: int) -> torch.Tensor:
    """the G pixel counts at the end of a forward stats buffer (what the backward finish phases read)"""
    return stats[G * 2 * Cc:]


def bn_stats_reduce(x: torch.Tensor, group_images: int, stats: torch.Tensor, ws) -> None:
    N, H, W, ld = x.shape
    Cc = (stats.numel() // (N // group_images) - 1) // 2
    check(lib().nvq_bn_stats_reduce(ptr(x), ld, Cc, N, group_images, H, W, ptr(stats), ptr(ws), ws.numel() * 4, is_bf16(x),
                                    stream()), "nvq_bn_stats_reduce")


def bn_stats_finish(stats: torch.Tensor, G: int, order: Sequence[int], mean, invstd, rmean, rvar, eps=1e-5,
                    momentum=0.1) -> None:
    check(lib().nvq_bn_stats_finish(ptr(stats), mean.shape[-1], G, eps, momentum, int_array(order), ptr(mean), ptr(invstd),
                                    ptr(rmean), ptr(rvar), stream()), "nvq_bn_stats_finish")


def dwpw_forward_sums(x: torch.Tensor, bn, dw_weight: torch.Tensor, pw_weight: torch.Tensor, d: torch.Tensor, p: torch.Tensor,
                      group_images: int, stats: torch.Tensor, ws) -> None:
    """dwpw_forward whose statistics leave as sums (nvq_dwpw_forward_sums)"""
    N, H, W, ld = x.shape
    assert x.dtype == d.dtype == p.dtype == torch.bfloat16 and tuple(pw_weight.shape[:2]) == (64, 64)
    b = _bn_input(bn)
    check(lib().nvq_dwpw_forward_sums(ptr(x), ld, C.byref(b) if b is not None else None, ptr(dw_weight.contiguous()),
                                      ptr(pw_weight.contiguous()), ptr(d), d.shape[-1], ptr(p), p.shape[-1], N, group_images, H,
                                      W, ptr(stats), ptr(ws), ws.numel() * 4, stream()), "nvq_dwpw_forward_sums")


def bn_relu_backward_reduce(dy: torch.Tensor, x: torch.Tensor, group_images: int, mean, invstd, gamma, beta,
                            sums: torch.Tensor, dgamma, dbeta, ws, accumulate=False) -> None:
    N, H, W, ld = x.shape
    check(lib().nvq_bn_relu_backward_reduce(ptr(dy), dy.shape[-1], ptr(x), ld, gamma.numel(), N, group_images, H, W, ptr(mean),
                                            ptr(invstd), ptr(gamma), ptr(beta), ptr(sums), ptr(dgamma), ptr(dbeta), ptr(ws),
                                            ws.numel() * 4, int(accumulate), is_bf16(dy), is_bf16(x), stream()),
          "nvq_bn_relu_backward_reduce")


def bn_relu_backward_finish(dy: torch.Tensor, x: torch.Tensor, group_images: int, mean, invstd, gamma, beta,
                            sums: torch.Tensor, count: torch.Tensor, dx: torch.Tensor) -> None:
    N, H, W, ld = x.shape
    check(lib().nvq_bn_relu_backward_finish(ptr(dy), dy.shape[-1], ptr(x), ld, gamma.numel(), N, group_images, H, W, ptr(mean),
                                            ptr(invstd), ptr(gamma), ptr(beta), ptr(sums), ptr(count), ptr(dx), dx.shape[-1],
                                            is_bf16(dy), is_bf16(x), is_bf16(dx), stream()), "nvq_bn_relu_backward_finish")


def pw_bn_backward_reduce(dy: torch.Tensor, p: torch.Tensor, group_images: int, mean, invstd, gamma, beta,
                          sums: torch.Tensor, dgamma, dbeta, ws) -> None:
    N, H, W, _ = p.shape
    assert p.dtype == torch.bfloat16
    check(lib().nvq_pw_bn_backward_reduce(ptr(dy), dy.shape[-1], is_bf16(dy), ptr(p), p.shape[-1], N, group_images, H, W,
                                          ptr(mean), ptr(invstd), ptr(gamma), ptr(beta), ptr(sums), ptr(dgamma), ptr(dbeta),
                                          ptr(ws), ws.numel() * 4, stream()), "nvq_pw_bn_backward_reduce")


def pw_bn_backward_finish(dy: torch.Tensor, p: torch.Tensor, d: torch.Tensor, group_images: int, mean, invstd, gamma, beta,
                          weight: torch.Tensor, dd: torch.Tensor, dweight, sums: torch.Tensor, count: torch.Tensor, ws,
                          recompute: bool = False) -> None:
    """recompute: as in pw_bn_backward"""
    N, H, W, _ = p.shape
    assert p.dtype == d.dtype == dd.dtype == torch.bfloat16 and tuple(weight.shape[:2]) == (64, 64)
    check(lib().nvq_pw_bn_backward_finish(ptr(dy), dy.shape[-1], is_bf16(dy), ptr(p), p.shape[-1], ptr(d), d.shape[-1], N,
                                          group_images, H, W, ptr(mean), ptr(invstd), ptr(gamma), ptr(beta),
                                          ptr(weight.contiguous()), ptr(dd), dd.shape[-1], ptr(dweight), ptr(sums), ptr(count),
                                          ptr(ws), ws.numel() * 4,
                                          (NO_WGRAD if dweight is None else 0) | (PW_RECOMPUTE if recompute else 0), stream()),
          "nvq_pw_bn_backward_finish")


# ----------------------------------------------------------------------------- motion
def correlation_forward(x1: Sl, x2: Sl, out: torch.Tensor, math: int = MATH_F32):
    """x1 / x2: fp32, or (MATH_BF16, C in {32, 64}) both bf16-stored feature tensors."""
    N, H, W, _ = x1.t.shape
    assert x1.bf16 == x2.bf16
    check(lib().nvq_correlation_forward(x1.base(), x1.ld, x2.base(), x2.ld, x2.n, x1.c, N, H, W, ptr(out),
                                        out.shape[-1], math, is_bf16(out), x1.bf16, stream()), "nvq_correlation_forward")


def correlation_backward(which: int, dcorr: torch.Tensor, other: Sl, dx: Sl, accumulate: bool, math: int = MATH_F32,
                         groups: int = 1, out16: Optional[torch.Tensor] = None, addends: Sequence[Sl] = ()):
    """groups > 1 (which == 2): dcorr / other hold groups * N images, frame-major; dx (N images) collects all of them in
    one pass.  out16 (bf16 [N/groups, H, W, >= C]): the finished gradient is written there as bf16 instead of back to dx;
    addends (with out16): up to two bf16 slices added in the same pass (accumulate False: dx is not read)."""
    N, H, W, ld = dcorr.shape
    assert N % groups == 0 and (out16 is None or out16.dtype == torch.bfloat16) and len(addends) <= 2
    ad = None
    if addends:
        assert out16 is not None and all(a.bf16 for a in addends)
        ad = CorrAddends()
        ad.a, ad.a_ld, ad.a_coff = ptr(addends[0].t), addends[0].ld, addends[0].coff
        if len(addends) > 1:
            ad.b, ad.b_ld, ad.b_coff = ptr(addends[1].t), addends[1].ld, addends[1].coff
    check(lib().nvq_correlation_backward(which, ptr(dcorr), ld, other.base(), other.ld, other.n, other.c, N // groups, H, W,
                                         ptr(dx.t), dx.ld, dx.coff, int(accumulate), math, is_bf16(dcorr), other.bf16,
                                         groups, ptr(out16), out16.shape[-1] if out16 is not None else 0,
                                         C.byref(ad) if ad is not None else None, stream()),
          "nvq_correlation_backward")


def warp_forward(feat: Sl, flow: torch.Tensor, out: Sl):
    N, H, W, _ = feat.t.shape
    check(lib().nvq_warp_forward(feat.base(), feat.ld, ptr(flow), flow.shape[-1], feat.c, N, H, W, ptr(out.t),
                                 out.ld, out.coff, feat.bf16, out.bf16, stream()), "nvq_warp_forward")


WARP_DETERMINISTIC = 1
NO_WGRAD = 2        # NVQ_NO_WGRAD: the _ex entry points' input gradient without the weight gradient
PW_RECOMPUTE = 4    # NVQ_PW_RECOMPUTE: nvq_pw_bn_backward_ex / _finish form p again from d instead of reading it


def warp_backward(dout: Sl, feat: Sl, flow: torch.Tensor, dfeat: Sl, dflow: torch.Tensor, gather: bool = True,
                  overwrite: bool = False, deterministic: bool = False):
    """gather=True: atomics-free two-pass form (needs 20 B of scratch per pixel, allocated here); False: scatter form.
    overwrite: dfeat is written instead of added to (gather form): no zero fill before, no read-modify-write here.
    deterministic (gather form, overwrite mode): no float atomics for any flow either (nvq_warp_backward_ex: the far sources
    are binned and gathered; a bf16 dfeat is rounded once); its workspace is allocated here too."""
    N, H, W, _ = feat.t.shape
    rec = torch.empty(N * H * W * 5 + 4, dtype=torch.float32, device=flow.device) if gather else None
    if deterministic:
        nbytes = int(lib().nvq_warp_backward_workspace_bytes(N, H, W, WARP_DETERMINISTIC))
        ws = torch.empty((nbytes + 3) // 4, dtype=torch.int32, device=flow.device)
        check(lib().nvq_warp_backward_ex(ptr(dout.t), dout.ld, dout.coff, feat.base(), feat.ld, ptr(flow),
                                         flow.shape[-1], feat.c, N, H, W, dfeat.base(), dfeat.ld, ptr(dflow),
                                         dflow.shape[-1], ptr(rec), rec.numel() * 4 if rec is not None else 0, feat.bf16,
                                         dout.bf16, int(overwrite), dfeat.bf16, WARP_DETERMINISTIC, ptr(ws), ws.numel() * 4,
                                         stream()),
              "nvq_warp_backward_ex")
        return
    check(lib().nvq_warp_backward(ptr(dout.t), dout.ld, dout.coff, feat.base(), feat.ld, ptr(flow),
                                  flow.shape[-1], feat.c, N, H, W, dfeat.base(), dfeat.ld, ptr(dflow),
                                  dflow.shape[-1], ptr(rec), rec.numel() * 4 if rec is not None else 0, feat.bf16, dout.bf16,
                                  int(overwrite), dfeat.bf16, stream()),
          "nvq_warp_backward")


# ----------------------------------------------------------------------------- aggregation
def tsum_blocks(H: int, W: int) -> int:
    return int(lib().nvq_tsum_blocks(H, W))


def tsum_forward(aligned: torch.Tensor, logits: torch.Tensor, T: int, Cc: int, attn, weighted, gap_partial):
    N, H, W, ld = aligned.shape
    check(lib().nvq_tsum_forward(ptr(aligned), ld, ptr(logits), logits.shape[-1], T, Cc, N, H, W, ptr(attn),
                                 attn.shape[-1], ptr(weighted), weighted.shape[-1], ptr(gap_partial), is_bf16(aligned),
                                 is_bf16(weighted), stream()),
          "nvq_tsum_forward")


def tsum_backward(dweighted, dgap_pix, aligned, attn, T: int, Cc: int, daligned, dlogits):
    N, H, W, ld = aligned.shape
    check(lib().nvq_tsum_backward(ptr(dweighted), dweighted.shape[-1], ptr(dgap_pix), ptr(aligned), ld, ptr(attn),
                                  attn.shape[-1], T, Cc, N, H, W, ptr(daligned), daligned.shape[-1], ptr(dlogits),
                                  dlogits.shape[-1], is_bf16(aligned), is_bf16(daligned), is_bf16(dweighted), stream()),
          "nvq_tsum_backward")


def cbam_channel(gap_partial, nblk, Cc, R, N, HW, w1, w2, gap, hid, ca):
    check(lib().nvq_cbam_channel(ptr(gap_partial), nblk, Cc, R, N, HW, ptr(w1), ptr(w2), ptr(gap), ptr(hid),
                                 ptr(ca), stream()), "nvq_cbam_channel")


def cbam_pool(x: torch.Tensor, ca, sm, amax):
    N, H, W, ld = x.shape
    check(lib().nvq_cbam_pool(ptr(x), ld, ptr(ca), ca.shape[-1], N, H, W, ptr(sm), ptr(amax), is_bf16(x), stream()),
          "nvq_cbam_pool")


def cbam_spatial_apply(x: torch.Tensor, ca, sm, w7, sa, out: Sl):
    N, H, W, ld = x.shape
    check(lib().nvq_cbam_spatial_apply(ptr(x), ld, ptr(ca), ptr(sm), ptr(w7), ca.shape[-1], N, H, W, ptr(sa),
                                       ptr(out.t), out.ld, out.coff, out.bf16, is_bf16(x), stream()), "nvq_cbam_spatial_apply")


def cbam_bwd_spatial_pre(dout: Sl, x: torch.Tensor, ca, sa, dpre):
    N, H, W, ld = x.shape
    assert dout.bf16 == is_bf16(x), "dout and x are stored alike"
    check(lib().nvq_cbam_bwd_spatial_pre(ptr(dout.t), dout.ld, dout.coff, ptr(x), ld, ptr(ca), ptr(sa),
                                         ca.shape[-1], N, H, W, ptr(dpre), is_bf16(x), stream()), "nvq_cbam_bwd_spatial_pre")


def cbam_bwd_spatial_conv(dpre, sm, w7, dsm, dw7, ws, accumulate=False):
    """dw7 None (a frozen spatial-attention conv): dsm alone (nvq_cbam_bwd_spatial_conv_ex, NVQ_NO_WGRAD)"""
    N, H, W = dpre.shape[:3]
    if dw7 is None:
        check(lib().nvq_cbam_bwd_spatial_conv_ex(ptr(dpre), ptr(sm), ptr(w7), N, H, W, ptr(dsm), None, ptr(ws), ws.numel() * 4,
                                                 int(accumulate), NO_WGRAD, stream()), "nvq_cbam_bwd_spatial_conv_ex")
        return
    check(lib().nvq_cbam_bwd_spatial_conv(ptr(dpre), ptr(sm), ptr(w7), N, H, W, ptr(dsm), ptr(dw7), ptr(ws),
                                          ws.numel() * 4, int(accumulate), stream()), "nvq_cbam_bwd_spatial_conv")


def cbam_bwd_scale(dout: Sl, x: torch.Tensor, ca, sa, dsm, amax, dx: torch.Tensor, dca_partial):
    N, H, W, ld = x.shape
    assert dout.bf16 == is_bf16(x) == is_bf16(dx), "dout, x and dx are stored alike"
    check(lib().nvq_cbam_bwd_scale(ptr(dout.t), dout.ld, dout.coff, ptr(x), ld, ptr(ca), ptr(sa), ptr(dsm),
                                   ptr(amax), ca.shape[-1], N, H, W, ptr(dx), dx.shape[-1], ptr(dca_partial),
                                   is_bf16(x), stream()), "nvq_cbam_bwd_scale")


def cbam_bwd_channel(dca_partial, nblk, Cc, R, N, HW, w1, w2, gap, hid, ca, dw1, dw2, dgap_pix, accumulate=False):
    """dw1 and dw2 None (a frozen channel attention): dgap_pix alone (nvq_cbam_bwd_channel_ex, NVQ_NO_WGRAD)"""
    if dw1 is None and dw2 is None:
        check(lib().nvq_cbam_bwd_channel_ex(ptr(dca_partial), nblk, Cc, R, N, HW, ptr(w1), ptr(w2), ptr(gap), ptr(hid), ptr(ca),
                                            None, None, ptr(dgap_pix), int(accumulate), NO_WGRAD, stream()),
              "nvq_cbam_bwd_channel_ex")
        return
    check(lib().nvq_cbam_bwd_channel(ptr(dca_partial), nblk, Cc, R, N, HW, ptr(w1), ptr(w2), ptr(gap), ptr(hid),
                                     ptr(ca), ptr(dw1), ptr(dw2), ptr(dgap_pix), int(accumulate), stream()),
          "nvq_cbam_bwd_channel")


# ----------------------------------------------------------------------------- upsampler tail
def upsampler_tail_forward(x: Sl, wpack: torch.Tensor, bias: torch.Tensor, frames: torch.Tensor, t_center: int, s: int, out,
                           passmask) -> None:
    """conv3x3(x -> Cimg*s*s) + PixelShuffle(s) + bicubic skip + clamp in one launch (bf16 mode, bf16 x)."""
    B, T, Cimg, H, W = frames.shape
    n, h, w, _ = x.t.shape
    assert (n, h, w) == (B, H, W)
    ev0 = TIMER.start() if TIMER is not None else None
    d = ConvDesc()
    d.inp, d.in_ld, d.in_coff, d.cin = ptr(x.t), x.ld, x.coff, x.c
    d.wpack, d.bias = ptr(wpack), ptr(bias)
    d.cout = d.cout_store = Cimg * s * s
    d.n, d.h, d.w, d.ksize, d.alpha, d.math, d.in_bf16 = n, h, w, 3, 1.0, MATH_BF16, x.bf16
    check(lib().nvq_upsampler_tail_forward(C.byref(d), ptr(frames), T, t_center, Cimg, s, ptr(out), ptr(passmask), stream()),
          "nvq_upsampler_tail_forward")
    if ev0 is not None:
        U = Cimg * s * s
        TIMER.stop(ev0, "upsampler_tail_kernel", 2.0 * n * h * w * x.c * 9 * U,
                   n * h * w * (x.c * 2.0 + Cimg * 4.0 + Cimg * s * s * 5.0), f"n{n} cin{x.c}h s{s}")


def shuffle_bicubic_clamp(u: torch.Tensor, frames: torch.Tensor, t_center: int, s: int, out, passmask):
    B, T, Cimg, H, W = frames.shape
    check(lib().nvq_shuffle_bicubic_clamp(ptr(u), u.shape[-1], ptr(frames), B, T, t_center, Cimg, H, W, s,
                                          ptr(out), ptr(passmask), stream()), "nvq_shuffle_bicubic_clamp")


def shuffle_clamp_backward(dout: torch.Tensor, passmask, s: int, du: torch.Tensor):
    B, Cimg, OH, OW = dout.shape
    check(lib().nvq_shuffle_clamp_backward(ptr(dout), ptr(passmask), B, Cimg, OH // s, OW // s, s, ptr(du),
                                           du.shape[-1], stream()), "nvq_shuffle_clamp_backward")


def bicubic_blend(sr: torch.Tensor, frames: torch.Tensor, t_center: int, s: int, strength: float, out: torch.Tensor):
    B, T, Cimg, H, W = frames.shape
    check(lib().nvq_bicubic_blend(ptr(sr), ptr(frames), B, T, t_center, Cimg, H, W, s, float(strength), ptr(out),
                                  stream()), "nvq_bicubic_blend")


def head_dgrad(dout: torch.Tensor, weight, B: int, slots: Sequence[int], dframes: torch.Tensor,
               act: Optional[torch.Tensor] = None, dout2: Optional[torch.Tensor] = None, accumulate: bool = False):
    """dframes (B,T,Cin,H,W) (+)= input gradient of the head conv for the images of `dout` ([len(slots)*B,H,W,ld], slot
    order).  act None: dout is the ReLU-masked gradient; else (dout + dout2) masked by act > 0."""
    _, T, Cin, H, W = dframes.shape
    F = weight.shape[0]
    check(lib().nvq_head_dgrad(ptr(dout), dout.shape[-1], is_bf16(dout), ptr(dout2),
                               dout2.shape[-1] if dout2 is not None else 0, ptr(act), act.shape[-1] if act is not None else 0,
                               is_bf16(act), ptr(weight), F, B, T, Cin, H, W, int_array(slots), len(slots), ptr(dframes),
                               int(accumulate), stream()), "nvq_head_dgrad")


def bicubic_adjoint(dout: torch.Tensor, passmask: Optional[torch.Tensor], s: int, t_center: int, coef: float,
                    dframes: torch.Tensor, accumulate: bool = False):
    """dframes[:, t_center] (+)= coef * bicubic_s^T(dout * passmask); dout (B,C,H*s,W*s), dframes (B,T,C,H,W)."""
    B, T, Cimg, H, W = dframes.shape
    assert tuple(dout.shape) == (B, Cimg, H * s, W * s) and dout.dtype == torch.float32
    assert passmask is None or (passmask.shape == dout.shape and passmask.dtype == torch.uint8)
    check(lib().nvq_bicubic_adjoint(ptr(dout), ptr(passmask), B, Cimg, H, W, s, T, t_center, float(coef), ptr(dframes),
                                    int(accumulate), stream()), "nvq_bicubic_adjoint")


def head_dgrad_tc(dout: torch.Tensor, weight, B: int, slots: Sequence[int], coffs: Sequence[int], slot_images: int,
                  dframes: torch.Tensor, accumulate: bool = False):
    """dframes (B,T,Cin,H,W) (+)= input gradient of a 3x3 conv (weight [F,Cin,3,3]) for the pre-masked gradient `dout`
    ([N,H,W,ld]): slot s = frame slots[s], read from images s * slot_images + b at channels coffs[s] .. + F."""
    _, T, Cin, H, W = dframes.shape
    check(lib().nvq_head_dgrad_tc(ptr(dout), dout.shape[-1], is_bf16(dout), ptr(weight), weight.shape[0], B, T, Cin, H, W,
                                  int_array(slots), int_array(coffs), len(slots), slot_images, ptr(dframes), int(accumulate),
                                  stream()), "nvq_head_dgrad_tc")


def stem7_dgrad(dy: torch.Tensor, weight, dframe: Optional[torch.Tensor], dmask: Optional[torch.Tensor], H: int, W: int,
                accumulate: bool = False):
    """input gradient of nn.Conv2d(4, Co, 7, 2, 3) (weight [Co,4,7,7]) for dy [N,OH,OW,ld]: channels 0..2 (+)= into
    dframe (N,3,H,W), channel 3 into dmask (N,1,H,W); either may be None"""
    N = dy.shape[0]
    for t, c in ((dframe, 3), (dmask, 1)):
        assert t is None or (tuple(t.shape) == (N, c, H, W) and t.dtype == torch.float32)
    check(lib().nvq_stem7_dgrad(ptr(dy), dy.shape[-1], is_bf16(dy), ptr(weight), N, H, W, weight.shape[0], ptr(dframe),
                                ptr(dmask), int(accumulate), stream()), "nvq_stem7_dgrad")


def mask_blend_backward_ex(dout: torch.Tensor, frame: torch.Tensor, rec: torch.Tensor, mask: torch.Tensor, drec: torch.Tensor,
                           dframe: Optional[torch.Tensor], dmask: Optional[torch.Tensor]):
    """backward of out = frame * (1 - m) + rec * m: drec [N,H,W,ld] = dout * m, dframe = dout * (1 - m),
    dmask = sum_c dout * (rec - frame) (dframe / dmask None: not written)"""
    N, C, H, W = dout.shape
    check(lib().nvq_mask_blend_backward_ex(ptr(dout), ptr(frame), ptr(rec), rec.shape[-1], ptr(mask), N, C, H, W, ptr(drec),
                                           ptr(dframe), ptr(dmask), stream()), "nvq_mask_blend_backward_ex")


# ----------------------------------------------------------------------------- helpers
def axpy_slice(dst: Sl, src: Sl, alpha: float = 1.0, accumulate: bool = True, mask: Optional[Sl] = None):
    npix = dst.t.shape[0] * dst.t.shape[1] * dst.t.shape[2]
    assert dst.c == src.c
    check(lib().nvq_axpy_slice(ptr(dst.t), dst.ld, dst.coff, ptr(src.t), src.ld, src.coff,
                               ptr(mask.t) if mask else None, mask.ld if mask else 0, mask.coff if mask else 0,
                               dst.c, npix, alpha, int(accumulate), src.bf16, stream()), "nvq_axpy_slice")


def colsum(x: Sl, out: torch.Tensor, ws, alpha=1.0, accumulate=False):
    npix = x.t.shape[0] * x.t.shape[1] * x.t.shape[2]
    check(lib().nvq_colsum(ptr(x.t), x.ld, x.coff, x.c, npix, alpha, ptr(out), ptr(ws), ws.numel() * 4,
                           int(accumulate), stream()), "nvq_colsum")


# ----------------------------------------------------------------------------- loss
def mse_forward(a: torch.Tensor, b: torch.Tensor, out: torch.Tensor, ws: torch.Tensor):
    check(lib().nvq_mse_forward(ptr(a), ptr(b), a.numel(), ptr(out), ptr(ws), ws.numel() * 4, stream()), "nvq_mse_forward")


def mse_backward(a: torch.Tensor, b: torch.Tensor, go_dev: Optional[torch.Tensor], da: torch.Tensor):
    check(lib().nvq_mse_backward(ptr(a), ptr(b), a.numel(), ptr(go_dev), ptr(da), stream()), "nvq_mse_backward")


LOSS_L1, LOSS_CHARBONNIER, LOSS_MSE = 0, 1, 2   # NVQ_LOSS_*


def quality_sums(x: torch.Tensor, y: torch.Tensor, out: torch.Tensor, ws: torch.Tensor):
    """out (B, 8) float64: per sample n and the seven sums of nvq_quality_sums; x, y (B, ...) fp32"""
    B = x.shape[0]
    check(lib().nvq_quality_sums(ptr(x), ptr(y), B, x.numel() // B, ptr(out), ptr(ws), ws.numel() * 4, stream()),
          "nvq_quality_sums")


def pixel_loss_forward(x: torch.Tensor, y: torch.Tensor, kind: int, eps: float, out: torch.Tensor, ws: torch.Tensor):
    """out (G,): G = 1 the mean over the whole tensor, G = x.shape[0] the mean over each sample"""
    G = out.numel()
    check(lib().nvq_pixel_loss_forward(ptr(x), ptr(y), G, x.numel() // G, kind, eps, ptr(out), ptr(ws), ws.numel() * 4,
                                       stream()), "nvq_pixel_loss_forward")


def pixel_loss_backward(x: torch.Tensor, y: torch.Tensor, kind: int, eps: float, go_dev: torch.Tensor, dx: torch.Tensor):
    G = go_dev.numel()
    check(lib().nvq_pixel_loss_backward(ptr(x), ptr(y), G, x.numel() // G, kind, eps, ptr(go_dev), ptr(dx), stream()),
          "nvq_pixel_loss_backward")


def ssim_forward(x: torch.Tensor, y: torch.Tensor, data_range: float, as_loss: bool, out: torch.Tensor, ws: torch.Tensor):
    """x, y (B, C, H, W) fp32; out (B,) per sample or (1,) over the batch"""
    B, Cc, H, W = x.shape
    check(lib().nvq_ssim_forward(ptr(x), ptr(y), B, Cc, H, W, data_range, int(out.numel() != 1 or B == 1), int(as_loss),
                                 ptr(out), ptr(ws), ws.numel() * 4, stream()), "nvq_ssim_forward")


def ssim_backward(x: torch.Tensor, y: torch.Tensor, data_range: float, go_dev: torch.Tensor, scale: float, dx: torch.Tensor):
    """dx = scale * go * d(mean SSIM) / dx; go_dev (B,) per sample or (1,) for the batch mean"""
    B, Cc, H, W = x.shape
    check(lib().nvq_ssim_backward(ptr(x), ptr(y), B, Cc, H, W, data_range, ptr(go_dev), int(go_dev.numel() != 1 or B == 1),
                                  scale, ptr(dx), stream()), "nvq_ssim_backward")


def avgpool2_pair(x: torch.Tensor, y: torch.Tensor, px: torch.Tensor, py: torch.Tensor):
    """px, py (..., H // 2, W // 2) = the 2 x 2 means of x, y (..., H, W), both in one launch"""
    H, W = x.shape[-2:]
    check(lib().nvq_avgpool2_pair(ptr(x), ptr(y), x.numel() // (H * W), H, W, ptr(px), ptr(py), stream()), "nvq_avgpool2_pair")


def msssim_scale_forward(xs: torch.Tensor, ys: torch.Tensor, H: int, W: int, scales: int, scale: int, data_range: float,
                         ws: torch.Tensor):
    """tile sums of scale `scale` of an M-scale pyramid whose finest planes are H x W; xs, ys: that scale's (B, C, h, w)"""
    check(lib().nvq_msssim_scale_forward(ptr(xs), ptr(ys), xs.shape[0] * xs.shape[1], H, W, scales, scale, data_range, ptr(ws),
                                         ws.numel() * 4, stream()), "nvq_msssim_scale_forward")


def msssim_finalize(ws: torch.Tensor, B: int, Cc: int, H: int, W: int, weights: torch.Tensor, as_loss: bool, out: torch.Tensor,
                    mtable: torch.Tensor, dtable: torch.Tensor):
    """out (B,) per sample or (1,) over the batch; mtable, dtable (M, B * C); weights (M,) on the device"""
    check(lib().nvq_msssim_finalize(ptr(ws), B, Cc, H, W, weights.numel(), ptr(weights), int(out.numel() != 1 or B == 1),
                                    int(as_loss), ptr(out), ptr(mtable), ptr(dtable), stream()), "nvq_msssim_finalize")


def msssim_scale_backward(xs: torch.Tensor, ys: torch.Tensor, H: int, W: int, scales: int, scale: int, data_range: float,
                          dtable: torch.Tensor, go_dev: torch.Tensor, sign: float, dx_coarser: Optional[torch.Tensor],
                          dx: torch.Tensor):
    """dx = sign * go * d ms / d xs through m_scale, plus the pooling adjoint of dx_coarser; go_dev (B,) or (1,)"""
    B, Cc = xs.shape[:2]
    check(lib().nvq_msssim_scale_backward(ptr(xs), ptr(ys), B, Cc, H, W, scales, scale, data_range, ptr(dtable), ptr(go_dev),
                                          int(go_dev.numel() != 1 or B == 1), sign, ptr(dx_coarser), ptr(dx), stream()),
          "nvq_msssim_scale_backward")


# ----------------------------------------------------------------------------- distillation
def distill_forward(s: torch.Tensor, t: torch.Tensor, y: Optional[torch.Tensor], wt: float, wy: float, out: torch.Tensor,
                    ws: torch.Tensor):
    """out (3, G): wt d + wy m, d = mean (s - t)^2, m = mean (s - y)^2 (0 without y); G = 1 the whole tensor, G = s.shape[0]
    one column per sample"""
    G = out.shape[1]
    check(lib().nvq_distill_forward(ptr(s), ptr(t), ptr(y), G, s.numel() // G, wt, wy, ptr(out), ptr(ws), ws.numel() * 4,
                                    stream()), "nvq_distill_forward")


def distill_backward(s: torch.Tensor, t: torch.Tensor, y: Optional[torch.Tensor], wt: float, wy: float, go_dev: torch.Tensor,
                     ds: torch.Tensor):
    G = go_dev.numel()
    check(lib().nvq_distill_backward(ptr(s), ptr(t), ptr(y), G, s.numel() // G, wt, wy, ptr(go_dev), ptr(ds), stream()),
          "nvq_distill_backward")


def cosine_distill_forward(s: torch.Tensor, t: torch.Tensor, eps: float, per_sample: bool, out: torch.Tensor, ws: torch.Tensor):
    """s, t (B, C, H, W) fp32; out (B,) per sample or (1,) over the batch"""
    B, Cc, H, W = s.shape
    check(lib().nvq_cosine_distill_forward(ptr(s), ptr(t), B, Cc, H * W, eps, int(per_sample), ptr(out), ptr(ws),
                                           ws.numel() * 4, stream()), "nvq_cosine_distill_forward")


def cosine_distill_backward(s: torch.Tensor, t: torch.Tensor, eps: float, go_dev: torch.Tensor, per_sample: bool,
                            ds: torch.Tensor):
    """go_dev (B,) per sample or (1,) for the batch mean"""
    B, Cc, H, W = s.shape
    check(lib().nvq_cosine_distill_backward(ptr(s), ptr(t), B, Cc, H * W, eps, ptr(go_dev), int(per_sample), ptr(ds), stream()),
          "nvq_cosine_distill_backward")


# ----------------------------------------------------------------------------- EWC
def ewc_penalty(theta, star, fisher, lam: float, out, ws):
    check(lib().nvq_ewc_penalty(ptr(theta), ptr(star), ptr(fisher), theta.numel(), lam, ptr(out), ptr(ws),
                                ws.numel() * 4, stream()), "nvq_ewc_penalty")


def ewc_penalty_grad(theta, star, fisher, lam: float, scale_dev, grad, accumulate: bool):
    check(lib().nvq_ewc_penalty_grad(ptr(theta), ptr(star), ptr(fisher), theta.numel(), lam, ptr(scale_dev),
                                     ptr(grad), int(accumulate), stream()), "nvq_ewc_penalty_grad")


def si_update(theta, grad, p_old, W):
    check(lib().nvq_si_update(ptr(theta), ptr(grad), theta.numel(), ptr(p_old), ptr(W), stream()), "nvq_si_update")


def si_consolidate(theta, damping: float, p_old, W, omega):
    check(lib().nvq_si_consolidate(ptr(theta), theta.numel(), damping, ptr(p_old), ptr(W), ptr(omega), stream()),
          "nvq_si_consolidate")


def fisher_accumulate(grad, fisher):
    check(lib().nvq_fisher_accumulate(ptr(grad), grad.numel(), ptr(fisher), stream()), "nvq_fisher_accumulate")


def _bucket_acc(acc: torch.Tensor) -> int:
    assert acc.dtype == torch.float64 and acc.numel() >= 5, "acc: 5 float64 slots (g.r, r.r, g.g, c, projections)"
    return ptr(acc)


def bucket_moments(g: torch.Tensor, r: Optional[torch.Tensor], acc: torch.Tensor, ws: torch.Tensor, accumulate: bool = False,
                   coefficient: bool = False):
    """acc[0..2] (+)= g.r, r.r, g.g over two flat fp32 tensors (r None: g.g only); ``coefficient``: also the A-GEM decision
    acc[3] = c, acc[4] += (c != 0) (nvq_bucket_moments)"""
    assert g.dtype == torch.float32 and (r is None or (r.dtype == torch.float32 and r.numel() == g.numel()))
    check(lib().nvq_bucket_moments(ptr(g), ptr(r), g.numel(), _bucket_acc(acc), int(accumulate), int(coefficient), ptr(ws),
                                   ws.numel() * 4, stream()), "nvq_bucket_moments")


def bucket_project(g: torch.Tensor, r: torch.Tensor, acc: torch.Tensor):
    """g -= acc[3] * r in place (untouched when acc[3] == 0)"""
    assert g.dtype == torch.float32 and r.dtype == torch.float32 and r.numel() == g.numel()
    check(lib().nvq_bucket_project(ptr(g), ptr(r), g.numel(), _bucket_acc(acc), stream()), "nvq_bucket_project")


GEM_MAX_TASKS = 15


def _gem_rows(refs: torch.Tensor, T: int, g: torch.Tensor, what: str) -> int:
    """row stride of the [rows >= T][stride] fp32 reference matrix whose first T rows go with the flat fp32 gradient g"""
    assert 1 <= T <= GEM_MAX_TASKS and refs.dim() == 2 and refs.shape[0] >= T, f"{what}: 1 .. {GEM_MAX_TASKS} reference rows"
    assert g.dtype == torch.float32 and g.dim() == 1, f"{what}: g is a flat fp32 tensor"
    return _rows_stride(refs, g.numel(), what)


def gem_gram(refs: torch.Tensor, T: int, g: torch.Tensor, gram: torch.Tensor, ws: torch.Tensor, accumulate: bool = False) -> None:
    """gram[i, j] (+)= row_i . row_j for the first T rows of refs and g as row T; 16 x 16 float64, symmetric bit for bit, zero
    outside (T + 1)^2 (nvq_gem_gram)"""
    stride = _gem_rows(refs, T, g, "gem_gram")
    assert gram.dtype == torch.float64 and gram.numel() == 256, "gram: 16 x 16 float64"
    check(lib().nvq_gem_gram(refs.data_ptr(), stride, int(T), ptr(g), g.numel(), ptr(gram), int(accumulate), ptr(ws),
                             ws.numel() * ws.element_size(), stream()), "nvq_gem_gram")


def gem_solve(gram: torch.Tensor, T: int, margin: float, eps: float, eps_relative: bool, v: torch.Tensor, stats: torch.Tensor) -> None:
    """v (16 float64) = GEM's multipliers from the Gram, zeros when nothing is violated; stats: the 8 float64 slots (nvq_gem_solve)"""
    assert gram.dtype == torch.float64 and gram.numel() == 256, "gram: 16 x 16 float64"
    assert v.dtype == torch.float64 and v.numel() >= 16 and stats.dtype == torch.float64 and stats.numel() >= 8, \
        "v: 16 float64, stats: 8 float64 slots"
    check(lib().nvq_gem_solve(ptr(gram), int(T), float(margin), float(eps), int(eps_relative), ptr(v), ptr(stats), stream()),
          "nvq_gem_solve")


def gem_project(g: torch.Tensor, refs: torch.Tensor, T: int, v: torch.Tensor) -> None:
    """g += sum_t v[t] refs[t] in place, in double, rounded once; untouched when v == 0 (nvq_gem_project)"""
    stride = _gem_rows(refs, T, g, "gem_project")
    assert v.dtype == torch.float64 and v.numel() >= 16, "v: 16 float64"
    check(lib().nvq_gem_project(ptr(g), refs.data_ptr(), stride, int(T), g.numel(), ptr(v), stream()), "nvq_gem_project")


def bucket_clip(g: torch.Tensor, acc: torch.Tensor, max_norm: float, norm_out: Optional[torch.Tensor]):
    """g *= max_norm / (sqrt(acc[2]) + 1e-6) in place when that is < 1; norm_out (fp32 device scalar) = sqrt(acc[2])"""
    assert g.dtype == torch.float32
    check(lib().nvq_bucket_clip(ptr(g), g.numel(), _bucket_acc(acc), float(max_norm), ptr(norm_out), stream()),
          "nvq_bucket_clip")


def adam_step(theta: torch.Tensor, grad: torch.Tensor, exp_avg: torch.Tensor, exp_avg_sq: torch.Tensor,
              ema: Optional[torch.Tensor], *, lr: float, beta1: float, beta2: float, eps: float, weight_decay: float,
              decoupled: bool, step: int, ema_decay: float = 0.0, acc: Optional[torch.Tensor] = None, max_norm: float = 0.0):
    """One Adam / AdamW step number ``step`` (>= 1) on flat fp32 tensors in place (nvq_adam_step): optional clipping from
    ``acc`` (the 5 float64 slots of bucket_moments; ``grad`` is not written) and optional weight EMA.  The bias corrections
    and 1 - beta are formed here in double, as torch forms its scalars."""
    n = theta.numel()
    for t in (theta, grad, exp_avg, exp_avg_sq) + ((ema,) if ema is not None else ()):
        assert t.dtype == torch.float32 and t.numel() == n, "adam_step: fp32 tensors of one size"
    bias1 = 1.0 - beta1 ** step
    bias2_sqrt = (1.0 - beta2 ** step) ** 0.5
    check(lib().nvq_adam_step(ptr(theta), ptr(grad), ptr(exp_avg), ptr(exp_avg_sq), ptr(ema), n, lr, beta1, beta2, 1.0 - beta1,
                              1.0 - beta2, eps, weight_decay, int(decoupled), bias1, bias2_sqrt, ema_decay,
                              _bucket_acc(acc) if acc is not None else None, max_norm, stream()), "nvq_adam_step")


# ----------------------------------------------------------------------------- device-resident episodic memory
REPLAY_MEANS_ONLY = 1   # NVQ_REPLAY_MEANS_ONLY


def require_replay_device(dev: torch.device) -> None:
    """DeviceEpisodicMemory keeps its tables in HBM and moves samples with libnvq kernels only."""
    if dev.type != "cuda":
        raise RuntimeError(
            f"DeviceEpisodicMemory on {dev}: the device-resident memory runs only as HIP kernels on an AMD GPU; there is "
            "no CPU fallback (nerve_cl.continual.EpisodicMemory is the host-side store).")
    lib()


def replay_store(src_lr: torch.Tensor, src_hr: torch.Tensor, slots: torch.Tensor, imps: torch.Tensor, times: torch.Tensor,
                 types: torch.Tensor, lr_store: torch.Tensor, hr_store: torch.Tensor, means: torch.Tensor,
                 importance: torch.Tensor, time: torch.Tensor, access: torch.Tensor, type_id: torch.Tensor) -> None:
    """src_lr / src_hr (n, ...) fp32 -> rows slots[j] of the (capacity, ...) fp32 or bf16 stores; the per-slot tables are
    written by the same call (nvq_replay_store).  slots / times / types int32 (n,), imps fp32 (n,), all on the device."""
    n, cap = src_lr.shape[0], lr_store.shape[0]
    check(lib().nvq_replay_store(ptr(src_lr), ptr(src_hr), n, src_lr.numel() // n, src_hr.numel() // n, means.shape[1],
                                 ptr(slots), ptr(imps), ptr(times), ptr(types), ptr(lr_store), ptr(hr_store),
                                 is_bf16(lr_store), cap, ptr(means), ptr(importance), ptr(time), ptr(access), ptr(type_id), 0,
                                 stream()), "nvq_replay_store")


def replay_means(src_lr: torch.Tensor, out: torch.Tensor) -> None:
    """out (n, C) = per-channel means of src_lr (n, C, ...): nvq_replay_store's mean pass alone, the same bits"""
    n = src_lr.shape[0]
    slots = torch.arange(n, dtype=torch.int32, device=src_lr.device)
    check(lib().nvq_replay_store(ptr(src_lr), None, n, src_lr.numel() // n, 1, out.shape[1], ptr(slots), None, None, None,
                                 None, None, 0, n, ptr(out), None, None, None, None, REPLAY_MEANS_ONLY, stream()),
          "nvq_replay_store(means)")


def replay_gather(lr_store: torch.Tensor, hr_store: torch.Tensor, idx: torch.Tensor, lr_batch: torch.Tensor,
                  hr_batch: torch.Tensor, row0: int, access: torch.Tensor) -> None:
    """rows [row0, row0 + k) of the fp32 batches = slots idx (int32 (k,), device) of the stores, one launch"""
    k, cap = idx.numel(), lr_store.shape[0]
    if row0 < 0 or row0 + k > lr_batch.shape[0] or lr_batch.shape[0] != hr_batch.shape[0]:
        raise ValueError(f"replay_gather: rows [{row0}, {row0 + k}) outside a batch of {lr_batch.shape[0]}")
    assert lr_batch.dtype == torch.float32 and hr_batch.dtype == torch.float32 and idx.dtype == torch.int32
    assert lr_batch.shape[1:] == lr_store.shape[1:] and hr_batch.shape[1:] == hr_store.shape[1:]
    check(lib().nvq_replay_gather(ptr(lr_store), ptr(hr_store), is_bf16(lr_store), cap, lr_store.numel() // cap,
                                  hr_store.numel() // cap, ptr(idx), k, ptr(lr_batch), ptr(hr_batch), row0, ptr(access),
                                  stream()), "nvq_replay_gather")


def replay_sample_weighted(importance: torch.Tensor, time: torch.Tensor, type_id: torch.Tensor, now: int,
                           recency_weight: float, type_filter: int, uniforms: torch.Tensor, out_idx: torch.Tensor) -> None:
    """out_idx (k,) int32 = the k slots with the largest keys log(u_i) / w_i (nvq_replay_sample_weighted), -1 padded"""
    assert uniforms.dtype == torch.float32 and uniforms.numel() == importance.numel() and out_idx.dtype == torch.int32
    check(lib().nvq_replay_sample_weighted(ptr(importance), ptr(time), ptr(type_id), importance.numel(), now, recency_weight,
                                           type_filter, ptr(uniforms), out_idx.numel(), ptr(out_idx), stream()),
          "nvq_replay_sample_weighted")


def replay_update_importance(importance: torch.Tensor, idx: torch.Tensor, values: torch.Tensor, momentum: float) -> None:
    """importance[idx[j]] = momentum * importance[idx[j]] + (1 - momentum) * values[j]; non-finite values are skipped"""
    assert idx.dtype == torch.int32 and values.dtype == torch.float32 and idx.numel() == values.numel()
    check(lib().nvq_replay_update_importance(ptr(importance), importance.numel(), ptr(idx), ptr(values), idx.numel(), momentum,
                                             stream()), "nvq_replay_update_importance")


def replay_nearest(query: Optional[torch.Tensor], table: torch.Tensor, type_id: torch.Tensor, out: torch.Tensor) -> None:
    """out (2,) int32 = [slot, bits of the fp32 distance]: the non-empty slot whose table row is nearest to `query`, or
    (query None, table (capacity,)) whose table value is smallest"""
    assert out.dtype == torch.int32 and out.numel() == 2
    cap = type_id.numel()
    check(lib().nvq_replay_nearest(ptr(query), ptr(table), ptr(type_id), cap, table.numel() // cap, ptr(out), ptr(out, 1),
                                   stream()), "nvq_replay_nearest")


# ----------------------------------------------------------------------------- drift detection (csrc/drift.hip)
def _rows(x: torch.Tensor, index: Optional[torch.Tensor]) -> int:
    assert x.dtype == torch.float32 and x.dim() == 2, "rbf_gram_sum: (rows, d) fp32 matrices"
    assert index is None or (index.dtype == torch.int32 and index.dim() == 1), "rbf_gram_sum: int32 row indices"
    return x.shape[0] if index is None else index.numel()


def rbf_gram_sum(a: torch.Tensor, b: torch.Tensor, out: torch.Tensor, ws: torch.Tensor, *, a_index: Optional[torch.Tensor] = None,
                 b_index: Optional[torch.Tensor] = None, gamma: Optional[torch.Tensor] = None, symmetric: bool = False) -> None:
    """out (one float64 element) = sum_ij exp(-gamma |a_i - b_j|^2) over the rows of a, b (rows, d) fp32, or over the rows the
    int32 index tensors name; gamma: a float64 device scalar, None = 1 / d (nvq_rbf_gram_sum)"""
    na, nb = _rows(a, a_index), _rows(b, b_index)
    assert a.shape[1] == b.shape[1] and out.dtype == torch.float64 and out.numel() == 1
    assert gamma is None or (gamma.dtype == torch.float64 and gamma.numel() == 1)
    check(lib().nvq_rbf_gram_sum(ptr(a), ptr(b), ptr(a_index), ptr(b_index), na, nb, a.shape[0], b.shape[0], a.shape[1], ptr(gamma),
                                 int(symmetric), ptr(out), ptr(ws), ws.numel() * ws.element_size(), stream()), "nvq_rbf_gram_sum")


def mmd_finish(sums: torch.Tensor, na: int, nb: int, threshold: float, score: torch.Tensor, flag: torch.Tensor) -> None:
    """score (float64 scalar), flag (bool scalar) from sums (3,) float64 = sum K(a,a), sum K(b,b), sum K(a,b)"""
    assert sums.dtype == torch.float64 and sums.numel() == 3 and score.dtype == torch.float64 and flag.dtype == torch.bool
    check(lib().nvq_mmd_finish(ptr(sums), na, nb, float(threshold), ptr(score), ptr(flag), stream()), "nvq_mmd_finish")


def psi_counts(x: torch.Tensor, edges: torch.Tensor, counts: torch.Tensor) -> None:
    """counts (edges - 1,) int32 = np.histogram(x, bins=edges)[0]; x flat fp32, edges float64 on the device"""
    assert x.dtype == torch.float32 and edges.dtype == torch.float64 and counts.dtype == torch.int32
    assert counts.numel() == edges.numel() - 1
    check(lib().nvq_psi_counts(ptr(x), x.numel(), ptr(edges), edges.numel(), ptr(counts), stream()), "nvq_psi_counts")


def psi_finish(cur_counts: torch.Tensor, ref_counts: torch.Tensor, len_cur: int, len_ref: int, score: torch.Tensor,
               flag: torch.Tensor) -> None:
    assert cur_counts.dtype == torch.int32 and ref_counts.dtype == torch.int32 and cur_counts.numel() == ref_counts.numel()
    assert score.dtype == torch.float64 and flag.dtype == torch.bool
    check(lib().nvq_psi_finish(ptr(cur_counts), ptr(ref_counts), cur_counts.numel(), len_cur, len_ref, ptr(score), ptr(flag),
                               stream()), "nvq_psi_finish")


def cell_descriptor(x: torch.Tensor, gh: int, gw: int, out: torch.Tensor) -> None:
    """out (B, 2 * C * gh * gw) fp32 = per-cell means, then per-cell population standard deviations of x (B, C, H, W) fp32"""
    B, Cc, H, W = x.shape
    assert x.dtype == torch.float32 and out.dtype == torch.float32 and tuple(out.shape) == (B, 2 * Cc * gh * gw)
    check(lib().nvq_cell_descriptor(ptr(x), B, Cc, H, W, gh, gw, ptr(out), stream()), "nvq_cell_descriptor")


def metric_window_update(value: torch.Tensor, ring: torch.Tensor, state: torch.Tensor, baseline: float, threshold: float,
                         mean: torch.Tensor, flag: torch.Tensor) -> None:
    """push the fp32 device scalar `value` into `ring`; state (2,) int32; mean float64 scalar, flag bool scalar"""
    assert value.dtype == torch.float32 and value.numel() == 1 and ring.dtype == torch.float32
    assert state.dtype == torch.int32 and state.numel() == 2 and mean.dtype == torch.float64 and flag.dtype == torch.bool
    check(lib().nvq_metric_window_update(ptr(value), ptr(ring), ptr(state), ring.numel(), float(baseline), float(threshold),
                                         ptr(mean), ptr(flag), stream()), "nvq_metric_window_update")


# ----------------------------------------------------------------------------- Kolmogorov-Smirnov drift test (csrc/ks.hip)
KS_MAX_N = 4096     # rows of one set: a column is sorted in LDS


def sort_columns(x: torch.Tensor, index: Optional[torch.Tensor], out: torch.Tensor) -> None:
    """out (d, n) fp32 = the ascending columns of x (rows, d) fp32, or of the n rows the int32 index tensor names"""
    n = _rows(x, index)
    assert out.dtype == torch.float32 and tuple(out.shape) == (x.shape[1], n)
    check(lib().nvq_sort_columns(ptr(x), ptr(index), n, x.shape[0], x.shape[1], ptr(out), stream()), "nvq_sort_columns")


def ks_statistic(ref_sorted: torch.Tensor, cur_sorted: torch.Tensor, h: torch.Tensor, stat: torch.Tensor) -> None:
    """h (d,) int32 = lcm(n1, n2) times the two-sided statistic of every feature, stat (d,) float64 the statistic, from
    ascending columns (d, n1) and (d, n2) fp32"""
    d, n1 = ref_sorted.shape
    assert ref_sorted.dtype == torch.float32 and cur_sorted.dtype == torch.float32 and cur_sorted.shape[0] == d
    assert h.dtype == torch.int32 and stat.dtype == torch.float64 and h.numel() == d and stat.numel() == d
    check(lib().nvq_ks_statistic(ptr(ref_sorted), ptr(cur_sorted), n1, cur_sorted.shape[1], d, ptr(h), ptr(stat), stream()),
          "nvq_ks_statistic")


def ks_pvalue(h: torch.Tensor, n1: int, n2: int, p: torch.Tensor) -> None:
    """p (d,) float64 = the exact two-sided p-value of every h (d,) int32 for sets of n1 and n2 values"""
    assert h.dtype == torch.int32 and p.dtype == torch.float64 and h.numel() == p.numel()
    check(lib().nvq_ks_pvalue(ptr(h), n1, n2, h.numel(), ptr(p), stream()), "nvq_ks_pvalue")


def ks_finish(p: torch.Tensor, threshold: float, score: torch.Tensor, flag: torch.Tensor) -> None:
    """score (float64 scalar) = p.numel() * min(p), flag (bool scalar) = score < threshold, compared in double"""
    assert p.dtype == torch.float64 and score.dtype == torch.float64 and flag.dtype == torch.bool
    thr = C.c_double(float(threshold))                                  # read by the library before the call returns
    check(lib().nvq_ks_finish(ptr(p), p.numel(), C.byref(thr), ptr(score), ptr(flag), stream()), "nvq_ks_finish")


# ----------------------------------------------------------------------------- federated rounds and differential privacy
FED_MAX_CLIENTS = 64
DP_CHUNK_QUADS = 1024   # quads per block of the per-slot kernels: 4 per thread


def fed_workspace_bytes(K: int, n: int) -> int:
    return int(lib().nvq_fed_workspace_bytes(int(K), int(n)))


def _fed_rows(clients: torch.Tensor, n: int) -> "tuple[int, int]":
    """(K, row stride) of the client matrix"""
    assert 1 <= clients.shape[0] <= FED_MAX_CLIENTS and n >= 0, "clients: 1 .. 64 rows"
    return clients.shape[0], _rows_stride(clients, n, "clients")


def _fed_vectors(K: int, n: int, weights=None, sq=None, out=None, base=None) -> None:
    """the per-client tables (float64, K values) and the vectors (fp32, n floats) of an aggregate wrapper, each if given"""
    assert all(t is None or (t.dtype == torch.float64 and t.numel() >= K) for t in (weights, sq)), "weights / sq: K float64 values"
    assert all(t is None or (t.dtype == torch.float32 and t.numel() >= n) for t in (out, base)), "out / base: fp32 vectors of n floats"


def fed_delta_norms(clients: torch.Tensor, n: int, base: Optional[torch.Tensor], sq: torch.Tensor, ws: torch.Tensor) -> None:
    """sq[k] = sum_i (clients[k, i] - base[i])^2 over the first n columns, in double (base None: the rows' own norms)"""
    K, stride = _fed_rows(clients, n)
    _fed_vectors(K, n, sq=sq, base=base)
    check(lib().nvq_fed_delta_norms(clients.data_ptr(), stride, K, ptr(base), n, ptr(sq), ptr(ws), ws.numel() * 4, stream()),
          "nvq_fed_delta_norms")


def fed_aggregate(clients: torch.Tensor, n: int, base: Optional[torch.Tensor], weights: torch.Tensor, sq: Optional[torch.Tensor],
                  out: torch.Tensor, *, clip_norm: float = 0.0, server_lr: float = 1.0, noise_std: float = 0.0, seed: int = 0,
                  offset: int = 0) -> None:
    """out[i] = base[i] + server_lr * sum_k c_k (clients[k, i] - base[i]) + noise_std * z_i (nvq_fed_aggregate); ``out`` may be
    ``base``"""
    K, stride = _fed_rows(clients, n)
    _fed_vectors(K, n, weights, sq, out, base)
    check(lib().nvq_fed_aggregate(clients.data_ptr(), stride, K, ptr(base), ptr(weights), ptr(sq), float(clip_norm),
                                  float(server_lr), float(noise_std), int(seed), int(offset), n, ptr(out), stream()),
          "nvq_fed_aggregate")


class DpTable:
    """The device tables of the per-slot DP kernels for one bucket layout: slot offsets and sizes (int64), the chunk triples
    (slot, first quad, quads) with at most DP_CHUNK_QUADS quads each, sorted by slot, and the norms sq (float64)."""

    def __init__(self, offsets: Sequence[int], numels: Sequence[int], device):
        assert len(offsets) == len(numels) >= 1
        chunks, end = [], 0
        for s, (o, k) in enumerate(zip(offsets, numels)):
            if o % 4 or o < end or k < 0:
                raise ValueError(f"slot {s} at float offset {o} ({k} floats): slots start at multiples of 4 floats and do not overlap")
            end = o + k
            q, nq = o // 4, (k + 3) // 4
            for c in range(0, nq, DP_CHUNK_QUADS):
                chunks.append((s, q + c, min(DP_CHUNK_QUADS, nq - c)))
        if not chunks:
            raise ValueError("every slot is empty")
        self.total = (end + 3) // 4 * 4
        self.S, self.n_chunks = len(offsets), len(chunks)
        self.seg_off = torch.tensor(list(offsets), dtype=torch.int64).to(device)
        self.seg_numel = torch.tensor(list(numels), dtype=torch.int64).to(device)
        self.chunks = torch.tensor(chunks, dtype=torch.int32).to(device)
        self.sq = torch.zeros(self.S, dtype=torch.float64, device=device)


def _dp_bucket(g: torch.Tensor, table: DpTable) -> int:
    assert g.dtype == torch.float32 and g.numel() >= table.total, "the bucket is fp32 and covers every slot of the table"
    return ptr(g)


def dp_segment_norms(g: torch.Tensor, table: DpTable, ws: torch.Tensor) -> None:
    """table.sq[s] = sum of g^2 over slot s (nvq_dp_segment_norms)"""
    check(lib().nvq_dp_segment_norms(_dp_bucket(g, table), ptr(table.seg_off), ptr(table.seg_numel), table.S, ptr(table.chunks),
                                     table.n_chunks, ptr(table.sq), ptr(ws), ws.numel() * 4, stream()), "nvq_dp_segment_norms")


def dp_clip_noise(g: torch.Tensor, table: DpTable, max_norm: float, noise_scale: float, seed: int, offset: int) -> None:
    """per slot: g = g * min(max_norm / (sqrt(sq) + 1e-6), 1) + noise_scale * z in place, padding kept 0 (nvq_dp_clip_noise)"""
    check(lib().nvq_dp_clip_noise(_dp_bucket(g, table), ptr(table.seg_off), ptr(table.seg_numel), table.S, ptr(table.chunks),
                                  table.n_chunks, ptr(table.sq), float(max_norm), float(noise_scale), int(seed), int(offset),
                                  stream()), "nvq_dp_clip_noise")


# ----------------------------------------------------------------------------- clustered federated learning
CLUSTER_MAX = 8


def fed_gram_workspace_bytes(K: int, n: int) -> int:
    return int(lib().nvq_fed_gram_workspace_bytes(int(K), int(n)))


def _rows_stride(m: torch.Tensor, n: int, what: str) -> int:
    """row stride of a [R][stride] fp32 matrix with rows of at least n floats (a one-row matrix: any stride >= n serves)"""
    assert m.dtype == torch.float32 and m.dim() == 2 and m.stride(1) == 1 and m.shape[1] >= n, f"{what}: a [rows][stride] fp32 matrix"
    require_device(m, what)
    stride = m.stride(0) if m.shape[0] > 1 else max(m.stride(0), m.shape[1])
    assert stride >= n, f"{what}: row stride {stride} < n {n}"
    return stride


def fed_update_gram(clients: torch.Tensor, n: int, base: Optional[torch.Tensor], gram: torch.Tensor, ws: torch.Tensor) -> None:
    """gram[i, j] = sum_t (clients[i, t] - base[t]) (clients[j, t] - base[t]) over the first n columns (nvq_fed_update_gram)"""
    K, stride = _fed_rows(clients, n)
    assert gram.dtype == torch.float64 and gram.numel() >= K * K and (base is None or (base.dtype == torch.float32 and base.numel() >= n))
    check(lib().nvq_fed_update_gram(clients.data_ptr(), stride, K, ptr(base), n, ptr(gram), ptr(ws), ws.numel() * ws.element_size(),
                                    stream()), "nvq_fed_update_gram")


def cluster_gram_kmeans(gram: torch.Tensor, K: int, C: int, init: Optional[torch.Tensor], max_iter: int, labels: torch.Tensor,
                        counts: torch.Tensor, inertia: torch.Tensor, n_iter: torch.Tensor) -> None:
    """Lloyd's algorithm from the K x K float64 Gram matrix alone (nvq_cluster_gram_kmeans); every output stays on the device"""
    assert gram.dtype == torch.float64 and gram.numel() >= K * K and (init is None or (init.dtype == torch.int32 and init.numel() >= C))
    assert labels.dtype == torch.int32 and labels.numel() >= K and counts.dtype == torch.int32 and counts.numel() >= C
    assert inertia.dtype == torch.float64 and inertia.numel() >= 1 and n_iter.dtype == torch.int32 and n_iter.numel() >= 1
    check(lib().nvq_cluster_gram_kmeans(ptr(gram), int(K), int(C), ptr(init), int(max_iter), ptr(labels), ptr(counts), ptr(inertia),
                                        ptr(n_iter), stream()), "nvq_cluster_gram_kmeans")


def fed_aggregate_clusters(clients: torch.Tensor, n: int, labels: torch.Tensor, C: int, bases: Optional[torch.Tensor],
                           weights: torch.Tensor, sq: Optional[torch.Tensor], out: torch.Tensor, *, clip_norm: float = 0.0,
                           server_lr: float = 1.0, noise_std: float = 0.0, seed: int = 0, offset: int = 0) -> None:
    """out[c] = base_c + server_lr * sum_{k: labels[k] == c} c_k (clients[k] - base_c) + noise_std * z (nvq_fed_aggregate_clusters).
    ``bases``: None (zeros), a vector (one shared base) or a [C][stride] matrix (one base per cluster; ``out`` may be it)."""
    K, stride = _fed_rows(clients, n)
    assert labels.dtype == torch.int32 and labels.numel() >= K and 1 <= C <= CLUSTER_MAX
    assert out.shape[0] == C, "out: one row per cluster"
    out_stride = _rows_stride(out, n, "out")
    base_stride = 0
    if bases is not None and bases.dim() == 2:
        assert bases.shape[0] == C, "bases: one row per cluster"
        base_stride = _rows_stride(bases, n, "bases")
    _fed_vectors(K, n, weights, sq, base=bases if base_stride == 0 else None)
    check(lib().nvq_fed_aggregate_clusters(clients.data_ptr(), stride, K, ptr(labels), int(C),
                                           None if bases is None else bases.data_ptr(), base_stride, ptr(weights), ptr(sq),
                                           float(clip_norm), float(server_lr), float(noise_std), int(seed), int(offset), n,
                                           out.data_ptr(), out_stride, stream()), "nvq_fed_aggregate_clusters")


# ----------------------------------------------------------------------------- Byzantine-robust aggregation (csrc/robust.hip)
FED_TRIM_MEDIAN = 64    # NVQ_FED_TRIM_MEDIAN: a trim of (K - 1) / 2 or more is the coordinate-wise median


def fed_trimmed_aggregate(clients: torch.Tensor, n: int, base: Optional[torch.Tensor], weights: Optional[torch.Tensor], trim: int,
                          out: torch.Tensor, *, server_lr: float = 1.0, noise_std: float = 0.0, seed: int = 0,
                          offset: int = 0) -> None:
    """out[i] = base[i] + server_lr * (trimmed mean over the live rows of clients[k, i] - base[i]) + noise_std * z_i
    (nvq_fed_trimmed_aggregate); a row is live when ``weights`` is None or weights[k] > 0; ``out`` may be ``base``"""
    K, stride = _fed_rows(clients, n)
    _fed_vectors(K, n, weights, None, out, base)
    check(lib().nvq_fed_trimmed_aggregate(clients.data_ptr(), stride, K, ptr(base), ptr(weights), int(trim), float(server_lr),
                                          float(noise_std), int(seed), int(offset), n, ptr(out), stream()),
          "nvq_fed_trimmed_aggregate")


def fed_krum_select(gram: torch.Tensor, K: int, weights: Optional[torch.Tensor], num_byzantine: int, num_selected: int,
                    out_weights: torch.Tensor, scores: torch.Tensor, order: torch.Tensor) -> None:
    """Krum scores, order and 0/1 selection weights from the K x K float64 Gram of the updates (nvq_fed_krum_select); every output
    stays on the device"""
    assert gram.dtype == torch.float64 and gram.numel() >= K * K and 1 <= K <= FED_MAX_CLIENTS
    assert weights is None or (weights.dtype == torch.float64 and weights.numel() >= K)
    assert out_weights.dtype == torch.float64 and out_weights.numel() >= K and scores.dtype == torch.float64 and scores.numel() >= K
    assert order.dtype == torch.int32 and order.numel() >= K
    check(lib().nvq_fed_krum_select(ptr(gram), int(K), ptr(weights), int(num_byzantine), int(num_selected), ptr(out_weights),
                                    ptr(scores), ptr(order), stream()), "nvq_fed_krum_select")


# ----------------------------------------------------------------------------- FedOpt server rules, FedProx (csrc/fedopt.hip)
FED_OPT_AVGM, FED_OPT_ADAGRAD, FED_OPT_ADAM, FED_OPT_YOGI = 0, 1, 2, 3    # NVQ_FED_OPT_*


def fed_server_opt(clients: torch.Tensor, n: int, base: Optional[torch.Tensor], weights: torch.Tensor, sq: Optional[torch.Tensor],
                   rule: int, m: Optional[torch.Tensor], v: Optional[torch.Tensor], out: torch.Tensor, *, clip_norm: float = 0.0,
                   server_lr: float = 1.0, beta1: float = 0.9, beta2: float = 0.99, tau: float = 1e-3, noise_std: float = 0.0,
                   seed: int = 0, offset: int = 0) -> None:
    """out[i] = base[i] + server_lr * step_i + noise_std * z_i, where step is server momentum (FED_OPT_AVGM), Adagrad, Adam or Yogi
    on the pseudo-gradient D_i = sum_k c_k (clients[k, i] - base[i]) and the moments ``m``, ``v`` (fp32, n floats) are stepped in
    place (nvq_fed_server_opt); ``out`` may be ``base``, ``v`` may be None for FED_OPT_AVGM.  The library checks K, the rule, the
    hyper-parameters and the required pointers."""
    for what, t in (("clients", clients), ("base", base), ("m", m), ("v", v), ("out", out)):
        if t is not None:
            require_device(t, f"nvq_fed_server_opt: {what}")
    K, stride = clients.shape[0], _rows_stride(clients, n, "clients")
    _fed_vectors(K, n, weights, sq, out, base)
    assert all(t is None or (t.dtype == torch.float32 and t.numel() >= n) for t in (m, v)), "m / v: fp32 vectors of n floats"
    check(lib().nvq_fed_server_opt(clients.data_ptr(), stride, K, ptr(base), ptr(weights), ptr(sq), float(clip_norm), int(rule),
                                   float(server_lr), float(beta1), float(beta2), float(tau), ptr(m), ptr(v), float(noise_std),
                                   int(seed), int(offset), n, ptr(out), stream()), "nvq_fed_server_opt")


def fed_prox_grad(grad: torch.Tensor, theta: torch.Tensor, anchor: torch.Tensor, mu: float) -> None:
    """grad += mu * (theta - anchor) over flat fp32 buffers of grad.numel() floats, in double, rounded once (nvq_fed_prox_grad)"""
    for what, t in (("grad", grad), ("theta", theta), ("anchor", anchor)):
        require_device(t, f"nvq_fed_prox_grad: {what}")
    n = grad.numel()
    assert all(t.dtype == torch.float32 and t.numel() >= n for t in (grad, theta, anchor)), "grad / theta / anchor: fp32, n floats"
    check(lib().nvq_fed_prox_grad(ptr(grad), ptr(theta), ptr(anchor), n, float(mu), stream()), "nvq_fed_prox_grad")


# ----------------------------------------------------------------------------- compressed client updates (csrc/compress.hip)
FED_COMPRESS_MAX_LEVELS = 32767
FED_COMPRESS_BLOCK_FLOATS = 8192    # floats of a row per workgroup of the compression passes (kCompressQuads quads)


def fed_compress_workspace_bytes(K: int, n: int) -> int:
    return int(lib().nvq_fed_compress_workspace_bytes(int(K), int(n)))


def fed_compress(clients: torch.Tensor, n: int, base: Optional[torch.Tensor], k: int, levels: int, residual: Optional[torch.Tensor],
                 slots: Optional[torch.Tensor], kept: Optional[torch.Tensor], ws: torch.Tensor, *, seed: int = 0,
                 offset: int = 0) -> None:
    """In place per row: a = (x - base) + residual row; the k largest |a| are kept (ties too; k = 0: all), quantised to ``levels``
    steps of the row maximum with the Philox stream (seed, offset + row) (0: not); x' = base + c or base, the residual row receives
    a - (x' - base) (nvq_fed_compress).  ``slots``: K int32 on the device, the residual row of every matrix row (None: the same
    row); ``kept``: K int32."""
    K, stride = _fed_rows(clients, n)
    _fed_vectors(K, n, base=base)
    residual_stride = 0
    if residual is not None:
        residual_stride = _rows_stride(residual, n, "residual")
    assert slots is None or (residual is not None and slots.dtype == torch.int32 and slots.numel() >= K), "slots: K int32 values"
    assert kept is None or (kept.dtype == torch.int32 and kept.numel() >= K), "kept: K int32 values"
    check(lib().nvq_fed_compress(clients.data_ptr(), stride, K, ptr(base), n, int(k), int(levels),
                                 None if residual is None else residual.data_ptr(), residual_stride, ptr(slots), int(seed),
                                 int(offset), ptr(kept), ptr(ws), ws.numel() * ws.element_size(), stream()), "nvq_fed_compress")


# ----------------------------------------------------------------------------- ABR agent (csrc/abr.hip)
ABR_MAX_LAYERS, ABR_MAX_HEADS = 3, 4


def abr_env_reset(state: torch.Tensor, counters: torch.Tensor, obs: torch.Tensor, params: torch.Tensor, nq: int, max_steps: int,
                  seed: int) -> None:
    N = state.shape[0]
    assert state.dtype == torch.float64 and tuple(state.shape) == (N, 8) and counters.dtype == torch.int64 and counters.numel() == N
    assert obs.dtype == torch.float32 and tuple(obs.shape) == (N, 7) and params.dtype == torch.float64 and params.numel() == 2
    check(lib().nvq_abr_env_reset(ptr(state), ptr(counters), ptr(obs), ptr(params), int(nq), int(max_steps), int(seed), N, stream()),
          "nvq_abr_env_reset")


def abr_env_step(state: torch.Tensor, counters: torch.Tensor, actions: torch.Tensor, bitrates: Sequence[int], enh_levels: int,
                 max_steps: int, params: torch.Tensor, seed: int, obs: torch.Tensor, reward: torch.Tensor, terminated: torch.Tensor,
                 truncated: torch.Tensor, info: Optional[torch.Tensor] = None, reward_f32: Optional[torch.Tensor] = None,
                 done_f32: Optional[torch.Tensor] = None, finished: Optional[torch.Tensor] = None) -> None:
    """One step of every environment with the same-step reset (nvq_abr_env_step); every tensor is written in place"""
    N = state.shape[0]
    assert state.dtype == torch.float64 and tuple(state.shape) == (N, 8) and counters.dtype == torch.int64 and counters.numel() == N
    assert actions.dtype == torch.int32 and tuple(actions.shape) == (N, 2), "actions: (N, 2) int32"
    assert obs.dtype == torch.float32 and tuple(obs.shape) == (N, 7) and params.dtype == torch.float64 and params.numel() == 2
    assert reward.dtype == torch.float64 and reward.numel() == N
    for f in (terminated, truncated):
        assert f.dtype in (torch.uint8, torch.bool) and f.numel() == N
    assert info is None or (info.dtype == torch.float64 and tuple(info.shape) == (5, N))
    for f in (reward_f32, done_f32):
        assert f is None or (f.dtype == torch.float32 and f.numel() == N)
    assert finished is None or (finished.dtype == torch.float64 and tuple(finished.shape) == (N, 2))
    check(lib().nvq_abr_env_step(ptr(state), ptr(counters), ptr(actions), int_array(list(bitrates)), len(bitrates), int(enh_levels),
                                 int(max_steps), ptr(params), int(seed), N, ptr(obs), ptr(reward), ptr(terminated), ptr(truncated),
                                 ptr(info), ptr(reward_f32), ptr(done_f32), ptr(finished), stream()), "nvq_abr_env_step")


def abr_dims(hidden: Sequence[int], heads: Sequence[int]):
    """the dims_host table of nvq_abr_act, or None when the counts alone rule the network out"""
    if not 1 <= len(hidden) <= ABR_MAX_LAYERS or not 1 <= len(heads) <= ABR_MAX_HEADS:
        return None
    return int_array([len(hidden)] + list(hidden) + [0] * (ABR_MAX_LAYERS - len(hidden))
                     + [len(heads)] + list(heads) + [0] * (ABR_MAX_HEADS - len(heads)))


def abr_act_supported(obs_dim: int, hidden: Sequence[int], heads: Sequence[int]) -> bool:
    dims = abr_dims(hidden, heads)
    return dims is not None and bool(lib().nvq_abr_act_supported(int(obs_dim), dims))


def abr_act(obs: torch.Tensor, layers: "Sequence[tuple[torch.Tensor, torch.Tensor]]",
            heads: "Sequence[tuple[torch.Tensor, torch.Tensor]]", value_head: "tuple[torch.Tensor, torch.Tensor]",
            counters: Optional[torch.Tensor], seed: int, deterministic: bool, actions: torch.Tensor, log_prob: torch.Tensor,
            value: torch.Tensor, head_out: Optional[torch.Tensor] = None) -> None:
    """layers / heads / value_head: (weight, bias) pairs as nn.Linear holds them (nvq_abr_act reads them in place)"""
    B, obs_dim = obs.shape
    width = obs_dim                           # the kernel strides every weight by the width before it: the shapes must chain
    for group, chained in ((layers, True), (list(heads) + [value_head], False)):
        for w, b in group:
            assert w.dtype == torch.float32 and b.dtype == torch.float32, "nvq_abr_act: fp32 weights and biases"
            assert w.device == obs.device and b.device == obs.device, "nvq_abr_act: weights on the observations' device"
            assert w.dim() == 2 and w.shape[1] == width and tuple(b.shape) == (w.shape[0],), \
                f"nvq_abr_act: a weight of shape {tuple(w.shape)} after a width of {width}"
            if chained:
                width = w.shape[0]
    assert value_head[0].shape[0] == 1, "nvq_abr_act: the value head has one output"
    dims = abr_dims([w.shape[0] for w, _ in layers], [w.shape[0] for w, _ in heads])
    if dims is None:
        raise RuntimeError("nvq_abr_act: unsupported network (1 to 3 hidden layers, 1 to 4 heads)")
    table = (vp * 16)()
    for i, (w, b) in enumerate(layers):
        table[2 * i], table[2 * i + 1] = ptr(w), ptr(b)
    for i, (w, b) in enumerate(heads):
        table[6 + 2 * i], table[7 + 2 * i] = ptr(w), ptr(b)
    table[14], table[15] = ptr(value_head[0]), ptr(value_head[1])
    P = sum(w.shape[0] for w, _ in heads) + 1
    assert obs.dtype == torch.float32 and actions.dtype == torch.int32 and tuple(actions.shape) == (B, len(heads))
    assert log_prob.dtype == torch.float32 and log_prob.numel() == B and value.dtype == torch.float32 and value.numel() == B
    assert counters is None or (counters.dtype == torch.int64 and counters.numel() == B)
    assert head_out is None or (head_out.dtype == torch.float32 and tuple(head_out.shape) == (B, P))
    check(lib().nvq_abr_act(ptr(obs), B, obs_dim, C.cast(table, vp), dims, ptr(counters), int(seed), int(deterministic), ptr(actions),
                            ptr(log_prob), ptr(value), ptr(head_out), stream()), "nvq_abr_act")


def abr_gae(rewards: torch.Tensor, values: torch.Tensor, dones: torch.Tensor, last_values: torch.Tensor, gamma: float, lam: float,
            returns: torch.Tensor, advantages: torch.Tensor) -> None:
    T, N = rewards.shape
    for t in (rewards, values, dones, returns, advantages):
        assert t.dtype == torch.float32 and tuple(t.shape) == (T, N)
    assert last_values.dtype == torch.float32 and last_values.numel() == N
    check(lib().nvq_abr_gae(ptr(rewards), ptr(values), ptr(dones), ptr(last_values), float(gamma), float(lam), T, N, ptr(returns),
                            ptr(advantages), stream()), "nvq_abr_gae")


def abr_adv_stats(adv: torch.Tensor, stats: torch.Tensor) -> None:
    assert adv.dtype == torch.float32 and stats.dtype == torch.float64 and stats.numel() == 2
    check(lib().nvq_abr_adv_stats(ptr(adv), adv.numel(), ptr(stats), stream()), "nvq_abr_adv_stats")


def ppo_loss(head_outputs: torch.Tensor, actions: torch.Tensor, old_log_probs: torch.Tensor, advantages: torch.Tensor,
             adv_stats: torch.Tensor, returns: torch.Tensor, heads: Sequence[int], clip_ratio: float, value_coef: float,
             entropy_coef: float, grad: torch.Tensor, out: torch.Tensor) -> None:
    """out (6 doubles) = loss and statistics, grad = d loss / d head_outputs (nvq_ppo_loss); two launches"""
    M, P = head_outputs.shape
    assert P == sum(heads) + 1, "head_outputs: the heads' logits, then the value"
    assert head_outputs.dtype == torch.float32 and grad.dtype == torch.float32 and grad.shape == head_outputs.shape
    assert actions.dtype == torch.int32 and tuple(actions.shape) == (M, len(heads))
    for t in (old_log_probs, advantages, returns):
        assert t.dtype == torch.float32 and t.numel() == M
    assert adv_stats.dtype == torch.float64 and adv_stats.numel() == 2 and out.dtype == torch.float64 and out.numel() == 6
    nbytes = int(lib().nvq_ppo_loss_workspace_bytes(M))
    ws = torch.empty(nbytes // 8, dtype=torch.float64, device=head_outputs.device)
    check(lib().nvq_ppo_loss(ptr(head_outputs), ptr(actions), ptr(old_log_probs), ptr(advantages), ptr(adv_stats), ptr(returns), M,
                             int_array(list(heads)), len(heads), float(clip_ratio), float(value_coef), float(entropy_coef), ptr(grad),
                             ptr(out), ptr(ws), nbytes, stream()), "nvq_ppo_loss")
