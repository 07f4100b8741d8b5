"""ctypes binding of ``include/coalign_amd.h`` (the C ABI of the gfx950 kernels).

There is NO fallback: if ``coalign_amd/lib/libcoalign_hip.so`` is missing and cannot be built with hipcc the
import of this module's ``lib()`` raises, and every op in :mod:`coalign_amd.ops` raises on non-GPU tensors.
"""
from __future__ import annotations

import ctypes
import os
from ctypes import POINTER, c_char_p, c_double, c_float, c_int, c_int32, c_int64, c_size_t, c_uint8, c_uint32, c_void_p

from . import build as _build

_LIB = None

P = c_void_p  # every device / host buffer crosses the ABI as a plain pointer

# name -> (restype, argtypes); mirrors include/coalign_amd.h one to one
SIGNATURES = {
    "coalign_abi_version": (c_int, []),
    "coalign_status_string": (c_char_p, [c_int]),
    "coalign_last_hip_error": (c_char_p, []),
    "coalign_pillar_scatter_workspace_bytes": (c_size_t, [c_int, c_int, c_int]),
    "coalign_pillar_vfe_scatter": (c_int, [P, P, P, c_int, c_int, P, P, P, P, P, P, c_float, c_int, c_int, c_int,
                                           POINTER(c_double), POINTER(c_double), c_int, c_int, c_int, P, P, P, c_size_t, P]),
    "coalign_pillar_vfe_scatter_nhwc": (c_int, [P, P, P, c_int, c_int, P, P, P, P, P, P, c_float, c_int, c_int, c_int,
                                                POINTER(c_double), POINTER(c_double), c_int, c_int, c_int, P, P, P, c_size_t, P]),
    "coalign_pillar_encode_persistent": (c_int, [P, P, P, c_int, c_int, P, P, P, P, P, P, c_float, c_int, c_int, c_int,
                                                 POINTER(c_double), POINTER(c_double), c_int, c_int, c_int, P, P, c_int, P, P, P]),
    "coalign_pillar_encode_stream": (c_int, [P, P, P, c_int, P, c_int, P, P, P, P, P, P, c_float, c_int, c_int, c_int,
                                             POINTER(c_double), POINTER(c_double), c_int, c_int, c_int, P, P, P, P, c_int, P]),
    "coalign_sparse_canvas_stamp_bytes": (c_size_t, [c_int, c_int, c_int]),
    "coalign_sparse_canvas_state_bytes": (c_size_t, []),
    "coalign_pillar_folded_param_bytes": (c_size_t, []),
    "coalign_pillar_fold_params": (c_int, [P, P, P, P, P, P, c_float, c_int, c_int, P, P]),
    "coalign_pillar_encode_sparse": (c_int, [P, P, P, c_int, P, c_int, P, c_int, c_int, POINTER(c_double), POINTER(c_double),
                                             c_int, c_int, c_int, P, P, P, P]),
    "coalign_pillar_encode_sparse_frame": (c_int, [P, c_int, c_int, P, c_int, c_int, POINTER(c_double), POINTER(c_double), c_int, c_int, c_int, P, P, P, P]),
    "coalign_conv3x3_emu_sparse": (c_int, [P, c_int, P, P, P, P, P, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, P, P]),
    "coalign_pointwise_conv_emu_sparse": (c_int, [P, c_int, P, P, P, P, P, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, P]),
    "coalign_scatter_to_bev": (c_int, [P, P, c_int, c_int, c_int, c_int, c_int, P, P, c_size_t, P]),
    "coalign_warp_fuse": (c_int, [P, c_int, c_int, c_int, c_int, P, POINTER(c_int32), c_int, c_int, P, c_int, c_int, P]),
    "coalign_normalize_pairwise": (c_int, [P, c_int, c_int, c_int, c_double, c_double, P, P]),
    "coalign_warp_fuse_rows": (c_int, [P, c_int, c_int, c_int, c_int, P, POINTER(c_int32), c_int, POINTER(c_int32), c_int, P, c_int, c_int, P]),
    "coalign_warp_fuse_nhwc": (c_int, [c_int, POINTER(P), POINTER(c_int32), POINTER(c_int32), POINTER(c_int32), POINTER(P), POINTER(c_int32),
                                       POINTER(c_int32), c_int, P, POINTER(c_int32), c_int, P]),
    "coalign_anchor_decode_workspace_bytes": (c_size_t, [c_int, c_int, c_int]),
    "coalign_anchor_decode": (c_int, [P, P, P, P, c_int, c_int, c_int, c_int, c_float, c_float, c_int, P, c_int, P, P, P,
                                      P, P, P, P, P, P, c_size_t, P]),
    "coalign_anchor_decode_first": (c_int, [P, P, P, P, c_int, c_int, c_int, c_int, c_float, c_float, c_int, P, c_int, P, P, P,
                                            P, P, P, P, P, P, c_size_t, P, c_int, P]),
    "coalign_nms_rotated_workspace_bytes": (c_size_t, [c_int, c_int]),
    "coalign_nms_rotated": (c_int, [P, c_int, c_int, P, P, c_int, P, c_float, c_int, P, P, P, c_size_t, P]),
    "coalign_nms_rotated_gather": (c_int, [P, P, P, c_int, P, c_float, c_int, P, P, POINTER(c_double), P, P, P, P, c_size_t, P]),
    "coalign_gather_in_range": (c_int, [P, P, P, P, c_int, POINTER(c_double), P, P, P, P]),
    "coalign_iou_rotated_matrix": (c_int, [P, c_int, c_int, c_int, P, c_int, c_int, c_int, P, P]),
    "coalign_boxes_iou_bev": (c_int, [P, c_int, P, c_int, P, P]),
    "coalign_boxes_overlap_bev": (c_int, [P, c_int, P, c_int, P, P]),
    "coalign_pcdet_nms_workspace_bytes": (c_size_t, [c_int]),
    "coalign_pcdet_nms": (c_int, [P, c_int, c_float, c_int, P, P, P, c_size_t, P]),
    "coalign_bias_act": (c_int, [P, P, P, c_int, c_int, c_int, c_int, P]),
    "coalign_fill_words": (c_int, [P, c_size_t, c_uint32, P]),
    "coalign_voxelize_capacity": (c_int64, [c_int64, c_int, POINTER(c_double), POINTER(c_double), c_int]),
    "coalign_voxelize_workspace_bytes": (c_size_t, [POINTER(c_int64), c_int, POINTER(c_double), POINTER(c_double), c_int]),
    "coalign_conv3x3_workspace_bytes": (c_size_t, [c_int, c_int, c_int, c_int, c_int]),
    "coalign_conv3x3_bias_act": (c_int, [P, P, P, P, P, c_int, c_int, c_int, c_int, c_int, c_int, P, c_size_t, P]),
    "coalign_conv3x3_emu_weight_bytes": (c_size_t, [c_int, c_int, c_int]),
    "coalign_conv3x3_emu_workspace_bytes": (c_size_t, [c_int, c_int, c_int, c_int, c_int, c_int]),
    "coalign_conv3x3_emu_weight_bytes_ex": (c_size_t, [c_int, c_int, c_int, c_int]),
    "coalign_conv3x3_emu_workspace_bytes_ex": (c_size_t, [c_int, c_int, c_int, c_int, c_int, c_int, c_int]),
    "coalign_conv3x3_emu_bias_act": (c_int, [P, P, P, P, P, c_int, c_int, c_int, c_int, c_int, c_int, c_int, P, c_size_t, P]),
    "coalign_conv3x3_emu_ex": (c_int, [P, P, P, P, P, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, P, P, c_size_t, P]),
    "coalign_sp_map_bytes": (c_size_t, [c_int, c_int, c_int, c_int]),
    "coalign_sp_pack": (c_int, [P, c_int, P, c_int, c_int, c_int, c_int, P, P]),
    "coalign_sp_unpack": (c_int, [P, P, c_int, c_int, c_int, c_int, c_int, P]),
    "coalign_conv3x3_sp_workspace_bytes": (c_size_t, [c_int, c_int, c_int, c_int, c_int, c_int]),
    "coalign_conv3x3_sp": (c_int, [P, P, P, P, c_int, P, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, P, P, c_size_t, P]),
    "coalign_conv3x3_sp_both": (c_int, [P, P, P, P, c_int, P, P, c_int, c_int, c_int, c_int, c_int, c_int, c_int, P, P, c_size_t, P]),
    "coalign_sp_rows_bytes": (c_size_t, [c_int, c_int]),
    "coalign_sp_pack_rows": (c_int, [P, c_int, P, c_int, P, P, P]),
    "coalign_conv3x3_sp_s2": (c_int, [P, P, P, P, c_int, c_int, c_int, c_int, c_int, c_int, P, P]),
    "coalign_conv3x3_sp_s2_sparse": (c_int, [P, c_int, P, P, P, P, P, c_int, c_int, c_int, c_int, c_int, c_int, P, P]),
    "coalign_conv1x1_sp_weight_bytes": (c_size_t, [c_int, c_int]),
    "coalign_conv3x3_sp_s2_skip": (c_int, [P, P, P, P, P, P, c_int, c_int, c_int, c_int, c_int, c_int, P, P]),
    "coalign_conv3x3_sp_s2_skip_sparse": (c_int, [P, c_int, P, P, P, P, P, P, P, c_int, c_int, c_int, c_int, c_int, c_int, P, P]),
    "coalign_pointwise_conv": (c_int, [P, P, P, P, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, P]),
    "coalign_pointwise_conv_ex": (c_int, [P, P, P, P, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, P]),
    "coalign_pointwise_emu_weight_bytes": (c_size_t, [c_int, c_int]),
    "coalign_pointwise_conv_emu": (c_int, [P, P, P, P, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, P]),
    "coalign_pointwise_conv_emu_sp": (c_int, [P, P, P, P, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, P, P]),
    "coalign_pointwise_conv_emu_sp_multi": (c_int, [c_int, POINTER(P), POINTER(P), POINTER(P), POINTER(c_int32), POINTER(c_int32), POINTER(c_int32), POINTER(c_int32), POINTER(c_int32),
                                            POINTER(c_int32), POINTER(c_int32), P, c_int, c_int, c_int, P, P]),
    "coalign_heads_sp": (c_int, [P, P, P, P, c_int, c_int, c_int, c_int, c_int, P]),
    "coalign_pose_graph_workspace_bytes": (c_size_t, [c_int]),
    "coalign_pose_graph_optimize": (c_int, [c_int, P, P, P, c_int, P, P, P, P, P, P, c_int, P, P, c_size_t, P]),
    "coalign_voxelize": (c_int, [P, POINTER(c_int64), c_int, POINTER(c_double), POINTER(c_double), c_int, c_int, c_int,
                                 POINTER(c_double), P, P, P, c_int64, P, P, c_size_t, P]),
}


# include/coalign_amd_lab.h: entry points of the laboratory library only (the Winograd kernel: measured, not adopted; the voxeliser's gather_kernel alone: for its limit tests)
LAB_SIGNATURES = {
    "coalign_conv3x3_wino_weight_bytes": (c_size_t, [c_int, c_int]),
    "coalign_conv3x3_wino": (c_int, [P, P, P, P, P, c_int, c_int, c_int, c_int, c_int, c_int, c_int, P]),
    "coalign_lab_voxelize_gather": (c_int, [P, c_int64, P, P, P, P, P, P, c_int, P, c_int64, P]),
}

# include/coalign_amd_narrow.h: extension header of ABI version 2 (product library; coalign_amd.h keeps its 68 names): the narrow-output 3x3 convolution
NARROW_SIGNATURES = {
    "coalign_conv3x3_narrow_weight_bytes": (c_size_t, [c_int, c_int]),
    "coalign_conv3x3_sp_narrow": (c_int, [P, c_int, P, P, P, c_int, c_int, c_int, c_int, c_int, c_int, P, P]),
}

# include/coalign_amd_narrow_sparse.h: extension header of ABI version 2 (product library): the narrow-output convolution reading the sparse canvas
NARROW_SPARSE_SIGNATURES = {
    "coalign_conv3x3_sp_narrow_sparse": (c_int, [P, c_int, P, P, P, P, P, c_int, c_int, c_int, c_int, c_int, c_int, P, P]),
}

# include/coalign_amd_align.h: extension header of ABI version 2 (product library): online pose correction -- stage-1 gather, pose-graph
# construction, corrected pairwise / affine matrices (csrc/pose_graph_build.hip)
ALIGN_SIGNATURES = {
    "coalign_align_store_boxes": (c_int, []),
    "coalign_stage1_gather": (c_int, [P, P, P, P, c_int, P, c_int, c_int, c_int, c_int, c_int, P, P, P, P, P]),
    "coalign_pose_graph_build": (c_int, [c_int, c_int, P, P, c_int, c_int, P, P, c_int, c_double, c_double, P, P, P, P, P, P, P, P, P, P, P]),
    "coalign_pose_correct_matrices": (c_int, [c_int, c_int, P, P, P, c_int, c_int, c_int, c_int, c_double, c_double, P, P, P, P]),
}

# include/coalign_amd_stage1.h: extension header of ABI version 2 (product library): stage 1 of all agents in one pass -- decode, rotated NMS and
# the store gather of every agent in five launches (csrc/decode.hip, csrc/nms.hip)
STAGE1_SIGNATURES = {
    "coalign_stage1_boxes_workspace_bytes": (c_size_t, [c_int, c_int, c_int, c_int, c_int]),
    "coalign_stage1_boxes": (c_int, [P, P, P, P, P, c_int, c_int, c_int, c_int, c_int, c_int, c_float, c_float, c_int, c_float, c_int, P, P, P, P, P, c_size_t, P]),
    "coalign_stage1_boxes_strided": (c_int, [P, P, P, P, c_size_t, c_size_t, c_size_t, c_size_t, P, c_int, c_int, c_int, c_int, c_int, c_int, c_float, c_float, c_int, c_float,
                                             c_int, P, P, P, P, P, c_size_t, P]),
}

# include/coalign_amd_disco.h: extension header of ABI version 2 (product library): DiscoNet's pixel-weight fusion -- warp, per-pixel MLP, softmax
# over agents and weighted sum in one launch (csrc/disco_fuse.hip)
DISCO_SIGNATURES = {
    "coalign_disco_param_bytes": (c_size_t, [c_int]),
    "coalign_disco_fuse": (c_int, [P, c_int, c_int, c_int, c_int, P, P, c_size_t, P, P]),
}

# include/coalign_amd_v2v.h: extension header of ABI version 2 (product library): the glue of V2VNet's message passing between its convolutions --
# warp + operand split, message mask + aggregation + GRU input, GRU gate (csrc/v2v_fuse.hip)
V2V_SIGNATURES = {
    "coalign_v2v_warp_split": (c_int, [P, c_int, c_int, c_int, c_int, c_int, P, P, P, P]),
    "coalign_v2v_aggregate": (c_int, [P, P, P, c_int, c_int, c_int, c_int, c_int, P, c_int, c_int, P, P, P]),
    "coalign_v2v_gate": (c_int, [P, c_int, c_int, c_int, c_int, c_int, P, P, P]),
}

# include/coalign_amd_v2x.h: extension header of ABI version 2 (product library): V2X-ViT's heterogeneous agent attention -- warp, LayerNorm, the folded
# q / k / v projection, softmax over the agents per head, output projection and residual in two launches (csrc/v2x_attn.hip)
V2X_SIGNATURES = {
    "coalign_v2x_param_bytes": (c_size_t, [c_int]),
    "coalign_v2x_workspace_bytes": (c_size_t, [c_int, c_int, c_int, c_int]),
    "coalign_v2x_agent_attention": (c_int, [P, c_int, c_int, c_int, c_int, c_int, P, P, c_size_t, P, P, c_size_t, P]),
}

# include/coalign_amd_v2x_window.h: extension header of ABI version 2 (product library): V2X-ViT's pyramid window attention with split attention --
# LayerNorm + the folded 9C x C projection, attention inside the 4 / 8 / 16 windows, the branch weights, output projections and residual in three or four
# launches (csrc/v2x_window.hip)
V2X_WINDOW_SIGNATURES = {
    "coalign_v2x_window_param_bytes": (c_size_t, [c_int, c_int]),
    "coalign_v2x_window_workspace_bytes": (c_size_t, [c_int, c_int, c_int, c_int]),
    "coalign_v2x_window_attention": (c_int, [P, c_int, c_int, c_int, c_int, c_int, P, c_size_t, P, P, c_size_t, P]),
}

# include/coalign_amd_w2c.h: extension header of ABI version 2 (product library): When2com's handshake fusion after its convolutions -- the pooled key /
# query heads with the softmax over the agents in two launches, the warp-and-weighted-sum of the agents' maps in one (csrc/w2c_fuse.hip)
W2C_SIGNATURES = {
    "coalign_w2c_workspace_bytes": (c_size_t, []),
    "coalign_w2c_score": (c_int, [P, c_int, P, c_int, c_int, c_int, P, c_size_t, P, P, P, c_size_t, P]),
    "coalign_w2c_fuse": (c_int, [P, c_int, c_int, c_int, c_int, P, P, P, P]),
}

# include/coalign_amd_v2v_robust.h: extension header of ABI version 2 (product library): the glue of the pose-robust V2VNet between its convolutions --
# pooling tails, the attention's score head, the pose regression's head, pairwise matrices, the whole WeightedEM in one workgroup, the weighted aggregation
# (csrc/v2v_robust.hip)
V2VR_SIGNATURES = {
    "coalign_v2vr_pool_act": (c_int, [P, P, c_int, c_int, c_int, c_int, c_int, c_int, P, P, P]),
    "coalign_v2vr_score_head": (c_int, [P, c_int, c_int, c_int, c_int, c_int, P, P, P, P, P, P]),
    "coalign_v2vr_pose_head_workspace_bytes": (c_size_t, [c_int, c_int]),
    "coalign_v2vr_pose_head": (c_int, [P, c_int, c_int, c_int, c_int, c_int, P, P, P, P, P, P, P, P, P, P, c_size_t, P]),
    "coalign_v2vr_pairwise": (c_int, [P, c_int, c_int, c_int, c_int, c_double, c_double, P, P, P]),
    "coalign_v2vr_consistency": (c_int, [P, P, c_int, c_int, c_int, c_int, c_double, c_double, P, P, P, P]),
    "coalign_v2vr_aggregate": (c_int, [P, P, P, c_int, c_int, c_int, c_int, c_int, P, P, c_int, c_int, P, P, P]),
}

# include/coalign_amd_where2comm.h: extension header of ABI version 2 (product library): Where2comm's confidence-masked fusion -- the communication
# masks and rates of every agent at every backbone level in one launch, the warp and fusion of the masked maps in one launch per frame (csrc/w2comm.hip)
W2COMM_SIGNATURES = {
    "coalign_w2comm_masks": (c_int, [P, c_int, c_int, c_int, c_int, POINTER(c_int32), c_int, P, P, c_int, c_float, c_int, POINTER(P), P, P]),
    "coalign_w2comm_fuse_nhwc": (c_int, [c_int, POINTER(P), POINTER(c_int32), POINTER(c_int32), POINTER(c_int32), POINTER(P), POINTER(P), POINTER(c_int32),
                                         POINTER(c_int32), c_int, P, POINTER(c_int32), c_int, P]),
}

# include/coalign_amd_where2comm_msg.h: extension header of ABI version 2 (product library): Where2comm's messages -- bitmaps, rank
# tables and counts of every agent and level in one launch, the masked pixels' rows packed in one launch, and the fusion that reads dense and packed sources
# (csrc/w2comm_msg.hip).  The reference has no counterpart.
W2COMM_MSG_SIGNATURES = {
    "coalign_w2comm_msg_index": (c_int, [c_int, c_int, POINTER(c_int32), POINTER(c_int32), POINTER(P), POINTER(P), POINTER(P), P, P]),
    "coalign_w2comm_msg_pack": (c_int, [c_int, c_int, POINTER(P), POINTER(c_int32), POINTER(c_int32), POINTER(c_int32), POINTER(P), POINTER(P), POINTER(P), P]),
    "coalign_w2comm_fuse_packed": (c_int, [c_int, POINTER(c_int32), POINTER(c_int32), POINTER(c_int32), POINTER(c_int32), POINTER(P), POINTER(P), POINTER(P), POINTER(P),
                                           POINTER(c_int32), POINTER(c_int32), c_int, P, c_int, P]),
}

# include/coalign_amd_v2x_ffn.h: extension header of ABI version 2 (product library): V2X-ViT's feed-forward block -- LayerNorm, the
# folded first linear, GELU, the second linear and the residual per token in one launch (csrc/v2x_ffn.hip)
V2X_FFN_SIGNATURES = {
    "coalign_v2x_ffn_param_bytes": (c_size_t, [c_int, c_int]),
    "coalign_v2x_feed_forward": (c_int, [P, c_int, c_int, c_int, P, c_size_t, P, P]),
}

# include/coalign_amd_lss.h: extension header of ABI version 2 (product library): Lift-Splat's frustum pooling -- the voxel of every
# frustum point once per camera rig, then per frame the depth softmax and the sum of probability x feature row per BEV cell through an inverted index, in two
# launches (csrc/lss_pool.hip)
LSS_SIGNATURES = {
    "coalign_lss_cells": (c_int, [P, P, P, P, P, c_int, c_int, P, P, P, c_int, c_int, c_int, c_float, c_float, c_float, c_float, c_float, c_float, c_int, c_int, c_int, P, P]),
    "coalign_lss_depth_prob": (c_int, [P, c_int, c_int, c_int, c_int, c_int, P, P]),
    "coalign_lss_pool": (c_int, [P, P, c_int, c_int, c_int, P, c_int, P, c_int, P, c_int, P, P]),
}

# include/coalign_amd_lss_bev.h: extension header of ABI version 2 (product library): the camera model's BEV encoder -- the 7 x 7 /
# stride-2 stem and the bilinear x 2 up-sampling with concatenation, both writing a SplitMap (csrc/lss_bev.hip)
LSS_BEV_SIGNATURES = {
    "coalign_conv7x7_s2_weight_bytes": (c_size_t, [c_int]),
    "coalign_conv7x7_s2_sp": (c_int, [P, P, P, P, c_int, c_int, c_int, c_int, c_int, P, P]),
    "coalign_up2x_concat_sp": (c_int, [P, P, P, c_int, c_int, c_int, c_int, c_int, P, P]),
}

# header under include/ -> its table, in the order of the ABI's growth (build.ABI_HEADERS without its last): what both loaders bind.  coalign_amd_lab.h's
# LAB_SIGNATURES: the laboratory library alone.
HEADERS = {
    "coalign_amd.h": SIGNATURES,
    "coalign_amd_narrow.h": NARROW_SIGNATURES,
    "coalign_amd_narrow_sparse.h": NARROW_SPARSE_SIGNATURES,
    "coalign_amd_align.h": ALIGN_SIGNATURES,
    "coalign_amd_stage1.h": STAGE1_SIGNATURES,
    "coalign_amd_disco.h": DISCO_SIGNATURES,
    "coalign_amd_v2v.h": V2V_SIGNATURES,
    "coalign_amd_v2x.h": V2X_SIGNATURES,
    "coalign_amd_v2x_window.h": V2X_WINDOW_SIGNATURES,
    "coalign_amd_w2c.h": W2C_SIGNATURES,
    "coalign_amd_v2v_robust.h": V2VR_SIGNATURES,
    "coalign_amd_where2comm.h": W2COMM_SIGNATURES,
    "coalign_amd_where2comm_msg.h": W2COMM_MSG_SIGNATURES,
    "coalign_amd_v2x_ffn.h": V2X_FFN_SIGNATURES,
    "coalign_amd_lss.h": LSS_SIGNATURES,
    "coalign_amd_lss_bev.h": LSS_BEV_SIGNATURES,
}

# include_ext/coalign_amd_sparse3d.h: extension header of ABI version 2 (product library), the first outside include/'s frozen set: the sparse 3-D trunk of the SECOND
# detectors -- MeanVFE, the site index, strided site generation, the neighbour table, the gather-GEMM convolution and the dense map (csrc/sparse_conv3d.hip)
SPARSE3D_SIGNATURES = {
    "coalign_sp3d_mean_vfe": (c_int, [P, P, c_int, c_int, c_int, P, P]),
    "coalign_sp3d_index_workspace_bytes": (c_size_t, [c_int, c_int, c_int, c_int, c_int]),
    "coalign_sp3d_index_build": (c_int, [P, P, c_int, c_int, c_int, c_int, c_int, P, c_size_t, P]),
    "coalign_sp3d_strided_sites": (c_int, [P, P, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, P, P, c_int, P, c_size_t, P, P]),
    "coalign_sp3d_neighbors": (c_int, [P, P, c_int, c_int, c_int, c_int, c_int, P, c_size_t, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int,
                                       c_int, P, P]),
    "coalign_sp3d_weight_bytes": (c_size_t, [c_int, c_int, c_int]),
    "coalign_sp3d_conv": (c_int, [P, c_int, P, c_int, P, c_int, c_int, c_int, P, c_size_t, P, P, P]),
    "coalign_sp3d_to_dense": (c_int, [P, P, c_int, c_int, P, c_size_t, c_int, c_int, c_int, c_int, P, P]),
}

# header under include_ext/ (build.EXT_HEADERS) -> its table: bound by both loaders AFTER the frozen tables above
EXT_HEADERS = {
    "coalign_amd_sparse3d.h": SPARSE3D_SIGNATURES,
}

# include_open/coalign_amd_ssfa.h: extension header of ABI version 2 (product library), the first under include_open/: the SSFA neck of the SECOND detectors -- the
# 3 x 3 / stride-2 transposed convolution on SplitMaps and the two-way softmax blend (csrc/ssfa_neck.hip)
SSFA_SIGNATURES = {
    "coalign_deconv3x3_s2_weight_bytes": (c_size_t, [c_int, c_int]),
    "coalign_deconv3x3_s2_sp": (c_int, [P, P, P, P, P, c_int, c_int, c_int, c_int, c_int, c_int, P, P]),
    "coalign_ssfa_blend": (c_int, [P, P, P, P, c_float, c_float, P, P, c_int, c_int, c_int, c_int, P, P]),
}

# include_open/coalign_amd_sp3d_voxelize.h: raw point clouds -> the input sparse tensor of VoxelBackBone8x (mean features, indices, device count, level-0 site
# index) on the bitmap + prefix-count site index (csrc/sparse_conv3d.hip); voxel_size / lidar_range / filter_range are host float64 arrays
SP3D_VOXELIZE_SIGNATURES = {
    "coalign_sp3d_voxelize_workspace_bytes": (c_size_t, [c_int, c_int, c_int]),
    "coalign_sp3d_voxelize": (c_int, [P, P, c_int, c_int, P, P, c_int, c_int, c_int, c_int, c_int, c_int, P, P, P, P, P, c_int, P, c_size_t, P, P, c_size_t, P]),
}

# header under include_open/ (build.OPEN_HEADERS) -> its table: bound by both loaders AFTER EXT_HEADERS; the next header joins this map
OPEN_HEADERS = {
    "coalign_amd_ssfa.h": SSFA_SIGNATURES,
    "coalign_amd_sp3d_voxelize.h": SP3D_VOXELIZE_SIGNATURES,
}
_LAB_LIB = None


class CoalignHipError(RuntimeError):
    pass


def lib_path() -> str:
    return _build.LIB_PATH


def _load(path: str, tables, no_fallback: str = "") -> ctypes.CDLL:
    """dlopen ``path``, building it first if it is missing, and give every name of ``tables`` its types."""
    import torch  # noqa: F401  -- load PyTorch-ROCm's HIP runtime first so both share one libamdhip64.so.7
    if not os.path.exists(path):
        try:
            _build.build(lab=path != _build.LIB_PATH, vectorize=path == _build.LABVEC_LIB_PATH)
        except Exception as exc:  # noqa: BLE001
            raise CoalignHipError(f"{path} is missing and could not be built ({exc}){no_fallback}") from exc
    handle = ctypes.CDLL(path)
    for table in tables:
        for name, (res, args) in table.items():
            fn = getattr(handle, name)  # AttributeError here == header / library mismatch
            fn.restype = res
            fn.argtypes = args
    return handle


def lib() -> ctypes.CDLL:
    """Load (building first if needed) the gfx950 library.  Raises if that is impossible."""
    global _LIB
    if _LIB is not None:
        return _LIB
    lab = os.environ.get("COALIGN_LAB", "0")             # tools/ only: "1" = the laboratory build with its ablation switches, "vec" = + packed fp32 allowed (build.py)
    path = _build.LABVEC_LIB_PATH if lab == "vec" else _build.LAB_LIB_PATH if lab == "1" else _build.LIB_PATH
    handle = _load(path, [*HEADERS.values(), *EXT_HEADERS.values(), *OPEN_HEADERS.values()], "; the CoAlign hot path has no CPU fallback")
    if handle.coalign_abi_version() != 2:
        raise CoalignHipError(f"ABI version mismatch: library reports {handle.coalign_abi_version()}, binding expects 2")
    _LIB = handle
    return handle


def lab_lib() -> ctypes.CDLL:
    """The laboratory library (product sources + -DCOALIGN_LAB + include/coalign_amd_lab.h's kernels), loaded beside the product library: the Winograd tests
    and tools call through it; nothing in the detector's default routes does."""
    global _LAB_LIB
    if _LAB_LIB is None:
        _LAB_LIB = _load(_build.LAB_LIB_PATH, [*HEADERS.values(), *EXT_HEADERS.values(), *OPEN_HEADERS.values(), LAB_SIGNATURES])
    return _LAB_LIB


def check(status: int, what: str) -> None:
    if status != 0:
        L = lib()
        msg = L.coalign_status_string(status).decode()
        if status == -5:
            msg += " [" + L.coalign_last_hip_error().decode() + "]"
        raise CoalignHipError(f"{what}: {msg}")
