/* Extension header of ABI version 2 (include/coalign_amd.h keeps its 68 entry points, include/coalign_amd_align.h its four): STAGE 1 OF ALL AGENTS IN ONE PASS.
 * The per-agent loop of online pose correction's first step -- decode, rotated NMS and the store gather, six launches per agent through coalign_anchor_decode*,
 * coalign_nms_rotated and coalign_stage1_gather -- as one sequence of five launches whose count does not depend on the number of agents.  Part of the product
 * library libcoalign_hip.so; same conventions as include/coalign_amd.h (status codes, every shape / pointer check before any HIP call, everything on the caller's
 * stream, no allocation, no host synchronisation, no environment variable: safe inside a captured graph on one stream). */
#ifndef COALIGN_AMD_STAGE1_H
#define COALIGN_AMD_STAGE1_H

#include "coalign_amd.h"
#include "coalign_amd_align.h"

#ifdef __cplusplus
extern "C" {
#endif

/* (12a) Workspace of coalign_stage1_boxes: the candidate arrays of all agents (every anchor may pass: n_agents * A * H * W rows) and, per agent, the order list,
 * the sorted count and the suppression bitmask (opencood/data_utils/post_processor/uncertainty_voxel_postprocessor.py:26-112 keeps these as Python lists and
 * host tensors).  0 for arguments coalign_stage1_boxes rejects. */
size_t coalign_stage1_boxes_workspace_bytes(int n_agents, int A, int H, int W, int top);

/* (12b) Stage-1 boxes of every agent of a sample.  Replaces UncertaintyVoxelPostprocessor.post_process_stage1
 * (opencood/data_utils/post_processor/uncertainty_voxel_postprocessor.py:26-112: per agent the score threshold, delta_to_boxes3d, the direction fix,
 * boxes_to_corners_3d, nms_rotated, boxes[keep] / unc[mask][keep]) for all agents at once, and leaves in the store bit for bit what the per-agent sequence
 * coalign_anchor_decode_first -> coalign_nms_rotated -> coalign_stage1_gather leaves there, status word included.
 *   cls [n_agents][A][H][W], reg [n_agents][7 A][H][W], dir [n_agents][num_bins * A][H][W] or NULL, unc [n_agents][A * udim][H][W] (NULL with udim 0; 0 <= udim
 *   <= 3): the stage-1 model's head maps as it returns them, float32.  anchors [H * W * A][7] float32.  1 <= n_agents <= COALIGN_ALIGN_MAX_AGENTS.
 *   Per agent: sigmoid(cls) > score_thr; decode with the identity transform and the direction fix (dir_offset, num_bins; order_hwl as coalign_anchor_decode);
 *   rotated NMS over THAT agent's candidates only, no sanity mask, rank key (score descending, index descending), the first `top` of them, float64 clipping,
 *   IoU rounded to float32 before the strict '>' iou_thr; top <= 1024 (the fast kernels of coalign_nms_rotated; more: COALIGN_ERR_UNSUPPORTED).
 *   store_corners [8][C][8][3], store_unc [8][C][udim], store_count [8], status [1]: the sample's store of include/coalign_amd_align.h, C =
 *   COALIGN_ALIGN_STORE_BOXES.  Slot i receives the first min(kept_i, C) kept boxes of agent i in pick order with the raw unc of their anchors; status becomes 0,
 *   or COALIGN_ALIGN_STORE_OVERFLOW when an agent kept more than C.  Slots n_agents .. 7 are left as they are.
 *   Launches: count, emit (agent i's candidates form one contiguous segment, in (h, w, anchor) order; no block straddles two agents), rank, mask (grid
 *   dimension = agent), reduce (one workgroup per agent, the store written from LDS).  Five, whatever n_agents is.
 *   Returns COALIGN_ERR_NULL_POINTER for a NULL array, COALIGN_ERR_BAD_SHAPE for n_agents outside 1 .. 8, udim outside 0 .. 3, non-positive A / H / W / top or
 *   dir with num_bins <= 0, COALIGN_ERR_UNSUPPORTED for top > 1024, COALIGN_ERR_WORKSPACE for workspace_bytes below (12a). */
int coalign_stage1_boxes(const float *cls, const float *reg, const float *dir, const float *unc, const float *anchors, int n_agents, int A, int H, int W,
                         int num_bins, int udim, float score_thr, float dir_offset, int order_hwl, float iou_thr, int top, float *store_corners, float *store_unc,
                         int32_t *store_count, int32_t *status, void *workspace, size_t workspace_bytes, void *stream);

/* (12c) The same with explicit agent strides: *_stride = floats between the maps of two consecutive agents (>= the size of one agent's maps).  A detector that
 * computes its heads as ONE convolution returns cls / reg / dir / unc as channel slices of one [n_agents][C][H][W] tensor: each agent's maps are dense, the agents
 * are C * H * W floats apart, and the pass reads them where they are (uncertainty_voxel_postprocessor.py:26-112 indexes the same maps through torch views).
 * coalign_stage1_boxes is this entry point with the dense strides A * H * W, 7 A * H * W, num_bins * A * H * W, A * udim * H * W.  A stride below one agent's maps:
 * COALIGN_ERR_BAD_SHAPE. */
int coalign_stage1_boxes_strided(const float *cls, const float *reg, const float *dir, const float *unc, size_t cls_stride, size_t reg_stride, size_t dir_stride,
                                 size_t unc_stride, const float *anchors, int n_agents, int A, int H, int W, int num_bins, int udim, float score_thr,
                                 float dir_offset, int order_hwl, float iou_thr, int top, float *store_corners, float *store_unc, int32_t *store_count,
                                 int32_t *status, void *workspace, size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif

#endif
