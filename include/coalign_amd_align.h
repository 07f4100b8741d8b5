/* Extension header of ABI version 2 (include/coalign_amd.h keeps its 68 entry points): ONLINE POSE CORRECTION.  The chain from the stage-1 detections of a
 * frame's agents to the normalised affine matrices the fusion model consumes, without the host in the middle: stage-1 gather -> pose-graph construction ->
 * coalign_pose_graph_optimize (include/coalign_amd.h (8), unchanged) -> corrected matrices.  Part of the product library libcoalign_hip.so; same conventions as
 * include/coalign_amd.h (status codes, every shape / pointer check before any HIP call, everything on the caller's stream, no allocation, no host
 * synchronisation: safe inside a captured graph on one stream). */
#ifndef COALIGN_AMD_ALIGN_H
#define COALIGN_AMD_ALIGN_H

#include "coalign_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Limits (those of coalign_pose_graph_optimize, plus the box store's) and the fixed per-sample capacities of the graph arrays */
#define COALIGN_ALIGN_MAX_AGENTS 8
#define COALIGN_ALIGN_MAX_LANDMARKS 256
#define COALIGN_ALIGN_STORE_BOXES 256                                                     /* C: kept stage-1 boxes per agent the store holds        */
#define COALIGN_ALIGN_MAX_VERTICES (COALIGN_ALIGN_MAX_AGENTS + COALIGN_ALIGN_MAX_LANDMARKS) /* rows of `vertices` / `kinds` per sample               */
#define COALIGN_ALIGN_MAX_EDGES (COALIGN_ALIGN_MAX_AGENTS * COALIGN_ALIGN_STORE_BOXES)      /* rows of the edge arrays per sample (a box: <= 1 edge) */

/* The per-sample status word (int32).  0 = the graph was built and is to be solved; in every other case the sample's noisy poses pass through unchanged
 * and the graph handed to the solver is empty (agents only, no edge). */
#define COALIGN_ALIGN_SOLVED 0
#define COALIGN_ALIGN_KEPT_NOISY 1      /* abandon_hard_cases decided to keep the noisy poses (box_align_v2.py:283-285)                            */
#define COALIGN_ALIGN_NO_BOXES 2        /* no agent has a stage-1 box (uncertainty_voxel_postprocessor.py: post_process_stage1 returns None)       */
#define COALIGN_ALIGN_OUTSIDE_LIMITS 4  /* outside the limits; one of the two bits below says which                                                 */
#define COALIGN_ALIGN_STORE_OVERFLOW 8  /*   an agent kept more than COALIGN_ALIGN_STORE_BOXES boxes (set by coalign_stage1_gather)                  */
#define COALIGN_ALIGN_TOO_MANY_LANDMARKS 16 /* more than COALIGN_ALIGN_MAX_LANDMARKS clusters                                                        */

/* flags of coalign_pose_graph_build: the keyword arguments of box_alignment_relative_sample_np (box_align_v2.py:101-118) */
#define COALIGN_ALIGN_USE_UNCERTAINTY 1
#define COALIGN_ALIGN_LANDMARK_SE2 2
#define COALIGN_ALIGN_ADAPTIVE_LANDMARK 4
#define COALIGN_ALIGN_NORMALIZE_UNCERTAINTY 8
#define COALIGN_ALIGN_ABANDON_HARD_CASES 16
#define COALIGN_ALIGN_DROP_HARD_BOXES 32
#define COALIGN_ALIGN_DROP_UNSURE_EDGE 64

/* COALIGN_ALIGN_STORE_BOXES, for bindings that cannot read the macro. */
int coalign_align_store_boxes(void);

/* (11a) Stage-1 gather.  Replaces the read-backs and torch indexing of UncertaintyVoxelPostprocessor.post_process_stage1
 * (opencood/data_utils/post_processor/uncertainty_voxel_postprocessor.py:26-112, the per-agent loop: boxes[mask], unc[mask], the NMS keep indices): after
 * coalign_anchor_decode* and coalign_nms_rotated* of ONE agent (identity transform, no sanity mask) copy the kept detections into slot `slot` of a sample's box
 * store (csrc/pose_graph_build.hip).
 *   keep [>= keep_count] int32 / keep_count [1] int32 / cand_index [capacity] int32 (flat (h, w, anchor) index) / cand_corners [capacity][8][3] float32: the
 *   outputs of the two kernels, read on the device.  unc: the agent's raw unc_preds [A * udim][H][W] float32 (NULL with udim 0); 0 <= udim <= 3.
 *   store_corners [8][C][8][3] float32, store_unc [8][C][udim] float32, store_count [8] int32, status [1] int32: the SAMPLE's store, C = COALIGN_ALIGN_STORE_BOXES.
 *   Slot 0 opens the frame: it writes the status word (0, or COALIGN_ALIGN_STORE_OVERFLOW); later slots OR the overflow bit in.  A slot holds the first
 *   min(keep_count, C) kept boxes in pick order, bit for bit what post_process_stage1 returns for that agent. */
int coalign_stage1_gather(const int32_t *keep, const int32_t *keep_count, const int32_t *cand_index, const float *cand_corners, int capacity, const float *unc,
                          int A, int udim, int H, int W, int slot, float *store_corners, float *store_unc, int32_t *store_count, int32_t *status, void *stream);

/* (11b) Pose-graph construction.  Replaces everything of box_alignment_relative_sample_np in front of the solver
 * (opencood/models/sub_modules/box_align_v2.py:150-372; pose_to_tfm transformation_utils.py:93-160, project_box3d box_utils.py:278-316, corner_to_center
 * box_utils.py:25-85, all_pair_l2 box_align_v2.py:79-96), one workgroup per sample, in the arithmetic coalign_amd/box_align.py:build_pose_graph restates:
 * float32 poses, projection, world-frame centres, all-pair test sqrt(sq_i + sq_j - 2 dot_ij) < thres (a negative radicand is NaN: not near) and yaw variance;
 * float64 agent-frame measurements and information.
 *   corners [S][8][C][8][3] and unc [S][8][C][udim] (NULL with udim 0: no uncertainties): float32, or float64 when `wide` is 1 (boxes that did not come from
 *   the float32 stage-1 kernels); count [S][8] int32; status [S] int32, read for COALIGN_ALIGN_STORE_OVERFLOW and rewritten with the sample's final word.
 *   noisy_poses [S][n_agents][6] float64 (x, y, z, roll, yaw, pitch; degrees); 1 <= n_agents <= 8 (every sample of one launch has the same number).
 *   Outputs, per sample, exactly what coalign_pose_graph_optimize reads for ONE graph: vertex_off [S][2] = {0, V}, edge_off [S][2] = {0, E}, graph_agents [S],
 *   vertices [S][MAX_VERTICES][3] float64 (agents first, yaw in radians; then the landmarks), kinds [S][MAX_VERTICES] (ego 0, SE(2) 1, point 2), edge_agent /
 *   edge_landmark [S][MAX_EDGES] int32 and edge_meas / edge_info [S][MAX_EDGES][3] float64, grouped by ascending landmark, members in [seed, ascending box]
 *   order.  The caller passes sample s's slices to the solver with n_graphs = 1 and total_vertices = COALIGN_ALIGN_MAX_VERTICES. */
int coalign_pose_graph_build(int n_samples, int n_agents, const void *corners, const void *unc, int wide, int udim, const int32_t *count, const double *noisy_poses,
                             int flags, double thres, double yaw_var_thres, int32_t *vertex_off, int32_t *edge_off, int32_t *graph_agents, double *vertices,
                             int32_t *kinds, int32_t *edge_agent, int32_t *edge_landmark, double *edge_meas, double *edge_info, int32_t *status, void *stream);

/* (11c) Corrected matrices.  Replaces the hook of intermediate_fusion_dataset.py:301-328 (refined (x, y, yaw) back into the 6-DOF poses),
 * opencood/utils/transformation_utils.py:22-67 (get_pairwise_transformation with x_to_world :263-306) and :69-91 (normalize_pairwise_tfm), one launch.
 *   noisy_poses [S][n_agents][6], vertices [S][MAX_VERTICES][3] (the solver's output), status [S]: a sample whose status is not 0 returns its noisy poses bit
 *   for bit.  n_agents <= max_cav <= 16.  den_x = downsample_rate * discrete_ratio * W, den_y = ... * H, as coalign_normalize_pairwise.
 *   Outputs float64: poses_out [S][n_agents][6]; pairwise [S][L][L][4][4], entry [i][j] = T_j^-1 T_i in closed form, identity on the diagonal, in the padding
 *   and everywhere with proj_first; affine [S][L][L][2][3] in the operation order of normalize_pairwise_tfm. */
int coalign_pose_correct_matrices(int n_samples, int n_agents, const double *noisy_poses, const double *vertices, const int32_t *status, int max_cav,
                                  int proj_first, int H, int W, double den_x, double den_y, double *poses_out, double *pairwise, double *affine, void *stream);

#ifdef __cplusplus
}
#endif

#endif
