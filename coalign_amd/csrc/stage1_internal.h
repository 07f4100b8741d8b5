// Stage 1 of all agents in one pass (include/coalign_amd_stage1.h): what csrc/nms.hip, which holds the entry point, needs from csrc/decode.hip.
#pragma once
#include "common.h"

namespace coalign {

// Blocks of the segmented decode launches: ceil(A * H * W / 256) per agent.
size_t stage1_decode_blocks(int n_agents, int A, int H, int W);

// count + emit over every agent's head maps (identity transform): agent g's candidates become rows seg_start[g] .. seg_start[g + 1] of the candidate arrays
// (capacity n_agents * A * H * W rows: every anchor may pass).  *_stride: floats between two agents' maps.  `clear_word` is zeroed by the first launch.  Arguments are the caller's, already validated.
int stage1_decode_segments(const float *cls, const float *reg, const float *dir, const float *anchors, size_t cls_stride, size_t reg_stride, size_t dir_stride,
                           int n_agents, int A, int H, int W, int num_bins,
                           float score_thr, float dir_offset, int order_hwl, int32_t *block_counts, int32_t *seg_start, int32_t *cand_index, float *cand_score,
                           float *cand_corners, uint8_t *cand_keep, uint32_t *clear_word, hipStream_t stream);

}  // namespace coalign
