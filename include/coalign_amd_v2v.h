/* Extension header of ABI version 2 (include/coalign_amd.h keeps its 68 entry points, the extension headers coalign_amd_narrow.h, coalign_amd_align.h,
 * coalign_amd_narrow_sparse.h, coalign_amd_stage1.h and coalign_amd_disco.h their 2 / 4 / 1 / 3 / 2): the glue of V2VNet's message passing
 * (V2VNetFusion, opencood/models/fuse_modules/fusion_in_one.py:173-293, with opencood/models/sub_modules/convgru.py) between the 3 x 3 convolutions, which run
 * on coalign_conv3x3_sp.  Part of the product library libcoalign_hip.so; same conventions as include/coalign_amd.h (status codes, every shape / pointer check
 * before any HIP call, everything on the caller's stream, no allocation, no workspace: safe inside a captured graph).
 *
 * Common to the three entry points: float32 maps are channels-last ([.., H, W, C]) and 16-byte aligned, theta is float64 and 8-byte aligned, SplitMaps are the
 * maps of include/coalign_amd.h (9e), 16-byte aligned.  n agents send, R receivers are updated (the first R agents of the frame): 1 <= R <= n <= 8, anything
 * else with n > 8 COALIGN_ERR_UNSUPPORTED, R > n or a negative count COALIGN_ERR_BAD_SHAPE.  n = 0 or R = 0 returns COALIGN_OK without a launch.  A map of
 * 2^31 floats or more (n * C * H * W for x, R * n * C * H * W for the pair maps) is COALIGN_ERR_BAD_SHAPE.  range_flag may be NULL; bit 0 is ORed in when a
 * value written to a SplitMap exceeds the pair's range (|v| > 65504), as by every SplitMap producer. */
#ifndef COALIGN_AMD_V2V_H
#define COALIGN_AMD_V2V_H

#include "coalign_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define COALIGN_V2V_AGG_MAX 0
#define COALIGN_V2V_AGG_AVG 1

#define COALIGN_V2V_OUT_NHWC 0
#define COALIGN_V2V_OUT_SP 1

/* (12a) Warp and operand split in one pass (V2VNetFusion.forward, fusion_in_one.py:173-293, the warp_affine_simple of lines 250-252 for every receiver): y_sp [R * n, C, H, W] = the SplitMap of warp_affine_simple(x_j, theta[i][j]) at index i * n + j (the warp of
 * coalign_warp_fuse_nhwc: float64 grid cast to float32, bilinear, zero padding, align_corners=False), bit for bit what coalign_sp_pack makes of that kernel's
 * output; the float32 warped maps are never stored.
 *   x [n, H, W, C]; theta [R, n, 2, 3]: row (i, j) maps receiver i's grid into sender j (normalized_affine_matrix[b, i, j]).  C % 16 == 0. */
int coalign_v2v_warp_split(const float *x, int n, int R, int C, int H, int W, const double *theta, void *y_sp, int32_t *range_flag, void *stream);

/* (12b) Message, mask, aggregation and the GRU's input (V2VNetFusion.forward, fusion_in_one.py:173-293, lines 223-228 and 262-281):
 *   mask_ij = the warp of a map of ones = w00 + w01 + w10 + w11 of the masked tap weights, summed left to right;
 *   m_ij = (a_ij + e_i) * mask_ij;  agg_i = max_j m_ij (COALIGN_V2V_AGG_MAX) or (m_i0 + m_i1 + ...) / n summed in order of j (COALIGN_V2V_AGG_AVG);
 *   out_kind COALIGN_V2V_OUT_SP: out = the SplitMap [R, 2C, H, W] of [x_i | agg_i] (gru_flag);  COALIGN_V2V_OUT_NHWC: out [R, H, W, C] = x_i + agg_i.
 *   a [R * n, H, W, C]: the convolution of the warped maps, without bias; e [R, H, W, C]: the ego term, carrying msg_cnn's bias; x [>= R, H, W, C]; theta as (12a).
 *   An agent warped wholly outside the map contributes zeros, which take part in the max and the mean.  C % 16 == 0; another agg or out_kind UNSUPPORTED. */
int coalign_v2v_aggregate(const float *a, const float *e, const float *x, int n, int R, int C, int H, int W, const double *theta, int agg, int out_kind, void *out,
                          int32_t *range_flag, void *stream);

/* (12c) The gate of ConvGRUCell.forward (opencood/models/sub_modules/convgru.py:48-70) with a zero hidden state, as V2VNetFusion (fusion_in_one.py:173-293) always
 * calls it: out = sigmoid(y[..., :Ch]) * tanh(y[..., Ch:]), fp32 arithmetic, expf accuracy.
 *   y [R, H, W, 2 Ch]; out [R, H, W, Ch] float32 (COALIGN_V2V_OUT_NHWC) or the SplitMap [R, Ch, H, W] (COALIGN_V2V_OUT_SP).  Ch % 16 == 0; R counts maps and is
 *   not limited to 8; R < 0 or 2 Ch H W R >= 2^31 COALIGN_ERR_BAD_SHAPE, R = 0 COALIGN_OK without a launch. */
int coalign_v2v_gate(const float *y, int R, int Ch, int H, int W, int out_kind, void *out, int32_t *range_flag, void *stream);

#ifdef __cplusplus
}
#endif

#endif
