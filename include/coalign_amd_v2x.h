/* Extension header of ABI version 2 (include/coalign_amd.h keeps its 68 entry points, the extension headers coalign_amd_narrow.h, coalign_amd_align.h,
 * coalign_amd_narrow_sparse.h, coalign_amd_stage1.h, coalign_amd_disco.h and coalign_amd_v2v.h their 2 / 4 / 1 / 3 / 2 / 3): the heterogeneous agent attention of
 * V2X-ViT, the block of that transformer that mixes the agents.  Part of the product library libcoalign_hip.so; same conventions as include/coalign_amd.h (status
 * codes, every shape / pointer check before any HIP call, everything on the caller's stream, no allocation, a caller-supplied workspace with a size query: safe
 * inside a captured graph). */
#ifndef COALIGN_AMD_V2X_H
#define COALIGN_AMD_V2X_H

#include "coalign_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define COALIGN_V2X_DIM_HEAD 32
#define COALIGN_V2X_LN_EPS 1e-5f

/* (13a) Bytes of the parameter image (13c) reads for maps of C channels; 0 for a C it does not take.  The image holds one PreNorm(HGTCavAttention) layer
 * (opencood/models/sub_modules/hmsa.py:7-151 under base_transformer.py:7-14) of agent type 0, folded by the host in float64: LayerNorm's gamma / beta, relation_att[0]
 * (into the key rows), relation_msg[0] transposed (into the value rows) and dim_head^-0.5 (into the query rows) are part of the projections, so that
 *   [q | k' | v'] = Wqkv yhat + bqkv,   yhat = (x - mean) / sqrt(var + 1e-5)   and   out = x + Wa o + ba.
 * Layout, in the order the kernel's matrix operands are read:
 *   Wqkv [C / 16 steps][3C / 32 row tiles][64 lanes][8 h | 8 l] fp16: lane (r = lane & 31, half = lane >> 5) of row tile t and step s holds W[32 t + r][16 s + 8 half + j],
 *        j = 0 .. 7, as an sp16 pair (h = the value rounded to 22 bits, then to fp16 to nearest; l = (that value - h) * 2^10); rows [0, C) the queries, [C, 2C) the
 *        keys, [2C, 3C) the values, head m in rows 32 m .. 32 m + 31 of each;
 *   Wa   [C / 16 steps][C / 32 row tiles][64 lanes][8 h | 8 l] fp16: a_linears[0];
 *   4C floats: bqkv[3C], ba[C].
 * The attention output o = sum_j att_ij v'_j enters Wa as sp16 pairs: the host packs only weights for which |Wv' yhat + bv'| stays below 65504 for EVERY token
 * (sum yhat^2 <= C, hence |.|_r <= ||Wv'_r||_2 sqrt(C) + |bv'_r| for the rows [2C, 3C); o is a convex combination of such rows), so the kernel carries no range flag. */
size_t coalign_v2x_param_bytes(int C);

/* (13b) Bytes of the workspace (13c) needs: the projections [n][H W][3C] float32 of opencood/models/sub_modules/hmsa.py:7-151, written by its first launch and read
 * by its second.  0 for a shape (13c) does not take. */
size_t coalign_v2x_workspace_bytes(int n, int C, int H, int W);

/* (13c) x + HGTCavAttention(LayerNorm(x)) over the n agents of ONE frame, opencood/models/sub_modules/hmsa.py:7-151 under PreNorm (base_transformer.py:7-14) and the
 * residual of V2XFusionBlock.forward (v2xvit_basic.py:118-122), all agents of type 0 (as opencood/models/fuse_modules/fusion_in_one.py:295-352 calls it), eval mode,
 * in two launches (csrc/v2x_attn.hip):
 *   xw_j  = warp_affine_simple(x_j, theta_j) (the warp of coalign_warp_fuse_nhwc, bit for bit), or x_j itself when theta is NULL;
 *   out_i = xw_i + Wa concat_m( sum_j softmax_j(q_i^m . k'_j^m) v'_j^m ) + ba      for the receivers i < R, every sender j < n, head m of 32 channels.
 *   A sender warped wholly outside contributes LayerNorm(0) = beta as key and value, as the reference does.  Padded agents are not passed: they are masked keys there.
 *   x [n, H, W, C] float32 channels-last; theta [n, 2, 3] float64 or NULL; params: the image of (13a), params_bytes its size; out [R, H, W, C] float32; workspace of at
 *   least (13b) bytes.  x, params, out and workspace 16-byte aligned, theta 8-byte.
 *   C = 256 (8 heads) or C = 64 (2 heads), n <= 8, R = n or R = 1: anything else COALIGN_ERR_UNSUPPORTED.  n or R < 0, R > n, C / H / W < 1, C * H * W >= 2^31, a
 *   params_bytes that is not (13a) or a workspace_bytes below (13b): COALIGN_ERR_BAD_SHAPE.  n = 0 or R = 0 returns COALIGN_OK without a launch.
 *   The two projections run on the fp16 matrix cores with sp16 operand pairs (22 significant bits, fp32 accumulation); LayerNorm's statistics, the scores, the
 *   softmax over the senders and the residual are fp32. */
int coalign_v2x_agent_attention(const float *x, int n, int R, int C, int H, int W, const double *theta, const void *params, size_t params_bytes, float *out,
                                void *workspace, size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif

#endif
