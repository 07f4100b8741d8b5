/* Extension header of ABI version 2 (include/coalign_amd.h keeps its 68 entry points, the extension headers coalign_amd_narrow.h, coalign_amd_align.h,
 * coalign_amd_narrow_sparse.h, coalign_amd_stage1.h, coalign_amd_disco.h, coalign_amd_v2v.h and coalign_amd_v2x.h their 2 / 4 / 1 / 3 / 2 / 3 / 3): the pyramid window
 * attention of V2X-ViT with its split attention, the block of that transformer that mixes the tokens of one agent's map.  Part of the product library
 * libcoalign_hip.so; same conventions as include/coalign_amd.h (status codes, every shape / pointer check before any HIP call, everything on the caller's stream, no
 * allocation, a caller-supplied workspace with a size query: safe inside a captured graph). */
#ifndef COALIGN_AMD_V2X_WINDOW_H
#define COALIGN_AMD_V2X_WINDOW_H

#include "coalign_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define COALIGN_V2X_WINDOW_BRANCHES 3      /* branch b: windows of 4 << b tokens a side, heads of 16 << b channels, C / (16 << b) heads */
#define COALIGN_V2X_WINDOW_FUSE_NAIVE 0
#define COALIGN_V2X_WINDOW_FUSE_SPLIT_ATTN 1
#define COALIGN_V2X_WINDOW_LN_EPS 1e-5f
#define COALIGN_V2X_WINDOW_POS_FLOATS 1236 /* 7 x 7 + 15 x 15 + 31 x 31 relative-position entries, padded to a multiple of four */

/* (14a) Bytes of the parameter image (14c) reads for maps of C channels and the fuse method; 0 for a pair it does not take.  The image holds one
 * PreNorm(PyramidWindowAttention) layer (opencood/models/sub_modules/mswin.py:19-121 under base_transformer.py:7-14, SplitAttn of split_attn.py:6-63) with windows
 * (4, 8, 16), dim_head (16, 32, 64) and a relative position table, folded by the host in float64: the three bias-free to_qkv stack into ONE [9C, C] matrix, LayerNorm's
 * gamma goes into its columns, beta becomes the bias W beta, each branch's dim_head^-0.5 goes into its query rows and query bias, so that
 *   [q0 | k0 | v0 | q1 | k1 | v1 | q2 | k2 | v2] = Wqkv yhat + bqkv,   yhat = (x - mean) / sqrt(var + 1e-5).
 * Layout, in the order the kernels read it:
 *   Wqkv [C / 16 steps][9C / 32 row tiles][64 lanes][8 h | 8 l] fp16: lane (r = lane & 31, half = lane >> 5) of row tile t and step s holds W[32 t + r][16 s + 8 half + j],
 *        j = 0 .. 7, as an sp16 pair (h = the value rounded to 22 bits, then to fp16 to nearest; l = (that value - h) * 2^10); rows [3C b, 3C b + C) the queries of
 *        branch b, the next C rows its keys, the next C its values, head m in rows dim_head m .. dim_head m + dim_head - 1 of each;
 *   Wout [3 branches][C / 16 steps][C / 32 row tiles][64 lanes][8 h | 8 l] fp16: pwmsa[b].to_out[0].weight, the same lane order;
 *   floats: bqkv[9C], bout[3][C] (to_out[0].bias), then COALIGN_V2X_WINDOW_POS_FLOATS floats: pos_embedding of branch 0 (7 x 7, row-major), branch 1 (15 x 15),
 *        branch 2 (31 x 31), one zero;
 *   fuse = split attention only, all float32: WoutT[3][C][C] (WoutT[b][k][c] = to_out[0].weight[c][k] of branch b), fc1T[C][C] (fc1T[k][c] = fc1.weight[c][k]),
 *        bn1.weight[C], bn1.bias[C], fc2T[C][3C] (fc2T[k][r] = fc2.weight[r][k]).
 * The attention outputs o_b enter Wout_b as sp16 pairs: the host packs only weights for which |Wv_b yhat + bv_b| stays below 65504 for EVERY token (sum yhat^2 <= C,
 * hence |.|_r <= ||Wv_b,r||_2 sqrt(C) + |bv_b,r| for the rows [3C b + 2C, 3C b + 3C) of every branch; o_b is a convex combination of such rows), so the kernels carry
 * no range flag. */
size_t coalign_v2x_window_param_bytes(int C, int fuse);

/* (14b) Bytes of the workspace (14c) needs; 0 for a shape (14c) does not take.  It holds, all float32 and all three branches at once: the projections
 * [n][H W][9C] of mswin.py:47-53 (written by the first launch, read by the second), the attention outputs o_b [n][H W][3C] in raster token order (mswin.py:71-77 before
 * to_out; second launch to fourth), the partial channel sums of o_b [n][3][H W / 16][C] and the branch weights a [n][3][C] of split_attn.py:40-63. */
size_t coalign_v2x_window_workspace_bytes(int n, int C, int H, int W);

/* (14c) x + PyramidWindowAttention(LayerNorm(x)) for the n maps of ONE frame, every map on its own: opencood/models/sub_modules/mswin.py:19-121 (BaseWindowAttention
 * and PyramidWindowAttention) under PreNorm (base_transformer.py:7-14) with SplitAttn and RadixSoftmax (split_attn.py:6-63) and the residual of
 * V2XFusionBlock.forward (v2xvit_basic.py:118-122), eval mode, in three launches (fuse 0) or four (csrc/v2x_window.hip):
 *   o_b   = softmax_j(q_i . k_j + pos_b[xj - xi + ws - 1][yj - yi + ws - 1]) v_j  inside every ws x ws window, token i = xi ws + yi, x the row (mswin.py:9-16, 55-70);
 *   a     = 1 / 3 (fuse 0), or softmax_b(fc2(relu(LayerNorm(fc1(gap))))) with gap = sum_b (Wout_b mean_HW(o_b) + bout_b) per map (fuse 1);
 *   out   = x + sum_b a_b * (Wout_b o_b + bout_b).
 *   x [n, H, W, C] float32 channels-last; params: the image of (14a), params_bytes its size; out [n, H, W, C] float32, a buffer of its own; workspace of at least
 *   (14b) bytes.  x, params, out and workspace 16-byte aligned.
 *   C = 256, or C = 64 with fuse 0 (the reference hard-wires SplitAttn(256)); fuse 0 or 1; n <= 8; H and W multiples of 16: anything else COALIGN_ERR_UNSUPPORTED.
 *   n < 0, C / H / W < 1, C * H * W >= 2^31, a params_bytes that is not (14a) or a workspace_bytes below (14b): COALIGN_ERR_BAD_SHAPE.  n = 0 returns COALIGN_OK without
 *   a launch.  The projections run on the fp16 matrix cores with sp16 operand pairs (22 significant bits, fp32 accumulation); LayerNorm's statistics, the scores, the
 *   position bias, the softmax, the weighted sums inside the windows, the split attention and the residual are fp32.  The pooled sums are reduced in a fixed order
 *   (no atomics): the same input gives the same bits. */
int coalign_v2x_window_attention(const float *x, int n, int C, int H, int W, int fuse, const void *params, size_t params_bytes, float *out,
                                 void *workspace, size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif

#endif
