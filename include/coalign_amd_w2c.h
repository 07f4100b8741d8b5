/* Extension header of ABI version 2 (include/coalign_amd.h keeps its 68 entry points, the eight earlier extension headers their 2 / 1 / 4 / 3 / 2 / 3 / 3 / 3):
 * what When2com's handshake fusion (When2commFusion, opencood/models/fuse_modules/fusion_in_one.py:354-431, with km_generator_v2 and AdditiveAttentin,
 * opencood/models/fuse_modules/when2com_fuse.py:253-270 and :342-363) computes after its 3 x 3 convolutions, which run on the SplitMap convolution kernels of
 * include/coalign_amd.h: the pooled key / query heads with the softmax over the agents, and the warp-and-weighted-sum of the agents' maps.  Part of the product
 * library libcoalign_hip.so; same conventions as include/coalign_amd.h (status codes, every shape / pointer check before any HIP call, everything on the caller's
 * stream, no allocation: safe inside a captured graph).
 *
 * n agents, agent 0 the ego: 1 <= n <= 8; n > 8 is COALIGN_ERR_UNSUPPORTED, a negative count COALIGN_ERR_BAD_SHAPE, n = 0 returns COALIGN_OK without a launch. */
#ifndef COALIGN_AMD_W2C_H
#define COALIGN_AMD_W2C_H

#include "coalign_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The heads' sizes (km_generator_v2, when2com_fuse.py:253-270; AdditiveAttentin, when2com_fuse.py:342-363): 128 channels pooled to 5 x 7 and flattened in
 * (channel, row, column) order = 4480 inputs, 256 and 128 hidden units, 128 attention features. */
#define COALIGN_W2C_CHANNELS 128
#define COALIGN_W2C_POOL_H 5
#define COALIGN_W2C_POOL_W 7
#define COALIGN_W2C_FEAT 4480
#define COALIGN_W2C_HIDDEN1 256
#define COALIGN_W2C_HIDDEN2 128
#define COALIGN_W2C_ATT 128

/* The parameter image of (13b), float32, in this order (the key net's block, then the query net's, per line):
 *   W1 [256][4480] (fc.0.weight as stored)                                      x 2
 *   b1 [256]                                                                    x 2
 *   W2^T [256][128] (fc.2.weight transposed), b2 [128]                          x 2
 *   T^T [128][128], tb [128]: the folded tail T = linear_feat.weight fc.4.weight (linear_context for the query net), tb = linear W fc.4.bias + linear bias   x 2 */
#define COALIGN_W2C_PARAM_FLOATS (2 * 256 * 4480 + 2 * 256 + 2 * (256 * 128 + 128) + 2 * (128 * 128 + 128))

/* (13a) Bytes of the workspace of (13b) (the partial sums of the first fully connected layer, written and read inside one call: nothing to initialise); replaces
 * nothing of the reference (fusion_in_one.py:354-431 allocates as it goes). */
size_t coalign_w2c_workspace_bytes(void);

/* (13b) Keys, query, logits and the softmax over the agents (When2commFusion.forward, fusion_in_one.py:354-431, lines 420-425; km_generator_v2.forward after its
 * conv1, when2com_fuse.py:253-270; AdditiveAttentin.forward with sparse=False, when2com_fuse.py:342-363):
 *   p_j = AdaptiveAvgPool2d((5, 7)) of key_map[j] (bins start = floor(i h / 5), end = ceil((i + 1) h / 5), likewise for 7 columns: overlapping when h or w does not
 *         divide, repeating when the map is smaller than the grid), flattened in (channel, row, column) order;
 *   k_j = T_k relu(W2_k relu(W1_k p_j + b1_k) + b2_k) + tb_k, q likewise from query_map with the query net's block;
 *   logits[j] = <k_j, q>, weights = softmax over j with the maximum subtracted.
 * fp32 accumulation, every sum in a fixed order (no float atomics: the same input gives the same bits), k_j independent of n.
 *   key_sp: SplitMap [n, key_channels, h, w] whose first 128 channels are the key maps (key_channels % 16 == 0 and >= 128, else COALIGN_ERR_UNSUPPORTED: 256 when
 *   the key and the query block ran as one stacked convolution); query_sp: SplitMap [1, 128, h, w] (the ego's -- inside a stacked map: the address of agent 0's
 *   channel 128, whose 128 channels are contiguous); both 16-byte aligned.  params: the image above, 16-byte aligned, param_bytes =
 *   4 COALIGN_W2C_PARAM_FLOATS (anything else COALIGN_ERR_BAD_SHAPE).  weights [n] float32; logits [n] float32 or NULL (a test aid).  Two launches: the pooled
 *   vectors times W1 spread over 256 workgroups (every W1 row is read once per call, not once per agent), then one workgroup for the rest.
 *   h, w >= 1; n key_channels h w >= 2^31 COALIGN_ERR_BAD_SHAPE; workspace_bytes below (13a) COALIGN_ERR_WORKSPACE. */
int coalign_w2c_score(const void *key_sp, int key_channels, const void *query_sp, int n, int h, int w, const float *params, size_t param_bytes, float *weights, float *logits,
                      void *workspace, size_t workspace_bytes, void *stream);

/* (13c) Warp and weighted sum (When2commFusion.forward, fusion_in_one.py:354-431, the warp_affine_simple of lines 415-417, and AdditiveAttentin.forward,
 * when2com_fuse.py:342-363, lines 360-362): out = sum_j weights[j] * warp_affine_simple(x[j], theta[j]), the warp of the channels-last fusion kernel of
 * include/coalign_amd.h in its no-fusion mode bit for bit (float64 grid cast to float32, bilinear, zero padding, align_corners=False), every product weights[j] * value rounded and the
 * products added in agent order.
 *   x [n, H, W, C] float32 channels-last, 16-byte aligned; theta [n, 2, 3] float64; weights [n] float32 on the device; out [1, H, W, C] float32 channels-last,
 *   16-byte aligned.  C % 16 == 0 (else COALIGN_ERR_UNSUPPORTED), any H, W; n C H W >= 2^31 COALIGN_ERR_BAD_SHAPE. */
int coalign_w2c_fuse(const float *x, int n, int C, int H, int W, const double *theta, const float *weights, float *out, void *stream);

#ifdef __cplusplus
}
#endif

#endif
