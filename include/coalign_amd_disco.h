/* Extension header of ABI version 2 (include/coalign_amd.h keeps its 68 entry points, the extension headers coalign_amd_narrow.h, coalign_amd_align.h,
 * coalign_amd_narrow_sparse.h and coalign_amd_stage1.h their 2 / 4 / 1 / 3): DiscoNet's pixel-weight fusion, the intermediate-fusion baseline beside CoAlign's
 * attention.  Part of the product library libcoalign_hip.so; same conventions as include/coalign_amd.h (status codes, every shape / pointer check before any
 * HIP call, everything on the caller's stream, no allocation, no workspace: safe inside a captured graph). */
#ifndef COALIGN_AMD_DISCO_H
#define COALIGN_AMD_DISCO_H

#include "coalign_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define COALIGN_DISCO_MAX_CHANNELS 384

/* (11a) Bytes of the parameter image (11b) reads for maps of C channels; 0 for a C it does not take.  The image holds PixelWeightLayer
 * (opencood/models/fuse_modules/disco_fuse.py:76-99) with its BatchNorms folded into the convolutions, as DiscoFusion.forward
 * (opencood/models/fuse_modules/fusion_in_one.py:144-171) applies it in eval mode, in the order the kernel's matrix operands are read:
 *   W1a [C / 16 steps][4 row tiles][64 lanes][8 h | 8 l] fp16: lane (r = lane & 31, half = lane >> 5) of row tile t and step s holds W1[32 t + r][16 s + 8 half + j],
 *       j = 0 .. 7, as an sp16 pair (h = the value rounded to 22 bits, then to fp16 to nearest; l = (that value - h) * 2^10) -- the columns [0, C) of conv1_1, which
 *       meet the warped neighbour map;
 *   W1b the same for the columns [C, 2C), which meet the unwarped ego map;
 *   W2  [8 steps][64 lanes][8 h | 8 l] fp16: conv1_2, W2[r][16 s + 8 half + j];
 *   436 floats: b1[128], b2[32], W3 as [2 halves][8 rows][16]: element q of (half, row o) is W3[o][8 (q >> 2) + 4 half + (q & 3)], b3[8], w4[8], b4, 3 of padding. */
size_t coalign_disco_param_bytes(int C);

/* (11b) DiscoFusion.forward of ONE frame, opencood/models/fuse_modules/fusion_in_one.py:144-171 with PixelWeightLayer,
 * opencood/models/fuse_modules/disco_fuse.py:76-99, in eval mode, in one launch (csrc/disco_fuse.hip):
 *   xw_j = warp_affine_simple(x_j, theta_j) for every agent j, the ego included (the warp of coalign_warp_fuse_nhwc: float64 grid cast to float32, bilinear, zero
 *   padding, align_corners=False);  s_j = PixelWeightLayer([xw_j | x_0]) with x_0 the unwarped ego map;  out = sum_j softmax_j(s_j) xw_j.  An agent warped wholly
 *   outside the map contributes zeros and still takes part in the softmax.
 *   x [n, H, W, C] float32 channels-last, agent 0 the ego; theta [n, 2, 3] float64, row 0 of the frame's normalised affine matrix; params: the image of (11a),
 *   params_bytes its size; out [H, W, C] float32 channels-last.  x, params and out 16-byte aligned.
 *   C % 32 == 0 and 32 <= C <= 384, n <= 8: anything else COALIGN_ERR_UNSUPPORTED.  n < 0, C / H / W < 1, C * H * W >= 2^31 or a params_bytes that is not
 *   coalign_disco_param_bytes(C): COALIGN_ERR_BAD_SHAPE.  n = 0 returns COALIGN_OK without a launch.
 *   The two matrix layers (C -> 128 -> 32) run on the fp16 matrix cores with sp16 operand pairs (22 significant bits, fp32 accumulation), the rest in fp32. */
int coalign_disco_fuse(const float *x, int n, int C, int H, int W, const double *theta, const void *params, size_t params_bytes, float *out, void *stream);

#ifdef __cplusplus
}
#endif

#endif
