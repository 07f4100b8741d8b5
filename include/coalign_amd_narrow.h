/* Extension header of ABI version 2 (include/coalign_amd.h keeps its 68 entry points): the NARROW-OUTPUT 3x3 convolution that puts NaiveCompressor's encoder on
 * the SplitMap kernels.  Part of the product library libcoalign_hip.so; same conventions as include/coalign_amd.h (status codes, every shape check before any
 * HIP call, everything on the caller's stream, no allocation, no workspace: safe inside a captured graph). */
#ifndef COALIGN_AMD_NARROW_H
#define COALIGN_AMD_NARROW_H

#include "coalign_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* in_kind of coalign_conv3x3_sp_narrow */
#define COALIGN_NARROW_IN_SP 0   /* x is an SP map (9e) [N, Cin, H, W]                                  */
#define COALIGN_NARROW_IN_NHWC 1 /* x is channels-last float32 [N][H][W][Cin]; the loader splits it      */

/* (9h) The encoder of NaiveCompressor, opencood/models/sub_modules/naive_compress.py:5-31 (Conv2d(input_dim, input_dim / ratio, 3, padding 1) + BatchNorm
 * folded + ReLU, at canvas resolution): bytes of the weight image of coalign_conv3x3_sp_narrow for (Cin, Cout); 0 for a pair the kernel does not take
 * (Cin % 16 != 0, Cout not 16 or 32).  Image: [Cin / 16][9 taps][2 terms][2 channel halves][Cout][8 cin] fp16 sp16 pairs of the per-output-channel scaled
 * weights -- the tap-major order of (9b) with a Cout-wide block in place of 64 -- then 16 zero bytes, [Cout] float32 2^-k_c, [Cout] float32 2^k_c. */
size_t coalign_conv3x3_narrow_weight_bytes(int Cin, int Cout);

/* (9h) The same layer, opencood/models/sub_modules/naive_compress.py:5-31: y_sp = relu?(conv3x3(x, w, stride 1, pad 1) + bias) written as an SP map
 * [N, Cout, H, W] (9e), Cout = 16 or 32 (a narrower layer is zero-padded by the caller: padded channels come out exactly 0), Cin % 16 == 0, any H, W
 * (csrc/conv3x3_narrow.hip).  One workgroup computes every output channel of its pixels -- each input byte is read once -- and keeps the weight image in LDS
 * when it fits (Cin * Cout <= 64 * 32).
 *   x: per in_kind, 16-byte aligned.  An SP map travels by LDS-DMA; a channels-last float32 map (the dense canvas) is split to sp16 pairs in the loader, which
 *   replaces a coalign_sp_pack pass over it: the two kinds give the same bits.
 *   The arithmetic is that of (9e), product by product in the same order: the output equals the first Cout channels of coalign_conv3x3_sp on the same weights
 *   zero-padded to 64 output channels, bit for bit.  range_flag (may be NULL) as (9e).  N = 0 returns COALIGN_OK without a launch. */
int coalign_conv3x3_sp_narrow(const void *x, int in_kind, const void *w_narrow, const float *bias, void *y_sp, int N, int Cin, int Cout, int H, int W, int relu,
                              int32_t *range_flag, void *stream);

#ifdef __cplusplus
}
#endif

#endif
