/* Extension header of ABI version 2 (include/coalign_amd.h keeps its 68 entry points, the fourteen earlier extension headers their 2 / 1 / 4 / 3 / 2 / 3 / 3 / 3 /
 * 3 / 7 / 2 / 3 / 2 / 3): the two operations of the camera model's BEV encoder (BevEncodeMSFusion, opencood/models/sub_modules/lss_submodule.py:357-417) that
 * had no kernel -- the 7 x 7 / stride-2 stem and the bilinear x 2 up-sampling with concatenation of `Up` -- both writing a SplitMap (include/coalign_amd.h (9e)),
 * so that every 3 x 3 convolution behind them runs on coalign_conv3x3_sp / coalign_conv3x3_sp_s2.  Part of the product library libcoalign_hip.so; same
 * conventions as include/coalign_amd_lss.h (status codes, every shape / pointer / alignment check before any HIP call, everything on the caller's stream, no
 * allocation, no workspace: safe inside a captured graph; a fixed summation order: the same input gives the same bits).
 *
 * SplitMap [N, C, H, W]: fp16 [N][C / 16][4 planes][H][W][8], plane = 2 * (8-channel half) + term, term 0 = h, term 1 = l' of the sp16 pair (csrc/common.h).
 * Both kernels OR bit 0 into *range_flag (may be NULL) when a value they store exceeds the pair's range (|y| > 65504). */
#ifndef COALIGN_AMD_LSS_BEV_H
#define COALIGN_AMD_LSS_BEV_H

#include "coalign_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define COALIGN_CONV7X7_COUT 64
#define COALIGN_CONV7X7_MAX_CIN 512

/* (18a) Bytes of the weight image (18b) reads for Cin input channels; 0 unless Cin % 16 == 0 and 16 <= Cin <= COALIGN_CONV7X7_MAX_CIN.  The image holds the
 * stem `conv1` of BevEncodeMSFusion with `bn1` folded into it (opencood/models/sub_modules/lss_submodule.py:19-38, 369-372, 402-404: the convolution and the
 * BatchNorm of the constructor, applied by `x = self.bn1(self.conv1(x))` in forward), in the terms-16 conventions of coalign_conv3x3_emu_weight_bytes_ex:
 *   [Cin / 16 intervals][7 ky][7 kx][2 terms][2 channel halves][64 cout][8 cin] fp16: every output channel multiplied by the power of two 2^k_c that puts its
 *   largest weight into [2^13, 2^14), rounded to 22 significant bits (ties away from zero); term 0 = that value to fp16 (nearest), term 1 = (value - term 0) 2^10;
 *   then 16 zero bytes, [64] float32 2^-k_c, [64] float32 2^k_c.
 * One (interval, ky) slice -- seven taps -- is 28 672 contiguous bytes: what the kernel moves to LDS per barrier interval. */
size_t coalign_conv7x7_s2_weight_bytes(int Cin);

/* (18b) y = act(conv7x7(x, w, stride 2, pad 3) + bias) with 64 output channels, written as a SplitMap (kernel conv7x7_s2_sp): the stem
 * `self.relu(self.bn1(self.conv1(x)))` of BevEncodeMSFusion (opencood/models/sub_modules/lss_submodule.py:19-38, 369-372, 402-404), BatchNorm folded by the host.
 *   x [N, H, W, Cin] float32: the logical map [N, Cin, H, W] in channels-last memory (what coalign_lss_pool writes), read in place; w_image: (18a); bias [64]
 *   float32 (the folded BatchNorm shift); y_sp: SplitMap [N, 64, Ho, Wo], Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1; relu in {0, 1}.
 *   Arithmetic: the fp16 mode of coalign_conv3x3_sp -- both operands rounded to 22 bits and entering v_mfma_f32_32x32x16_f16 as sp16 pairs, three products per
 *   fp32 product (w_h x_h into one fp32 accumulator, w_h x_l' + w_l' x_h into a second that enters with 2^-10), y = sum 2^-k_c + bias.  The input is split by
 *   the kernel while it stages a patch to LDS.  An implicit GEMM with K = 49 Cin: one matrix instruction = the 16 channels of one tap, summed interval by
 *   interval, ky by ky, kx by kx -- a fixed order, no split over K.
 *   A workgroup (8 wavefronts) owns 8 x 32 output pixels; its 21 x 69 input patch lies in LDS DE-INTERLEAVED BY COLUMN PARITY (row = [35 even columns | 35 odd
 *   columns] of 16-byte groups), so that the 32 lanes of a stride-2 operand read touch 32 consecutive groups: conflict-free for ds_read_b128.
 *   N < 0, H < 1, W < 1, N H W >= 2^31: COALIGN_ERR_BAD_SHAPE; Cin % 16 != 0, Cin < 16 or Cin > COALIGN_CONV7X7_MAX_CIN, a relu outside {0, 1}:
 *   COALIGN_ERR_UNSUPPORTED; a NULL pointer (range_flag excepted), x / w_image / y_sp not aligned to 16 bytes, bias or range_flag to 4:
 *   COALIGN_ERR_NULL_POINTER.  N = 0 returns COALIGN_OK without a launch.  The kernel reads nothing outside x (padding is zeros made in registers) and writes
 *   only y_sp and the range word. */
int coalign_conv7x7_s2_sp(const float *x, const void *w_image, const float *bias, void *y_sp, int N, int Cin, int H, int W, int relu, int32_t *range_flag,
                          void *stream);

/* (18c) y = SplitMap of cat([skip, up(low)], dim = 1) in ONE pass (kernel up2x_concat_sp): `Up.forward` up to its convolutions,
 * `torch.cat([x2, self.up(x1)], dim=1)` (opencood/models/sub_modules/lss_submodule.py:19-38, 369-372, 402-404) with
 * nn.Upsample(scale_factor=2, mode='bilinear', align_corners=True) (opencood/models/sub_modules/lss_submodule.py:23-24).
 *   skip [N, 2h, 2w, Cs] float32 and low [N, h, w, Cl] float32, both channels-last memory; y_sp: SplitMap [N, Cs + Cl, 2h, 2w].
 *   Channels [0, Cs) hold the pairs coalign_sp_pack makes of skip, bit for bit.  Channel Cs + c at (Y, X) is the bilinear value of low[:, c]: source row
 *   Y (h - 1) / (2h - 1) (0 when h = 1), its integer part y0 and fraction ly taken EXACTLY from the integer division, neighbour min(y0 + 1, h - 1), the same
 *   along x; the four-tap sum is evaluated in float64, rounded to float32 once and then to the pair.  No float32 up-sampled map and no concatenated float32
 *   map exist.  EVERY element of y_sp is written.  16-byte loads along the channels, 16-byte stores along the pixels.
 *   N < 0, h < 1, w < 1, N (2h) (2w) >= 2^31: COALIGN_ERR_BAD_SHAPE; Cs or Cl not a positive multiple of 16, or more than
 *   2^36 output values: COALIGN_ERR_UNSUPPORTED; a NULL pointer
 *   (range_flag excepted), skip / low / y_sp not aligned to 16 bytes, range_flag to 4: COALIGN_ERR_NULL_POINTER.  N = 0 returns COALIGN_OK without a launch. */
int coalign_up2x_concat_sp(const float *skip, const float *low, void *y_sp, int N, int Cs, int Cl, int h, int w, int32_t *range_flag, void *stream);

#ifdef __cplusplus
}
#endif

#endif
