/* Extension header of ABI version 2, the first one under include_open/ (include/ keeps its seventeen headers, include_ext/ its one; this directory takes every
 * later header: build.OPEN_HEADERS lists them): the two operations of the SECOND detectors' SSFA neck (opencood/models/sub_modules/cia_ssd_utils.py:6-55, layers
 * built by get_conv_layers, cia_ssd_utils.py:58-74) that had no kernel -- the 3 x 3 / stride-2 transposed convolution and the per-pixel two-way softmax blend --
 * reading and writing SplitMaps (include/coalign_amd.h (9e)), so that every other layer of the neck runs on coalign_conv3x3_sp / coalign_conv3x3_sp_s2 / the
 * pointwise kernel.  Part of the product library libcoalign_hip.so; same conventions as include/coalign_amd_lss_bev.h (status codes, every shape / support /
 * pointer / alignment check before any HIP call, everything on the caller's stream, no allocation, no workspace: safe inside a captured graph; a fixed summation
 * order, no atomics on data: the same input gives the same bits).
 *
 * SplitMap [N, C, H, W]: fp16 [N][C / 16][4 planes][H][W][8], plane = 2 * (8-channel half) + term, term 0 = h, term 1 = l' of the sp16 pair (csrc/common.h).
 * Both kernels OR bit 0 into *range_flag (may be NULL) when a value they store in a SplitMap exceeds the pair's range (|y| > 65504). */
#ifndef COALIGN_AMD_SSFA_H
#define COALIGN_AMD_SSFA_H

#include "coalign_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define COALIGN_DECONV3X3_MAX_COUT 1024 /* = the SplitMap convolutions' limit (backbone.SP_MAX_COUT) */
#define COALIGN_DECONV3X3_TILE_H 8      /* a workgroup's tile of INPUT pixels */
#define COALIGN_DECONV3X3_TILE_W 16
#define COALIGN_SSFA_BLEND_MAX_C 512

/* (19a) Bytes of the weight image (19b) reads; 0 unless Cin % 16 == 0, Cin >= 16, Cout % 64 == 0 and 64 <= Cout <= COALIGN_DECONV3X3_MAX_COUT.  Equal to
 * coalign_conv3x3_emu_weight_bytes_ex(Cin, Cout, 16, 1) and the SAME image: the tap-major terms-16 image of the ConvTranspose2d weight [Cin, Cout, 3, 3]
 * (cia_ssd_utils.py:6-55: deconv_block_0 / deconv_block_1; cia_ssd_utils.py:58-74: ConvTranspose2d without bias + BatchNorm2d(eps 1e-3) + ReLU) read as a
 * convolution weight [Cout, Cin, 3, 3] with its taps NOT flipped, the BatchNorm scale folded into it: tap 3 ky + kx of the image is w[:, :, ky, kx]. */
size_t coalign_deconv3x3_s2_weight_bytes(int Cin, int Cout);

/* (19b) y = act(deconv3x3(x, w, stride 2, padding 1, output_padding 1) + bias) [+ residual], written as a SplitMap (kernel deconv3x3_s2_sp):
 * `self.deconv_block_0(x_trans_1) + x_trans_0` and `self.deconv_block_1(x_trans_1)` (cia_ssd_utils.py:6-55, lines 45-46 of forward; the layers:
 * cia_ssd_utils.py:58-74), BatchNorm folded by the host.  The residual is added AFTER the activation, as line 45 does.
 *   x_sp: SplitMap [N, Cin, h, w]; w_image: (19a); bias [Cout] float32 (the folded BatchNorm shift); residual: NULL or [N, 2h, 2w, Cout] float32, the logical map
 *   [N, Cout, 2h, 2w] in channels-last memory; y_sp: SplitMap [N, Cout, 2h, 2w], EVERY element written; relu in {0, 1}.
 *   Definition: out[co, 2y - 1 + ky, 2x - 1 + kx] += x[ci, y, x] w[ci, co, ky, kx].  Per output parity (Y mod 2, X mod 2), with (i, j) = (Y / 2, X / 2):
 *     (0, 0): tap (1, 1) of x[i, j];     (0, 1): taps (1, 2) of x[i, j], (1, 0) of x[i, j + 1];     (1, 0): taps (2, 1) of x[i, j], (0, 1) of x[i + 1, j];
 *     (1, 1): taps (2, 2) of x[i, j], (2, 0) of x[i, j + 1], (0, 2) of x[i + 1, j], (0, 0) of x[i + 1, j + 1]  -- each class in THIS order.
 *   Inputs beyond row h - 1 or column w - 1 are zeros (lanes whose group lies outside the map fetch the weight image's 16 zero bytes); nothing outside x is read.
 *   Arithmetic: that of coalign_conv3x3_sp -- sp16 pairs on v_mfma_f32_32x32x16_f16, accumulator `acc` takes w_h x_h, `accl` takes w_h x_l' then w_l' x_h,
 *   t = acc + 2^-10 accl, v = max(t 2^-k_c + bias, floor), y = v + residual.  An implicit GEMM at the LOW resolution: a workgroup (8 wavefronts) owns
 *   COALIGN_DECONV3X3_TILE_H x COALIGN_DECONV3X3_TILE_W input pixels x 64 output channels; its patch (the tile + one row below + one column to the right) and one
 *   16-channel interval of the weights travel global -> LDS by LDS-DMA, double buffered, one barrier per interval.  A wavefront owns 2 x 16 input pixels x 32
 *   output channels and holds the accumulators of all four classes; per interval it runs the nine taps in DESCENDING 3 ky + kx, each into its class: 2.25 taps per
 *   output pixel.  Intervals ascend.  No split over K.  This is the order in which coalign_conv3x3_sp (whole tiles) meets the non-zero taps of the zero-stuffed
 *   map with the 180-degree-flipped kernel, so the two agree bit for bit (tests/test_ssfa_gpu.py).
 *   N < 0, h < 1, w < 1, N (2h) (2w) >= 2^31: COALIGN_ERR_BAD_SHAPE; Cin or Cout outside (19a)'s set, a relu outside {0, 1}: COALIGN_ERR_UNSUPPORTED; a NULL
 *   pointer (residual and range_flag excepted), x_sp / w_image / y_sp / residual not aligned to 16 bytes, bias or range_flag to 4: COALIGN_ERR_NULL_POINTER.
 *   N = 0 returns COALIGN_OK without a launch. */
int coalign_deconv3x3_s2_sp(const void *x_sp, const void *w_image, const float *bias, const float *residual, void *y_sp, int N, int Cin, int Cout, int h, int w,
                            int relu, int32_t *range_flag, void *stream);

/* (19c) The blend of the neck's two branches in ONE launch (kernel ssfa_blend): `x_weight_0 = self.w_0(x_output_0)`, `x_weight_1 = self.w_1(x_output_1)`, the
 * softmax over the two and `x_output_0 * x_weight[:, 0:1] + x_output_1 * x_weight[:, 1:]` (cia_ssd_utils.py:6-55, lines 50-53 of forward; w_0 / w_1 are
 * Conv2d(128, 1, 1) without bias + BatchNorm2d, cia_ssd_utils.py:58-74, folded by the host into wa / wb and the scalars bias_a / bias_b).
 *   a, b [N, H, W, C] float32: the logical maps [N, C, H, W] in channels-last memory; wa, wb [C] float32.  Per pixel
 *     la = sum_c wa[c] a[c] + bias_a, lb likewise;   p = 1 / (1 + exp(lb - la));   y[c] = a[c] p + b[c] (1 - p)      (all float32).
 *   Order of a sum: 16 lanes share a pixel; lane k takes the 8-channel groups k, k + 16, ... ascending, the channels of a group ascending, by fused
 *   multiply-add into one partial that starts at 0; the 16 partials are added pairwise over lane distance 1, 2, then mirrored over 8 and 16 lanes; the bias last.
 *   exp overflows to +inf and underflows to 0 without a NaN: lb - la = +200 gives p = 0, -200 gives p = 1.
 *   y_nhwc: NULL or [N, H, W, C] float32 channels-last; y_sp: NULL or SplitMap [N, C, H, W] holding coalign_sp_pack(y_nhwc), bit for bit.  At least one of them.
 *   One pass over a and b, 16-byte loads and stores.
 *   N < 0, H < 1, W < 1, N H W >= 2^31: COALIGN_ERR_BAD_SHAPE; C % 16 != 0, C < 16 or C > COALIGN_SSFA_BLEND_MAX_C: COALIGN_ERR_UNSUPPORTED; a / b / wa / wb
 *   NULL, both outputs NULL, a / b / wa / wb / y_nhwc / y_sp not aligned to 16 bytes, range_flag to 4: COALIGN_ERR_NULL_POINTER.  N = 0 returns COALIGN_OK without
 *   a launch. */
int coalign_ssfa_blend(const float *a, const float *b, const float *wa, const float *wb, float bias_a, float bias_b, float *y_nhwc, void *y_sp, int N, int C,
                       int H, int W, int32_t *range_flag, void *stream);

#ifdef __cplusplus
}
#endif

#endif
