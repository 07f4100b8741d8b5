/* Extension header of ABI version 2 (include/coalign_amd.h keeps its 68 entry points, the twelve earlier extension headers their 2 / 1 / 4 / 3 / 2 / 3 / 3 / 3 / 3 /
 * 7 / 2 / 3): the feed-forward block of V2X-ViT's encoder layers, x + FeedForward(LayerNorm(x)), in ONE launch.  Part of the product library libcoalign_hip.so; same
 * conventions as include/coalign_amd_v2x_window.h (status codes, every shape / pointer check before any HIP call, everything on the caller's stream, no allocation,
 * no workspace: safe inside a captured graph; no atomics: the same input gives the same bits). */
#ifndef COALIGN_AMD_V2X_FFN_H
#define COALIGN_AMD_V2X_FFN_H

#include "coalign_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define COALIGN_V2X_FFN_LN_EPS 1e-5f
#define COALIGN_V2X_FFN_MAX_HIDDEN 512

/* (16a) Bytes of the parameter image (16b) reads for tokens of C channels and a hidden width M; 0 for a pair it does not take (C in {64, 256}; M % 32 == 0,
 * 32 <= M <= COALIGN_V2X_FFN_MAX_HIDDEN).  The image holds one PreNorm(FeedForward) layer -- opencood/models/sub_modules/base_transformer.py:7-14 (PreNorm) over
 * base_transformer.py:17-29 (FeedForward: Linear, GELU, Dropout, Linear, Dropout) -- folded by the host in float64: LayerNorm's gamma goes into the columns of the
 * first linear, beta becomes part of its bias,
 *   W1' = W1 diag(gamma),   b1' = W1 beta + b1,   so that   net(LayerNorm(x)) = W2 GELU(W1' yhat + b1') + b2,   yhat = (x - mean) / sqrt(var + 1e-5).
 * Layout, in the order the kernel reads it:
 *   W1' [C / 16 steps][M / 32 row tiles][64 lanes][8 h | 8 l] fp16: the lane order of include/coalign_amd_v2x_window.h (14a) -- lane (r = lane & 31, half = lane >> 5)
 *        of row tile t and step s holds W[32 t + r][16 s + 8 half + j], j = 0 .. 7, as an sp16 pair (h = the value rounded to 22 bits, then to fp16 to nearest;
 *        l = (that value - h) * 2^10);
 *   W2  [M / 16 steps][C / 32 row tiles][64 lanes][8 h | 8 l] fp16, the same lane order;
 *   floats: b1'[M], b2[C].
 * The hidden activations enter the second product as sp16 pairs: the host packs only weights for which |W1' yhat + b1'| stays below 65504 for EVERY token
 * (sum yhat^2 <= C, hence |.|_r <= ||W1'_r||_2 sqrt(C) + |b1'_r|), so the kernel carries no range flag. */
size_t coalign_v2x_ffn_param_bytes(int C, int M);

/* (16b) out = x + W2 GELU(W1' yhat + b1') + b2 per token, in ONE launch (csrc/v2x_ffn.hip): PreNorm (base_transformer.py:7-14) of FeedForward
 * (base_transformer.py:17-29) with the residual of V2XTEncoder.forward (v2xvit_basic.py:179, `x = ff(x) + x`), eval mode (no dropout), the exact GELU
 * (0.5 z (1 + erf(z / sqrt 2))).
 *   x [tokens, C] float32 -- any channels-last [n, H, W, C] map is that; params: the image of (16a), params_bytes its size; out [tokens, C] float32, a buffer of
 *   its own; x, params and out 16-byte aligned.
 *   C in {64, 256}, M % 32 == 0 with 32 <= M <= 512: anything else COALIGN_ERR_UNSUPPORTED, as is out == x.  tokens < 0, C < 1, M < 1,
 *   tokens * max(C, M) >= 2^31 or a params_bytes that is not (16a): COALIGN_ERR_BAD_SHAPE.  A NULL or misaligned x, params or out: COALIGN_ERR_NULL_POINTER.
 *   tokens = 0 returns COALIGN_OK without a launch.
 *   A workgroup owns 32 consecutive tokens (the last one masks its stores and reads nothing behind `tokens`); tokens are independent, so the result of a token
 *   does not depend on its neighbours or on where a map ends.  LayerNorm's statistics, GELU and the residual are fp32; both products run on the fp16 matrix cores
 *   with sp16 operand pairs (22 significant bits, fp32 accumulation), yhat and the hidden vector living in LDS between them. */
int coalign_v2x_feed_forward(const float *x, int tokens, int C, int M, const void *params, size_t params_bytes, float *out, void *stream);

#ifdef __cplusplus
}
#endif

#endif
