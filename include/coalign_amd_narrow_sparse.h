/* Extension header of ABI version 2 (include/coalign_amd.h keeps its 68 entry points, include/coalign_amd_narrow.h its two): the narrow-output 3x3 convolution
 * READING THE SPARSE CANVAS, which lets a model with NaiveCompressor keep the one-launch pillar encoder and never materialise the dense canvas.  Part of the
 * product library libcoalign_hip.so; same conventions as include/coalign_amd.h (status codes, every shape / pointer check before any HIP call, everything on the
 * caller's stream, no allocation, no workspace: safe inside a captured graph). */
#ifndef COALIGN_AMD_NARROW_SPARSE_H
#define COALIGN_AMD_NARROW_SPARSE_H

#include "coalign_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* (9i) The encoder of NaiveCompressor, opencood/models/sub_modules/naive_compress.py:5-31, on the sparse canvas of (1b): coalign_conv3x3_sp_narrow (9h) whose
 * input is the pair (feature rows, cell stamps) instead of a map (csrc/conv3x3_narrow.hip, input kind 2).
 *   rows_sp [M_rows][Cin / 16][4 planes][8 x fp16]: the sp16 rows coalign_sp_pack_rows (9f) made of the encoder's float32 rows, 16-byte aligned, not NULL even
 *   with M_rows = 0.  stamps [N * H * W] 64-bit words (8-byte aligned) and state (word 0: the tag of the last completed frame): (1b)'s.  Input pixel (n, y, x) is
 *   row (stamp & 0xffffffff) when stamp >> 32 == state[0], state[0] != 0 and row < M_rows, and zero otherwise -- the rule of (9f)'s _sparse form, M_rows guard
 *   included: a stale canvas can never index past its array.  The row travels global -> LDS by LDS-DMA, one 16-byte source address per lane.
 *   w_narrow, bias, y_sp, Cout = 16 or 32, relu, range_flag: as (9h).  Cin % 16 == 0 and Cin >= 32: a tile's stamps are loaded one 16-channel interval before
 *   its first DMA instruction, so a single-interval layer (Cin = 16) returns COALIGN_ERR_UNSUPPORTED, as (9f)'s _sparse form does.  M_rows * Cin / 4 < 2^31 (row
 *   offsets are 32-bit).
 *   The arithmetic is that of (9h), product by product in the same order: the output equals coalign_conv3x3_sp_narrow on the densified canvas, bit for bit.
 *   N = 0 returns COALIGN_OK without a launch. */
int coalign_conv3x3_sp_narrow_sparse(const void *rows_sp, int M_rows, const void *stamps, const int32_t *state, const void *w_narrow, const float *bias, void *y_sp,
                                     int N, int Cin, int Cout, int H, int W, int relu, int32_t *range_flag, void *stream);

#ifdef __cplusplus
}
#endif

#endif
