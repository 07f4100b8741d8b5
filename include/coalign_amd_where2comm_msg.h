/* Extension header of ABI version 2 (include/coalign_amd.h keeps its 68 entry points, the eleven earlier extension headers their 2 / 1 / 4 / 3 / 2 / 3 / 3 / 3 / 3 /
 * 7 / 2): Where2comm's MESSAGES -- what an agent transmits once its communication mask is known, and a fusion that reads it.  Part of the product library
 * libcoalign_hip.so; same conventions as include/coalign_amd_where2comm.h (status codes, every shape / pointer check before any HIP call, everything on the
 * caller's stream, no allocation, no host read-back: safe inside a captured graph; the same input gives the same bits).
 *
 * THE REFERENCE HAS NO COUNTERPART of any of this: its Communication (opencood/models/comm_modules/where2comm.py:9-78) and Where2comm
 * (opencood/models/fuse_modules/where2comm_attn.py:224-341) multiply dense maps by masks and stop there.  The format is this project's.
 *
 * One message per sending agent; per level l (1..3 levels, C_l in {64, 128, 256}, any H_l, W_l), all on the device, all of static shape:
 *   bits[l]   uint32 [H_l, Wd_l], Wd_l = ceil(W_l / 32): bit (x & 31) of word [y, x >> 5] is the mask at (y, x); padding bits are zero
 *   rows[l]   float32 [cap_l, C_l], cap_l = max(1, H_l W_l): the first K_l rows are the masked pixels' channel vectors in raster order (y major, x ascending),
 *             copied bit for bit; rows from K_l on are never written
 *   count     int32 [levels]: the K_l
 * and, made by sender and receiver alike and never transmitted,
 *   rank[l]   int32 [H_l, Wd_l]: the number of set bits before that word in raster order; pixel (y, x), when set, is row rank[y, x >> 5] + popcount(word & lower bits).
 *
 * ON THE WIRE (coalign_amd.where2comm.W2Message.to_wire / from_wire; little-endian 32-bit words throughout):
 *   words 0..3             0x4D433257 ("W2CM"), format version 1, levels, 0
 *   words 4 + 4 l .. + 3   C_l, H_l, W_l, K_l for l = 0, 1, 2 (zeros for the levels the message does not have): a header of 64 bytes
 *   then bits[0], bits[1], ... (H_l Wd_l words each), then rows[0][:K_0], rows[1][:K_1], ... (K_l C_l float32 each)
 *   size = 64 + sum over l of 4 (H_l Wd_l + K_l C_l) bytes. */
#ifndef COALIGN_AMD_WHERE2COMM_MSG_H
#define COALIGN_AMD_WHERE2COMM_MSG_H

#include "coalign_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Source kinds of (15c). */
#define COALIGN_W2COMM_SRC_DENSE 0
#define COALIGN_W2COMM_SRC_PACKED 1

/* (15a) bitmaps, rank tables and counts of n agents at `levels` levels in ONE launch (the reference has no counterpart: where2comm.py:61-71 stops at the 0 / 1
 * mask).  One workgroup per (agent, level): a word per lane, __popc, a scan over the workgroup's 64-lane wavefronts, a running carry from pass to pass.  Integer
 * arithmetic: exact, and the same in any order.
 *   sender form:   masks != NULL, HOST array of `levels` DEVICE pointers, masks[l] [n, H[l], W[l]] bytes (nonzero = set): bits, rank and count are written;
 *   receiver form: masks == NULL: bits is read (padding bits are ignored, not required to be zero), rank and count are written.
 *   H, W [levels] HOST int32, each >= 1 with H W < 2^31 (else COALIGN_ERR_BAD_SHAPE); 1 <= n <= 8 and 1 <= levels <= 3 (more: COALIGN_ERR_UNSUPPORTED; fewer:
 *   COALIGN_ERR_BAD_SHAPE); bits, rank: HOST arrays of `levels` DEVICE pointers, [n, H[l], ceil(W[l] / 32)] uint32 / int32, 4-byte aligned (else
 *   COALIGN_ERR_UNSUPPORTED); count [n, levels] int32 DEVICE. */
int coalign_w2comm_msg_index(int n, int levels, const int32_t *H, const int32_t *W, const uint8_t *const *masks, uint32_t *const *bits, int32_t *const *rank,
                             int32_t *count, void *stream);

/* (15b) rows of n agents at `levels` levels in ONE launch (the reference has no counterpart: it keeps the dense product x * mask, where2comm_attn.py:269, :275,
 * :334): every set pixel's C[l] floats go from the channels-last map to row rank + popcount(word & lower bits), 16-byte loads and stores, C / 8 lanes per pixel;
 * unset pixels write nothing, rows behind the count are not touched.
 *   x: HOST array of `levels` DEVICE pointers, x[l] [n, H[l], W[l], C[l]] float32; bits, rank as (15a) gives them; rows[l] [n, max(1, H[l] W[l]), C[l]] float32;
 *   x and rows 16-byte aligned, bits and rank 4-byte (else COALIGN_ERR_UNSUPPORTED); C[l] in {64, 128, 256}, n <= 8, levels <= 3 (else COALIGN_ERR_UNSUPPORTED);
 *   C H W < 2^31 (else COALIGN_ERR_BAD_SHAPE).  A row number outside the buffer (a rank table that is not these bits') is skipped, never written. */
int coalign_w2comm_msg_pack(int n, int levels, const float *const *x, const int32_t *C, const int32_t *H, const int32_t *W, const uint32_t *const *bits,
                            const int32_t *const *rank, float *const *rows, void *stream);

/* (15c) coalign_w2comm_fuse_nhwc (include/coalign_amd_where2comm.h: Where2comm.forward, where2comm_attn.py:224-341, the products of :269, :275 and :334,
 * warp_affine_simple of :292 and :335, AttenFusion :44-54 / MaxFusion :56-61) with a SOURCE per agent and scale in place of one tensor and a row table; for the
 * packed source the reference has no counterpart.  Entry [i * n + j] of kind / src / aux / rank (HOST arrays of n_scales * n) describes agent j at scale i:
 *   COALIGN_W2COMM_SRC_DENSE:  src = the agent's plane [H[i], W[i], C[i]] float32, aux = its mask bytes [H[i], W[i]] or NULL (all ones), rank ignored:
 *                              exactly coalign_w2comm_fuse_nhwc's tap;
 *   COALIGN_W2COMM_SRC_PACKED: src = rows, aux = bits, rank = rank of a message (all three required, COALIGN_ERR_NULL_POINTER otherwise): the tap's source pixel
 *                              is looked up; a set bit reads row rank + popcount, a clear bit contributes exactly zero WHATEVER rows holds -- its value is
 *                              replaced by zero after the load, not multiplied by a zero weight, so NaN behind the count and a count of 0 are harmless.
 * Same tile, lanes and arithmetic as coalign_w2comm_fuse_nhwc (csrc/w2comm_fuse_tile.h): on the same maps, masks and theta the two outputs are equal as values
 * (torch.equal); a zero may differ in sign, since a pixel that was not sent has no sign to give its product.
 *   mode COALIGN_FUSE_ATT or COALIGN_FUSE_MAX; C[i] in {64, 128, 256}, 1 <= n <= 8, 1 <= n_scales <= 3 (more: COALIGN_ERR_UNSUPPORTED), src and out 16-byte aligned,
 *   bits and rank 4-byte (else COALIGN_ERR_UNSUPPORTED); out[i] [Ho[i], Wo[i], C[i]]; theta [n, 2, 3] float64 DEVICE; C H W < 2^31 (else COALIGN_ERR_BAD_SHAPE). */
int coalign_w2comm_fuse_packed(int n_scales, const int32_t *C, const int32_t *H, const int32_t *W, const int32_t *kind, const float *const *src,
                               const void *const *aux, const int32_t *const *rank, float *const *out, const int32_t *Ho, const int32_t *Wo, int n,
                               const double *theta, int mode, void *stream);

#ifdef __cplusplus
}
#endif

#endif
