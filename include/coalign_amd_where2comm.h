/* Extension header of ABI version 2 (include/coalign_amd.h keeps its 68 entry points, the ten earlier extension headers their 2 / 1 / 4 / 3 / 2 / 3 / 3 / 3 / 3 / 7):
 * Where2comm's confidence-masked fusion (Where2comm, opencood/models/fuse_modules/where2comm_attn.py:174-341, with AttenFusion :44-54 and MaxFusion :56-61, and
 * Communication, opencood/models/comm_modules/where2comm.py:9-78): the communication masks of every agent at every backbone level in one launch, and the pose-aware
 * warp and per-pixel fusion of the masked maps in one launch per frame.  Part of the product library libcoalign_hip.so; same conventions as include/coalign_amd.h
 * (status codes, every shape / pointer check before any HIP call, everything on the caller's stream, no allocation, no host read-back: safe inside a captured
 * graph; the same input gives the same bits). */
#ifndef COALIGN_AMD_WHERE2COMM_H
#define COALIGN_AMD_WHERE2COMM_H

#include "coalign_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Frames per call of (14a): more is COALIGN_ERR_UNSUPPORTED. */
#define COALIGN_W2COMM_MAX_GROUPS 64

/* (14a) The communication masks and rates (Communication.forward, where2comm.py:34-78, and the mask pyramid of Where2comm.forward, where2comm_attn.py:273-275),
 * one launch, in the reference's order:
 *   conf     = max over the A anchors of sigmoid(psm[:, a])                                        (where2comm.py:52)
 *   smoothed = cross-correlation of conf with weights [k, k], zero padding (k - 1) / 2, plus bias  (where2comm.py:55; k = 0: smoothed = conf, :57)
 *   mask     = smoothed > thre, a strict comparison                                                (where2comm.py:61)
 *   rates[b] = count(mask of frame b's agent 0) / (H W), counted in integers BEFORE the next step  (where2comm.py:63)
 *   the masks of the agents with an even index inside their frame become all ones                  (communication_mask_nodiag[::2] = 1, where2comm.py:69-71)
 *   masks[l] for l > 0 = 2 x 2, stride-2 max pool with floor of masks[l - 1]                       (F.max_pool2d(kernel_size=2), where2comm_attn.py:274)
 * fp32 arithmetic, the taps of the smoothing added in row-major order with fmaf, then the bias.
 *   psm [n_total, A, H, W] float32 DEVICE, the single-agent classification logits, 1 <= A <= 8 (more: COALIGN_ERR_UNSUPPORTED); group_len [n_groups] HOST int32,
 *   agents per frame, each 1..8 (more: COALIGN_ERR_UNSUPPORTED; fewer: COALIGN_ERR_BAD_SHAPE), sum == n_total, 1 <= n_groups <= COALIGN_W2COMM_MAX_GROUPS;
 *   weights [k * k] and bias [1] float32 DEVICE (the module's gaussian_filter.weight / .bias as stored), k odd and <= 9, or k = 0 with both ignored; an even k or
 *   k > 9 is COALIGN_ERR_UNSUPPORTED (with an even k the reference's padding (k - 1) // 2 changes the map size and its forward fails);
 *   levels 1..3 with H >> (levels - 1) >= 1 and W >> (levels - 1) >= 1 (else COALIGN_ERR_BAD_SHAPE);
 *   masks: HOST array of `levels` DEVICE pointers, masks[l] [n_total, H >> l, W >> l] one byte (0 / 1) per pixel; rates [n_groups] float32 DEVICE.
 *   n_total A H W >= 2^31 is COALIGN_ERR_BAD_SHAPE. */
int coalign_w2comm_masks(const float *psm, int n_total, int A, int H, int W, const int32_t *group_len, int n_groups, const float *weights, const float *bias,
                         int k, float thre, int levels, uint8_t *const *masks, float *rates, void *stream);

/* (14b) fuse(warp(x_j * mask_j)) on CHANNELS-LAST maps, up to three feature scales of ONE frame in one launch (Where2comm.forward, where2comm_attn.py:224-341: the
 * products of :269, :275 and :334, warp_affine_simple of :292 and :335, AttenFusion :44-54 / MaxFusion :56-61 of :295 and :338): the masked counterpart of
 * coalign_warp_fuse_nhwc (include/coalign_amd.h), same arguments plus masks[i] [n, H[i], W[i]] bytes (HOST array of DEVICE pointers; row r of masks[i] belongs to row r
 * of x[i], whatever `rows` says about the agent it holds).  Each of the four bilinear taps of agent j is weighted by the mask byte at the tap's SOURCE pixel; no
 * masked copy of a map is written.  With all-ones masks the output equals coalign_warp_fuse_nhwc's bit for bit; with any 0 / 1 masks it equals
 * coalign_warp_fuse_nhwc's on the maps multiplied by their masks beforehand, bit for bit (finite maps).
 *   mode: COALIGN_FUSE_ATT or COALIGN_FUSE_MAX; COALIGN_FUSE_NONE is COALIGN_ERR_UNSUPPORTED.  Limits as for coalign_warp_fuse_nhwc: C[i] in {64, 128, 256},
 *   1 <= n <= 8, any H, W, x and out 16-byte aligned, rows [n] HOST or NULL as in coalign_warp_fuse_rows. */
int coalign_w2comm_fuse_nhwc(int n_scales, const float *const *x, const int32_t *C, const int32_t *H, const int32_t *W, const uint8_t *const *masks,
                             float *const *out, const int32_t *Ho, const int32_t *Wo, int n, const double *theta, const int32_t *rows, int mode, void *stream);

#ifdef __cplusplus
}
#endif

#endif
