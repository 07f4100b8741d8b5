/* Extension header of ABI version 2 (include/coalign_amd.h keeps its 68 entry points, the thirteen earlier extension headers their 2 / 1 / 4 / 3 / 2 / 3 / 3 / 3 /
 * 3 / 7 / 2 / 3 / 2): Lift-Splat's frustum pooling -- the step of the camera model that turns per-camera image features and depth logits into the BEV map the
 * fusion families read.  Part of the product library libcoalign_hip.so; same conventions as include/coalign_amd_v2x_ffn.h (status codes, every shape / pointer /
 * alignment check before any HIP call, everything on the caller's stream, no allocation, no workspace: safe inside a captured graph; no float atomics: the same
 * input gives the same bits).
 *
 * The reference materialises depth x features ([A N, C, D, fH, fW], lss_submodule.py:134-136), sorts every frustum point by its voxel and takes differences of a
 * running sum (lift_splat_shoot.py:116-169).  Here the voxel of a point is computed once per camera rig (17a); the host turns those cells into an inverted index
 * -- per output cell the list of its points, ascending (coalign_amd.ops.build_lss_index) -- and a frame is (17b) + (17c): two launches.
 *
 * THE INDEX (read by (17c)), all int32 on the device:
 *   key      of the cell (z, y, x) of agent a: ((a ny + y) nx + x) nz + z -- the position of the cell's C channels in the channels-last output;
 *   starts   [cells + 1], cells = A ny nx nz: the points of key k are points[starts[k] .. starts[k + 1]), ascending in the flat point number
 *            ((m D + d) fH + h) fW + w, m = a N + n; starts[0] = 0, starts[cells] = n_points;
 *   points   [n_points, 2]: per listed point (row, prob) = ((m fH + h) fW + w, row D + d): the feature row and the element of (17b)'s output it multiplies;
 *   long     [n_long]: the keys whose list is longer than COALIGN_LSS_CHUNK, ascending. */
#ifndef COALIGN_AMD_LSS_H
#define COALIGN_AMD_LSS_H

#include "coalign_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define COALIGN_LSS_CHUNK 512
#define COALIGN_LSS_MAX_DEPTH 128

/* (17a) cell[(m, d, h, w)] = (z ny + y) nx + x inside the map of agent m / N, or -1 for a point that is dropped (kernel lss_cells; once per camera rig).
 * A FLOAT64 evaluation, from the float32 inputs, of LiftSplatShoot.get_geometry (opencood/models/lift_splat_shoot.py:80-102) on the frustum of create_frustum
 * (lift_splat_shoot.py:65-78), followed by voxel_pooling's index line (lift_splat_shoot.py:126) and its bounds test (lift_splat_shoot.py:133-135):
 *   p = inverse(post_rots) ((xs[w], ys[h], ds[d]) - post_trans);  p = (p.x p.z, p.y p.z, p.z);  g = rots inverse(intrins) p + trans;
 *   v = (g - lower) / dx per axis;  index = v truncated TOWARDS ZERO (the reference's .long(), not floor: a coordinate in (-1, 0) becomes index 0 and is kept);
 *   kept when 0 <= index < (nx, ny, nz) on all three axes.
 * rots, intrins, post_rots [A N, 3, 3], trans, post_trans [A N, 3]; xs [fW], ys [fH] (torch.linspace's values), ds [D] (depth_discretization,
 * opencood/utils/camera_utils.py:187-196, as float32); lower = bx - dx / 2 and dx: the float32 constants of gen_dx_bx (camera_utils.py:129-134) per axis x, y, z;
 * cell [A N, D, fH, fW] int32.  The matrices are inverted by their adjugates in float64: a singular matrix gives non-finite coordinates.  A non-finite coordinate, or
 * one at or beyond +-2^31, is DROPPED (-1); the reference leaves both undefined (the result of .long() on such a value depends on the platform).
 *   A, N, D, fH, fW < 1, nx, ny, nz < 1, A N D fH fW >= 2^31 or nx ny nz >= 2^31: COALIGN_ERR_BAD_SHAPE; a dx that is not a positive finite number, a non-finite
 *   lower: COALIGN_ERR_BAD_SHAPE; a NULL pointer, or one not aligned to 4 bytes: COALIGN_ERR_NULL_POINTER. */
int coalign_lss_cells(const float *rots, const float *trans, const float *intrins, const float *post_rots, const float *post_trans, int A, int N, const float *xs,
                      const float *ys, const float *ds, int D, int fH, int fW, float lower_x, float lower_y, float lower_z, float dx_x, float dx_y, float dx_z, int nx,
                      int ny, int nz, int *cell, void *stream);

/* (17b) prob[(m fH + h) fW + w][d] = softmax over d of depth_logit[m, d, h, w] (kernel lss_depth_prob): CamEncode.get_depth_dist
 * (opencood/models/sub_modules/lss_submodule.py:66-67) as called by CamEncode.forward (lss_submodule.py:134-135), the pixel's maximum subtracted first, the
 * hardware exponential.  depth_logit [M, D, fH, fW] float32 in plain NCHW memory (channels_last = 0) or in channels-last memory (channels_last = 1: a pixel's D
 * logits contiguous); prob [M fH fW, D] float32, a buffer of its own.
 *   M, fH, fW < 0, D < 1 or M fH fW D >= 2^31: COALIGN_ERR_BAD_SHAPE; D > COALIGN_LSS_MAX_DEPTH or a channels_last outside {0, 1}: COALIGN_ERR_UNSUPPORTED;
 *   a NULL or 4-byte-misaligned pointer: COALIGN_ERR_NULL_POINTER.  M fH fW = 0 returns COALIGN_OK without a launch. */
int coalign_lss_depth_prob(const float *depth_logit, int M, int D, int fH, int fW, int channels_last, float *prob, void *stream);

/* (17c) out[k][c] = sum over the points p of key k, in list order, of prob[p.prob] x_rows[p.row][c] (kernel lss_pool): the outer product of CamEncode.forward
 * (opencood/models/sub_modules/lss_submodule.py:134-136) and LiftSplatShoot.voxel_pooling (opencood/models/lift_splat_shoot.py:116-169) in one launch.
 *   x_rows [rows, C] float32: the image features [M, C, fH, fW] in channels-last memory (rows = M fH fW); prob: (17b)'s output [rows, D]; the index as described
 *   at the top; out [cells, C] float32 = [A, ny, nx, nz C]: the map [A, nz C, ny, nx] of the reference (rows = y, columns = x, channel z C + c, the order of
 *   `torch.cat(final.unbind(dim=2), 1)`, lift_splat_shoot.py:167) in CHANNELS-LAST memory -- a cell's C values are one contiguous 256- or 512-byte row, written
 *   by one wavefront with one store; plain NCHW would scatter them over C planes.  EVERY element of out is written by the launch (zeros for an empty list): no
 *   memset, no dependence on earlier contents.
 *   A list of at most COALIGN_LSS_CHUNK points is summed by one wavefront, lanes across the channels, in list order.  A longer list (a key of `long_cells`) is
 *   cut into chunks of COALIGN_LSS_CHUNK consecutive points (the last one shorter); the four wavefronts of a workgroup take chunks, each summed in list order, and
 *   the chunk sums are added in chunk order through LDS.  No atomics.
 *   C in {64, 128} and 1 <= D <= COALIGN_LSS_MAX_DEPTH: anything else COALIGN_ERR_UNSUPPORTED.  rows, n_points, cells, n_long < 0, n_long > cells,
 *   rows D >= 2^31 or n_points > 0 with rows = 0: COALIGN_ERR_BAD_SHAPE.  NULL out / starts with cells > 0, NULL x_rows / prob / points with n_points > 0, NULL
 *   long_cells with n_long > 0, x_rows / out not aligned to 16 bytes, points to 8, the others to 4: COALIGN_ERR_NULL_POINTER.  cells = 0 returns COALIGN_OK
 *   without a launch.  The kernel reads nothing outside [0, rows) and [0, n_points) whatever the index holds (entries outside are skipped), and writes only out.
 *   "Every element is written" presumes that `long_cells` is complete: the row of a list longer than COALIGN_LSS_CHUNK that `long_cells` does not name is left as it was. */
int coalign_lss_pool(const float *x_rows, const float *prob, int rows, int C, int D, const int *points, int n_points, const int *starts, int cells,
                     const int *long_cells, int n_long, float *out, void *stream);

#ifdef __cplusplus
}
#endif

#endif
