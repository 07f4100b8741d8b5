/* Entry points of the LABORATORY library only (coalign_amd/lib/libcoalign_hip_lab.so = the product sources + -DCOALIGN_LAB + the kernels below): variants that were
 * measured against the product's and not adopted.  They stay buildable and tested (tests/test_round4_gpu.py through coalign_amd.hip.lab_lib()); the product
 * library libcoalign_hip.so does not contain them.  (7-lab) is of another kind: a test entry onto a kernel the product does ship.  Same conventions as include/coalign_amd.h. */
#ifndef COALIGN_AMD_LAB_H
#define COALIGN_AMD_LAB_H

#include "coalign_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* (9c) Round 4: the stride-1 3x3 convolutions as Winograd F(2x2, 3x3) on the bf16 matrix cores -- 16 instead of 36 products per 2 x 2 outputs and
 * (cin, cout), fp32 operands by the same 3-way error-free bf16 split, fp32 accumulation (csrc/conv3x3_wino.hip).  Same layers as (9b):
 * BasicBlock.forward opencood/models/sub_modules/resblock.py:53-69 and DoubleConv downsample_conv.py:7-27.
 *   x, residual (may be NULL), y: CHANNELS-LAST, [N][H][W][C] float32, 16-byte aligned; Cin % 16 == 0, Cout % 64 == 0, any H, W.
 *   u_split: coalign_conv3x3_wino_weight_bytes(Cin, Cout) bytes: the transformed weights U = G g G^T (float64 on the host, G = [1 0 0; .5 .5 .5;
 *   .5 -.5 .5; 0 0 1]) as three bf16 terms in the order the kernel's wavefronts load them:
 *   [Cout / 64][Cin / 16][h 2][wave 8 = (c, i)][jj 2][term 3][lane 64][8] bf16 = term of U[i][2 h + jj][64 g + 32 c + lane % 32][16 k + 8 (lane / 32) + e].
 *   tile_block_w: 0 = chosen from W, 8 = blocks of 8 x 8 Winograd tiles, 16 = 4 x 16 tiles per workgroup.
 * No workspace.  y = relu?(conv3x3(x, g) + bias (+ residual)); against a float64 convolution the error is of the size of the direct
 * split-bf16 kernel's (measured: tests/test_round4_gpu.py). */
size_t coalign_conv3x3_wino_weight_bytes(int Cin, int Cout);
int coalign_conv3x3_wino(const float *x, const void *u_split, const float *bias, const float *residual, float *y, int N, int Cin, int Cout,
                         int H, int W, int relu, int tile_block_w, void *stream);

/* (7-lab) The voxeliser's last launch alone: gather_kernel of csrc/voxelize.hip on tables the caller made, with the grid rule of coalign_voxelize
 * ((7) of coalign_amd.h; the sequential loop it restates: sp_voxel_preprocessor.py:62-85).  The public entry fills a cell's bucket segment nearly sorted,
 * so the kernel's selection rounds (more than 64 candidates under the bound, over the LDS copy; more than 1024, over global memory) cannot be reached
 * through it; here the order inside a segment is the caller's (tests/test_voxel_limits_gpu.py).  All tables are DEVICE memory and must be well formed --
 * nothing on the device checks an index:
 *   points      [n_points, 4] float32, 16-byte aligned
 *   bucket      [n_points] int32: point indices, one contiguous segment per cell, any order inside a segment, no index twice in one segment
 *   seg         [capacity, 2] int32 per voxel row: (segment start in bucket, point count), 8-byte aligned; rows of <= 16 points are gathered from it
 *   cellinfo    [*, 4] int32, 16-byte aligned: (point count, unused, segment start, voxel row or -1 = dropped: skipped) for every entry of biglist
 *   biglist     [n_points / 17 + 1] int32: cellinfo rows of the cells of > 16 points; big_count [1] int32: how many of them are listed
 *   voxel_total [1] int32: M <= capacity, the voxel rows in use
 *   voxels      [capacity, max_points, 4] float32 out, 16-byte aligned: row v = the min(count, max_points) smallest point indices of its segment in
 *               ascending order, gathered from points, then zeros; rows >= M are not written.  1 <= max_points <= 64, 1 <= capacity <= n_points. */
int coalign_lab_voxelize_gather(const float *points, int64_t n_points, const int32_t *bucket, const int32_t *seg, const int32_t *cellinfo,
                                const int32_t *biglist, const int32_t *big_count, const int32_t *voxel_total, int max_points, float *voxels,
                                int64_t capacity, void *stream);

#ifdef __cplusplus
}
#endif

#endif
