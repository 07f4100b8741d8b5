/* Extension header of ABI version 2, the second one under include_open/ (build.OPEN_HEADERS): the front of the SECOND detectors' sparse 3-D trunk -- raw point
 * clouds of all agents of a frame in, the INPUT SPARSE TENSOR of VoxelBackBone8x out: MeanVFE features, indices, a device count and the level-0 site index of
 * include_ext/coalign_amd_sparse3d.h, already built.  It restates SpVoxelPreprocessor.preprocess + collate_batch
 * (opencood/data_utils/pre_processor/sp_voxel_preprocessor.py:62-147), MeanVFE.forward (opencood/models/sub_modules/mean_vfe.py:26-30) and the two point filters of
 * opencood/utils/pcd_utils.py:41-88 without ever writing the [M, T, 4] voxel tensor.  Part of the product library libcoalign_hip.so; the conventions of
 * include_ext/coalign_amd_sparse3d.h apply (status codes, every shape / pointer / alignment check before any HIP call, everything on the caller's stream, no
 * allocation, no host read, every launch sized by P_cap and capacity: safe inside a captured graph, which may be replayed on other clouds of other lengths; integer
 * atomics only: the same input gives the same bits).  coalign_voxelize (include/coalign_amd.h) and its 20 971 520-cell limit are untouched: its dense per-cell tables
 * do not fit this grid (2816 x 800 x 40 cells per agent), the bitmap + prefix-count site index does.
 *
 * THE CONTRACT
 *   1. A point is VALID iff it passes the enabled filters (COALIGN_VOX_FILTER_EGO / COALIGN_VOX_FILTER_RANGE of include/coalign_amd.h, meaning the same) and each of
 *      floorf((p - lo) / vs) lies in [0, g) per axis: float32, IEEE divide, no contraction -- the expression of coalign_voxelize.  NaN coordinates are rejected.
 *      g = round((hi - lo) / vs) in float32 per axis, as coalign_voxelize converts voxel_size and lidar_range.
 *   2. The smallest valid point index in a cell of a cloud OPENS that cell.  A cell's voxel number is the rank of its opening point among the cloud's opening points;
 *      the cell is KEPT iff that number < max_voxels; points in cells that are not kept are ignored (spconv's sequential generator, which stops opening voxels at
 *      max_voxels but keeps filling the open ones).
 *   3. A kept voxel's points are its T = max_points smallest point indices, n = min(points in the cell, T), and
 *      features[c] = (((0 + p_0[c]) + p_1[c]) + ...) / (float)n in float32, ascending point order: the bits coalign_sp3d_mean_vfe gives on the zero-padded [T, 4] slots.
 *   4. ROW ORDER: rows are the kept voxels of all clouds in ASCENDING LINEAR CELL INDEX ((b D + z) H + y) W + x, b = the cloud -- this library's order for generated
 *      sites (coalign_sp3d_strided_sites), NOT the generator's first-appearance order.  The dense map of the trunk cannot depend on it: a layer adds its taps per output
 *      row in a fixed order and the strided layers sort anyway.
 *   5. *count = min(kept, capacity); on overflow the first `capacity` rows (ascending) are kept and COALIGN_SP3D_STATUS_OVERFLOW is ORed into *status.
 *      COALIGN_SP3D_STATUS_MAX_VOXELS is ORed in when some cloud opened max_voxels cells or more (its voxel count reached the limit); informational.  The caller zeroes
 *      *status.  cloud_counts[c] = kept voxels of cloud c BEFORE the capacity cut, cloud_counts[n_clouds] = their sum.
 *   6. `index` is the site index of (indices, *count) in exactly the layout of coalign_sp3d_index_workspace_bytes(n_clouds, D, H, W, capacity), rank = row:
 *      coalign_sp3d_neighbors and coalign_sp3d_to_dense answer as after coalign_sp3d_index_build(indices, count, ...).
 *   7. Rows at or past *count are not written; nothing outside the buffers is read or written whatever `points` and `offsets` hold.
 *
 * OFFSETS live on the DEVICE: int32 [n_clouds + 1].  The kernels clamp each entry to [0, P_cap] and make the sequence non-decreasing by a running maximum, so a
 * decreasing pair is an empty cloud and clouds never overlap; points in front of offsets[0] or behind offsets[n_clouds] belong to no cloud. */
#ifndef COALIGN_AMD_SP3D_VOXELIZE_H
#define COALIGN_AMD_SP3D_VOXELIZE_H

#include "coalign_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define COALIGN_SP3D_STATUS_MAX_VOXELS 2u      /* bit of the status word beside COALIGN_SP3D_STATUS_OVERFLOW (1u): a cloud reached max_voxels */
#define COALIGN_SP3D_VOXELIZE_MAX_POINTS 8     /* the limit of max_points (T): 1 .. 8 */
#define COALIGN_SP3D_VOXELIZE_MAX_CLOUDS 16
#define COALIGN_SP3D_VOXELIZE_MAX_P_CAP (1 << 27)

/* (20a) bytes of the workspace (20b) needs for P_cap points, n_clouds clouds and max_points slots per voxel (sp_voxel_preprocessor.py:62-147 sizes its arrays by
 * max_voxels x max_points instead): (2 + max_points) int32 per point + one per 1024-point block and cloud; 0 for anything (20b) refuses. */
size_t coalign_sp3d_voxelize_workspace_bytes(int P_cap, int n_clouds, int max_points);

/* (20b) points -> the input sparse tensor of VoxelBackBone8x with its site index: SpVoxelPreprocessor.preprocess per cloud + collate_batch
 * (sp_voxel_preprocessor.py:62-147), MeanVFE.forward (mean_vfe.py:26-30), mask_points_by_range / mask_ego_points (pcd_utils.py:41-88); the contract above.
 *   points [P_cap, 4] float32 (the frame's clouds concatenated); offsets: DEVICE int32 [n_clouds + 1]; voxel_size [3], lidar_range [6], filter_range [6]: HOST float64;
 *   the index grid (n_clouds, D, H, W): H, W = the voxel grid's y, x counts, D >= its z count (VoxelBackBone8x.sparse_shape has D = gz + 1);
 *   features [capacity, 4] float32, indices [capacity, 4] int32 = (cloud, z, y, x), count [1], cloud_counts [n_clouds + 1], status [1]: device.
 *   Launches: clear, mark, three of the prefix count, first point, max_points - 1 selection rounds, two of the max_voxels cut, three of a prefix recount that exit at
 *   once unless a cell was cut, emit.
 *   Refusals, before any HIP call: P_cap < 1 or > COALIGN_SP3D_VOXELIZE_MAX_P_CAP, capacity < 1 (an empty call is REFUSED, not answered with a zero count), n_clouds
 *   < 1, max_voxels < 1, max_points < 1, a grid axis that rounds to 0 or to 65536 and more, H / W different from the voxel grid's, D below its z count,
 *   n_clouds D H W >= 2^31: COALIGN_ERR_BAD_SHAPE; n_clouds > COALIGN_SP3D_VOXELIZE_MAX_CLOUDS, max_points > COALIGN_SP3D_VOXELIZE_MAX_POINTS, an unknown flag:
 *   COALIGN_ERR_UNSUPPORTED; index_bytes below coalign_sp3d_index_workspace_bytes(n_clouds, D, H, W, capacity) or workspace_bytes below (20a): COALIGN_ERR_WORKSPACE;
 *   a NULL pointer (filter_range only with COALIGN_VOX_FILTER_RANGE), points / features / indices / index / workspace not aligned to 16 bytes, the others to 4:
 *   COALIGN_ERR_NULL_POINTER. */
int coalign_sp3d_voxelize(const float *points, const int *offsets, int P_cap, int n_clouds, const double *voxel_size, const double *lidar_range, int D, int H, int W,
                          int max_points, int max_voxels, int flags, const double *filter_range, float *features, int *indices, int *count, int *cloud_counts,
                          int capacity, void *index, size_t index_bytes, unsigned *status, void *workspace, size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif

#endif
