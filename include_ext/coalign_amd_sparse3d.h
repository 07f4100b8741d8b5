/* Extension header of ABI version 2, the first one under include_ext/ (include/ keeps its seventeen headers and their counts): the sparse 3-D trunk of the SECOND
 * detectors -- MeanVFE, VoxelBackBone8x (spconv's SubMConv3d / SparseConv3d, restated: spconv is not linked) and HeightCompression.  Part of the product library
 * libcoalign_hip.so; the conventions of include/coalign_amd_lss.h apply (status codes, every shape / pointer / alignment check before any HIP call, everything on
 * the caller's stream, no allocation, safe inside a captured graph; no float atomics: the same input gives the same bits).
 *
 * A SPARSE TENSOR is features [capacity, C] float32 + indices [capacity, 4] int32 = (batch, z, y, x) + a DEVICE count (one int32; rows at or past it are never
 * read) + spatial shape (D, H, W) + batch size N.  Indices are unique.  A row whose coordinates lie outside [0, N) x [0, D) x [0, H) x [0, W) is IGNORED: it is
 * no site, no neighbour and produces no output site; whatever `indices` holds, nothing is read or written outside the buffers.  N D H W >= 2^31 is
 * COALIGN_ERR_BAD_SHAPE everywhere.
 *
 * THE SITE INDEX of a tensor (cell -> row) is a dense bitmap over the linear cell index ((b D + z) H + y) W + x with one prefix count per 32-bit word and a
 * rank -> row table: row(cell) = perm[prefix[cell / 32] + popcount(bits[cell / 32] below cell % 32)].  coalign_sp3d_index_workspace_bytes() is its size:
 * 8 bytes per 32 cells + 4 bytes per 1024 words + 4 bytes per row of capacity, each part rounded up to 256 bytes.
 *
 * A NEIGHBOUR TABLE nbr [taps, cap_out] int32 (tap-major) holds, per output row and tap kappa = (kz kh + ky) kw + kx ... in ascending (kz, ky, kx) order, the
 * input row at o s - p + kappa or -1.  The submanifold layers of one level share one table (spconv's indice_key). */
#ifndef COALIGN_AMD_SPARSE3D_H
#define COALIGN_AMD_SPARSE3D_H

#include "coalign_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define COALIGN_SP3D_STATUS_OVERFLOW 1u /* bit of the status word: a strided layer produced more sites than its output capacity */

/* (18a) out[m][c] = sum over the T slots of voxels[m][t][c] / max(num_points[m], 1): MeanVFE.forward (opencood/models/sub_modules/mean_vfe.py:26-30).
 * voxels [M, T, C] float32, num_points [M] int32, out [M, C] float32.  M < 0, T < 1, C < 1 or M T C >= 2^31: COALIGN_ERR_BAD_SHAPE; a NULL or 4-byte-misaligned
 * pointer with M > 0: COALIGN_ERR_NULL_POINTER.  M = 0 returns COALIGN_OK without a launch. */
int coalign_sp3d_mean_vfe(const float *voxels, const int *num_points, int M, int T, int C, float *out, void *stream);

/* (18b) bytes of the site index of a tensor of `capacity` rows on the grid N x (D, H, W) (layout above); 0 for a shape that (18c) refuses. */
size_t coalign_sp3d_index_workspace_bytes(int N, int D, int H, int W, int capacity);

/* (18c) the site index of (indices, *count) into `index`: what spconv's hash table of ops.get_indice_pairs holds for the SparseConvTensor that
 * VoxelBackBone8x.forward builds (opencood/models/sub_modules/sparse_backbone_3d.py:114-119).  Six launches (clear, mark, three of the prefix count, rank -> row).
 *   N, D, H, W < 1, capacity < 0, N D H W >= 2^31: COALIGN_ERR_BAD_SHAPE; index_bytes below (18b): COALIGN_ERR_WORKSPACE; NULL count / index, NULL indices with
 *   capacity > 0, index / indices not aligned to 16 bytes, count to 4: COALIGN_ERR_NULL_POINTER. */
int coalign_sp3d_index_build(const int *indices, const int *count, int capacity, int N, int D, int H, int W, void *index, size_t index_bytes, void *stream);

/* (18d) the output sites of SparseConv3d(kernel (kd, kh, kw), stride (sd, sh, sw), padding (pd, ph, pw)) -- the layers of sparse_backbone_3d.py:61, :68, :75, :87;
 * spconv's get_indice_pairs for a non-submanifold convolution.  Output site o is active iff an active input i = o s - p + kappa, 0 <= kappa < k, exists with o inside
 * (oD, oH, oW) = (n + 2 p - k) / s + 1 per axis (computed here).  spconv leaves the row order to its hash table; HERE rows ascend in ((b oD + z) oH + y) oW + x.
 * Writes out_indices [cap_out, 4], *out_count = min(sites, cap_out) -- the count stays on the device --, the site index of the output into out_index (rank = row), and
 * sets COALIGN_SP3D_STATUS_OVERFLOW in *status when sites > cap_out (the first cap_out sites in ascending order are kept).  Six launches.
 *   Shapes as (18c), k < 1, s < 1, p < 0, k > 3, an output axis < 1, N oD oH oW >= 2^31, cap_in / cap_out < 0: COALIGN_ERR_BAD_SHAPE; out_index_bytes below (18b) for
 *   the output grid and cap_out: COALIGN_ERR_WORKSPACE; NULL in_count / out_count / out_index / status, NULL in_indices with cap_in > 0, NULL out_indices with cap_out > 0,
 *   indices / index not aligned to 16 bytes, the others to 4: COALIGN_ERR_NULL_POINTER. */
int coalign_sp3d_strided_sites(const int *in_indices, const int *in_count, int cap_in, int N, int D, int H, int W, int kd, int kh, int kw, int sd, int sh, int sw, int pd,
                               int ph, int pw, int *out_indices, int *out_count, int cap_out, void *out_index, size_t out_index_bytes, unsigned *status, void *stream);

/* (18e) the neighbour table of the output rows (out_indices, *out_count) on the grid (oD, oH, oW) against the input tensor indexed by in_index on (D, H, W): the
 * rulebook of spconv's get_indice_pairs, output-stationary.  For SubMConv3d(.., 3) (sparse_backbone_3d.py:49, :56, :62-63, :69-70, :76-77) pass the tensor's own
 * indices and index, k = 3, s = 1, p = 1.  nbr [kd kh kw, cap_out] int32.  One launch.
 *   Shape rules of (18d); NULL out_count / in_index, NULL out_indices / nbr with cap_out > 0, misalignment (indices / index 16, others 4): COALIGN_ERR_NULL_POINTER;
 *   in_index_bytes below (18b) for (N, D, H, W, cap_in): COALIGN_ERR_WORKSPACE. */
int coalign_sp3d_neighbors(const int *out_indices, const int *out_count, int cap_out, int N, int oD, int oH, int oW, const void *in_index, size_t in_index_bytes, int cap_in,
                           int D, int H, int W, int kd, int kh, int kw, int sd, int sh, int sw, int pd, int ph, int pw, int *nbr, void *stream);

/* (18f) bytes of the weight image (18g) reads; 0 for an unsupported combination.  (Cin, Cout, taps) = (4, 16, 27): float32 [taps][Cin][Cout].  Cin >= 16: the A
 * operand of v_mfma_f32_32x32x16_f16 as sp16 pairs, [taps Cin / 16 steps][ceil(Cout / 32) row tiles][64 lanes][8 h | 8 l] fp16, rows past Cout zero, column
 * k = tap Cin + c, every row c DIVIDED by the power of two 2^k_c that brings its largest |w| into [1, 2) (k_c = 0 for a zero row) -- an unscaled pair keeps an absolute
 * 2^-34 of a weight below 2^-14 --, followed by 32 ceil(Cout / 32) float32: 2^k_c per row, which (18g) multiplies the sum by (coalign_amd.ops.pack_sp3d_weights). */
size_t coalign_sp3d_weight_bytes(int Cin, int Cout, int taps);

/* (18g) out[r] = relu(sum over the taps, ascending, of W[tap] in[nbr[tap][r]] + shift) for r < *out_count: SubMConv3d / SparseConv3d + eval BatchNorm1d(eps 1e-3) +
 * ReLU on the active rows (post_act_block, sparse_backbone_3d.py:11-30; conv_input :48-52; conv_out :85-91), the batch norm folded into W and shift by the caller.
 * A missing neighbour (-1, or any value outside [0, cap_in)) is a zero row; a row WITHOUT any neighbour is no site (its coordinates lie outside the grid: (18e) gives it
 * -1 throughout) and is written as zeros.  Output-stationary: 32 output rows x 32 output channels per wavefront, the neighbour rows
 * gathered per tap and split into sp16 pairs in registers, three matrix instructions per fp32 product; (4, 16) on fp32 vector arithmetic.  No atomics.  One launch.
 *   Supported (Cin, Cout) at taps = 27: (4, 16), (16, 16), (16, 32), (32, 32), (32, 64), (64, 64); at taps = 3: (64, 64), (64, 128); anything else
 *   COALIGN_ERR_UNSUPPORTED.  cap_in, cap_out < 0 or cap_out taps >= 2^31: COALIGN_ERR_BAD_SHAPE; weight_bytes below (18f): COALIGN_ERR_WORKSPACE; NULL out_count /
 *   weights / shift, NULL in_feat with cap_in > 0, NULL nbr / out_feat with cap_out > 0, in_feat / out_feat / weights / shift not aligned to 16 bytes, the others to 4:
 *   COALIGN_ERR_NULL_POINTER.  Rows at or past *out_count are not written. */
int coalign_sp3d_conv(const float *in_feat, int cap_in, const int *nbr, int taps, const int *out_count, int cap_out, int Cin, int Cout, const void *weights,
                      size_t weight_bytes, const float *shift, float *out_feat, void *stream);

/* (18h) out[b][y][x][c D + d] = feat[row(b, d, y, x)][c], or 0 where the cell is no site: SparseConvTensor.dense() followed by HeightCompression's view
 * (opencood/models/sub_modules/height_compression.py:20-23).  out is [N, C D, H, W] float32 in CHANNELS-LAST memory; EVERY element is written by the launch: no
 * memset, no dependence on earlier contents.  One wavefront per (b, y, x), lanes across the C D channels.  One launch.
 *   Shapes as (18c), C < 1, capacity < 0, N H W C D >= 2^31: COALIGN_ERR_BAD_SHAPE; index_bytes below (18b): COALIGN_ERR_WORKSPACE; NULL count / index / out, NULL feat
 *   with capacity > 0, feat / index / out not aligned to 16 bytes, count to 4: COALIGN_ERR_NULL_POINTER. */
int coalign_sp3d_to_dense(const float *feat, const int *count, int capacity, int C, const void *index, size_t index_bytes, int N, int D, int H, int W, float *out,
                          void *stream);

#ifdef __cplusplus
}
#endif

#endif
