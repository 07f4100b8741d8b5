/* Extension header of ABI version 2, the tenth (include/coalign_amd.h keeps its 68 entry points, the nine earlier extension headers their 2 / 4 / 1 / 3 / 2 / 3 /
 * 3 / 3 / 3): the glue of the pose-robust V2VNet (opencood/models/point_pillar_v2vnet_robust.py, opencood/models/sub_modules/v2v_robust_module.py,
 * opencood/models/fuse_modules/v2v_fuse.py) between its 3 x 3 convolutions, which run on coalign_conv3x3_sp / coalign_conv3x3_sp_s2, and the warp, which is
 * coalign_v2v_warp_split.  Part of the product library libcoalign_hip.so; the conventions of include/coalign_amd_v2v.h: status codes, every shape / pointer
 * check before any HIP call, everything on the caller's stream, no allocation, no host synchronisation (safe inside a captured graph), fixed summation orders,
 * no atomics except the range word.
 *
 * Common: float32 maps are channels-last ([.., H, W, C]) and 16-byte aligned; SplitMaps are the maps of include/coalign_amd.h (9e), 16-byte aligned; float64
 * arrays are 8-byte aligned.  n agents (1 <= n <= 8; n > 8 COALIGN_ERR_UNSUPPORTED), L = max_cav slots per matrix side (n <= L <= 16; L > 16 UNSUPPORTED,
 * L < n BAD_SHAPE); pair (i, j) -- receiver i, sender j -- is map i * n + j and entry [i][j] of an [L, L, ..] array.  A map array of 2^31 values or more is
 * COALIGN_ERR_BAD_SHAPE.  range_flag may be NULL; bit 0 is ORed in when a value written to a SplitMap exceeds the pair's range (|v| > 65504). */
#ifndef COALIGN_AMD_V2V_ROBUST_H
#define COALIGN_AMD_V2V_ROBUST_H

#include "coalign_amd.h"
#include "coalign_amd_v2v.h"

#ifdef __cplusplus
extern "C" {
#endif

/* (14a) Bias term, MaxPool 2 and LeakyReLU behind a convolution of the two small nets (PoseRegression.model and Attention.model, v2v_robust_module.py:33-47 and
 * 331-337: Conv2d, LeakyReLU(0.01), MaxPool2d(2)):  out = lrelu(max over each 2 x 2 block of (a_p + e_{p / n})), floor cropping (Ho = H / 2, Wo = W / 2), the
 * window scanned row by row keeping the first of equal values, as max_pool2d does; lrelu(v) = v > 0 ? v : 0.01 v.  LeakyReLU is monotone, so this is the
 * reference's lrelu-then-pool bit for bit.
 *   a [P, H, W, C]: convolution output; e [P / n, H, W, C]: the ego half of a first convolution (carrying the bias), or NULL (then n is ignored);
 *   out: the SplitMap [P, C, Ho, Wo] (COALIGN_V2V_OUT_SP) or float32 [P, Ho, Wo, C] (COALIGN_V2V_OUT_NHWC).
 *   C % 16 == 0; H < 2 or W < 2, P < 0, e with P % n != 0: BAD_SHAPE; P = 0: OK without a launch.  Memory-bound: one pass, streaming stores. */
int coalign_v2vr_pool_act(const float *a, const float *e, int P, int n, int C, int H, int W, int out_kind, void *out, int32_t *range_flag, void *stream);

/* (14b) The tail of Attention.model and the weights of AttentionWrapper.forward (v2v_robust_module.py:337-341 and 397-405): per pair map
 *   s_ij = sigmoid(b + sum_c w_c * lrelu(max over rows < 2 (H / 2), columns < 2 (W / 2) of y[i n + j, :, :, c]))        (MaxPool 2 then the global max),
 *   scores [L, L] = s inside n x n, 0 outside;  weight[i][j] = scores[i][j] / ((sum_j scores[i][j], in order of j over all L entries) + alpha + 1e-4).
 *   y [n * n, H, W, h]: the second convolution's output, bias included; w [h], b [1], alpha [1]: float32 on the device (alpha is read, not passed by value,
 *   so that a learnable alpha needs no host copy); scores, weight: float32 [L, L].  h % 64 == 0, h <= 1024 (else UNSUPPORTED); H < 2 or W < 2 BAD_SHAPE.
 *   Two launches: one workgroup per pair, then one for the rows. */
int coalign_v2vr_score_head(const float *y, int n, int L, int h, int H, int W, const float *w, const float *b, const float *alpha, float *scores, float *weight,
                            void *stream);

/* (14c) Workspace of (14d), the tail of PoseRegression.model (v2v_robust_module.py:46-54): the pooled means and the two hidden layers of every pair, float32. */
size_t coalign_v2vr_pose_head_workspace_bytes(int n, int h);

/* (14d) The tail of PoseRegression.model and the correction of PoseRegressionWraper.forward (v2v_robust_module.py:46-54 and 107-112, pose_to_tfm
 * transformation_utils.py:93-122): per pair, LeakyReLU, MaxPool 2 (floor cropping), the mean over the pooled map, Linear h -> h, LeakyReLU, Linear h -> h,
 * LeakyReLU, Linear h -> 3;  pose_corr [L, L, 3] float32 (dx, dy, dyaw in degrees; zero outside n x n);  T_new [L, L, 4, 4] float64 =
 * pose_to_tfm(pose_corr[i][j]) @ T[i][j] inside n x n, the identity outside.
 *   y4: the SplitMap [n * n, h, H4, W4] the strided fourth convolution (coalign_conv3x3_sp_s2, no activation) wrote; fc1_w [h, h], fc1_b [h], fc2_w [h, h],
 *   fc2_b [h], fc3_w [3, h], fc3_b [3]: float32, row-major as nn.Linear holds them; T [L, L, 4, 4] float64.  h % 64 == 0, h <= 1024; H4 < 2 or W4 < 2 BAD_SHAPE.
 *   One workgroup per frame: every fc row is read once and applied to all n * n pairs. */
int coalign_v2vr_pose_head(const void *y4_sp, int n, int L, int h, int H4, int W4, const float *fc1_w, const float *fc1_b, const float *fc2_w, const float *fc2_b,
                           const float *fc3_w, const float *fc3_b, const double *T, float *pose_corr, double *T_new, void *workspace, size_t workspace_bytes,
                           void *stream);

/* (14e) Pairwise matrices of 3-dof poses (get_pairwise_transformation_torch with dof = 3, transformation_utils.py:365-415, and the normalisation every warp of
 * the model applies, v2v_robust_module.py:94-98 = v2v_fuse.py:83-87): pairwise[i][j] = T_j^-1 T_i of pose_to_tfm(poses) in closed form (identity on the diagonal
 * and outside n x n), affine [L, L, 2, 3] = rows 0, 1 and columns 0, 1, 3 of it with [0][1] * H / W, [1][0] * W / H, [0][2] / den_x * 2, [1][2] / den_y * 2
 * (den_x = downsample_rate * discrete_ratio * W, den_y = .. * H), the operation order of normalize_pairwise_tfm.  poses [n, 3] (x, y, yaw in degrees), all float64. */
int coalign_v2vr_pairwise(const double *poses, int n, int L, int H, int W, double den_x, double den_y, double *pairwise, double *affine, void *stream);

/* (14f) Global consistency: the whole WeightedEM of one frame (v2v_robust_module.py:165-315; tfm_to_xycs_torch / xycs_to_tfm_torch,
 * transformation_utils.py:189-221) in one workgroup, float64.  Ten rounds of WeightedMLE on the INPUT poses -- per agent the 2 (n - 1) samples
 * xycs(tfm(pose_k) @ T_new[i][k]) and xycs(tfm(pose_k) @ inv(T_new[k][i])), the lower median as the start, 15 Student-t reweighting steps with a 4 x 4 Sigma --
 * each followed by update_weight (log_t with df = 2, k = 120, the constant intersection 0.01 that get_intersection returns for every pose);
 * poses_out [n, 3] = (mu_x, mu_y, atan2(mu_sin, mu_cos) in degrees); pairwise and affine of poses_out as (14e).  n = 1 copies the pose through.
 *   poses [n, 3], T_new [L, L, 4, 4] (planar rigid matrices, as (14d) writes them), all float64. */
int coalign_v2vr_consistency(const double *poses, const double *T_new, int n, int L, int H, int W, double den_x, double den_y, double *poses_out, double *pairwise,
                             double *affine, void *stream);

/* (14g) coalign_v2v_aggregate (12b) with the weighted sum of v2v_fuse.py:140-141:  m_ij = (a_ij + e_i) * mask_ij;  agg_i = m_i0 * weight[i][0] + m_i1 * weight[i][1]
 * + ..., every product and every sum rounded, in order of j;  weight: float32 on the device, row i at weight + i * L.  Both output kinds and every other argument
 * as (12b). */
int coalign_v2vr_aggregate(const float *a, const float *e, const float *x, int n, int R, int C, int H, int W, const double *theta, const float *weight, int L,
                           int out_kind, void *out, int32_t *range_flag, void *stream);

#ifdef __cplusplus
}
#endif

#endif
