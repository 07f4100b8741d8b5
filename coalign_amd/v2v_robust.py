"""The pose-robust V2VNet's three parts around the fusion (opencood/models/sub_modules/v2v_robust_module.py): pose regression on pairs of maps, a globally
consistent pose estimate (a weighted EM over the regressed pairwise transforms), attention scores that weight V2VNet's aggregation.

Classes with the reference's constructor arguments and ``state_dict`` names: ``PoseRegression``, ``PoseRegressionWraper`` (sic), ``Attention``,
``AttentionWrapper``; free functions in the reference's dtypes: ``get_intersection``, ``weighted_mle``, ``weighted_em``, ``update_weight``, ``log_t``,
``pose_to_tfm``, ``tfm_to_xycs``, ``xycs_to_tfm``.  With float32 maps every buffer has the dtype the reference gives it; with float64 maps (the identity tests) the
buffers the reference creates with ``torch.eye`` / ``torch.zeros`` follow the maps instead of truncating them.

Each wrapper has three routes.  ``forward`` (= ``forward_torch``) states the reference op by op.  ``forward_reduced`` applies the exact identities
  (a) the first convolution is linear in [warp | ego]: the ego half is computed once per receiver and carries the bias, the warped half runs over all n^2 maps;
  (b) LeakyReLU is monotone: lrelu(maxpool(v)) = maxpool(lrelu(v)) bit for bit; MaxPool 2 followed by the global max is the max over rows < 2 floor(H / 2) and
      columns < 2 floor(W / 2); MaxPool 2 followed by the global mean is the mean of the pooled floor-cropped map;
  (d) ``get_intersection`` warps a map of ZEROS: the intersection is 0.01 for every pose (``constant_intersection``)
in torch ops.  ``forward_kernels`` runs that schedule on the gfx950 kernels: ``ops.v2v_warp_split`` (one warp serves the attention's first convolution and
iteration 0 of the fusion: identity (c)), ``ops.conv3x3_sp`` / ``conv3x3_sp_s2``, ``ops.v2vr_pool_act`` / ``v2vr_score_head`` / ``v2vr_pose_head``, and
``ops.v2vr_consistency`` for the whole EM.

Quirks of the reference, kept: both wrappers warp to (robust.H, robust.W) but normalise the translation by the map's own H, W (the model refuses maps of another
size, so nothing depends on it); ``weighted_mle`` is called with the INPUT poses in every one of the ten rounds, only the weights change; the intersection is the
constant above.
"""
from __future__ import annotations

import math
from typing import Optional, Sequence

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import ops
from . import backbone as _bb
from .backbone import Conv3x3Pack, _cache_of
from .encoder import host_ints
from .pose import pose_to_tfm  # noqa: F401  (re-exported: the reference keeps it beside tfm_to_xycs_torch)

SLOPE = 0.01
MIN_MAP = 24          # the smallest H and W PoseRegression's pooling accepts (23 x 24 and 24 x 23 fail in PyTorch, 24 x 24 runs); Attention needs 4 x 4


def regroup(x: torch.Tensor, record_len):
    return torch.split(x, host_ints(record_len), dim=0)


def _warp(src: torch.Tensor, M: torch.Tensor, dsize) -> torch.Tensor:
    """warp_affine_simple (torch_transformation_utils.py:322-331)."""
    B, C = src.shape[:2]
    grid = F.affine_grid(M, [B, C, dsize[0], dsize[1]], align_corners=False).to(src)
    return F.grid_sample(src, grid, align_corners=False)


def normalize_tfm(t: torch.Tensor, Hr, Wr, H: int, W: int, downsample_rate, discrete_ratio) -> torch.Tensor:
    """[.., 4, 4] -> [.., 2, 3], the wrappers' normalisation (v2v_robust_module.py:94-98): the rotation terms by (Hr, Wr), the translation by the map's (H, W)."""
    t = t[..., [0, 1], :][..., [0, 1, 3]]
    t[..., 0, 1] = t[..., 0, 1] * Hr / Wr
    t[..., 1, 0] = t[..., 1, 0] * Wr / Hr
    t[..., 0, 2] = t[..., 0, 2] / (downsample_rate * discrete_ratio * W) * 2
    t[..., 1, 2] = t[..., 1, 2] / (downsample_rate * discrete_ratio * H) * 2
    return t


def tfm_to_xycs(tfm: torch.Tensor) -> torch.Tensor:
    """[N, 4, 4] -> [N, 4]: x, y, cos(yaw), sin(yaw) (tfm_to_xycs_torch, transformation_utils.py:189-202)."""
    return torch.stack([tfm[:, 0, 3], tfm[:, 1, 3], tfm[:, 0, 0], tfm[:, 1, 0]]).T


def xycs_to_tfm(xycs: torch.Tensor) -> torch.Tensor:
    """[N, 4] -> [N, 4, 4] (xycs_to_tfm_torch, transformation_utils.py:204-221)."""
    N = xycs.shape[0]
    tfm = torch.eye(4, device=xycs.device, dtype=xycs.dtype).view(1, 4, 4).repeat(N, 1, 1)
    x, y, cos, sin = xycs[:, 0], xycs[:, 1], xycs[:, 2], xycs[:, 3]
    tfm[:, 0, 0] = cos
    tfm[:, 0, 1] = -sin
    tfm[:, 1, 0] = sin
    tfm[:, 1, 1] = cos
    tfm[:, 0, 3] = x
    tfm[:, 1, 3] = y
    return tfm


# what ``routes.plan`` prints for the pose-robust model's fusion (``detector.PointPillarV2VNetRobust.plan_fusion``)
KERNELS = ("v2vr_pairwise + v2v_warp_split + [conv3x3_sp + v2vr_pool_act] x 3 + conv3x3_sp_s2 + v2vr_pose_head (pose regression over all pairs) + v2vr_consistency (the whole "
           "weighted EM in one launch) + v2v_warp_split + conv3x3_sp + v2vr_pool_act + conv3x3_sp + v2vr_score_head (attention; its warp also serves the fusion's first "
           "iteration) + V2VNet's message passing with v2vr_aggregate (weighted sum over the senders)")
TORCH = "PointPillarV2VNetRobust op by op in PyTorch"


# ---- part 1: pose regression ---------------------------------------------------------------------------------------------------------------------------------
class PoseRegression(nn.Module):
    """[N, 2C, H, W] -> [N, 3] (dx, dy, dyaw) (v2v_robust_module.py:19-60)."""

    def __init__(self, in_ch: int = 512, hidden_ch: int = 256):
        super().__init__()
        self.model = nn.Sequential(
            nn.Conv2d(in_ch, hidden_ch, kernel_size=(3, 3), padding=1), nn.LeakyReLU(negative_slope=SLOPE), nn.MaxPool2d(kernel_size=2, stride=2, padding=0),
            nn.Conv2d(hidden_ch, hidden_ch, kernel_size=(3, 3), padding=1), nn.LeakyReLU(negative_slope=SLOPE), nn.MaxPool2d(kernel_size=2, stride=2, padding=0),
            nn.Conv2d(hidden_ch, hidden_ch, kernel_size=(3, 3), padding=1), nn.LeakyReLU(negative_slope=SLOPE), nn.MaxPool2d(kernel_size=2, stride=2),
            nn.Conv2d(hidden_ch, hidden_ch, kernel_size=(3, 3), stride=(2, 2), padding=1), nn.LeakyReLU(negative_slope=SLOPE), nn.MaxPool2d(kernel_size=2, stride=2),
            nn.AdaptiveAvgPool2d(output_size=1), nn.Flatten(),
            nn.Linear(in_features=hidden_ch, out_features=hidden_ch, bias=True), nn.LeakyReLU(negative_slope=SLOPE),
            nn.Linear(in_features=hidden_ch, out_features=hidden_ch, bias=True), nn.LeakyReLU(negative_slope=SLOPE),
            nn.Linear(in_features=hidden_ch, out_features=3, bias=True))

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return self.model(x)


class _PairNet(nn.Module):
    """What the two wrappers share: the affine parameters, the route switch, the split of the first convolution."""

    def _init_affine(self, affine_parameter: dict) -> None:
        self.H, self.W = affine_parameter["H"], affine_parameter["W"]
        self.downsample_rate, self.discrete_ratio = affine_parameter["downsample_rate"], affine_parameter["discrete_ratio"]
        self.force_torch = False      # measurement / test aid: take the op-by-op route whatever the device

    def _net(self) -> nn.Sequential:
        raise NotImplementedError

    def _first_split(self):
        """(warped-map columns [h, C, 3, 3], ego columns, bias) of the first convolution: identity (a)."""
        conv = self._net()[0]
        C = conv.in_channels // 2
        return conv.weight[:, :C].contiguous(), conv.weight[:, C:].contiguous(), conv.bias

    def widths_reason(self, channels: int) -> Optional[str]:
        """None when C and hidden are multiples of 64 within ``conv3x3_sp``'s and the heads' limits, else the words of the pose-robust model's plan."""
        conv = self._net()[0]
        hidden = conv.out_channels
        if (conv.in_channels == 2 * channels and channels % 64 == 0 and hidden % 64 == 0 and _bb.sp_channels_ok(channels, hidden) and _bb.sp_channels_ok(hidden, hidden)
                and ops.v2vr_shape_ok(channels, hidden, 1)):
            return None
        return f"{channels} channels or hidden {hidden} outside C % 64 == 0"

    def kernel_shape_reason(self, channels: int, n_agents: int = 1, terms: Optional[int] = None, max_cav: int = 5) -> Optional[str]:
        """None when the kernels take (channels, n_agents) in the arithmetic in force, else why not, in words."""
        why = self.widths_reason(channels)
        if why is None and not ops.v2vr_shape_ok(channels, self._net()[0].out_channels, n_agents, max(max_cav, n_agents)):
            why = f"{n_agents} agents in a frame outside 1 .. 8, or more than {ops.V2VR_MAX_CAV} slots"
        return why if why is not None or _bb.split_maps_active(terms) else "the SplitMap arithmetic (fp16 x 2) is not in force"

    def kernel_route(self, channels: int, n_agents: int = 1, terms: Optional[int] = None, max_cav: int = 5) -> bool:
        """The static half of the decision: eval mode, C and hidden multiples of 64 within ``conv3x3_sp``'s limits, at most 8 agents, SplitMap arithmetic in force."""
        return bool(not self.training and not self.force_torch and self.kernel_shape_reason(channels, n_agents, terms, max_cav) is None)

    def plan_layer(self, name: str, layer: nn.Module, terms: Optional[int], ok: bool):
        """-> (``routes.plan``'s line, fallback) of one convolution or linear of the net, given the model's ONE decision for its three parts."""
        if isinstance(layer, nn.Linear):
            return (self.HEAD if ok else _bb.LINEAR_LIBRARY + ", PointPillarV2VNetRobust op by op)"), not ok
        first = " (the warped-map and the ego columns as two C -> hidden convolutions over all pairs; bias, pooling and LeakyReLU in v2vr_pool_act)" if name.endswith("model.0") else ""
        kernel = _bb.SP_S2 + " (LeakyReLU, pooling and the mean in v2vr_pose_head)" if layer.stride[0] == 2 else _bb.SP + first
        return (kernel if ok else _bb.MIOPEN + " (PointPillarV2VNetRobust op by op)"), not ok

    def _thetas(self, pairwise_t_matrix_b: torch.Tensor, Hr, Wr, H: int, W: int) -> torch.Tensor:
        return normalize_tfm(pairwise_t_matrix_b, Hr, Wr, H, W, self.downsample_rate, self.discrete_ratio)

    def _first_reduced(self, xb: torch.Tensor, theta: torch.Tensor) -> torch.Tensor:
        """The first convolution + LeakyReLU + MaxPool 2 over all n^2 pairs by identities (a) and (b): [n n, h, H / 2, W / 2]."""
        n, C, H, W = xb.shape
        wn, we, b = self._first_split()
        e = F.conv2d(xb, we, b, padding=1)                                                                      # the ego term, once per receiver
        warped = torch.cat([_warp(xb, theta[i, :n], (self.H, self.W)) for i in range(n)], dim=0)              # [n n, C, H, W]
        a = F.conv2d(warped, wn, None, padding=1).view(n, n, -1, H, W)
        return F.leaky_relu(F.max_pool2d((a + e.unsqueeze(1)).flatten(0, 1), 2), SLOPE)


class PoseRegressionWraper(_PairNet):
    """features [sum(cav), C, H, W], record_len, pairwise_t_matrix [B, L, L, 4, 4] -> (pose_corr_matrix [B, L, L, 3], pairwise_t_matrix_new [B, L, L, 4, 4]):
    every receiver i and sender j, the diagonal included (v2v_robust_module.py:64-114)."""

    HEAD = "v2vr_pose_head (all pairs in one workgroup, every row read once, fp32)"

    def __init__(self, in_ch: int, hidden_ch: int, affine_parameter: dict):
        super().__init__()
        self.pose_regression = PoseRegression(in_ch=in_ch, hidden_ch=hidden_ch)
        self._init_affine(affine_parameter)

    def _net(self):
        return self.pose_regression.model

    def _outputs(self, features: torch.Tensor, pairwise_t_matrix: torch.Tensor):
        B, L = pairwise_t_matrix.shape[:2]
        dev = pairwise_t_matrix.device
        return (torch.zeros((B, L, L, 3), device=dev, dtype=features.dtype), torch.eye(4, device=dev, dtype=features.dtype).view(1, 1, 1, 4, 4).repeat(B, L, L, 1, 1))

    def forward_torch(self, features: torch.Tensor, record_len, pairwise_t_matrix: torch.Tensor):
        _, C, H, W = features.shape
        groups = host_ints(record_len)
        pose_corr_matrix, pairwise_t_matrix_new = self._outputs(features, pairwise_t_matrix)
        for b, agent_features in enumerate(regroup(features, groups)):
            N = groups[b]
            for i in range(N):
                t_matrix = self._thetas(pairwise_t_matrix[b], H, W, H, W)
                neighbors = _warp(agent_features, t_matrix[i, :N], (self.H, self.W))
                ego_agent_feature = agent_features[i].unsqueeze(0).repeat(N, 1, 1, 1)
                pose_corr = self.pose_regression(torch.cat([neighbors, ego_agent_feature], dim=1))
                pose_corr_matrix[b, i, :N] = pose_corr
                pairwise_t_matrix_new[b, i, :N] = pose_to_tfm(pose_corr) @ pairwise_t_matrix[b, i, :N].to(pose_corr)
        return pose_corr_matrix, pairwise_t_matrix_new

    forward = forward_torch

    def forward_reduced(self, features: torch.Tensor, record_len, pairwise_t_matrix: torch.Tensor):
        _, C, H, W = features.shape
        groups = host_ints(record_len)
        m = self._net()
        pose_corr_matrix, pairwise_t_matrix_new = self._outputs(features, pairwise_t_matrix)
        for b, xb in enumerate(regroup(features, groups)):
            N = groups[b]
            y = self._first_reduced(xb, self._thetas(pairwise_t_matrix[b], H, W, H, W))
            for k in (3, 6):
                y = F.leaky_relu(F.max_pool2d(m[k](y), 2), SLOPE)                                                # (b): pool first, one LeakyReLU on a quarter of the values
            y = F.leaky_relu(F.max_pool2d(m[9](y), 2), SLOPE).mean(dim=(2, 3))                                   # (b): the mean of the pooled floor-cropped map
            pose_corr = m[18](F.leaky_relu(m[16](F.leaky_relu(m[14](y), SLOPE)), SLOPE)).view(N, N, 3)
            pose_corr_matrix[b, :N, :N] = pose_corr
            pairwise_t_matrix_new[b, :N, :N] = (pose_to_tfm(pose_corr.reshape(N * N, 3)) @ pairwise_t_matrix[b, :N, :N].reshape(N * N, 4, 4).to(pose_corr)).view(N, N, 4, 4)
        return pose_corr_matrix, pairwise_t_matrix_new

    def packed(self):
        """The kernel route's weight images, cached until a parameter changes: (warped-map image, ego image, bias 1, zero bias, [(image, bias) of convolutions 2 .. 4],
        (W1, b1, W2, b2, W3, b3) of the linears)."""
        def build():
            m = self._net()
            wn, we, b = self._first_split()
            f32 = lambda t: t.detach().float().contiguous()      # noqa: E731
            return (Conv3x3Pack(wn).emu(16, True), Conv3x3Pack(we).emu(16, True), f32(b), torch.zeros_like(b, dtype=torch.float32),
                    [(Conv3x3Pack(m[k].weight).emu(16, True), f32(m[k].bias)) for k in (3, 6, 9)], tuple(f32(t) for k in (14, 16, 18) for t in (m[k].weight, m[k].bias)))
        return _cache_of(self, "_coalign_v2vr_images").get(self, build)

    def forward_kernels(self, xb: torch.Tensor, warped: "ops.SplitMap", T: torch.Tensor):
        """One frame: xb [n, C, H, W] float32 channels-last, ``warped`` = ``ops.v2v_warp_split(xb, theta)`` of the noisy poses, T [L, L, 4, 4] float64 ->
        (pose_corr [L, L, 3] float32, T_new [L, L, 4, 4] float64)."""
        img_n, img_e, b1, zero, convs, fc = self.packed()
        n, h = xb.shape[0], b1.numel()
        e = ops.conv3x3_sp(ops.SplitMap.pack(xb), img_e, b1, h, None, False, out_split=False)
        a = ops.conv3x3_sp(warped, img_n, zero, h, None, False, out_split=False)
        y = ops.v2vr_pool_act(a, e, n)
        for img, bias in convs[:2]:
            y = ops.v2vr_pool_act(ops.conv3x3_sp(y, img, bias, h, None, False, out_split=False))
        y4 = ops.conv3x3_sp_s2(y, convs[2][0], convs[2][1], h, relu=False)
        return ops.v2vr_pose_head(y4, n, T.shape[0], fc, T)


# ---- part 2: global consistency ------------------------------------------------------------------------------------------------------------------------------
def get_intersection(pairwise_t_matrix: torch.Tensor, affine_parameter: dict) -> torch.Tensor:
    """[L, L, 4, 4] -> [L, L] (v2v_robust_module.py:119-160), op by op.  The reference warps a tensor of ZEROS, so the result is 0.01 everywhere whatever the
    poses: ``constant_intersection`` is the same tensor without a warp."""
    H, W = affine_parameter["H"], affine_parameter["W"]
    L = pairwise_t_matrix.shape[0]
    one_tensor = torch.zeros((L, 1, H, W), device=pairwise_t_matrix.device, dtype=pairwise_t_matrix.dtype)
    intersections = []
    for i in range(L):
        t_matrix = normalize_tfm(pairwise_t_matrix, H, W, H, W, affine_parameter["downsample_rate"], affine_parameter["discrete_ratio"])
        neighbors = _warp(one_tensor, t_matrix[i, :L], (H, W))
        intersections.append(torch.sum(neighbors, dim=[1, 2, 3]) / (H * W))
    intersections = torch.stack(intersections)
    intersections += 0.01
    return intersections


def constant_intersection(pairwise_t_matrix: torch.Tensor) -> torch.Tensor:
    L = pairwise_t_matrix.shape[0]
    return torch.full((L, L), 0.01, device=pairwise_t_matrix.device, dtype=pairwise_t_matrix.dtype)


def weighted_mle(pose: torch.Tensor, pairwise_t_matrix: torch.Tensor, weight: torch.Tensor):
    """Weighted MLE of the mean and the scatter of a multivariate Student-t per agent (WeightedMLE, v2v_robust_module.py:165-224): pose [N, 3],
    pairwise_t_matrix [L, L, 4, 4], weight [L, L] -> (pose_mu [N, 4] as x, y, cos, sin; pose_sigma [N, 4, 4]) in the matrices' dtype, the 15 steps in float64."""
    N = pose.shape[0]
    out = pairwise_t_matrix.dtype
    mu_list, sigma_list = [], []
    for i in range(N):
        neighbor_ids = [k for k in range(N) if k != i]
        weights = weight[i, neighbor_ids].repeat(2)
        relative_pose = torch.cat([pairwise_t_matrix[i, neighbor_ids], torch.inverse(pairwise_t_matrix[neighbor_ids, i])], dim=0)
        tfm = pose_to_tfm(pose[neighbor_ids]).repeat(2, 1, 1)
        samples = tfm_to_xycs(tfm.to(relative_pose) @ relative_pose).to(torch.float64)
        mu = samples.median(0).values
        Sigma = torch.eye(4, device=pose.device, dtype=torch.float64)
        small_identity = torch.eye(4, device=pose.device, dtype=torch.float64) * 0.05
        diff = mu[None] - samples
        v = 2
        for _ in range(15):
            eta = (v + mu.size(0)) / (v + torch.einsum("ni,ij,nj->n", diff, Sigma.inverse(), diff))
            mu = torch.einsum("n,n,ni->i", weights.to(torch.float64), eta, samples) / (weights * eta).sum()
            diff = mu[None] - samples
            Sigma = torch.einsum("n,ni,nj->ij", eta, diff, diff) / diff.size(0) + small_identity
        mu_list.append(mu.to(out))
        sigma_list.append(Sigma.to(out))
    return torch.stack(mu_list), torch.stack(sigma_list)


def log_t(x: torch.Tensor, mu: torch.Tensor, Sigma: torch.Tensor, df) -> torch.Tensor:
    """log pdf of the multivariate t distribution (v2v_robust_module.py:282-315): x [n, p], mu [p], Sigma [p, p]."""
    assert len(x.shape) == 2
    n, p = x.shape
    assert Sigma.shape == (p, p)
    v = torch.as_tensor(df, dtype=x.dtype, device=x.device)
    p = torch.as_tensor(p, dtype=x.dtype, device=x.device)
    pi = torch.tensor(math.pi, dtype=x.dtype, device=x.device)
    half_v, half_p = v / 2.0, p / 2.0
    log_num = (half_v + half_p).lgamma()
    log_denom = half_v.lgamma() + half_p * (v.log() + pi.log()) + 0.5 * Sigma.logdet()
    d = x - mu
    log_val = -(half_p + half_v) * torch.log(1 + torch.einsum("ni,ij,nj->n", d, Sigma.inverse(), d) / v)
    return log_num - log_denom + log_val


def update_weight(pose_mu: torch.Tensor, pose_sigma: torch.Tensor, pairwise_t_matrix: torch.Tensor, intersection: torch.Tensor) -> torch.Tensor:
    """The closed-form weight update (v2v_robust_module.py:256-278): k = 120, df = 2."""
    k, df = 120, 2
    N = pose_mu.shape[0]
    weight = torch.zeros_like(intersection)
    for i in range(N):
        for j in range(N):
            if i != j:
                pose_estimate1 = xycs_to_tfm(pose_mu[[j]])[0] @ pairwise_t_matrix[i, j]
                pose_estimate2 = xycs_to_tfm(pose_mu[[i]])[0] @ torch.inverse(pairwise_t_matrix[i, j])
                pose_estimate = tfm_to_xycs(torch.stack([pose_estimate1, pose_estimate2]))
                weight[i, j] = k * intersection[i, j] / (k - log_t(pose_estimate, pose_mu[i], pose_sigma[i], df).sum())
    return weight


def weighted_em(lidar_pose: torch.Tensor, pairwise_t_matrix: torch.Tensor, intersection: torch.Tensor) -> torch.Tensor:
    """WeightedEM of one frame (v2v_robust_module.py:227-254): lidar_pose [N, 3], pairwise_t_matrix [L, L, 4, 4], intersection [L, L] -> the new poses [N, 3].
    ``weighted_mle`` sees the INPUT poses in every round (the reference never feeds its estimate back); only the weights change."""
    pose = lidar_pose
    weight = torch.ones_like(intersection)
    for _ in range(10):
        pose_mu, pose_sigma = weighted_mle(pose, pairwise_t_matrix, weight)
        weight = update_weight(pose_mu, pose_sigma, pairwise_t_matrix, intersection)
    pose_new = torch.zeros((lidar_pose.shape[0], 3), device=lidar_pose.device, dtype=lidar_pose.dtype)
    pose_new[:, :2] = pose_mu[:, :2]
    pose_new[:, 2] = torch.rad2deg(torch.atan2(pose_mu[:, 3], pose_mu[:, 2]))
    return pose_new


# ---- part 3: attention ---------------------------------------------------------------------------------------------------------------------------------------
class Attention(nn.Module):
    """[N, 2C, H, W] -> [N, 1] in (0, 1) (v2v_robust_module.py:320-346)."""

    def __init__(self, in_ch: int, hidden_ch: int = 160):
        super().__init__()
        self.model = nn.Sequential(
            nn.Conv2d(in_ch, hidden_ch, 3, 1, 1), nn.LeakyReLU(negative_slope=SLOPE), nn.MaxPool2d(kernel_size=2, stride=2),
            nn.Conv2d(hidden_ch, hidden_ch, 3, 1, 1), nn.LeakyReLU(negative_slope=SLOPE), nn.MaxPool2d(kernel_size=2, stride=2),
            nn.AdaptiveMaxPool2d(output_size=1), nn.Flatten(), nn.Linear(in_features=hidden_ch, out_features=1, bias=True), nn.Sigmoid())

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return self.model(x)


class AttentionWrapper(_PairNet):
    """features, record_len, pairwise_t_matrix [B, L, L, 4, 4] -> (scores [B, L, L], weight [B, L, L]): scores[b, i, j] rates sender j in receiver i's frame,
    weight = score / (sum_j score + alpha + 1e-4) (v2v_robust_module.py:348-407).  ``alpha``: a learnable [1] parameter (0.15) or the constant 0.35."""

    HEAD = "v2vr_score_head (cropped global max, linear, sigmoid and the weights, fp32)"

    def __init__(self, in_ch: int, hidden_ch: int, affine_parameter: dict, learnable_alpha: bool = True):
        super().__init__()
        self.attention_net = Attention(in_ch, hidden_ch)
        self._init_affine(affine_parameter)
        if learnable_alpha:
            self.alpha = nn.Parameter(torch.Tensor([0.15]))
        else:
            self.alpha = 0.35

    def _net(self):
        return self.attention_net.model

    def _weights(self, pairwise_score: torch.Tensor) -> torch.Tensor:
        return pairwise_score / (torch.sum(pairwise_score, dim=2, keepdim=True) + self.alpha + 1e-4)

    def forward_torch(self, features: torch.Tensor, record_len, pairwise_t_matrix: torch.Tensor):
        _, C, H, W = features.shape
        B, L = pairwise_t_matrix.shape[:2]
        groups = host_ints(record_len)
        pairwise_score = torch.zeros((B, L, L), device=features.device, dtype=features.dtype)
        for b, agent_features in enumerate(regroup(features, groups)):
            N = groups[b]
            for i in range(N):
                t_matrix = self._thetas(pairwise_t_matrix[b], self.H, self.W, H, W)
                neighbors = _warp(agent_features, t_matrix[i, :N], (self.H, self.W))
                ego_agent_feature = agent_features[i].unsqueeze(0).repeat(N, 1, 1, 1)
                pairwise_score[b, i, :N] = self.attention_net(torch.cat([neighbors, ego_agent_feature], dim=1)).flatten()
        return pairwise_score, self._weights(pairwise_score)

    forward = forward_torch

    def forward_reduced(self, features: torch.Tensor, record_len, pairwise_t_matrix: torch.Tensor):
        _, C, H, W = features.shape
        B, L = pairwise_t_matrix.shape[:2]
        groups = host_ints(record_len)
        m = self._net()
        pairwise_score = torch.zeros((B, L, L), device=features.device, dtype=features.dtype)
        for b, xb in enumerate(regroup(features, groups)):
            N = groups[b]
            y = m[3](self._first_reduced(xb, self._thetas(pairwise_t_matrix[b], self.H, self.W, H, W)))
            Hc, Wc = y.shape[2] // 2 * 2, y.shape[3] // 2 * 2
            z = F.leaky_relu(y[:, :, :Hc, :Wc].amax(dim=(2, 3)), SLOPE)                                      # (b): MaxPool 2 + global max = the max over the cropped map
            pairwise_score[b, :N, :N] = torch.sigmoid(m[8](z)).view(N, N)
        return pairwise_score, self._weights(pairwise_score)

    def packed(self):
        """(warped-map image, ego image, bias 1, zero bias, second convolution's image, its bias, linear weight [h], linear bias [1], alpha [1])."""
        def build():
            m = self._net()
            wn, we, b = self._first_split()
            f32 = lambda t: t.detach().float().contiguous()      # noqa: E731
            alpha = f32(self.alpha) if torch.is_tensor(self.alpha) else torch.full((1,), float(self.alpha), dtype=torch.float32, device=b.device)
            return (Conv3x3Pack(wn).emu(16, True), Conv3x3Pack(we).emu(16, True), f32(b), torch.zeros_like(b, dtype=torch.float32), Conv3x3Pack(m[3].weight).emu(16, True),
                    f32(m[3].bias), f32(m[8].weight.reshape(-1)), f32(m[8].bias), alpha)
        return _cache_of(self, "_coalign_v2vr_images").get(self, build)

    def forward_kernels(self, xb: torch.Tensor, warped: "ops.SplitMap", max_cav: int):
        """One frame: xb [n, C, H, W] float32 channels-last, ``warped`` = ``ops.v2v_warp_split(xb, theta)`` -> (scores [L, L], weight [L, L]) float32."""
        img_n, img_e, b1, zero, img2, b2, w, b, alpha = self.packed()
        n, h = xb.shape[0], b1.numel()
        e = ops.conv3x3_sp(ops.SplitMap.pack(xb), img_e, b1, h, None, False, out_split=False)
        a = ops.conv3x3_sp(warped, img_n, zero, h, None, False, out_split=False)
        y = ops.conv3x3_sp(ops.v2vr_pool_act(a, e, n), img2, b2, h, None, False, out_split=False)
        return ops.v2vr_score_head(y, n, max_cav, w, b, alpha)
