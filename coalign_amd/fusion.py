"""Multi-agent feature fusion modules (SURVEY §8a rows G, H, H'), host side.

Class / function names and signatures follow opencood/models/fuse_modules/fusion_in_one.py
(``regroup`` :21-24, ``warp_feature`` :26-45, ``MaxFusion`` :47-89, ``AttFusion`` :91-136, ``DiscoFusion`` :138-171) and
opencood/models/sub_modules/torch_transformation_utils.py (``warp_affine_simple`` :322-331).  ``MaxFusion`` / ``AttFusion`` own no
parameters; all their arithmetic is the fused gfx950 kernel ``coalign_warp_fuse``.  ``DiscoFusion`` owns ``PixelWeightLayer``
(opencood/models/fuse_modules/disco_fuse.py:76-99) and runs on ``coalign_disco_fuse``.
"""
from __future__ import annotations

from typing import List, Optional, Sequence

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import ops
from .backbone import _cache_of, fold_bn
from .encoder import host_ints


def regroup(x: torch.Tensor, record_len) -> List[torch.Tensor]:
    """Split the concatenated agent batch into per-frame views."""
    return list(torch.split(x, host_ints(record_len), dim=0))


def _ego_rows(affine: torch.Tensor, groups: Sequence[int]) -> torch.Tensor:
    """normalized_affine_matrix [B, L, L, 2, 3] -> theta [sum N, 2, 3]: row ``[b, 0, :N_b]`` of every frame
    (ego coordinates -> agent j; fusion_in_one.py:125-128)."""
    if affine.shape[0] == 1:
        return affine[0, 0, : groups[0]]
    return torch.cat([affine[b, 0, :n] for b, n in enumerate(groups)], dim=0)


def warp_affine_simple(src: torch.Tensor, M: torch.Tensor, dsize, mode="bilinear", padding_mode="zeros",
                       align_corners=False) -> torch.Tensor:
    """``F.grid_sample(src, F.affine_grid(M, ...).to(src))``, bilinear / zeros / align_corners=False
    (the extra keyword arguments are accepted and ignored exactly like the reference does)."""
    n = src.shape[0]
    return ops.warp_fuse(src, M, [1] * n if n <= 0 else _chunks(n), ops.FUSE_NONE, out_hw=(int(dsize[0]), int(dsize[1])))


def _chunks(n: int) -> List[int]:
    out = []
    while n > 0:
        out.append(min(8, n))
        n -= out[-1]
    return out


def warp_feature(x: torch.Tensor, record_len, pairwise_t_matrix: torch.Tensor) -> torch.Tensor:
    """Warp every agent of every frame into its ego frame; returns [sum N, C, H, W]."""
    groups = host_ints(record_len)
    return ops.warp_fuse(x, _ego_rows(pairwise_t_matrix, groups), groups, ops.FUSE_NONE)


def fuse_multiscale(xs: Sequence[torch.Tensor], record_len, affine: torch.Tensor, mode: int, rows=None):
    """All feature scales of a batch in ONE launch per frame when every map is channels-last (the route the split-bf16 backbone
    produces): -> list of fused maps [B, C_s, H_s, W_s] (channels-last), or None when the maps do not qualify (caller falls back
    to one ``coalign_warp_fuse`` launch per scale)."""
    # (the map predicate on the first 8 rows: the 8-agent limit is per frame, checked below; a batch may hold more agents in all)
    if len(xs) > 3 or not all(ops.warp_fuse_nhwc_ok(x[:8]) for x in xs):
        return None
    groups = host_ints(record_len)
    if any(x.shape[0] != xs[0].shape[0] for x in xs) or sum(groups) != xs[0].shape[0] or max(groups) > 8:
        return None
    outs, off = [], 0
    for b, n in enumerate(groups):
        theta = affine[b, 0, :n]
        r = None if rows is None else [int(v) for v in rows[off:off + n]]
        outs.append(ops.warp_fuse_nhwc([x[off:off + n] for x in xs], theta, mode, rows=r))
        off += n
    if len(outs) == 1:
        return outs[0]
    return [torch.cat([o[k] for o in outs], dim=0) for k in range(len(xs))]


class MaxFusion(nn.Module):
    def forward(self, x: torch.Tensor, record_len, pairwise_t_matrix: torch.Tensor, rows=None) -> torch.Tensor:
        """``rows`` (not in the reference): row of ``x`` holding logical agent i, for agent-sharded callers."""
        groups = host_ints(record_len)
        return ops.warp_fuse(x, _ego_rows(pairwise_t_matrix, groups), groups, ops.FUSE_MAX, rows=rows)


class AttFusion(nn.Module):
    def __init__(self, feature_dims: int):
        super().__init__()
        self.feature_dims = feature_dims

    def forward(self, xx: torch.Tensor, record_len, normalized_affine_matrix: torch.Tensor, rows=None) -> torch.Tensor:
        groups = host_ints(record_len)
        # ScaledDotProductAttention divides by sqrt(feat_dim) of the CONFIG (att_fuse.py:36-44), the kernel by sqrt(C) of the tensor:
        # the two agree for every shipped yaml; a config where they differ would silently diverge from the reference's checkpoints
        if self.feature_dims != xx.shape[1]:
            # not the case in any shipped yaml.  The kernel's scores are <X0, Xj> / sqrt(C); feeding s X with s = (C / feat_dim)^(1/4) turns them
            # into <X0, Xj> / sqrt(feat_dim) and scales the output by s, which is divided out again (the warp is linear): the reference's
            # result to float32 rounding (one extra multiply and divide per element), instead of raising
            s = (xx.shape[1] / float(self.feature_dims)) ** 0.25
            return ops.warp_fuse(xx * s, _ego_rows(normalized_affine_matrix, groups), groups, ops.FUSE_ATT, rows=rows) / s
        return ops.warp_fuse(xx, _ego_rows(normalized_affine_matrix, groups), groups, ops.FUSE_ATT, rows=rows)


class PixelWeightLayer(nn.Module):
    """The per-pixel weight MLP of DiscoNet (disco_fuse.py:76-99): 1 x 1 convolutions 2C -> 128 -> 32 -> 8 -> 1, BatchNorm after the first three, ReLU after all four."""

    def __init__(self, channel: int):
        super().__init__()
        self.conv1_1 = nn.Conv2d(channel * 2, 128, kernel_size=1, stride=1, padding=0)
        self.bn1_1 = nn.BatchNorm2d(128)
        self.conv1_2 = nn.Conv2d(128, 32, kernel_size=1, stride=1, padding=0)
        self.bn1_2 = nn.BatchNorm2d(32)
        self.conv1_3 = nn.Conv2d(32, 8, kernel_size=1, stride=1, padding=0)
        self.bn1_3 = nn.BatchNorm2d(8)
        self.conv1_4 = nn.Conv2d(8, 1, kernel_size=1, stride=1, padding=0)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        x = x.view(-1, x.size(-3), x.size(-2), x.size(-1))
        x = F.relu(self.bn1_1(self.conv1_1(x)))
        x = F.relu(self.bn1_2(self.conv1_2(x)))
        x = F.relu(self.bn1_3(self.conv1_3(x)))
        return F.relu(self.conv1_4(x))

    def folded(self):
        """Eval mode: the BatchNorms folded into their convolutions -> [(weight [Cout, Cin, 1, 1], bias)] of the four layers (cached until a tensor changes)."""
        def build():
            layers = [fold_bn(c.weight, c.bias, bn) for c, bn in ((self.conv1_1, self.bn1_1), (self.conv1_2, self.bn1_2), (self.conv1_3, self.bn1_3))]
            return layers + [(self.conv1_4.weight.contiguous(), self.conv1_4.bias.contiguous())]
        return _cache_of(self).get(self, build)

    def forward_folded(self, x: torch.Tensor) -> torch.Tensor:
        """``forward`` of eval mode on the folded layers (what the kernel's parameter image is made of)."""
        x = x.view(-1, x.size(-3), x.size(-2), x.size(-1))
        for w, b in self.folded():
            x = F.relu(F.conv2d(x, w, b))
        return x

    def packed(self) -> Optional[torch.Tensor]:
        """The parameter image ``ops.disco_fuse`` reads (None: a folded weight outside the fp16 range), cached like ``folded``."""
        def build():
            (w1, b1), (w2, b2), (w3, b3), (w4, b4) = self.folded()
            img = ops.pack_disco_weights(w1, b1, w2, b2, w3, b3, w4, b4)
            return (img,)
        return _cache_of(self, "_coalign_disco_image").get(self, build)[0]


class DiscoFusion(nn.Module):
    """DiscoNet's fusion (fusion_in_one.py:138-171): every agent's map warped to the ego, a per-pixel weight from ``PixelWeightLayer([warped | ego])``, softmax over
    the agents, weighted sum.  On the GPU in eval mode, at a shape ``coalign_disco_fuse`` takes, one launch per frame; everywhere else (CPU, training, other channel
    counts, more than 8 agents) the reference's operations one by one -- which is also the statement of the semantics."""

    def __init__(self, feature_dims: int):
        super().__init__()
        self.pixel_weight_layer = PixelWeightLayer(feature_dims)
        self.force_torch = False      # measurement / test aid: take the op-by-op route whatever the device

    def kernel_route(self, channels: int, n_agents: int = 1) -> bool:
        """The static half of the decision (``routes.plan`` asks it): eval mode and a shape the kernel takes.  ``forward`` adds: a CUDA float32 map, packable weights."""
        return bool(not self.training and not self.force_torch and ops.disco_fuse_shape_ok(channels, n_agents))

    def forward_torch(self, xx: torch.Tensor, record_len, normalized_affine_matrix: torch.Tensor, folded: bool = False) -> torch.Tensor:
        _, C, H, W = xx.shape
        out = []
        for b, x in enumerate(regroup(xx, record_len)):
            N = x.shape[0]
            M = normalized_affine_matrix[b, 0, :N]
            grid = F.affine_grid(M, [N, C, H, W], align_corners=False).to(x)           # warp_affine_simple, torch_transformation_utils.py:322-331
            neighbor_feature = F.grid_sample(x, grid, align_corners=False)
            ego_feature = x[0].view(1, C, H, W).expand(N, -1, -1, -1)
            cat = torch.cat((neighbor_feature, ego_feature), dim=1)
            agent_weight = self.pixel_weight_layer.forward_folded(cat) if folded else self.pixel_weight_layer(cat)
            agent_weight = F.softmax(agent_weight, dim=0)
            out.append(torch.sum(agent_weight.expand(-1, C, -1, -1) * neighbor_feature, dim=0))
        return torch.stack(out)

    def forward(self, xx: torch.Tensor, record_len, normalized_affine_matrix: torch.Tensor, rows=None) -> torch.Tensor:
        if rows is not None:
            raise NotImplementedError("DiscoFusion does not run agent-sharded (rows)")
        groups = host_ints(record_len)
        image = None
        if xx.is_cuda and xx.dtype == torch.float32 and self.kernel_route(xx.shape[1], max(groups)) and sum(groups) == xx.shape[0]:
            image = self.pixel_weight_layer.packed()
        if image is None:
            return self.forward_torch(xx, groups, normalized_affine_matrix)
        if not xx.is_contiguous(memory_format=torch.channels_last):
            xx = xx.contiguous(memory_format=torch.channels_last)      # (the shrink header's conv3x3_sp writes channels-last: no copy on the detector's route)
        outs, off = [], 0
        for b, n in enumerate(groups):
            outs.append(ops.disco_fuse(xx[off:off + n], normalized_affine_matrix[b, 0, :n], image))
            off += n
        return outs[0] if len(outs) == 1 else torch.cat(outs, dim=0)
