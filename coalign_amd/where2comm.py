"""Where2comm's confidence-masked fusion (``Where2comm``, ``AttenFusion`` and ``MaxFusion``, opencood/models/fuse_modules/where2comm_attn.py:44-61 and :174-341;
``Communication``, opencood/models/comm_modules/where2comm.py:9-78), host side.

Every agent thresholds a (smoothed) confidence map of its own detections into a 0 / 1 mask; only masked features are "sent"; the receiver warps every agent's
masked map into the ego frame and fuses them per pixel (attention or maximum), at every backbone level in multi-scale mode.  Same constructor argument dict and
``state_dict`` names as the reference (``naive_communication.gaussian_filter.weight`` / ``.bias``, initialised by the reference's formula).

``forward_torch`` states the reference op by op and serves everything it serves.  ``forward_kernels`` runs two launches per call and frame: ``ops.w2comm_masks`` (all
masks of all levels and the rates) and ``ops.w2comm_fuse_nhwc`` (warp and fusion of the masked maps of up to three levels; the masked maps are never written).

Quirks of the reference that are kept: the masks of the agents with an even index inside their frame are all ones
(``communication_mask_nodiag[::2] = 1``, where2comm.py:71), the rate counts the ego's mask before that; single-scale mode masks every agent of frame b with the
mask of the batch's agent number b (``Where2comm.frame_masks``); ``round`` is read and never used; without ``communication``
the rate is the integer tensor 0.  Refused: ``agg_operator.mode: Transformer`` (it cannot run in the reference either, see ``Where2comm.__init__``)."""
from __future__ import annotations

from typing import List, Optional, Sequence

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import ops
from .encoder import host_ints
from .pose import normalize_pairwise_tfm


def _warp_torch(src: torch.Tensor, M: torch.Tensor) -> torch.Tensor:
    """warp_affine_simple (torch_transformation_utils.py:322-331) in torch ops, output size = input size."""
    grid = F.affine_grid(M, list(src.shape), align_corners=False).to(src)
    return F.grid_sample(src, grid, align_corners=False)


class ScaledDotProductAttention(nn.Module):
    """where2comm_attn.py:11-42."""

    def __init__(self, dim):
        super().__init__()
        self.sqrt_dim = np.sqrt(dim)

    def forward(self, query, key, value):
        score = torch.bmm(query, key.transpose(1, 2)) / self.sqrt_dim
        attn = F.softmax(score, -1)
        return torch.bmm(attn, value)


class AttenFusion(nn.Module):
    """where2comm_attn.py:44-54: self attention over the agents at every pixel, the ego's row returned."""

    def __init__(self, feature_dim):
        super().__init__()
        self.feature_dim = feature_dim
        self.att = ScaledDotProductAttention(feature_dim)

    def forward(self, x):
        cav_num, C, H, W = x.shape
        x = x.reshape(cav_num, C, -1).permute(2, 0, 1)
        x = self.att(x, x, x)
        return x.permute(1, 2, 0).reshape(cav_num, C, H, W)[0]


class MaxFusion(nn.Module):
    """where2comm_attn.py:56-61."""

    def forward(self, x):
        return torch.max(x, dim=0)[0]


class Communication(nn.Module):
    """where2comm.py:9-78: the confidence maps of every agent -> communication masks and the batch's communication rate."""

    def __init__(self, args):
        super().__init__()
        self.smooth = False
        self.thre = args["thre"]
        if "gaussian_smooth" in args:
            self.smooth = True
            kernel_size = args["gaussian_smooth"]["k_size"]
            c_sigma = args["gaussian_smooth"]["c_sigma"]
            self.gaussian_filter = nn.Conv2d(1, 1, kernel_size=kernel_size, stride=1, padding=(kernel_size - 1) // 2)
            self.init_gaussian_filter(kernel_size, c_sigma)
            self.gaussian_filter.requires_grad = False          # (as in the reference: an attribute of the module, the parameters keep theirs)

    def init_gaussian_filter(self, k_size=5, sigma=1):
        center = k_size // 2
        x, y = np.mgrid[0 - center: k_size - center, 0 - center: k_size - center]
        g = 1 / (2 * np.pi * sigma) * np.exp(-(np.square(x) + np.square(y)) / (2 * np.square(sigma)))      # (the reference's 1 / (2 pi sigma), where2comm.py:28)
        self.gaussian_filter.weight.data = torch.Tensor(g).to(self.gaussian_filter.weight.device).unsqueeze(0).unsqueeze(0)
        self.gaussian_filter.bias.data.zero_()

    def kernel_size(self) -> int:
        return int(self.gaussian_filter.kernel_size[0]) if self.smooth else 0

    def forward(self, batch_confidence_maps, record_len, pairwise_t_matrix=None):
        """``pairwise_t_matrix`` is accepted and, as in the reference, not read."""
        B = len(batch_confidence_maps)
        _, _, H, W = batch_confidence_maps[0].shape
        communication_masks, communication_rates, batch_communication_maps = [], [], []
        for b in range(B):
            ori_communication_maps = batch_confidence_maps[b].sigmoid().max(dim=1)[0].unsqueeze(1)
            communication_maps = self.gaussian_filter(ori_communication_maps) if self.smooth else ori_communication_maps
            ones_mask = torch.ones_like(communication_maps)
            zeros_mask = torch.zeros_like(communication_maps)
            communication_mask = torch.where(communication_maps > self.thre, ones_mask, zeros_mask)
            communication_rate = communication_mask[0].sum() / (H * W)
            communication_mask_nodiag = communication_mask.clone()
            communication_mask_nodiag[::2] = ones_mask[::2]
            communication_masks.append(communication_mask_nodiag)
            communication_rates.append(communication_rate)
            batch_communication_maps.append(ori_communication_maps * communication_mask_nodiag)
        communication_rates = sum(communication_rates) / B
        return batch_communication_maps, torch.cat(communication_masks, dim=0), communication_rates


class Where2comm(nn.Module):
    """where2comm_attn.py:174-341.  ``forward`` keeps the reference's signature and normalises ``pairwise_t_matrix`` itself (:248-252); ``fuse`` is the entry point of
    callers that hold the normalised affine and, in multi-scale mode, the backbone's levels already (``feats``), so that the ResNet does not run twice.

    Not in the reference: ``rows`` (see ``fusion.AttFusion.forward``; refused, as by the other baselines: ``ops.w2comm_fuse_nhwc`` takes a row table, the masks do
    not), ``force_torch``."""

    def __init__(self, args):
        super().__init__()
        self.communication = False
        self.round = 1
        if "communication" in args:
            self.communication = True
            self.naive_communication = Communication(args["communication"])
            if "round" in args["communication"]:
                self.round = args["communication"]["round"]          # read and never used, as in the reference
        self.discrete_ratio = args["voxel_size"][0]
        self.downsample_rate = args["downsample_rate"]
        self.agg_mode = args["agg_operator"]["mode"]
        self.multi_scale = args["multi_scale"]
        if self.agg_mode == "Transformer":
            raise NotImplementedError(
                "agg_operator.mode 'Transformer' of Where2comm is not built: it cannot run in the reference either -- TransformerFusion.forward takes four arguments "
                "and is called with one (where2comm_attn.py:295, :338), EncodeLayer passes quality_map to nn.MultiheadAttention, which has no such argument (:91), "
                "and the single-scale branch stores the module as fuse_network while forward reads fuse_modules (:213, :338)")
        if self.agg_mode not in ("ATTEN", "MAX"):
            raise NotImplementedError(f"agg_operator.mode '{self.agg_mode}' of Where2comm (ATTEN | MAX)")
        if self.multi_scale:
            layer_nums, num_filters = args["layer_nums"], args["num_filters"]
            self.num_levels = len(layer_nums)
            self.fuse_modules = nn.ModuleList([AttenFusion(num_filters[idx]) if self.agg_mode == "ATTEN" else MaxFusion() for idx in range(self.num_levels)])
        else:
            self.fuse_modules = AttenFusion(args["agg_operator"]["feature_dim"]) if self.agg_mode == "ATTEN" else MaxFusion()
        self.force_torch = False      # measurement / test aid: take the op-by-op route whatever the device

    def regroup(self, x, record_len):
        return list(torch.split(x, host_ints(record_len), dim=0))

    # ---- route decision --------------------------------------------------------------------------------------------------------------------------------------
    def _modules_of(self) -> List[nn.Module]:
        return list(self.fuse_modules) if self.multi_scale else [self.fuse_modules]

    KERNELS = ("w2comm_masks + w2comm_fuse_nhwc: the communication masks of every agent and level and the rates in one launch, then per frame the warp and fusion of "
               "the masked maps of all levels in one launch (channels-last; no masked map is written)")
    KERNELS_PLAIN = "warp_fuse_nhwc: all scales in one launch (channels-last); no communication section: no masks, rate 0"
    TORCH = "Where2comm op by op in PyTorch"
    MASKS = "w2comm_masks (the smoothing runs inside the mask launch, fp32)"

    def kernel_shape_reason(self, channels: Sequence[int], n_agents: int = 1, resnet: bool = True, anchors: int = 1) -> Optional[str]:
        """None when the kernels take maps of ``channels`` (one entry per level) from ``n_agents`` agents, else why not, in words (``routes.plan`` prints it)."""
        channels, mods = list(channels), self._modules_of()
        if self.multi_scale and not resnet:
            return "a plain BaseBEVBackbone feeds every block the masked map of the one before: the levels cannot be fused in one launch"
        if len(channels) != len(mods) or not 1 <= len(channels) <= 3 or any(c not in (64, 128, 256) for c in channels):
            return f"maps of {channels} channels outside the kernel's 64 / 128 / 256, at most three levels"
        if any(isinstance(m, AttenFusion) and m.feature_dim != c for m, c in zip(mods, channels)):
            return "an attention whose feature_dim differs from its map's channels"
        if not 1 <= n_agents <= 8:
            return f"{n_agents} agents in a frame outside 1 .. 8"
        if self.communication and not ops.w2comm_masks_shape_ok(anchors, [n_agents], self.naive_communication.kernel_size(), len(channels)):
            return "a smoothing kernel (even, or larger than 9) or an anchor count (more than 8) the mask kernel does not take"
        return None

    def kernel_route(self, channels: Sequence[int], n_agents: int = 1, resnet: bool = True, anchors: int = 1) -> bool:
        """The static half of the decision (``routes.plan`` asks it): eval mode and shapes the kernels take.  ``fuse`` adds: CUDA float32 channels-last maps, levels that
        halve exactly, logits of the kernel's anchor count."""
        return bool(not self.training and not self.force_torch and self.kernel_shape_reason(channels, n_agents, resnet, anchors) is None)

    def _kernel_inputs_ok(self, xs: Sequence[torch.Tensor], rm: torch.Tensor, groups: Sequence[int], backbone) -> bool:
        anchors = rm.shape[1] if self.communication else 1
        if not all(torch.is_tensor(x) and x.dim() == 4 for x in xs) or not self.kernel_route([x.shape[1] for x in xs], max(groups), backbone is None or hasattr(backbone, "resnet"), anchors):
            return False
        if not all(ops.warp_fuse_nhwc_ok(x[:8]) and x.shape[0] == sum(groups) for x in xs) or (self.communication and not (rm.is_cuda and rm.dtype == torch.float32 and rm.dim() == 4)):
            return False
        if any(tuple(b.shape[2:]) != (a.shape[2] // 2, a.shape[3] // 2) for a, b in zip(xs[:-1], xs[1:])):
            return False
        return len(groups) <= ops.W2COMM_MAX_GROUPS or not self.communication

    # ---- the reference, op by op ------------------------------------------------------------------------------------------------------------------------------
    def _check_rm(self, rm: torch.Tensor, x: torch.Tensor) -> None:
        if self.communication and tuple(rm.shape[2:]) != tuple(x.shape[2:]):
            raise ValueError(f"Where2comm: the confidence map is {tuple(rm.shape[2:])}, the map it masks {tuple(x.shape[2:])}: they must have one size")

    @staticmethod
    def frame_masks(communication_masks: torch.Tensor, groups: Sequence[int]) -> torch.Tensor:
        """Single-scale mode multiplies frame b's maps by ``communication_masks[b]`` (where2comm_attn.py:334), and ``communication_masks`` is the concatenation over
        ALL agents (where2comm.py:77): every agent of frame b is masked by the mask of the batch's agent number b -- for a batch of one frame the ego's, which is all
        ones.  Kept as it is: [n_total, ...] -> [n_total, ...] with frame b's rows all equal to row b."""
        return torch.cat([communication_masks[b:b + 1].expand(n, *communication_masks.shape[1:]) for b, n in enumerate(groups)], dim=0)

    def _fuse_frames(self, x: torch.Tensor, groups: Sequence[int], affine: torch.Tensor, module: nn.Module) -> torch.Tensor:
        x_fuse = []
        for b, node_features in enumerate(self.regroup(x, groups)):
            N = groups[b]
            neighbor_feature = _warp_torch(node_features, affine[b, 0, :N])
            x_fuse.append(module(neighbor_feature))
        return torch.stack(x_fuse)

    def forward_torch(self, x: torch.Tensor, rm: torch.Tensor, record_len, affine: torch.Tensor, backbone=None, feats=None):
        """``affine``: the normalised [B, L, L, 2, 3] of where2comm_attn.py:248-252.  ``feats``: ``backbone.resnet(x)`` when the caller has it already."""
        groups = host_ints(record_len)
        if self.multi_scale:
            ups = []
            with_resnet = hasattr(backbone, "resnet")
            if with_resnet and feats is None:
                feats = backbone.resnet(x)
            for i in range(self.num_levels):
                x = feats[i] if with_resnet else backbone.blocks[i](x)
                if i == 0:
                    if self.communication:
                        self._check_rm(rm, x)
                        _, communication_masks, communication_rates = self.naive_communication(self.regroup(rm, groups), groups, affine)
                        x = x * communication_masks
                    else:
                        communication_rates = torch.tensor(0).to(x.device)
                elif self.communication:
                    communication_masks = F.max_pool2d(communication_masks, kernel_size=2)
                    x = x * communication_masks
                x_fuse = self._fuse_frames(x, groups, affine, self.fuse_modules[i])
                ups.append(backbone.deblocks[i](x_fuse) if len(backbone.deblocks) > 0 else x_fuse)
            x_fuse = torch.cat(ups, dim=1) if len(ups) > 1 else ups[0]
            if len(backbone.deblocks) > self.num_levels:
                x_fuse = backbone.deblocks[-1](x_fuse)
        else:
            if self.communication:
                self._check_rm(rm, x)
                _, communication_masks, communication_rates = self.naive_communication(self.regroup(rm, groups), groups, affine)
                x = x * self.frame_masks(communication_masks, groups)
            else:
                communication_rates = torch.tensor(0).to(x.device)
            x_fuse = self._fuse_frames(x, groups, affine, self.fuse_modules)
        return x_fuse, communication_rates, {}

    # ---- the kernel route -------------------------------------------------------------------------------------------------------------------------------------
    def fuse_levels(self, xs: Sequence[torch.Tensor], rm: torch.Tensor, groups: Sequence[int], affine: torch.Tensor):
        """The two launches: the agents' maps of every level (channels-last) and their logits -> (the fused maps [B, C_l, H_l, W_l] per level, the rate)."""
        mode = ops.FUSE_ATT if self.agg_mode == "ATTEN" else ops.FUSE_MAX
        if not self.communication:
            from .fusion import fuse_multiscale
            fused = fuse_multiscale(list(xs), groups, affine, mode)
            if fused is None:          # (its predicate is the one the route has just asked)
                raise ops.hip.CoalignHipError("Where2comm: the maps passed the kernel route's checks and the fusion kernel declined them")
            return fused, torch.tensor(0).to(xs[0].device)
        self._check_rm(rm, xs[0])
        comm = self.naive_communication
        w, b = (comm.gaussian_filter.weight.detach(), comm.gaussian_filter.bias.detach()) if comm.smooth else (None, None)
        masks, rates = ops.w2comm_masks(rm, groups, w, b, comm.thre, levels=len(xs))
        if not self.multi_scale:
            masks = [self.frame_masks(masks[0], groups).contiguous()]          # (bytes: n_total H W of them)
        outs, off = [], 0
        for bi, n in enumerate(groups):
            outs.append(ops.w2comm_fuse_nhwc([x[off:off + n] for x in xs], [m[off:off + n] for m in masks], affine[bi, 0, :n], mode))
            off += n
        fused = outs[0] if len(outs) == 1 else [torch.cat([o[k] for o in outs], dim=0) for k in range(len(xs))]
        return fused, sum(rates.unbind(0)) / len(groups)          # sum(communication_rates) / B in the reference's order (where2comm.py:76)

    def forward_kernels(self, xs: Sequence[torch.Tensor], rm: torch.Tensor, groups: Sequence[int], affine: torch.Tensor, backbone=None):
        fused, rates = self.fuse_levels(xs, rm, groups, affine)
        return (backbone.decode_multiscale_feature(fused) if self.multi_scale else fused[0]), rates, {}

    def fuse(self, x, rm: torch.Tensor, record_len, affine: torch.Tensor, backbone=None, feats=None, rows=None, decode: bool = True):
        """``forward`` behind its normalisation.  ``feats``: the levels ``backbone.resnet(x)`` gives, when the caller has them (``x`` is then not read).
        ``decode=False`` (multi-scale callers with a tail of their own): -> (the LIST of fused levels, rate) on the kernel route, (the decoded map, rate) else."""
        if rows is not None:
            raise NotImplementedError("Where2comm does not run agent-sharded (rows): the masks follow the agents' order inside their frame")
        groups = host_ints(record_len)
        xs = None
        if self.multi_scale and hasattr(backbone, "resnet"):
            xs = feats if feats is not None else (backbone.resnet(x) if x.is_cuda and not self.training and not self.force_torch else None)
        elif not self.multi_scale:
            xs = [x]
            if x.is_cuda and x.dtype == torch.float32 and not ops.is_channels_last(x) and self.kernel_route([x.shape[1]], max(groups), True, rm.shape[1] if self.communication else 1):
                xs = [x.contiguous(memory_format=torch.channels_last)]          # (a stride-1 shrink header on the SplitMap route writes channels-last: no copy there)
        if xs is not None and self._kernel_inputs_ok(xs, rm, groups, backbone):
            if not decode and self.multi_scale:
                return self.fuse_levels(xs, rm, groups, affine)
            return self.forward_kernels(xs, rm, groups, affine, backbone)
        out = self.forward_torch(x, rm, groups, affine, backbone, feats=xs if self.multi_scale else None)
        return out if decode or not self.multi_scale else out[:2]

    def forward(self, x, rm, record_len, pairwise_t_matrix, backbone=None, rows=None):
        _, C, H, W = x.shape
        affine = normalize_pairwise_tfm(pairwise_t_matrix, H, W, self.discrete_ratio, self.downsample_rate)          # where2comm_attn.py:248-252, on a copy
        return self.fuse(x, rm, record_len, affine, backbone, rows=rows)
