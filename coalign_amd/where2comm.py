"""Where2comm's confidence-masked fusion (``Where2comm``, ``AttenFusion`` and ``MaxFusion``, opencood/models/fuse_modules/where2comm_attn.py:44-61 and :174-341;
``Communication``, opencood/models/comm_modules/where2comm.py:9-78), host side.

Every agent thresholds a (smoothed) confidence map of its own detections into a 0 / 1 mask; only masked features are "sent"; the receiver warps every agent's
masked map into the ego frame and fuses them per pixel (attention or maximum), at every backbone level in multi-scale mode.  Same constructor argument dict and
``state_dict`` names as the reference (``naive_communication.gaussian_filter.weight`` / ``.bias``, initialised by the reference's formula).

``forward_torch`` states the reference op by op and serves everything it serves.  ``forward_kernels`` runs two launches per call and frame: ``ops.w2comm_masks`` (all
masks of all levels and the rates) and ``ops.w2comm_fuse_nhwc`` (warp and fusion of the masked maps of up to three levels; the masked maps are never written).

``wire="packed"`` (off by default; ``PointPillarWhere2comm.packed_wire``) fuses from MESSAGES instead of the agents' dense maps: every non-ego agent's masked pixels
are packed (``W2Message``: a bitmap and the masked pixels' rows per level, ``ops.w2comm_msg_index`` + ``ops.w2comm_msg_pack``) and ``ops.w2comm_fuse_packed`` reads the
ego's dense maps and the others' messages -- to the same values as the dense route.  The reference has no counterpart; the format is stated in
include/coalign_amd_where2comm_msg.h and, op by op, by ``pack_messages_torch``.

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


# ---- messages: what an agent transmits (this project's format; the reference has none) ------------------------------------------------------------------------------
_I32 = 2 ** 32


def words_of(W: int) -> int:
    return (int(W) + 31) // 32


def pack_bits_torch(mask: torch.Tensor) -> torch.Tensor:
    """[..., H, W] 0 / nonzero -> int32 [..., H, ceil(W / 32)]: bit (x & 31) of word [y, x >> 5] is the mask at (y, x), padding bits zero (the words' bit patterns:
    torch has no arithmetic on uint32, so bit 31 is the int32's sign)."""
    W = mask.shape[-1]
    Wd = words_of(W)
    m = F.pad((mask != 0).to(torch.int64), (0, Wd * 32 - W)).reshape(*mask.shape[:-1], Wd, 32)
    v = (m << torch.arange(32, device=mask.device)).sum(-1)
    return (((v + 2 ** 31) % _I32) - 2 ** 31).to(torch.int32)


def unpack_bits_torch(bits: torch.Tensor, W: int) -> torch.Tensor:
    """int32 [..., H, Wd] -> uint8 [..., H, W] of 0 / 1 (padding bits are dropped, whatever they hold)."""
    b = (bits.to(torch.int64).unsqueeze(-1) >> torch.arange(32, device=bits.device)) & 1
    return b.reshape(*bits.shape[:-1], bits.shape[-1] * 32)[..., :W].to(torch.uint8)


def rank_torch(bits: torch.Tensor, W: int):
    """[H, Wd] -> (rank int32 [H, Wd]: the set bits before each word in raster order, K: their total as a 0-d int32 tensor)."""
    H, Wd = bits.shape
    per_word = F.pad(unpack_bits_torch(bits, W).to(torch.int64), (0, Wd * 32 - W)).reshape(H, Wd, 32).sum(-1).reshape(-1)
    inc = per_word.cumsum(0)
    return (inc - per_word).reshape(H, Wd).to(torch.int32), (inc[-1] if inc.numel() else inc.sum()).to(torch.int32)


class W2Message:
    """What ONE agent transmits (include/coalign_amd_where2comm_msg.h states the format and the wire layout).  Per level l: ``shapes[l]`` = (C, H, W), ``bits[l]`` int32
    [H, ceil(W / 32)] (the uint32 words' bit patterns), ``rows[l]`` float32 [max(1, H W), C] whose first K_l rows are the masked pixels in raster order, ``count``
    int32 [levels] ON THE DEVICE, and ``rank[l]`` int32 [H, Wd], which sender and receiver each compute and which does not travel.  Everything has a static shape;
    nothing here reads a count back except ``counts`` / ``nbytes`` / ``to_wire``, on demand."""
    MAGIC, VERSION, HEADER_BYTES, MAX_LEVELS = 0x4D433257, 1, 64, 3

    def __init__(self, shapes, bits, rows, count, rank):
        self.shapes = [tuple(int(v) for v in s) for s in shapes]
        self.bits, self.rows, self.count, self.rank = list(bits), list(rows), count, list(rank)
        if not 1 <= len(self.shapes) <= self.MAX_LEVELS or not len(self.bits) == len(self.rows) == len(self.rank) == len(self.shapes) or tuple(count.shape) != (len(self.shapes),):
            raise ValueError("W2Message: 1 .. 3 levels with bits, rows and rank each, count [levels]")
        for (C, H, W), b, r, k in zip(self.shapes, self.bits, self.rows, self.rank):
            if tuple(b.shape) != (H, words_of(W)) or tuple(k.shape) != (H, words_of(W)) or tuple(r.shape) != (max(1, H * W), C) or b.dtype != torch.int32 or r.dtype != torch.float32:
                raise ValueError(f"W2Message: level ({C}, {H}, {W}) with bits {tuple(b.shape)}, rank {tuple(k.shape)}, rows {tuple(r.shape)}")

    @property
    def levels(self) -> int:
        return len(self.shapes)

    @property
    def device(self):
        return self.count.device

    def fixed_bytes(self) -> int:
        """Header and bitmaps: the part of the size that does not depend on the masks."""
        return self.HEADER_BYTES + sum(4 * H * words_of(W) for _, H, W in self.shapes)

    def nbytes_device(self) -> torch.Tensor:
        """The message's size as a 0-d int64 tensor on the device, from ``count``: no read-back (``comm_bytes`` sums these inside a captured frame)."""
        count = self.count.to(torch.int64)          # (python scalars only: a constant tensor would be a host-to-device copy, which a capture refuses)
        return sum(count[l] * (4 * C) for l, (C, _, _) in enumerate(self.shapes)) + self.fixed_bytes()

    def counts(self) -> List[int]:
        """The K_l on the host: THE read-back."""
        return [int(v) for v in self.count.cpu().tolist()]

    @property
    def nbytes(self) -> int:
        return self.fixed_bytes() + sum(4 * K * C for K, (C, _, _) in zip(self.counts(), self.shapes))

    def masks(self) -> List[torch.Tensor]:
        return [unpack_bits_torch(b, W) for b, (_, _, W) in zip(self.bits, self.shapes)]

    def to_wire(self) -> torch.Tensor:
        """One contiguous uint8 tensor of exactly ``nbytes``, on the message's device: header, bits of every level, ``rows[:K]`` of every level."""
        counts = self.counts()
        head = np.zeros(self.HEADER_BYTES // 4, dtype="<u4")
        head[:3] = (self.MAGIC, self.VERSION, self.levels)
        for l, ((C, H, W), K) in enumerate(zip(self.shapes, counts)):
            head[4 + 4 * l: 8 + 4 * l] = (C, H, W, K)
        parts = [torch.from_numpy(head.view(np.uint8).copy()).to(self.device)]
        parts += [b.contiguous().view(torch.uint8).reshape(-1) for b in self.bits]
        parts += [r[:K].contiguous().view(torch.uint8).reshape(-1) for r, K in zip(self.rows, counts)]
        return torch.cat(parts)

    @classmethod
    def from_wire(cls, buf: torch.Tensor, device=None) -> "W2Message":
        """The device form of a wire buffer (uint8, any device).  The header, the buffer's length and the bitmaps' population are checked against each other on the
        host; the rank tables are recomputed (``ops.w2comm_msg_index``'s receiver form on a GPU, ``rank_torch`` on the CPU)."""
        device = torch.device(buf.device if device is None else device)
        if buf.dtype != torch.uint8 or buf.dim() != 1 or buf.numel() < cls.HEADER_BYTES or buf.numel() % 4:
            raise ValueError("W2Message.from_wire: a 1-d uint8 buffer of whole 32-bit words, at least a header long")
        raw = buf.detach().cpu().contiguous().numpy()
        head = raw[:cls.HEADER_BYTES].view("<u4")
        if int(head[0]) != cls.MAGIC or int(head[1]) != cls.VERSION or not 1 <= int(head[2]) <= cls.MAX_LEVELS:
            raise ValueError("W2Message.from_wire: not a version-1 Where2comm message")
        levels = int(head[2])
        shapes, counts = [], []
        for l in range(levels):
            C, H, W, K = (int(v) for v in head[4 + 4 * l: 8 + 4 * l])
            if C not in (64, 128, 256) or H < 1 or W < 1 or C * H * W >= 2 ** 31 or K > H * W:
                raise ValueError(f"W2Message.from_wire: level {l} says C {C}, H {H}, W {W}, K {K}")
            shapes.append((C, H, W)); counts.append(K)
        want = cls.HEADER_BYTES + sum(4 * (H * words_of(W) + K * C) for (C, H, W), K in zip(shapes, counts))
        if raw.size != want:
            raise ValueError(f"W2Message.from_wire: the header describes {want} bytes, the buffer has {raw.size}")
        pos, bits, rows = cls.HEADER_BYTES, [], []
        for (C, H, W), K in zip(shapes, counts):
            nb = 4 * H * words_of(W)
            b = torch.from_numpy(raw[pos:pos + nb].view("<i4").reshape(H, words_of(W)).copy())
            if int(unpack_bits_torch(b, W).sum()) != K:
                raise ValueError("W2Message.from_wire: a bitmap's population differs from the header's count")
            bits.append(b); pos += nb
        for (C, H, W), K in zip(shapes, counts):
            r = torch.zeros((max(1, H * W), C), dtype=torch.float32)
            r[:K] = torch.from_numpy(raw[pos:pos + 4 * K * C].view("<f4").reshape(K, C).copy())
            rows.append(r); pos += 4 * K * C
        bits, rows = [b.to(device) for b in bits], [r.to(device) for r in rows]
        count = torch.tensor(counts, dtype=torch.int32, device=device)
        if device.type == "cuda":
            _, rank, _ = ops.w2comm_msg_index(None, [b.unsqueeze(0) for b in bits], [(H, W) for _, H, W in shapes])
            rank = [r[0] for r in rank]
        else:
            rank = [rank_torch(b, W)[0] for b, (_, _, W) in zip(bits, shapes)]
        return cls(shapes, bits, rows, count, rank)


def pack_messages_torch(xs: Sequence[torch.Tensor], masks: Sequence[torch.Tensor]) -> List[W2Message]:
    """The format, op by op (any device; the CPU tests' side and the specification of ``Where2comm.pack_messages``): ``xs[l]`` [n, C_l, H_l, W_l], ``masks[l]``
    [n, H_l, W_l] -> one message per agent.  Rows behind the count are zero here; the kernels leave them unwritten."""
    out = []
    for j in range(xs[0].shape[0]):
        shapes, bits, rows, counts, rank = [], [], [], [], []
        for x, m in zip(xs, masks):
            _, C, H, W = x.shape
            on = m[j] != 0
            b = pack_bits_torch(on)
            rk, K = rank_torch(b, W)
            r = torch.zeros((max(1, H * W), C), dtype=torch.float32, device=x.device)
            sent = x[j].permute(1, 2, 0)[on]                        # raster order: y major, x ascending
            r[:sent.shape[0]] = sent
            shapes.append((C, H, W)); bits.append(b); rows.append(r); counts.append(K); rank.append(rk)
        out.append(W2Message(shapes, bits, rows, torch.stack(counts), rank))
    return out


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
    KERNELS_PACKED = ("w2comm_masks + w2comm_msg_index + w2comm_msg_pack + w2comm_fuse_packed: the masks and rates in one launch, then per frame the bitmaps, rank tables and "
                      "counts of the non-ego agents in one launch, their masked pixels packed into rows in one launch, and the warp and fusion of the ego's dense maps "
                      "and the others' messages in one launch (channels-last; the messages' sizes summed on the device)")
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

    def packed_route_reason(self, channels: Sequence[int], n_agents: int = 1, resnet: bool = True, anchors: int = 1) -> Optional[str]:
        """None when ``wire="packed"`` is served for these shapes, else why not, in words: the packed route has no op-by-op fallback, it raises with these."""
        if self.training:
            return "training mode: the message kernels run in eval mode only"
        if self.force_torch:
            return "force_torch: the op-by-op route builds no messages"
        if not self.communication:
            return "no communication section: there are no masks to pack by"
        reason = self.kernel_shape_reason(channels, n_agents, resnet, anchors)
        if reason is None and not ops.w2comm_msg_shape_ok(channels, n_agents):
            reason = f"maps of {list(channels)} channels from {n_agents} agents outside the message kernels' shapes"
        return reason

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
    def pack_messages(self, xs: Sequence[torch.Tensor], masks: Sequence[torch.Tensor]) -> List[W2Message]:
        """What the agents of ``xs`` transmit: ``xs[l]`` [n, C_l, H_l, W_l] channels-last float32 on the GPU, ``masks[l]`` [n, H_l, W_l] uint8 -> one ``W2Message`` per
        agent, in two launches for all of them (``pack_messages_torch`` states the result op by op)."""
        bits, rank, count = ops.w2comm_msg_index(list(masks))
        rows = ops.w2comm_msg_pack(list(xs), bits, rank)
        shapes = [tuple(x.shape[1:]) for x in xs]
        return [W2Message(shapes, [b[j] for b in bits], [r[j] for r in rows], count[j], [k[j] for k in rank]) for j in range(xs[0].shape[0])]

    def fuse_messages(self, ego_xs: Sequence[torch.Tensor], ego_masks: Sequence[Optional[torch.Tensor]], messages: Sequence[W2Message], affine_row: torch.Tensor, mode=None) -> list:
        """The receiver: the ego's own dense maps (``ego_xs[l]`` [1, C_l, H_l, W_l] channels-last, ``ego_masks[l]`` [1, H_l, W_l] uint8 or None) and the other agents'
        messages, in the agents' order, ``affine_row`` [n, 2, 3] -> the fused map [1, C_l, H_l, W_l] per level, in one launch."""
        mode = (ops.FUSE_ATT if self.agg_mode == "ATTEN" else ops.FUSE_MAX) if mode is None else mode
        shapes = [tuple(x.shape[-3:]) for x in ego_xs]
        for m in messages:
            if m.shapes != [tuple(int(v) for v in s) for s in shapes]:
                raise ValueError(f"Where2comm.fuse_messages: a message of levels {m.shapes} for an ego of levels {shapes}")
        sources = [[(x, None if mk is None else mk.reshape(mk.shape[-2:]))] + [(m.rows[l], m.bits[l], m.rank[l]) for m in messages] for l, (x, mk) in enumerate(zip(ego_xs, ego_masks))]
        return ops.w2comm_fuse_packed(sources, shapes, affine_row, mode)

    def fuse_levels(self, xs: Sequence[torch.Tensor], rm: torch.Tensor, groups: Sequence[int], affine: torch.Tensor, wire: str = "dense"):
        """The two launches: the agents' maps of every level (channels-last) and their logits -> (the fused maps [B, C_l, H_l, W_l] per level, the rate).
        ``wire="packed"``: every non-ego agent is packed into a message and the fusion reads the messages -> (the same fused maps, the rate, the messages: per frame the
        list of its non-ego agents').  No check of the route is made here: ``fuse`` makes it."""
        if wire not in ("dense", "packed"):
            raise ValueError(f"Where2comm: wire '{wire}' (dense | packed)")
        mode = ops.FUSE_ATT if self.agg_mode == "ATTEN" else ops.FUSE_MAX
        if wire == "packed" and not self.communication:
            raise NotImplementedError("Where2comm, wire='packed': " + self.packed_route_reason([x.shape[1] for x in xs], max(groups)))
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
        outs, messages, off = [], [], 0
        for bi, n in enumerate(groups):
            if wire == "packed":
                sent = self.pack_messages([x[off + 1:off + n] for x in xs], [m[off + 1:off + n] for m in masks]) if n > 1 else []
                outs.append(self.fuse_messages([x[off:off + 1] for x in xs], [m[off:off + 1] for m in masks], sent, affine[bi, 0, :n], mode))
                messages.append(sent)
            else:
                outs.append(ops.w2comm_fuse_nhwc([x[off:off + n] for x in xs], [m[off:off + n] for m in masks], affine[bi, 0, :n], mode))
            off += n
        fused = outs[0] if len(outs) == 1 else [torch.cat([o[k] for o in outs], dim=0) for k in range(len(xs))]
        rate = sum(rates.unbind(0)) / len(groups)          # sum(communication_rates) / B in the reference's order (where2comm.py:76)
        return (fused, rate, messages) if wire == "packed" else (fused, rate)

    def forward_kernels(self, xs: Sequence[torch.Tensor], rm: torch.Tensor, groups: Sequence[int], affine: torch.Tensor, backbone=None, wire: str = "dense"):
        fused, rates, *messages = self.fuse_levels(xs, rm, groups, affine, wire)
        return (backbone.decode_multiscale_feature(fused) if self.multi_scale else fused[0]), rates, ({"messages": messages[0]} if messages else {})

    def fuse(self, x, rm: torch.Tensor, record_len, affine: torch.Tensor, backbone=None, feats=None, rows=None, decode: bool = True, wire: str = "dense"):
        """``forward`` behind its normalisation.  ``feats``: the levels ``backbone.resnet(x)`` gives, when the caller has them (``x`` is then not read).
        ``decode=False`` (multi-scale callers with a tail of their own): -> (the LIST of fused levels, rate) on the kernel route, (the decoded map, rate) else.
        ``wire="packed"``: the kernel route through messages or an error that says why not -- never the op-by-op route; the messages come back as the third value
        (``decode=False``) or under ``"messages"`` in the third value's dict."""
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
        if wire not in ("dense", "packed"):
            raise ValueError(f"Where2comm: wire '{wire}' (dense | packed)")
        served = xs is not None and self._kernel_inputs_ok(xs, rm, groups, backbone)
        if wire == "packed" and not (served and self.communication):
            raise NotImplementedError("Where2comm, wire='packed' has no op-by-op route: " + self._packed_refusal(x, xs, rm, groups, backbone))
        if served:
            if not decode and self.multi_scale:
                return self.fuse_levels(xs, rm, groups, affine, wire)
            return self.forward_kernels(xs, rm, groups, affine, backbone, wire)
        out = self.forward_torch(x, rm, groups, affine, backbone, feats=xs if self.multi_scale else None)
        return out if decode or not self.multi_scale else out[:2]

    def _packed_refusal(self, x, xs, rm, groups, backbone) -> str:
        """Why ``fuse(wire="packed")`` cannot run, in words: the static reasons first (``packed_route_reason``), then the inputs'."""
        maps = xs if xs is not None else [x]
        resnet = backbone is None or hasattr(backbone, "resnet")
        channels = [m.shape[1] for m in maps] if not (self.multi_scale and not resnet) else [0] * len(self._modules_of())
        anchors = rm.shape[1] if self.communication and torch.is_tensor(rm) and rm.dim() == 4 else 1
        reason = self.packed_route_reason(channels, max(groups), resnet, anchors)
        if reason is None and not all(torch.is_tensor(m) and m.is_cuda for m in maps):
            reason = "maps on the CPU: the message kernels run on the GPU only"
        return reason or "maps that are not float32 channels-last, levels that do not halve exactly, or logits that are not float32 on the GPU"

    def forward(self, x, rm, record_len, pairwise_t_matrix, backbone=None, rows=None):
        _, C, H, W = x.shape
        affine = normalize_pairwise_tfm(pairwise_t_matrix, H, W, self.discrete_ratio, self.downsample_rate)          # where2comm_attn.py:248-252, on a copy
        return self.fuse(x, rm, record_len, affine, backbone, rows=rows)
