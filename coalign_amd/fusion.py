"""Multi-agent feature fusion modules (SURVEY §8a rows G, H, H'), host side.

Class / function names and signatures follow opencood/models/fuse_modules/fusion_in_one.py
(``regroup`` :21-24, ``warp_feature`` :26-45, ``MaxFusion`` :47-89, ``AttFusion`` :91-136, ``DiscoFusion`` :138-171, ``V2VNetFusion`` :173-293) and
opencood/models/sub_modules/torch_transformation_utils.py (``warp_affine_simple`` :322-331).  ``MaxFusion`` / ``AttFusion`` own no
parameters; all their arithmetic is the fused gfx950 kernel ``coalign_warp_fuse``.  ``DiscoFusion`` owns ``PixelWeightLayer``
(opencood/models/fuse_modules/disco_fuse.py:76-99) and runs on ``coalign_disco_fuse``.  ``V2VNetFusion`` owns ``msg_cnn``, a ``ConvGRU``
(opencood/models/sub_modules/convgru.py) and ``mlp``; its convolutions run on ``coalign_conv3x3_sp``, what lies between them on the three ``coalign_v2v_*`` kernels.
``V2XViTFusion`` (fusion_in_one.py:295-352) and its transformer blocks live in :mod:`coalign_amd.v2xvit` and are re-exported here, as is ``When2comFusion``
(``When2commFusion``, fusion_in_one.py:354-431) of :mod:`coalign_amd.when2com` and ``Where2commFusion`` (``Where2comm``, fuse_modules/where2comm_attn.py:174-341) of
:mod:`coalign_amd.where2comm`.
"""
from __future__ import annotations

from typing import List, Optional, Sequence

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import ops
from . import backbone as _bb
from .backbone import Conv3x3Pack, PointwisePack, _cache_of, fold_bn
from .encoder import host_ints
from .v2xvit import V2XViTFusion  # noqa: F401  (fusion.V2XViTFusion: the house address of every fusion module)
from .when2com import When2comFusion  # noqa: F401  (fusion.When2comFusion)
from .where2comm import Where2comm as Where2commFusion  # noqa: F401  (fusion.Where2commFusion: the name the reference's lss_submodule.py imports)


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
    def plan_fusion(self, channels: int, terms: Optional[int] = None):
        """``routes.plan``'s fusion line of ONE parameter-free module on the shrunk map (point_pillar_baseline: max | att): the NCHW kernel, listed as a fallback."""
        return "warp_fuse: one launch (NCHW, LDS-staged patches)", True, {}

    def forward(self, x: torch.Tensor, record_len, pairwise_t_matrix: torch.Tensor, rows=None) -> torch.Tensor:
        """``rows`` (not in the reference): row of ``x`` holding logical agent i, for agent-sharded callers."""
        groups = host_ints(record_len)
        return ops.warp_fuse(x, _ego_rows(pairwise_t_matrix, groups), groups, ops.FUSE_MAX, rows=rows)


class AttFusion(nn.Module):
    plan_fusion = MaxFusion.plan_fusion

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

    KERNELS, TORCH = "disco_fuse: warp + pixel-weight MLP + softmax in one launch", "DiscoFusion op by op in PyTorch"

    def kernel_shape_reason(self, channels: int, n_agents: int = 1) -> Optional[str]:
        """None when ``coalign_disco_fuse`` takes (channels, n_agents), else why not, in words (``routes.plan`` prints it)."""
        if not ops.disco_fuse_shape_ok(channels, 1):
            return "channels outside the kernel's C % 32 == 0, 32 .. 384"
        return None if ops.disco_fuse_shape_ok(channels, n_agents) else f"{n_agents} agents in a frame outside 1 .. 8"

    def kernel_route(self, channels: int, n_agents: int = 1) -> bool:
        """The static half of the decision (``routes.plan`` asks it): eval mode and a shape the kernel takes.  ``forward`` adds: a CUDA float32 map, packable weights."""
        return bool(not self.training and not self.force_torch and self.kernel_shape_reason(channels, n_agents) is None)

    def plan_fusion(self, channels: int, terms: Optional[int] = None):
        """-> (``routes.plan``'s fusion line, whether it is a fallback, {layers noted with it: (line, fallback)})."""
        if self.kernel_route(channels):
            return self.KERNELS, False, {}
        return f"{self.TORCH} ({self.kernel_shape_reason(channels) or _bb.TORCH_MODE})", True, {}

    def plan_layer(self, name: str, layer: nn.Module, channels: int, terms: Optional[int] = None):
        """-> (line, fallback) of one of this module's layers: the four 1 x 1 layers of ``PixelWeightLayer`` run inside the fusion launch."""
        ok = self.kernel_route(channels)
        return ("disco_fuse (pixel-weight MLP layer inside the fusion launch)" if ok else _bb.MIOPEN + " (DiscoFusion op by op)"), not ok

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


class ConvGRUCell(nn.Module):
    """convgru.py:7-70: gates and candidate of one GRU step as two convolutions over [input | hidden]."""

    def __init__(self, input_size, input_dim: int, hidden_dim: int, kernel_size, bias: bool):
        super().__init__()
        self.height, self.width = input_size
        self.padding = kernel_size[0] // 2, kernel_size[1] // 2
        self.input_dim, self.hidden_dim, self.bias = input_dim, hidden_dim, bias
        self.conv_gates = nn.Conv2d(input_dim + hidden_dim, 2 * hidden_dim, kernel_size=tuple(kernel_size), padding=self.padding, bias=bias)
        self.conv_can = nn.Conv2d(input_dim + hidden_dim, hidden_dim, kernel_size=tuple(kernel_size), padding=self.padding, bias=bias)

    def init_hidden(self, batch_size: int) -> torch.Tensor:
        return torch.zeros(batch_size, self.hidden_dim, self.height, self.width)

    def forward(self, input_tensor: torch.Tensor, h_cur: torch.Tensor) -> torch.Tensor:
        combined_conv = self.conv_gates(torch.cat([input_tensor, h_cur], dim=1))
        gamma, beta = torch.split(combined_conv, self.hidden_dim, dim=1)
        reset_gate, update_gate = torch.sigmoid(gamma), torch.sigmoid(beta)
        cnm = torch.tanh(self.conv_can(torch.cat([input_tensor, reset_gate * h_cur], dim=1)))
        return (1 - update_gate) * h_cur + update_gate * cnm

    def reduced(self):
        """With h_cur = 0 the cell is ONE convolution input_dim -> 2 hidden followed by sigmoid(first half) * tanh(second half): rows [hidden, 2 hidden) of
        ``conv_gates`` (the update gate) stacked on ``conv_can``, the first ``input_dim`` input columns of both -> (weight [2 hidden, input_dim, k, k], bias)."""
        h, i = self.hidden_dim, self.input_dim
        w = torch.cat([self.conv_gates.weight[h:2 * h, :i], self.conv_can.weight[:, :i]], dim=0).contiguous()
        if self.conv_gates.bias is None:
            return w, w.new_zeros(2 * h)
        return w, torch.cat([self.conv_gates.bias[h:2 * h], self.conv_can.bias]).contiguous()


class ConvGRU(nn.Module):
    """convgru.py:73-196, as far as V2VNetFusion uses it: stacked cells, ``hidden_state`` None (zeros), the last layer's outputs returned."""

    def __init__(self, input_size, input_dim: int, hidden_dim, kernel_size, num_layers: int, batch_first: bool = False, bias: bool = True,
                 return_all_layers: bool = False):
        super().__init__()
        kernel_size = kernel_size if isinstance(kernel_size, list) else [kernel_size] * num_layers
        hidden_dim = hidden_dim if isinstance(hidden_dim, list) else [hidden_dim] * num_layers
        if not len(kernel_size) == len(hidden_dim) == num_layers:
            raise ValueError("Inconsistent list length.")
        self.height, self.width = input_size
        self.input_dim, self.hidden_dim, self.kernel_size, self.num_layers = input_dim, hidden_dim, kernel_size, num_layers
        self.batch_first, self.bias, self.return_all_layers = batch_first, bias, return_all_layers
        self.cell_list = nn.ModuleList([ConvGRUCell((self.height, self.width), input_dim if i == 0 else hidden_dim[i - 1], hidden_dim[i], kernel_size[i], bias)
                                        for i in range(num_layers)])

    def forward(self, input_tensor: torch.Tensor, hidden_state=None):
        if not self.batch_first:
            input_tensor = input_tensor.permute(1, 0, 2, 3, 4)
        if hidden_state is not None:
            raise NotImplementedError()
        layer_output_list, last_state_list = [], []
        cur = input_tensor
        for cell in self.cell_list:
            h = cell.init_hidden(input_tensor.size(0)).to(input_tensor.device).to(input_tensor.dtype)
            outs = []
            for t in range(cur.size(1)):
                h = cell(cur[:, t], h)
                outs.append(h)
            cur = torch.stack(outs, dim=1)
            layer_output_list.append(cur)
            last_state_list.append([h])
        if not self.return_all_layers:
            layer_output_list, last_state_list = layer_output_list[-1:], last_state_list[-1:]
        return layer_output_list, last_state_list


def _warp_torch(src: torch.Tensor, M: torch.Tensor) -> torch.Tensor:
    """warp_affine_simple (torch_transformation_utils.py:322-331) in torch ops, output size = input size."""
    grid = F.affine_grid(M, list(src.shape), align_corners=False).to(src)
    return F.grid_sample(src, grid, align_corners=False)


class V2VNetFusion(nn.Module):
    """V2VNet's message passing (fusion_in_one.py:173-293).  Per iteration every agent i receives, from every agent j, ``msg_cnn([warp_i(x_j) | x_i])`` masked by the
    warp of a map of ones; the messages are reduced over j (max / mean) and a ConvGRU with a ZERO hidden state (or a plain sum) turns [x_i | agg_i] into the new x_i;
    after the last iteration the ego's map goes through ``mlp``.

    ``forward_torch`` states that op by op.  Three exact identities cut its work to a third (``forward_reduced``, the schedule of the kernel route):
    a GRU cell with h = 0 is one convolution in -> 2 hidden and ``sigmoid(beta) * tanh(cnm)`` (``ConvGRUCell.reduced``); ``msg_cnn`` is linear, so its ego half is
    computed once per receiver; the last iteration updates the ego alone.  On the GPU in eval mode (``kernel_route``) the convolutions run on ``ops.conv3x3_sp`` and
    the glue on ``ops.v2v_warp_split`` / ``v2v_aggregate`` / ``v2v_gate``, one launch per stage over all (receiver, sender) pairs of a frame.

    ``agg_operator: weight`` (fuse_modules/v2v_fuse.py:140-141, the pose-robust V2VNet's fusion): ``agg_i = sum_j message_ij * weight[b, i, j]`` with the caller's
    ``weight`` [B, L, L], products and sums in order of j; on the kernel route ``ops.v2vr_aggregate``.  Without a weight every route raises ``ValueError``."""

    def __init__(self, args: dict):
        super().__init__()
        in_channels = args["in_channels"]
        gru = args["conv_gru"]
        self.num_iteration = args["num_iteration"]
        self.gru_flag = args["gru_flag"]
        self.agg_operator = args["agg_operator"]
        self.msg_cnn = nn.Conv2d(in_channels * 2, in_channels, kernel_size=3, stride=1, padding=1)
        self.conv_gru = ConvGRU(input_size=(gru["H"], gru["W"]), input_dim=in_channels * 2, hidden_dim=[in_channels] * gru["num_layers"], kernel_size=gru["kernel_size"],
                                num_layers=gru["num_layers"], batch_first=True, bias=True, return_all_layers=False)
        self.mlp = nn.Linear(in_channels, in_channels)
        self.force_torch = False      # measurement / test aid: take the op-by-op route whatever the device

    def _check_agg(self, weight=None, static: bool = False) -> None:
        """``static``: the name alone (``kernel_route`` answers before any weight exists)."""
        if self.agg_operator not in ("max", "avg", "weight"):
            raise ValueError("agg_operator has wrong value")
        if self.agg_operator == "weight" and weight is None and not static:
            raise ValueError("agg_operator 'weight' needs the weight [B, L, L] of the senders (v2v_fuse.py:140-141)")

    def kernel_route(self, channels: int, n_agents: int = 1, terms: Optional[int] = None) -> bool:
        """The static half of the decision (``routes.plan`` asks it): eval mode, 3 x 3 GRU kernels, widths ``conv3x3_sp`` takes (C % 64 == 0, 2C <= its 1024-channel
        limit), at most 8 agents, the SplitMap arithmetic in force.  ``forward`` adds: a CUDA float32 map."""
        self._check_agg(static=True)
        return bool(not self.training and not self.force_torch and self.kernel_shape_reason(channels, n_agents, terms) is None)

    KERNELS = "v2v_warp_split + conv3x3_sp + v2v_aggregate + conv3x3_sp + v2v_gate per iteration, one launch per stage over all (receiver, sender) pairs"
    TORCH = "V2VNetFusion op by op in PyTorch"

    def kernel_shape_reason(self, channels: int, n_agents: int = 1, terms: Optional[int] = None) -> Optional[str]:
        """None when the kernels take (channels, n_agents) in the arithmetic in force, else why not, in words (``routes.plan`` prints it)."""
        if not all(tuple(c.conv_gates.kernel_size) == (3, 3) for c in self.conv_gru.cell_list):
            return "GRU kernels other than 3 x 3"
        if channels != self.msg_cnn.out_channels or channels % 64 or not _bb.sp_channels_ok(2 * channels, 2 * channels) or not ops.v2v_shape_ok(channels, 1):
            return f"{channels} channels outside C % 64 == 0, C <= 512"
        if not ops.v2v_shape_ok(channels, n_agents):
            return f"{n_agents} agents in a frame outside 1 .. 8"
        return None if _bb.split_maps_active(terms) else "the SplitMap arithmetic (fp16 x 2) is not in force"

    def plan_mlp(self, terms: Optional[int], ok: bool) -> dict:
        """``mlp``'s line, noted with the fusion line (after the walk of the layers)."""
        return {"fusion_net.mlp": (_bb.pointwise_text(self.mlp.in_features, terms) + ", 1 x 1 on the fused map" if ok else _bb.LINEAR_LIBRARY + ", V2VNetFusion op by op)", not ok)}

    def plan_fusion(self, channels: int, terms: Optional[int] = None):
        """-> (``routes.plan``'s fusion line, whether it is a fallback, {layers noted with it: (line, fallback)})."""
        ok = self.kernel_route(channels, 1, terms)
        return (self.KERNELS if ok else f"{self.TORCH} ({self.kernel_shape_reason(channels, 1, terms) or _bb.TORCH_MODE})"), not ok, self.plan_mlp(terms, ok)

    def plan_layer(self, name: str, layer: nn.Module, channels: int, terms: Optional[int] = None, ok: Optional[bool] = None):
        """-> (line, fallback) of msg_cnn and the GRU cells' convolutions; None for ``mlp``, which is noted with the fusion line.  ``ok``: the decision of a model
        that takes the kernels for all of its parts or for none (the pose-robust V2VNet), in place of this module's own."""
        if not isinstance(layer, nn.Conv2d):
            return None
        ok = self.kernel_route(channels, 1, terms) if ok is None else ok
        what = (" (V2VNet: the warped-map and the ego columns as two C -> C convolutions)" if name.endswith("msg_cnn") else
                " (V2VNet: update-gate rows of conv_gates stacked on conv_can, one convolution per GRU cell)")
        return (_bb.SP + what if ok else _bb.MIOPEN + " (V2VNetFusion op by op)"), not ok

    # ---- the reference's loops, op by op -----------------------------------------------------------------------------------------------------------------
    def forward_torch(self, x: torch.Tensor, record_len, normalized_affine_matrix: torch.Tensor, weight: Optional[torch.Tensor] = None) -> torch.Tensor:
        _, C, H, W = x.shape
        groups = host_ints(record_len)
        feats = list(torch.split(x, groups, dim=0))
        A = normalized_affine_matrix
        if self.agg_operator == "weight":
            self._check_agg(weight)
        masks = [[_warp_torch(x.new_ones((N, 1, H, W)), A[b, i, :N]) for i in range(N)] for b, N in enumerate(groups)]
        for _ in range(self.num_iteration):
            updated_batch = []
            for b, N in enumerate(groups):
                updated = []
                for i in range(N):
                    neighbor_feature = _warp_torch(feats[b], A[b, i, :N])
                    ego_agent_feature = feats[b][i].unsqueeze(0).repeat(N, 1, 1, 1)
                    message = self.msg_cnn(torch.cat([neighbor_feature, ego_agent_feature], dim=1)) * masks[b][i]
                    if self.agg_operator == "avg":
                        agg_feature = torch.mean(message, dim=0)
                    elif self.agg_operator == "max":
                        agg_feature = torch.max(message, dim=0)[0]
                    elif self.agg_operator == "weight":                                                            # v2v_fuse.py:140-141
                        agg_feature = torch.sum(message * weight[b][i, :N].view(-1, 1, 1, 1).to(message), dim=0)
                    else:
                        raise ValueError("agg_operator has wrong value")
                    if self.gru_flag:
                        cat_feature = torch.cat([feats[b][i], agg_feature], dim=0)
                        gru_out = self.conv_gru(cat_feature.unsqueeze(0).unsqueeze(0))[0][0].squeeze(0).squeeze(0)
                    else:
                        gru_out = feats[b][i] + agg_feature
                    updated.append(gru_out.unsqueeze(0))
                updated_batch.append(torch.cat(updated, dim=0))
            feats = updated_batch
        out = torch.cat([f[0].unsqueeze(0) for f in feats], dim=0)
        return self.mlp(out.permute(0, 2, 3, 1)).permute(0, 3, 1, 2)

    # ---- the three identities, in the kernel route's schedule ------------------------------------------------------------------------------------------------
    def reduced_weights(self):
        """(msg_cnn's warped-map columns [C, C, 3, 3], its ego columns, its bias, [(cell weight [2 hidden, in, 3, 3], bias)]): views / stacks of the parameters."""
        C = self.msg_cnn.out_channels
        w = self.msg_cnn.weight
        return w[:, :C].contiguous(), w[:, C:].contiguous(), self.msg_cnn.bias, [c.reduced() for c in self.conv_gru.cell_list]

    @staticmethod
    def _receivers(iteration: int, iterations: int, n: int) -> int:
        return n if iteration < iterations - 1 else 1      # the output reads agent 0 of the last iteration only

    def forward_reduced(self, x: torch.Tensor, record_len, normalized_affine_matrix: torch.Tensor, weight: Optional[torch.Tensor] = None) -> torch.Tensor:
        self._check_agg(weight)
        _, C, H, W = x.shape
        groups = host_ints(record_len)
        wn, we, bm, cells = self.reduced_weights()
        outs, off = [], 0
        for b, N in enumerate(groups):
            xb, theta = x[off:off + N], normalized_affine_matrix[b, :N, :N]
            off += N
            for it in range(self.num_iteration):
                R = self._receivers(it, self.num_iteration, N)
                e = F.conv2d(xb[:R], we, bm, padding=1)                                                              # the ego term, once per receiver
                warped = torch.cat([_warp_torch(xb, theta[i]) for i in range(R)], dim=0)                             # [R N, C, H, W]
                a = F.conv2d(warped, wn, None, padding=1).view(R, N, C, H, W)
                mask = torch.stack([_warp_torch(xb.new_ones((N, 1, H, W)), theta[i]) for i in range(R)], dim=0)      # [R, N, 1, H, W]
                m = (a + e.unsqueeze(1)) * mask
                if self.agg_operator == "max":
                    agg = m.max(dim=1)[0]
                elif self.agg_operator == "weight":                                                                # the products and the sum in order of j
                    wb = weight[b].to(m)
                    agg = m[:, 0] * wb[:R, 0].view(R, 1, 1, 1)
                    for j in range(1, N):
                        agg = agg + m[:, j] * wb[:R, j].view(R, 1, 1, 1)
                else:
                    agg = m[:, 0]
                    for j in range(1, N):
                        agg = agg + m[:, j]
                    agg = agg / N
                if self.gru_flag:
                    h = torch.cat([xb[:R], agg], dim=1)
                    for cw, cb in cells:
                        y = F.conv2d(h, cw, cb, padding=1)
                        hid = cw.shape[0] // 2
                        h = torch.sigmoid(y[:, :hid]) * torch.tanh(y[:, hid:])
                else:
                    h = xb[:R] + agg
                xb = h
            outs.append(xb[:1])
        out = torch.cat(outs, dim=0)
        return self.mlp(out.permute(0, 2, 3, 1)).permute(0, 3, 1, 2)

    # ---- the kernel route ----------------------------------------------------------------------------------------------------------------------------------------
    def packed(self):
        """The weight images of the kernel route (``Conv3x3Pack(...).emu(16, True)`` of the sliced weights, the pointwise image of ``mlp``), cached until a parameter
        changes: (warped-map image, ego image, msg bias, zero bias, [(cell image, bias, 2 hidden)], mlp image, mlp bias)."""
        def build():
            wn, we, bm, cells = self.reduced_weights()
            C = wn.shape[0]
            mlp = PointwisePack(self.mlp.weight.detach().reshape(C, C, 1, 1), False)
            return (Conv3x3Pack(wn).emu(16, True), Conv3x3Pack(we).emu(16, True), bm.detach().float().contiguous(), torch.zeros_like(bm, dtype=torch.float32),
                    [(Conv3x3Pack(cw).emu(16, True), cb.detach().float().contiguous(), cw.shape[0]) for cw, cb in cells], mlp.get(), self.mlp.bias.detach().float().contiguous())
        return _cache_of(self, "_coalign_v2v_images").get(self, build)

    def forward_kernels(self, xx: torch.Tensor, groups: Sequence[int], normalized_affine_matrix: torch.Tensor, weight: Optional[torch.Tensor] = None,
                        first_warp=None) -> torch.Tensor:
        """``first_warp``: per frame the SplitMap ``ops.v2v_warp_split(x_b, theta_b)`` a caller has already made of the INPUT maps (the pose-robust model's attention
        reads the same warp), used in place of iteration 0's own."""
        self._check_agg(weight)
        img_n, img_e, bm, zero, cells, img_mlp, b_mlp = self.packed()
        C = xx.shape[1]
        if not ops.nhwc_memory(xx):
            xx = xx.contiguous(memory_format=torch.channels_last)      # (a stride-1 shrink header's conv3x3_sp writes channels-last: no copy there)
            if not ops.nhwc_memory(xx):                                 # (a 1 x 1 map or C = 1: every stride order counts as channels-last)
                xx = xx.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
        outs, off = [], 0
        for b, n in enumerate(groups):
            xb = xx[off:off + n]
            theta = normalized_affine_matrix[b, :n, :n].to(device=xx.device, dtype=torch.float64).contiguous()
            off += n
            wb = None
            if self.agg_operator == "weight":
                wb = weight[b].to(device=xx.device, dtype=torch.float32).contiguous()
            for it in range(self.num_iteration):
                R = self._receivers(it, self.num_iteration, n)
                th = theta[:R]
                e = ops.conv3x3_sp(ops.SplitMap.pack(xb[:R]), img_e, bm, C, None, False, out_split=False)
                warped = ops.v2v_warp_split(xb, th) if it > 0 or first_warp is None else ops.SplitMap(first_warp[b].data[:R * n])
                a = ops.conv3x3_sp(warped, img_n, zero, C, None, False, out_split=False)
                if wb is not None:
                    h = ops.v2vr_aggregate(a, e, xb, th, wb, gru=bool(self.gru_flag))
                else:
                    h = ops.v2v_aggregate(a, e, xb, th, self.agg_operator, gru=bool(self.gru_flag))
                if self.gru_flag:
                    for k, (img, bias, width) in enumerate(cells):
                        h = ops.v2v_gate(ops.conv3x3_sp(h, img, bias, width, None, False, out_split=False), out_split=k + 1 < len(cells))
                xb = h
            outs.append(xb[:1])
        out = outs[0] if len(outs) == 1 else torch.cat(outs, dim=0)
        return ops.pointwise_conv(out, img_mlp, b_mlp, C, relu=False, out_channels_last=True)

    def forward(self, x: torch.Tensor, record_len, normalized_affine_matrix: torch.Tensor, weight: Optional[torch.Tensor] = None, rows=None) -> torch.Tensor:
        if rows is not None:
            raise NotImplementedError("V2VNetFusion does not run agent-sharded (rows)")
        groups = host_ints(record_len)
        if x.is_cuda and x.dtype == torch.float32 and sum(groups) == x.shape[0] and self.kernel_route(x.shape[1], max(groups)):
            return self.forward_kernels(x, groups, normalized_affine_matrix, weight)
        self._check_agg(weight)
        return self.forward_torch(x, groups, normalized_affine_matrix, weight)
