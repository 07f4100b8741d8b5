"""When2com's handshake fusion as OpenCOOD's ``point_pillar_baseline`` runs it (``When2commFusion``, opencood/models/fuse_modules/fusion_in_one.py:354-431, with
``policy_net4``, ``km_generator_v2``, ``conv2DBatchNormRelu`` and ``AdditiveAttentin`` of opencood/models/fuse_modules/when2com_fuse.py:133-363), host side.

Per frame every agent's map is warped into the ego frame (the ego's own too), five 3 x 3 convolution blocks (``query_key_net``) shrink it to a quarter of its size
at 256 channels, a key net on every agent and a query net on the ego alone (a strided block, a 5 x 7 adaptive average pool, three linears) give one vector each, an
additive attention's two linears and a dot product give one logit per agent, and the output is the softmax-weighted sum of the warped maps.  Same constructor keys
and ``state_dict`` names as the reference, members it never reads included (``attention_net.linear_out``, ``sparsemax``).

``forward_torch`` states that op by op.  ``forward_reduced`` applies the exact identities the kernel route is built on; ``forward_kernels`` runs them on the gfx950
kernels: ``ops.v2v_warp_split``, six launches of ``ops.conv3x3_sp`` / ``conv3x3_sp_s2`` on SplitMaps (the key and the query block stacked in the sixth),
``ops.w2c_score`` and ``ops.w2c_fuse``."""
from __future__ import annotations

from typing import Optional, Sequence

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import backbone as _bb
from . import ops
from .backbone import Conv3x3Pack, _cache_of, fold_bn
from .encoder import host_ints


class conv2DBatchNormRelu(nn.Module):
    """when2com_fuse.py:133-166: Conv2d (with bias) + BatchNorm2d + ReLU as ``cbr_unit``."""

    def __init__(self, in_channels, n_filters, k_size, stride, padding, bias=True, dilation=1, is_batchnorm=True):
        super().__init__()
        conv_mod = nn.Conv2d(int(in_channels), int(n_filters), kernel_size=k_size, padding=padding, stride=stride, bias=bias, dilation=dilation)
        if is_batchnorm:
            self.cbr_unit = nn.Sequential(conv_mod, nn.BatchNorm2d(int(n_filters)), nn.ReLU(inplace=True))
        else:
            self.cbr_unit = nn.Sequential(conv_mod, nn.ReLU(inplace=True))

    def forward(self, inputs):
        return self.cbr_unit(inputs)

    def folded(self):
        """Eval mode: (weight with the BatchNorm's scale, shift carrying the convolution's bias, stride)."""
        conv = self.cbr_unit[0]
        if isinstance(self.cbr_unit[1], nn.BatchNorm2d):
            w, b = fold_bn(conv.weight, conv.bias, self.cbr_unit[1])
        else:
            w, b = conv.weight, conv.bias if conv.bias is not None else conv.weight.new_zeros(conv.out_channels)
        return w, b, conv.stride[0]


class Sparsemax(nn.Module):
    """when2com_fuse.py:169-235.  Constructed by ``AdditiveAttentin`` like in the reference (it owns no parameters); ``When2comFusion`` always calls the attention
    with ``sparse=False``, so it is never evaluated and is not restated here."""

    def __init__(self, dim=None):
        super().__init__()
        self.dim = -1 if dim is None else dim

    def forward(self, input):
        raise NotImplementedError("sparsemax (AdditiveAttentin with sparse=True) is outside what When2comFusion runs")


class km_generator_v2(nn.Module):
    """when2com_fuse.py:253-270: a strided 256 -> 128 block, AdaptiveAvgPool2d((5, 7)), Linear 4480 -> 256 -> 128 -> out_size with ReLU between."""

    def __init__(self, out_size=128):
        super().__init__()
        self.conv1 = conv2DBatchNormRelu(256, 128, k_size=3, stride=2, padding=1)
        self.avgp = nn.AdaptiveAvgPool2d((5, 7))
        self.n_feat = int(128 * 5 * 7)
        self.fc = nn.Sequential(nn.Linear(self.n_feat, 256), nn.ReLU(inplace=True), nn.Linear(256, 128), nn.ReLU(inplace=True), nn.Linear(128, out_size))

    def forward(self, feat_map):
        feat_map = self.avgp(self.conv1(feat_map))
        return self.fc(feat_map.view(-1, self.n_feat))


class policy_net4(nn.Module):
    """when2com_fuse.py:272-291: C -> 512 -> 256, stride 2, 256, stride 2."""

    def __init__(self, in_channel):
        super().__init__()
        self.conv1 = conv2DBatchNormRelu(in_channel, 512, k_size=3, stride=1, padding=1)
        self.conv2 = conv2DBatchNormRelu(512, 256, k_size=3, stride=1, padding=1)
        self.conv3 = conv2DBatchNormRelu(256, 256, k_size=3, stride=2, padding=1)
        self.conv4 = conv2DBatchNormRelu(256, 256, k_size=3, stride=1, padding=1)
        self.conv5 = conv2DBatchNormRelu(256, 256, k_size=3, stride=2, padding=1)

    def blocks(self):
        return [self.conv1, self.conv2, self.conv3, self.conv4, self.conv5]

    def forward(self, x):
        for block in self.blocks():
            x = block(x)
        return x


class AdditiveAttentin(nn.Module):
    """when2com_fuse.py:342-363 (the reference's spelling): logits = linear_feat(k) . linear_context(q), softmax (or sparsemax) over the agents, weighted sum."""

    def __init__(self, c_k, c_q):
        super().__init__()
        self.softmax = nn.Softmax(dim=1)
        self.sparsemax = Sparsemax(dim=1)
        self.linear_feat = nn.Linear(c_k, 128)
        self.linear_context = nn.Linear(c_q, 128)
        self.linear_out = nn.Linear(128, 1)      # constructed and never read, as in the reference

    def logits(self, q, k):
        return torch.bmm(self.linear_feat(k), self.linear_context(q).transpose(2, 1))      # [b, N, 1]

    def forward(self, q, k, v, sparse=True):
        attn_orig = self.logits(q, k)
        attn_orig = self.sparsemax(attn_orig) if sparse else self.softmax(attn_orig)
        attn = attn_orig.unsqueeze(-1).unsqueeze(-1)
        return (attn * v).sum(1), attn


def _warp_torch(src: torch.Tensor, M: torch.Tensor) -> torch.Tensor:
    """warp_affine_simple (torch_transformation_utils.py:322-331) in torch ops, output size = input size."""
    grid = F.affine_grid(M, list(src.shape), align_corners=False).to(src)
    return F.grid_sample(src, grid, align_corners=False)


class When2comFusion(nn.Module):
    """``When2commFusion`` (fusion_in_one.py:354-431).  ``forward_torch`` is the reference op by op: the yardstick, and the route on the CPU, in training mode and at
    shapes the kernels do not take.  The kernel route rests on exact identities (``forward_reduced`` states them in torch ops):

    (a) eval BatchNorm and the convolution's bias fold into weight and shift (``backbone.fold_bn``);
    (b) ``linear_feat(fc[4](.))`` and ``linear_context(fc[4](.))`` are two linears with nothing between them: one 128 x 128 matrix and a bias each, folded in float64
        (``key_size`` and ``query_size`` vanish from the run);
    (c) ``key_net.conv1`` and ``query_net.conv1`` read the same map: their rows run stacked as one 256 -> 256 convolution, and the query head reads the ego's rows
        128 .. 255 of it alone (one stacked launch measured 24.8 us against 48.1 us for a key launch on n maps plus a query launch on one, at 5 x 256 x 13 x 44);
    (d) a frame with one agent has the weight 1 (a softmax over one logit), whatever the logit: its output is the warp of its map, and the heads are not run.

    ``feat_H`` / ``feat_W`` are stored and never read, like in the reference."""

    def __init__(self, args: dict):
        super().__init__()
        self.in_channels = args["in_channels"]
        self.feat_H = args["H"]
        self.feat_W = args["W"]
        self.query_size = args["query_size"]
        self.key_size = args["key_size"]
        self.query_key_net = policy_net4(self.in_channels)
        self.key_net = km_generator_v2(out_size=self.key_size)
        self.query_net = km_generator_v2(out_size=self.query_size)
        self.attention_net = AdditiveAttentin(self.key_size, self.query_size)
        self.force_torch = False      # measurement / test aid: take the op-by-op route whatever the device

    # ---- the route decision ----------------------------------------------------------------------------------------------------------------------------------
    def kernel_shape_reason(self, channels: int, n_agents: int = 1, terms: Optional[int] = None) -> Optional[str]:
        """None when the kernels take (channels, n_agents) in the arithmetic in force, else why not, in words (``routes.plan`` prints it)."""
        if channels != self.in_channels:
            return f"{channels} channels, but query_key_net.conv1 reads {self.in_channels}"
        if not ops.w2c_shape_ok(channels, 1) or not _bb.sp_channels_ok(channels, 512):
            return f"{channels} channels outside C % 16 == 0"
        if not 1 <= n_agents <= 8:
            return f"{n_agents} agents in a frame outside 1 .. 8"
        if not _bb.split_maps_active(terms):
            return "the SplitMap arithmetic (fp16 x 2) is not in force"
        return None

    def kernel_route(self, channels: int, n_agents: int = 1, terms: Optional[int] = None) -> bool:
        """The static half of the decision (``routes.plan`` asks it): eval mode and a shape the kernels take.  ``forward`` adds: a CUDA float32 map."""
        return bool(not self.training and not self.force_torch and self.kernel_shape_reason(channels, n_agents, terms) is None)

    KERNELS = ("v2v_warp_split + conv3x3_sp x 3 + conv3x3_sp_s2 x 3 + w2c_score + w2c_fuse per frame: the warped maps as SplitMaps, policy_net4 and the stacked key | query block on "
               "the SplitMap convolutions, the pooled heads with the softmax over the agents in two launches, warp and weighted sum in one; a one-agent frame is w2c_fuse alone")
    TORCH = "When2comFusion op by op in PyTorch"
    SCORE, UNREAD = "w2c_score", "never read (AdditiveAttentin.forward does not use linear_out)"

    def plan_fusion(self, channels: int, terms: Optional[int] = None):
        """-> (``routes.plan``'s fusion line, whether it is a fallback, {layers noted with it: (line, fallback)})."""
        if self.kernel_route(channels, 1, terms):
            return self.KERNELS, False, {}
        return f"{self.TORCH} ({self.kernel_shape_reason(channels, 1, terms) or _bb.TORCH_MODE})", True, {}

    def plan_layer(self, name: str, layer: nn.Module, channels: int, terms: Optional[int] = None):
        """-> (line, fallback) of one of this module's convolutions or linears."""
        ok = self.kernel_route(channels, 1, terms)
        if isinstance(layer, nn.Conv2d):
            what = (" (When2com: stacked under key_net.conv1 in one launch; the ego's rows are read)" if name.startswith("fusion_net.query_net.") else
                    " (When2com: query_net.conv1 stacked under it in one launch)" if name.startswith("fusion_net.key_net.") else " (When2com: every agent's warped map)")
            return ((_bb.SP_S2 if layer.stride[0] == 2 else _bb.SP + _bb.SPLIT_OUT) + what if ok else _bb.MIOPEN + " (When2comFusion op by op)"), not ok
        if name.endswith("attention_net.linear_out"):
            return self.UNREAD, False
        if not ok:
            return _bb.LINEAR_LIBRARY + ", When2comFusion op by op)", True
        part = ("first layer, 4480 inputs spread over 256 workgroups" if name.endswith("fc.0") else "second layer" if name.endswith("fc.2") else
                "folded with the attention's linear into one 128 x 128 matrix" if name.endswith("fc.4") else "folded into the key / query net's last layer")
        return f"{self.SCORE} ({part}, fp32)", False

    # ---- the reference, op by op ----------------------------------------------------------------------------------------------------------------------------------
    def frame_torch(self, x: torch.Tensor, theta: torch.Tensor):
        """One frame: x [N, C, H, W], theta [N, 2, 3] (the ego's row) -> (fused [1, C, H, W], logits [N], weights [N])."""
        neighbor_feature = _warp_torch(x, theta)                                        # all N maps, the ego's own included
        query_key_maps = self.query_key_net(neighbor_feature)
        keys = self.key_net(query_key_maps).unsqueeze(0)                                  # [1, N, key_size]
        query = self.query_net(query_key_maps[0].unsqueeze(0)).unsqueeze(0)              # [1, 1, query_size]
        logits = self.attention_net.logits(query, keys)
        feat_fuse, attn = self.attention_net(query, keys, neighbor_feature.unsqueeze(0), sparse=False)
        return feat_fuse, logits.reshape(-1), attn.reshape(-1)

    def forward_torch(self, x: torch.Tensor, record_len, normalized_affine_matrix: torch.Tensor, details: Optional[list] = None) -> torch.Tensor:
        """``details`` (tests): a list that receives (logits, weights) per frame."""
        groups = host_ints(record_len)
        out = []
        for b, xb in enumerate(torch.split(x, groups, dim=0)):
            fused, logits, w = self.frame_torch(xb, normalized_affine_matrix[b, 0, :groups[b]].to(x.device))
            out.append(fused)
            if details is not None:
                details.append((logits, w))
        return torch.cat(out, dim=0)

    # ---- the identities ---------------------------------------------------------------------------------------------------------------------------------------------
    def folded_tail(self, which: str):
        """(b): (T [128, out of fc.2], tb [128]) of ``key`` (linear_feat o key_net.fc[4]) or ``query`` (linear_context o query_net.fc[4]), float64."""
        net, lin = (self.key_net, self.attention_net.linear_feat) if which == "key" else (self.query_net, self.attention_net.linear_context)
        last = net.fc[4]
        A, W = lin.weight.detach().double(), last.weight.detach().double()
        return A @ W, A @ last.bias.detach().double() + lin.bias.detach().double()

    def reduced_weights(self):
        """([(weight, shift, stride)] of the five folded blocks, the stacked key | query block, [(W1, b1, W2, b2, T, tb)] of key and query net; T, tb in float64)."""
        heads = []
        for which, net in (("key", self.key_net), ("query", self.query_net)):
            T, tb = self.folded_tail(which)
            heads.append((net.fc[0].weight, net.fc[0].bias, net.fc[2].weight, net.fc[2].bias, T, tb))
        (wk, sk, stride), (wq, sq, _) = self.key_net.conv1.folded(), self.query_net.conv1.folded()
        return [blk.folded() for blk in self.query_key_net.blocks()], (torch.cat([wk, wq]), torch.cat([sk, sq]), stride), heads

    @staticmethod
    def _head(pooled_in: torch.Tensor, head) -> torch.Tensor:
        W1, b1, W2, b2, T, tb = head
        p = F.adaptive_avg_pool2d(pooled_in, (5, 7)).reshape(pooled_in.shape[0], -1)
        h = F.relu(F.linear(F.relu(F.linear(p, W1, b1)), W2, b2))
        return F.linear(h, T.to(h.dtype), tb.to(h.dtype))

    def forward_reduced(self, x: torch.Tensor, record_len, normalized_affine_matrix: torch.Tensor, details: Optional[list] = None) -> torch.Tensor:
        groups = host_ints(record_len)
        blocks, (wkq, skq, _), (khead, qhead) = self.reduced_weights()
        out = []
        for b, xb in enumerate(torch.split(x, groups, dim=0)):
            n = groups[b]
            v = _warp_torch(xb, normalized_affine_matrix[b, 0, :n].to(x.device))
            if n == 1:                                                                       # (d)
                out.append(v)
                if details is not None:
                    details.append((None, v.new_ones(1)))
                continue
            m = v
            for w, s, stride in blocks:                                                      # (a)
                m = F.relu(F.conv2d(m, w, s, stride=stride, padding=1))
            kq = F.relu(F.conv2d(m, wkq, skq, stride=2, padding=1))                                          # (c): key rows | query rows
            kf, qf = self._head(kq[:, :128], khead), self._head(kq[:1, 128:], qhead)                         # [n, 128], [1, 128]  (b)
            logits = kf @ qf[0]
            w = torch.softmax(logits, dim=0)
            fused = w[0] * v[0]
            for j in range(1, n):
                fused = fused + w[j] * v[j]
            out.append(fused.unsqueeze(0))
            if details is not None:
                details.append((logits, w))
        return torch.cat(out, dim=0)

    # ---- the kernel route -----------------------------------------------------------------------------------------------------------------------------------------
    def packed(self):
        """The weight images of the kernel route, cached until a parameter changes: ([(image, shift, Cout, stride)] of the five blocks, the stacked key | query
        block, the parameter image of ``ops.w2c_score``, the weight of a one-agent frame)."""
        def build():
            blocks, kqconv, (khead, qhead) = self.reduced_weights()

            def image(w, s, stride):
                return Conv3x3Pack(w.detach()).emu(16, True), s.detach().float().contiguous(), w.shape[0], stride
            one = torch.ones(1, dtype=torch.float32, device=kqconv[0].device)
            return [image(*blk) for blk in blocks], image(*kqconv), ops.pack_w2c_weights(khead, qhead), one
        return _cache_of(self, "_coalign_w2c_images").get(self, build)

    @staticmethod
    def _conv(x: "ops.SplitMap", layer) -> "ops.SplitMap":
        img, shift, cout, stride = layer
        if stride == 2:
            return ops.conv3x3_sp_s2(x, img, shift, cout, relu=True)
        return ops.conv3x3_sp(x, img, shift, cout, None, True, out_split=True)

    def forward_kernels(self, xx: torch.Tensor, groups: Sequence[int], normalized_affine_matrix: torch.Tensor, details: Optional[list] = None) -> torch.Tensor:
        blocks, kqconv, params, one = self.packed()
        if not ops.nhwc_memory(xx):
            xx = xx.contiguous(memory_format=torch.channels_last)      # (a stride-1 shrink header's conv3x3_sp writes channels-last: no copy there)
            if not ops.nhwc_memory(xx):                                 # (a 1 x 1 map or C = 1: every stride order counts as channels-last)
                xx = xx.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
        outs, off = [], 0
        for b, n in enumerate(groups):
            xb = xx[off:off + n]
            theta = normalized_affine_matrix[b, 0, :n].to(device=xx.device, dtype=torch.float64).contiguous()
            off += n
            if n == 1:                                                                       # (d)
                w = one
                if details is not None:
                    details.append((None, w))
            else:
                m = ops.v2v_warp_split(xb, theta[None])
                for layer in blocks:
                    m = self._conv(m, layer)
                key = self._conv(m, kqconv)                                                  # (c): [n, key | query, h, w]
                query = ops.SplitMap(key.data[:1, ops.W2C_CHANNELS // 16:])                  # the ego's query rows, read in place
                if details is not None:
                    w, logits = ops.w2c_score(key, query, params, return_logits=True)
                    details.append((logits, w))
                else:
                    w = ops.w2c_score(key, query, params)
            outs.append(ops.w2c_fuse(xb, theta, w))
        return outs[0] if len(outs) == 1 else torch.cat(outs, dim=0)

    def forward(self, x: torch.Tensor, record_len, normalized_affine_matrix: torch.Tensor, rows=None) -> torch.Tensor:
        if rows is not None:
            raise NotImplementedError("When2comFusion does not run agent-sharded (rows)")
        groups = host_ints(record_len)
        if x.is_cuda and x.dtype == torch.float32 and sum(groups) == x.shape[0] and self.kernel_route(x.shape[1], max(groups)):
            return self.forward_kernels(x, groups, normalized_affine_matrix)
        return self.forward_torch(x, groups, normalized_affine_matrix)
