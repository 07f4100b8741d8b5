"""V2X-ViT's fusion transformer, host side.

Class names, constructor keys and ``state_dict`` names follow the reference: ``V2XViTFusion`` (opencood/models/fuse_modules/fusion_in_one.py:295-352) owns
``fusion_net = V2XTransformer`` (opencood/models/sub_modules/v2xvit_basic.py:183-193) -> ``encoder = V2XTEncoder`` (:125-180) with ``STTF`` (:13-34), ``RTE`` (:37-81)
and ``depth`` x [``V2XFusionBlock`` (:84-122), ``PreNorm(FeedForward)`` (base_transformer.py:7-29)]; a fusion block is ``num_blocks`` x [``PreNorm(HGTCavAttention)``
(hmsa.py:7-151) or ``PreNorm(CavAttention)`` (base_transformer.py:32-80), ``PreNorm(PyramidWindowAttention)`` (mswin.py:83-121 over ``BaseWindowAttention`` :19-80 and
``SplitAttn``, split_attn.py:30-63)].  Parameters the forward never reads (``prior_feed``, the type-1 linears) exist because the reference's checkpoints hold them.

What fusion_in_one.py fixes for every call, and what follows from it:
  * ``prior_encoding`` is all zeros: every agent has type 0 and time delay 0.  The type-0 linears and relation 0 are indexed statically (no tensor-valued index, no
    host synchronisation), ``RTE`` adds ``lin(emb[0])``.
  * ``spatial_correction_matrix`` is the identity.  ``get_roi_and_cav_mask`` then returns exactly the agent mask at every map shape tried (recorded from the reference
    in tests/golden/v2xvit_fuse.npz); ``STTF`` however is NOT bit-identical to its input: its float32 chain of two 3 x 3 inversions leaves sampling positions a few
    1e-6 of a pixel off the grid, which changes the non-ego maps by up to 2e-5 of their scale.  Both are restated here (``STTF.positions`` -- data independent,
    computed once per map shape on the CPU as the reference's CPU run does, and cached); the resample is skipped only at a shape where the positions ARE the grid.

On the GPU in eval mode (``kernel_route``) the agent attention of every layer runs on ``ops.v2x_agent_attention``; the pyramid window attention, split attention
and feed-forward stay torch ops on the device (library kernels) -- unless ``window_kernels`` is set (off by default), which puts the pyramid window attention with
its split attention on ``ops.v2x_window_attention`` where ``window_kernel_reason`` allows it, and unless ``ffn_kernels`` is set (off by default too, independent of
the first), which puts ``x + FeedForward(LayerNorm(x))`` on ``ops.v2x_feed_forward`` where ``ffn_kernel_reason`` allows it.  With both set an encoder layer of the
kernel route is hand-written from end to end.
"""
from __future__ import annotations

import math
import os
from typing import List, Optional, Sequence

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import ops
from .backbone import LINEAR_LIBRARY, TORCH_MODE, _cache_of
from .encoder import host_ints

# Measurement switch: the pyramid window attention and split attention of the kernel route on ``ops.v2x_window_attention`` (csrc/v2x_window.hip) instead of torch
# ops.  Off by default; copied into ``V2XViTFusion.window_kernels`` at construction (tests and tools set the attribute).
V2X_WINDOW_KERNELS = os.environ.get("COALIGN_V2X_WINDOW", "0") != "0"
# Measurement switch: the feed-forward block of the kernel route on ``ops.v2x_feed_forward`` (csrc/v2x_ffn.hip) instead of torch ops.  Off by default; copied into
# ``V2XViTFusion.ffn_kernels`` at construction (tests and tools set the attribute).  Independent of the window switch.
V2X_FFN_KERNELS = os.environ.get("COALIGN_V2X_FFN", "0") != "0"


def _warp_torch(src: torch.Tensor, M: torch.Tensor) -> torch.Tensor:
    """warp_affine_simple (torch_transformation_utils.py:322-331) in torch ops, output size = input size."""
    grid = F.affine_grid(M, list(src.shape), align_corners=False).to(src)
    return F.grid_sample(src, grid, align_corners=False)


class PreNorm(nn.Module):
    def __init__(self, dim: int, fn: nn.Module):
        super().__init__()
        self.norm = nn.LayerNorm(dim)
        self.fn = fn

    def forward(self, x, **kwargs):
        return self.fn(self.norm(x), **kwargs)


class FeedForward(nn.Module):
    def __init__(self, dim: int, hidden_dim: int, dropout: float = 0.):
        super().__init__()
        self.net = nn.Sequential(nn.Linear(dim, hidden_dim), nn.GELU(), nn.Dropout(dropout), nn.Linear(hidden_dim, dim), nn.Dropout(dropout))

    def forward(self, x):
        return self.net(x)


def _heads(t: torch.Tensor, m: int) -> torch.Tensor:
    """(B, H, W, L, m c) -> (B, m, H, W, L, c)"""
    B, H, W, L, _ = t.shape
    return t.reshape(B, H, W, L, m, -1).permute(0, 4, 1, 2, 3, 5)


class CavAttention(nn.Module):
    """Vanilla agent attention (base_transformer.py:32-80), ``use_hetero: false``."""

    def __init__(self, dim: int, heads: int, dim_head: int = 64, dropout: float = 0.1):
        super().__init__()
        inner_dim = heads * dim_head
        self.heads = heads
        self.scale = dim_head ** -0.5
        self.attend = nn.Softmax(dim=-1)
        self.to_qkv = nn.Linear(dim, inner_dim * 3, bias=False)
        self.to_out = nn.Sequential(nn.Linear(inner_dim, dim), nn.Dropout(dropout))

    def forward(self, x, mask, prior_encoding=None):
        x = x.permute(0, 2, 3, 1, 4)                                        # (B, L, H, W, C) -> (B, H, W, L, C)
        mask = mask.unsqueeze(1)
        q, k, v = (_heads(t, self.heads) for t in self.to_qkv(x).chunk(3, dim=-1))
        att_map = torch.einsum("bmhwic,bmhwjc->bmhwij", q, k) * self.scale
        att_map = self.attend(att_map.masked_fill(mask == 0, -float("inf")))
        out = torch.einsum("bmhwij,bmhwjc->bmhwic", att_map, v)
        out = out.permute(0, 2, 3, 4, 1, 5).reshape(*x.shape[:4], -1)
        return self.to_out(out).permute(0, 3, 1, 2, 4)


class HGTCavAttention(nn.Module):
    """Heterogeneous agent attention (hmsa.py:7-151): per agent type its own q / k / v / output linears, per ordered pair of types a [dim_head, dim_head] matrix
    per head between query and key (``relation_att``) and on the value (``relation_msg``).  ``forward`` is the reference's arithmetic for agents of type 0."""

    def __init__(self, dim: int, heads: int, num_types: int = 2, num_relations: int = 4, dim_head: int = 64, dropout: float = 0.1):
        super().__init__()
        inner_dim = heads * dim_head
        self.heads, self.dim_head, self.num_types = heads, dim_head, num_types
        self.scale = dim_head ** -0.5
        self.attend = nn.Softmax(dim=-1)
        self.drop_out = nn.Dropout(dropout)
        self.k_linears, self.q_linears, self.v_linears, self.a_linears, self.norms = nn.ModuleList(), nn.ModuleList(), nn.ModuleList(), nn.ModuleList(), nn.ModuleList()
        for _ in range(num_types):
            self.k_linears.append(nn.Linear(dim, inner_dim))
            self.q_linears.append(nn.Linear(dim, inner_dim))
            self.v_linears.append(nn.Linear(dim, inner_dim))
            self.a_linears.append(nn.Linear(inner_dim, dim))
        self.relation_att = nn.Parameter(torch.empty(num_relations, heads, dim_head, dim_head))
        self.relation_msg = nn.Parameter(torch.empty(num_relations, heads, dim_head, dim_head))
        nn.init.xavier_uniform_(self.relation_att)
        nn.init.xavier_uniform_(self.relation_msg)

    def forward(self, x, mask, prior_encoding=None):
        x = x.permute(0, 2, 3, 1, 4)                                        # (B, L, H, W, C) -> (B, H, W, L, C)
        mask = mask.unsqueeze(1)                                             # (B, 1, 1 | H, 1 | W, 1, L): the keys
        q, k, v = (_heads(lin[0](x), self.heads) for lin in (self.q_linears, self.k_linears, self.v_linears))
        att_map = torch.einsum("bmhwip,mpq,bmhwjq->bmhwij", q, self.relation_att[0], k) * self.scale
        att_map = self.attend(att_map.masked_fill(mask == 0, -float("inf")))
        v_msg = torch.einsum("mpc,bmhwjp->bmhwjc", self.relation_msg[0], v)
        out = torch.einsum("bmhwij,bmhwjc->bmhwic", att_map, v_msg)
        out = out.permute(0, 2, 3, 4, 1, 5).reshape(*x.shape[:4], -1)
        return self.drop_out(self.a_linears[0](out)).permute(0, 3, 1, 2, 4)


def folded_agent_attention(norm: nn.LayerNorm, att: nn.Module, fold_norm: bool = True):
    """One PreNorm(agent attention) layer as ONE projection, folded in float64: -> (wqkv [3C, C], bqkv [3C], wa [C, C], ba [C]) in the parameters' dtype with
        [q | k' | v'] = wqkv y + bqkv,   att = softmax_j(q_i^m . k'_j^m),   out = wa concat_m(sum_j att_ij v'_j^m) + ba.
    Exact identities: ``relation_att[0]`` into the key rows (q^T A k = q^T (A k)), ``relation_msg[0]`` transposed into the value rows (sum_p M[p, c] v[p]), the scale
    into the query rows and bias.  ``fold_norm``: y = (x - mean) / sqrt(var + eps) and LayerNorm's gamma / beta are part of wqkv / bqkv; else y = LayerNorm(x)."""
    dt = norm.weight.dtype
    d = torch.float64
    if isinstance(att, HGTCavAttention):
        m, c = att.heads, att.dim_head
        wq, bq = att.q_linears[0].weight.to(d) * att.scale, att.q_linears[0].bias.to(d) * att.scale
        A, M = att.relation_att[0].to(d), att.relation_msg[0].to(d)
        wk = torch.einsum("mpq,mqk->mpk", A, att.k_linears[0].weight.to(d).view(m, c, -1)).reshape(m * c, -1)
        bk = torch.einsum("mpq,mq->mp", A, att.k_linears[0].bias.to(d).view(m, c)).reshape(-1)
        wv = torch.einsum("mpc,mpk->mck", M, att.v_linears[0].weight.to(d).view(m, c, -1)).reshape(m * c, -1)
        bv = torch.einsum("mpc,mp->mc", M, att.v_linears[0].bias.to(d).view(m, c)).reshape(-1)
        wa, ba = att.a_linears[0].weight.to(d), att.a_linears[0].bias.to(d)
    else:
        w = att.to_qkv.weight.to(d)
        inner = w.shape[0] // 3
        wq, wk, wv = w[:inner] * att.scale, w[inner:2 * inner], w[2 * inner:]
        bq = bk = bv = w.new_zeros(inner)
        wa, ba = att.to_out[0].weight.to(d), att.to_out[0].bias.to(d)
    wqkv, bqkv = torch.cat([wq, wk, wv]), torch.cat([bq, bk, bv])
    if fold_norm:
        bqkv = bqkv + wqkv @ norm.bias.to(d)
        wqkv = wqkv * norm.weight.to(d)[None, :]
    return wqkv.to(dt).contiguous(), bqkv.to(dt).contiguous(), wa.to(dt).contiguous(), ba.to(dt).contiguous()


def agent_attention_reduced(x: torch.Tensor, R: int, norm: nn.LayerNorm, att: nn.Module, fold_norm: bool = True) -> torch.Tensor:
    """x [N, H, W, C] (one frame's real agents) -> x[:R] + attention(LayerNorm(x))[:R] on the folded projection: the arithmetic of ``ops.v2x_agent_attention`` in
    torch ops (eval mode: no dropout)."""
    wqkv, bqkv, wa, ba = _cache_of(att, "_coalign_v2x_fold%d" % fold_norm).get(list(norm.parameters()) + list(att.parameters()), lambda: folded_agent_attention(norm, att, fold_norm))
    N, H, W, C = x.shape
    y = F.layer_norm(x, (C,), None, None, norm.eps) if fold_norm else norm(x)
    inner = wa.shape[1]
    m = att.heads
    q = (F.linear(y[:R], wqkv[:inner], bqkv[:inner])).reshape(R, H, W, m, -1)
    kv = F.linear(y, wqkv[inner:], bqkv[inner:]).reshape(N, H, W, 2, m, -1)
    p = torch.einsum("ihwmc,jhwmc->hwmij", q, kv[:, :, :, 0]).softmax(dim=-1)
    o = torch.einsum("hwmij,jhwmc->ihwmc", p, kv[:, :, :, 1]).reshape(R, H, W, inner)
    return x[:R] + F.linear(o, wa, ba)


def folded_window_attention(norm: nn.LayerNorm, pw: "PyramidWindowAttention"):
    """One PreNorm(PyramidWindowAttention) layer with ONE projection, folded in float64: -> (wqkv [3BC, C], bqkv [3BC], wout [B, C, C], bout [B, C], pos = the B position
    tables) in the parameters' dtype, B branches, with yhat = (x - mean) / sqrt(var + eps):
        [q_0 | k_0 | v_0 | q_1 | ...] = wqkv yhat + bqkv,   o_b = softmax_j(q_i . k_j + pos_b[xj - xi + ws - 1][yj - yi + ws - 1]) v_j,   out_b = wout_b o_b + bout_b.
    Exact identities: the bias-free ``to_qkv`` stacked, LayerNorm's gamma into the columns, beta as the bias W beta, each branch's scale into its query rows and bias."""
    dt, d = norm.weight.dtype, torch.float64
    ws, bs = [], []
    for att in pw.pwmsa:
        w = att.to_qkv.weight.to(d).clone()
        inner = w.shape[0] // 3
        w[:inner] *= att.scale
        bs.append(w @ norm.bias.to(d))
        ws.append(w * norm.weight.to(d)[None, :])
    wout = torch.stack([att.to_out[0].weight.to(d) for att in pw.pwmsa])
    bout = torch.stack([att.to_out[0].bias.to(d) for att in pw.pwmsa])
    return (torch.cat(ws).to(dt).contiguous(), torch.cat(bs).to(dt).contiguous(), wout.to(dt).contiguous(), bout.to(dt).contiguous(),
            [att.pos_embedding.detach().to(dt).contiguous() for att in pw.pwmsa])


def window_attention_reduced(x: torch.Tensor, norm: nn.LayerNorm, pw: "PyramidWindowAttention") -> torch.Tensor:
    """x [n, H, W, C] (one frame's maps) -> x + PyramidWindowAttention(LayerNorm(x)) on the folded projection, in the schedule of ``ops.v2x_window_attention`` in torch
    ops (eval mode: no dropout; any dtype, any device): one projection, the attention inside the windows with the position table indexed directly, the split
    attention's branch weights from the per-map channel means of the attention outputs (the pooled sum is linear in them), one weighted sum of the output projections."""
    if any(not att.relative_pos_embedding for att in pw.pwmsa) or pw.fuse_mehod not in ("naive", "split_attn"):
        raise NotImplementedError("window_attention_reduced: relative position tables, fusion_method naive or split_attn")
    wqkv, bqkv, wout, bout, pos = _cache_of(pw, "_coalign_v2x_window_fold").get(list(norm.parameters()) + list(pw.parameters()), lambda: folded_window_attention(norm, pw))
    n, H, W, C = x.shape
    qkv = F.linear(F.layer_norm(x, (C,), None, None, norm.eps), wqkv, bqkv)
    outs, off = [], 0
    for att, table in zip(pw.pwmsa, pos):
        ws, m = att.window_size, att.heads
        inner = att.to_out[0].in_features
        nh, nw = H // ws, W // ws
        q, k, v = (qkv[..., off + i * inner:off + (i + 1) * inner].reshape(n, nh, ws, nw, ws, m, -1).permute(0, 1, 3, 5, 2, 4, 6).reshape(n, nh, nw, m, ws * ws, -1) for i in range(3))
        off += 3 * inner
        r = torch.arange(ws, device=x.device)
        rows = (r[None, :] - r[:, None] + ws - 1)                                               # [i, j] -> j - i + ws - 1
        bias = table[rows[:, None, :, None], rows[None, :, None, :]].reshape(ws * ws, ws * ws)  # [(xi, yi), (xj, yj)]
        p = (torch.einsum("nhwmic,nhwmjc->nhwmij", q, k) + bias).softmax(dim=-1)
        o = torch.einsum("nhwmij,nhwmjc->nhwmic", p, v).reshape(n, nh, nw, m, ws, ws, -1).permute(0, 1, 4, 2, 5, 3, 6).reshape(n, H, W, inner)
        outs.append(o)
    B = len(outs)
    if pw.fuse_mehod == "naive":
        a = x.new_full((n, B, C), 1.0 / B)
    else:
        sa = pw.split_attn
        gap = sum(F.linear(o.mean(dim=(1, 2)), wout[b], bout[b]) for b, o in enumerate(outs))      # [n, C]
        a = sa.fc2(sa.act1(sa.bn1(sa.fc1(gap)))).reshape(n, B, -1).softmax(dim=1)
    return x + sum(a[:, b, None, None, :] * F.linear(o, wout[b], bout[b]) for b, o in enumerate(outs))


def folded_feed_forward(norm: nn.LayerNorm, ff: "FeedForward"):
    """One PreNorm(FeedForward) layer with LayerNorm folded into the first linear: -> (W1' [M, C], b1' [M], W2 [C, M], b2 [C]) in float64 with
        ff(LayerNorm(x)) = W2 GELU(W1' yhat + b1') + b2,   yhat = (x - mean) / sqrt(var + eps).
    Exact identities: gamma into the columns (W1' = W1 diag(gamma)), beta into the bias (b1' = W1 beta + b1)."""
    d = torch.float64
    w1, b1 = ff.net[0].weight.detach().to(d), ff.net[0].bias.detach().to(d)
    return ((w1 * norm.weight.detach().to(d)[None, :]).contiguous(), (w1 @ norm.bias.detach().to(d) + b1).contiguous(),
            ff.net[3].weight.detach().to(d).contiguous(), ff.net[3].bias.detach().to(d).contiguous())


def feed_forward_reduced(x: torch.Tensor, norm: nn.LayerNorm, ff: "FeedForward") -> torch.Tensor:
    """x [..., C] -> x + FeedForward(LayerNorm(x)) on the folded first linear: the arithmetic of ``ops.v2x_feed_forward`` in torch ops (eval mode: no dropout; any
    dtype, any device)."""
    w1, b1, w2, b2 = (t.to(x.dtype) for t in _cache_of(ff, "_coalign_v2x_ffn_fold").get(list(norm.parameters()) + list(ff.parameters()), lambda: folded_feed_forward(norm, ff)))
    yhat = F.layer_norm(x, (x.shape[-1],), None, None, norm.eps)
    return x + F.linear(F.gelu(F.linear(yhat, w1, b1)), w2, b2)


def get_relative_distances(window_size: int) -> torch.Tensor:
    idx = torch.tensor([[x, y] for x in range(window_size) for y in range(window_size)])
    return idx[None, :, :] - idx[:, None, :]


class BaseWindowAttention(nn.Module):
    """Attention inside non-overlapping ``window_size`` x ``window_size`` windows of every agent's map (mswin.py:19-80)."""

    def __init__(self, dim, heads, dim_head, drop_out, window_size, relative_pos_embedding):
        super().__init__()
        inner_dim = dim_head * heads
        self.heads = heads
        self.scale = dim_head ** -0.5
        self.window_size = window_size
        self.relative_pos_embedding = relative_pos_embedding
        self.to_qkv = nn.Linear(dim, inner_dim * 3, bias=False)
        if self.relative_pos_embedding:
            self.relative_indices = get_relative_distances(window_size) + window_size - 1      # a plain attribute, as in the reference
            self.pos_embedding = nn.Parameter(torch.randn(2 * window_size - 1, 2 * window_size - 1))
        else:
            self.pos_embedding = nn.Parameter(torch.randn(window_size ** 2, window_size ** 2))
        self.to_out = nn.Sequential(nn.Linear(inner_dim, dim), nn.Dropout(drop_out))

    def _flat_index(self, device) -> torch.Tensor:
        """``relative_indices`` as ONE flat index on ``device``, made once per device: indexing with the host tensor would copy it to the device in every call,
        which a graph capture refuses."""
        cache = self.__dict__.setdefault("_coalign_index", {})
        if device not in cache:
            ri = self.relative_indices
            cache[device] = (ri[:, :, 0] * (2 * self.window_size - 1) + ri[:, :, 1]).reshape(-1).to(device)
        return cache[device]

    def forward(self, x):
        b, l, h, w, c = x.shape
        m, ws = self.heads, self.window_size
        nh, nw = h // ws, w // ws

        def windows(t):      # b l (nh ws) (nw ws) (m c) -> b l m (nh nw) (ws ws) c
            return t.reshape(b, l, nh, ws, nw, ws, m, -1).permute(0, 1, 6, 2, 4, 3, 5, 7).reshape(b, l, m, nh * nw, ws * ws, -1)
        q, k, v = (windows(t) for t in self.to_qkv(x).chunk(3, dim=-1))
        dots = torch.einsum("blmhic,blmhjc->blmhij", q, k) * self.scale
        if self.relative_pos_embedding:
            dots = dots + self.pos_embedding.reshape(-1)[self._flat_index(x.device)].view(ws * ws, ws * ws)
        else:
            dots = dots + self.pos_embedding
        attn = dots.softmax(dim=-1)
        out = torch.einsum("blmhij,blmhjc->blmhic", attn, v)
        out = out.reshape(b, l, m, nh, nw, ws, ws, -1).permute(0, 1, 3, 5, 4, 6, 2, 7).reshape(b, l, h, w, -1)
        return self.to_out(out)


class RadixSoftmax(nn.Module):
    def __init__(self, radix: int, cardinality: int):
        super().__init__()
        self.radix, self.cardinality = radix, cardinality

    def forward(self, x):
        batch, cav_num = x.size(0), x.size(1)
        if self.radix > 1:
            x = F.softmax(x.view(batch, cav_num, self.cardinality, self.radix, -1), dim=3)
            return x.reshape(batch, -1)
        return torch.sigmoid(x)


class SplitAttn(nn.Module):
    """Channel-wise softmax over the three window sizes, from the globally pooled sum (split_attn.py:30-63)."""

    def __init__(self, input_dim: int):
        super().__init__()
        self.input_dim = input_dim
        self.fc1 = nn.Linear(input_dim, input_dim, bias=False)
        self.bn1 = nn.LayerNorm(input_dim)
        self.act1 = nn.ReLU()
        self.fc2 = nn.Linear(input_dim, input_dim * 3, bias=False)
        self.rsoftmax = RadixSoftmax(3, 1)

    def forward(self, window_list):
        assert len(window_list) == 3, "only 3 windows are supported"
        sw, mw, bw = window_list
        B, L = sw.shape[0], sw.shape[1]
        x_gap = (sw + mw + bw).mean((2, 3), keepdim=True)
        x_attn = self.rsoftmax(self.fc2(self.act1(self.bn1(self.fc1(x_gap))))).view(B, L, 1, 1, -1)
        d = self.input_dim
        return sw * x_attn[..., 0:d] + mw * x_attn[..., d:2 * d] + bw * x_attn[..., 2 * d:]


class PyramidWindowAttention(nn.Module):
    def __init__(self, dim, heads, dim_heads, drop_out, window_size, relative_pos_embedding, fuse_method="naive"):
        super().__init__()
        assert isinstance(window_size, list) and isinstance(heads, list) and isinstance(dim_heads, list) and len(dim_heads) == len(heads)
        self.pwmsa = nn.ModuleList([BaseWindowAttention(dim, head, dim_head, drop_out, ws, relative_pos_embedding)
                                    for head, dim_head, ws in zip(heads, dim_heads, window_size)])
        self.fuse_mehod = fuse_method      # (the reference's spelling)
        if fuse_method == "split_attn":
            self.split_attn = SplitAttn(256)
        elif fuse_method == "split_attn128":
            self.split_attn = SplitAttn(128)

    def forward(self, x):
        if self.fuse_mehod == "naive":
            output = None
            for wmsa in self.pwmsa:
                output = wmsa(x) if output is None else output + wmsa(x)
            return output / len(self.pwmsa)
        if self.fuse_mehod == "split_attn":
            return self.split_attn([wmsa(x) for wmsa in self.pwmsa])
        raise NotImplementedError(f"PyramidWindowAttention: fusion_method '{self.fuse_mehod}' returns nothing in the reference")


class STTF(nn.Module):
    """The spatial-temporal correction (v2xvit_basic.py:13-34) for the identity ``spatial_correction_matrix`` fusion_in_one.py always passes: every non-ego map is
    resampled bilinearly (zero padding, align_corners=True) at positions the reference derives in float32 -- get_discretized_transformation_matrix,
    get_transformation_matrix and warp_affine's normalize_homography with its two 3 x 3 inversions (torch_transformation_utils.py:110-373).  In exact arithmetic they
    are the pixel centres; in float32 they are not."""

    def __init__(self, args: dict):
        super().__init__()
        self.discrete_ratio = args["voxel_size"][0]
        self.downsample_rate = args["downsample_rate"]

    def positions(self, H: int, W: int):
        """-> (grid [1, H, W, 2] float32 on the CPU, is_identity, roi_is_ones), cached per map shape.  ``is_identity``: every sampling position is its own pixel
        centre bit for bit (the resample then returns its input); ``roi_is_ones``: the nearest-neighbour warp of a map of ones at these positions
        (get_rotated_roi) is all ones, i.e. ``get_roi_and_cav_mask`` is the agent mask."""
        cache = self.__dict__.setdefault("_coalign_positions", {})
        if (H, W) not in cache:
            with torch.no_grad():
                M = torch.eye(4)[None, [0, 1], :][:, :, [0, 1, 3]]
                M[:, :, -1] = M[:, :, -1] / (self.discrete_ratio * self.downsample_rate)
                M = M.float()
                eye = torch.eye(3)[None]
                shift, shift_inv, rot = eye.clone(), eye.clone(), eye.clone()
                center = torch.tensor([W / 2, H / 2])
                shift[:, :2, 2], shift_inv[:, :2, 2] = center, -center
                rot[:, :2, :2] = M[:, :2, :2]
                T = (shift @ rot @ shift_inv)[:, :2, :]
                T[..., 2] += M[..., 2]
                M3 = F.pad(T, [0, 0, 0, 1], "constant", value=0.0)
                M3[..., -1, -1] += 1.0
                norm = torch.tensor([[1.0, 0.0, -1.0], [0.0, 1.0, -1.0], [0.0, 0.0, 1.0]])
                norm[0, 0] = norm[0, 0] * 2.0 / (1e-14 if W == 1 else W - 1.0)
                norm[1, 1] = norm[1, 1] * 2.0 / (1e-14 if H == 1 else H - 1.0)
                norm = norm[None]
                dst_norm_trans_src_norm = norm @ (M3 @ torch.inverse(norm))
                theta = torch.inverse(dst_norm_trans_src_norm)[:, :2, :]
                grid = F.affine_grid(theta, [1, 1, H, W], align_corners=True)
                ix, iy = (grid[0, ..., 0] + 1) / 2 * (W - 1), (grid[0, ..., 1] + 1) / 2 * (H - 1)      # grid_sample's pixel coordinates, its float32 arithmetic
                ident = bool(torch.equal(ix, torch.arange(W).float()[None, :].expand(H, W)) and torch.equal(iy, torch.arange(H).float()[:, None].expand(H, W)))
                roi = F.grid_sample(torch.ones(1, 1, H, W), grid, mode="nearest", padding_mode="zeros", align_corners=True)
                cache[(H, W)] = (grid, ident, bool((roi == 1).all()), roi[0, 0])
        return cache[(H, W)]

    def _grid_on(self, H: int, W: int, device, dtype) -> torch.Tensor:
        cache = self.__dict__.setdefault("_coalign_grids", {})
        key = (H, W, device, dtype)
        if key not in cache:
            cache[key] = self.positions(H, W)[0].to(device=device, dtype=dtype)
        return cache[key]

    def resample(self, x: torch.Tensor) -> torch.Tensor:
        """x [N, C, H, W] -> every map resampled at the cached positions (the caller leaves the ego out)."""
        N, _, H, W = x.shape
        if N == 0 or self.positions(H, W)[1]:
            return x
        return F.grid_sample(x, self._grid_on(H, W, x.device, x.dtype).expand(N, -1, -1, -1), mode="bilinear", padding_mode="zeros", align_corners=True)

    def roi_mask(self, H: int, W: int, device, dtype) -> Optional[torch.Tensor]:
        """None when the ROI mask is all ones, else the [H, W] mask on ``device``."""
        _, _, ones, roi = self.positions(H, W)
        return None if ones else roi.to(device=device, dtype=dtype)

    def forward(self, x, mask=None, spatial_correction_matrix=None):
        """x (B, L, H, W, C): agents 1 .. L - 1 resampled, the ego as it is."""
        B, L, H, W, C = x.shape
        cav = self.resample(x[:, 1:].permute(0, 1, 4, 2, 3).reshape(-1, C, H, W)).reshape(B, L - 1, C, H, W).permute(0, 1, 3, 4, 2)
        return torch.cat([x[:, :1], cav], dim=1)


class RelTemporalEncoding(nn.Module):
    def __init__(self, n_hid: int, RTE_ratio, max_len: int = 100, dropout: float = 0.2):
        super().__init__()
        position = torch.arange(0., max_len).unsqueeze(1)
        div_term = torch.exp(torch.arange(0, n_hid, 2) * -(math.log(10000.0) / n_hid))
        emb = nn.Embedding(max_len, n_hid)
        emb.weight.data[:, 0::2] = torch.sin(position * div_term) / math.sqrt(n_hid)
        emb.weight.data[:, 1::2] = torch.cos(position * div_term) / math.sqrt(n_hid)
        emb.requires_grad = False
        self.RTE_ratio = RTE_ratio
        self.emb = emb
        self.lin = nn.Linear(n_hid, n_hid)

    def forward(self, x, t=0):
        """Time delay 0 (all this path ever sees): row 0 of the table, whatever the ratio."""
        return x + self.lin(self.emb.weight[0])


class RTE(nn.Module):
    def __init__(self, dim: int, RTE_ratio=2):
        super().__init__()
        self.RTE_ratio = RTE_ratio
        self.emb = RelTemporalEncoding(dim, RTE_ratio=self.RTE_ratio)

    def forward(self, x, dts=None):
        return self.emb(x)


class V2XFusionBlock(nn.Module):
    def __init__(self, num_blocks: int, cav_att_config: dict, pwindow_config: dict):
        super().__init__()
        self.layers = nn.ModuleList([])
        self.num_blocks = num_blocks
        c, p = cav_att_config, pwindow_config
        for _ in range(num_blocks):
            att = (HGTCavAttention(c["dim"], heads=c["heads"], dim_head=c["dim_head"], dropout=c["dropout"]) if c["use_hetero"] else
                   CavAttention(c["dim"], heads=c["heads"], dim_head=c["dim_head"], dropout=c["dropout"]))
            self.layers.append(nn.ModuleList([
                PreNorm(c["dim"], att),
                PreNorm(c["dim"], PyramidWindowAttention(p["dim"], heads=p["heads"], dim_heads=p["dim_head"], drop_out=p["dropout"], window_size=p["window_size"],
                                                         relative_pos_embedding=p["relative_pos_embedding"], fuse_method=p["fusion_method"]))]))

    def forward(self, x, mask, prior_encoding=None):
        for cav_attn, pwindow_attn in self.layers:
            x = cav_attn(x, mask=mask, prior_encoding=prior_encoding) + x
            x = pwindow_attn(x) + x
        return x


class V2XTEncoder(nn.Module):
    def __init__(self, args: dict):
        super().__init__()
        cav_att_config, pwindow_att_config, feed_config = args["cav_att_config"], args["pwindow_att_config"], args["feed_forward"]
        self.downsample_rate = args["sttf"]["downsample_rate"]
        self.discrete_ratio = args["sttf"]["voxel_size"][0]
        self.use_roi_mask = args["use_roi_mask"]
        self.use_RTE = cav_att_config["use_RTE"]
        self.RTE_ratio = cav_att_config["RTE_ratio"]
        self.sttf = STTF(args["sttf"])
        self.prior_feed = nn.Linear(cav_att_config["dim"] + 3, cav_att_config["dim"])      # (never read by the reference's forward either)
        self.layers = nn.ModuleList([])
        if self.use_RTE:
            self.rte = RTE(cav_att_config["dim"], self.RTE_ratio)
        for _ in range(args["depth"]):
            self.layers.append(nn.ModuleList([V2XFusionBlock(args["num_blocks"], cav_att_config, pwindow_att_config),
                                              PreNorm(cav_att_config["dim"], FeedForward(cav_att_config["dim"], feed_config["mlp_dim"], dropout=feed_config["dropout"]))]))

    def com_mask(self, mask: torch.Tensor, H: int, W: int, dtype) -> torch.Tensor:
        """The keys' mask: (B, 1, 1, 1, L), or with an ROI mask that is not all ones (B, H, W, 1, L) = roi x agent mask (get_roi_and_cav_mask)."""
        roi = self.sttf.roi_mask(H, W, mask.device, dtype) if self.use_roi_mask else None
        if roi is None:
            return mask[:, None, None, None, :]
        return roi[None, :, :, None, None] * mask.to(dtype)[:, None, None, None, :]

    def forward(self, x, mask, spatial_correction_matrix=None):
        """x (B, L, H, W, C) the warped maps (the reference's three zero prior channels are not carried), mask (B, L)."""
        if self.use_RTE:
            x = self.rte(x)
        x = self.sttf(x)
        com_mask = self.com_mask(mask, x.shape[2], x.shape[3], x.dtype)
        for attn, ff in self.layers:
            x = attn(x, mask=com_mask)
            x = ff(x) + x
        return x


class V2XTransformer(nn.Module):
    def __init__(self, args: dict):
        super().__init__()
        self.encoder = V2XTEncoder(args["encoder"])

    def forward(self, x, mask, spatial_correction_matrix=None):
        return self.encoder(x, mask, spatial_correction_matrix)[:, 0]


class V2XViTFusion(nn.Module):
    """V2X-ViT's fusion (fusion_in_one.py:295-352): the agents' maps padded to L and warped into the ego frame, ``depth`` encoder layers of agent attention, pyramid
    window attention and feed-forward (all pre-norm, all residual), the ego's tokens of the last layer returned.

    ``forward_torch`` states that op by op (CPU, training, any shape).  ``forward_reduced`` is the kernel route's schedule in torch ops and rests on exact identities:
      1. Padded agents are masked as keys and every other block acts per agent: a frame's N real agents suffice (no padding to L).
      2. The output is agent 0 of the last layer: its agent attention needs queries and output for the ego alone (R = 1), its window attention and feed-forward
         run on the ego alone.
      3. With one agent type ``relation_att[0]`` folds into the key projection, ``relation_msg[0]`` (transposed) into the value projection and ``dim_head^-0.5``
         into the query projection, biases included (``folded_agent_attention``, float64, cached until a parameter changes).
      4. LayerNorm's gamma / beta fold into the same projection (``fold_norm``).
    It needs the ROI mask to be all ones at the map's shape (it is at every shape recorded from the reference) and eval mode (no dropout); else ``forward_torch`` runs.

    On the GPU in eval mode (``kernel_route``) the agent attention of every layer is ``ops.v2x_agent_attention``; the first layer reads the unwarped maps with
    ``theta`` where ``STTF`` is the identity at the map's shape and there is no RTE, else the maps are warped by ``ops.warp_fuse_nhwc`` and resampled first."""

    def __init__(self, args: dict):
        super().__init__()
        self.fusion_net = V2XTransformer(args["transformer"])
        self.force_torch = False      # measurement / test aid: take the op-by-op route whatever the device
        self.window_kernels = V2X_WINDOW_KERNELS      # the kernel route's window attention on ops.v2x_window_attention (off by default)
        self.ffn_kernels = V2X_FFN_KERNELS            # the kernel route's feed-forward on ops.v2x_feed_forward (off by default)

    # ---- the decision --------------------------------------------------------------------------------------------------------------------------------------
    def _attentions(self):
        return [blk[0].fn for layer in self.fusion_net.encoder.layers for blk in layer[0].layers]

    def kernel_shape_reason(self, channels: int, n_agents: int = 1) -> Optional[str]:
        """None when ``ops.v2x_agent_attention`` takes every agent-attention layer at ``channels``; else why not."""
        for att in self._attentions():
            if not isinstance(att, HGTCavAttention):
                return "use_hetero: false (CavAttention has no kernel)"
            if not ops.v2x_attn_shape_ok(channels, att.heads, att.dim_head, n_agents):
                return f"dim {channels} = {att.heads} heads x {att.dim_head} outside the kernel's 8 x 32 | 2 x 32, or more than 8 agents"
            if att.q_linears[0].in_features != channels:
                return f"the map's {channels} channels are not the transformer's dim {att.q_linears[0].in_features}"
        return None

    def kernel_weight_reason(self) -> Optional[str]:
        """None when every agent-attention layer packs (``packed``); else why not.  Asked after ``kernel_shape_reason``: the packer takes the kernel's shapes only."""
        if self.packed() is None:
            return "a folded agent-attention weight, or the static bound of an attention output, lies outside the fp16 range"
        return None

    def _windows(self):
        return [blk[1].fn for layer in self.fusion_net.encoder.layers for blk in layer[0].layers]

    def window_kernel_reason(self, channels: int, hw=None) -> Optional[str]:
        """None when ``ops.v2x_window_attention`` takes every pyramid window attention of the kernel route at ``channels`` (and the map shape ``hw``, when given);
        else why not."""
        if not self.window_kernels:
            return "the window kernels are switched off (COALIGN_V2X_WINDOW / window_kernels)"
        for pw in self._windows():
            if pw.fuse_mehod not in ops.V2X_WINDOW_FUSE:
                return f"fusion_method {pw.fuse_mehod} has no kernel"
            if any(not att.relative_pos_embedding for att in pw.pwmsa):
                return "relative_pos_embedding: false has no kernel"
            heads, dim_heads, windows = [att.heads for att in pw.pwmsa], [att.to_out[0].in_features // att.heads for att in pw.pwmsa], [att.window_size for att in pw.pwmsa]
            if pw.pwmsa[0].to_qkv.in_features != channels or not ops.v2x_window_shape_ok(channels, heads, dim_heads, windows, pw.fuse_mehod, True):
                return (f"windows {windows} x heads {heads} x dim_head {dim_heads} on {channels} channels ({pw.fuse_mehod}) outside the kernel's 4 / 8 / 16 windows of "
                        f"16 / 32 / 64 channels a head on 256 channels (64: naive only)")
        if hw is not None and (int(hw[0]) % 16 or int(hw[1]) % 16):
            return f"a {int(hw[0])} x {int(hw[1])} map: H and W must be multiples of 16"
        if self.packed_windows() is None:
            return "a folded window-attention weight, or the static bound of an attention output, lies outside the fp16 range"
        return None

    def _feed_forwards(self):
        return [layer[1] for layer in self.fusion_net.encoder.layers]

    def ffn_kernel_reason(self, channels: int) -> Optional[str]:
        """None when ``ops.v2x_feed_forward`` takes every feed-forward block of the kernel route at ``channels``; else why not."""
        if not self.ffn_kernels:
            return "the feed-forward kernel is switched off (COALIGN_V2X_FFN / ffn_kernels)"
        for ff in self._feed_forwards():
            lin1, lin2 = ff.fn.net[0], ff.fn.net[3]
            if lin1.in_features != channels or lin2.out_features != channels or not ops.v2x_ffn_shape_ok(channels, lin1.out_features):
                return (f"feed-forward {lin1.in_features} -> {lin1.out_features} -> {lin2.out_features} on {channels} channels outside the kernel's 64 | 256 channels "
                        f"with mlp_dim a multiple of 32 in 32 .. {ops.V2X_FFN_MAX_HIDDEN}")
        if self.packed_ffn() is None:
            return "a folded feed-forward weight, or the static bound of a hidden pre-activation, lies outside the fp16 range"
        return None

    def kernel_route(self, channels: int, n_agents: int = 1, hw=None) -> bool:
        """The static half of the decision (``routes.plan`` asks it): eval mode, hetero attention of 8 or 2 heads of 32 on ``channels``, at most 8 agents, and -- when
        the map's shape ``hw`` is given -- an ROI mask that is all ones there.  ``forward`` adds: a CUDA float32 map, packable weights."""
        if self.training or self.force_torch or self.kernel_shape_reason(channels, n_agents) is not None:
            return False
        enc = self.fusion_net.encoder
        return bool(hw is None or not enc.use_roi_mask or enc.sttf.positions(int(hw[0]), int(hw[1]))[2])

    KERNELS = ("v2x_agent_attention per encoder layer: LayerNorm + folded q | k' | v' projection + softmax over the agents + output projection + residual in two launches; "
               "pyramid window attention, split attention and feed-forward as torch ops on the device (library kernels)")
    KERNELS_WINDOW = ("v2x_agent_attention + v2x_window_attention per encoder layer: the agent attention in two launches, the pyramid window attention with its split attention "
                      "(LayerNorm + folded 9C x C projection, attention inside the 4 / 8 / 16 windows, branch weights, output projections + residual) in three or four; "
                      "the feed-forward is still torch ops on the device (library kernels)")
    KERNELS_FFN = ("v2x_agent_attention + v2x_feed_forward per encoder layer: the agent attention in two launches, the feed-forward (LayerNorm + folded first linear, GELU, "
                   "second linear + residual) in one; pyramid window attention and split attention as torch ops on the device (library kernels)")
    KERNELS_WINDOW_FFN = ("v2x_agent_attention + v2x_window_attention + v2x_feed_forward per encoder layer: the agent attention in two launches, the pyramid window attention with "
                          "its split attention (LayerNorm + folded 9C x C projection, attention inside the 4 / 8 / 16 windows, branch weights, output projections + residual) in "
                          "three or four, the feed-forward (LayerNorm + folded first linear, GELU, second linear + residual) in one")
    TORCH = "V2XViTFusion op by op in PyTorch"
    FFN = "v2x_feed_forward"
    ATT, WIN, UNREAD = "v2x_agent_attention", "v2x_window_attention", "never read (every agent is of type 0; prior_feed has no caller)"

    def plan_fusion(self, channels: int, terms: Optional[int] = None):
        """-> (``routes.plan``'s fusion line, whether it is a fallback, {layers noted with it: (line, fallback)})."""
        if self.kernel_route(channels) and self.kernel_weight_reason() is not None:
            return f"{self.TORCH} ({self.kernel_weight_reason()})", True, {}
        if self.kernel_route(channels):
            window = self.window_kernel_reason(channels) is None
            if self.ffn_kernel_reason(channels) is None:
                return (self.KERNELS_WINDOW_FFN if window else self.KERNELS_FFN), False, {}
            return (self.KERNELS_WINDOW if window else self.KERNELS), False, {}
        return f"{self.TORCH} ({self.kernel_shape_reason(channels) or TORCH_MODE})", True, {}

    def plan_layer(self, name: str, layer: nn.Module, channels: int, terms: Optional[int] = None):
        """-> (line, fallback) of one of the transformer's linears."""
        if not isinstance(layer, nn.Linear):
            return None
        ok, leaf = self.kernel_route(channels) and self.kernel_weight_reason() is None, name.split(".")
        typed = leaf[-2] in ("q_linears", "k_linears", "v_linears", "a_linears")
        if name.endswith("prior_feed") or (typed and leaf[-1] != "0"):
            return self.UNREAD, False
        if typed:
            part = "output projection" if leaf[-2] == "a_linears" else "one third of the folded q | k' | v' projection"
            return (f"{self.ATT} ({part}, fp16 x 2 on the matrix cores)" if ok else LINEAR_LIBRARY + ", V2XViTFusion op by op)"), not ok
        if ok and (".pwmsa." in name or ".split_attn." in name) and self.window_kernel_reason(channels) is None:
            part = ("one third of the folded 9C x C projection, fp16 x 2 on the matrix cores" if leaf[-1] == "to_qkv" else "output projection, fp16 x 2 on the matrix cores"
                    if ".to_out." in name else "split attention's branch weights, fp32")
            return f"{self.WIN} ({part})", False
        if ok and ".net." in name and self.ffn_kernel_reason(channels) is None:
            part = "first linear with LayerNorm folded in, GELU" if leaf[-1] == "0" else "second linear + residual"
            return f"{self.FFN} ({part}, fp16 x 2 on the matrix cores)", False
        block = "pyramid window attention" if ".pwmsa." in name else "split attention" if ".split_attn." in name else "feed-forward" if ".net." in name else "agent attention" if ".to_" in name else "time encoding"
        return LINEAR_LIBRARY + f", {block}: torch op on the device)", True

    # ---- the reference's forward, op by op -----------------------------------------------------------------------------------------------------------------
    def forward_torch(self, x: torch.Tensor, record_len, normalized_affine_matrix: torch.Tensor) -> torch.Tensor:
        _, C, H, W = x.shape
        groups = host_ints(record_len)
        B, L = normalized_affine_matrix.shape[:2]
        feats, off = [], 0
        for b, n in enumerate(groups):
            padded = torch.cat([x[off:off + n], x.new_zeros(L - n, C, H, W)], dim=0)                                     # fuse_utils.regroup
            feats.append(_warp_torch(padded, normalized_affine_matrix[b, 0]))
            off += n
        mask = torch.tensor([[1] * n + [0] * (L - n) for n in groups], device=x.device)
        fused = self.fusion_net(torch.stack(feats).permute(0, 1, 3, 4, 2), mask)
        return fused.permute(0, 3, 1, 2)

    # ---- the identities, in the kernel route's schedule ------------------------------------------------------------------------------------------------------
    def _schedule(self, N: int):
        """[(norm, attention, R, window PreNorm, feed-forward PreNorm or None)] of every fusion block in order: R = N but for the very last block."""
        enc = self.fusion_net.encoder
        steps = []
        for d, (block, ff) in enumerate(enc.layers):
            for k, (cav, pw) in enumerate(block.layers):
                last = d + 1 == len(enc.layers) and k + 1 == len(block.layers)
                steps.append((cav.norm, cav.fn, 1 if last else N, pw, ff if k + 1 == len(block.layers) else None))
        return steps

    def forward_reduced(self, x: torch.Tensor, record_len, normalized_affine_matrix: torch.Tensor, fold_norm: bool = True) -> torch.Tensor:
        _, C, H, W = x.shape
        groups = host_ints(record_len)
        enc = self.fusion_net.encoder
        if self.training or (enc.use_roi_mask and not enc.sttf.positions(H, W)[2]):
            return self.forward_torch(x, groups, normalized_affine_matrix)
        outs, off = [], 0
        for b, N in enumerate(groups):
            xb = _warp_torch(x[off:off + N], normalized_affine_matrix[b, 0, :N])
            off += N
            if enc.use_RTE:
                xb = enc.rte(xb.permute(0, 2, 3, 1)).permute(0, 3, 1, 2)
            xb = torch.cat([xb[:1], enc.sttf.resample(xb[1:])], dim=0).permute(0, 2, 3, 1)                                 # [N, H, W, C]
            for norm, att, R, pw, ff in self._schedule(N):
                xb = agent_attention_reduced(xb, R, norm, att, fold_norm)
                xb = xb + pw(xb.unsqueeze(0)).squeeze(0)
                if ff is not None:
                    xb = xb + ff(xb)
            outs.append(xb[:1])
        return torch.cat(outs, dim=0).permute(0, 3, 1, 2)

    # ---- the kernel route --------------------------------------------------------------------------------------------------------------------------------------
    def packed(self) -> Optional[List[torch.Tensor]]:
        """The parameter image of every agent-attention layer (``ops.pack_v2x_weights`` of ``folded_agent_attention``), cached until a parameter changes; None when a
        folded weight or the static bound of an attention output lies outside the fp16 range."""
        def build():
            imgs = [ops.pack_v2x_weights(*folded_agent_attention(norm, att, True)) for norm, att, _, _, _ in self._schedule(1)]
            return (None if any(i is None for i in imgs) else imgs,)
        return _cache_of(self, "_coalign_v2x_images").get(self, build)[0]

    def packed_windows(self) -> Optional[List[torch.Tensor]]:
        """The parameter image of every window-attention layer (``ops.pack_v2x_window_weights`` of ``folded_window_attention``), cached until a parameter changes; None
        when a folded weight or the static bound of an attention output lies outside the fp16 range."""
        def build():
            imgs = []
            for _, _, _, pw, _ in self._schedule(1):
                sa = pw.fn.split_attn if pw.fn.fuse_mehod == "split_attn" else None
                imgs.append(ops.pack_v2x_window_weights(*folded_window_attention(pw.norm, pw.fn), split=None if sa is None else (sa.fc1.weight, sa.bn1.weight, sa.bn1.bias, sa.fc2.weight)))
            return (None if any(i is None for i in imgs) else imgs,)
        return _cache_of(self, "_coalign_v2x_window_images").get(self, build)[0]

    def packed_ffn(self) -> Optional[List[torch.Tensor]]:
        """The parameter image of every feed-forward block (``ops.pack_v2x_ffn_weights`` of ``folded_feed_forward``), one per encoder layer, cached until a parameter
        changes; None when a folded weight or the static bound of a hidden pre-activation lies outside the fp16 range."""
        def build():
            imgs = [ops.pack_v2x_ffn_weights(*folded_feed_forward(ff.norm, ff.fn)) for ff in self._feed_forwards()]
            return (None if any(i is None for i in imgs) else imgs,)
        return _cache_of(self, "_coalign_v2x_ffn_images").get([p for ff in self._feed_forwards() for p in ff.parameters()], build)[0]

    def forward_kernels(self, xx: torch.Tensor, groups: Sequence[int], normalized_affine_matrix: torch.Tensor, images: List[torch.Tensor]) -> torch.Tensor:
        enc = self.fusion_net.encoder
        _, C, H, W = xx.shape
        in_place = bool(not enc.use_RTE and enc.sttf.positions(H, W)[1])      # the first layer can warp inside the kernel
        if not ops.nhwc_memory(xx):
            xx = xx.contiguous(memory_format=torch.channels_last)             # (the shrink header's conv3x3_sp writes channels-last: no copy on the detector's route)
            if not ops.nhwc_memory(xx):
                xx = xx.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
        wimages = self.packed_windows() if self.window_kernel_reason(C, (H, W)) is None else None      # (one decision per call)
        fimages = {id(ff): img for ff, img in zip(self._feed_forwards(), self.packed_ffn())} if self.ffn_kernel_reason(C) is None else None
        outs, off = [], 0
        for b, n in enumerate(groups):
            xb = xx[off:off + n]
            theta = normalized_affine_matrix[b, 0, :n].to(device=xx.device, dtype=torch.float64).contiguous()
            off += n
            if in_place:
                xb, th = xb.permute(0, 2, 3, 1), theta
            else:
                xb = ops.warp_fuse_nhwc([xb], theta, ops.FUSE_NONE)[0] if ops.warp_fuse_nhwc_ok(xb) else _warp_torch(xb, theta.to(xb.dtype))
                if enc.use_RTE:
                    xb = enc.rte(xb.permute(0, 2, 3, 1)).permute(0, 3, 1, 2)
                xb, th = torch.cat([xb[:1], enc.sttf.resample(xb[1:])], dim=0).permute(0, 2, 3, 1).contiguous(), None
            for k, (img, (norm, att, R, pw, ff)) in enumerate(zip(images, self._schedule(n))):
                xb = ops.v2x_agent_attention(xb.contiguous(), th, img, receivers=R)
                th = None
                if wimages is not None:
                    xb = ops.v2x_window_attention(xb, wimages[k], pw.fn.fuse_mehod)
                else:
                    xb = xb + pw(xb.unsqueeze(0)).squeeze(0)
                if ff is not None:
                    xb = ops.v2x_feed_forward(xb.contiguous(), fimages[id(ff)]) if fimages is not None else xb + ff(xb)
            outs.append(xb[:1])
        out = outs[0] if len(outs) == 1 else torch.cat(outs, dim=0)
        return out.permute(0, 3, 1, 2)                                        # [B, C, H, W] in channels-last memory

    def forward(self, x: torch.Tensor, record_len, normalized_affine_matrix: torch.Tensor, rows=None) -> torch.Tensor:
        if rows is not None:
            raise NotImplementedError("V2XViTFusion does not run agent-sharded (rows)")
        groups = host_ints(record_len)
        if x.is_cuda and x.dtype == torch.float32 and sum(groups) == x.shape[0] and self.kernel_route(x.shape[1], max(groups), x.shape[2:]):
            images = self.packed()
            if images is not None:
                return self.forward_kernels(x, groups, normalized_affine_matrix, images)
        return self.forward_torch(x, groups, normalized_affine_matrix)
