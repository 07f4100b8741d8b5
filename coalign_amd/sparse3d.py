"""The sparse 3-D trunk of the SECOND detectors: ``MeanVFE`` -> ``VoxelBackBone8x`` -> ``HeightCompression`` (opencood/models/sub_modules/mean_vfe.py,
sparse_backbone_3d.py, height_compression.py), with spconv's ``SubMConv3d`` / ``SparseConv3d`` RESTATED -- spconv is not a dependency.

Semantics (spconv's, with the one thing it leaves open defined).  A sparse tensor is features [M, C] + indices [M, 4] int32 = (batch, z, y, x), unique + a spatial
shape (D, H, W) + a batch size.  ``SubMConv3d(Cin, Cout, 3)`` keeps the sites and their row order; ``SparseConv3d`` produces the sites some input reaches, rows
ASCENDING in the linear cell index ((b D' + z) H' + y) W' + x (spconv leaves the order to its hash table).  Taps are added in ascending (kz, ky, kx) order; only
active neighbours inside the grid and of the same batch item contribute.  A row whose coordinates lie outside the grid is ignored: it is nobody's neighbour, makes no
output site, is absent from ``dense()``, and a submanifold layer answers it with a zero row.

Every layer of the backbone is ``SparseSequential(conv, BatchNorm1d(eps 1e-3), ReLU)`` and has two routes:

* the torch-op route (any device, any float dtype, training too): sorted keys + ``searchsorted`` per tap, gather, ``matmul``; batch norm and ReLU on the active rows;
* the kernel route (``coalign_amd.ops.sp3d_*``, csrc/sparse_conv3d.hip): eval mode, CUDA float32, one of VoxelBackBone8x's (Cin, Cout, kernel) combinations.  Site
  counts stay on the device: no host read-back between the voxel tensors and the dense map, so the trunk can be captured in a graph.

``COALIGN_SP3D=0`` keeps the torch-op route on the GPU, ``COALIGN_SP3D=1`` asks for the kernel route; unset, ``KERNEL_DEFAULT`` decides (DESIGN.md section 8n has the
measurement behind it).  ``kernel_reason`` words why a layer does not take the kernel route; ``plan`` words every layer of a config without a GPU.
"""
from __future__ import annotations

import os
from typing import Optional, Sequence, Tuple

import numpy as np
import torch
import torch.nn as nn

from . import ops
from .backbone import _cache_of

KERNEL_DEFAULT = True          # the kernel route on the GPU when COALIGN_SP3D is unset: 1.69 ms against 105 ms for the torch-op route at the OPV2V grid, 5 agents
KERNEL_TEXT = "coalign_sp3d_conv"
TORCH_TEXT = "torch ops (searchsorted + gather + matmul)"


def kernels_enabled() -> bool:
    v = os.environ.get("COALIGN_SP3D")
    return KERNEL_DEFAULT if v is None else v != "0"


def _triple(v) -> Tuple[int, int, int]:
    return (int(v),) * 3 if isinstance(v, int) else tuple(int(a) for a in v)


class SparseTensor3d:
    """features [capacity, C], indices [capacity, 4] int32 (batch, z, y, x), ``count``: None (every row is a row) or a DEVICE int32 [1] (rows at or past it are
    unused capacity), spatial_shape (D, H, W), batch_size.  ``status``: the device status word of the kernel route (bit 0: a strided layer overflowed its capacity;
    the kernels only ever OR into it).  The cells of the rows in use are UNIQUE, as csrc/sparse_conv3d.hip assumes: of two rows that name one cell the site index
    keeps whichever arrives last, so the result of a list with duplicates is not defined."""

    def __init__(self, features: torch.Tensor, indices: torch.Tensor, spatial_shape: Sequence[int], batch_size: int, count: Optional[torch.Tensor] = None,
                 status: Optional[torch.Tensor] = None):
        assert features.dim() == 2 and indices.dim() == 2 and indices.shape[1] == 4 and indices.shape[0] == features.shape[0]
        self.features = features
        self.indices = indices if indices.dtype == torch.int32 else indices.to(torch.int32)
        self.spatial_shape = tuple(int(v) for v in spatial_shape)
        self.batch_size = int(batch_size)
        self.count = count
        self.status = status
        self._index = None                 # the kernel route's site index of these sites
        self._nbr = {}                     # (k, s, p) -> neighbour table; shared by the tensors that share the sites (spconv's indice_key)

    @property
    def capacity(self) -> int:
        return self.features.shape[0]

    def rows(self) -> int:
        """The number of rows in use (a host read-back when the count lives on the device)."""
        return self.capacity if self.count is None else min(int(self.count.item()), self.capacity)

    def replace_feature(self, features: torch.Tensor) -> "SparseTensor3d":
        out = SparseTensor3d(features, self.indices, self.spatial_shape, self.batch_size, self.count, self.status)
        out._index, out._nbr = self._index, self._nbr
        return out

    def valid_rows(self) -> torch.Tensor:
        """bool [rows()]: the rows whose coordinates lie inside the grid."""
        idx = self.indices[:self.rows()].long()
        hi = torch.tensor([self.batch_size, *self.spatial_shape], device=idx.device)
        return ((idx >= 0) & (idx < hi)).all(dim=1)

    def dense(self) -> torch.Tensor:
        """[N, C, D, H, W]: zeros where no site is (spconv's SparseConvTensor.dense())."""
        n = self.rows()
        D, H, W = self.spatial_shape
        C = self.features.shape[1]
        ok = self.valid_rows()
        idx, f = self.indices[:n][ok].long(), self.features[:n][ok]
        out = self.features.new_zeros((self.batch_size, D, H, W, C))
        out[idx[:, 0], idx[:, 1], idx[:, 2], idx[:, 3]] = f
        return out.permute(0, 4, 1, 2, 3).contiguous()


def _keys(idx: torch.Tensor, shape, batch: int):
    """(inside mask, linear cell index) of int64 coordinates [.., 4]."""
    D, H, W = shape
    b, z, y, x = idx.unbind(-1)
    ok = (b >= 0) & (b < batch) & (z >= 0) & (z < D) & (y >= 0) & (y < H) & (x >= 0) & (x < W)
    return ok, ((b * D + z) * H + y) * W + x


class _SparseConvBase(nn.Module):
    """weight [Cout, kd, kh, kw, Cin] (spconv 2's layout); spconv 1.2.1's [kd, kh, kw, Cin, Cout] is recognised by shape on load and permuted."""
    subm = False

    def __init__(self, in_channels: int, out_channels: int, kernel_size, stride=1, padding=0, bias: bool = False, indice_key: Optional[str] = None):
        super().__init__()
        if bias:
            raise NotImplementedError("the backbone's sparse convolutions have bias=False")
        self.in_channels, self.out_channels = in_channels, out_channels
        self.kernel_size, self.stride, self.padding = _triple(kernel_size), _triple(stride), _triple(padding)
        self.indice_key = indice_key
        self.site_capacity = None
        self.weight = nn.Parameter(torch.empty(out_channels, *self.kernel_size, in_channels))
        nn.init.kaiming_uniform_(self.weight.view(out_channels, -1), a=5 ** 0.5)

    @property
    def taps(self) -> int:
        return self.kernel_size[0] * self.kernel_size[1] * self.kernel_size[2]

    def _load_from_state_dict(self, state_dict, prefix, *args, **kwargs):
        key = prefix + "weight"
        w = state_dict.get(key)
        old = (*self.kernel_size, self.in_channels, self.out_channels)
        if w is not None and tuple(w.shape) == old and tuple(w.shape) != tuple(self.weight.shape):
            state_dict[key] = w.permute(4, 0, 1, 2, 3).contiguous()
        super()._load_from_state_dict(state_dict, prefix, *args, **kwargs)

    def extra_repr(self) -> str:
        return f"{self.in_channels}, {self.out_channels}, kernel_size={self.kernel_size}, stride={self.stride}, padding={self.padding}, bias=False"

    # ---- routes ---------------------------------------------------------------------------------------------------------------------------------------------
    def static_reason(self) -> Optional[str]:
        """Why the kernel route is closed whatever the input (None: it is open)."""
        if not kernels_enabled():
            return "COALIGN_SP3D=0" if os.environ.get("COALIGN_SP3D") == "0" else "the kernel route is not the default: COALIGN_SP3D=1 asks for it"
        if self.training:
            return "training mode"
        if not ops.sp3d_supported(self.in_channels, self.out_channels, self.taps) or max(self.kernel_size) > 3:
            return f"({self.in_channels}, {self.out_channels}) at kernel {self.kernel_size} is not one of VoxelBackBone8x's combinations"
        return None

    def kernel_reason(self, x: Optional[SparseTensor3d] = None) -> Optional[str]:
        """Why ``x`` would not take the kernel route through this layer (None: it takes it)."""
        why = self.static_reason()
        if why is None and x is not None:
            if not x.features.is_cuda:
                return "CPU tensors"
            if x.features.dtype != torch.float32:
                return f"{x.features.dtype} features"
        return why

    def route_text(self) -> str:
        why = self.static_reason()
        if why is not None:
            return f"{TORCH_TEXT} ({why})"
        arith = "fp32 vector arithmetic" if self.in_channels == 4 else "sp16 pairs on v_mfma_f32_32x32x16_f16"
        return f"{KERNEL_TEXT} ({self.taps} taps, {arith})"

    # ---- the torch-op route ---------------------------------------------------------------------------------------------------------------------------------
    def _gather_matmul(self, x: SparseTensor3d, n_in: int, out_idx: torch.Tensor) -> torch.Tensor:
        """sum over the taps, ascending, of W[tap] in[out * s - p + tap] for int64 output coordinates ``out_idx`` (rows outside the grid answer zero)."""
        f = x.features[:n_in]
        in_idx = x.indices[:n_in].long()
        ok_in, key_in = _keys(in_idx, x.spatial_shape, x.batch_size)
        rows_in = torch.nonzero(ok_in).flatten()
        skeys, order = torch.sort(key_in[rows_in])
        rows_in = rows_in[order]
        out = f.new_zeros((out_idx.shape[0], self.out_channels))
        if skeys.numel() == 0 or out_idx.shape[0] == 0:
            return out
        s = out_idx.new_tensor([1, *self.stride])
        p = out_idx.new_tensor([0, *self.padding])
        base = out_idx * s - p
        kd, kh, kw = self.kernel_size
        w = self.weight.to(f.dtype)
        for kz in range(kd):
            for ky in range(kh):
                for kx in range(kw):
                    ok, key = _keys(base + base.new_tensor([0, kz, ky, kx]), x.spatial_shape, x.batch_size)
                    pos = torch.searchsorted(skeys, key).clamp_(max=skeys.numel() - 1)
                    hit = ok & (skeys[pos] == key)
                    if not bool(hit.any()):
                        continue
                    g = f[rows_in[pos]]
                    g = torch.where(hit.unsqueeze(1), g, torch.zeros_like(g))          # (where, not a product: 0 x NaN of an unrelated row would leak)
                    out = out + g @ w[:, kz, ky, kx, :].t()
        return out

    def forward_torch(self, x: SparseTensor3d):
        raise NotImplementedError

    def forward(self, x: SparseTensor3d) -> SparseTensor3d:
        """The bare convolution (no batch norm, no ReLU): the torch-op route.  The kernels fuse the layer's batch norm and ReLU and are reached through ``SparseSequential``."""
        return self.forward_torch(x)


class SubMConv3d(_SparseConvBase):
    """Submanifold convolution, kernel 3, padding 1 (sparse_backbone_3d.py:49, :15): output sites = input sites, same row order."""
    subm = True

    def __init__(self, in_channels, out_channels, kernel_size=3, stride=1, padding=1, bias=False, indice_key=None):
        k = _triple(kernel_size)
        super().__init__(in_channels, out_channels, k, 1, tuple(v // 2 for v in k), bias, indice_key)

    def forward_torch(self, x: SparseTensor3d) -> SparseTensor3d:
        n = x.rows()
        idx = x.indices[:n].long()
        ok, _ = _keys(idx, x.spatial_shape, x.batch_size)
        y = self._gather_matmul(x, n, idx) * ok.unsqueeze(1).to(x.features.dtype)
        out = SparseTensor3d(y, x.indices[:n], x.spatial_shape, x.batch_size, None, x.status)
        return out


class SparseConv3d(_SparseConvBase):
    """Strided sparse convolution (sparse_backbone_3d.py:17-18, :87-88): output rows ascend in the linear cell index."""

    def out_shape(self, shape) -> Tuple[int, int, int]:
        return ops.sp3d_out_shape(shape, self.kernel_size, self.stride, self.padding)

    def capacity_bound(self, batch: int, shape, cap_in: int) -> int:
        """min(N D' H' W', capacity_in * prod ceil(k / s)), capped by ``site_capacity``."""
        o = self.out_shape(shape)
        per = int(np.prod([-(-k // s) for k, s in zip(self.kernel_size, self.stride)]))
        cap = min(batch * o[0] * o[1] * o[2], cap_in * per)
        return cap if self.site_capacity is None else min(cap, int(self.site_capacity))

    def forward_torch(self, x: SparseTensor3d) -> SparseTensor3d:
        n = x.rows()
        oshape = self.out_shape(x.spatial_shape)
        if min(oshape) < 1:
            raise ValueError(f"spatial shape {x.spatial_shape} is too small for kernel {self.kernel_size}")
        idx = x.indices[:n].long()
        ok_in, _ = _keys(idx, x.spatial_shape, x.batch_size)
        idx = idx[ok_in]
        s = idx.new_tensor([1, *self.stride])
        p = idx.new_tensor([0, *self.padding])
        cands = []
        kd, kh, kw = self.kernel_size
        for kz in range(kd):
            for ky in range(kh):
                for kx in range(kw):
                    t = idx + p - idx.new_tensor([0, kz, ky, kx])
                    o = torch.div(t, s, rounding_mode="floor")
                    ok, key = _keys(o, oshape, x.batch_size)
                    ok = ok & (t >= 0).all(dim=1) & (t % s == 0).all(dim=1)
                    cands.append(key[ok])
        keys = torch.unique(torch.cat(cands)) if cands else idx.new_zeros(0)          # sorted ascending
        status = x.status
        if self.site_capacity is not None and keys.numel() > self.site_capacity:
            keys = keys[:int(self.site_capacity)]
            status = (x.status if x.status is not None else torch.zeros(1, dtype=torch.int32, device=keys.device)) | ops.SP3D_STATUS_OVERFLOW
        D, H, W = oshape
        out_idx = torch.stack([keys // (D * H * W), keys // (H * W) % D, keys // W % H, keys % W], dim=1)
        y = self._gather_matmul(x, n, out_idx)
        return SparseTensor3d(y, out_idx.to(torch.int32), oshape, x.batch_size, None, status)


def _fold(conv: _SparseConvBase, bn: nn.BatchNorm1d):
    """(weight image, shift) of conv + eval batch norm, cached until a source tensor changes (``backbone._cache_of``)."""
    def build():
        scale = bn.weight * (1.0 / torch.sqrt(bn.running_var + bn.eps))
        shift = (bn.bias - bn.running_mean * scale).float().contiguous()
        w = (conv.weight * scale.view(-1, 1, 1, 1, 1)).reshape(conv.out_channels, conv.taps, conv.in_channels)
        return ops.pack_sp3d_weights(w), shift
    return _cache_of(conv, "_coalign_sp3d_cache").get([conv.weight, *bn.parameters(), *bn.buffers()], build)


def _kernel_layer(x: SparseTensor3d, conv: _SparseConvBase, bn: nn.BatchNorm1d) -> SparseTensor3d:
    """conv + batch norm + ReLU of one layer on the kernels; no host read-back."""
    dev = x.features.device
    feats = ops._aligned16(x.features)
    indices = ops._aligned16(x.indices)
    count = x.count if x.count is not None else torch.full((1,), x.capacity, dtype=torch.int32, device=dev)
    status = x.status if x.status is not None else torch.zeros(1, dtype=torch.int32, device=dev)
    if x._index is None:
        x._index = ops.sp3d_index_build(indices, count, x.batch_size, x.spatial_shape)
    wimg, shift = _fold(conv, bn)
    geo = (conv.kernel_size, conv.stride, conv.padding)
    if conv.subm:
        nbr = x._nbr.get(geo)
        if nbr is None:
            nbr = x._nbr[geo] = ops.sp3d_neighbors(indices, count, x.batch_size, x.spatial_shape, x._index, x.capacity, x.spatial_shape, *geo)
        y = ops.sp3d_conv(feats, nbr, count, conv.out_channels, wimg, shift)
        out = SparseTensor3d(y, indices, x.spatial_shape, x.batch_size, count, status)
        out._index, out._nbr = x._index, x._nbr
        return out
    oshape = conv.out_shape(x.spatial_shape)
    if min(oshape) < 1:
        raise ValueError(f"spatial shape {x.spatial_shape} is too small for kernel {conv.kernel_size}")
    cap_out = conv.capacity_bound(x.batch_size, x.spatial_shape, x.capacity)
    out_indices, out_count, out_index = ops.sp3d_strided_sites(indices, count, x.batch_size, x.spatial_shape, *geo, cap_out, status)
    nbr = ops.sp3d_neighbors(out_indices, out_count, x.batch_size, oshape, x._index, x.capacity, x.spatial_shape, *geo)
    y = ops.sp3d_conv(feats, nbr, out_count, conv.out_channels, wimg, shift)
    out = SparseTensor3d(y, out_indices, oshape, x.batch_size, out_count, status)
    out._index = out_index
    return out


class SparseSequential(nn.Sequential):
    """spconv's SparseSequential for this backbone: children are sparse convolutions, ``BatchNorm1d`` / ``ReLU`` (applied to the active rows' features) or nested
    SparseSequentials.  A (conv, BatchNorm1d, ReLU) run is ONE kernel launch on the kernel route."""

    def forward(self, x: SparseTensor3d) -> SparseTensor3d:
        mods = list(self)
        i = 0
        while i < len(mods):
            m = mods[i]
            if isinstance(m, _SparseConvBase):
                fused = i + 2 < len(mods) and isinstance(mods[i + 1], nn.BatchNorm1d) and isinstance(mods[i + 2], nn.ReLU)
                if fused and m.kernel_reason(x) is None and not mods[i + 1].training:
                    x = _kernel_layer(x, m, mods[i + 1])
                    i += 3
                    continue
                x = m.forward_torch(x)
            elif isinstance(m, SparseSequential):
                x = m(x)
            else:                                              # BatchNorm1d / ReLU: on the features of the active rows; a row outside the grid stays zero
                f = x.features
                if f.shape[0] > 0:
                    ok = x.valid_rows().unsqueeze(1)
                    f = torch.where(ok, m(f), torch.zeros_like(f))
                x = x.replace_feature(f)
            i += 1
        return x


def post_act_block(cin, cout, kernel_size, indice_key=None, stride=1, padding=0, conv_type="subm", norm_fn=None) -> SparseSequential:
    """sparse_backbone_3d.py:11-30."""
    if conv_type == "subm":
        conv = SubMConv3d(cin, cout, kernel_size, bias=False, indice_key=indice_key)
    elif conv_type == "spconv":
        conv = SparseConv3d(cin, cout, kernel_size, stride=stride, padding=padding, bias=False, indice_key=indice_key)
    else:
        raise NotImplementedError(conv_type)
    return SparseSequential(conv, norm_fn(cout), nn.ReLU())


def _norm(c: int) -> nn.BatchNorm1d:
    return nn.BatchNorm1d(c, eps=1e-3, momentum=0.01)


class MeanVFE(nn.Module):
    """mean_vfe.py:4-32: the mean of a voxel's points."""

    def __init__(self, model_cfg: dict, num_point_features: int, **kwargs):
        super().__init__()
        self.model_cfg = model_cfg
        self.num_point_features = num_point_features

    def get_output_feature_dim(self) -> int:
        return self.num_point_features

    def route_text(self) -> str:
        return "coalign_sp3d_mean_vfe" if kernels_enabled() else "torch ops (sum / clamp_min)"

    def forward(self, batch_dict: dict, **kwargs) -> dict:
        v, n = batch_dict["voxel_features"], batch_dict["voxel_num_points"]
        if kernels_enabled() and v.is_cuda and v.dtype == torch.float32 and not torch.is_floating_point(n):
            batch_dict["voxel_features"] = ops.sp3d_mean_vfe(v, n)
        else:
            mean = v.sum(dim=1, keepdim=False) / torch.clamp_min(n.view(-1, 1), min=1.0).type_as(v)
            batch_dict["voxel_features"] = mean.contiguous()
        return batch_dict


class VoxelBackBone8x(nn.Module):
    """sparse_backbone_3d.py:33-153, layer for layer, with the reference's module names (``conv_input.0.weight`` ... ``conv_out.1.running_var``).
    ``site_capacity`` (None: the bound min(N D' H' W', capacity_in * prod ceil(k / s))) caps the rows a strided layer may produce: on overflow the first
    ``site_capacity`` sites in ascending order are kept and bit 0 of the device status word ``last_status`` is set (nothing on the path reads it)."""

    def __init__(self, model_cfg: dict, input_channels: int, grid_size, site_capacity: Optional[int] = None, **kwargs):
        super().__init__()
        self.model_cfg = model_cfg
        g = [int(v) for v in grid_size]
        self.sparse_shape = (g[2] + 1, g[1], g[0])
        self.site_capacity = site_capacity
        self.last_status = None
        block = post_act_block
        self.conv_input = SparseSequential(SubMConv3d(input_channels, 16, 3, padding=1, bias=False, indice_key="subm1"), _norm(16), nn.ReLU())
        self.conv1 = SparseSequential(block(16, 16, 3, norm_fn=_norm, padding=1, indice_key="subm1"))
        self.conv2 = SparseSequential(block(16, 32, 3, norm_fn=_norm, stride=2, padding=1, indice_key="spconv2", conv_type="spconv"),
                                      block(32, 32, 3, norm_fn=_norm, padding=1, indice_key="subm2"), block(32, 32, 3, norm_fn=_norm, padding=1, indice_key="subm2"))
        self.conv3 = SparseSequential(block(32, 64, 3, norm_fn=_norm, stride=2, padding=1, indice_key="spconv3", conv_type="spconv"),
                                      block(64, 64, 3, norm_fn=_norm, padding=1, indice_key="subm3"), block(64, 64, 3, norm_fn=_norm, padding=1, indice_key="subm3"))
        self.conv4 = SparseSequential(block(64, 64, 3, norm_fn=_norm, stride=2, padding=(0, 1, 1), indice_key="spconv4", conv_type="spconv"),
                                      block(64, 64, 3, norm_fn=_norm, padding=1, indice_key="subm4"), block(64, 64, 3, norm_fn=_norm, padding=1, indice_key="subm4"))
        self.num_point_features = model_cfg["num_features_out"] if "num_features_out" in model_cfg else 128
        self.conv_out = SparseSequential(SparseConv3d(64, self.num_point_features, (3, 1, 1), stride=(2, 1, 1), padding=0, bias=False, indice_key="spconv_down2"),
                                         _norm(self.num_point_features), nn.ReLU())
        self.backbone_channels = {"x_conv1": 16, "x_conv2": 32, "x_conv3": 64, "x_conv4": 64}

    def sparse_convs(self):
        return [(n, m) for n, m in self.named_modules() if isinstance(m, _SparseConvBase)]

    def plan(self) -> dict:
        """{layer name: route text} from the modules and switches alone (no GPU, no tensor)."""
        return {n: m.route_text() for n, m in self.sparse_convs()}

    def level_shapes(self):
        """The spatial shapes after conv_input / conv2 / conv3 / conv4 / conv_out."""
        shapes, s = [self.sparse_shape], self.sparse_shape
        for name in ("conv2", "conv3", "conv4"):
            s = getattr(self, name)[0][0].out_shape(s)
            shapes.append(s)
        shapes.append(self.conv_out[0].out_shape(s))
        return shapes

    def forward(self, batch_dict: dict) -> dict:
        for _, m in self.sparse_convs():
            m.site_capacity = self.site_capacity
        if batch_dict.get("voxel_sites") is not None:      # ``voxel_sites``' tensor: mean features, a device count, the batch size and (kernel route) the site index are its own
            x = batch_dict["voxel_sites"]
            if tuple(x.spatial_shape) != tuple(self.sparse_shape):
                raise ValueError(f"voxel_sites of spatial shape {x.spatial_shape} for a backbone of sparse shape {self.sparse_shape}")
        else:
            f, coords = batch_dict["voxel_features"], batch_dict["voxel_coords"]
            x = SparseTensor3d(f, coords.int(), self.sparse_shape, int(batch_dict["batch_size"]))
            if f.is_cuda:
                x.status = torch.zeros(1, dtype=torch.int32, device=f.device)
        x = self.conv_input(x)
        x_conv1 = self.conv1(x)
        x_conv2 = self.conv2(x_conv1)
        x_conv3 = self.conv3(x_conv2)
        x_conv4 = self.conv4(x_conv3)
        out = self.conv_out(x_conv4)
        self.last_status = out.status
        batch_dict.update({"encoded_spconv_tensor": out, "encoded_spconv_tensor_stride": 8,
                           "multi_scale_3d_features": {"x_conv1": x_conv1, "x_conv2": x_conv2, "x_conv3": x_conv3, "x_conv4": x_conv4},
                           "multi_scale_3d_strides": {"x_conv1": 1, "x_conv2": 2, "x_conv3": 4, "x_conv4": 8}})
        return batch_dict


class HeightCompression(nn.Module):
    """height_compression.py:4-27: dense() viewed as [N, C D, H, W], channel c D + d.  On the kernel route one launch writes the map (channels-last memory)."""

    def __init__(self, model_cfg: dict, **kwargs):
        super().__init__()
        self.model_cfg = model_cfg
        self.num_bev_features = model_cfg["feature_num"]

    def route_text(self) -> str:
        return "coalign_sp3d_to_dense (channels-last, every element written)" if kernels_enabled() else "torch ops (zeros + index_put)"

    def compress(self, t: SparseTensor3d) -> torch.Tensor:
        if t.count is not None and t._index is not None and t.features.is_cuda and t.features.dtype == torch.float32:
            return ops.sp3d_to_dense(t.features, t.count, t._index, t.batch_size, t.spatial_shape)
        d = t.dense()
        N, C, D, H, W = d.shape
        return d.view(N, C * D, H, W)

    def forward(self, batch_dict: dict) -> dict:
        batch_dict["spatial_features"] = self.compress(batch_dict["encoded_spconv_tensor"])
        batch_dict["spatial_features_stride"] = batch_dict["encoded_spconv_tensor_stride"]
        return batch_dict


# ---- raw point clouds -> the trunk's input tensor ------------------------------------------------------------------------------------------------------------------
VOXEL_SITES_KERNEL_DEFAULT = True          # ``voxel_sites`` on ``ops.sp3d_voxelize`` for CUDA points when COALIGN_SP3D is unset: 0.283 ms against 2.25 ms for the torch ops at the OPV2V grid, 5 agents
VOXEL_SITES_KERNEL_TEXT = "coalign_sp3d_voxelize (bitmap mark + prefix count, integer atomicMin rounds, mean features and the level-0 site index in one call)"
VOXEL_SITES_TORCH_TEXT = "torch ops (floor-divide, sort by (cell, point), segment ranks, index_add)"


def voxel_sites_kernels() -> bool:
    v = os.environ.get("COALIGN_SP3D")
    return VOXEL_SITES_KERNEL_DEFAULT if v is None else v != "0"


def voxel_sites_route_text() -> str:
    if voxel_sites_kernels():
        return VOXEL_SITES_KERNEL_TEXT
    return f"{VOXEL_SITES_TORCH_TEXT} ({'COALIGN_SP3D=0' if os.environ.get('COALIGN_SP3D') == '0' else 'the kernel route is not the default: COALIGN_SP3D=1 asks for it'})"


def _voxel_sites_torch(points, offsets, voxel_size, lidar_range, shape, max_points, max_voxels, capacity, ego_filter, filter_range):
    """The contract of include_open/coalign_amd_sp3d_voxelize.h in torch ops (any device; reads counts back to size its tensors): same rows, same order, same bits."""
    dev, P = points.device, points.shape[0]
    D, H, W = shape
    f32 = lambda v: torch.tensor(v, dtype=torch.float32, device=dev)
    n_clouds = offsets.numel() - 1
    off = torch.cummax(offsets.to(device=dev, dtype=torch.int64).clamp(0, P), dim=0).values
    p = torch.arange(P, device=dev)
    cloud = torch.searchsorted(off[1:].contiguous(), p, right=True)
    ok = (p >= off[0]) & (cloud < n_clouds)
    x, y, z = points[:, 0], points[:, 1], points[:, 2]
    if ego_filter:                                   # pcd_utils.py:69-88, closed box
        ok &= ~((x >= f32(-1.95)) & (x <= f32(2.95)) & (y >= f32(-1.1)) & (y <= f32(1.1)))
    if filter_range is not None:                     # pcd_utils.py:41-66, strict
        fr = f32([float(v) for v in filter_range])
        ok &= (x > fr[0]) & (x < fr[3]) & (y > fr[1]) & (y < fr[4]) & (z > fr[2]) & (z < fr[5])
    rng = f32([float(v) for v in lidar_range])
    vs = f32([float(v) for v in voxel_size])
    grid = f32([float(g) for g in ops.sp3d_voxel_grid(voxel_size, lidar_range)])
    c = torch.floor((points[:, :3] - rng[:3]) / vs)                                    # float32, IEEE divide: the kernels' expression
    ok &= ((c >= 0) & (c < grid)).all(dim=1)                                           # (NaN fails every comparison)
    p = p[ok]
    ci = c[ok].to(torch.int64)
    cell = ((cloud[ok] * D + ci[:, 2]) * H + ci[:, 1]) * W + ci[:, 0]
    key, _ = torch.sort(cell * max(P, 1) + p)                                          # by cell, then by point index
    cell, p = key // max(P, 1), key % max(P, 1)
    start = torch.ones_like(cell, dtype=torch.bool)
    start[1:] = cell[1:] != cell[:-1]
    group = torch.cumsum(start, 0) - 1                                                 # the cell's place among the occupied cells (ascending)
    first = torch.nonzero(start).flatten()
    pos = torch.arange(cell.numel(), device=dev) - first[group] if cell.numel() else group
    gcell, gfirst = cell[first], p[first]                                              # per occupied cell: the cell, its opening point
    gcloud = gcell // (D * H * W)
    rank = torch.empty_like(gfirst)
    rank[torch.argsort(gfirst)] = torch.arange(gfirst.numel(), device=dev)             # clouds are contiguous and ascending in the point index:
    per_cloud = torch.bincount(gcloud, minlength=n_clouds)[:n_clouds]                   # the rank among ALL opening points minus the opened cells of the clouds in front
    number = rank - (torch.cumsum(per_cloud, 0) - per_cloud)[gcloud]
    keep = number < max_voxels
    kept_per_cloud = torch.bincount(gcloud[keep], minlength=n_clouds)[:n_clouds]
    cloud_counts = torch.cat([kept_per_cloud, kept_per_cloud.sum().view(1)]).to(torch.int32)
    row = torch.cumsum(keep, 0) - 1
    kept = int(keep.sum())
    n_rows = min(kept, capacity)
    live = keep & (row < capacity)
    feats = points.new_zeros((capacity, 4))
    indices = torch.zeros((capacity, 4), dtype=torch.int32, device=dev)
    counts = torch.zeros(capacity, dtype=torch.int64, device=dev)
    pl = live[group] if cell.numel() else live
    for t in range(max_points):                                                        # ascending point order: slot t of every voxel in one step
        m = pl & (pos == t)
        r = row[group[m]]
        feats[r] = feats[r] + points[p[m]]
        counts[r] += 1
    feats[:n_rows] = feats[:n_rows] / counts[:n_rows].to(torch.float32).unsqueeze(1)
    lc = gcell[live]
    indices[:n_rows] = torch.stack([lc // (D * H * W), lc // (H * W) % D, lc // W % H, lc % W], dim=1).to(torch.int32)
    status = (ops.SP3D_STATUS_OVERFLOW if kept > capacity else 0) | (ops.SP3D_STATUS_MAX_VOXELS if bool((per_cloud >= max_voxels).any()) else 0)
    count = torch.tensor([n_rows], dtype=torch.int32, device=dev)
    return feats, indices, count, cloud_counts, torch.tensor([status], dtype=torch.int32, device=dev)


def voxel_sites(points: torch.Tensor, offsets: torch.Tensor, voxel_size, lidar_range, spatial_shape, max_points: int, max_voxels: int, capacity: int,
                ego_filter: bool = False, filter_range=None) -> SparseTensor3d:
    """Raw clouds -> the input tensor of ``VoxelBackBone8x``: ``points`` [P, 4] float32 (the clouds of a frame concatenated), ``offsets`` int32 [n_clouds + 1] (on the
    points' device for the kernel route) -> a ``SparseTensor3d`` of ``capacity`` rows with the mean of each voxel's first ``max_points`` points (MeanVFE), rows ascending
    in the linear cell index, a device ``count``, ``status`` (bit 0: more voxels than ``capacity``, bit 1: a cloud reached ``max_voxels``), ``cloud_counts`` int32
    [n_clouds + 1] and, on the kernel route, ``_index`` already built.  The contract is that of include_open/coalign_amd_sp3d_voxelize.h on both routes, bit for bit."""
    shape = tuple(int(v) for v in spatial_shape)
    n_clouds = int(offsets.numel()) - 1
    gx, gy, gz = ops.sp3d_voxel_grid(voxel_size, lidar_range)
    if points.dim() != 2 or points.shape[1] != 4 or n_clouds < 1 or capacity < 1 or max_points < 1 or max_voxels < 1:
        raise ValueError("voxel_sites: points [P, 4], at least one cloud, capacity, max_points and max_voxels of at least 1")
    if shape[1:] != (gy, gx) or shape[0] < gz:
        raise ValueError(f"voxel_sites: the sparse shape {shape} does not hold the voxel grid (z, y, x) = {(gz, gy, gx)}")
    if points.is_cuda and points.dtype == torch.float32 and voxel_sites_kernels():
        feats, indices, count, cloud_counts, index, status = ops.sp3d_voxelize(points, offsets.to(device=points.device, dtype=torch.int32), voxel_size, lidar_range, shape,
                                                                               max_points, max_voxels, capacity, ego_filter, filter_range)
    else:
        feats, indices, count, cloud_counts, status = _voxel_sites_torch(points.float(), offsets, voxel_size, lidar_range, shape, int(max_points), int(max_voxels),
                                                                         int(capacity), ego_filter, filter_range)
        index = None
    x = SparseTensor3d(feats, indices, shape, n_clouds, count, status)
    x._index = index
    x.cloud_counts = cloud_counts
    return x


def plan(hypes: dict) -> dict:
    """{layer name: route text} of the sparse trunk a ``second_ssfa*`` config builds -- MeanVFE, every sparse convolution of VoxelBackBone8x, HeightCompression --
    from the config and the switches alone (no GPU, no tensor), as the camera model's ``plan`` does for its trunk."""
    args = hypes["model"]["args"]
    rng = np.asarray(args["lidar_range"], dtype=np.float64)
    grid = np.round((rng[3:6] - rng[:3]) / np.asarray(args["voxel_size"], dtype=np.float64)).astype(np.int64)
    bb = VoxelBackBone8x(args["spconv"], args["spconv"]["num_features_in"], grid).eval()
    lines = {"vfe": MeanVFE(args["mean_vfe"], args["mean_vfe"]["num_point_features"]).route_text()}
    lines.update({f"spconv_block.{n}": t for n, t in bb.plan().items()})
    lines["map_to_bev"] = HeightCompression(args["map2bev"]).route_text()
    return lines
