"""The camera model of the reference, ``lift_splat_shoot_intermediate``: Lift-Splat frustum pooling on the gfx950 kernels of
csrc/lss_pool.hip, the multi-scale BEV encoder with the existing ``AttFusion`` / ``MaxFusion`` kernels, the detector class.

Restated from the reference, with its names and signatures:

* ``gen_dx_bx``                   <- opencood/utils/camera_utils.py:129-134 (``nx`` keeps ``LongTensor``'s truncation: (4.8 - (-4.8)) / 0.4 gives 23, not 24)
* ``depth_discretization``        <- opencood/utils/camera_utils.py:187-196
* ``create_frustum``              <- opencood/models/lift_splat_shoot.py:65-78
* ``LiftSplat``                   <- ``get_geometry`` / ``voxel_pooling`` of opencood/models/lift_splat_shoot.py:80-102, 116-169 and the outer product of
                                     ``CamEncode.forward``, opencood/models/sub_modules/lss_submodule.py:134-136
* ``Up``, ``BevEncodeMSFusion``   <- opencood/models/sub_modules/lss_submodule.py:19-38, 357-417
* ``LiftSplatShootIntermediate``  <- opencood/models/lift_splat_shoot_intermediate.py:18-69

What the reference does per frame -- materialise depth x features, sort 10^6 keys per agent, running sum, difference -- is replaced by an inverted index that
depends on the camera matrices alone (``LiftSplat.build_index``, once per rig) and two launches per frame (``ops.lss_pool``).  ``COALIGN_LSS_POOL=0`` selects the
torch route (``LiftSplat.forward_torch``), which is also what runs on the CPU and for shapes the kernel refuses.

Out of scope here, as in the issue that introduced this module: the EfficientNet / ResNet-101 image trunks (pluggable), depth supervision and ground-truth
depth, ``BevEncodeSSFusion``, training.  The BEV trunk's convolutions have a kernel route behind ``COALIGN_LSS_BEV`` (off by default, ``BevEncodeMSFusion``).
"""
from __future__ import annotations

import math
import os
from typing import Optional

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import backbone, ops
from .encoder import host_ints
from .fusion import AttFusion, MaxFusion, regroup
from .pose import normalize_pairwise_tfm

# The kernel route of the frustum pooling: on by default on the GPU; "0" selects the torch route (module attribute, read at every call).
LSS_POOL = os.environ.get("COALIGN_LSS_POOL", "1") != "0"
# The kernel route of the BEV encoder (``BevEncodeMSFusion``: stem, ResNet stages, ``Up`` and ``down_layer`` on the SplitMap kernels): OFF by default, "1" switches it
# on.  Read once at import; a module copies it into ``bev_kernels`` when it is built, and that attribute can be set per module.
LSS_BEV = os.environ.get("COALIGN_LSS_BEV", "0") != "0"


def gen_dx_bx(xbound, ybound, zbound):
    """camera_utils.py:129-134: float32 ``dx`` (cell size) and ``bx`` (centre of the first cell), int64 ``nx`` (cells per axis, TRUNCATED like ``LongTensor``)."""
    rows = [xbound, ybound, zbound]
    dx = torch.tensor([float(row[2]) for row in rows], dtype=torch.float32)
    bx = torch.tensor([row[0] + row[2] / 2.0 for row in rows], dtype=torch.float32)
    nx = torch.tensor([int((row[1] - row[0]) / row[2]) for row in rows], dtype=torch.int64)
    return dx, bx, nx


def depth_discretization(depth_min, depth_max, num_bins, mode):
    """camera_utils.py:187-196: the depth of every bin, float64 numpy (UD: uniform, LID: linearly increasing)."""
    if mode == "UD":
        bin_size = (depth_max - depth_min) / num_bins
        return depth_min + bin_size * np.arange(num_bins)
    if mode == "LID":
        bin_size = 2 * (depth_max - depth_min) / (num_bins * (1 + num_bins))
        return depth_min + bin_size * (np.arange(num_bins) * np.arange(1, 1 + num_bins)) / 2
    raise NotImplementedError(mode)


def frustum_axes(grid_conf: dict, data_aug_conf: dict, downsample: int):
    """The three float32 axes ``create_frustum`` stacks: xs [fW], ys [fH] (``torch.linspace``'s own rounding), ds [D]."""
    ogfH, ogfW = data_aug_conf["final_dim"]
    fH, fW = ogfH // downsample, ogfW // downsample
    ds = torch.tensor(depth_discretization(*grid_conf["ddiscr"], grid_conf["mode"]), dtype=torch.float)
    xs = torch.linspace(0, ogfW - 1, fW, dtype=torch.float)
    ys = torch.linspace(0, ogfH - 1, fH, dtype=torch.float)
    return xs, ys, ds


def create_frustum(grid_conf: dict, data_aug_conf: dict, downsample: int) -> torch.Tensor:
    """lift_splat_shoot.py:65-78: [D, fH, fW, 3] float32, (pixel x, pixel y, depth) of every frustum point."""
    xs, ys, ds = frustum_axes(grid_conf, data_aug_conf, downsample)
    D, fH, fW = ds.numel(), ys.numel(), xs.numel()
    return torch.stack((xs.view(1, 1, fW).expand(D, fH, fW), ys.view(1, fH, 1).expand(D, fH, fW), ds.view(-1, 1, 1).expand(D, fH, fW)), -1)


def _inverse3(a: torch.Tensor) -> torch.Tensor:
    """[..., 3, 3] by the adjugate, the arithmetic of the kernel (a singular matrix gives non-finite entries instead of raising)."""
    c00 = a[..., 1, 1] * a[..., 2, 2] - a[..., 1, 2] * a[..., 2, 1]
    c01 = a[..., 1, 2] * a[..., 2, 0] - a[..., 1, 0] * a[..., 2, 2]
    c02 = a[..., 1, 0] * a[..., 2, 1] - a[..., 1, 1] * a[..., 2, 0]
    det = a[..., 0, 0] * c00 + a[..., 0, 1] * c01 + a[..., 0, 2] * c02
    rows = [c00, a[..., 0, 2] * a[..., 2, 1] - a[..., 0, 1] * a[..., 2, 2], a[..., 0, 1] * a[..., 1, 2] - a[..., 0, 2] * a[..., 1, 1],
            c01, a[..., 0, 0] * a[..., 2, 2] - a[..., 0, 2] * a[..., 2, 0], a[..., 0, 2] * a[..., 1, 0] - a[..., 0, 0] * a[..., 1, 2],
            c02, a[..., 0, 1] * a[..., 2, 0] - a[..., 0, 0] * a[..., 2, 1], a[..., 0, 0] * a[..., 1, 1] - a[..., 0, 1] * a[..., 1, 0]]
    return (torch.stack(rows, -1) / det[..., None]).reshape(a.shape)


class LiftSplat(nn.Module):
    """Frustum pooling: ``forward(depth_logit [A N, D, fH, fW], x_img [A N, C, fH, fW], rots, trans, intrins, post_rots, post_trans)`` -> the BEV map
    [A, nz C, ny, nx] (rows = y, columns = x, channel z C + c) of ``voxel_pooling``.  A = agents (the reference's B), N = cameras per agent; the camera tensors
    are [A, N, 3, 3] / [A, N, 3].  Owns no parameter; grid and frustum are non-persistent buffers (absent from ``state_dict``, like the reference's attributes).

    On the GPU the kernel route: ``build_index`` turns the camera matrices into an inverted index once per rig, a frame is two launches (``ops.lss_pool``), its
    output is channels-last.  The module keeps its last index with a copy of the camera tensors and reuses it while they are ``torch.equal`` (one comparison of
    30 floats per camera; on the device that is one small launch and one host read per frame -- pass ``index=`` to skip it); ``index_builds`` counts builds."""

    def __init__(self, grid_conf: dict, data_aug_conf: dict, downsample: int):
        super().__init__()
        self.grid_conf, self.data_aug_conf, self.downsample = grid_conf, data_aug_conf, int(downsample)
        dx, bx, nx = gen_dx_bx(grid_conf["xbound"], grid_conf["ybound"], grid_conf["zbound"])
        self.register_buffer("dx", dx, persistent=False)
        self.register_buffer("bx", bx, persistent=False)
        self.register_buffer("frustum", create_frustum(grid_conf, data_aug_conf, self.downsample), persistent=False)
        self.nx = [int(v) for v in nx]                        # (nx, ny, nz), host integers
        self.lower = [float(v) for v in (bx - dx / 2.0)]      # bx - dx / 2 evaluated in float32, as voxel_pooling does (lift_splat_shoot.py:126)
        self.cell_size = [float(v) for v in dx]
        self.axes = frustum_axes(grid_conf, data_aug_conf, self.downsample)
        self.D, self.fH, self.fW = (int(v) for v in self.frustum.shape[:3])
        self.force_torch = False                              # measurement / test aid: the torch route whatever the device
        self.reference_cells = False                          # True: the index is built from the reference's float32 geometry (get_geometry) instead of the float64 cells
        self.index_builds = 0
        self._index = self._index_key = None

    # ---- geometry ------------------------------------------------------------------------------------------------------------------------------------------
    def get_geometry(self, rots, trans, intrins, post_rots, post_trans) -> torch.Tensor:
        """lift_splat_shoot.py:80-102 in float32, op for op: [A, N, D, fH, fW, 3], the ego-frame position of every frustum point."""
        B, N, _ = trans.shape
        points = self.frustum - post_trans.view(B, N, 1, 1, 1, 3)
        points = torch.inverse(post_rots).view(B, N, 1, 1, 1, 3, 3).matmul(points.unsqueeze(-1))
        points = torch.cat((points[:, :, :, :, :, :2] * points[:, :, :, :, :, 2:3], points[:, :, :, :, :, 2:3]), 5)
        combine = rots.matmul(torch.inverse(intrins))
        points = combine.view(B, N, 1, 1, 1, 3, 3).matmul(points).squeeze(-1)
        return points + trans.view(B, N, 1, 1, 1, 3)

    def voxel_indices(self, geom: torch.Tensor):
        """voxel_pooling's index line and bounds test (lift_splat_shoot.py:126, :133-135) on a float32 geometry: (int64 [P, 3] = (x, y, z), kept [P])."""
        idx = ((geom - (self.bx - self.dx / 2.0)) / self.dx).long().view(-1, 3)
        nx, ny, nz = self.nx
        kept = (idx[:, 0] >= 0) & (idx[:, 0] < nx) & (idx[:, 1] >= 0) & (idx[:, 1] < ny) & (idx[:, 2] >= 0) & (idx[:, 2] < nz)
        return idx, kept

    def cells_float64(self, rots, trans, intrins, post_rots, post_trans) -> torch.Tensor:
        """What ``coalign_lss_cells`` computes, with torch ops in float64 from the float32 inputs: int32 [A N, D, fH, fW], (z ny + y) nx + x or -1 (non-finite
        coordinates and those at or beyond +-2^31 are dropped)."""
        B, N, _ = trans.shape
        f = self.frustum.double() - post_trans.double().view(B, N, 1, 1, 1, 3)
        q = (_inverse3(post_rots.double()).view(B, N, 1, 1, 1, 3, 3) * f.unsqueeze(-2)).sum(-1)
        q = torch.cat((q[..., :2] * q[..., 2:3], q[..., 2:3]), -1)
        comb = rots.double().matmul(_inverse3(intrins.double()))
        g = (comb.view(B, N, 1, 1, 1, 3, 3) * q.unsqueeze(-2)).sum(-1) + trans.double().view(B, N, 1, 1, 1, 3)
        v = (g - torch.tensor(self.lower, dtype=torch.float64, device=g.device)) / torch.tensor(self.cell_size, dtype=torch.float64, device=g.device)
        ok = v.abs() < 2.0 ** 31                               # (False for NaN)
        idx = torch.where(ok, v, torch.full_like(v, -1.0)).trunc().long()
        nx, ny, nz = self.nx
        kept = ok.all(-1) & (idx[..., 0] >= 0) & (idx[..., 0] < nx) & (idx[..., 1] >= 0) & (idx[..., 1] < ny) & (idx[..., 2] >= 0) & (idx[..., 2] < nz)
        cell = (idx[..., 2] * ny + idx[..., 1]) * nx + idx[..., 0]
        return torch.where(kept, cell, torch.full_like(cell, -1)).to(torch.int32).reshape(B * N, self.D, self.fH, self.fW)

    # ---- the index ------------------------------------------------------------------------------------------------------------------------------------------
    def build_index(self, rots, trans, intrins, post_rots, post_trans) -> ops.LiftSplatIndex:
        """The inverted index of a camera rig: cells from ``ops.lss_cells`` on the GPU (``cells_float64`` on the CPU), lists from ``ops.build_lss_index``.  The float64
        cells differ from the reference's float32 ones for the few points that lie within ~1e-5 cells of a boundary (18 of 2 764 800 on a seeded full-size rig);
        ``reference_cells = True`` builds the index from the float32 geometry instead, for a bit-for-bit choice of cells against a reference checkpoint's run."""
        A, N, _ = trans.shape
        cams = (rots, trans, intrins, post_rots, post_trans)
        if self.reference_cells:
            idx, kept = self.voxel_indices(self.get_geometry(*(t.float() for t in cams)))
            cell = torch.where(kept, (idx[:, 2] * self.nx[1] + idx[:, 1]) * self.nx[0] + idx[:, 0], torch.full_like(idx[:, 0], -1)).to(torch.int32).view(A * N, self.D, self.fH, self.fW)
        elif trans.is_cuda:
            xs, ys, ds = (v.to(trans.device) for v in self.axes)
            cell = ops.lss_cells(*cams, xs, ys, ds, self.lower, self.cell_size, self.nx, N)
        else:
            cell = self.cells_float64(*(t.float() for t in cams))
        self.index_builds += 1
        return ops.build_lss_index(cell, A, N, *self.nx)

    def index_for(self, rots, trans, intrins, post_rots, post_trans) -> ops.LiftSplatIndex:
        """The cached index when the five camera tensors are those it was built from, else a new one (which replaces it)."""
        key = torch.cat([t.reshape(trans.shape[0] * trans.shape[1], -1).float() for t in (rots, trans, intrins, post_rots, post_trans)], dim=1)
        if self._index is None or self._index_key.device != key.device or not torch.equal(self._index_key, key):
            self._index = self.build_index(rots, trans, intrins, post_rots, post_trans)
            self._index_key = key.clone()
        return self._index

    # ---- routes ---------------------------------------------------------------------------------------------------------------------------------------------
    def kernel_reason(self, depth_logit: torch.Tensor, x_img: torch.Tensor) -> Optional[str]:
        """None when ``forward`` takes the kernel route for these tensors, else why not, in words."""
        if not LSS_POOL or self.force_torch:
            return "switched off (COALIGN_LSS_POOL=0)"
        if not (depth_logit.is_cuda and x_img.is_cuda):
            return "not on the GPU"
        if depth_logit.dtype != torch.float32 or x_img.dtype != torch.float32 or torch.is_grad_enabled() and (depth_logit.requires_grad or x_img.requires_grad):
            return "float32 inference only"
        if not ops.lss_shape_ok(int(x_img.shape[1]), int(depth_logit.shape[1])):
            return f"C = {int(x_img.shape[1])}, D = {int(depth_logit.shape[1])} outside the kernel's C in {{64, 128}}, D <= 128"
        return None

    def _lift(self, depth_logit, x_img, A, N):
        """The reference's materialised volume: softmax x features (lss_submodule.py:134-136), permuted and flattened to [P, C] (lift_splat_shoot.py:111-122)."""
        C = x_img.shape[1]
        vol = F.softmax(depth_logit, dim=1).unsqueeze(1) * x_img.unsqueeze(2)
        return vol.view(A, N, C, self.D, self.fH, self.fW).permute(0, 1, 3, 4, 5, 2).reshape(-1, C)

    def forward_torch(self, depth_logit, x_img, rots, trans, intrins, post_rots, post_trans) -> torch.Tensor:
        """Outer product -> float32 cells -> float32 ``index_add``: the CPU route and the fallback."""
        A, N, _ = trans.shape
        C = x_img.shape[1]
        nx, ny, nz = self.nx
        x = self._lift(depth_logit, x_img, A, N)
        idx, kept = self.voxel_indices(self.get_geometry(rots, trans, intrins, post_rots, post_trans))
        agent = torch.arange(idx.shape[0], device=idx.device) // (N * self.D * self.fH * self.fW)
        key = ((agent * nz + idx[:, 2]) * ny + idx[:, 1]) * nx + idx[:, 0]
        final = torch.zeros((A * nz * ny * nx, C), dtype=x.dtype, device=x.device).index_add_(0, key[kept], x[kept])
        return final.view(A, nz, ny, nx, C).permute(0, 1, 4, 2, 3).reshape(A, nz * C, ny, nx)

    def forward_reference_ops(self, depth_logit, x_img, rots, trans, intrins, post_rots, post_trans) -> torch.Tensor:
        """The reference's route op for op (lift_splat_shoot.py:116-169 with camera_utils.py:209-217): kept, ranks, argsort, cumsum, difference, scatter.  The
        timing baseline of tools/time_lss_pool.py."""
        B, N, _ = trans.shape
        C = x_img.shape[1]
        nx, ny, nz = self.nx
        x = self._lift(depth_logit, x_img, B, N)
        Nprime = x.shape[0]
        geom_feats, _ = self.voxel_indices(self.get_geometry(rots, trans, intrins, post_rots, post_trans))
        batch_ix = torch.cat([torch.full([Nprime // B, 1], ix, device=x.device, dtype=torch.long) for ix in range(B)])
        geom_feats = torch.cat((geom_feats, batch_ix), 1)
        kept = (geom_feats[:, 0] >= 0) & (geom_feats[:, 0] < nx) & (geom_feats[:, 1] >= 0) & (geom_feats[:, 1] < ny) & (geom_feats[:, 2] >= 0) & (geom_feats[:, 2] < nz)
        x, geom_feats = x[kept], geom_feats[kept]
        ranks = geom_feats[:, 0] * (ny * nz * B) + geom_feats[:, 1] * (nz * B) + geom_feats[:, 2] * B + geom_feats[:, 3]
        sorts = ranks.argsort()
        x, geom_feats, ranks = x[sorts], geom_feats[sorts], ranks[sorts]
        final = torch.zeros((B, C, nz, ny, nx), dtype=x.dtype, device=x.device)
        if x.shape[0]:
            x = x.cumsum(0)
            last = torch.ones(x.shape[0], device=x.device, dtype=torch.bool)
            last[:-1] = ranks[1:] != ranks[:-1]
            x, geom_feats = x[last], geom_feats[last]
            x = torch.cat((x[:1], x[1:] - x[:-1]))
            final[geom_feats[:, 3], :, geom_feats[:, 2], geom_feats[:, 1], geom_feats[:, 0]] = x
        return torch.cat(final.unbind(dim=2), 1)

    def forward(self, depth_logit, x_img, rots, trans, intrins, post_rots, post_trans, index: Optional[ops.LiftSplatIndex] = None) -> torch.Tensor:
        if self.kernel_reason(depth_logit, x_img) is not None:
            return self.forward_torch(depth_logit, x_img, rots, trans, intrins, post_rots, post_trans)
        if index is None:
            index = self.index_for(rots, trans, intrins, post_rots, post_trans)
        return ops.lss_pool(depth_logit, x_img, index)


class Up(nn.Module):
    """lss_submodule.py:19-38: bilinear up-sampling (``align_corners=True``), concatenation behind the skip map, two 3 x 3 convolutions with BatchNorm and ReLU."""

    def __init__(self, in_channels: int, out_channels: int, scale_factor: int = 2):
        super().__init__()
        self.up = nn.Upsample(scale_factor=scale_factor, mode="bilinear", align_corners=True)
        self.conv = nn.Sequential(nn.Conv2d(in_channels, out_channels, kernel_size=3, padding=1, bias=False), nn.BatchNorm2d(out_channels), nn.ReLU(inplace=True),
                                  nn.Conv2d(out_channels, out_channels, kernel_size=3, padding=1, bias=False), nn.BatchNorm2d(out_channels), nn.ReLU(inplace=True))

    def forward(self, x1, x2):
        return self.conv(torch.cat([x2, self.up(x1)], dim=1))


class _BasicBlock(nn.Module):
    """torchvision's ResNet ``BasicBlock`` under its attribute names (conv1, bn1, relu, conv2, bn2, downsample).  A call is the reference's op sequence on every
    device.  The names are also those of ``backbone.BasicBlock``, whose SplitMap route (route decision, folded weights, ``_forward_split``) is shared below as plain
    functions: the kernel route of ``BevEncodeMSFusion`` calls it.  Not a subclass, so that whatever walks a model for ``backbone.BasicBlock`` sees what it saw before."""

    def __init__(self, inplanes: int, planes: int, stride: int = 1):
        super().__init__()
        self.conv1 = nn.Conv2d(inplanes, planes, kernel_size=3, stride=stride, padding=1, bias=False)
        self.bn1 = nn.BatchNorm2d(planes)
        self.relu = nn.ReLU(inplace=True)
        self.conv2 = nn.Conv2d(planes, planes, kernel_size=3, stride=1, padding=1, bias=False)
        self.bn2 = nn.BatchNorm2d(planes)
        self.downsample = None
        self.stride = stride
        if stride != 1 or inplanes != planes:
            self.downsample = nn.Sequential(nn.Conv2d(inplanes, planes, kernel_size=1, stride=stride, bias=False), nn.BatchNorm2d(planes))

    route = backbone.BasicBlock.route
    skip_pointwise = backbone.BasicBlock.skip_pointwise
    _folded = backbone.BasicBlock._folded
    _forward_split = backbone.BasicBlock._forward_split

    def forward(self, x):
        out = self.bn2(self.conv2(self.relu(self.bn1(self.conv1(x)))))
        return self.relu(out + (x if self.downsample is None else self.downsample(x)))


def _resnet18_layer(inplanes: int, planes: int, stride: int) -> nn.Sequential:
    return nn.Sequential(_BasicBlock(inplanes, planes, stride), _BasicBlock(planes, planes, 1))


def _fuse_torch(x: torch.Tensor, record_len, affine: torch.Tensor, att: bool) -> torch.Tensor:
    """``AttFusion`` / ``MaxFusion`` op by op (fusion_in_one.py:47-136) for maps that are not on the GPU: warp every agent into the ego frame, then per pixel the
    scaled dot-product attention over the agents (the ego's row) or the maximum."""
    out = []
    for b, xb in enumerate(regroup(x, record_len)):
        n, C, H, W = xb.shape
        grid = F.affine_grid(affine[b, 0, :n].to(xb.dtype), [n, C, H, W], align_corners=False)
        w = F.grid_sample(xb, grid, align_corners=False)
        if att:
            q = w.view(n, C, -1).permute(2, 0, 1)
            ctx = torch.bmm(F.softmax(torch.bmm(q, q.transpose(1, 2)) / math.sqrt(C), -1), q)
            out.append(ctx.permute(1, 2, 0).view(n, C, H, W)[0])
        else:
            out.append(w.max(dim=0)[0])
    return torch.stack(out)


class BevEncodeMSFusion(nn.Module):
    """lss_submodule.py:357-417 (``att_ms`` | ``max_ms``): a 7 x 7 stem, ResNet-18's ``layer1..3``, the three maps fused across the agents, ``Up`` twice and
    ``down_layer``.  By default the convolutions are torch ops; the three fusions are the ``AttFusion`` / ``MaxFusion`` kernels on the GPU.  With ``bev_kernels``
    (``COALIGN_LSS_BEV=1``) an eval-mode float32 CUDA map takes the kernel route (``kernel_route``): stem on ``ops.conv7x7_s2_sp``, the stages on
    the SplitMap route of ``backbone.BasicBlock``, both ``Up`` steps on ``ops.up2x_concat_sp`` + ``ops.conv3x3_sp``, decoded once on the batch [single maps ; fused
    maps]; its two outputs are channels-last.  Parameter names are the
    reference's (``conv1``, ``bn1``, ``layer1.0.conv1`` ... ``layer2.0.downsample.0``, ``up_layer1.conv.0``, ...).  torchvision is not a dependency of this package:
    the ``layerN`` names are written from its ``BasicBlock`` attribute names and are NOT pinned by a golden fixture made from the reference."""

    def __init__(self, fusion_args: dict):
        super().__init__()
        args = fusion_args["args"]
        inC = args["in_channels"]
        self.discrete_ratio = args["voxel_size"][0]
        self.downsample_rate = 1
        self.bev_kernels = LSS_BEV                              # the kernel route of the convolutions (off by default); may be set per module
        self.conv1 = nn.Conv2d(inC, 64, kernel_size=7, stride=2, padding=3, bias=False)
        self.bn1 = nn.BatchNorm2d(64)
        self.relu = nn.ReLU(inplace=True)
        self.layer1 = _resnet18_layer(64, 64, 1)
        self.layer2 = _resnet18_layer(64, 128, 2)
        self.layer3 = _resnet18_layer(128, 256, 2)
        self.up_layer1 = Up(64 + 256, 256, scale_factor=2)
        self.up_layer2 = Up(128 + 256, 256, scale_factor=2)
        self.down_layer = nn.Sequential(nn.Conv2d(256, 256, kernel_size=3, stride=1, padding=1), nn.ReLU(inplace=True),
                                        nn.Conv2d(256, 128, kernel_size=3, stride=1, padding=1), nn.ReLU(inplace=True))
        if fusion_args["core_method"] == "max_ms":
            self.fuse_module = nn.ModuleList([MaxFusion(), MaxFusion(), MaxFusion()])      # (parameter-free: the state_dict is the reference's plain list's)
        elif fusion_args["core_method"] == "att_ms":
            self.fuse_module = nn.ModuleList([AttFusion(64), AttFusion(128), AttFusion(256)])
        else:
            raise NotImplementedError(f"fusion core_method '{fusion_args['core_method']}' (att_ms | max_ms; BevEncodeSSFusion is outside this package)")

    def _fuse(self, i: int, x: torch.Tensor, record_len, affine: torch.Tensor) -> torch.Tensor:
        if x.is_cuda and not self.training:
            return self.fuse_module[i](x, record_len, affine)
        return _fuse_torch(x, record_len, affine, isinstance(self.fuse_module[i], AttFusion))

    # ---- the kernel route -----------------------------------------------------------------------------------------------------------------------------------
    STEM_KERNEL = "conv7x7_s2_sp (7 x 7 / stride 2, channels-last float32 in, SplitMap out, fp16 x 2)"
    UP_KERNEL = "up2x_concat_sp (bilinear x 2 + concatenation written as one SplitMap)"
    SWITCHED_OFF = "switched off (COALIGN_LSS_BEV=0)"

    def _blocks(self):
        return [(f"layer{i + 1}.{j}", blk) for i, layer in enumerate((self.layer1, self.layer2, self.layer3)) for j, blk in enumerate(layer)]

    def _static_reason(self) -> Optional[str]:
        """The part of ``kernel_shape_reason`` that the module's shapes, its mode and the switches decide, without a tensor."""
        inC = self.conv1.in_channels
        if not ops.conv7x7_s2_shape_ok(inC, self.conv1.out_channels):
            return f"in_channels = {inC} outside the stem kernel's Cin % 16 == 0, 16 .. {ops.CONV7X7_MAX_CIN}"
        if self.training:
            return "training mode"
        if not backbone.split_maps_active():
            return "the SplitMap arithmetic (fp16 x 2) is not in force"
        if any(blk.route().kind != backbone.BLOCK_SPLIT for _, blk in self._blocks()):
            return "a BasicBlock is off the SplitMap route (backbone's switches)"
        return None

    def kernel_shape_reason(self, x: torch.Tensor) -> Optional[str]:
        """None when the kernels take the map ``x``, else why not, in words."""
        static = self._static_reason()
        if static is not None:
            return static
        if x.dim() != 4 or x.shape[1] != self.conv1.in_channels:
            return f"a map of shape {tuple(x.shape)} for in_channels = {self.conv1.in_channels}"
        H, W = int(x.shape[2]), int(x.shape[3])
        if H % 8 or W % 8:
            return f"H x W = {H} x {W}, not multiples of 8 (the Up concatenations do not match)"
        if not x.is_cuda or x.dtype != torch.float32 or torch.is_grad_enabled() and x.requires_grad:
            return "not a float32 CUDA tensor in inference"
        return None

    def kernel_route(self, x: torch.Tensor) -> bool:
        """Eval mode, ``bev_kernels`` and no reason against (the family convention of DESIGN.md section 8k)."""
        return bool(not self.training and self.bev_kernels and self.kernel_shape_reason(x) is None)

    def plan(self) -> dict:
        """{layer name: route text} from the module's shapes, mode and switches alone (no GPU, no tensor; the map-size and device conditions of
        ``kernel_shape_reason`` are decided per call).  ``routes.plan`` does not walk camera models; this is the camera trunk's own answer."""
        from .routes import conv3x3_text                      # (routes imports the detector classes, which import this module)
        why = self.SWITCHED_OFF if not self.bev_kernels else self._static_reason()
        lines = {}
        convs = [(n, m) for n, m in self.named_modules() if isinstance(m, nn.Conv2d)]
        if why is not None:
            for n, m in convs:
                lines[n] = f"{backbone.MIOPEN} ({why})"
            lines["up_layer2.up"] = lines["up_layer1.up"] = f"torch bilinear interpolation + cat ({why})"
        else:
            lines["conv1"] = self.STEM_KERNEL
            for n, blk in self._blocks():
                r = blk.route()
                if blk.stride == 1:
                    lines[f"{n}.conv1"] = backbone.SP
                else:
                    lines[f"{n}.conv1"] = backbone.SP_S2 if r.s2_dense else conv3x3_text(blk.conv1, backbone.CONV_EMU_TERMS) + backbone.SPLIT_OUT
                    lines[f"{n}.downsample.0"] = ("tenth tap of " + backbone.SP_S2.split(" (")[0] if r.s2_dense and r.skip_fused
                                                  else backbone.pointwise_text(blk.downsample[0].in_channels, backbone.CONV_EMU_TERMS))
                lines[f"{n}.conv2"] = backbone.SP
            for up in ("up_layer2", "up_layer1"):
                lines[f"{up}.up"] = self.UP_KERNEL
                lines[f"{up}.conv.0"] = lines[f"{up}.conv.3"] = backbone.SP
            lines["down_layer.0"] = lines["down_layer.2"] = backbone.SP
        lines["fuse_module"] = MaxFusion.plan_fusion(self.fuse_module[0], self.conv1.out_channels)[0]
        return lines

    def _folded(self):
        """(stem image, bias), per ``Up`` and for ``down_layer`` the (tap-major terms-16 image, bias) pairs: BatchNorm folded (``backbone.fold_bn``), cached until a
        parameter or buffer changes -- a warmed-up forward allocates no weight memory."""
        def pack(conv, bn):
            w, b = backbone.fold_bn(conv.weight, conv.bias, bn) if bn is not None else (conv.weight, conv.bias)
            return backbone.Conv3x3Pack(w.detach().float().contiguous()).emu(16, True), b.detach().float().contiguous(), conv.out_channels

        def build():
            w, b = backbone.fold_bn(self.conv1.weight, None, self.bn1)
            ups = [[pack(u.conv[0], u.conv[1]), pack(u.conv[3], u.conv[4])] for u in (self.up_layer2, self.up_layer1)]
            return (ops.pack_conv7x7_s2_weight(w), b.float().contiguous()), ups, [pack(self.down_layer[0], None), pack(self.down_layer[2], None)]
        return backbone._cache_of(self).get(self, build)

    def _forward_kernels(self, x, record_len, affine):
        stem, ups, down = self._folded()
        A = x.shape[0]
        cur = ops.conv7x7_s2_sp(x, stem[0], stem[1], relu=True)
        # layer1..3 as ResNetStages.forward runs them: SplitMaps inside a stage; its last block hands out the channels-last float32 map (fusion, Up) and, when the
        # next stage opens with conv3x3_sp_s2, the SplitMap of that map as well
        layers, maps, carry = (self.layer1, self.layer2, self.layer3), [], None
        for i, layer in enumerate(layers):
            both = i + 1 < len(layers) and layers[i + 1][0].route().s2_dense
            for j, blk in enumerate(layer):
                last = j == len(layer) - 1
                cur = blk._forward_split(cur, blk.route(), last, out_both=last and both, x_split=carry if j == 0 and not isinstance(cur, ops.SplitMap) else None)
                carry = None
                if last and both:
                    cur, carry = cur
            maps.append(cur)
        x1, x2, x3 = maps
        f1, f2, f3 = (self._fuse(i, v, record_len, affine) for i, v in enumerate(maps))

        def batch(single, fused):                               # [single maps ; fused maps] in channels-last memory
            return torch.cat([single.permute(0, 2, 3, 1), fused.permute(0, 2, 3, 1)]).permute(0, 3, 1, 2)

        def conv(y, layer, out_split=True, relu=True):
            return ops.conv3x3_sp(y, layer[0], layer[1], layer[2], None, relu, out_split=out_split)

        y = ops.up2x_concat_sp(batch(x2, f2), batch(x3, f3))
        y = conv(conv(y, ups[0][0]), ups[0][1], out_split=False)             # (channels-last float32: the next Up's low map)
        y = ops.up2x_concat_sp(batch(x1, f1), y)
        y = conv(conv(y, ups[1][0]), ups[1][1])
        y = conv(conv(y, down[0]), down[1], out_split=False)
        return y[:A], y[A:]

    def forward(self, x, record_len, pairwise_t_matrix):
        _, _, H, W = x.shape
        affine = normalize_pairwise_tfm(pairwise_t_matrix, H, W, self.discrete_ratio, self.downsample_rate)
        if self.kernel_route(x):
            return self._forward_kernels(x, record_len, affine)
        x = self.relu(self.bn1(self.conv1(x)))
        x1 = self.layer1(x)
        x2 = self.layer2(x1)
        x3 = self.layer3(x2)
        x_single = self.down_layer(self.up_layer1(self.up_layer2(x3, x2), x1))
        x1_fuse, x2_fuse, x3_fuse = (self._fuse(i, v, record_len, affine) for i, v in enumerate((x1, x2, x3)))
        x_fuse = self.down_layer(self.up_layer1(self.up_layer2(x3_fuse, x2_fuse), x1_fuse))
        return x_single, x_fuse


class CamHeads(nn.Module):
    """What the model owns of ``CamEncode`` (lss_submodule.py:41-63) when no image trunk is injected: the 1 x 1 ``depth_head`` (512 -> D) and ``image_head``
    (512 -> C) under the reference's names.  They read the map ``get_eff_features`` returns."""
    TRUNK_CHANNELS = 512

    def __init__(self, D: int, C: int):
        super().__init__()
        self.D, self.C = D, C
        self.depth_head = nn.Conv2d(self.TRUNK_CHANNELS, D, kernel_size=1, padding=0)
        self.image_head = nn.Conv2d(self.TRUNK_CHANNELS, C, kernel_size=1, padding=0)


class LiftSplatShootIntermediate(nn.Module):
    """lift_splat_shoot_intermediate.py:18-69 over lift_splat_shoot.py:16-62: ``args`` = ``hypes['model']['args']``; ``forward(data_dict)`` reads ``image_inputs``
    (``rots, trans, intrins, post_rots, post_trans`` as [A, N, ...]), ``record_len`` and ``pairwise_t_matrix`` and returns the reference's keys -- ``cls_preds,
    reg_preds, depth_items`` (None: no depth supervision here), ``dir_preds`` and, with ``supervise_single``, their ``_single`` forms.

    The image trunk is pluggable (EfficientNet is not a dependency of this package).  Without one the model owns ``camencode.depth_head`` and
    ``camencode.image_head`` only and reads ``image_inputs['trunk_features']`` [A N, 512, fH, fW] -- what ``CamEncode.get_eff_features`` returns.  With
    ``camencode=`` an encoder that has ``get_eff_features``, ``depth_head`` and ``image_head`` it reads ``image_inputs['imgs']`` [A, N, >= 3, H, W]."""

    def __init__(self, args: dict, camencode: Optional[nn.Module] = None):
        super().__init__()
        if args.get("use_depth_gt"):
            raise NotImplementedError("use_depth_gt: ground-truth depth is outside this package")
        self.grid_conf, self.data_aug_conf = args["grid_conf"], args["data_aug_conf"]
        self.bevout_feature = args["bevout_feature"]
        self.downsample, self.camC = args["img_downsample"], args["img_features"]
        self.splat = LiftSplat(self.grid_conf, self.data_aug_conf, self.downsample)
        self.D = self.splat.D
        self.camera_encoder_type = args.get("camera_encoder", "EfficientNet")
        self.camencode = camencode if camencode is not None else CamHeads(self.D, self.camC)
        fusion_args = args["fusion_args"]
        self.ms = fusion_args["core_method"].endswith("ms")
        if not self.ms:
            raise NotImplementedError("BevEncodeSSFusion (single-scale fusion) is outside this package: fusion_args.core_method must be att_ms or max_ms")
        self.bevencode = BevEncodeMSFusion(fusion_args)
        self.cls_head = nn.Conv2d(self.bevout_feature, args["anchor_number"], kernel_size=1)
        self.reg_head = nn.Conv2d(self.bevout_feature, 7 * args["anchor_number"], kernel_size=1)
        self.use_dir = "dir_args" in args
        if self.use_dir:
            self.dir_head = nn.Conv2d(self.bevout_feature, args["dir_args"]["num_bins"] * args["anchor_number"], kernel_size=1)
        self.supervise_single = bool(args.get("supervise_single", False))
        for p in self.camencode.parameters():
            p.requires_grad_(False)
        if self.supervise_single:
            self.cls_head_before_fusion = nn.Conv2d(self.bevout_feature, args["anchor_number"], kernel_size=1)
            self.reg_head_before_fusion = nn.Conv2d(self.bevout_feature, 7 * args["anchor_number"], kernel_size=1)
            if self.use_dir:
                self.dir_head_before_fusion = nn.Conv2d(self.bevout_feature, args["dir_args"]["num_bins"] * args["anchor_number"], kernel_size=1)

    def camera_features(self, image_inputs: dict):
        """-> (depth_logit [A N, D, fH, fW], x_img [A N, C, fH, fW]): the two 1 x 1 heads on the trunk's map."""
        if hasattr(self.camencode, "get_eff_features"):
            imgs = image_inputs["imgs"]
            feats = self.camencode.get_eff_features(imgs.reshape(-1, *imgs.shape[2:])[:, :3])
        else:
            feats = image_inputs["trunk_features"]
        return self.camencode.depth_head(feats), self.camencode.image_head(feats)

    def get_voxels(self, image_inputs: dict) -> torch.Tensor:
        depth_logit, x_img = self.camera_features(image_inputs)
        return self.splat(depth_logit, x_img, *(image_inputs[k] for k in ("rots", "trans", "intrins", "post_rots", "post_trans")))

    def forward(self, data_dict: dict) -> dict:
        record_len = host_ints(data_dict["record_len"])
        x = self.get_voxels(data_dict["image_inputs"])
        x_single, x_fuse = self.bevencode(x, record_len, data_dict["pairwise_t_matrix"])
        out = {"cls_preds": self.cls_head(x_fuse), "reg_preds": self.reg_head(x_fuse), "depth_items": None}
        if self.use_dir:
            out["dir_preds"] = self.dir_head(x_fuse)
        if self.supervise_single:
            out["cls_preds_single"] = self.cls_head_before_fusion(x_single)
            out["reg_preds_single"] = self.reg_head_before_fusion(x_single)
            if self.use_dir:
                out["dir_preds_single"] = self.dir_head_before_fusion(x_single)
        return out


__all__ = ["LSS_POOL", "LSS_BEV", "gen_dx_bx", "depth_discretization", "frustum_axes", "create_frustum", "LiftSplat", "Up", "BevEncodeMSFusion", "CamHeads",
           "LiftSplatShootIntermediate"]
