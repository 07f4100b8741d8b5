"""Detector classes of the hot path -- the plugin boundary.

``PointPillarBaselineMultiscale`` / ``CoAlign`` / ``PointPillar`` keep the reference's class names, constructor
(``args`` = ``hypes['model']['args']``), ``forward(data_dict) -> {'cls_preds', 'reg_preds'[, 'dir_preds']}`` and
``state_dict`` key names (opencood/models/point_pillar_baseline_multiscale.py:17-135,
opencood/models/point_pillar_coalign.py:9-10, opencood/models/point_pillar.py:16-80), so reference yamls and
checkpoints drive them unchanged.  Pillar encode + scatter and warp + fusion run in the gfx950 kernels; the
dense convolutions run on MIOpen through PyTorch-ROCm.
"""
from __future__ import annotations

import os
from collections import namedtuple
from typing import Optional, Sequence

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import backbone as _bb
from . import ops
from .backbone import BaseBEVBackbone, BasicBlock, DownsampleConv, NaiveCompressor, ResNetBEVBackbone, _cache_of, _fast_ok
from .encoder import PillarVFE, PointPillarScatter, host_ints
from .fusion import AttFusion, DiscoFusion, MaxFusion, V2VNetFusion, V2XViTFusion, When2comFusion, fuse_multiscale
from .pose import normalize_pairwise_tfm

# Round 4: PillarVFE + PointPillarScatter as one launch with a sparse canvas (csrc/pillar_sparse.hip) feeding the first ResNet block directly.
# "0": the dense persistent canvas of rounds 2-3 (measurement aid; module attribute, read at every call).
SPARSE_CANVAS = os.environ.get("COALIGN_SPARSE_CANVAS", "1") != "0"


def _heads(model: nn.Module) -> list:
    names = ["cls", "reg"] + (["unc"] if getattr(model, "unc_head", None) is not None else []) + (["dir"] if model.use_dir else [])
    return [(k + "_preds", getattr(model, k + "_head")) for k in names]


def _run_heads(model: nn.Module, x: torch.Tensor) -> dict:
    """cls / reg / dir 1x1 heads.  Inference fast path: one convolution with the concatenated head weights (+ one fused
    bias pass) instead of three convolutions and three bias kernels; the outputs are channel slices of one tensor."""
    heads = _heads(model)
    route = heads_route(model)
    if isinstance(x, ops.SplitMap) and not (route.split_in and model.cls_head.weight.is_cuda):
        x = x.dense()
    if not isinstance(x, ops.SplitMap) and not _fast_ok(model, x):
        return {k: h(x) for k, h in heads}

    def build():
        return (torch.cat([h.weight for _, h in heads]).contiguous(), torch.cat([h.bias for _, h in heads]).contiguous())
    w, b = _cache_of(model.cls_head).get([t for _, h in heads for t in (h.weight, h.bias)], build)
    if isinstance(x, ops.SplitMap):
        # round 6: the shrink header's last convolution handed its map over as a SplitMap: the merged heads read it with one 16-byte load per lane and operand
        img = _cache_of(model.reg_head, "_coalign_pw_cache").get([t for _, h in heads for t in (h.weight, h.bias)], lambda: ops.pack_heads_sp_weight(w))      # (a cache slot of its own: reg_head's fold cache holds the pointwise image)
        y = ops.heads_sp(x, img, b, w.shape[0])
    elif route.pointwise:
        # round 4: the merged 1x1 heads on the hand-written pointwise kernel (split-bf16 matrix cores; GEMM rows padded to 32), reading the shrink
        # header's map in whatever layout it has and writing the NCHW maps the decode kernel reads -- no rocBLAS / bias pass in the frame
        pk = _cache_of(model.reg_head).get([t for _, h in heads for t in (h.weight, h.bias)], lambda: _bb.PointwisePack(w, False))
        y = ops.pointwise_conv(x, pk.get(), b, w.shape[0], relu=False)
    else:
        y = ops.bias_act_(F.conv2d(x, w, None), b, None, False)
    out, c0 = {}, 0
    for k, h in heads:
        out[k] = y[:, c0:c0 + h.out_channels]
        c0 += h.out_channels
    return out


# split_in: a SplitMap handed over by the shrink header is read by ops.heads_sp (else it is made dense first); pointwise: a float32 map is read by the pointwise kernel
# (split-bf16 image, Cin <= 512; GEMM rows padded to 32), else by rocBLAS
HeadsRoute = namedtuple("HeadsRoute", "split_in pointwise")


def heads_route(model: nn.Module, terms: Optional[int] = None) -> HeadsRoute:
    return HeadsRoute(split_in=bool(_bb.HEADS_SPLIT_IN and not model.training and _bb.split_maps_active(terms) and heads_sp_shape_ok(model)),
                      pointwise=_bb.pointwise_split(model.cls_head.in_channels, terms) and model.cls_head.in_channels <= 512)


def heads_take_split_map(model: nn.Module, x=None) -> bool:
    """The merged heads can read the shrink header's map as a SplitMap (``ops.heads_sp``): <= 32 head channels in all, Cin % 16 == 0, eval mode, the switch on."""
    return heads_route(model).split_in and model.cls_head.weight.is_cuda


def sparse_canvas_route(model: nn.Module, terms: Optional[int] = None) -> bool:
    """``encode`` has the pillar encoder hand a ``SparseCanvas`` to a backbone whose first block reads it (the encoder adds its own ``matrix_core_ok``)."""
    resnet = getattr(model.backbone, "resnet", None)
    first = resnet.layer0[0] if resnet is not None and hasattr(resnet, "layer0") and hasattr(resnet.layer0[0], "takes_sparse_canvas") else None
    return bool(SPARSE_CANVAS and _bb.FAST_INFERENCE and isinstance(model, PointPillarBaselineMultiscale) and not model.compression and not model.training
                and first is not None and first.takes_sparse_canvas(terms))


def compressor_sparse_route(model: nn.Module, terms: Optional[int] = None) -> bool:
    """``encode`` has the pillar encoder hand a ``SparseCanvas`` to NaiveCompressor, whose narrow encoder reads it in place; the first block then reads the
    compressor's ``SplitMap`` as before (``sparse_canvas_route`` stays "the FIRST BLOCK reads the canvas")."""
    comp = getattr(model, "naive_compressor", None) if getattr(model, "compression", False) else None
    return bool(SPARSE_CANVAS and _bb.FAST_INFERENCE and isinstance(model, PointPillarBaselineMultiscale) and not model.training
                and comp is not None and comp.takes_sparse_canvas(terms))


def fusion_route(model: nn.Module, channels: Sequence[int]) -> bool:
    """The static half of the one-launch channels-last fusion: plain attention (``feat_dim`` = the map's channels) or max at every scale, and scales the kernel
    takes (<= 3 of 64 / 128 / 256 channels: ``ops.warp_fuse_nhwc_ok`` and ``ops.warp_fuse_nhwc`` are the authority and check every call; this copy serves the plan)."""
    kinds = {type(f) for f in model.fusion_net}
    plain = kinds == {MaxFusion} or (kinds == {AttFusion} and all(f.feature_dims == c for f, c in zip(model.fusion_net, channels)))
    return bool(plain and not model.training and len(channels) <= 3 and all(c in (64, 128, 256) for c in channels))


def heads_sp_shape_ok(model: nn.Module) -> bool:
    """The merged heads' shape fits ``coalign_heads_sp``: 1 x 1 heads of at most 32 rows in all (``ops.HEADS_SP_MAX_ROWS``) over Cin % 16 == 0 channels."""
    heads = [h for _, h in _heads(model)]
    rows = sum(h.out_channels for h in heads)
    return rows <= ops.HEADS_SP_MAX_ROWS and model.cls_head.in_channels % 16 == 0 and all(tuple(h.kernel_size) == (1, 1) for h in heads)


def _single_agent_batch(data_dict: dict) -> dict:
    """``batch_dict`` of the single-agent models (point_pillar.py:52-60) plus the optional keys of this build's callers: ``record_len`` when the batch carries one
    (saves PillarVFE its host read of the largest agent index), the device voxeliser's streaming keys and FramePipeline's frame record -- PillarVFE raises
    ``FrameRecordUnsupported`` for a record on a route that reads the arrays directly, so a record can never be dropped silently."""
    pl = data_dict["processed_lidar"]
    batch_dict = {"voxel_features": pl["voxel_features"], "voxel_coords": pl["voxel_coords"], "voxel_num_points": pl["voxel_num_points"]}
    if data_dict.get("record_len") is not None:
        batch_dict["record_len"] = host_ints(data_dict["record_len"])
    for k in ("voxel_count_dev", "voxel_cells_unique", "want_pillar_features", "pillar_frame"):
        if k in pl:
            batch_dict[k] = pl[k]
    return batch_dict


class PointPillarBaselineMultiscale(nn.Module):
    def __init__(self, args: dict):
        super().__init__()
        self.pillar_vfe = PillarVFE(args["pillar_vfe"], num_point_features=4, voxel_size=args["voxel_size"],
                                    point_cloud_range=args["lidar_range"])
        self.scatter = PointPillarScatter(args["point_pillar_scatter"])
        bb = args["base_bev_backbone"]
        self.backbone = ResNetBEVBackbone(bb, 64) if bb.get("resnet", True) else BaseBEVBackbone(bb, 64)
        self.voxel_size = args["voxel_size"]
        self.fusion_net = nn.ModuleList()
        for i in range(len(bb["layer_nums"])):
            if args["fusion_method"] == "max":
                self.fusion_net.append(MaxFusion())
            elif args["fusion_method"] == "att":
                self.fusion_net.append(AttFusion(args["att"]["feat_dim"][i]))
            else:
                raise NotImplementedError(f"fusion_method '{args['fusion_method']}' is outside the CoAlign hot path (att | max)")
        self.out_channel = sum(bb["num_upsample_filter"])
        self.shrink_flag = "shrink_header" in args
        if self.shrink_flag:
            self.shrink_conv = DownsampleConv(args["shrink_header"])
            self.out_channel = args["shrink_header"]["dim"][-1]
        self.compression = "compression" in args
        if self.compression:
            self.naive_compressor = NaiveCompressor(64, args["compression"])
        self.cls_head = nn.Conv2d(self.out_channel, args["anchor_number"], kernel_size=1)
        self.reg_head = nn.Conv2d(self.out_channel, 7 * args["anchor_number"], kernel_size=1)
        self.use_dir = "dir_args" in args
        if self.use_dir:
            self.dir_head = nn.Conv2d(self.out_channel, args["dir_args"]["num_bins"] * args["anchor_number"], kernel_size=1)
        if args.get("backbone_fix"):
            self.backbone_fix()

    def backbone_fix(self):
        frozen = [self.pillar_vfe, self.scatter, self.backbone, self.cls_head, self.reg_head]
        if self.compression:
            frozen.append(self.naive_compressor)
        if self.shrink_flag:
            frozen.append(self.shrink_conv)
        for m in frozen:
            for p in m.parameters():
                p.requires_grad = False

    # -- stages, exposed separately so the sharded runner can place them on different ranks ----------------
    accepts_normalized_affine = True      # encode() takes data_dict['normalized_affine_matrix'] in place of normalising pairwise_t_matrix itself (FramePipeline)
    accepts_pillar_frame = True           # encode() hands processed_lidar['pillar_frame'] (ops.PillarFrameRecord) to PillarVFE: FramePipeline may read frames in place

    def encode(self, data_dict: dict):
        """Per-agent part: pillars -> canvas -> multiscale features.  Returns (feature list, normalised affine)."""
        batch_dict = _single_agent_batch(dict(data_dict, record_len=host_ints(data_dict["record_len"])))      # (with the device voxeliser's streaming keys and FramePipeline's frame record)
        # round 4: the encoder hands a SparseCanvas (one launch, no dense canvas) to a backbone whose first block reads it
        resnet = getattr(self.backbone, "resnet", None)
        keep_sparse = self.pillar_vfe.sparse_canvas
        self.pillar_vfe.sparse_canvas = sparse_canvas_route(self) or compressor_sparse_route(self)
        try:
            batch_dict = self.scatter(self.pillar_vfe(batch_dict))
        finally:
            self.pillar_vfe.sparse_canvas = keep_sparse
        spatial_features = batch_dict["spatial_features"]
        H0, W0 = spatial_features.shape[2:]
        affine = data_dict.get("normalized_affine_matrix")      # FramePipeline: normalised on the host from the dataset's host copy of the matrix (same float64 steps)
        if affine is None:
            affine = normalize_pairwise_tfm(data_dict["pairwise_t_matrix"], H0, W0, self.voxel_size[0])
        if self.compression:
            # the compressor hands the first ResNet block a SplitMap when that block reads one: its strided opener + skip then run as one launch on it
            opener = resnet.layer0[0] if resnet is not None and hasattr(resnet, "layer0") else None
            want_split = bool(not self.training and isinstance(opener, BasicBlock) and opener.takes_split_maps() and opener.conv1.in_channels % 16 == 0)
            spatial_features = self.naive_compressor(spatial_features, out_split=True) if want_split else self.naive_compressor(spatial_features)
        return self.backbone.get_multiscale_feature(spatial_features), affine

    def _fuse_scales(self, feature_list, record_len, affine, rows=None):
        """The per-scale fusion launches are independent: on the GPU the coarser scales (few workgroups, latency bound)
        run on side streams next to the finest one instead of queueing behind it."""
        n = len(feature_list)
        x0 = feature_list[0]
        # (an AttFusion whose configured feat_dim differs from its map's channels -- no shipped yaml -- takes the per-scale route below,
        #  where the module rescales its input so that the scores are divided by sqrt(feat_dim) like the reference's)
        if x0.is_cuda and fusion_route(self, [x.shape[1] for x in feature_list]):
            fused = fuse_multiscale(feature_list, record_len, affine, ops.FUSE_ATT if isinstance(self.fusion_net[0], AttFusion) else ops.FUSE_MAX, rows)
            if fused is not None:
                return fused
        if n == 1 or not x0.is_cuda or self.training:
            return [f(x, record_len, affine, rows=rows) for f, x in zip(self.fusion_net, feature_list)]
        main = torch.cuda.current_stream(x0.device)
        side = self.__dict__.get("_fusion_streams")
        if side is None or len(side) != n - 1 or side[0].device != x0.device:
            side = self.__dict__["_fusion_streams"] = [torch.cuda.Stream(device=x0.device) for _ in range(n - 1)]
        fused = [None] * n
        for i in range(1, n):
            s = side[i - 1]
            s.wait_stream(main)
            with torch.cuda.stream(s):
                fused[i] = self.fusion_net[i](feature_list[i], record_len, affine, rows=rows)
            feature_list[i].record_stream(s)
            affine.record_stream(s)
        fused[0] = self.fusion_net[0](feature_list[0], record_len, affine, rows=rows)
        for i in range(1, n):
            main.wait_stream(side[i - 1])
            fused[i].record_stream(main)
        return fused

    def fuse_and_head(self, feature_list, record_len, affine, rows=None) -> dict:
        """Ego part: per-scale warp + fusion, deblocks, shrink header, heads.  ``rows``: see ``AttFusion.forward``."""
        fused = self._fuse_scales(feature_list, record_len, affine, rows)
        # round 5: a shrink header on the SplitMap route gets the concatenated map from the up-sampling heads already split
        want_split = bool(self.shrink_flag and len(fused) > 0 and all(getattr(m, "is_cuda", False) for m in fused) and self.shrink_conv.takes_split_maps())
        x = self.backbone.decode_multiscale_feature(fused, out_split=True) if want_split else self.backbone.decode_multiscale_feature(fused)
        if self.shrink_flag:
            x = self.shrink_conv(x, out_split=isinstance(x, ops.SplitMap) and heads_take_split_map(self))
        elif isinstance(x, ops.SplitMap):
            x = x.dense()
        return _run_heads(self, x)

    def forward(self, data_dict: dict) -> dict:
        record_len = host_ints(data_dict["record_len"])
        feats, affine = self.encode(dict(data_dict, record_len=record_len))
        return self.fuse_and_head(feats, record_len, affine)


class CoAlign(PointPillarBaselineMultiscale):
    pass


class PointPillar(nn.Module):
    """Single-agent PointPillar (late-fusion config)."""

    def __init__(self, args: dict):
        super().__init__()
        self.pillar_vfe = PillarVFE(args["pillar_vfe"], num_point_features=4, voxel_size=args["voxel_size"],
                                    point_cloud_range=args["lidar_range"])
        self.scatter = PointPillarScatter(args["point_pillar_scatter"])
        bb = args["base_bev_backbone"]
        self.backbone = ResNetBEVBackbone(bb, 64) if bb.get("resnet", False) else BaseBEVBackbone(bb, 64)
        self.out_channel = sum(bb["num_upsample_filter"])
        self.shrink_flag = "shrink_header" in args
        if self.shrink_flag:
            self.shrink_conv = DownsampleConv(args["shrink_header"])
            self.out_channel = args["shrink_header"]["dim"][-1]
        self.cls_head = nn.Conv2d(self.out_channel, args["anchor_number"], kernel_size=1)
        self.reg_head = nn.Conv2d(self.out_channel, 7 * args["anchor_number"], kernel_size=1)
        self.use_dir = "dir_args" in args
        if self.use_dir:
            self.dir_head = nn.Conv2d(self.out_channel, args["dir_args"]["num_bins"] * args["anchor_number"], kernel_size=1)

    def forward(self, data_dict: dict) -> dict:
        batch_dict = self.backbone(self.scatter(self.pillar_vfe(_single_agent_batch(data_dict))))
        x = batch_dict["spatial_features_2d"]
        if self.shrink_flag:
            x = self.shrink_conv(x)
        return _run_heads(self, x)


class PointPillarUncertainty(nn.Module):
    """Stage-1 single-agent detector of CoAlign's box alignment (opencood/models/point_pillar_uncertainty.py:15-84): PointPillar
    with a fourth 1x1 head ``unc_head`` predicting ``uncertainty_dim`` log-variances (x, y[, yaw]) per anchor."""

    def __init__(self, args: dict):
        super().__init__()
        self.pillar_vfe = PillarVFE(args["pillar_vfe"], num_point_features=4, voxel_size=args["voxel_size"],
                                    point_cloud_range=args["lidar_range"])
        self.scatter = PointPillarScatter(args["point_pillar_scatter"])
        self.backbone = BaseBEVBackbone(args["base_bev_backbone"], 64)
        self.uncertainty_dim = args["uncertainty_dim"]
        width = 128 * 3                                          # hard-coded in the reference (:26-37)
        self.cls_head = nn.Conv2d(width, args["anchor_number"], kernel_size=1)
        self.reg_head = nn.Conv2d(width, 7 * args["anchor_number"], kernel_size=1)
        self.unc_head = nn.Conv2d(width, self.uncertainty_dim * args["anchor_number"], kernel_size=1)
        self.use_dir = "dir_args" in args
        if self.use_dir:
            self.dir_head = nn.Conv2d(width, args["dir_args"]["num_bins"] * args["anchor_number"], kernel_size=1)

    def forward(self, data_dict: dict) -> dict:
        batch_dict = self.backbone(self.scatter(self.pillar_vfe(_single_agent_batch(data_dict))))
        return _run_heads(self, batch_dict["spatial_features_2d"])


class PointPillarDiscoNet(nn.Module):
    """DiscoNet on PointPillars (opencood/models/point_pillar_disconet.py:19-96): pillar encoder, ``BaseBEVBackbone``, shrink header, ONE single-scale
    ``DiscoFusion`` on the shrunk map, 1 x 1 heads.  Same constructor keys, ``state_dict`` names and outputs (``feature`` / ``cls_preds`` / ``reg_preds`` [/ ``dir_preds``])
    as the reference; the ``teacher_processed_lidar`` keys, which the reference's forward reads and never uses, are not required.  ``encode`` / ``fuse_and_head`` and
    the two ``accepts_*`` flags follow ``PointPillarBaselineMultiscale``'s contracts: ``FramePipeline`` and the inference drivers run it unchanged."""

    def __init__(self, args: dict):
        super().__init__()
        self.discrete_ratio = args["voxel_size"][0]
        self.pillar_vfe = PillarVFE(args["pillar_vfe"], num_point_features=4, voxel_size=args["voxel_size"],
                                    point_cloud_range=args["lidar_range"])
        self.scatter = PointPillarScatter(args["point_pillar_scatter"])
        self.backbone = BaseBEVBackbone(args["base_bev_backbone"], 64)
        self.out_channel = sum(args["base_bev_backbone"]["num_upsample_filter"])
        self.voxel_size = args["voxel_size"]
        self.shrink_flag = "shrink_header" in args
        if self.shrink_flag:
            self.shrink_conv = DownsampleConv(args["shrink_header"])
            self.out_channel = args["shrink_header"]["dim"][-1]
        self.fusion_net = DiscoFusion(self.out_channel)
        self.cls_head = nn.Conv2d(self.out_channel, args["anchor_number"], kernel_size=1)
        self.reg_head = nn.Conv2d(self.out_channel, 7 * args["anchor_number"], kernel_size=1)
        self.use_dir = "dir_args" in args
        if self.use_dir:
            self.dir_head = nn.Conv2d(self.out_channel, args["dir_args"]["num_bins"] * args["anchor_number"], kernel_size=1)

    accepts_normalized_affine = True      # encode() takes data_dict['normalized_affine_matrix'] in place of normalising pairwise_t_matrix itself
    accepts_pillar_frame = True           # encode() hands processed_lidar['pillar_frame'] to PillarVFE (whose dense-canvas route refuses it: FramePipeline then copies frames)

    def encode(self, data_dict: dict):
        """Per-agent part: pillars -> canvas -> backbone -> shrink header.  Returns ([the agents' maps, channels-last float32 on the SplitMap route], normalised affine)."""
        batch_dict = self.scatter(self.pillar_vfe(_single_agent_batch(dict(data_dict, record_len=host_ints(data_dict["record_len"])))))
        spatial_features = batch_dict["spatial_features"]
        H0, W0 = spatial_features.shape[2:]
        affine = data_dict.get("normalized_affine_matrix")
        if affine is None:
            affine = normalize_pairwise_tfm(data_dict["pairwise_t_matrix"], H0, W0, self.voxel_size[0])
        feats = self.backbone.get_multiscale_feature(spatial_features)
        # the up-sampling heads hand a shrink header on the SplitMap route ONE SplitMap; its second convolution (conv3x3_sp) writes the channels-last float32 map
        # the fusion kernel reads in place
        want_split = bool(self.shrink_flag and all(getattr(m, "is_cuda", False) for m in feats) and self.shrink_conv.takes_split_maps())
        x = self.backbone.decode_multiscale_feature(feats, out_split=True) if want_split else self.backbone.decode_multiscale_feature(feats)
        if self.shrink_flag:
            x = self.shrink_conv(x)
        elif isinstance(x, ops.SplitMap):
            x = x.dense()
        return [x], affine

    def fuse_and_head(self, feature_list, record_len, affine, rows=None) -> dict:
        """Ego part: the pixel-weight fusion of the agents' maps, then the heads on the fused map."""
        fused = self.fusion_net(feature_list[0], record_len, affine, rows=rows)
        return dict({"feature": fused}, **_run_heads(self, fused))

    def forward(self, data_dict: dict) -> dict:
        record_len = host_ints(data_dict["record_len"])
        feats, affine = self.encode(dict(data_dict, record_len=record_len))
        return self.fuse_and_head(feats, record_len, affine)


class PointPillarBaseline(nn.Module):
    """The single-scale collaborative baselines on PointPillars (opencood/models/point_pillar_baseline.py:17-138: F-Cooper, self-attention, DiscoNet without
    distillation, V2VNet, V2X-ViT, When2com): pillar encoder, ``BaseBEVBackbone`` or ``ResNetBEVBackbone``, shrink header, optional ``NaiveCompressor``, ONE fusion
    module on the shrunk map chosen by ``fusion_method`` (max | att | disconet | v2vnet | v2xvit | when2comm), 1 x 1 heads.  Same constructor keys, ``state_dict``
    names and outputs as the reference; ``v2xvit`` reads the ``v2xvit`` section and ``when2comm`` the ``when2comm`` section (without its section either is refused
    with ``NotImplementedError``); any other name is refused at construction -- the reference would build a model without ``fusion_net`` and fail in ``forward``.
    ``encode`` / ``fuse_and_head`` and the two ``accepts_*`` flags follow ``PointPillarDiscoNet``'s contracts: ``FramePipeline`` and the inference drivers run it
    unchanged.  The fusion receives the whole [L, L] affine matrix (V2VNet reads every receiver's row)."""

    def __init__(self, args: dict):
        super().__init__()
        self.pillar_vfe = PillarVFE(args["pillar_vfe"], num_point_features=4, voxel_size=args["voxel_size"],
                                    point_cloud_range=args["lidar_range"])
        self.scatter = PointPillarScatter(args["point_pillar_scatter"])
        bb = args["base_bev_backbone"]
        self.backbone = ResNetBEVBackbone(bb, 64) if bb.get("resnet", False) else BaseBEVBackbone(bb, 64)
        self.voxel_size = args["voxel_size"]
        method = args["fusion_method"]
        if method == "max":
            self.fusion_net = MaxFusion()
        elif method == "att":
            self.fusion_net = AttFusion(args["att"]["feat_dim"])
        elif method == "disconet":
            self.fusion_net = DiscoFusion(args["disconet"]["feat_dim"])
        elif method == "v2vnet":
            self.fusion_net = V2VNetFusion(args["v2vnet"])
        elif method == "v2xvit":
            if "v2xvit" not in args:
                raise NotImplementedError("fusion_method 'v2xvit' of point_pillar_baseline needs the model's 'v2xvit' section (the transformer's arguments), which this config lacks")
            self.fusion_net = V2XViTFusion(args["v2xvit"])
        elif method == "when2comm":
            if "when2comm" not in args:
                raise NotImplementedError("fusion_method 'when2comm' of point_pillar_baseline needs the model's 'when2comm' section (in_channels, H, W, query_size, key_size), which this config lacks")
            self.fusion_net = When2comFusion(args["when2comm"])
        else:
            raise NotImplementedError(f"fusion_method '{method}' of point_pillar_baseline is not built here (max | att | disconet | v2vnet | v2xvit | when2comm)")
        self.out_channel = sum(bb["num_upsample_filter"])
        self.shrink_flag = "shrink_header" in args
        if self.shrink_flag:
            self.shrink_conv = DownsampleConv(args["shrink_header"])
            self.out_channel = args["shrink_header"]["dim"][-1]
        self.compression = "compression" in args
        if self.compression:
            self.naive_compressor = NaiveCompressor(self.out_channel, args["compression"])
        self.cls_head = nn.Conv2d(self.out_channel, args["anchor_number"], kernel_size=1)
        self.reg_head = nn.Conv2d(self.out_channel, 7 * args["anchor_number"], kernel_size=1)
        self.use_dir = "dir_args" in args
        if self.use_dir:
            self.dir_head = nn.Conv2d(self.out_channel, args["dir_args"]["num_bins"] * args["anchor_number"], kernel_size=1)
        if args.get("backbone_fix"):
            self.backbone_fix()

    backbone_fix = PointPillarBaselineMultiscale.backbone_fix

    accepts_normalized_affine = True      # encode() takes data_dict['normalized_affine_matrix'] in place of normalising pairwise_t_matrix itself
    accepts_pillar_frame = True           # encode() hands processed_lidar['pillar_frame'] to PillarVFE (whose dense-canvas route refuses it: FramePipeline then copies frames)

    def encode(self, data_dict: dict):
        """Per-agent part: pillars -> canvas -> backbone -> shrink header (-> compressor).  Returns ([the agents' map], normalised affine)."""
        batch_dict = self.scatter(self.pillar_vfe(_single_agent_batch(dict(data_dict, record_len=host_ints(data_dict["record_len"])))))
        spatial_features = batch_dict["spatial_features"]
        H0, W0 = spatial_features.shape[2:]
        affine = data_dict.get("normalized_affine_matrix")
        if affine is None:
            affine = normalize_pairwise_tfm(data_dict["pairwise_t_matrix"], H0, W0, self.voxel_size[0])
        feats = self.backbone.get_multiscale_feature(spatial_features)
        # (a stride-1 shrink header on the SplitMap route takes ONE SplitMap from the up-sampling heads and writes channels-last float32, which the fusion reads in place)
        want_split = bool(self.shrink_flag and all(getattr(m, "is_cuda", False) for m in feats) and self.shrink_conv.takes_split_maps())
        x = self.backbone.decode_multiscale_feature(feats, out_split=True) if want_split else self.backbone.decode_multiscale_feature(feats)
        if self.shrink_flag:
            x = self.shrink_conv(x)
        elif isinstance(x, ops.SplitMap):
            x = x.dense()
        if self.compression:
            x = self.naive_compressor(x)
        return [x], affine

    def fuse_and_head(self, feature_list, record_len, affine, rows=None) -> dict:
        """Ego part: the fusion of the agents' maps, then the heads on the fused map."""
        return _run_heads(self, self.fusion_net(feature_list[0], record_len, affine, rows=rows))

    def forward(self, data_dict: dict) -> dict:
        record_len = host_ints(data_dict["record_len"])
        feats, affine = self.encode(dict(data_dict, record_len=record_len))
        return self.fuse_and_head(feats, record_len, affine)


MODEL_REGISTRY = {
    "point_pillar_baseline_multiscale": PointPillarBaselineMultiscale,
    "point_pillar_coalign": CoAlign,
    "point_pillar": PointPillar,
    "point_pillar_uncertainty": PointPillarUncertainty,
}

# Comparison baselines: the other collaborative detectors the reference ships in the same framework and CoAlign is measured against under pose noise.  ``build_model``
# constructs them like any model; they are NOT families of the CoAlign hot path, so ``routes.plan`` -- whose default walk answers "which of the reference's yamls does the
# CoAlign hot path serve" -- plans them only when asked to (``plan(hypes, baselines=True)``).
BASELINE_REGISTRY = {
    "point_pillar_disconet": PointPillarDiscoNet,
    "point_pillar_baseline": PointPillarBaseline,
}


def build_model(hypes: dict) -> nn.Module:
    """``train_utils.create_model`` for the hot-path model families and the comparison baselines (opencood/tools/train_utils.py:113-146):
    ``hypes['model']['core_method']`` names the model, ``hypes['model']['args']`` is its constructor argument."""
    name = hypes["model"]["core_method"]
    families = {**MODEL_REGISTRY, **BASELINE_REGISTRY}
    if name not in families:
        raise KeyError(f"model '{name}' is outside the CoAlign hot path and its baselines (available: {sorted(families)})")
    return families[name](hypes["model"]["args"])


def load_saved_model(saved_path: str, model: nn.Module):
    """``train_utils.load_saved_model`` (opencood/tools/train_utils.py:29-74): find the checkpoint of a training folder and load it into ``model``.

    * ``net_epoch_bestval_at<E>.pth`` present (exactly one is allowed) -> that file, returns ``(E, model)``;
    * else the highest ``net_epoch<E>.pth`` among ``*epoch*.pth`` -> that file, returns ``(E, model)``;
    * else nothing is loaded and ``(0, model)`` comes back.

    Like the reference: tensors are loaded onto the CPU (``map_location='cpu'``) and copied into whatever device the model lives on, ``strict=False`` (keys the
    model does not have are ignored, keys the file lacks keep their initial values), a missing folder is an ``AssertionError``.  Unlike the reference the epoch is
    parsed with a regular expression, never ``eval``-ed, and the file is read with ``weights_only=True`` (a ``state_dict`` holds tensors only)."""
    import glob
    import os
    import re
    assert os.path.exists(saved_path), "{} not found".format(saved_path)

    def load(path):
        try:
            sd = torch.load(path, map_location="cpu", weights_only=True)
        except TypeError:                       # (a torch without the keyword)
            sd = torch.load(path, map_location="cpu")
        model.load_state_dict(sd, strict=False)

    best = glob.glob(os.path.join(saved_path, "net_epoch_bestval_at*.pth"))
    if best:
        assert len(best) == 1
        m = re.fullmatch(r"net_epoch_bestval_at(\d+)\.pth", os.path.basename(best[0]))
        if m is None:
            raise ValueError(f"cannot read the epoch out of '{os.path.basename(best[0])}'")
        epoch = int(m.group(1))
        print("resuming best validation model at epoch %d" % epoch)
        load(best[0])
        return epoch, model
    epochs = []
    for f in glob.glob(os.path.join(saved_path, "*epoch*.pth")):
        m = re.search(r"epoch(\d+)\.pth", os.path.basename(f))
        if m is not None:
            epochs.append(int(m.group(1)))
    initial_epoch = max(epochs) if epochs else 0
    if initial_epoch > 0:
        print("resuming by loading epoch %d" % initial_epoch)
        load(os.path.join(saved_path, "net_epoch%d.pth" % initial_epoch))
    return initial_epoch, model


def to_device(inputs, device):
    """Recursive ``.to(device)`` over lists / dicts; non-tensors pass through (opencood/tools/train_utils.py:249-258)."""
    if isinstance(inputs, list):
        return [to_device(x, device) for x in inputs]
    if isinstance(inputs, dict):
        return {k: to_device(v, device) for k, v in inputs.items()}
    if isinstance(inputs, (int, float, str)) or inputs is None or not hasattr(inputs, "to"):
        return inputs
    return inputs.to(device)
