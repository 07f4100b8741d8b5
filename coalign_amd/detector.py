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
from .lss import LiftSplatShootIntermediate
from .second import SecondSSFA, SecondSSFAUncertainty
from .fusion import AttFusion, DiscoFusion, MaxFusion, V2VNetFusion, V2XViTFusion, When2comFusion, Where2commFusion, fuse_multiscale
from . import v2v_robust
from .pose import generate_noise_torch, get_pairwise_transformation_torch, normalize_pairwise_tfm
from .v2v_robust import AttentionWrapper, PoseRegressionWraper

ROBUST_MIN_MAP = v2v_robust.MIN_MAP

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


class _PillarTrunk(nn.Module):
    """What every detector here is built of: pillar encoder + scatter, a BEV backbone, an optional shrink header, the 1 x 1 heads.  The ``_build_*`` helpers register
    their submodules when CALLED: each model calls them in its own order, which fixes its ``state_dict`` order and the random numbers a seeded construction hands out."""

    def _build_pillars(self, args: dict) -> None:
        self.pillar_vfe = PillarVFE(args["pillar_vfe"], num_point_features=4, voxel_size=args["voxel_size"], point_cloud_range=args["lidar_range"])
        self.scatter = PointPillarScatter(args["point_pillar_scatter"])
        self.voxel_size = args["voxel_size"]

    def _build_backbone(self, args: dict, resnet: Optional[bool] = None) -> None:      # resnet: what a config without base_bev_backbone.resnet gets; None: BaseBEVBackbone whatever it says
        bb = args["base_bev_backbone"]
        self.backbone = ResNetBEVBackbone(bb, 64) if resnet is not None and bb.get("resnet", resnet) else BaseBEVBackbone(bb, 64)

    def _build_shrink(self, args: dict) -> None:
        self.out_channel = sum(args["base_bev_backbone"]["num_upsample_filter"])
        self.shrink_flag = "shrink_header" in args
        if self.shrink_flag:
            self.shrink_conv = DownsampleConv(args["shrink_header"])
            self.out_channel = args["shrink_header"]["dim"][-1]

    def _build_heads(self, args: dict, width: Optional[int] = None, uncertainty_dim: int = 0) -> None:
        width = self.out_channel if width is None else width
        self.cls_head = nn.Conv2d(width, args["anchor_number"], kernel_size=1)
        self.reg_head = nn.Conv2d(width, 7 * args["anchor_number"], kernel_size=1)
        if uncertainty_dim:
            self.unc_head = nn.Conv2d(width, uncertainty_dim * args["anchor_number"], kernel_size=1)
        self.use_dir = "dir_args" in args
        if self.use_dir:
            self.dir_head = nn.Conv2d(width, args["dir_args"]["num_bins"] * args["anchor_number"], kernel_size=1)

    def _frozen_parts(self) -> list:
        parts = [self.pillar_vfe, self.scatter, self.backbone, self.cls_head, self.reg_head]
        return parts + ([self.naive_compressor] if getattr(self, "compression", False) else []) + ([self.shrink_conv] if self.shrink_flag else [])

    def backbone_fix(self, frozen: bool = True) -> None:
        for m in self._frozen_parts():
            for p in m.parameters():
                p.requires_grad = not frozen

    def _single_agent_map(self, data_dict: dict) -> torch.Tensor:
        """The single-agent detectors' pillars -> canvas -> backbone -> concatenated up-sampled map."""
        return self.backbone(self.scatter(self.pillar_vfe(_single_agent_batch(data_dict))))["spatial_features_2d"]

    def _decode_shrink(self, feats, out_split: bool = False):
        """Up-sampling heads and shrink header.  A shrink header on the SplitMap route gets the concatenated map from the up-sampling heads as ONE SplitMap (round 5);
        its last convolution writes channels-last float32, which a fusion kernel reads in place, or -- ``out_split``, for a map that feeds the heads: the caller
        passes ``heads_take_split_map(self)`` -- a SplitMap again."""
        want_split = bool(self.shrink_flag and len(feats) > 0 and all(getattr(m, "is_cuda", False) for m in feats) and self.shrink_conv.takes_split_maps())
        x = self.backbone.decode_multiscale_feature(feats, out_split=True) if want_split else self.backbone.decode_multiscale_feature(feats)
        if self.shrink_flag:
            return self.shrink_conv(x, out_split=out_split and isinstance(x, ops.SplitMap))
        return x.dense() if isinstance(x, ops.SplitMap) else x


class _Collaborative(_PillarTrunk):
    """The detectors of several agents: ``encode`` (per agent) and ``fuse_and_head`` (ego) are exposed separately so the sharded runner can place them on different
    ranks; ``FramePipeline`` and the inference drivers run every subclass through the same two flags and two stages."""
    accepts_normalized_affine = True      # encode() takes data_dict['normalized_affine_matrix'] in place of normalising pairwise_t_matrix itself (FramePipeline)
    accepts_pillar_frame = True           # encode() hands processed_lidar['pillar_frame'] (ops.PillarFrameRecord) to PillarVFE, whose dense-canvas route refuses it: FramePipeline then copies frames
    plan_words_library_shrink = False     # routes.plan words a shrink-header convolution DoubleConv.forward builds no weight image for as a library layer (the single-scale baselines)

    def _spatial_features(self, data_dict: dict, want_affine: bool = True):
        """pillars -> canvas: what the backbone (or the compressor in front of it) reads, and the normalised affine."""
        batch_dict = _single_agent_batch(dict(data_dict, record_len=host_ints(data_dict["record_len"])))      # (with the device voxeliser's streaming keys and FramePipeline's frame record)
        # round 4: the encoder hands a SparseCanvas (one launch, no dense canvas) to a backbone whose first block, or a compressor whose encoder, reads it
        keep_sparse = getattr(self.pillar_vfe, "sparse_canvas", False)      # (False also for a stand-in encoder without the switch: the CPU tests of the baselines)
        self.pillar_vfe.sparse_canvas = sparse_canvas_route(self) or compressor_sparse_route(self)
        try:
            batch_dict = self.scatter(self.pillar_vfe(batch_dict))
        finally:
            self.pillar_vfe.sparse_canvas = keep_sparse
        spatial_features = batch_dict["spatial_features"]
        affine = data_dict.get("normalized_affine_matrix") if want_affine else None      # FramePipeline: normalised on the host from the dataset's host copy of the matrix (same float64 steps)
        if affine is None and want_affine:
            H0, W0 = spatial_features.shape[2:]
            affine = normalize_pairwise_tfm(data_dict["pairwise_t_matrix"], H0, W0, self.voxel_size[0])
        return spatial_features, affine

    def forward(self, data_dict: dict) -> dict:
        record_len = host_ints(data_dict["record_len"])
        feats, affine = self.encode(dict(data_dict, record_len=record_len))
        return self.fuse_and_head(feats, record_len, affine)


class PointPillarBaselineMultiscale(_Collaborative):
    def __init__(self, args: dict):
        super().__init__()
        self._build_pillars(args)
        self._build_backbone(args, resnet=True)
        self.fusion_net = nn.ModuleList()
        for i in range(len(args["base_bev_backbone"]["layer_nums"])):
            if args["fusion_method"] == "max":
                self.fusion_net.append(MaxFusion())
            elif args["fusion_method"] == "att":
                self.fusion_net.append(AttFusion(args["att"]["feat_dim"][i]))
            else:
                raise NotImplementedError(f"fusion_method '{args['fusion_method']}' is outside the CoAlign hot path (att | max)")
        self._build_shrink(args)
        self.compression = "compression" in args
        if self.compression:
            self.naive_compressor = NaiveCompressor(64, args["compression"])
        self._build_heads(args)
        if args.get("backbone_fix"):
            self.backbone_fix()

    def _level_channels(self) -> list:
        """The backbone's own widths, one per level."""
        resnet = getattr(self.backbone, "resnet", None)
        levels = [getattr(resnet, f"layer{i}") for i in range(resnet.layernum)] if resnet is not None else list(self.backbone.blocks)
        return [b[0].conv1.out_channels if isinstance(b[0], BasicBlock) else b[1].out_channels for b in levels]

    def plan_fusion(self, channels=None, terms: Optional[int] = None):
        """-> (``routes.plan``'s fusion line, whether it is a fallback, {layers noted with it})."""
        if _bb.NHWC_STAGE_OUTPUTS and _bb.emu_active(terms) and fusion_route(self, self._level_channels()):      # (channels-last stage outputs)
            return "warp_fuse_nhwc: all scales in one launch (channels-last)", False, {}
        return "warp_fuse: one launch per scale (NCHW, LDS-staged patches)", True, {}

    def encode(self, data_dict: dict):
        """Per-agent part: pillars -> canvas (-> compressor) -> multiscale features.  Returns (feature list, normalised affine)."""
        spatial_features, affine = self._spatial_features(data_dict)
        return self.backbone.get_multiscale_feature(self._compress(spatial_features)), affine

    def _compress(self, spatial_features):
        if not self.compression:
            return spatial_features
        # the compressor hands the first ResNet block a SplitMap when that block reads one: its strided opener + skip then run as one launch on it
        resnet = getattr(self.backbone, "resnet", None)
        opener = resnet.layer0[0] if resnet is not None and hasattr(resnet, "layer0") else None
        want_split = bool(not self.training and isinstance(opener, BasicBlock) and opener.takes_split_maps() and opener.conv1.in_channels % 16 == 0)
        return self.naive_compressor(spatial_features, out_split=True) if want_split else self.naive_compressor(spatial_features)

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
        return _run_heads(self, self._decode_shrink(fused, out_split=heads_take_split_map(self)))


class CoAlign(PointPillarBaselineMultiscale):
    pass


class PointPillar(_PillarTrunk):
    """Single-agent PointPillar (late-fusion config)."""

    def __init__(self, args: dict):
        super().__init__()
        self._build_pillars(args)
        self._build_backbone(args, resnet=False)
        self._build_shrink(args)
        self._build_heads(args)

    def forward(self, data_dict: dict) -> dict:
        x = self._single_agent_map(data_dict)
        return _run_heads(self, self.shrink_conv(x) if self.shrink_flag else x)


class PointPillarUncertainty(_PillarTrunk):
    """Stage-1 single-agent detector of CoAlign's box alignment (opencood/models/point_pillar_uncertainty.py:15-84): PointPillar
    with a fourth 1x1 head ``unc_head`` predicting ``uncertainty_dim`` log-variances (x, y[, yaw]) per anchor."""

    def __init__(self, args: dict):
        super().__init__()
        self._build_pillars(args)
        self._build_backbone(args)
        self.uncertainty_dim = args["uncertainty_dim"]
        self._build_heads(args, width=128 * 3, uncertainty_dim=self.uncertainty_dim)      # (the width is hard-coded in the reference, :26-37)

    def forward(self, data_dict: dict) -> dict:
        return _run_heads(self, self._single_agent_map(data_dict))


class PointPillarDiscoNet(_Collaborative):
    """DiscoNet on PointPillars (opencood/models/point_pillar_disconet.py:19-96): pillar encoder, ``BaseBEVBackbone``, shrink header, ONE single-scale
    ``DiscoFusion`` on the shrunk map, 1 x 1 heads.  Same constructor keys, ``state_dict`` names and outputs (``feature`` / ``cls_preds`` / ``reg_preds`` [/ ``dir_preds``])
    as the reference; the ``teacher_processed_lidar`` keys, which the reference's forward reads and never uses, are not required.  ``encode`` / ``fuse_and_head`` and
    the two ``accepts_*`` flags follow ``PointPillarBaselineMultiscale``'s contracts: ``FramePipeline`` and the inference drivers run it unchanged."""

    def __init__(self, args: dict):
        super().__init__()
        self.discrete_ratio = args["voxel_size"][0]
        self._build_pillars(args)
        self._build_backbone(args)
        self._build_shrink(args)
        self.fusion_net = DiscoFusion(self.out_channel)
        self._build_heads(args)

    def encode(self, data_dict: dict):
        """Per-agent part: pillars -> canvas -> backbone -> shrink header.  Returns ([the agents' maps, channels-last float32 on the SplitMap route], normalised affine)."""
        spatial_features, affine = self._spatial_features(data_dict)
        return [self._decode_shrink(self.backbone.get_multiscale_feature(spatial_features))], affine

    def fuse_and_head(self, feature_list, record_len, affine, rows=None) -> dict:
        """Ego part: the pixel-weight fusion of the agents' maps, then the heads on the fused map."""
        fused = self.fusion_net(feature_list[0], record_len, affine, rows=rows)
        return dict({"feature": fused}, **_run_heads(self, fused))


class PointPillarBaseline(_Collaborative):
    """The single-scale collaborative baselines on PointPillars (opencood/models/point_pillar_baseline.py:17-138: F-Cooper, self-attention, DiscoNet without
    distillation, V2VNet, V2X-ViT, When2com): pillar encoder, ``BaseBEVBackbone`` or ``ResNetBEVBackbone``, shrink header, optional ``NaiveCompressor``, ONE fusion
    module on the shrunk map chosen by ``fusion_method`` (max | att | disconet | v2vnet | v2xvit | when2comm), 1 x 1 heads.  Same constructor keys, ``state_dict``
    names and outputs as the reference; ``v2xvit`` reads the ``v2xvit`` section and ``when2comm`` the ``when2comm`` section (without its section either is refused
    with ``NotImplementedError``); any other name is refused at construction -- the reference would build a model without ``fusion_net`` and fail in ``forward``.
    ``encode`` / ``fuse_and_head`` and the two ``accepts_*`` flags follow ``PointPillarDiscoNet``'s contracts: ``FramePipeline`` and the inference drivers run it
    unchanged.  The fusion receives the whole [L, L] affine matrix (V2VNet reads every receiver's row)."""
    plan_words_library_shrink = True

    def __init__(self, args: dict):
        super().__init__()
        self._build_pillars(args)
        self._build_backbone(args, resnet=False)
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
        self._build_shrink(args)
        self.compression = "compression" in args
        if self.compression:
            self.naive_compressor = NaiveCompressor(self.out_channel, args["compression"])
        self._build_heads(args)
        if args.get("backbone_fix"):
            self.backbone_fix()

    def encode(self, data_dict: dict):
        """Per-agent part: pillars -> canvas -> backbone -> shrink header (-> compressor).  Returns ([the agents' map], normalised affine)."""
        spatial_features, affine = self._spatial_features(data_dict)
        x = self._decode_shrink(self.backbone.get_multiscale_feature(spatial_features))
        return [self.naive_compressor(x) if self.compression else x], affine

    def fuse_and_head(self, feature_list, record_len, affine, rows=None) -> dict:
        """Ego part: the fusion of the agents' maps, then the heads on the fused map."""
        return _run_heads(self, self.fusion_net(feature_list[0], record_len, affine, rows=rows))


class PointPillarWhere2comm(PointPillarBaselineMultiscale):
    """Where2comm on PointPillars.  THIS MODEL CLASS IS THIS PROJECT'S: the reference snapshot ships the fusion module (``Where2comm``,
    opencood/models/fuse_modules/where2comm_attn.py:174-341, with ``Communication``, opencood/models/comm_modules/where2comm.py:9-78) and neither a model class nor
    a yaml that constructs it.  Layout and constructor keys are ``PointPillarBaselineMultiscale``'s -- pillar encoder, ``ResNetBEVBackbone`` or ``BaseBEVBackbone``,
    optional shrink header and compressor, 1 x 1 heads -- with a ``where2comm`` section (the module's argument dict) in place of ``fusion_method``; ``fusion_net`` is
    ONE ``fusion.Where2commFusion``.

    Forward: every agent's multi-scale maps; decode, shrink header and ``cls_head`` on EVERY agent give the single-agent logits the masks are made of;
    ``multi_scale: true``: masked fusion of the backbone's levels, then decode, shrink header and heads on the fused map; otherwise: masked fusion of the agents'
    shrunk maps, then the heads.  Output: the other models' dict plus ``comm_rates``, a 0-d device tensor.  ``encode`` / ``fuse_and_head`` and the two ``accepts_*``
    flags keep ``PointPillarBaselineMultiscale``'s contracts; the single-agent logits travel as the LAST entry of the feature list.

    ``packed_wire`` (False; settable on the class, an instance, or by the model arguments' optional ``packed_wire`` key): ``fuse_and_head`` goes through MESSAGES --
    every non-ego agent's masked pixels packed into a ``where2comm.W2Message``, the fusion reading the ego's dense maps and the messages -- to the same heads, and the
    output gains ``messages`` (per frame, the list of its non-ego agents' messages) and ``comm_bytes`` (a 0-d int64 device tensor: the messages' sizes summed on the
    device from their counts).  A route the message kernels do not serve raises; nothing falls back.  With the flag off nothing differs, ``state_dict`` included."""
    packed_wire = False

    def __init__(self, args: dict):
        if "where2comm" not in args:
            raise NotImplementedError("point_pillar_where2comm needs the model's 'where2comm' section (the arguments of the Where2comm module), which this config lacks")
        super().__init__(dict(args, fusion_method="max"))          # (the parent's per-level list of parameter-free modules is replaced right below)
        del self.fusion_net
        self.fusion_net = Where2commFusion(args["where2comm"])
        self.multi_scale = bool(self.fusion_net.multi_scale)
        if "packed_wire" in args:
            self.packed_wire = bool(args["packed_wire"])
        if self.multi_scale and self.fusion_net.num_levels != self.backbone.num_levels:
            raise ValueError(f"where2comm.layer_nums names {self.fusion_net.num_levels} levels, the backbone has {self.backbone.num_levels}")

    def _route_args(self, n_agents: int):      # the module decides on this model's widths, backbone kind and anchor count
        return self._level_channels() if self.multi_scale else [self.out_channel], n_agents, hasattr(self.backbone, "resnet"), self.cls_head.out_channels

    def kernel_route(self, n_agents: int = 1) -> bool:
        """The static half of the fusion's decision (``routes.plan`` asks it)."""
        return self.fusion_net.kernel_route(*self._route_args(n_agents))

    def kernel_route_reason(self, n_agents: int = 1) -> Optional[str]:
        """Why ``kernel_route`` says no, in words (None when it says yes, or for the module's mode alone)."""
        return self.fusion_net.kernel_shape_reason(*self._route_args(n_agents))

    def plan_fusion(self, channels=None, terms: Optional[int] = None):
        """-> (``routes.plan``'s fusion line, whether it is a fallback, {layers noted with it})."""
        f = self.fusion_net
        if self.kernel_route() and (not f.multi_scale or (_bb.NHWC_STAGE_OUTPUTS and _bb.emu_active(terms))):      # (channels-last stage outputs)
            if self.packed_wire:          # (served only with a communication section; otherwise the refusal, in the words ``fuse`` raises with)
                reason = f.packed_route_reason(*self._route_args(1))
                return (f.KERNELS_PACKED, False, {}) if reason is None else (f"packed wire refused ({reason})", True, {})
            return (f.KERNELS if f.communication else f.KERNELS_PLAIN), False, {}
        if self.packed_wire:
            return f"packed wire refused ({f.packed_route_reason(*self._route_args(1)) or 'stage outputs not channels-last, ' + _bb.TORCH_MODE})", True, {}
        return f"{f.TORCH} ({self.kernel_route_reason() or 'stage outputs not channels-last, ' + _bb.TORCH_MODE})", True, {}

    def plan_layer(self, name: str, layer: nn.Module, channels=None, terms: Optional[int] = None):
        """-> (line, fallback) of ``naive_communication.gaussian_filter``."""
        if not isinstance(layer, nn.Conv2d):
            return None
        ok = self.kernel_route()
        return (self.fusion_net.MASKS if ok else _bb.MIOPEN + " (Where2comm op by op)"), not ok

    def encode(self, data_dict: dict):
        """Per-agent part.  Returns ([the maps the fusion reads ..., the single-agent logits], normalised affine): the backbone's levels in multi-scale mode on a
        backbone with ``.resnet``, the canvas on a plain ``BaseBEVBackbone`` (whose later blocks read the MASKED maps, where2comm_attn.py:262), else the shrunk map."""
        spatial_features, affine = self._spatial_features(data_dict)
        spatial_features = self._compress(spatial_features)
        feats = self.backbone.get_multiscale_feature(spatial_features)
        x = self._decode_shrink(feats)          # (for the logits and the single-scale fusion: a float32 map)
        psm = _run_heads(self, x)["cls_preds"]
        if not self.multi_scale:
            return [x, psm], affine
        if hasattr(self.backbone, "resnet"):
            return [*feats, psm], affine
        return [spatial_features.dense() if isinstance(spatial_features, (ops.SparseCanvas, ops.SplitMap)) else spatial_features, psm], affine

    def fuse_and_head(self, feature_list, record_len, affine, rows=None) -> dict:
        """Ego part: the masked fusion, (decode and shrink header,) the heads."""
        *maps, psm = feature_list
        wire, messages = ("packed" if self.packed_wire else "dense"), None
        if not self.multi_scale:
            x, rates, extra = self.fusion_net.fuse(maps[0], psm, record_len, affine, rows=rows, wire=wire)
            messages = extra.get("messages")
        elif hasattr(self.backbone, "resnet"):
            fused, rates, *sent = self.fusion_net.fuse(None, psm, record_len, affine, self.backbone, feats=maps, rows=rows, decode=False, wire=wire)
            messages = sent[0] if sent else None
            x = self._decode_shrink(fused, out_split=heads_take_split_map(self)) if isinstance(fused, list) else self._shrink_decoded(fused)
        else:
            x, rates, extra = self.fusion_net.fuse(maps[0], psm, record_len, affine, self.backbone, rows=rows, wire=wire)
            messages = extra.get("messages")
            x = self._shrink_decoded(x)
        out = _run_heads(self, x)
        out["comm_rates"] = torch.as_tensor(rates, device=psm.device)
        if self.packed_wire:
            out["messages"] = messages
            out["comm_bytes"] = sum((m.nbytes_device() for frame in messages for m in frame), torch.zeros((), dtype=torch.int64, device=psm.device))
        return out

    def _shrink_decoded(self, x):
        return self.shrink_conv(x) if self.shrink_flag else x


class PointPillarV2VNetRobust(_Collaborative):
    """V2VNet with learned pose correction (opencood/models/point_pillar_v2vnet_robust.py:21-332), the baseline CoAlign is compared with under pose noise: pillar
    encoder, ``BaseBEVBackbone``, shrink header, optional ``NaiveCompressor(256, rate)`` when the integer ``compression`` > 0, then on the shrunk maps the pose
    regression over all pairs (``pose_reg_net``), the globally consistent poses (``v2v_robust.weighted_em``), the attention scores (``attention_net``, with
    ``attention_net.alpha``) and ``V2VNetFusion`` with ``agg_operator: weight``, 1 x 1 heads.  Same constructor keys, members, ``state_dict`` names and output keys
    as the reference; its ``self.apply(weight_init)`` is not mirrored.

    ``forward`` follows ``train_forward`` for ``stage`` 0 / 1 / 2.  Quirks of the reference, kept as they are:
      * ``forward`` ALWAYS runs ``train_forward``: noise is added to the poses in eval mode too (stage 0: strong or weak per agent; stages 1 and 2: strong);
        ``eval_forward`` exists and is never called by ``forward``;
      * the rotation noise is a von Mises sample in RADIANS added to a yaw in degrees (``pose.generate_noise_torch``);
      * ``get_intersection`` warps a tensor of zeros: the intersection is 0.01 whatever the poses;
      * ``weighted_mle`` sees the INPUT poses in every one of the ten rounds, only the weights change;
      * both wrappers warp to (robust.H, robust.W) but normalise the translation by the map's own H, W;
      * stage 1 returns no ``cls_preds``: its outputs are ``pairwise_corr`` and ``pairwise_t_matrix`` only.
    NOT kept: the reference adds the noise to the caller's ``lidar_pose`` in place; here the caller's tensor is left untouched.
    Extension: ``data_dict['pose_noise']`` [n, 6] (and ``data_dict['noise_choice']`` [n, 1] for stage 0) replaces the drawn noise -- a run becomes repeatable, and
    zeros give ``eval_forward``'s arithmetic.

    Maps whose H, W differ from robust.H, robust.W, or lie below 24 x 24 (the smallest map the regression's pooling accepts), are refused with
    ``NotImplementedError``.  Three routes: ``forward_torch`` (the reference op by op), ``forward_reduced`` (the exact identities of ``v2v_robust`` and
    ``V2VNetFusion.forward_reduced`` in torch ops), ``forward_kernels`` (CUDA float32 in eval mode when ``kernel_route`` holds; ``force_torch`` is the test aid)."""
    accepts_normalized_affine = accepts_pillar_frame = False      # (its ``encode`` returns the maps alone and ``forward`` reads the poses: no pipeline stage pair)
    plan_words_library_shrink = True
    plan_prefixes = ("pose_reg_net.", "attention_net.", "fusion_net.")      # the submodules ``plan_layer`` words: ONE decision serves the three parts

    def __init__(self, args: dict):
        super().__init__()
        self.max_cav = args["max_cav"]
        self._build_pillars(args)
        self._build_backbone(args)
        self._build_shrink(args)
        self.compression = args.get("compression", 0) > 0
        if self.compression:
            self.naive_compressor = NaiveCompressor(256, args["compression"])
        self.fusion_net = V2VNetFusion(args["v2vfusion"])
        self.fusion_downsample_rate, self.fusion_discrete_ratio = args["v2vfusion"]["downsample_rate"], args["v2vfusion"]["voxel_size"][0]
        self._build_heads({k: v for k, v in args.items() if k != "dir_args"})      # (no direction head, whatever the config says)
        robust = args["robust"]
        self.downsample_rate, self.discrete_ratio, self.H, self.W = robust["downsample_rate"], robust["discrete_ratio"], robust["H"], robust["W"]
        self.affine_parameter = {"H": self.H, "W": self.W, "downsample_rate": self.downsample_rate, "discrete_ratio": self.discrete_ratio}
        self.pose_reg_net = PoseRegressionWraper(robust["feature_dim"] * 2, robust["hidden_dim"], self.affine_parameter)
        self.attention_net = AttentionWrapper(robust["feature_dim"] * 2, robust["hidden_dim"], self.affine_parameter, robust.get("learnable_alpha", True))
        self.stage = args["stage"]
        self.force_torch = False      # measurement / test aid: take the op-by-op route whatever the device
        if self.stage == 1:
            self.backbone_fix()
        if self.stage == 2:
            self.backbone_unfix()

    def _frozen_parts(self) -> list:
        """Stage 1 trains the pose regression alone: everything else is frozen (point_pillar_v2vnet_robust.py:81-110)."""
        return super()._frozen_parts() + [self.fusion_net, self.attention_net]

    def backbone_unfix(self) -> None:
        self.backbone_fix(False)

    # ---- encoder -------------------------------------------------------------------------------------------------------------------------------------------
    def encode(self, data_dict: dict) -> torch.Tensor:
        """Per-agent part: pillars -> canvas -> backbone -> shrink header (-> compressor): the agents' maps [N, C, H, W]."""
        spatial_features, _ = self._spatial_features(data_dict, want_affine=False)
        x = self._decode_shrink(self.backbone.get_multiscale_feature(spatial_features))
        return self.naive_compressor(x) if self.compression else x

    # ---- noise ---------------------------------------------------------------------------------------------------------------------------------------------
    def noise_generator(self, lidar_pose: torch.Tensor, all_strong: bool = False):
        """(noise [N, 6], choice [N, 1]: 0 strong (0.4 m, 4 deg), 1 weak (0.01 m, 0.1 deg)) (point_pillar_v2vnet_robust.py:190-202)."""
        noise_s = generate_noise_torch(lidar_pose, pos_std=0.4, rot_std=4)
        noise_w = generate_noise_torch(lidar_pose, pos_std=0.01, rot_std=0.1)
        N = lidar_pose.shape[0]
        if all_strong:
            return noise_s, torch.zeros((N, 1), device=lidar_pose.device)
        choice = torch.randint(0, 2, (N, 1), device=lidar_pose.device)
        return choice * noise_w + (1 - choice) * noise_s, choice

    # ---- routes --------------------------------------------------------------------------------------------------------------------------------------------
    def _check_map(self, x: torch.Tensor) -> None:
        H, W = x.shape[2:]
        if (H, W) != (self.H, self.W):
            raise NotImplementedError(f"point_pillar_v2vnet_robust: the shrunk map is {H} x {W} but robust.H x robust.W is {self.H} x {self.W}")
        if H < ROBUST_MIN_MAP or W < ROBUST_MIN_MAP:
            raise NotImplementedError(f"point_pillar_v2vnet_robust: a {H} x {W} map is below {ROBUST_MIN_MAP} x {ROBUST_MIN_MAP}, the smallest the pose regression's pooling accepts")

    def one_normalisation(self) -> bool:
        """The three warps (pose regression, attention, fusion) normalise alike: ONE affine per pose set serves them, and one warp the attention and the fusion."""
        return float(self.fusion_downsample_rate) * float(self.fusion_discrete_ratio) == float(self.downsample_rate) * float(self.discrete_ratio)

    def kernel_shape_reason(self, channels: int, n_agents: int = 1, terms: Optional[int] = None) -> Optional[str]:
        """None when the three parts' kernels take (channels, n_agents) in the arithmetic in force, else why not, in words (``routes.plan`` prints it)."""
        if not self.one_normalisation():
            return "the three warps normalise differently (robust vs v2vfusion downsample_rate x discrete_ratio)"
        nets = (self.pose_reg_net, self.attention_net)
        widths = next((w for w in (net.widths_reason(channels) for net in nets) if w is not None), None)
        if widths is not None or (self.fusion_net.kernel_shape_reason(channels, n_agents, terms) is None
                                  and all(net.kernel_shape_reason(channels, n_agents, terms, self.max_cav) is None for net in nets)):
            return widths
        return "the fusion's own conditions (3 x 3 GRU kernels, widths) or the SplitMap arithmetic (fp16 x 2) is not in force"

    def kernel_route(self, channels: int, n_agents: int = 1, terms: Optional[int] = None) -> bool:
        """The static half of the decision (``routes.plan`` asks it): the fusion's, both small nets' and the shapes' conditions; ``forward`` adds a CUDA float32 map."""
        parts = (self, self.fusion_net, self.pose_reg_net, self.attention_net)      # (each part's own mode and ``force_torch`` count, as in its own ``kernel_route``)
        return bool(not any(m.training or m.force_torch for m in parts) and self.kernel_shape_reason(channels, n_agents, terms) is None)

    def plan_fusion(self, channels: int, terms: Optional[int] = None):
        """-> (``routes.plan``'s fusion line, whether it is a fallback, {layers noted with it}): pose regression, EM, attention and the weighted V2VNet on the shrunk map."""
        ok = self.kernel_route(channels, 1, terms)
        line = v2v_robust.KERNELS if ok else f"{v2v_robust.TORCH} ({self.kernel_shape_reason(channels, 1, terms) or _bb.TORCH_MODE})"
        return line, not ok, self.fusion_net.plan_mlp(terms, ok)

    def plan_layer(self, name: str, layer: nn.Module, channels: int, terms: Optional[int] = None):
        """-> (line, fallback) of a convolution or linear of the three parts: the model's forward takes the kernels for all of them or for none."""
        ok = self.kernel_route(channels, 1, terms)
        if name.startswith("fusion_net."):
            return self.fusion_net.plan_layer(name, layer, channels, terms, ok)
        return (self.pose_reg_net if name.startswith("pose_reg_net.") else self.attention_net).plan_layer(name, layer, terms, ok)

    def _fusion_affine(self, T: torch.Tensor, H: int, W: int) -> torch.Tensor:
        return normalize_pairwise_tfm(T, H, W, self.fusion_discrete_ratio, self.fusion_downsample_rate)

    def _stages(self, x: torch.Tensor, groups, pose3: torch.Tensor, stage: int, reduced: bool) -> dict:
        """train_forward after the noise, in torch ops: ``reduced`` picks every part's ``forward_reduced`` and the constant intersection."""
        H, W = x.shape[2:]
        L = max(self.max_cav, max(groups))
        reg = self.pose_reg_net.forward_reduced if reduced else self.pose_reg_net.forward_torch
        att = self.attention_net.forward_reduced if reduced else self.attention_net.forward_torch
        fuse = self.fusion_net.forward_reduced if reduced else self.fusion_net.forward_torch
        T = get_pairwise_transformation_torch(pose3, L, groups, dof=3)
        out = {"stage": stage}
        if stage in (1, 2):
            out["pairwise_corr"], T_new = reg(x, groups, T)
            out["pairwise_t_matrix"], out["pairwise_t_matrix_new"] = T, T_new
        if stage == 1:
            return out
        if stage == 2:
            poses, off = [], 0
            for b, n in enumerate(groups):
                p = pose3[off:off + n]
                off += n
                if n > 1:
                    inter = v2v_robust.constant_intersection(T_new[b]) if reduced else v2v_robust.get_intersection(T_new[b], self.affine_parameter)
                    p = v2v_robust.weighted_em(p, T_new[b], inter)
                poses.append(p)
            out["lidar_pose_corrected"] = torch.cat(poses, dim=0)
            T = get_pairwise_transformation_torch(out["lidar_pose_corrected"], L, groups, dof=3)
        out["scores"], weight = att(x, groups, T)
        fused = fuse(x, groups, self._fusion_affine(T, H, W), weight)
        return dict(out, weight=weight, **_run_heads(self, fused))

    def forward_torch(self, x: torch.Tensor, record_len, pose3: torch.Tensor, stage: Optional[int] = None) -> dict:
        self._check_map(x)
        return self._stages(x, host_ints(record_len), pose3, self.stage if stage is None else stage, False)

    def forward_reduced(self, x: torch.Tensor, record_len, pose3: torch.Tensor, stage: Optional[int] = None) -> dict:
        self._check_map(x)
        return self._stages(x, host_ints(record_len), pose3, self.stage if stage is None else stage, True)

    def forward_kernels(self, x: torch.Tensor, record_len, pose3: torch.Tensor, stage: Optional[int] = None) -> dict:
        """The same on the gfx950 kernels, frame by frame; nothing returns to the host between the maps and the head outputs (capturable)."""
        self._check_map(x)
        groups = host_ints(record_len)
        stage = self.stage if stage is None else stage
        C, H, W = x.shape[1:]
        L = max(self.max_cav, max(groups))
        den_x, den_y = self.downsample_rate * self.discrete_ratio * W, self.downsample_rate * self.discrete_ratio * H
        if not ops.nhwc_memory(x):
            x = x.contiguous(memory_format=torch.channels_last)
        per = {k: [] for k in ("pairwise_corr", "pairwise_t_matrix", "pairwise_t_matrix_new", "lidar_pose_corrected", "scores", "weight", "fused")}
        off = 0
        for b, n in enumerate(groups):
            xb = x[off:off + n]
            poses = pose3[off:off + n].to(torch.float64).contiguous()
            off += n
            T, theta = ops.v2vr_pairwise(poses, L, H, W, den_x, den_y)
            per["pairwise_t_matrix"].append(T)
            warped = ops.v2v_warp_split(xb, theta[:n, :n])
            if stage in (1, 2):
                corr, T_new = self.pose_reg_net.forward_kernels(xb, warped, T)
                per["pairwise_corr"].append(corr)
                per["pairwise_t_matrix_new"].append(T_new)
            if stage == 1:
                continue
            if stage == 2:
                fixed, T, theta = ops.v2vr_consistency(poses, T_new, H, W, den_x, den_y)
                per["lidar_pose_corrected"].append(fixed)
                warped = ops.v2v_warp_split(xb, theta[:n, :n])
            scores, weight = self.attention_net.forward_kernels(xb, warped, L)
            per["scores"].append(scores)
            per["weight"].append(weight)
            per["fused"].append(self.fusion_net.forward_kernels(xb, [n], theta.unsqueeze(0), weight.unsqueeze(0), first_warp=[warped]))      # identity (c): one warp
        out = {"stage": stage}
        if stage in (1, 2):
            out["pairwise_corr"] = torch.stack(per["pairwise_corr"])
            out["pairwise_t_matrix"], out["pairwise_t_matrix_new"] = torch.stack(per["pairwise_t_matrix"]).float(), torch.stack(per["pairwise_t_matrix_new"]).float()
        if stage == 1:
            return out
        if stage == 2:
            out["lidar_pose_corrected"] = torch.cat(per["lidar_pose_corrected"], dim=0).to(pose3.dtype)
        out["scores"], out["weight"] = torch.stack(per["scores"]), torch.stack(per["weight"])
        fused = per["fused"][0] if len(per["fused"]) == 1 else torch.cat(per["fused"], dim=0)
        return dict(out, **_run_heads(self, fused))

    # ---- the reference's entry points ----------------------------------------------------------------------------------------------------------------------
    def _route(self, x: torch.Tensor, record_len, pose3: torch.Tensor, stage: int) -> dict:
        groups = host_ints(record_len)
        if x.is_cuda and x.dtype == torch.float32 and sum(groups) == x.shape[0] and self.kernel_route(x.shape[1], max(groups)):
            return self.forward_kernels(x, groups, pose3, stage)
        return self.forward_torch(x, groups, pose3, stage)

    def train_forward(self, spatial_features_2d: torch.Tensor, record_len, lidar_pose: torch.Tensor, pairwise_t_matrix=None, noise=None, choice=None) -> dict:
        """point_pillar_v2vnet_robust.py:205-267.  ``pairwise_t_matrix`` is accepted and, like in the reference, never read: the matrices come from the noisy poses."""
        stage = self.stage
        if noise is None:
            noise, choice = self.noise_generator(lidar_pose, all_strong=stage != 0)
        elif choice is None:
            choice = torch.zeros((lidar_pose.shape[0], 1), device=lidar_pose.device)
        noisy = lidar_pose + noise.to(lidar_pose)                                      # (a copy: the reference's ``lidar_pose += noise`` changes the caller's tensor)
        pose3 = noisy[:, [0, 1, 4]].to(spatial_features_2d.dtype)
        out = self._route(spatial_features_2d, record_len, pose3, stage)
        keys = {0: ("stage", "scores", "cls_preds", "reg_preds"), 1: ("stage", "pairwise_corr", "pairwise_t_matrix"),
                2: ("stage", "scores", "cls_preds", "reg_preds", "pairwise_corr", "pairwise_t_matrix")}[stage]
        out = {k: out[k] for k in keys}
        if stage == 0:
            out["choice"] = choice
        return out

    def eval_forward(self, spatial_features_2d: torch.Tensor, record_len, lidar_pose: torch.Tensor, pairwise_t_matrix=None) -> dict:
        """Stage 2 without noise (point_pillar_v2vnet_robust.py:271-295); its ``pairwise_t_matrix`` is the regressed one, as in the reference.  Not called by ``forward``."""
        pose3 = lidar_pose[:, [0, 1, 4]].to(spatial_features_2d.dtype)
        out = self._route(spatial_features_2d, record_len, pose3, 2)
        return {"stage": self.stage, "scores": out["scores"], "cls_preds": out["cls_preds"], "reg_preds": out["reg_preds"], "pairwise_t_matrix": out["pairwise_t_matrix_new"]}

    def forward(self, data_dict: dict) -> dict:
        record_len = host_ints(data_dict["record_len"])
        x = self.encode(dict(data_dict, record_len=record_len))
        return self.train_forward(x, record_len, data_dict["lidar_pose"], data_dict.get("pairwise_t_matrix"), noise=data_dict.get("pose_noise"), choice=data_dict.get("noise_choice"))


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
    "point_pillar_v2vnet_robust": PointPillarV2VNetRobust,
    "point_pillar_where2comm": PointPillarWhere2comm,
}

# The camera model (coalign_amd.lss): Lift-Splat frustum pooling in front of the multi-scale BEV fusion.  It has no pillar trunk, so ``routes.plan`` does not walk it.
CAMERA_REGISTRY = {
    "lift_splat_shoot_intermediate": LiftSplatShootIntermediate,
}

# CoAlign's second stage-1 detector family (coalign_amd.second): SECOND on the sparse 3-D trunk of coalign_amd.sparse3d with the SSFA neck.  No pillar trunk: ``routes.plan``
# does not walk it; ``sparse3d.plan`` words its trunk.
SECOND_REGISTRY = {
    "second_ssfa": SecondSSFA,
    "second_ssfa_uncertainty": SecondSSFAUncertainty,
}


def build_model(hypes: dict) -> nn.Module:
    """``train_utils.create_model`` for the hot-path model families and the comparison baselines (opencood/tools/train_utils.py:113-146):
    ``hypes['model']['core_method']`` names the model, ``hypes['model']['args']`` is its constructor argument."""
    name = hypes["model"]["core_method"]
    families = {**MODEL_REGISTRY, **BASELINE_REGISTRY, **CAMERA_REGISTRY, **SECOND_REGISTRY}
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
