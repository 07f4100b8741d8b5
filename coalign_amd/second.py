"""CoAlign's second stage-1 detector family: SECOND with the SSFA neck (opencood/models/second_ssfa.py, second_ssfa_uncertainty.py).

``MeanVFE`` -> ``VoxelBackBone8x`` -> ``HeightCompression`` (coalign_amd.sparse3d: the gfx950 kernels of csrc/sparse_conv3d.hip, or torch ops) -> ``SSFA`` ->
shrink header -> heads.  ``SSFA`` and ``Head`` keep the reference's parameter names.  By default they are torch ops; with ``COALIGN_SSFA=1`` (``SSFA.neck_kernels``,
off by default) an eval-mode float32 CUDA map takes the kernel route of DESIGN.md section 8n-2: the 3 x 3 convolutions on ``ops.conv3x3_sp`` / ``ops.conv3x3_sp_s2``,
``trans_0`` / ``trans_1`` on the pointwise kernel, the transposed convolutions on ``ops.deconv3x3_s2_sp``, the blend on ``ops.ssfa_blend``, the shrink header on SplitMaps
and the heads as one ``ops.heads_sp`` launch.  ``SecondSSFAUncertainty`` emits the four head maps of ``PointPillarUncertainty`` (cls / reg / unc [/ dir]), so ``post_process_stage1_device``,
``PoseCorrector`` and ``inference_intermediate_fusion_aligned(stage1_model=...)`` take it unchanged.  The model reads ``processed_lidar`` as the reference does
(``voxel_features`` / ``voxel_coords`` / ``voxel_num_points`` from the host voxeliser), or -- ``lidar_from_points`` -- a ``voxel_sites`` entry made from the raw clouds
on the device: ``sparse3d.voxel_sites`` (``ops.sp3d_voxelize``) voxelises on the trunk's own site index, which holds this grid's 90 M cells per
agent where ``coalign_voxelize``'s dense tables do not; MeanVFE is inside it and no count is read back.
"""
from __future__ import annotations

import os
from typing import Optional

import numpy as np
import torch
import torch.nn as nn

from . import backbone, ops
from .backbone import DownsampleConv
from .sparse3d import HeightCompression, MeanVFE, VoxelBackBone8x


def get_conv_layers(conv_name, in_channels, out_channels, n_layers, kernel_size, stride, padding, relu_last=True, sequential=True, **kwargs):
    """cia_ssd_utils.py:58-74."""
    seq = []
    for i in range(n_layers):
        seq.extend([getattr(nn, conv_name)(in_channels, out_channels, kernel_size[i], stride=stride[i], padding=padding[i], bias=False,
                                           **{k: v[i] for k, v in kwargs.items()}),
                    nn.BatchNorm2d(out_channels, eps=1e-3, momentum=0.01)])
        if i < n_layers - 1 or relu_last:
            seq.append(nn.ReLU())
        in_channels = out_channels
    return nn.Sequential(*seq) if sequential else seq


def ssfa_switch() -> bool:
    """``COALIGN_SSFA=1``: the neck, the shrink header behind it and the heads on kernels.  Off by default; read when a module is built."""
    return os.environ.get("COALIGN_SSFA", "0") == "1"


class SSFA(nn.Module):
    """Spatial-semantic feature aggregation (cia_ssd_utils.py:6-55); the widths are hard-coded in the reference.  ``neck_kernels`` selects the kernel route
    (``kernel_route``) for an eval-mode float32 CUDA map with even H and W; everything else runs the torch ops below, as always."""

    DECONV_KERNEL = "deconv3x3_s2_sp (transposed 3 x 3 / stride 2 at the low resolution, SplitMap in and out, fp16 x 2)"
    BLEND_KERNEL = "ssfa_blend (both 1 x 1 weight convolutions, softmax over the two and the weighted sum in one launch)"
    SWITCHED_OFF = "switched off (COALIGN_SSFA=0)"

    def __init__(self, args: dict):
        super().__init__()
        self._num_input_features = args["feature_num"]
        self.neck_kernels = ssfa_switch()                        # the kernel route (off by default); may be set per module
        seq = [nn.ZeroPad2d(1)]
        seq += get_conv_layers("Conv2d", 128, 128, n_layers=3, kernel_size=[3, 3, 3], stride=[1, 1, 1], padding=[0, 1, 1], sequential=False)
        self.bottom_up_block_0 = nn.Sequential(*seq)
        self.bottom_up_block_1 = get_conv_layers("Conv2d", 128, 256, n_layers=3, kernel_size=[3, 3, 3], stride=[2, 1, 1], padding=[1, 1, 1])
        self.trans_0 = get_conv_layers("Conv2d", 128, 128, n_layers=1, kernel_size=[1], stride=[1], padding=[0])
        self.trans_1 = get_conv_layers("Conv2d", 256, 256, n_layers=1, kernel_size=[1], stride=[1], padding=[0])
        self.deconv_block_0 = get_conv_layers("ConvTranspose2d", 256, 128, n_layers=1, kernel_size=[3], stride=[2], padding=[1], output_padding=[1])
        self.deconv_block_1 = get_conv_layers("ConvTranspose2d", 256, 128, n_layers=1, kernel_size=[3], stride=[2], padding=[1], output_padding=[1])
        self.conv_0 = get_conv_layers("Conv2d", 128, 128, n_layers=1, kernel_size=[3], stride=[1], padding=[1])
        self.conv_1 = get_conv_layers("Conv2d", 128, 128, n_layers=1, kernel_size=[3], stride=[1], padding=[1])
        self.w_0 = get_conv_layers("Conv2d", 128, 1, n_layers=1, kernel_size=[1], stride=[1], padding=[0], relu_last=False)
        self.w_1 = get_conv_layers("Conv2d", 128, 1, n_layers=1, kernel_size=[1], stride=[1], padding=[0], relu_last=False)

    def init_weights(self):
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.xavier_normal_(m.weight, gain=1)
                if hasattr(m, "bias") and m.bias is not None:
                    nn.init.constant_(m.bias, 0)

    # ---- the kernel route -----------------------------------------------------------------------------------------------------------------------------------
    def _static_reason(self) -> Optional[str]:
        """The part of ``kernel_shape_reason`` that the module's mode and the switches decide, without a tensor."""
        if self.training:
            return "training mode"
        if not backbone.split_maps_active():
            return "the SplitMap arithmetic (fp16 x 2) is not in force"
        return None

    def kernel_shape_reason(self, x: torch.Tensor) -> Optional[str]:
        """None when the kernels take the map ``x``, else why not, in words."""
        static = self._static_reason()
        if static is not None:
            return static
        if x.dim() != 4 or x.shape[1] != 128:
            return f"a map of shape {tuple(x.shape)} for 128 input channels"
        H, W = int(x.shape[2]), int(x.shape[3])
        if H % 2 or W % 2:
            return f"H x W = {H} x {W}, H or W odd (the transposed convolutions' maps do not match x_trans_0; the reference fails too)"
        if not x.is_cuda or x.dtype != torch.float32 or torch.is_grad_enabled() and x.requires_grad:
            return "not a float32 CUDA tensor in inference"
        return None

    def kernel_route(self, x: torch.Tensor) -> bool:
        """Eval mode, ``neck_kernels`` and no reason against (the family convention of DESIGN.md section 8k)."""
        return bool(not self.training and self.neck_kernels and self.kernel_shape_reason(x) is None)

    def plan(self) -> dict:
        """{layer name: route text} from the module's mode and switches alone (no GPU, no tensor; the map-size and device conditions of ``kernel_shape_reason`` are
        decided per call)."""
        why = self.SWITCHED_OFF if not self.neck_kernels else self._static_reason()
        names = [n for n, m in self.named_modules() if isinstance(m, (nn.Conv2d, nn.ConvTranspose2d))]
        if why is not None:
            lines = {n: f"{backbone.MIOPEN} ({why})" for n in names}
            lines["blend"] = f"torch softmax + weighted sum ({why})"
            return lines
        lines = {}
        for n in names:
            m = self.get_submodule(n)
            if isinstance(m, nn.ConvTranspose2d):
                lines[n] = self.DECONV_KERNEL
            elif m.kernel_size == (3, 3):
                lines[n] = backbone.SP_S2 if m.stride == (2, 2) else backbone.SP
            elif m.out_channels == 1:
                lines[n] = "inside " + self.BLEND_KERNEL.split(" (")[0]
            else:
                lines[n] = backbone.pointwise_text(m.in_channels, backbone.CONV_EMU_TERMS) + (backbone.SPLIT_OUT if n.startswith("trans_1") else "")
        lines["blend"] = self.BLEND_KERNEL
        return lines

    def _folded(self) -> dict:
        """Per layer the weight image with BatchNorm (eps 1e-3) folded (``backbone.fold_bn``), its shift and its width, cached until a parameter or buffer changes --
        a warmed-up forward allocates no weight memory."""
        def c3(conv, bn):
            w, b = backbone.fold_bn(conv.weight, None, bn)
            return backbone.Conv3x3Pack(w.detach().float().contiguous()).emu(16, True), b.detach().float().contiguous(), conv.out_channels

        def pw(conv, bn):
            w, b = backbone.fold_bn(conv.weight, None, bn)
            return backbone.PointwisePack(w.detach().float().contiguous(), False).get(), b.detach().float().contiguous(), conv.out_channels

        def dc(conv, bn):      # the tap-major image of the ConvTranspose2d weight read as [Cout, Cin, 3, 3], taps not flipped
            w, b = backbone.fold_bn(conv.weight, None, bn, out_dim=1)
            return ops.pack_conv3x3_emu_weight(w.detach().float().permute(1, 0, 2, 3).contiguous(), 16, True), b.detach().float().contiguous(), conv.out_channels

        def lg(conv, bn):      # a 1-channel 1 x 1 convolution: ([C] weights, the shift as a float)
            w, b = backbone.fold_bn(conv.weight, None, bn)
            return w.detach().float().reshape(-1).contiguous(), float(b.detach().float().reshape(-1)[0])

        def build():
            b0, b1 = self.bottom_up_block_0, self.bottom_up_block_1
            return {"bu0": [c3(b0[i], b0[i + 1]) for i in (1, 4, 7)], "bu1": [c3(b1[i], b1[i + 1]) for i in (0, 3, 6)],
                    "trans_0": pw(self.trans_0[0], self.trans_0[1]), "trans_1": pw(self.trans_1[0], self.trans_1[1]),
                    "deconv_0": dc(self.deconv_block_0[0], self.deconv_block_0[1]), "deconv_1": dc(self.deconv_block_1[0], self.deconv_block_1[1]),
                    "conv_0": c3(self.conv_0[0], self.conv_0[1]), "conv_1": c3(self.conv_1[0], self.conv_1[1]),
                    "w_0": lg(self.w_0[0], self.w_0[1]), "w_1": lg(self.w_1[0], self.w_1[1])}
        return backbone._cache_of(self).get(self, build)

    def forward_kernels(self, x: torch.Tensor, out_split: bool = False, out_nhwc: bool = True):
        """The kernel route (callers ask ``kernel_route`` first): the channels-last float32 map, its SplitMap (``out_split``: a shrink header that takes SplitMaps or
        the merged heads follow), or both."""
        f = self._folded()

        def sp(y, layer, **kw):
            return ops.conv3x3_sp(y, layer[0], layer[1], layer[2], None, True, **kw)

        N, _, H, W = x.shape
        cur = ops.SplitMap.pack(x)
        # bottom_up_block_0: ZeroPad2d(1) + a padding-0 convolution IS a padding-1 convolution; its last layer hands x_0 out as float32 (trans_0) and as a SplitMap (the strided layer)
        x_0, x_0_sp = sp(sp(sp(cur, f["bu0"][0]), f["bu0"][1]), f["bu0"][2], out_both=True)
        s2 = f["bu1"][0]
        x_1 = sp(sp(ops.conv3x3_sp_s2(x_0_sp, s2[0], s2[1], s2[2], relu=True), f["bu1"][1]), f["bu1"][2], out_split=False)
        t0, t1 = f["trans_0"], f["trans_1"]
        x_trans_0 = ops.pointwise_conv(x_0, t0[0], t0[1], t0[2], relu=True, out_channels_last=True)
        x_trans_1 = ops.pointwise_conv(x_1, t1[0], t1[1], t1[2], relu=True, out=ops.SplitMap.empty(N, t1[2], H // 2, W // 2, x.device))
        d0, d1 = f["deconv_0"], f["deconv_1"]
        x_middle_0 = ops.deconv3x3_s2_sp(x_trans_1, d0[0], d0[1], d0[2], residual=x_trans_0, relu=True)      # the residual AFTER the activation (cia_ssd_utils.py:45)
        x_middle_1 = ops.deconv3x3_s2_sp(x_trans_1, d1[0], d1[1], d1[2], relu=True)
        x_output_0, x_output_1 = sp(x_middle_0, f["conv_0"], out_split=False), sp(x_middle_1, f["conv_1"], out_split=False)
        return ops.ssfa_blend(x_output_0, x_output_1, f["w_0"][0], f["w_1"][0], f["w_0"][1], f["w_1"][1], out_split=out_split, out_nhwc=out_nhwc)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        if self.kernel_route(x):
            return self.forward_kernels(x)
        x_0 = self.bottom_up_block_0(x)
        x_1 = self.bottom_up_block_1(x_0)
        x_trans_0 = self.trans_0(x_0)
        x_trans_1 = self.trans_1(x_1)
        x_middle_0 = self.deconv_block_0(x_trans_1) + x_trans_0
        x_middle_1 = self.deconv_block_1(x_trans_1)
        x_output_0 = self.conv_0(x_middle_0)
        x_output_1 = self.conv_1(x_middle_1)
        x_weight = torch.softmax(torch.cat([self.w_0(x_output_0), self.w_1(x_output_1)], dim=1), dim=1)
        x_output = x_output_0 * x_weight[:, 0:1, :, :] + x_output_1 * x_weight[:, 1:, :, :]
        return x_output.contiguous()


class Head(nn.Module):
    """cia_ssd_utils.py:77-101."""

    def __init__(self, num_input, num_pred, num_cls, num_iou=2, use_dir=False, num_dir=1):
        super().__init__()
        self.use_dir = use_dir
        self.conv_box = nn.Conv2d(num_input, num_pred, 1)
        self.conv_cls = nn.Conv2d(num_input, num_cls, 1)
        self.conv_iou = nn.Conv2d(num_input, num_iou, 1, bias=False)
        if self.use_dir:
            self.conv_dir = nn.Conv2d(num_input, num_dir, 1)

    def _convs(self) -> list:
        return [("reg_preds", self.conv_box), ("cls_preds", self.conv_cls), ("iou_preds", self.conv_iou)] + ([("dir_preds", self.conv_dir)] if self.use_dir else [])

    def forward(self, x) -> dict:
        if isinstance(x, ops.SplitMap):      # the neck's kernel route handed its map over: box / cls / iou (zero bias) / dir as ONE ops.heads_sp launch, channel slices out
            y = merged_heads_sp(self, self._convs(), x)
            return {"reg_preds": y["reg_preds"], "cls_preds": y["cls_preds"], "dir_preds": y["dir_preds"] if self.use_dir else torch.zeros((x.shape[0], 1, 2)),
                    "iou_preds": y["iou_preds"]}
        box_preds = self.conv_box(x)
        ret = {"reg_preds": box_preds, "cls_preds": self.conv_cls(x)}
        ret["dir_preds"] = self.conv_dir(x) if self.use_dir else torch.zeros((len(box_preds), 1, 2))
        ret["iou_preds"] = self.conv_iou(x)
        return ret


def weight_init(m: nn.Module) -> None:
    """opencood/utils/model_utils.py:29-38."""
    if isinstance(m, nn.Linear):
        nn.init.xavier_normal_(m.weight.data, gain=0.1)
        if hasattr(m.bias, "data"):
            nn.init.constant_(m.bias.data, 0)
    elif isinstance(m, nn.Conv2d):
        nn.init.xavier_normal_(m.weight, gain=0.1)


def heads_take_split_map(owner: nn.Module, convs) -> bool:
    """The 1 x 1 heads ``convs`` = [(key, conv), ...] can read a SplitMap as one ``ops.heads_sp`` launch: eval mode, the SplitMap arithmetic in force, at most
    ``ops.HEADS_SP_MAX_ROWS`` rows in all over Cin % 16 == 0 channels, weights on the GPU."""
    hs = [c for _, c in convs]
    return bool(not owner.training and backbone.HEADS_SPLIT_IN and backbone.split_maps_active() and sum(c.out_channels for c in hs) <= ops.HEADS_SP_MAX_ROWS
                and hs[0].in_channels % 16 == 0 and all(tuple(c.kernel_size) == (1, 1) for c in hs) and hs[0].weight.is_cuda)


def merged_heads_sp(owner: nn.Module, convs, x: "ops.SplitMap") -> dict:
    """{key: channel slice} of ONE ``ops.heads_sp`` launch over the merged weight rows and biases of ``convs`` (a head without bias gets zeros); the image is cached
    on ``owner`` until a head's tensor changes."""
    tensors = [t for _, c in convs for t in (c.weight, c.bias) if t is not None]

    def build():
        w = torch.cat([c.weight.detach().float().reshape(c.out_channels, -1) for _, c in convs]).contiguous()
        b = torch.cat([c.bias.detach().float() if c.bias is not None else torch.zeros(c.out_channels, device=w.device) for _, c in convs]).contiguous()
        return ops.pack_heads_sp_weight(w), b, w.shape[0]
    img, b, M = backbone._cache_of(owner, "_coalign_heads_sp_cache").get(tensors, build)
    y = ops.heads_sp(x, img, b, M)
    out, c0 = {}, 0
    for k, c in convs:
        out[k] = y[:, c0:c0 + c.out_channels]
        c0 += c.out_channels
    return out


def _batch_size(data_dict: dict, coords: torch.Tensor) -> int:
    """``data_dict['batch_size']`` or the sum of ``record_len`` when present (no device read-back), else the reference's ``coords[:, 0].max() + 1``."""
    if data_dict.get("batch_size") is not None:
        return int(data_dict["batch_size"])
    rl = data_dict.get("record_len")
    if rl is not None:
        return int(rl.sum()) if torch.is_tensor(rl) else int(np.sum(rl))
    return int(coords[:, 0].max()) + 1 if coords.shape[0] else 1


def lidar_from_points(model_or_hypes, clouds, ego_filter: bool = False, filter_range=None, capacity: Optional[int] = None, train: bool = False,
                      max_points: int = 5, max_voxels: Optional[int] = None, device=None) -> dict:
    """The ``processed_lidar`` of a frame from its raw clouds (a list of [n_i, 4] arrays / tensors, one per agent), without the host voxeliser:
    ``model({"processed_lidar": lidar_from_points(model, clouds)})``.  -> {"voxel_sites": ``sparse3d.voxel_sites``' tensor, "voxel_counts": device int32 [n + 1]}
    (``preprocess.SpVoxelPreprocessor.preprocess_clouds_sites``).  ``model_or_hypes``: a config (its ``preprocess`` section gives voxel size, range, points per voxel
    and ``max_voxel_train`` / ``max_voxel_test`` by ``train``) or a built SECOND model (its own voxel size and range; ``max_points`` and ``max_voxels`` -- 70 000, in
    training 36 000: the shipped configs' -- from the arguments).  ``device``: the model's, else the GPU when there is one."""
    from .preprocess import SpVoxelPreprocessor
    if isinstance(model_or_hypes, dict):
        params = model_or_hypes["preprocess"]
        dev = device if device is not None else ("cuda" if torch.cuda.is_available() else "cpu")
    else:
        m = model_or_hypes
        mv = int(max_voxels) if max_voxels is not None else (36000 if train else 70000)
        params = {"cav_lidar_range": list(m.lidar_range), "args": {"voxel_size": list(m.voxel_size), "max_points_per_voxel": int(max_points), "max_voxel_train": mv,
                                                                   "max_voxel_test": mv}}
        dev = device if device is not None else next(m.parameters()).device
    return SpVoxelPreprocessor(params, train, dev).preprocess_clouds_sites(clouds, ego_filter=ego_filter, filter_range=filter_range, capacity=capacity)


class _SecondTrunk(nn.Module):
    def _build_trunk(self, args: dict) -> None:
        self.lidar_range, self.voxel_size = [float(v) for v in args["lidar_range"]], [float(v) for v in args["voxel_size"]]
        rng = np.array(args["lidar_range"])
        grid_size = np.round((rng[3:6] - rng[:3]) / np.array(args["voxel_size"])).astype(np.int64)
        self.vfe = MeanVFE(args["mean_vfe"], args["mean_vfe"]["num_point_features"])
        self.spconv_block = VoxelBackBone8x(args["spconv"], input_channels=args["spconv"]["num_features_in"], grid_size=grid_size,
                                            site_capacity=args["spconv"].get("site_capacity"))
        self.map_to_bev = HeightCompression(args["map2bev"])
        self.ssfa = SSFA(args["ssfa"])
        self.shrink_flag = False
        if "shrink_header" in args:
            self.shrink_flag = True
            self.shrink_conv = DownsampleConv(args["shrink_header"])
            self.out_channel = args["shrink_header"]["dim"][-1]

    def bev_features(self, data_dict: dict) -> torch.Tensor:
        """processed_lidar -> the dense map [N, C D, H, W] in front of SSFA."""
        pl = data_dict["processed_lidar"]
        if pl.get("voxel_sites") is not None:      # ``lidar_from_points``: MeanVFE is inside the tensor, the batch size is its own (no ``_batch_size`` read-back)
            sites = pl["voxel_sites"]
            return self.map_to_bev(self.spconv_block({"voxel_sites": sites, "batch_size": sites.batch_size}))["spatial_features"]
        batch = {"voxel_features": pl["voxel_features"], "voxel_coords": pl["voxel_coords"], "voxel_num_points": pl["voxel_num_points"],
                 "batch_size": _batch_size(data_dict, pl["voxel_coords"])}
        return self.map_to_bev(self.spconv_block(self.vfe(batch)))["spatial_features"]

    def neck(self, data_dict: dict, heads_split: bool = False):
        """The map the heads read.  On the neck's kernel route (``SSFA.kernel_route``) the blend writes a SplitMap when a shrink header that takes SplitMaps follows
        or (``heads_split``: the merged heads can read one) when the heads follow directly, and the shrink header hands its own SplitMap on; otherwise a float32
        tensor, as always."""
        x = self.bev_features(data_dict)
        if not self.ssfa.kernel_route(x):
            out = self.ssfa(x)
            return self.shrink_conv(out) if self.shrink_flag else out
        if self.shrink_flag:
            if self.shrink_conv.takes_split_maps():
                return self.shrink_conv(self.ssfa.forward_kernels(x, out_split=True, out_nhwc=False), out_split=heads_split)
            return self.shrink_conv(self.ssfa.forward_kernels(x))
        return self.ssfa.forward_kernels(x, out_split=True, out_nhwc=False) if heads_split else self.ssfa.forward_kernels(x)


class SecondSSFA(_SecondTrunk):
    """second_ssfa.py:16-58."""

    def __init__(self, args: dict):
        super().__init__()
        self._build_trunk(args)
        self.head = Head(**args["head"])

    def forward(self, data_dict: dict) -> dict:
        return self.head(self.neck(data_dict, heads_split=heads_take_split_map(self.head, self.head._convs())))


class SecondSSFAUncertainty(_SecondTrunk):
    """second_ssfa_uncertainty.py:17-87: the stage-1 detector of CoAlign's box alignment on the SECOND trunk."""

    def __init__(self, args: dict):
        super().__init__()
        self.out_channel = args["ssfa"]["feature_num"]
        self._build_trunk(args)
        self.uncertainty_dim = args["uncertainty_dim"]
        self.cls_head = nn.Conv2d(self.out_channel, args["anchor_num"], kernel_size=1)
        self.reg_head = nn.Conv2d(self.out_channel, 7 * args["anchor_num"], kernel_size=1)
        self.unc_head = nn.Conv2d(self.out_channel, self.uncertainty_dim * args["anchor_num"], kernel_size=1)
        self.use_dir = False
        if "dir_args" in args.keys():
            self.use_dir = True
            self.dir_head = nn.Conv2d(self.out_channel, args["dir_args"]["num_bins"] * args["anchor_num"], kernel_size=1)
        self.apply(weight_init)

    def _convs(self) -> list:
        return [("cls_preds", self.cls_head), ("reg_preds", self.reg_head), ("unc_preds", self.unc_head)] + ([("dir_preds", self.dir_head)] if self.use_dir else [])

    def forward(self, data_dict: dict) -> dict:
        out = self.neck(data_dict, heads_split=heads_take_split_map(self, self._convs()))
        if isinstance(out, ops.SplitMap):      # cls / reg / unc / dir as ONE ops.heads_sp launch; post_process_stage1_device reads the channel slices in place
            return merged_heads_sp(self, self._convs(), out)
        output = {"cls_preds": self.cls_head(out), "reg_preds": self.reg_head(out), "unc_preds": self.unc_head(out)}
        if self.use_dir:
            output["dir_preds"] = self.dir_head(out)
        return output


# ---- plan words ----------------------------------------------------------------------------------------------------------------------------------------------
HEADS_KERNEL = "heads_sp (the merged 1 x 1 heads in one launch, SplitMap input)"


def plan(hypes: dict) -> dict:
    """{layer name: route text} of everything behind the sparse 3-D trunk (``sparse3d.plan`` words the trunk): ``ssfa.*``, ``shrink_conv.*`` and the heads of the model
    ``hypes`` describes, from its shapes, its mode (eval) and the switches alone -- no GPU, no tensor."""
    from .detector import build_model                          # (detector imports this module)
    model = build_model(hypes).eval()
    lines = {"ssfa." + k: v for k, v in model.ssfa.plan().items()}
    on = "ssfa.blend" in lines and lines["ssfa.blend"] == SSFA.BLEND_KERNEL
    why = lines["ssfa.blend"].split(" (", 1)[1][:-1] if not on else None
    split = on
    if model.shrink_flag:
        convs = [(n, m) for n, m in model.shrink_conv.named_modules() if isinstance(m, nn.Conv2d)]
        split = on and all(layer.on_split_maps() for layer in model.shrink_conv.layers) and backbone.HEAD_SPLIT_MAPS
        for n, m in convs:
            lines["shrink_conv." + n] = backbone.SP if split else f"{backbone.MIOPEN} or the consumer-split kernel (DoubleConv's own route; the neck hands over float32)"
    owner, convs = (model.head, model.head._convs()) if isinstance(model, SecondSSFA) else (model, model._convs())
    rows = sum(c.out_channels for _, c in convs)
    heads_on = split and backbone.HEADS_SPLIT_IN and rows <= ops.HEADS_SP_MAX_ROWS and convs[0][1].in_channels % 16 == 0
    prefix = "head." if isinstance(model, SecondSSFA) else ""
    for k, c in convs:
        name = prefix + [n for n, m in owner.named_modules() if m is c][0]
        lines[name] = HEADS_KERNEL if heads_on else f"{backbone.ROCBLAS} ({why if why else 'the neck hands over float32'})"
    return lines
