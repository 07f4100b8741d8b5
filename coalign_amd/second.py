"""CoAlign's second stage-1 detector family: SECOND with the SSFA neck (opencood/models/second_ssfa.py, second_ssfa_uncertainty.py).

``MeanVFE`` -> ``VoxelBackBone8x`` -> ``HeightCompression`` (coalign_amd.sparse3d: the gfx950 kernels of csrc/sparse_conv3d.hip, or torch ops) -> ``SSFA`` ->
shrink header -> heads.  ``SSFA`` and ``Head`` are plain torch modules with the reference's parameter names: SSFA's 3 x 3 / stride-2 transposed convolutions have no
SplitMap kernel.  ``SecondSSFAUncertainty`` emits the four head maps of ``PointPillarUncertainty`` (cls / reg / unc [/ dir]), so ``post_process_stage1_device``,
``PoseCorrector`` and ``inference_intermediate_fusion_aligned(stage1_model=...)`` take it unchanged.  The model reads ``processed_lidar`` as the reference does (the
device voxeliser refuses this grid's 90 M cells).
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn as nn

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


class SSFA(nn.Module):
    """Spatial-semantic feature aggregation (cia_ssd_utils.py:6-55); the widths are hard-coded in the reference."""

    def __init__(self, args: dict):
        super().__init__()
        self._num_input_features = args["feature_num"]
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

    def forward(self, x: torch.Tensor) -> torch.Tensor:
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

    def forward(self, x: torch.Tensor) -> dict:
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


def _batch_size(data_dict: dict, coords: torch.Tensor) -> int:
    """``data_dict['batch_size']`` or the sum of ``record_len`` when present (no device read-back), else the reference's ``coords[:, 0].max() + 1``."""
    if data_dict.get("batch_size") is not None:
        return int(data_dict["batch_size"])
    rl = data_dict.get("record_len")
    if rl is not None:
        return int(rl.sum()) if torch.is_tensor(rl) else int(np.sum(rl))
    return int(coords[:, 0].max()) + 1 if coords.shape[0] else 1


class _SecondTrunk(nn.Module):
    def _build_trunk(self, args: dict) -> None:
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
        batch = {"voxel_features": pl["voxel_features"], "voxel_coords": pl["voxel_coords"], "voxel_num_points": pl["voxel_num_points"],
                 "batch_size": _batch_size(data_dict, pl["voxel_coords"])}
        return self.map_to_bev(self.spconv_block(self.vfe(batch)))["spatial_features"]

    def neck(self, data_dict: dict) -> torch.Tensor:
        out = self.ssfa(self.bev_features(data_dict))
        return self.shrink_conv(out) if self.shrink_flag else out


class SecondSSFA(_SecondTrunk):
    """second_ssfa.py:16-58."""

    def __init__(self, args: dict):
        super().__init__()
        self._build_trunk(args)
        self.head = Head(**args["head"])

    def forward(self, data_dict: dict) -> dict:
        return self.head(self.neck(data_dict))


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

    def forward(self, data_dict: dict) -> dict:
        out = self.neck(data_dict)
        output = {"cls_preds": self.cls_head(out), "reg_preds": self.reg_head(out), "unc_preds": self.unc_head(out)}
        if self.use_dir:
            output["dir_preds"] = self.dir_head(out)
        return output
