#!/usr/bin/env python
"""Generate tests/golden/where2comm_fuse.npz by IMPORTING THE REFERENCE ITSELF (build container only: needs /root/reference; the ``.npz`` travels, this script's
import does not).  Usage:  python tests/golden/make_where2comm_golden.py

What is pinned: the reference's ``Where2comm`` (opencood/models/fuse_modules/where2comm_attn.py:174-341, with ``Communication``,
opencood/models/comm_modules/where2comm.py:9-78) called unmodified in eval mode:

* single scale: C = 16, 10 x 12, record_len [3, 1], ATTEN and MAX, with (5 x 5, sigma 1) and without smoothing, thre 0.3;
* multi scale: the reference's ``ResNetBEVBackbone`` (inplanes 16, filters 16 / 32 / 64, one block per level, strides 1 / 2 / 2, 16 x 24 input), ATTEN and MAX,
  with smoothing.

The pairwise matrices put a shift on agent 1, a rotation on agent 2 and, in a second set, agent 2 half out of view.  The logits are ``2 randn - 2`` (smoothed) and
``2 randn - 1.5`` (not smoothed), the first seed from 50 on at which ``where2comm_reference.check_mask_inputs`` holds in float64: every agent's mask 20-80 % ones,
no smoothed confidence within 2e-5 of the threshold.  Stored: inputs, the backbone's state, outputs, ``communication_rates``, the masks (the reference's
``Communication`` called on the same inputs) and the ``state_dict`` keys.  Only data goes into the fixture."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from make_disco_golden import import_reference      # noqa: E402  (puts the repository and the reference on sys.path)
from where2comm_reference import check_mask_inputs, gaussian_weight      # noqa: E402

VOXEL = [0.4, 0.4, 4]
THRE = 0.3
SMOOTH = {"k_size": 5, "c_sigma": 1.0}
BACKBONE = {"layer_nums": [1, 1, 1], "layer_strides": [1, 2, 2], "num_filters": [16, 32, 64], "upsample_strides": [1, 2, 4], "num_upsample_filter": [32, 32, 32],
            "inplanes": 16}


def module_args(mode, multi_scale, smooth, C=16):
    comm = {"thre": THRE}
    if smooth:
        comm["gaussian_smooth"] = dict(SMOOTH)
    args = {"voxel_size": VOXEL, "downsample_rate": 1, "multi_scale": multi_scale, "agg_operator": {"mode": mode, "feature_dim": C}, "communication": comm}
    if multi_scale:
        args.update(layer_nums=BACKBONE["layer_nums"], num_filters=BACKBONE["num_filters"])
    return args


def pairwise(H, W, half_out, L=5):
    """pairwise_t_matrix [2, L, L, 4, 4] float64 in metres: row [0, 0, j] takes the ego grid into agent j -- identity, a sub-pixel shift, a 20 degree rotation with
    a shift (``half_out``: half the map's width, so that half of agent 2 is out of view)."""
    T = torch.eye(4, dtype=torch.float64).repeat(2, L, L, 1, 1)
    T[0, 0, 1, 0, 3], T[0, 0, 1, 1, 3] = 0.37 * VOXEL[0], -0.58 * VOXEL[0]
    c, s = np.cos(np.pi / 9), np.sin(np.pi / 9)
    T[0, 0, 2, :2, :2] = torch.tensor([[c, -s], [s, c]], dtype=torch.float64)
    T[0, 0, 2, 0, 3] = (W / 2 if half_out else 1.3) * VOXEL[0]
    T[0, 0, 2, 1, 3] = -0.7 * VOXEL[0]
    return T


def logits(shape, smooth):
    weight = gaussian_weight(SMOOTH["k_size"], SMOOTH["c_sigma"]) if smooth else None
    bias = torch.zeros(1) if smooth else None
    for seed in range(50, 114):
        psm = 2 * torch.randn(shape, generator=torch.Generator().manual_seed(seed)) - (2.0 if smooth else 1.5)
        try:
            check_mask_inputs(psm, weight, bias, THRE)
        except AssertionError:
            continue
        return psm, seed
    raise RuntimeError("no seed in 50..113 gives mixed masks with the margin")


def randomise_(module, seed):
    """Weights of order one and BatchNorm statistics that are not the identity."""
    g = torch.Generator().manual_seed(seed)
    for m in module.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            m.running_mean.copy_(0.1 * torch.randn(m.running_mean.shape, generator=g))
            m.running_var.copy_(0.5 + torch.rand(m.running_var.shape, generator=g))
            m.weight.data.copy_(0.8 + 0.4 * torch.rand(m.weight.shape, generator=g))
            m.bias.data.copy_(0.1 * torch.randn(m.bias.shape, generator=g))


def main():
    w2c = import_reference("opencood.models.fuse_modules.where2comm_attn")
    comm_mod = import_reference("opencood.models.comm_modules.where2comm")
    bev = import_reference("opencood.models.sub_modules.base_bev_backbone_resnet")
    record_len = torch.tensor([3, 1])
    fixture = {"record_len": record_len.numpy(), "thre": np.array(THRE)}
    with torch.no_grad():
        # ---- single scale
        C, H, W = 16, 10, 12
        x = torch.randn(4, C, H, W, generator=torch.Generator().manual_seed(61))
        fixture["single_x"] = x.numpy()
        for half_out in (False, True):
            fixture[f"single_pairwise_{int(half_out)}"] = pairwise(H, W, half_out).numpy()
        for smooth in (False, True):
            psm, seed = logits((4, 2, H, W), smooth)
            fixture[f"single_psm_{int(smooth)}"], fixture[f"single_seed_{int(smooth)}"] = psm.numpy(), np.array(seed)
            for mode in ("ATTEN", "MAX"):
                m = w2c.Where2comm(module_args(mode, False, smooth)).eval()
                fixture[f"single_keys_{int(smooth)}"] = np.array(list(m.state_dict().keys()), dtype=str)
                if smooth:
                    fixture["gaussian_weight"] = m.naive_communication.gaussian_filter.weight.numpy().copy()
                    fixture["gaussian_bias"] = m.naive_communication.gaussian_filter.bias.numpy().copy()
                for half_out in (False, True):
                    T = pairwise(H, W, half_out)
                    out, rate, _ = m(x.clone(), psm.clone(), record_len, T.clone())
                    tag = f"single_{mode}_{int(smooth)}_{int(half_out)}"
                    fixture[tag + "_out"], fixture[tag + "_rate"] = out.numpy(), rate.numpy()
                    print(tag, tuple(out.shape), "rate", float(rate))
            comm = comm_mod.Communication(module_args("MAX", False, smooth)["communication"]).eval()
            _, masks, rate = comm(list(torch.split(psm, record_len.tolist())), record_len, torch.zeros(2, 5, 5, 2, 3))
            fixture[f"single_masks_{int(smooth)}"] = masks[:, 0].numpy().astype(np.uint8)
        # ---- multi scale
        H, W = 16, 24
        backbone = bev.ResNetBEVBackbone(dict(BACKBONE), 16)
        randomise_(backbone, seed=62)
        backbone.eval()
        x = torch.randn(4, 16, H, W, generator=torch.Generator().manual_seed(63))
        psm, seed = logits((4, 2, H, W), True)
        fixture["multi_x"], fixture["multi_psm"], fixture["multi_seed"] = x.numpy(), psm.numpy(), np.array(seed)
        fixture["multi_pairwise"] = pairwise(H, W, True).numpy()
        for k, v in backbone.state_dict().items():
            fixture["backbone." + k] = v.numpy()
        fixture["backbone_keys"] = np.array(list(backbone.state_dict().keys()), dtype=str)
        for mode in ("ATTEN", "MAX"):
            m = w2c.Where2comm(module_args(mode, True, True)).eval()
            fixture["multi_keys"] = np.array(list(m.state_dict().keys()), dtype=str)
            out, rate, _ = m(x.clone(), psm.clone(), record_len, pairwise(H, W, True), backbone)
            fixture[f"multi_{mode}_out"], fixture[f"multi_{mode}_rate"] = out.numpy(), rate.numpy()
            print("multi", mode, tuple(out.shape), "rate", float(rate))
        comm = comm_mod.Communication(module_args("MAX", True, True)["communication"]).eval()
        _, masks, _ = comm(list(torch.split(psm, record_len.tolist())), record_len, torch.zeros(2, 5, 5, 2, 3))
        fixture["multi_masks"] = masks[:, 0].numpy().astype(np.uint8)
    path = os.path.join(HERE, "where2comm_fuse.npz")
    np.savez_compressed(path, **fixture)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
