#!/usr/bin/env python
"""Generate tests/golden/v2v_robust.npz by IMPORTING THE REFERENCE ITSELF (build container only: needs /root/reference; the ``.npz`` travels, this script's
import does not).  Usage:  python tests/golden/make_v2v_robust_golden.py

What is pinned: the reference's own ``PoseRegressionWraper``, ``get_intersection``, ``WeightedEM`` and ``AttentionWrapper``
(opencood/models/sub_modules/v2v_robust_module.py) and ``V2VNetFusion`` with ``agg_operator: weight`` (opencood/models/fuse_modules/v2v_fuse.py), called unmodified
in eval mode in the order of ``PointPillarV2VNetRobust.eval_forward`` on a small batch -- feature_dim = hidden_dim = 16, 24 x 40, record_len [3, 1], max_cav 5 --
with the weights of ``synthetic.v2v_robust_parameters_`` and poses that carry strong noise.  Stored: the inputs, the three ``state_dict``s (names and tensors), every
intermediate result, and the ``state_dict`` key list and numels of the reference's ``PointPillarV2VNetRobust`` built from its unchanged opv2v yaml.  Only data goes
into the fixture.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from make_disco_golden import REF, import_reference      # noqa: E402  (puts the repository and the reference on sys.path)

YAML = REF + "/opencood/hypes_yaml/opv2v/lidar_only_with_noise/pointpillar_v2vnet_robust.yaml"
C, HID, H, W, L, SEED = 16, 16, 24, 40, 5, 50
AFFINE = {"H": H, "W": W, "downsample_rate": 2, "discrete_ratio": 0.4}
FUSION = {"voxel_size": [0.4, 0.4, 4], "downsample_rate": 2, "num_iteration": 2, "in_channels": C, "gru_flag": True, "agg_operator": "weight",
          "conv_gru": {"H": H, "W": W, "num_layers": 1, "kernel_size": [[3, 3]]}}


def inputs():
    g = torch.Generator().manual_seed(SEED + 1)
    x = torch.randn(4, C, H, W, generator=g)
    poses = torch.tensor([[0.0, 0.0, 0.0], [3.0, 1.2, 9.0], [-2.4, 2.0, -7.0], [10.0, -4.0, 30.0]])
    poses[:, :2] += torch.randn(4, 2, generator=g) * 0.4                     # strong noise (0.4 m); the yaw noise of the model is a fraction of a degree
    poses[:, 2] += torch.randn(4, generator=g) * 0.07
    return x, poses, torch.tensor([3, 1])


def main():
    R = import_reference("opencood.models.sub_modules.v2v_robust_module")
    V = import_reference("opencood.models.fuse_modules.v2v_fuse")
    tu = import_reference("opencood.utils.transformation_utils")
    from coalign_amd.synthetic import v2v_parameters_, v2v_robust_parameters_
    reg, att, fus = R.PoseRegressionWraper(2 * C, HID, AFFINE), R.AttentionWrapper(2 * C, HID, AFFINE, True), V.V2VNetFusion(FUSION)
    v2v_robust_parameters_(reg, seed=SEED)
    v2v_robust_parameters_(att, seed=SEED)
    v2v_parameters_(fus, seed=SEED)
    for m in (reg, att, fus):
        m.eval()
    x, poses, record_len = inputs()
    with torch.no_grad():
        T = tu.get_pairwise_transformation_torch(poses, L, record_len, 3)
        corr, T_new = reg(x, record_len, T)
        inter = R.get_intersection(T_new[0], AFFINE)
        fixed = torch.cat([R.WeightedEM(poses[:3], T_new[0], inter), poses[3:]], dim=0)
        T_fixed = tu.get_pairwise_transformation_torch(fixed, L, record_len, 3)
        scores, weight = att(x, record_len, T_fixed)
        fused = fus(x, record_len, T_fixed, weight)
    print("corr", corr[0, :3, :3].flatten().tolist(), "\nfixed - noisy", (fixed - poses).tolist(), "\nscores", scores[0, :3, :3].tolist(), "\nintersection", inter.unique().tolist(),
          "max |fused|", float(fused.abs().max()))
    fixture = {"x": x.numpy(), "poses": poses.numpy(), "record_len": record_len.numpy(), "T": T.numpy(), "corr": corr.numpy(), "T_new": T_new.numpy(),
               "intersection": inter.numpy(), "fixed": fixed.numpy(), "T_fixed": T_fixed.numpy(), "scores": scores.numpy(), "weight": weight.numpy(), "fused": fused.numpy()}
    for tag, m in (("reg", reg), ("att", att), ("fus", fus)):
        sd = m.state_dict()
        fixture[tag + "_keys"] = np.array(list(sd.keys()))
        fixture.update({f"{tag}.{k}": v.numpy() for k, v in sd.items()})
    yaml_utils = import_reference("opencood.hypes_yaml.yaml_utils")
    hypes = yaml_utils.load_yaml(YAML)
    model = import_reference("opencood.models.point_pillar_v2vnet_robust").PointPillarV2VNetRobust(hypes["model"]["args"])
    fixture["model_state_keys"] = np.array(list(model.state_dict().keys()))
    fixture["model_state_numel"] = np.array([v.numel() for v in model.state_dict().values()], dtype=np.int64)
    path = os.path.join(HERE, "v2v_robust.npz")
    np.savez_compressed(path, **fixture)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
