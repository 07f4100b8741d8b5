#!/usr/bin/env python
"""Generate tests/golden/v2v_fuse.npz by IMPORTING THE REFERENCE ITSELF (build container only: needs /root/reference; the ``.npz`` travels, this script's
import does not).  Usage:  python tests/golden/make_v2v_golden.py

What is pinned: the reference's ``V2VNetFusion`` (opencood/models/fuse_modules/fusion_in_one.py:173-293, with ``ConvGRU``, sub_modules/convgru.py) called
unmodified in eval mode on a small batch -- C = 16, 9 x 14, record_len [3, 1], max, 2 iterations, 1 GRU layer -- with affines filled for ALL receiver rows (shift,
rotation, one agent half outside) and the weights of ``synthetic.v2v_parameters_`` (gates unsaturated, messages of the order of the node features).  Stored: the
inputs, the ``state_dict`` (names and tensors), the output, and the ``state_dict`` key list and numels of the reference's ``PointPillarBaseline`` built from its
unchanged v2vnet yaml.  Only data goes into the fixture.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from make_disco_golden import REF, import_reference      # noqa: E402  (puts the repository and the reference on sys.path)
from v2v_reference import make_thetas                    # noqa: E402

YAML_V2V = REF + "/opencood/hypes_yaml/opv2v/lidar_only_with_noise/pointpillar_v2vnet.yaml"
ARGS = {"num_iteration": 2, "in_channels": 16, "gru_flag": True, "agg_operator": "max", "conv_gru": {"H": 9, "W": 14, "num_layers": 1, "kernel_size": [[3, 3]]}}


def affines(L=5):
    """normalized_affine_matrix [2, L, L, 2, 3] float64, every receiver row of frame 0's three agents filled; identity elsewhere."""
    A = torch.zeros(2, L, L, 2, 3, dtype=torch.float64)
    A[..., 0, 0] = A[..., 1, 1] = 1.0
    A[0, :3, :3] = make_thetas(3, 9, 14, seed=30)
    return A


def main():
    fio = import_reference("opencood.models.fuse_modules.fusion_in_one")
    from coalign_amd.synthetic import v2v_parameters_
    torch.manual_seed(30)
    C, H, W = ARGS["in_channels"], 9, 14
    m = fio.V2VNetFusion(ARGS)
    v2v_parameters_(m, seed=30)
    m.eval()
    x = torch.randn(4, C, H, W, generator=torch.Generator().manual_seed(31))
    record_len = torch.tensor([3, 1])
    A = affines()
    with torch.no_grad():
        out = m(x, record_len, A)
    print("output", tuple(out.shape), "max |out|", float(out.abs().max()))
    sd = m.state_dict()
    fixture = {"x": x.numpy(), "record_len": record_len.numpy(), "affine": A.numpy(), "out": out.numpy(),
               "state_keys": np.array(list(sd.keys())), **{"sd." + k: v.numpy() for k, v in sd.items()}}
    yaml_utils = import_reference("opencood.hypes_yaml.yaml_utils")
    hypes = yaml_utils.load_yaml(YAML_V2V)
    model = import_reference("opencood.models.point_pillar_baseline").PointPillarBaseline(hypes["model"]["args"])
    fixture["model_state_keys"] = np.array(list(model.state_dict().keys()))
    fixture["model_state_numel"] = np.array([v.numel() for v in model.state_dict().values()], dtype=np.int64)
    path = os.path.join(HERE, "v2v_fuse.npz")
    np.savez_compressed(path, **fixture)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
