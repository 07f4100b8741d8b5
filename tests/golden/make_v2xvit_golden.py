#!/usr/bin/env python
"""Generate tests/golden/v2xvit_fuse.npz by IMPORTING THE REFERENCE ITSELF (build container only: needs /root/reference; the ``.npz`` travels, this script's
import does not).  Usage:  python tests/golden/make_v2xvit_golden.py

What is pinned: the reference's ``V2XViTFusion`` (opencood/models/fuse_modules/fusion_in_one.py:295-352 over sub_modules/v2xvit_basic.py, hmsa.py, mswin.py,
split_attn.py, base_transformer.py) called unmodified in eval mode, weights from ``synthetic.v2xvit_parameters_``:
  case A  dim 32 = 2 heads of 16, windows [2, 4, 8] fused naively, depth 2, an 8 x 16 map, record_len [3, 1] padded to L = 5, affines with a shift, a rotation and
          one agent half outside -- inputs, ``state_dict`` (names and tensors) and output;
  case B  dim 256 = 8 heads of 32 with ``split_attn``, depth 1, the same map -- affines, output and checksums of the weights and of the map (both regenerated from
          their seeds by the test: the map alone is half a megabyte).
Before anything is stored the cases are examined in float64: the agent attention's softmax is neither uniform nor saturated, and taking any of the three blocks out
changes the output by far more than the comparison bound (``examine``; tests/test_v2xvit_cpu.py repeats it).
Also recorded, from the reference itself with the identity ``spatial_correction_matrix`` fusion_in_one.py passes, at the three yamls' map shapes and one odd shape:
whether ``STTF``'s output is bit-identical to its input (and how far off it is), and whether ``get_roi_and_cav_mask`` is exactly the agent mask.  And the
``state_dict`` key list and numels of the reference's ``PointPillarBaseline`` built from its unchanged OPV2V v2xvit yaml.  Only data goes into the fixture.
"""
import copy
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from make_disco_golden import REF, import_reference      # noqa: E402  (puts the repository and the reference on sys.path)
from v2xvit_reference import ARGS_A, ARGS_B, SEED_A, SEED_B, args, examine, inputs, weight_checksum      # noqa: E402  (the cases: shared with the tests)

YAML_V2X = REF + "/opencood/hypes_yaml/opv2v/lidar_only_with_noise/pointpillar_v2xvit.yaml"
SHAPES = [(48, 176, 0.4, 4), (48, 128, 0.4, 4), (80, 80, 0.4, 2), (7, 13, 0.4, 4)]      # opv2v, dairv2x, v2xsim (map height, width, voxel size, downsample rate), odd


def findings(vb, ttu):
    rows = []
    for (h, w, vs, ds) in SHAPES:
        sttf = vb.STTF({"voxel_size": [vs, vs, 4], "downsample_rate": ds})
        B, L, C = 2, 5, 4
        x = torch.randn(B, L, h, w, C, generator=torch.Generator().manual_seed(h * w))
        eye = torch.eye(4).expand(B, L, 4, 4)
        y = sttf(x, None, eye.clone())
        mask = torch.tensor([[1, 1, 1, 0, 0], [1, 0, 0, 0, 0]])
        cm = ttu.get_roi_and_cav_mask((B, L, h, w, C), mask, eye.clone(), vs, ds)
        want = mask.view(B, 1, 1, 1, L).expand(B, h, w, 1, L).to(cm.dtype)
        rows.append([h, w, vs, ds, float(torch.equal(x, y)), float((x - y).abs().max() / x.abs().max()), float(torch.equal(cm, want))])
        print("map", h, "x", w, "STTF bit-identical:", bool(rows[-1][4]), "worst deviation / scale", rows[-1][5], "| ROI mask == agent mask:", bool(rows[-1][6]))
    return np.array(rows, dtype=np.float64), x, y


def main():
    fio = import_reference("opencood.models.fuse_modules.fusion_in_one")
    vb = import_reference("opencood.models.sub_modules.v2xvit_basic")
    ttu = import_reference("opencood.models.sub_modules.torch_transformation_utils")
    from coalign_amd.synthetic import v2xvit_parameters_
    fixture = {}
    for tag, a, seed in (("a", ARGS_A, SEED_A), ("b", ARGS_B, SEED_B)):
        C = a["transformer"]["encoder"]["cav_att_config"]["dim"]
        x, rl, A = inputs(C, seed + 100)
        examine(a, seed, x, rl, A, "case " + tag.upper())
        torch.manual_seed(seed)
        m = fio.V2XViTFusion(copy.deepcopy(a))
        v2xvit_parameters_(m, seed=seed)
        m.eval()
        with torch.no_grad():
            out = m(x, rl, A)
        print("case", tag.upper(), "output", tuple(out.shape), "max |out|", float(out.abs().max()))
        fixture.update({tag + ".record_len": rl.numpy(), tag + ".affine": A.numpy(), tag + ".out": out.numpy(), tag + ".weight_checksum": weight_checksum(m),
                        tag + ".x_checksum": np.array([float(x.double().sum()), float(x.double().abs().sum())])})
        if tag == "a":
            fixture["a.x"] = x.numpy()      # (case B's 512 KB map is regenerated from its seed by the test, like its weights, and checked against x_checksum)
        if tag == "a":
            sd = m.state_dict()
            fixture.update({"state_keys": np.array(list(sd.keys())), "state_numel": np.array([v.numel() for v in sd.values()], dtype=np.int64),
                            **{"sd." + k: v.numpy() for k, v in sd.items()}})
    # the same names with RTE, which no shipped yaml switches on
    rte = fio.V2XViTFusion(args(32, 2, 16, [4, 2, 1], [8, 16, 32], [2, 4, 8], "naive", 1, use_rte=True))
    fixture["rte_state_keys"] = np.array(list(rte.state_dict().keys()))
    fixture["rte_state_numel"] = np.array([v.numel() for v in rte.state_dict().values()], dtype=np.int64)
    table, sx, sy = findings(vb, ttu)
    fixture["identity_findings"] = table                                         # rows: H, W, voxel size, downsample rate, STTF bit-identical, its deviation / scale, ROI == agent mask
    fixture["sttf_probe_in"], fixture["sttf_probe_out"] = sx.numpy(), sy.numpy()      # the odd shape's probe through the reference's STTF
    yaml_utils = import_reference("opencood.hypes_yaml.yaml_utils")
    hypes = yaml_utils.load_yaml(YAML_V2X)
    model = import_reference("opencood.models.point_pillar_baseline").PointPillarBaseline(hypes["model"]["args"])
    fixture["model_state_keys"] = np.array(list(model.state_dict().keys()))
    fixture["model_state_numel"] = np.array([v.numel() for v in model.state_dict().values()], dtype=np.int64)
    path = os.path.join(HERE, "v2xvit_fuse.npz")
    np.savez_compressed(path, **fixture)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
