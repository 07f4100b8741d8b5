#!/usr/bin/env python
"""Generate tests/golden/pillar_variants.npz by IMPORTING THE REFERENCE ITSELF (build container only: needs /root/reference; the ``.npz`` travels, this script's
import does not).  Usage:  python tests/golden/make_pillar_variants_golden.py

What is pinned: the reference's ``PillarVFE`` (opencood/models/sub_modules/pillar_vfe.py:31-53,105-155) called unmodified in eval mode for the four flag sets
``oracle.pillar_vfe`` does not cover -- the distance feature on, no BatchNorm (a Linear bias instead), no absolute xyz, and distance without BatchNorm -- on
M = 48 pillars of P = 32 slots, C = 64, point counts 1..32 (1, 16, 17 and 32 among them), a third of the BatchNorm scales negative.  Stored per flag set: the
inputs, the ``state_dict`` (names and tensors), the float32 output.  Only data goes into the fixture.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"
sys.path.insert(0, REPO)
sys.path.insert(0, HERE)
sys.path.insert(0, REF)

VARIANTS = {"dist": (True, True, True), "bias": (True, False, False), "noabs": (False, False, True), "dist_bias": (True, True, False)}      # (abs, distance, norm)


def main():
    from make_disco_golden import import_reference
    from tests.pillar_cases import make_case
    from tests.pillar_reference import PREFIX
    vfe = import_reference("opencood.models.sub_modules.pillar_vfe")
    fixture = {"variants": np.array(list(VARIANTS))}
    for name, (use_abs, with_dist, use_norm) in VARIANTS.items():
        case = make_case("golden_" + name, "golden", M=48, use_abs=use_abs, with_dist=with_dist, use_norm=use_norm, counts=np.arange(48) % 32 + 1)
        cfg = {"use_norm": use_norm, "with_distance": with_dist, "use_absolute_xyz": use_abs, "num_filters": [64]}
        m = vfe.PillarVFE(cfg, 4, case.voxel_size, case.lidar_range)
        sd = {k[len("pillar_vfe."):]: v for k, v in case.sd.items()}
        if use_norm:
            sd["pfn_layers.0.norm.num_batches_tracked"] = torch.tensor(0)
        m.load_state_dict(sd)
        m.eval()
        with torch.no_grad():
            out = m({"voxel_features": case.vf.clone(), "voxel_num_points": case.npts.clone(), "voxel_coords": case.coords.clone()})["pillar_features"]
        assert out.shape == (48, 64) and out.dtype == torch.float32
        fixture.update({f"{name}.flags": np.array([use_abs, with_dist, use_norm]), f"{name}.voxel_features": case.vf.numpy(), f"{name}.voxel_num_points": case.npts.numpy(),
                        f"{name}.voxel_coords": case.coords.numpy(), f"{name}.voxel_size": np.array(case.voxel_size), f"{name}.lidar_range": np.array(case.lidar_range),
                        f"{name}.out": out.numpy(), f"{name}.state_keys": np.array(list(case.sd))})
        fixture.update({f"{name}.sd.{k}": v.numpy() for k, v in case.sd.items()})
        print(name, "max", float(out.max()), "zeros", float((out == 0).float().mean()))
    path = os.path.join(HERE, "pillar_variants.npz")
    np.savez_compressed(path, **fixture)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
