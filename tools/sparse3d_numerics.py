"""Error of the sparse 3-D trunk's kernels, layer by layer and for the whole backbone, at sparse shape (41, 64, 64) x 2 agents: the worst |kernel - float64| / scale
beside the same quantity for the torch-op route in float32 ON THE SAME INPUTS.  The float64 value is the dense restatement of tests/sparse3d_reference.py.  A layer's
input is the kernel route's output of the layer before it.  A kernel error above twice the float32 route's is flagged: a different summation order over <= 1728
products does not do that, a dropped tap does.

    python tools/sparse3d_numerics.py [--out profiles/sparse3d/numerics.json]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import sparse3d_cases as cases  # noqa: E402
import sparse3d_reference as ref  # noqa: E402
from coalign_amd import sparse3d  # noqa: E402

SHAPE = (41, 64, 64)


def worst(got_rows, idx, dense):
    i = idx.long().cpu()
    want = dense[i[:, 0], :, i[:, 1], i[:, 2], i[:, 3]]
    return float((got_rows.double().cpu() - want).abs().max()) / max(float(want.abs().max()), 1e-300)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sparse3d", "numerics.json"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    bb = cases.seed_backbone_(sparse3d.VoxelBackBone8x({"num_features_out": 64}, 4, [SHAPE[2], SHAPE[1], SHAPE[0] - 1]), 5).eval().to(dev)
    vox = cases.voxels(SHAPE, 2, seed=6)
    mean = (vox["voxel_features"].sum(dim=1) / vox["voxel_num_points"].clamp(min=1).view(-1, 1)).to(dev)
    x = sparse3d.SparseTensor3d(mean, vox["voxel_coords"].to(dev), SHAPE, 2)
    layers = []
    for name in ("conv_input", "conv1", "conv2", "conv3", "conv4", "conv_out"):
        seq = getattr(bb, name)
        layers += [(name, seq)] if hasattr(seq[0], "kernel_size") else [(f"{name}.{i}", s) for i, s in enumerate(seq)]
    rows_out, flagged = {}, []
    with torch.no_grad():
        for name, seq in layers:
            n = x.rows()
            host = sparse3d.SparseTensor3d(x.features[:n].clone(), x.indices[:n].clone(), x.spatial_shape, 2)       # the same input for the three
            dense, mask = ref.sequential(seq, *ref.scatter(host.features, host.indices, x.spatial_shape, 2))
            os.environ["COALIGN_SP3D"] = "1"
            k = seq(x)
            os.environ["COALIGN_SP3D"] = "0"
            t = seq(host)
            nk = k.rows()
            assert nk == t.rows() and torch.equal(k.indices[:nk], t.indices[:nk]), name
            ek, et = worst(k.features[:nk], k.indices[:nk], dense), worst(t.features[:nk], t.indices[:nk], dense)
            conv = seq[0]
            rows_out[name] = {"cin": conv.in_channels, "cout": conv.out_channels, "kernel": list(conv.kernel_size), "stride": list(conv.stride), "rows_in": n, "rows_out": nk,
                              "kernel_route_worst_of_scale": ek, "torch_float32_worst_of_scale": et}
            if ek > 2 * et:
                flagged.append(name)
            print(f"{name:12s} {conv.in_channels:3d} -> {conv.out_channels:3d} rows {n:6d} -> {nk:6d}  kernel {ek:.3e}  torch fp32 {et:.3e}", flush=True)
            x = k
        dense, _ = ref.backbone(bb, mean.cpu().double(), vox["voxel_coords"], 2)
        want = ref.height_compression(dense)
        d = {"voxel_features": mean, "voxel_coords": vox["voxel_coords"].to(dev), "batch_size": 2}
        hc = sparse3d.HeightCompression({"feature_num": 128})
        os.environ["COALIGN_SP3D"] = "1"
        gk = hc(bb(dict(d)))["spatial_features"].cpu().double()
        os.environ["COALIGN_SP3D"] = "0"
        gt = hc(bb(dict(d)))["spatial_features"].cpu().double()
    scale = float(want.abs().max())
    whole = {"kernel_route_worst_of_scale": float((gk - want).abs().max()) / scale, "torch_float32_worst_of_scale": float((gt - want).abs().max()) / scale}
    print("backbone + to-dense", whole)
    result = {"sparse_shape": list(SHAPE), "agents": 2, "voxels": int(vox["voxel_coords"].shape[0]), "layers": rows_out, "backbone_and_to_dense": whole,
              "layers_where_the_kernel_exceeds_twice_the_float32_route": flagged,
              "what": "worst |route - float64 dense restatement| / max |float64|, per layer on the same float32 input (the kernel route's output of the layer before)"}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(result, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
