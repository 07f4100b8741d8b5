"""Time the sparse 3-D trunk (MeanVFE -> VoxelBackBone8x -> HeightCompression) at the OPV2V grid, 5 agents: the kernel route against the torch-op route on the
same device.  Voxels: ``coalign_amd.synthetic.make_point_cloud`` sweeps binned by torch ops (at most 5 points per voxel).  Every shape is warmed up; device events;
5 alternating rounds x 10 forwards; median and min .. max per route.  Also the voxel and per-level site counts, the kernel route's workspace bytes (site indices +
neighbour tables) and its launch count.  The reference itself cannot be timed: spconv is not installed.

    python tools/time_sparse3d.py [--out profiles/sparse3d/timing.json] [--agents 5] [--config second/opv2v_second_uncertainty]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from coalign_amd import ops, sparse3d  # noqa: E402
from coalign_amd.config import builtin_config  # noqa: E402
from coalign_amd.synthetic import make_point_cloud  # noqa: E402

LAUNCHES = {"sp3d_index": 6, "sp3d_sites": 6}          # launches per ABI call; every other call is one


def bin_cloud(points: torch.Tensor, rng, voxel, shape, agent: int, T: int = 5):
    """One sweep [n, 4] -> (voxel_features [M, T, 4], voxel_coords [M, 4] int32, voxel_num_points [M] int32) by torch ops: the first T points of a voxel in sweep order."""
    lo = torch.tensor(rng[:3], dtype=torch.float32)
    c = torch.floor((points[:, :3] - lo) / torch.tensor(voxel, dtype=torch.float32)).long()          # (x, y, z)
    D, H, W = shape
    ok = (c[:, 0] >= 0) & (c[:, 0] < W) & (c[:, 1] >= 0) & (c[:, 1] < H) & (c[:, 2] >= 0) & (c[:, 2] < D - 1)
    points, c = points[ok], c[ok]
    key = (c[:, 2] * H + c[:, 1]) * W + c[:, 0]
    key, order = torch.sort(key, stable=True)
    points = points[order]
    uniq, inverse, counts = torch.unique_consecutive(key, return_inverse=True, return_counts=True)
    first = torch.cumsum(counts, 0) - counts
    slot = torch.arange(key.numel()) - first[inverse]
    keep = slot < T
    feats = torch.zeros((uniq.numel(), T, 4))
    feats[inverse[keep], slot[keep]] = points[keep]
    coords = torch.stack([torch.full_like(uniq, agent), uniq // (H * W), uniq // W % H, uniq % W], dim=1).to(torch.int32)
    return feats, coords, counts.clamp(max=T).to(torch.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sparse3d", "timing.json"))
    ap.add_argument("--agents", type=int, default=5)
    ap.add_argument("--config", default="second/opv2v_second_uncertainty")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--forwards", type=int, default=10)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    h = builtin_config(a.config)
    args = h["model"]["args"]
    rng, voxel = args["lidar_range"], args["voxel_size"]
    grid = np.round((np.array(rng[3:6]) - np.array(rng[:3])) / np.array(voxel)).astype(np.int64)
    bb = sparse3d.VoxelBackBone8x(args["spconv"], args["spconv"]["num_features_in"], grid).eval()
    g = torch.Generator().manual_seed(0)
    with torch.no_grad():
        for m in bb.modules():
            if isinstance(m, sparse3d._SparseConvBase):
                m.weight.copy_(torch.randn(m.weight.shape, generator=g) * (4.0 / (m.taps * m.in_channels)) ** 0.5)
            elif isinstance(m, torch.nn.BatchNorm1d):
                m.running_var.copy_(torch.rand(m.bias.shape, generator=g) * 0.5 + 0.75)
                m.bias.copy_(torch.randn(m.bias.shape, generator=g) * 0.1 + 0.05)
    bb = bb.to(dev)
    parts = [bin_cloud(torch.from_numpy(make_point_cloud(40 + i)), rng, voxel, bb.sparse_shape, i) for i in range(a.agents)]
    vox = {"voxel_features": torch.cat([p[0] for p in parts]).to(dev), "voxel_coords": torch.cat([p[1] for p in parts]).to(dev),
           "voxel_num_points": torch.cat([p[2] for p in parts]).to(dev)}
    M = vox["voxel_coords"].shape[0]
    bb.site_capacity = 2 * M                                   # the bound capacity_in * 8 per strided layer is gigabytes of neighbour table at this grid
    vfe, hc = sparse3d.MeanVFE(args["mean_vfe"], 4), sparse3d.HeightCompression(args["map2bev"])

    def forward(route):
        os.environ["COALIGN_SP3D"] = route
        with torch.no_grad():
            return hc(bb(vfe(dict(vox, batch_size=a.agents))))

    out = {r: forward(r) for r in ("1", "0")}                 # warm-up of both routes at this shape (allocator, weight images)
    torch.cuda.synchronize()
    k, t = out["1"], out["0"]
    levels = {n: int(x.count.item()) for n, x in k["multi_scale_3d_features"].items()}
    levels["conv_out"] = int(k["encoded_spconv_tensor"].count.item())
    torch_levels = {n: x.rows() for n, x in t["multi_scale_3d_features"].items()}
    torch_levels["conv_out"] = t["encoded_spconv_tensor"].rows()
    diff = float((k["spatial_features"] - t["spatial_features"]).abs().max()) / max(float(t["spatial_features"].abs().max()), 1e-30)
    seen, workspace = set(), 0
    for x in list(k["multi_scale_3d_features"].values()) + [k["encoded_spconv_tensor"]]:
        for ten in [x._index, *x._nbr.values()]:
            if ten is not None and ten.data_ptr() not in seen:
                seen.add(ten.data_ptr())
                workspace += ten.numel() * ten.element_size()
    ops.PROFILE = {}
    forward("1")
    torch.cuda.synchronize()
    calls = {n: len(v) for n, v in ops.PROFILE.items()}
    ops.PROFILE = None
    launches = sum(LAUNCHES.get(n, 1) * c for n, c in calls.items())
    times = {"1": [], "0": []}
    for _ in range(a.rounds):
        for route in ("1", "0"):
            forward(route)                                      # (the route's first forward of a round is not timed)
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(a.forwards):
                forward(route)
            e.record()
            torch.cuda.synchronize()
            times[route].append(s.elapsed_time(e) / a.forwards)

    def stats(v):
        return {"median_ms": float(np.median(v)), "min_ms": float(min(v)), "max_ms": float(max(v)), "rounds_ms": [float(x) for x in v]}

    result = {"config": a.config, "agents": a.agents, "sparse_shape": list(bb.sparse_shape), "voxels": M, "site_capacity": 2 * M,
              "sites_kernel_route": levels, "sites_torch_route": torch_levels, "status_word": int(bb.last_status.item()) if bb.last_status is not None else None,
              "kernel_vs_torch_worst_of_scale": diff, "kernel_route": stats(times["1"]), "torch_route": stats(times["0"]),
              "kernel_route_workspace_bytes": workspace, "kernel_route_abi_calls": calls, "kernel_route_launches": launches,
              "method": f"device events, {a.rounds} alternating rounds x {a.forwards} forwards, both routes warmed up at this shape; the count of launches leaves out the "
                        "two torch fills (count, status word) of a forward",
              "reference": "not timed: spconv is not installed, the reference cannot run this model here"}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(result, open(a.out, "w"), indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
