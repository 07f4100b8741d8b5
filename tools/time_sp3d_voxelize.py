"""Time the front of the SECOND detectors -- raw point clouds to the input sparse tensor of VoxelBackBone8x -- at the shape of tools/time_sparse3d.py: the OPV2V
grid, 5 agents, ``coalign_amd.synthetic.make_point_cloud`` sweeps.  Four things, every shape warmed up, alternating rounds, median and min .. max:

  kernel_route   ``sparse3d.voxel_sites`` on ``coalign_sp3d_voxelize`` (points on the device -> mean features, indices, count, site index); device events
  torch_route    the same call on torch ops on the same device (COALIGN_SP3D=0); device events
  host_route     what the model needs without it: the oracle's C loop per cloud on the host + the upload of [M, 5, 4] voxels, coords and counts + ``sp3d_mean_vfe`` +
                 ``sp3d_index_build``; host clock around a device synchronise, the C loop's share apart
  forward        ``second_ssfa_uncertainty`` (COALIGN_SP3D=1, COALIGN_SSFA=1) from the points on the device against the same model from the pre-made, already
                 uploaded ``processed_lidar``; device events

    python tools/time_sp3d_voxelize.py [--out profiles/sp3d_voxelize/timing.json] [--agents 5] [--config second/opv2v_second_uncertainty]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from coalign_amd import ops, second, sparse3d  # noqa: E402
from coalign_amd.config import builtin_config  # noqa: E402
from coalign_amd.detector import build_model  # noqa: E402
from coalign_amd.synthetic import make_point_cloud  # noqa: E402
from oracle import coalign_oracle as oracle  # noqa: E402


def stats(v):
    return {"median_ms": float(np.median(v)), "min_ms": float(min(v)), "max_ms": float(max(v)), "rounds_ms": [float(x) for x in v]}


def device_ms(fn, n):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(n):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sp3d_voxelize", "timing.json"))
    ap.add_argument("--agents", type=int, default=5)
    ap.add_argument("--config", default="second/opv2v_second_uncertainty")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=10)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    os.environ["COALIGN_SSFA"] = "1"
    h = builtin_config(a.config)
    pre = h["preprocess"]
    voxel, rng, T, max_voxels = pre["args"]["voxel_size"], pre["cav_lidar_range"], pre["args"]["max_points_per_voxel"], pre["args"]["max_voxel_test"]
    gx, gy, gz = ops.sp3d_voxel_grid(voxel, rng)
    shape = (gz + 1, gy, gx)
    clouds = [np.ascontiguousarray(make_point_cloud(40 + i), dtype=np.float32) for i in range(a.agents)]
    points = torch.from_numpy(np.concatenate(clouds)).to(dev)
    offsets = torch.tensor(np.concatenate([[0], np.cumsum([len(c) for c in clouds])]), dtype=torch.int32, device=dev)
    P = points.shape[0]

    def sites(route, capacity):
        os.environ["COALIGN_SP3D"] = route
        return sparse3d.voxel_sites(points, offsets, voxel, rng, shape, T, max_voxels, capacity)

    first = sites("1", min(P, a.agents * max_voxels))
    M = int(first.cloud_counts[-1].item())
    cap = (M + 4095) // 4096 * 4096
    k, t = sites("1", cap), sites("0", cap)                      # warm-up of both routes at this shape; and they agree, bit for bit
    torch.cuda.synchronize()
    same = bool(int(k.count) == int(t.count) == M and torch.equal(k.indices[:M], t.indices[:M]) and torch.equal(k.features[:M].view(torch.int32), t.features[:M].view(torch.int32)))
    ops.PROFILE = {}
    sites("1", cap)
    torch.cuda.synchronize()
    calls = {n: len(v) for n, v in ops.PROFILE.items()}
    ops.PROFILE = None

    # the host route: the oracle's C loop per cloud, the upload, MeanVFE and the site index
    def host_route():
        t0 = time.perf_counter()
        per = [oracle.points_to_voxel(c, voxel, rng, T, max_voxels) for c in clouds]
        v, co, n = oracle.collate_voxels(per)
        t1 = time.perf_counter()
        vd, cd, nd = torch.from_numpy(v).to(dev), torch.from_numpy(co).to(dev), torch.from_numpy(n).to(dev)
        feats = ops.sp3d_mean_vfe(vd, nd)
        count = torch.full((1,), cd.shape[0], dtype=torch.int32, device=dev)
        index = ops.sp3d_index_build(ops._aligned16(cd), count, a.agents, shape)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        return (t2 - t0) * 1e3, (t1 - t0) * 1e3, {"voxel_features": vd, "voxel_coords": cd, "voxel_num_points": nd}, feats, index

    _, _, lidar, host_feats, _ = host_route()                    # warm-up (the oracle's library is built and loaded here)
    host_M = lidar["voxel_coords"].shape[0]
    order = torch.argsort(((lidar["voxel_coords"][:, 0].long() * shape[0] + lidar["voxel_coords"][:, 1]) * shape[1] + lidar["voxel_coords"][:, 2]) * shape[2] + lidar["voxel_coords"][:, 3])
    same_as_host = bool(host_M == M and torch.equal(lidar["voxel_coords"][order], k.indices[:M]) and torch.equal(host_feats[order].view(torch.int32), k.features[:M].view(torch.int32)))

    model = build_model(h).eval().to(dev)
    model.spconv_block.site_capacity = 2 * cap

    def forward(from_points):
        os.environ["COALIGN_SP3D"] = "1"
        with torch.no_grad():
            if from_points:
                x = sparse3d.voxel_sites(points, offsets, voxel, rng, shape, T, max_voxels, cap)
                return model({"processed_lidar": {"voxel_sites": x}})
            return model({"processed_lidar": lidar, "batch_size": a.agents})

    fa, fb = forward(True), forward(False)
    torch.cuda.synchronize()
    forward_same = all(torch.equal(fa[key], fb[key]) for key in fb)
    times = {"kernel": [], "torch": [], "host": [], "host_c_loop": [], "forward_points": [], "forward_premade": []}
    for _ in range(a.rounds):
        for name, fn in (("kernel", lambda: sites("1", cap)), ("torch", lambda: sites("0", cap)), ("forward_points", lambda: forward(True)),
                         ("forward_premade", lambda: forward(False))):
            fn()                                                 # (a route's first call of a round is not timed)
            torch.cuda.synchronize()
            times[name].append(device_ms(fn, a.calls if name != "torch" else max(a.calls // 5, 1)))
        total, loop = host_route()[:2]
        times["host"].append(total)
        times["host_c_loop"].append(loop)
    trunk_ms = 1.69                                              # MeanVFE + VoxelBackBone8x + to-dense at this shape
    kernel = stats(times["kernel"])
    result = {"config": a.config, "agents": a.agents, "sparse_shape": list(shape), "points": int(P), "points_per_cloud": [len(c) for c in clouds], "voxels": M,
              "voxels_per_cloud": [int(v) for v in first.cloud_counts[:-1].tolist()], "capacity": cap, "max_points": T, "max_voxels": max_voxels,
              "status_word": int(k.status.item()), "kernel_equals_torch_route_bitwise": same, "kernel_equals_host_route_bitwise": same_as_host,
              "forward_from_points_equals_forward_from_premade_bitwise": forward_same,
              "kernel_route": kernel, "torch_route": stats(times["torch"]), "host_route": stats(times["host"]), "host_route_c_loop_share": stats(times["host_c_loop"]),
              "forward_from_points": stats(times["forward_points"]), "forward_from_premade_processed_lidar": stats(times["forward_premade"]),
              "kernel_route_abi_calls": calls, "kernel_route_launches": 11 + T,
              "kernel_route_share_of_the_1.69_ms_trunk": kernel["median_ms"] / trunk_ms,
              "method": f"{a.rounds} alternating rounds; device events over {a.calls} calls (torch route: {max(a.calls // 5, 1)}) after one untimed call; host route: host clock "
                        "around the C loop, the upload, sp3d_mean_vfe, sp3d_index_build and a device synchronise, once per round"}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(result, open(a.out, "w"), indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
