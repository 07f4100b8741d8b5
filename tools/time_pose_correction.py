"""Time the online pose correction (include/coalign_amd_align.h) against the host chain it replaces, from stage-1 head maps to a device-resident normalised
affine matrix, on two scenes with a trained-like box count (40-80 kept boxes per agent): the 2-agent DAIR-V2X-C geometry and a 5-agent OPV2V geometry.

  (i)  host chain: post_process_stage1 -> box_alignment_relative_sample_np (host graph, device solve) -> get_pairwise_transformation -> normalize_pairwise_np
       -> upload;
  (ii) device chain: post_process_stage1_device -> PoseCorrector.correct, eager and as ONE captured graph replayed.

Warm-up, then --reps timed repetitions each (device-synchronised wall time): median and p90, with the solver's LM iteration count.

    python tools/time_pose_correction.py [--reps 200] [--out FILE]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/time_pose_correction.py --replay-only 200      # per-kernel split of the graph replay
"""
import argparse
import copy
import json
import math
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from coalign_amd import box_align  # noqa: E402
from coalign_amd.config import builtin_config, load_point_pillar_params  # noqa: E402
from coalign_amd.pose import generate_noise, get_pairwise_transformation, normalize_pairwise_np  # noqa: E402
from coalign_amd.postprocess import build_postprocessor  # noqa: E402

DEV = torch.device("cuda:0")
FLAGS = dict(use_uncertainty=True, landmark_SE2=True, adaptive_landmark=False, normalize_uncertainty=False, abandon_hard_cases=True, drop_hard_boxes=True)


def stage1_hypes(dair: bool):
    h = copy.deepcopy(builtin_config("opv2v_pointpillar_uncertainty"))
    if dair:
        hd = builtin_config("dairv2x_coalign")
        rng, vox = list(hd["preprocess"]["cav_lidar_range"]), list(hd["preprocess"]["args"]["voxel_size"])
        h["preprocess"]["cav_lidar_range"], h["preprocess"]["args"]["voxel_size"] = rng, vox
        h["model"]["args"]["lidar_range"], h["model"]["args"]["voxel_size"] = rng, vox
        h["postprocess"]["anchor_args"].update({"cav_lidar_range": rng, "l": 4.5, "w": 2, "h": 1.56})
        h["postprocess"]["gt_range"] = rng
    return load_point_pillar_params(h)


def plant(objects, anchors, rs):
    """Head maps whose decode gives exactly ``objects`` ([K, 7] = x, y, z, h, w, l, yaw): logit +4 at the nearest anchor, -9 elsewhere."""
    H, W, A, _ = anchors.shape
    cls = np.full((1, A, H, W), -9.0, np.float32)
    reg = np.zeros((1, A * 7, H, W), np.float32)
    unc = rs.normal(-2.0, 0.3, (1, A * 3, H, W)).astype(np.float32)
    xs, ys = anchors[0, :, 0, 0], anchors[:, 0, 0, 1]
    for b in objects:
        j, i = int(np.abs(xs - b[0]).argmin()), int(np.abs(ys - b[1]).argmin())
        a = int(np.abs(np.cos(b[6] - anchors[i, j, :, 6])).argmax())
        an = anchors[i, j, a]
        d = np.sqrt(an[4] ** 2 + an[5] ** 2)
        cls[0, a, i, j] = 4.0
        reg[0, a * 7: a * 7 + 7, i, j] = [(b[0] - an[0]) / d, (b[1] - an[1]) / d, (b[2] - an[2]) / an[3], np.log(b[3] / an[3]), np.log(b[4] / an[4]),
                                         np.log(b[5] / an[5]), b[6] - an[6]]
    return cls, reg, unc


def make_scene(name: str):
    dair = name == "dair_2_agents"
    h1 = stage1_hypes(dair)
    pp1 = build_postprocessor(h1["postprocess"], False)
    anchors = pp1.generate_anchor_box()
    aa = h1["postprocess"]["anchor_args"]
    rng = aa["cav_lidar_range"]
    rs = np.random.RandomState(42)
    if dair:
        clean = [np.zeros(6), np.array([30.0, 5.0, 0.0, 0.0, 170.0, 0.0])]
        gx, gy = np.meshgrid(np.arange(-24, 72, 12.0), np.arange(-30, 31, 10.0))
    else:
        clean = [np.zeros(6)] + [np.array([rs.uniform(-20, 20), rs.uniform(-10, 10), 0, 0, rs.uniform(-30, 30), 0]) for _ in range(4)]
        gx, gy = np.meshgrid(np.arange(-60, 61, 12.0), np.arange(-30, 31, 10.0))
    world = np.stack([gx.ravel() + rs.uniform(-2, 2, gx.size), gy.ravel() + rs.uniform(-2, 2, gx.size)], 1)
    yaw_w = rs.uniform(-2.5, 2.5, len(world))
    parts = []
    for pose in clean:
        th = math.radians(pose[4])
        R = np.array([[math.cos(th), math.sin(th)], [-math.sin(th), math.cos(th)]])
        xy = (world - pose[:2]) @ R.T + rs.normal(0, 0.05, world.shape)
        inside = (xy[:, 0] > rng[0] + 6) & (xy[:, 0] < rng[3] - 6) & (xy[:, 1] > rng[1] + 6) & (xy[:, 1] < rng[4] - 6)
        obj = np.zeros((int(inside.sum()), 7))
        obj[:, :2], obj[:, 2], obj[:, 3:6], obj[:, 6] = xy[inside], -1.0, [aa["h"], aa["w"], aa["l"]], yaw_w[inside] - th
        parts.append(plant(obj, anchors, rs))
    heads = {k: torch.from_numpy(np.concatenate([p[i] for p in parts])).to(DEV) for i, k in enumerate(("cls_preds", "reg_preds", "unc_preds"))}
    noisy = np.array([p + generate_noise(0.4, 0.4, rng=rs) for p in clean])
    H, W = [int(v) for v in h1["model"]["args"]["point_pillar_scatter"]["grid_size"]][1::-1]
    return dict(pp1=pp1, a1=torch.from_numpy(anchors), heads=heads, noisy=noisy, H=H, W=W, ratio=float(h1["model"]["args"]["voxel_size"][0]), n=len(clean))


def host_chain(S, out_dev):
    corners, _, unc = S["pp1"].post_process_stage1(S["heads"], S["a1"])
    corners = [c.cpu().numpy().astype(np.float64) for c in corners]
    unc = [u.cpu().numpy().astype(np.float64) for u in unc]
    fixed = S["noisy"].copy()
    fixed[:, [0, 1, 4]] = box_align.box_alignment_relative_sample_np(corners, S["noisy"].copy(), uncertainty_list=unc, **FLAGS)
    aff = normalize_pairwise_np(get_pairwise_transformation(fixed, 5)[None], S["H"], S["W"], S["ratio"])
    out_dev.copy_(torch.from_numpy(aff), non_blocking=False)
    return [len(c) for c in corners]


def timed(fn, reps, warm=20):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    ts = np.sort(np.array(ts))
    return {"median_ms": round(float(np.median(ts)), 4), "p90_ms": round(float(ts[int(0.9 * (len(ts) - 1))]), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--out", default=None)
    ap.add_argument("--replay-only", type=int, default=0, help="only N graph replays per scene (for a rocprofv3 --kernel-trace --stats pass)")
    args = ap.parse_args()
    results = {}
    for name in ("dair_2_agents", "opv2v_5_agents"):
        S = make_scene(name)
        corrector = box_align.PoseCorrector(FLAGS, 5, S["H"], S["W"], S["ratio"], device=DEV)
        poses = torch.from_numpy(S["noisy"]).to(DEV)

        def device_chain():
            return corrector.correct(S["pp1"].post_process_stage1_device(S["heads"], S["a1"], corrector.store), poses)

        stream = torch.cuda.Stream(device=DEV)
        with torch.no_grad(), torch.cuda.stream(stream):
            out = device_chain()
            stream.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=stream):
                device_chain()
            if args.replay_only:
                for _ in range(args.replay_only):
                    graph.replay()
                stream.synchronize()
                continue
            host_out = torch.zeros_like(out["normalized_affine_matrix"])
            kept = host_chain(S, host_out)
            graph.replay()
            stream.synchronize()
            r = {"kept_boxes_per_agent": kept, "status": int(out["status"][0]), "lm_iterations": int(corrector.graph.stats[0, 0]),
                 "landmarks": int(corrector.graph.vertex_off[1]) - S["n"], "edges": int(corrector.graph.edge_off[1]),
                 "max_abs_difference_of_the_affine_matrices": float((host_out - out["normalized_affine_matrix"]).abs().max()),
                 "host_chain": timed(lambda: host_chain(S, host_out), args.reps), "device_chain_eager": timed(device_chain, args.reps),
                 "device_chain_graph_replay": timed(graph.replay, args.reps)}
        results[name] = r
        print(name, json.dumps(r), flush=True)
    torch.cuda.synchronize()
    if args.out and results:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
