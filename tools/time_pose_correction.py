"""Time the online pose correction (include/coalign_amd_align.h) against the host chain it replaces, from stage-1 head maps to a device-resident normalised
affine matrix, on two scenes with a trained-like box count (40-80 kept boxes per agent): the 2-agent DAIR-V2X-C geometry and a 5-agent OPV2V geometry.

  (i)  host chain: post_process_stage1 -> box_alignment_relative_sample_np (host graph, device solve) -> get_pairwise_transformation -> normalize_pairwise_np
       -> upload;
  (ii) device chain: post_process_stage1_device -> PoseCorrector.correct, eager and as ONE captured graph replayed.

Warm-up, then --reps timed repetitions each (device-synchronised wall time): median and p90, with the solver's LM iteration count.

    python tools/time_pose_correction.py [--reps 200] [--out FILE]
    python tools/time_pose_correction.py --stage1 [--reps 200] [--out FILE]        # stage 1 alone: the one-pass form against the per-agent launches it replaced
    python tools/time_pose_correction.py --pipeline [--frames 300] [--out FILE]    # FramePipeline without / with the aligner, one-pass and per-agent stage 1

--stage1 and --pipeline follow one protocol: warm-up, both versions in ONE process, alternating, several rounds each; a round of --stage1 is device events around
``--reps`` graph replays.  The spread over the rounds of one version is printed beside the difference between the versions.
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/time_pose_correction.py --replay-only 200      # per-kernel split of the graph replay
"""
import argparse
import copy
import json
import math
import os
import sys
import time
import weakref

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from coalign_amd import box_align  # noqa: E402
from coalign_amd.config import builtin_config, load_point_pillar_params  # noqa: E402
from coalign_amd.pose import generate_noise, get_pairwise_transformation, normalize_pairwise_np  # noqa: E402
from coalign_amd.postprocess import build_postprocessor  # noqa: E402

DEV = torch.device("cuda:0")
FLAGS = dict(use_uncertainty=True, landmark_SE2=True, adaptive_landmark=False, normalize_uncertainty=False, abandon_hard_cases=True, drop_hard_boxes=True)


def stage1_hypes(dair: bool, canvas_of: str = None):
    """The stage-1 config; ``canvas_of``: on the range and voxel grid of that fusion config (FramePipeline feeds both encoders the same pillars)."""
    h = copy.deepcopy(builtin_config("opv2v_pointpillar_uncertainty"))
    if canvas_of is not None and not dair:
        hf = builtin_config(canvas_of)
        rng, vox = list(hf["preprocess"]["cav_lidar_range"]), list(hf["preprocess"]["args"]["voxel_size"])
        h["preprocess"]["cav_lidar_range"], h["preprocess"]["args"]["voxel_size"] = rng, vox
        h["model"]["args"]["lidar_range"], h["model"]["args"]["voxel_size"] = rng, vox
        h["postprocess"]["anchor_args"]["cav_lidar_range"] = rng
        h["postprocess"]["gt_range"] = rng
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


def per_agent_stage1(pp1, heads, a1, store, buffers):
    """The per-agent sequence ``post_process_stage1_device`` ran before the one-pass form: six launches per agent (count, emit, rank16, mask2, reduce2,
    stage1_gather).  ``buffers``: a ``weakref.WeakKeyDictionary`` store -> DecodeBuffers, one per store (stores of different pipeline lanes are filled at the same time)."""
    from coalign_amd import ops
    from coalign_amd.postprocess import NMS_TOP
    cls, reg, unc, dirp = heads["cls_preds"], heads["reg_preds"], heads["unc_preds"], heads.get("dir_preds")
    n_agents, A, H, W = cls.shape
    anchors = pp1._anchors_f32(a1, cls.device)
    buf = buffers.get(store)
    if buf is None:
        buf = buffers[store] = ops.DecodeBuffers(A * H * W, A, H, W, NMS_TOP, cls.device)
    da = pp1.params.get("dir_args", {})
    for i in range(n_agents):
        ops.anchor_decode(buf, 0, cls[i], reg[i], None if dirp is None else dirp[i], anchors, pp1.params["target_args"]["score_threshold"], da.get("dir_offset", 0.0),
                          da.get("num_bins", 2), pp1.params["order"], None, clear_frame=True)
        ops.nms_rotated_device(buf.cand_corners, buf.cand_score, pp1.params["nms_thresh"], NMS_TOP, valid=None, k_dev=buf.counts[1:2], keep=buf.keep,
                               keep_count=buf.keep_count, ws=buf.nms_ws)
        ops.stage1_gather(buf, unc[i], store, i)
    store.n_agents = n_agents
    return store


class Stage1Variant:
    """A stage-1 post-processor as ``box_align.Aligner`` takes it, with ``post_process_stage1_device`` replaced by ``fn(heads, anchor_box, store)``."""

    def __init__(self, pp1, fn):
        self.params, self._fn = pp1.params, fn

    def post_process_stage1_device(self, heads, anchor_box, store):
        return self._fn(heads, anchor_box, store)


def spread(xs):
    xs = sorted(xs)
    return {"median": round(float(np.median(xs)), 4), "min": round(xs[0], 4), "max": round(xs[-1], 4)}


def stage1_alone(reps, rounds=7):
    """Stage 1 alone on the two scenes: each version captured in a graph of its own, ``rounds`` alternating rounds of ``reps`` replays between device events."""
    from coalign_amd import ops
    results = {}
    for name in ("dair_2_agents", "opv2v_5_agents"):
        S = make_scene(name)
        # the head maps as a detector with merged 1 x 1 heads returns them: channel slices of ONE [n, C, H, W] tensor
        merged, sliced, c0 = torch.cat([S["heads"][k] for k in ("cls_preds", "reg_preds", "unc_preds")], dim=1), {}, 0
        for k in ("cls_preds", "reg_preds", "unc_preds"):
            sliced[k] = merged[:, c0: c0 + S["heads"][k].shape[1]]
            c0 += S["heads"][k].shape[1]
        stores = {k: ops.Stage1Store(DEV, 3) for k in ("one_pass", "one_pass_dense_copies", "per_agent")}
        buffers = weakref.WeakKeyDictionary()
        bodies = {"one_pass": lambda: S["pp1"].post_process_stage1_device(sliced, S["a1"], stores["one_pass"]),       # slices read in place (the strided entry point)
                  "one_pass_dense_copies": lambda: S["pp1"].post_process_stage1_device({k: v.contiguous() for k, v in sliced.items()}, S["a1"],
                                                                                       stores["one_pass_dense_copies"]),
                  "per_agent": lambda: per_agent_stage1(S["pp1"], sliced, S["a1"], stores["per_agent"], buffers)}
        stream = torch.cuda.Stream(device=DEV)
        graphs, us = {}, {k: [] for k in bodies}
        with torch.no_grad(), torch.cuda.stream(stream):
            for k, body in bodies.items():
                body()
                stream.synchronize()
                graphs[k] = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graphs[k], stream=stream):
                    body()
            for k in graphs:
                for _ in range(50):
                    graphs[k].replay()
            stream.synchronize()
            same = all(torch.equal(getattr(stores[k], f), getattr(stores["per_agent"], f)) for f in ("corners", "unc", "words") for k in stores)
            for _ in range(rounds):
                for k in graphs:                                                   # alternating
                    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    t0.record(stream)
                    for _ in range(reps):
                        graphs[k].replay()
                    t1.record(stream)
                    t1.synchronize()
                    us[k].append(t0.elapsed_time(t1) * 1e3 / reps)
        r = {"kept_boxes_per_agent": stores["one_pass"].count[: S["n"]].tolist(), "stores_bit_equal": bool(same), "replays_per_round": reps, "rounds": rounds,
             "one_pass_us_per_replay": spread(us["one_pass"]), "one_pass_dense_copies_us_per_replay": spread(us["one_pass_dense_copies"]),
             "per_agent_us_per_replay": spread(us["per_agent"])}
        r["difference_us(per_agent - one_pass, medians)"] = round(r["per_agent_us_per_replay"]["median"] - r["one_pass_us_per_replay"]["median"], 4)
        results[name] = r
        print("stage1_alone", name, json.dumps(r), flush=True)
    return results


def pipeline_runs(n_frames, rounds=3):
    """FramePipeline on the two scenes with a real, calibrated PointPillarUncertainty: no aligner | aligner (one-pass stage 1) | aligner with the per-agent stage 1;
    frames/s at lanes=2, queue_depth=3 and the one-frame-in-flight p50 latency, ``rounds`` alternating rounds each."""
    from coalign_amd.detector import build_model, to_device
    from coalign_amd.pipeline import FramePipeline
    from coalign_amd.synthetic import calibrate_heads_, fill_parameters_, make_frame, make_poses
    results = {}
    for name, cfg, n, pillars, dair in (("dair_2_agents_7000_pillars", "dairv2x_coalign", 2, 7000, True), ("opv2v_5_agents_8000_pillars", "opv2v_coalign", 5, 8000, False)):
        h, h1 = builtin_config(cfg), stage1_hypes(dair, canvas_of=cfg)
        model, model1 = build_model(h), build_model(h1)
        fill_parameters_(model, seed=1)
        fill_parameters_(model1, seed=2)
        model, model1 = model.to(DEV).eval(), model1.to(DEV).eval()
        pp1 = build_postprocessor(h1["postprocess"], False)
        a1 = torch.from_numpy(pp1.generate_anchor_box())
        anchors = torch.from_numpy(build_postprocessor(h["postprocess"], False).generate_anchor_box())
        frames = []
        for i in range(4):
            f = to_device(make_frame(h, n, pillars_per_agent=pillars, seed=5 + i, infra_agent=dair), DEV)
            poses = np.array(make_poses(np.random.RandomState(5 + i), n, noise=(0.2, 0.2), infra_agent=dair))
            frames.append(dict(f, lidar_poses=torch.from_numpy(poses).to(DEV)))
        thr = h["postprocess"]["target_args"]["score_threshold"]
        calibrate_heads_(model, frames[0], thr, 400)
        calibrate_heads_(model1, frames[0], pp1.params["target_args"]["score_threshold"], 150 * n)
        vfe = model.pillar_vfe
        aligner = box_align.Aligner(model1, pp1, a1, FLAGS, 5, vfe.ny, vfe.nx, float(vfe.voxel_size[0]), 2)
        buffers = weakref.WeakKeyDictionary()
        per_agent = Stage1Variant(pp1, lambda heads, anchor_box, store: per_agent_stage1(pp1, heads, anchor_box, store, buffers))
        variants = {"no_aligner": None, "aligner_one_pass": aligner,
                    "aligner_per_agent": box_align.Aligner(model1, per_agent, a1, FLAGS, 5, vfe.ny, vfe.nx, float(vfe.voxel_size[0]), 2)}
        streams = [torch.cuda.Stream(device=DEV) for _ in range(2)]
        fps, p50, statuses = {k: [] for k in variants}, {k: [] for k in variants}, {}
        for _ in range(rounds):
            for k, al in variants.items():                                        # alternating
                for lanes, depth, lag, sink in ((2, 3, 5, fps), (1, 1, 0, p50)):
                    pipe = FramePipeline(model, build_postprocessor(h["postprocess"], False), anchors, lanes=lanes, queue_depth=depth, result_lag=lag, graph=True,
                                         device=DEV, streams=streams, aligner=al)
                    count = n_frames if sink is fps else max(50, n_frames // 3)
                    for i in range(24):
                        pipe.submit(frames[i % 4])
                    pipe.drain()
                    pipe.synchronize()
                    pipe.latencies_ms.clear()
                    t0 = time.perf_counter()
                    for i in range(count):
                        pipe.submit(frames[i % 4])
                    pipe.drain()
                    pipe.synchronize()
                    dt = time.perf_counter() - t0
                    sink[k].append(count / dt if sink is fps else float(np.median(pipe.latencies_ms)))
                    if al is not None:
                        statuses[k] = sorted({a[1] for a in pipe.alignments})
                    copied = pipe.frames_copied
                    pipe.close()
        r = {"frames_per_round": n_frames, "rounds": rounds, "align_statuses_seen": statuses, "frames_copied_in_the_last_pipeline": copied,
             "frames_per_s(lanes=2,queue_depth=3)": {k: spread(v) for k, v in fps.items()}, "one_frame_in_flight_p50_ms": {k: spread(v) for k, v in p50.items()}}
        results[name] = r
        print("pipeline", name, json.dumps(r), flush=True)
        del model, model1
        torch.cuda.empty_cache()
    return results


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
    ap.add_argument("--stage1", action="store_true", help="stage 1 alone: one pass over all agents against the per-agent launches")
    ap.add_argument("--pipeline", action="store_true", help="FramePipeline without / with the aligner")
    ap.add_argument("--frames", type=int, default=300, help="frames per throughput round of --pipeline")
    args = ap.parse_args()
    if args.stage1 or args.pipeline:
        results = {}
        if args.stage1:
            results["stage1_alone"] = stage1_alone(args.reps)
        if args.pipeline:
            results["pipeline"] = pipeline_runs(args.frames)
        torch.cuda.synchronize()
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                json.dump(results, f, indent=1)
        return
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
