"""Frames/s of FramePipeline (graph mode) on opv2v_coalign with ``compression: 4``: the dense-canvas route of before (COALIGN_COMPRESS_SPARSE=0: frames copied into
the graph's buffers) against the sparse-canvas route (frames read in place through frame records), alternating in one process on one box.

    python tools/compressor_pipeline_fps.py [--frames 200] [--rounds 5] [--out profiles/compressor/pipeline_fps.json]

The bench pipeline's form: 5 agents x 8000 pillars, a pool of 4 frames, 2 lane streams x 3 queued frames, result lag 5.  One pipeline per route is built (and its
graphs captured) first; the timed windows alternate between the two.  Needs the GPU.
"""
import argparse
import copy
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from coalign_amd import backbone as bb  # noqa: E402
from coalign_amd.config import builtin_config  # noqa: E402
from coalign_amd.detector import build_model, to_device  # noqa: E402
from coalign_amd.pipeline import FramePipeline  # noqa: E402
from coalign_amd.postprocess import build_postprocessor  # noqa: E402
from coalign_amd.synthetic import calibrate_heads_, fill_parameters_, make_frame  # noqa: E402

DEV = torch.device("cuda:0")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--ratio", type=int, default=4)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("compressor_pipeline_fps needs the GPU")
    h = copy.deepcopy(builtin_config("opv2v_coalign"))
    h["model"]["args"]["compression"] = a.ratio
    model = build_model(h)
    fill_parameters_(model, seed=0)
    model = model.to(DEV).eval()
    pp = build_postprocessor(h["postprocess"], False)
    anchors = torch.from_numpy(pp.generate_anchor_box())
    pool = []
    for i in range(4):
        f = make_frame(h, 5, pillars_per_agent=8000, seed=303 + i, noise=(0.2, 0.2))
        d = to_device(f, DEV)
        d["record_len"] = [5]
        d["pairwise_t_matrix_host"] = f["pairwise_t_matrix"]
        pool.append(d)
    calibrate_heads_(model, pool[0], pp.params["target_args"]["score_threshold"], 600)
    streams = [torch.cuda.Stream(device=DEV) for _ in range(2)]
    pipes = {}
    for name, on in (("dense_canvas", False), ("sparse_canvas", True)):
        bb.COMPRESS_SPARSE = on
        p = FramePipeline(model, build_postprocessor(h["postprocess"], False), anchors, lanes=2, queue_depth=3, result_lag=5, graph=True, device=DEV, streams=streams)
        for i in range(24):                                       # capture + warm-up
            p.submit(pool[i % 4])
        p.drain()
        torch.cuda.synchronize()
        pipes[name] = (on, p, (p.frames_in_place, p.frames_copied))
    fps = {k: [] for k in pipes}
    for _ in range(a.rounds):
        for name, (on, p, _) in pipes.items():
            bb.COMPRESS_SPARSE = on
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            n = 0
            for i in range(a.frames):
                n += len(p.submit(pool[i % 4]))
            n += len(p.drain())
            torch.cuda.synchronize()
            fps[name].append(a.frames / (time.perf_counter() - t0))
            assert n == a.frames
    bb.COMPRESS_SPARSE = True
    med = {k: statistics.median(v) for k, v in fps.items()}
    result = {"config": f"opv2v_coalign + compression: {a.ratio}", "frames_per_window": a.frames, "rounds": a.rounds, "device": torch.cuda.get_device_name(0),
              "frames_per_s_median": {k: round(v, 1) for k, v in med.items()}, "frames_per_s_min_max": {k: [round(min(v), 1), round(max(v), 1)] for k, v in fps.items()},
              "frames_in_place_copied_after_warm_up": {k: list(v[2]) for k, v in pipes.items()},
              "sparse_over_dense": round(med["sparse_canvas"] / med["dense_canvas"], 4)}
    for _, p, _ in pipes.values():
        p.close()
    text = json.dumps(result, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text + "\n")


if __name__ == "__main__":
    main()
