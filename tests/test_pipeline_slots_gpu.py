"""GPU tests of the two slot-table behaviours of FramePipeline's HIP-graph path (coalign_amd/pipeline.py) that no other test reaches: a captured frame is
dropped and captured again when a weight of the model has changed (a graph bakes pointers to the folded / packed weight images of its moment), and a lane
keeps at most ``max_graphs_per_lane`` captured frames, the oldest leaving first.  The smallest world of the pipeline tests: mini_coalign, 3 agents,
120-170 pillars per agent, heads scaled so that frames carry detections (tests/test_round4_gpu.py::test_ragged_pillar_counts_share_a_capacity_sized_graph).
"""
import pytest
import torch

from coalign_amd import pipeline as pl_mod
from coalign_amd.config import builtin_config
from coalign_amd.detector import build_model, to_device
from coalign_amd.postprocess import build_postprocessor
from coalign_amd.synthetic import fill_parameters_, make_frame

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _world(pillars):
    """-> (hypes, model, anchors, one frame per entry of ``pillars``)."""
    h = builtin_config("mini_coalign")
    model = build_model(h)
    fill_parameters_(model, seed=0, cls_bias=-1.0)
    with torch.no_grad():
        model.reg_head.weight.mul_(0.01); model.reg_head.bias.zero_(); model.cls_head.weight.mul_(0.05)
    model = model.to(DEV).eval()
    anchors = torch.from_numpy(build_postprocessor(h["postprocess"], False).generate_anchor_box())
    frames = [to_device(make_frame(h, 3, pillars_per_agent=m, seed=40 + i, spread_xy=(4.0, 2.0), spread_yaw=45.0), DEV) for i, m in enumerate(pillars)]
    return h, model, anchors, frames


def _same(a, b):
    (ba, sa), (bb, sb) = a, b
    if ba is None or bb is None:
        return ba is None and bb is None
    return ba.shape == bb.shape and torch.equal(ba, bb) and torch.equal(sa, sb)


def test_a_weight_change_recaptures_every_lanes_graph():
    """An in-place write to a parameter, then a load_state_dict: each drops the captured frames (``_weights_signature``) and every lane captures once more --
    detections equal ``post_process(model(frame))`` under the CURRENT weights and differ from the run before, so a graph replaying the old weight images fails."""
    lanes = 2
    h, model, anchors, frames = _world([150] * 6)
    assert len({tuple(f["processed_lidar"]["voxel_features"].shape) for f in frames}) == 1
    pp = build_postprocessor(h["postprocess"], False)
    meta = {"ego": {"transformation_matrix": torch.eye(4, device=DEV), "anchor_box": anchors}}

    def synchronous():
        with torch.no_grad():
            return [pp.post_process(meta, {"ego": model(f)}) for f in frames]

    def bias_write():
        with torch.no_grad():
            model.cls_head.bias.add_(0.25)

    def state_dict_load():
        sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
        sd["reg_head.bias"] = sd["reg_head.bias"] + 0.05
        model.load_state_dict(sd)

    pipe = pl_mod.FramePipeline(model, build_postprocessor(h["postprocess"], False), anchors, lanes=lanes, result_lag=1, graph=True, device=DEV)
    try:
        prev = pipe.run(frames)
        for i, (g, w) in enumerate(zip(prev, synchronous())):
            assert _same(g, w), f"frame {i} before any change"
        assert sum(0 if b is None else b.shape[0] for b, _ in prev) > 0
        assert pipe.graphs_captured == lanes
        held = [len(d) for d in pipe._slots]
        for change in (bias_write, state_dict_load):
            captured = pipe.graphs_captured
            change()
            want = synchronous()
            got = pipe.run(frames)
            for i, (g, w) in enumerate(zip(got, want)):
                assert _same(g, w), f"frame {i} after {change.__name__}"
            for k in range(lanes):          # (frame i ran on lane i mod lanes: a lane that replayed its old graph would repeat the run before)
                assert any(not _same(g, p) for g, p in list(zip(got, prev))[k::lanes]), f"lane {k} after {change.__name__}"
            assert pipe.graphs_captured == captured + lanes, (change.__name__, pipe.graphs_captured)
            assert all(len(d) <= n for d, n in zip(pipe._slots, held))
            prev = got
    finally:
        pipe.close()


@pytest.fixture(scope="module")
def ragged():
    """Five frames of five pillar counts and what the eager pipeline returns for them, the first frame once more at the end."""
    h, model, anchors, frames = _world([120, 131, 144, 157, 170])
    assert len({int(f["processed_lidar"]["voxel_features"].shape[0]) for f in frames}) == 5
    frames = frames + frames[:1]
    eager = pl_mod.FramePipeline(model, build_postprocessor(h["postprocess"], False), anchors, lanes=1, result_lag=0, graph=False, device=DEV)
    want = eager.run(frames)
    eager.close()
    assert sum(0 if b is None else b.shape[0] for b, _ in want) > 0
    return {"hypes": h, "model": model, "anchors": anchors, "frames": frames, "want": want}


@pytest.mark.parametrize("records", [True, False], ids=["in_place", "copied"])
def test_a_lane_keeps_four_captured_frames_and_evicts_the_oldest(ragged, records):
    """Without capacity buckets every pillar count is a graph of its own: the fifth evicts the first, which is captured again when its frame comes back."""
    w = ragged
    keep, pipe = pl_mod.FRAME_RECORDS, None
    try:
        pl_mod.FRAME_RECORDS = records
        pipe = pl_mod.FramePipeline(w["model"], build_postprocessor(w["hypes"]["postprocess"], False), w["anchors"], lanes=1, result_lag=0, graph=True,
                                    pillar_buckets=False, device=DEV)
        assert pipe.max_graphs_per_lane == 4
        got = []
        for f in w["frames"]:
            got += [(b, s) for _, b, s in pipe.submit(f)]
            assert len(pipe._slots[0]) <= pipe.max_graphs_per_lane
        got += [(b, s) for _, b, s in pipe.drain()]
        assert pipe.graphs_captured == 6
        assert (pipe.frames_in_place, pipe.frames_copied) == ((6, 0) if records else (0, 6))      # (the two cases are two input forms, not one twice)
        assert len(got) == 6
        for i, (g, x) in enumerate(zip(got, w["want"])):
            assert _same(g, x), f"frame {i}"
    finally:
        pl_mod.FRAME_RECORDS = keep
        if pipe is not None:
            pipe.close()
