"""``FramePipeline(aligner=...)`` on the MI355X: pose-corrected frames inside the lane's frame (eager and captured) against the eager driver
``inference_intermediate_fusion_aligned`` on the same inputs -- detections ``torch.equal``, ``pipe.alignments`` equal to the driver's status word and corrected
poses --, with planted and with real stage-1 models, from pillars and from raw points; the refusals; and a pipeline without an aligner."""
import copy

import numpy as np
import pytest
import torch

from coalign_amd import box_align, ops
from coalign_amd.config import builtin_config, load_point_pillar_params
from coalign_amd.detector import build_model, to_device
from coalign_amd.inference import inference_intermediate_fusion_aligned
from coalign_amd.pipeline import FramePipeline
from coalign_amd.pose import generate_noise
from coalign_amd.postprocess import build_postprocessor
from coalign_amd.synthetic import calibrate_heads_, fill_parameters_, make_frame, make_point_cloud, make_poses
from tests.test_pose_correction_gpu import FLAGS, _dair_scene, _heads

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _same(a, b):
    return (a is None and b is None) or (a is not None and b is not None and a.shape == b.shape and torch.equal(a, b))


def _driver(frame, model, pp, anchors, stage1_model, pp1, a1, corrector):
    """The eager driver on one pipeline frame -> (boxes, scores, status word, corrected poses ndarray)."""
    ego = dict(frame, anchor_box=anchors, anchor_box_stage1=a1, transformation_matrix=torch.eye(4, device=DEV))
    res = inference_intermediate_fusion_aligned({"ego": ego}, model, pp, stage1_model=stage1_model, stage1_post_processor=pp1, corrector=corrector)
    torch.cuda.synchronize()
    return res["pred_box_tensor"], res["pred_score"], int(res["align_status"][0]), res["lidar_poses_corrected"].cpu().numpy().copy()


def _compare(pipe, results, want, order):
    assert [r[0] for r in results] == list(range(len(order)))
    assert [a[0] for a in pipe.alignments] == list(range(len(order)))
    for (idx, boxes, scores), (_, status, poses), i in zip(results, pipe.alignments, order):
        wb, ws, wstat, wposes = want[i]
        assert _same(boxes, wb) and _same(scores, ws), f"frame {idx} (input {i}): detections differ from the eager driver's"
        assert status == wstat and poses.dtype == np.float64 and np.array_equal(poses, wposes), f"frame {idx} (input {i}): alignment {status} vs {wstat}"


# ------------------------------------------------------------------------------------------------ planted stage 1
@pytest.mark.parametrize("graph", [True, False], ids=["hip_graph", "eager"])
def test_planted_stage1_frames_equal_the_eager_driver(graph):
    """The two-agent DAIR-geometry scene; the stage-1 "model" returns static head tensors the test rewrites between frames (the inputs of
    ``test_chain_in_one_captured_graph``: ``ALIGN_SOLVED`` with different matrices).  Frame order 1, 2, 0, 1: nothing of a previous frame survives in the slot."""
    S = _dair_scene()
    model, pp, pp1, a1, fd = S["model"], S["pp"], S["pp1"], S["a1"], S["fd"]
    inputs = []
    for k, sigma in enumerate((0.2, 0.4, 0.6)):
        rs = np.random.RandomState(100 + k)
        views = [v[rs.permutation(len(v))[: len(v) - 2 * k]] for v in S["views"]]
        noisy = np.array([p + generate_noise(sigma, sigma, rng=rs) for p in S["clean"]])
        inputs.append((_heads(views, S["anchors1"], rs), noisy))
    static_heads = {k: v.clone() for k, v in inputs[0][0].items()}
    stage1 = lambda data: static_heads
    aligner = box_align.Aligner(stage1, pp1, a1, FLAGS, 5, S["H"], S["W"], S["ratio"])

    def load(i):
        for k in static_heads:
            static_heads[k].copy_(inputs[i][0][k])
        frame = {k: v for k, v in fd.items() if k != "pairwise_t_matrix"}                  # (ignored by an aligned pipeline, and may be absent)
        return dict(frame, lidar_poses=inputs[i][1] if i != 1 else torch.from_numpy(inputs[i][1]).to(DEV))      # poses on the host or on the device

    want = []
    corrector = aligner.corrector(DEV)
    for i in range(3):
        want.append(_driver(dict(load(i), pairwise_t_matrix=fd["pairwise_t_matrix"]), model, pp, S["anchors"], stage1, pp1, a1, corrector))
    assert all(w[2] == ops.ALIGN_SOLVED for w in want) and not np.array_equal(want[0][3], want[1][3]) and want[0][0].shape[0] > 30
    pipe = FramePipeline(model, build_postprocessor(S["hd"]["postprocess"], False), S["anchors"], lanes=1, result_lag=0, graph=graph, device=DEV, aligner=aligner)
    try:
        order, results = [1, 2, 0, 1], []
        for i in order:
            results += pipe.submit(load(i))
            torch.cuda.synchronize()
        results += pipe.drain()
        _compare(pipe, results, want, order)
        assert pipe.graphs_captured == (1 if graph else 0)
    finally:
        pipe.close()


# ------------------------------------------------------------------------------------------------ real stage 1
def _mini_world():
    """``mini_coalign`` + ``mini_pointpillar_uncertainty`` (same grid), seeded parameters, heads calibrated so that both emit candidates."""
    h, h1 = builtin_config("mini_coalign"), builtin_config("mini_pointpillar_uncertainty")
    model, model1 = build_model(h), build_model(h1)
    fill_parameters_(model, seed=0)
    fill_parameters_(model1, seed=3)
    model, model1 = model.to(DEV).eval(), model1.to(DEV).eval()
    pp, pp1 = build_postprocessor(h["postprocess"], False), build_postprocessor(h1["postprocess"], False)
    anchors, a1 = torch.from_numpy(pp.generate_anchor_box()), torch.from_numpy(pp1.generate_anchor_box())
    first = to_device(make_frame(h, 3, pillars_per_agent=150, seed=40, spread_xy=(4.0, 2.0), spread_yaw=45.0), DEV)
    calibrate_heads_(model, first, pp.params["target_args"]["score_threshold"], 150)
    calibrate_heads_(model1, first, pp1.params["target_args"]["score_threshold"], 200)
    vfe = model.pillar_vfe
    # (no hard-case rule: whatever clusters the random-weight detections form are solved, so the corrected poses differ from the noisy ones)
    aligner = box_align.Aligner(model1, pp1, a1, dict(use_uncertainty=True, landmark_SE2=True), 5, vfe.ny, vfe.nx, float(vfe.voxel_size[0]), 2)
    return dict(h=h, h1=h1, model=model, model1=model1, pp=pp, pp1=pp1, anchors=anchors, a1=a1, aligner=aligner)


@pytest.fixture(scope="module")
def mini():
    w = _mini_world()
    frames = []
    for i, (n, m) in enumerate([(2, 120), (3, 131), (2, 144), (3, 157), (2, 170), (3, 120)]):      # 2 and 3 agents, ragged pillar counts
        f = to_device(make_frame(w["h"], n, pillars_per_agent=m, seed=60 + i, spread_xy=(4.0, 2.0), spread_yaw=45.0), DEV)
        poses = np.array(make_poses(np.random.RandomState(60 + i), n, noise=(0.2, 0.2), spread_xy=(4.0, 2.0), spread_yaw=45.0))
        frames.append(dict(f, lidar_poses=poses))
    corrector = w["aligner"].corrector(DEV)
    with torch.no_grad():
        w["want"] = [_driver(f, w["model"], w["pp"], w["anchors"], w["model1"], w["pp1"], w["a1"], corrector) for f in frames]
    w["frames"] = frames
    assert sum(0 if b is None else b.shape[0] for b, *_ in w["want"]) > 0
    store = w["pp1"].post_process_stage1_device(w["model1"]({"processed_lidar": frames[1]["processed_lidar"]}), w["a1"], corrector.store)
    torch.cuda.synchronize()
    print("stage-1 boxes per agent:", store.count[:3].tolist(), "statuses:", [x[2] for x in w["want"]])
    assert int(store.count[:3].sum()) > 0, "the stage-1 model must emit boxes"
    return w


@pytest.mark.parametrize("graph", [True, False], ids=["hip_graph", "eager"])
def test_real_stage1_frames_equal_the_eager_driver(mini, graph):
    """``lanes=2, queue_depth=2``: four pipeline lanes, twelve frames -- every lane sees three frames of other pillar counts, so a stale stage-1 canvas shows as a
    mismatch on a lane's second frame.  ``PointPillarUncertainty`` takes no frame record: the pipeline switches to copied frames (``frames_copied``)."""
    w = mini
    pipe = FramePipeline(w["model"], build_postprocessor(w["h"]["postprocess"], False), w["anchors"], lanes=2, queue_depth=2, result_lag=3, graph=graph, device=DEV,
                         aligner=w["aligner"])
    try:
        assert w["model"].pillar_vfe.persistent_canvas and w["model1"].pillar_vfe.persistent_canvas
        order, results = [0, 1, 2, 3, 4, 5, 3, 2, 1, 0, 5, 4], []
        for i in order:
            results += pipe.submit(w["frames"][i])
        results += pipe.drain()
        _compare(pipe, results, w["want"], order)
        if graph:
            assert pipe.frames_copied == len(order) and pipe.frames_in_place == 0
            assert 4 <= pipe.graphs_captured <= 4 * 2 * 2                                  # per lane and agent count: one exact capture + one capacity-sized (the bucket rule)
    finally:
        pipe.close()
    assert not w["model"].pillar_vfe.persistent_canvas and not w["model1"].pillar_vfe.persistent_canvas
    assert "_canvas_cache" not in w["model1"].pillar_vfe.__dict__


@pytest.mark.parametrize("graph", [True, False], ids=["hip_graph", "eager"])
def test_submit_points_with_an_aligner(mini, graph):
    """Two raw clouds per frame through ``submit_points`` against the from-pillars result of the same frame (the clouds voxelised up front, the eager driver)."""
    from coalign_amd.preprocess import build_preprocessor
    w = mini
    pre = build_preprocessor(w["h"]["preprocess"], False, DEV)
    raw, want = [], []
    corrector = w["aligner"].corrector(DEV)
    for i in range(2):
        clouds = [make_point_cloud(900 + 2 * i + a, beams=32, azimuth_steps=450, max_range=14.0, n_boxes=6) for a in range(2)]
        poses = np.array(make_poses(np.random.RandomState(90 + i), 2, noise=(0.2, 0.2), spread_xy=(4.0, 2.0), spread_yaw=45.0))
        raw.append({"clouds": clouds, "record_len": [2], "lidar_poses": poses})
        out = pre.preprocess_clouds(clouds, ego_filter=True)
        pillars = {"processed_lidar": {k: out[k] for k in ("voxel_features", "voxel_coords", "voxel_num_points")}, "record_len": [2], "lidar_poses": poses,
                   "pairwise_t_matrix": torch.eye(4, dtype=torch.float64, device=DEV).repeat(1, 5, 5, 1, 1)}
        assert out["voxel_features"].shape[0] > 50
        with torch.no_grad():
            want.append(_driver(pillars, w["model"], w["pp"], w["anchors"], w["model1"], w["pp1"], w["a1"], corrector))
    pipe = FramePipeline(w["model"], build_postprocessor(w["h"]["postprocess"], False), w["anchors"], lanes=2, result_lag=1, graph=graph, device=DEV,
                         aligner=w["aligner"], preprocessor=pre, points_per_cloud=16384)
    try:
        order, results = [0, 1, 1, 0, 0, 1], []
        for i in order:
            results += pipe.submit_points(raw[i])
        results += pipe.drain()
        _compare(pipe, results, want, order)
    finally:
        pipe.close()


# ------------------------------------------------------------------------------------------------ refusals, and no aligner
def test_refusals(mini):
    w = mini
    pp = build_postprocessor(w["h"]["postprocess"], False)
    with pytest.raises(ValueError, match="exchange"):
        FramePipeline(w["model"], pp, w["anchors"], lanes=1, device=DEV, aligner=w["aligner"], exchange=[lambda feats: (feats, None)])
    h1 = copy.deepcopy(builtin_config("mini_pointpillar_uncertainty"))
    rng = [-12.4, -6.0, -3, 12.4, 6.0, 1]
    h1["preprocess"]["cav_lidar_range"] = h1["postprocess"]["anchor_args"]["cav_lidar_range"] = rng
    other = build_postprocessor(load_point_pillar_params(h1)["postprocess"], False)
    with pytest.raises(ValueError, match="canvas"):
        FramePipeline(w["model"], pp, w["anchors"], lanes=1, device=DEV,
                      aligner=box_align.Aligner(w["model1"], other, torch.from_numpy(other.generate_anchor_box()), FLAGS, 5, 32, 64, 0.4, 2))
    h1 = copy.deepcopy(builtin_config("mini_pointpillar_uncertainty"))                # the same range on another voxel grid (0.8 m: 32 x 16 voxels)
    h1["preprocess"]["args"]["voxel_size"] = [0.8, 0.8, 4]
    coarse = build_postprocessor(load_point_pillar_params(h1)["postprocess"], False)
    assert coarse.params["anchor_args"]["cav_lidar_range"] == w["pp1"].params["anchor_args"]["cav_lidar_range"] and coarse.params["anchor_args"]["W"] == 32
    with pytest.raises(ValueError, match="canvas"):
        FramePipeline(w["model"], pp, w["anchors"], lanes=1, device=DEV,
                      aligner=box_align.Aligner(w["model1"], coarse, torch.from_numpy(coarse.generate_anchor_box()), FLAGS, 5, 32, 64, 0.4, 2))
    assert not w["model"].pillar_vfe.persistent_canvas and not w["model1"].pillar_vfe.persistent_canvas      # a refused construction touched neither model
    narrow = box_align.Aligner(w["model1"], w["pp1"], w["a1"], FLAGS, 2, 32, 64, 0.4, 2)
    for graph in (False, True):
        pipe = FramePipeline(w["model"], pp, w["anchors"], lanes=1, graph=graph, device=DEV, aligner=w["aligner"])
        tight = FramePipeline(w["model"], pp, w["anchors"], lanes=1, graph=graph, device=DEV, aligner=narrow)
        try:
            f2, f3 = w["frames"][0], w["frames"][1]
            with pytest.raises(ValueError, match="one sample"):
                pipe.submit(dict(f2, record_len=[1, 1]))
            with pytest.raises(ValueError, match="agents"):
                pipe.submit(dict(f2, record_len=[9], lidar_poses=np.zeros((9, 6))))
            with pytest.raises(ValueError, match="max_cav"):
                tight.submit(f3)
            with pytest.raises(ValueError, match="lidar_poses"):
                pipe.submit({k: v for k, v in f2.items() if k != "lidar_poses"})
            with pytest.raises(ValueError, match="lidar_poses"):
                pipe.submit(dict(f2, lidar_poses=np.zeros((3, 6))))
            assert pipe.drain() == [] and tight.drain() == [] and pipe.graphs_captured == 0
        finally:
            tight.close()                # (built second on the same models: it gives back the flags the first one had set)
            pipe.close()


@pytest.mark.parametrize("graph", [True, False], ids=["hip_graph", "eager"])
def test_a_pipeline_without_an_aligner_never_touches_lidar_poses(mini, graph):
    class Untouchable:
        def __getattr__(self, name):
            raise AssertionError(f"lidar_poses was touched ({name})")

    w = mini
    pp = build_postprocessor(w["h"]["postprocess"], False)
    meta = {"ego": {"transformation_matrix": torch.eye(4, device=DEV), "anchor_box": w["anchors"]}}
    frames = [dict(f, lidar_poses=Untouchable()) for f in w["frames"][:3]]
    with torch.no_grad():
        want = [w["pp"].post_process(meta, {"ego": w["model"](f)}) for f in frames]
    pipe = FramePipeline(w["model"], pp, w["anchors"], lanes=1, result_lag=0, graph=graph, device=DEV, aligner=None)
    try:
        got = pipe.run(frames)
        for i, ((b, s), (wb, ws)) in enumerate(zip(got, want)):
            assert _same(b, wb) and _same(s, ws), i
        assert len(pipe.alignments) == 0
    finally:
        pipe.close()
