"""Online pose correction on the MI355X (include/coalign_amd_align.h): the construction kernel graph for graph against ``box_align.build_pose_graph`` and the
reference's recorded graphs, corrected poses against ``box_alignment_relative_sample_np``, the matrices against ``pose.get_pairwise_transformation`` +
``normalize_pairwise_np``, the stage-1 gather against ``post_process_stage1``, the whole chain inside ONE captured graph, and end to end through
``inference_intermediate_fusion_aligned`` against the host chain."""
import copy
import functools
import math

import numpy as np
import pytest
import torch

from coalign_amd import box_align, ops
from coalign_amd.config import builtin_config
from coalign_amd.detector import build_model, to_device
from coalign_amd.pose import generate_noise, get_pairwise_transformation, normalize_pairwise_np
from coalign_amd.postprocess import build_postprocessor
from coalign_amd.synthetic import calibrate_heads_, fill_parameters_, make_frame
from tests.conftest import assert_elementwise
from tests.pose_correction_scenes import order_robust, scene
from tests.test_oracle_golden import BOX_ALIGN_CASES, box_align_inputs

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
NORM = dict(H=100, W=252, discrete_ratio=0.4, downsample_rate=2)


# ------------------------------------------------------------------------------------------------ helpers
def _store(corners, unc):
    """A float64 store holding exactly the host's inputs (the golden boxes are float64 values that float32 cannot hold)."""
    return ops.Stage1Store(DEV, 0 if unc is None else 3, torch.float64).upload(corners, unc)


def _device_graph(corners, noisy, unc, flags):
    store, graph = _store(corners, unc), ops.PoseGraphArrays(DEV)
    poses = torch.from_numpy(np.ascontiguousarray(noisy, dtype=np.float64)).to(DEV)
    ops.pose_graph_build(store, poses, graph, ops.align_flags(**{k: v for k, v in flags.items() if k not in ("thres", "yaw_var_thres")}))
    torch.cuda.synchronize()
    V, E = int(graph.vertex_off[1]), int(graph.edge_off[1])
    host = lambda t, n: t[:n].cpu().numpy()
    return {"status": int(store.status[0]), "V": V, "E": E, "n_agents": int(graph.n_agents[0]), "vertices": host(graph.vertices, V), "kinds": host(graph.kinds, V),
            "edge_agent": host(graph.edge_agent, E), "edge_landmark": host(graph.edge_landmark, E), "edge_meas": host(graph.edge_meas, E),
            "edge_info": host(graph.edge_info, E), "offsets": (int(graph.vertex_off[0]), int(graph.edge_off[0]))}


def _compare_graph(dev, ref_vertices, ref_kinds, ref_agent, ref_landmark, ref_meas, ref_info, n, what):
    """The comparison of the issue's item 5: structure EQUAL, measurements 1e-12 absolute, information 1e-13 relative, agent vertices equal, landmark starting
    values 1e-4 m / 1e-5 rad."""
    assert dev["status"] == ops.ALIGN_SOLVED and dev["offsets"] == (0, 0) and dev["n_agents"] == n, (what, dev["status"])
    assert dev["V"] == len(ref_vertices) and dev["E"] == len(ref_agent), (what, dev["V"], len(ref_vertices), dev["E"], len(ref_agent))
    assert np.array_equal(dev["kinds"], ref_kinds), what
    assert np.array_equal(dev["edge_agent"], ref_agent) and np.array_equal(dev["edge_landmark"], ref_landmark), what
    e_meas = float(np.abs(dev["edge_meas"] - ref_meas).max()) if len(ref_meas) else 0.0
    e_info = float((np.abs(dev["edge_info"] - ref_info) / np.maximum(np.abs(ref_info), 1e-300)).max()) if len(ref_info) else 0.0
    lm_d, lm_r = dev["vertices"][n:], np.asarray(ref_vertices)[n:]
    e_xy = float(np.abs(lm_d[:, :2] - lm_r[:, :2]).max()) if len(lm_r) else 0.0
    e_yaw = float(np.abs(lm_d[:, 2] - lm_r[:, 2]).max()) if len(lm_r) else 0.0
    print(f"{what}: V {dev['V']} E {dev['E']} edge_meas {e_meas:.2e} edge_info {e_info:.2e} (rel) landmarks {e_xy:.2e} m {e_yaw:.2e} rad")
    assert e_meas <= 1e-12 and e_info <= 1e-13, (what, e_meas, e_info)
    assert np.array_equal(dev["vertices"][:n], np.asarray(ref_vertices)[:n]), what
    assert e_xy <= 1e-4 and e_yaw <= 1e-5, (what, e_xy, e_yaw)


def _well_formed(dev, n):
    assert dev["status"] in (ops.ALIGN_SOLVED, ops.ALIGN_KEPT_NOISY), dev["status"]
    assert n <= dev["V"] <= ops.ALIGN_MAX_VERTICES and 0 <= dev["E"] <= ops.ALIGN_MAX_AGENTS * 256
    assert np.all(np.diff(dev["edge_landmark"]) >= 0)
    assert np.all((dev["edge_agent"] >= 0) & (dev["edge_agent"] < n)) and np.all((dev["edge_landmark"] >= n) & (dev["edge_landmark"] < dev["V"]))
    assert np.isfinite(dev["edge_meas"]).all() and np.isfinite(dev["edge_info"]).all() and np.isfinite(dev["vertices"]).all()


def _correct(corners, noisy, unc, flags, max_cav=5, proj_first=False):
    """``PoseCorrector.correct`` on the host's exact inputs -> (poses [N, 6], pairwise, affine, status), host copies."""
    corrector = box_align.PoseCorrector(flags, max_cav, proj_first=proj_first, device=DEV, **NORM)
    out = corrector.correct(_store(corners, unc), torch.from_numpy(np.ascontiguousarray(noisy, dtype=np.float64)).to(DEV))
    torch.cuda.synchronize()
    return out["lidar_poses"].cpu().numpy(), out["pairwise_t_matrix"].cpu().numpy(), out["normalized_affine_matrix"].cpu().numpy(), int(out["status"][0])


def _compare_poses(poses, noisy, corners, unc, flags, what):
    """The issue's item 7: x, y within 1e-5 m, yaw within 1e-4 degrees of ``box_alignment_relative_sample_np`` on the same boxes; z / roll / pitch untouched."""
    ref = box_align.box_alignment_relative_sample_np(corners, np.array(noisy, dtype=np.float64), uncertainty_list=unc, **flags)
    e_xy = float(np.abs(poses[:, :2] - ref[:, :2]).max())
    e_yaw = float(np.abs((poses[:, 4] - ref[:, 2] + 180) % 360 - 180).max())
    print(f"{what}: corrected poses against the host chain {e_xy:.2e} m {e_yaw:.2e} deg")
    assert e_xy <= 1e-5 and e_yaw <= 1e-4, (what, e_xy, e_yaw)
    assert np.array_equal(poses[:, [2, 3, 5]], np.asarray(noisy)[:, [2, 3, 5]]), what


def _compare_matrices(poses, pairwise, affine, max_cav, proj_first, what):
    """The issue's item 8: against the host functions evaluated on the DEVICE's corrected poses, 1e-11 in every entry; padding and proj_first exactly identity."""
    n = len(poses)
    ref = get_pairwise_transformation(poses, max_cav, proj_first)
    ref_aff = normalize_pairwise_np(ref[None], **NORM)
    assert pairwise.shape == (1, max_cav, max_cav, 4, 4) and affine.shape == (1, max_cav, max_cav, 2, 3)
    e_pw, e_aff = float(np.abs(pairwise[0] - ref).max()), float(np.abs(affine - ref_aff).max())
    print(f"{what}: pairwise {e_pw:.2e} affine {e_aff:.2e}")
    assert e_pw <= 1e-11 and e_aff <= 1e-11, (what, e_pw, e_aff)
    eye = np.eye(4)
    for i in range(max_cav):
        for j in range(max_cav):
            if proj_first or i == j or i >= n or j >= n:
                assert np.array_equal(pairwise[0, i, j], eye), (what, i, j)
                assert np.array_equal(affine[0, i, j], ref_aff[0, i, j]), (what, i, j)


# ------------------------------------------------------------------------------------------------ items 5, 7, 8 on the golden cases
@pytest.mark.parametrize("tag", BOX_ALIGN_CASES)
def test_construction_kernel_graph_for_graph_on_the_golden_cases(golden, tag):
    """Item 5: the nine cases of tests/golden/box_align.npz (flag combinations, an empty agent, both abandon rules) -- the device graph against
    ``build_pose_graph`` on the same inputs AND against the arrays recorded from the reference; item 7 on the same case."""
    g = golden("box_align.npz")
    corners, noisy, unc, flags = box_align_inputs(g, tag)
    assert all(order_robust(corners, noisy, unc, **flags)), tag                  # (checked when the issue was written: all nine are order-robust)
    host = box_align.build_pose_graph(corners, noisy, unc, **flags)
    dev = _device_graph(corners, noisy, unc, flags)
    n = len(noisy)
    poses, pairwise, affine, status = _correct(corners, noisy, unc, flags)
    if int(g[f"{tag}_solved"]) == 0:
        assert host is None and dev["status"] == ops.ALIGN_KEPT_NOISY and status == ops.ALIGN_KEPT_NOISY, (tag, dev["status"])
        assert dev["V"] == n and dev["E"] == 0
        assert np.array_equal(poses, noisy), tag                                   # the noisy poses, bit for bit
    else:
        _compare_graph(dev, host.vertices, host.kinds, host.edge_agent, host.edge_landmark, host.edge_meas, host.edge_info, n, f"{tag} vs host")
        _compare_graph(dev, g[f"{tag}_vertices"], g[f"{tag}_kinds"], g[f"{tag}_edge_agent"], g[f"{tag}_edge_landmark"], g[f"{tag}_edge_meas"],
                       g[f"{tag}_edge_info"], n, f"{tag} vs reference")
        assert status == ops.ALIGN_SOLVED
        _compare_poses(poses, noisy, corners, unc, flags, tag)
    _compare_matrices(poses, pairwise, affine, 5, False, tag)


# ------------------------------------------------------------------------------------------------ items 6, 7 on the synthetic sweep
def test_construction_kernel_on_the_synthetic_sweep():
    """Item 6: 200 scenes (N in {2, 3, 5}, 5 cm detection noise, pose noise 0 .. 0.6); the order-robust ones (decided on the CPU from the host functions)
    are compared graph for graph and pose for pose, the others must give a well-formed graph and finite poses.  At most 15 % may be left out."""
    flags = dict(use_uncertainty=False)
    left_out, reasons = 0, np.zeros(3, int)
    for seed in range(200):
        corners, noisy = scene(seed)
        robust = order_robust(corners, noisy)
        dev = _device_graph(corners, noisy, None, flags)
        poses, _, _, status = _correct(corners, noisy, None, flags)
        n = len(noisy)
        if all(robust):
            host = box_align.build_pose_graph(corners, noisy, None, **flags)
            _compare_graph(dev, host.vertices, host.kinds, host.edge_agent, host.edge_landmark, host.edge_meas, host.edge_info, n, f"scene {seed}")
            assert status == ops.ALIGN_SOLVED
            _compare_poses(poses, noisy, corners, None, flags, f"scene {seed}")
        else:
            left_out += 1
            reasons += ~np.array(robust)
            _well_formed(dev, n)
            assert np.isfinite(poses).all(), seed
    print(f"synthetic sweep: {left_out} of 200 scenes not order-robust (a: {reasons[0]}, b: {reasons[1]}, c: {reasons[2]})")
    assert left_out <= 0.15 * 200, left_out


def test_abandoned_and_empty_samples_return_the_noisy_poses():
    """Item 7: with the hard-case rule a 2-agent scene of three objects is abandoned (n_lm <= 3), a sample without any box is "no boxes": both return the noisy
    poses bit for bit with the matching status, and identity-padded matrices of those poses."""
    corners, noisy = scene(3)
    few = [c[:3] for c in corners]
    poses, pairwise, affine, status = _correct(few, noisy, None, dict(use_uncertainty=False, abandon_hard_cases=True))
    assert box_align.build_pose_graph(few, noisy, None, use_uncertainty=False, abandon_hard_cases=True) is None
    assert status == ops.ALIGN_KEPT_NOISY and np.array_equal(poses, noisy)
    _compare_matrices(poses, pairwise, affine, 5, False, "abandoned")
    empty = [np.zeros((0, 8, 3)) for _ in corners]
    poses, pairwise, affine, status = _correct(empty, noisy, None, dict(use_uncertainty=False))
    assert status == ops.ALIGN_NO_BOXES and np.array_equal(poses, noisy)
    _compare_matrices(poses, pairwise, affine, 5, False, "no boxes")
    many = [np.concatenate([c] * 40)[:300] for c in corners]                       # more boxes than a slot of the store holds
    poses, _, _, status = _correct(many, noisy, None, dict(use_uncertainty=False))
    assert status == ops.ALIGN_OUTSIDE_LIMITS | ops.ALIGN_STORE_OVERFLOW and np.array_equal(poses, noisy)


@pytest.mark.parametrize("max_cav", [2, 5, 7])
def test_corrected_matrices_against_the_host_functions(max_cav):
    """Item 8: ``pairwise_t_matrix`` / ``normalized_affine_matrix`` against the host functions on the device's corrected poses, 6-DOF poses with z / roll /
    pitch, padding exactly identity, ``proj_first`` all identity."""
    for seed in (3, 5, 7):                                                          # 2, 5 and 3 agents
        corners, noisy = scene(seed)
        if len(noisy) > max_cav:
            continue
        rs = np.random.RandomState(seed)
        noisy = noisy.copy()
        noisy[:, 2], noisy[:, 3], noisy[:, 5] = rs.uniform(-0.3, 0.3, len(noisy)), rs.uniform(-0.5, 0.5, len(noisy)), rs.uniform(-0.5, 0.5, len(noisy))
        noisy[:, :2] += rs.uniform(-150, 150, 2)                                   # entries up to ~300 m
        for proj_first in (False, True):
            poses, pairwise, affine, status = _correct(corners, noisy, None, dict(use_uncertainty=False), max_cav, proj_first)
            assert status == ops.ALIGN_SOLVED
            _compare_matrices(poses, pairwise, affine, max_cav, proj_first, f"scene {seed} max_cav {max_cav} proj_first {proj_first}")


# ------------------------------------------------------------------------------------------------ the DAIR-geometry scene (items 9 - 11)
def _stage1_hypes():
    """The stage-1 (PointPillarUncertainty) config at DAIR-V2X-C geometry: 504 x 200 canvas, anchors l = 4.5, w = 2."""
    from coalign_amd.config import load_point_pillar_params
    h, hd = copy.deepcopy(builtin_config("opv2v_pointpillar_uncertainty")), builtin_config("dairv2x_coalign")
    rng, vox = list(hd["preprocess"]["cav_lidar_range"]), list(hd["preprocess"]["args"]["voxel_size"])
    h["preprocess"]["cav_lidar_range"], h["preprocess"]["args"]["voxel_size"] = rng, vox
    h["model"]["args"]["lidar_range"], h["model"]["args"]["voxel_size"] = rng, vox
    h["postprocess"]["anchor_args"].update({"cav_lidar_range": rng, "l": 4.5, "w": 2, "h": 1.56})
    h["postprocess"]["gt_range"] = rng
    return load_point_pillar_params(h)


def _plant(objects_agent, anchors, rs):
    """Head maps (cls / reg / unc, [1, A * k, H, W]) whose decode gives exactly ``objects_agent`` ([K, 7] = x, y, z, h, w, l, yaw in the agent's frame): logit +4
    at the nearest anchor, -9 elsewhere; regression deltas = the inverse of the anchor decode."""
    H, W, A, _ = anchors.shape
    cls = np.full((1, A, H, W), -9.0, np.float32)
    reg = np.zeros((1, A * 7, H, W), np.float32)
    unc = rs.normal(-2.0, 0.3, (1, A * 3, H, W)).astype(np.float32)
    xs, ys = anchors[0, :, 0, 0], anchors[:, 0, 0, 1]
    for b in objects_agent:
        j, i = int(np.abs(xs - b[0]).argmin()), int(np.abs(ys - b[1]).argmin())
        a = int(np.abs(np.cos(b[6] - anchors[i, j, :, 6])).argmax())
        an = anchors[i, j, a]
        d = np.sqrt(an[4] ** 2 + an[5] ** 2)
        delta = [(b[0] - an[0]) / d, (b[1] - an[1]) / d, (b[2] - an[2]) / an[3], np.log(b[3] / an[3]), np.log(b[4] / an[4]), np.log(b[5] / an[5]), b[6] - an[6]]
        cls[0, a, i, j] = 4.0
        reg[0, a * 7: a * 7 + 7, i, j] = delta
    return cls, reg, unc


def _objects(xy, yaw):
    obj = np.zeros((len(xy), 7))
    obj[:, :2], obj[:, 2], obj[:, 3:6], obj[:, 6] = xy, -1.0, [1.56, 2.0, 4.5], yaw
    return obj


def _heads(object_lists, anchors, rs):
    parts = [_plant(obj, anchors, rs) for obj in object_lists]
    return {k: torch.from_numpy(np.concatenate([p[i] for p in parts])).to(DEV) for i, k in enumerate(("cls_preds", "reg_preds", "unc_preds"))}


@functools.lru_cache(maxsize=1)
def _stage1():
    h1 = _stage1_hypes()
    pp1 = build_postprocessor(h1["postprocess"], False)
    anchors = pp1.generate_anchor_box()
    return h1, pp1, anchors, torch.from_numpy(anchors)


def _scene_views(clean, rs, rngd, plant_on=None):
    """One scene, one view per agent: objects in the ego (= world) frame, each agent sees the ones inside its range with 5 cm of detection noise.  With
    ``plant_on`` (the stage-1 anchors) each view's head maps are planted right after the view is drawn, and (views, head maps on the device) is returned."""
    gx, gy = np.meshgrid(np.arange(-24, 72, 12.0), np.arange(-30, 31, 10.0))
    world = np.stack([gx.ravel() + rs.uniform(-2, 2, gx.size), gy.ravel() + rs.uniform(-2, 2, gx.size)], 1)
    yaw_w = rs.uniform(-2.5, 2.5, len(world))
    views, parts = [], []
    for pose in clean:
        th = math.radians(pose[4])
        R = np.array([[math.cos(th), math.sin(th)], [-math.sin(th), math.cos(th)]])
        xy = (world - pose[:2]) @ R.T + rs.normal(0, 0.05, world.shape)
        inside = (xy[:, 0] > rngd[0] + 6) & (xy[:, 0] < rngd[3] - 6) & (xy[:, 1] > rngd[1] + 6) & (xy[:, 1] < rngd[4] - 6)
        views.append(_objects(xy[inside], yaw_w[inside] - th))
        if plant_on is not None:
            parts.append(_plant(views[-1], plant_on, rs))
    if plant_on is None:
        return views
    return views, {k: torch.from_numpy(np.concatenate([p[i] for p in parts])).to(DEV) for i, k in enumerate(("cls_preds", "reg_preds", "unc_preds"))}


def _store_lists(store, n_agents):
    counts = store.count.cpu().numpy()
    return ([store.corners[i, : counts[i]].cpu().numpy() for i in range(n_agents)], [store.unc[i, : counts[i]].cpu().numpy() for i in range(n_agents)], counts)


@pytest.mark.parametrize("n_agents", [2, 5])
def test_stage1_gather_equals_post_process_stage1(n_agents):
    """Item 9: the store after ``post_process_stage1_device`` equals ``post_process_stage1``'s lists bit for bit (corners, uncertainties, counts), including an
    agent with no candidate, a frame where nothing passes the threshold, and an agent with more kept boxes than a slot holds."""
    h1, pp1, anchors, a1 = _stage1()
    rs = np.random.RandomState(7 + n_agents)
    rngd = h1["postprocess"]["anchor_args"]["cav_lidar_range"]
    clean = [np.zeros(6)] + [np.array([rs.uniform(-20, 20), rs.uniform(-8, 8), 0, 0, rs.uniform(-40, 40), 0]) for _ in range(n_agents - 1)]
    views = _scene_views(clean, rs, rngd)
    views[1] = views[1][:0]                                                         # an agent with no candidate
    heads = _heads(views, anchors, rs)
    corrector = box_align.PoseCorrector(dict(abandon_hard_cases=True, drop_hard_boxes=True), 5, device=DEV, **NORM)
    store = pp1.post_process_stage1_device(heads, a1, corrector.store)
    torch.cuda.synchronize()
    got_c, got_u, counts = _store_lists(store, n_agents)
    ref_c, _, ref_u = pp1.post_process_stage1(heads, a1)
    assert list(counts[:n_agents]) == [len(c) for c in ref_c] and counts[1] == 0 and counts[0] >= 20 and int(store.status[0]) == 0
    for i in range(n_agents):
        assert np.array_equal(got_c[i], ref_c[i].cpu().numpy()) and np.array_equal(got_u[i], ref_u[i].cpu().numpy()), i
    # nothing passes the threshold: all counts 0, "no boxes", noisy poses pass through
    nothing = _heads([v[:0] for v in views], anchors, rs)
    assert pp1.post_process_stage1(nothing, a1) == (None, None, None)
    store = pp1.post_process_stage1_device(nothing, a1, corrector.store)
    noisy = torch.from_numpy(np.array([p + generate_noise(0.2, 0.2, rng=rs) for p in clean])).to(DEV)
    out = corrector.correct(store, noisy)
    torch.cuda.synchronize()
    assert int(store.count.sum()) == 0 and int(out["status"][0]) == ops.ALIGN_NO_BOXES and torch.equal(out["lidar_poses"], noisy)
    # more kept boxes than a slot holds: the overflow bit, noisy poses pass through
    gx, gy = np.meshgrid(np.arange(-90, 90, 6.0), np.arange(-31.5, 32, 7.0))
    crowd = _objects(np.stack([gx.ravel(), gy.ravel()], 1), np.zeros(gx.size))
    assert len(crowd) == 300
    over = _heads([views[0], crowd] + views[2:], anchors, rs)
    ref_c, _, _ = pp1.post_process_stage1(over, a1)
    assert len(ref_c[1]) > store.boxes
    store = pp1.post_process_stage1_device(over, a1, corrector.store)
    out = corrector.correct(store, noisy)
    torch.cuda.synchronize()
    got_c, _, counts = _store_lists(store, n_agents)
    assert counts[1] == store.boxes and np.array_equal(got_c[1], ref_c[1][: store.boxes].cpu().numpy()) and np.array_equal(got_c[0], ref_c[0].cpu().numpy())
    assert int(out["status"][0]) == ops.ALIGN_OUTSIDE_LIMITS | ops.ALIGN_STORE_OVERFLOW and torch.equal(out["lidar_poses"], noisy)


@functools.lru_cache(maxsize=1)
def _dair_scene():
    """The two-agent DAIR-geometry scene (vehicle + road-side unit facing back) with planted stage-1 detections and a calibrated fusion model."""
    h1, pp1, anchors1, a1 = _stage1()
    hd = builtin_config("dairv2x_coalign")
    frame = make_frame(hd, 2, pillars_per_agent=7000, seed=5, infra_agent=True)
    rs = np.random.RandomState(42)
    clean = [np.zeros(6), np.array([30.0, 5.0, 0.0, 0.0, 170.0, 0.0])]
    views, heads = _scene_views(clean, rs, hd["preprocess"]["cav_lidar_range"], plant_on=anchors1)
    model = build_model(hd)
    fill_parameters_(model, seed=1)
    model = model.to(DEV).eval()
    pp = build_postprocessor(hd["postprocess"], False)
    fd = to_device(frame, DEV)
    calibrate_heads_(model, fd, pp.params["target_args"]["score_threshold"], 400)
    gx, gy = [int(v) for v in hd["model"]["args"]["point_pillar_scatter"]["grid_size"]][:2]
    return dict(h1=h1, pp1=pp1, anchors1=anchors1, a1=a1, hd=hd, fd=fd, clean=clean, views=views, heads=heads, model=model, pp=pp,
                anchors=torch.from_numpy(pp.generate_anchor_box()), H=gy, W=gx, ratio=float(hd["model"]["args"]["voxel_size"][0]))


FLAGS = dict(use_uncertainty=True, landmark_SE2=True, adaptive_landmark=False, normalize_uncertainty=False, abandon_hard_cases=True, drop_hard_boxes=True)


def test_chain_in_one_captured_graph():
    """Item 10: head maps -> ``post_process_stage1_device`` -> ``correct`` -> fusion model forward captured in ONE ``torch.cuda.graph`` on one stream (after a
    warm-up call that allocates); three replays with other head maps and noisy poses give ``normalized_affine_matrix``, corrected poses and ``cls_preds``
    bit-equal to the eager chain on the same inputs.  A synchronisation or an allocation of the chain inside the capture fails it."""
    S = _dair_scene()
    model, pp1, a1, fd = S["model"], S["pp1"], S["a1"], S["fd"]
    corrector = box_align.PoseCorrector(FLAGS, 5, S["H"], S["W"], S["ratio"], device=DEV)
    inputs = []
    for k, sigma in enumerate((0.2, 0.4, 0.6)):
        rs = np.random.RandomState(100 + k)
        views = [v[rs.permutation(len(v))[: len(v) - 2 * k]] for v in S["views"]]      # other detections per replay
        noisy = np.array([p + generate_noise(sigma, sigma, rng=rs) for p in S["clean"]])
        inputs.append((_heads(views, S["anchors1"], rs), torch.from_numpy(noisy).to(DEV)))
    static_heads = {k: v.clone() for k, v in inputs[0][0].items()}
    static_poses = inputs[0][1].clone()
    lidar = {k: v for k, v in fd["processed_lidar"].items()}

    def body():
        store = pp1.post_process_stage1_device(static_heads, a1, corrector.store)
        fixed = corrector.correct(store, static_poses)
        out = model({"processed_lidar": lidar, "record_len": [2], "pairwise_t_matrix": fixed["pairwise_t_matrix"],
                     "normalized_affine_matrix": fixed["normalized_affine_matrix"]})
        return fixed, out

    def load(i):
        for k in static_heads:
            static_heads[k].copy_(inputs[i][0][k])
        static_poses.copy_(inputs[i][1])

    stream = torch.cuda.Stream(device=DEV)
    with torch.no_grad(), torch.cuda.stream(stream):
        eager = []
        for i in range(3):                                                             # eager chain (the first call is the warm-up that allocates)
            load(i)
            fixed, out = body()
            eager.append((fixed["normalized_affine_matrix"].clone(), fixed["lidar_poses"].clone(), out["cls_preds"].clone(), int(fixed["status"][0])))
        assert all(e[3] == ops.ALIGN_SOLVED for e in eager) and not torch.equal(eager[0][0], eager[1][0])
        stream.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            fixed, out = body()
        for i in (1, 2, 0):
            load(i)
            graph.replay()
            stream.synchronize()
            assert torch.equal(fixed["normalized_affine_matrix"], eager[i][0]), i
            assert torch.equal(fixed["lidar_poses"], eager[i][1]), i
            assert torch.equal(out["cls_preds"], eager[i][2]), i
            assert int(fixed["status"][0]) == ops.ALIGN_SOLVED
    torch.cuda.synchronize()


def _relative_error(poses, clean):
    T, Tc = get_pairwise_transformation(poses, 2)[1, 0], get_pairwise_transformation(clean, 2)[1, 0]
    dyaw = np.degrees(np.arctan2(T[1, 0], T[0, 0]) - np.arctan2(Tc[1, 0], Tc[0, 0]))
    return float(np.hypot(*(T[:2, 3] - Tc[:2, 3]))), float(abs((dyaw + 180) % 360 - 180))


def test_aligned_inference_end_to_end_against_the_host_chain():
    """Item 11: the DAIR-geometry scene with planted detections, pose noise sigma in {0, 0.2, 0.4, 0.6}: ``inference_intermediate_fusion_aligned`` against the host
    chain (``post_process_stage1`` -> ``box_alignment_relative_sample_np`` -> ``get_pairwise_transformation`` -> model -> ``post_process``).  Corrected poses
    are held to item 7's bound where item 7 applies, i.e. on the order-robust samples (sigma 0.2 / 0.4 / 0.6: 5e-10 m / 7e-10 deg measured).  The sigma 0 sample
    is NOT order-robust by criterion (a) -- two views of one object under (almost) the same pose: the float32 radicand cancels to rounding noise, the very case
    coalign_amd/box_align.py:108-111 describes -- and there the device's explicit order and the host's BLAS order cluster one pair differently (measured:
    4.4e-4 m / 1.1e-3 deg between the two optima, both within 1 cm / 0.013 deg of the clean pose); its relative pose error and its detections are still
    asserted, the detections against the model run on the device's poses through the host's matrix functions."""
    from coalign_amd.inference import inference_intermediate_fusion_aligned
    S = _dair_scene()
    model, pp, pp1, a1, fd, clean = S["model"], S["pp"], S["pp1"], S["a1"], S["fd"], S["clean"]
    heads = S["heads"]
    meta = {"transformation_matrix": torch.eye(4), "anchor_box": S["anchors"]}
    cd, _, ud = pp1.post_process_stage1(heads, a1)
    corners = [c.cpu().numpy().astype(np.float64) for c in cd]
    unc = [u.cpu().numpy().astype(np.float64) for u in ud]
    assert min(len(c) for c in corners) >= 20
    runs = []
    for s in (0.0, 0.2, 0.4, 0.6):
        g = np.random.RandomState(1000 + int(10 * s))
        noisy = np.array([p + generate_noise(s, s, rng=g) for p in clean])
        robust = order_robust(corners, noisy, unc, **FLAGS)                           # decided on the CPU from the host functions
        print(f"sigma {s}: order-robust (a, b, c) = {robust}")
        ref = box_align.box_alignment_relative_sample_np(corners, noisy.copy(), uncertainty_list=unc, **FLAGS)
        fixed = noisy.copy()
        fixed[:, [0, 1, 4]] = ref
        e_noisy, e_fixed = _relative_error(noisy, clean), _relative_error(fixed, clean)
        runs.append((s, noisy, fixed, torch.from_numpy(get_pairwise_transformation(fixed, 5)[None]).to(DEV), e_noisy, all(robust)))
    # a common bias shift that keeps every logit of every run away from the threshold's logit (a 1e-6 difference must not flip a candidate)
    lt = math.log(0.2 / 0.8)
    with torch.no_grad():
        logits = [model(dict(fd, pairwise_t_matrix=pw))["cls_preds"].double().flatten() for *_, pw, _, _ in runs]
        for shift in np.arange(0.0, 0.05, 0.0005):
            if all(float((l + shift - lt).abs().min()) > 2e-4 for l in logits):
                break
        else:
            raise AssertionError("no bias shift clears the threshold for all four runs")
        model.cls_head.bias += float(shift)
    try:
        corrector = box_align.PoseCorrector(FLAGS, 5, S["H"], S["W"], S["ratio"], device=DEV)
        for s, noisy, fixed, pw, e_noisy, robust in runs:
            batch = {"ego": dict(fd, lidar_poses=torch.from_numpy(noisy), anchor_box_stage1=a1, **meta)}
            res = inference_intermediate_fusion_aligned(batch, model, pp, stage1_model=lambda data: heads, stage1_post_processor=pp1, corrector=corrector)
            poses = res["lidar_poses_corrected"].cpu().numpy()
            assert int(res["align_status"][0]) == ops.ALIGN_SOLVED, s
            e_xy, e_yaw = float(np.abs(poses[:, :2] - fixed[:, :2]).max()), float(np.abs((poses[:, 4] - fixed[:, 4] + 180) % 360 - 180).max())
            e_fixed = _relative_error(poses, clean)
            print(f"sigma {s}: device against host poses {e_xy:.2e} m {e_yaw:.2e} deg; relative pose error noisy {e_noisy[0]:.3f} m / {e_noisy[1]:.3f} deg -> "
                  f"aligned {e_fixed[0]:.3f} m / {e_fixed[1]:.3f} deg")
            if robust:
                assert e_xy <= 1e-5 and e_yaw <= 1e-4, (s, e_xy, e_yaw)
            else:       # the host's float32 clustering of this sample depends on its BLAS's summation order: its graph is not THE graph; the detections below are
                pw = torch.from_numpy(get_pairwise_transformation(poses, 5)[None]).to(DEV)      # compared on the device's poses through the host's matrices
            with torch.no_grad():
                ref_boxes, ref_scores = pp.post_process({"ego": meta}, {"ego": model(dict(fd, pairwise_t_matrix=pw))})
            if s > 0:
                assert e_fixed[0] < 0.5 * e_noisy[0] + 0.02 and e_fixed[1] < 0.5 * e_noisy[1] + 0.02, (s, e_noisy, e_fixed)
            assert e_fixed[0] < 0.08 and e_fixed[1] < 0.08, (s, e_fixed)
            assert res["pred_box_tensor"].shape == ref_boxes.shape and ref_boxes.shape[0] > 30, (s, res["pred_box_tensor"].shape, ref_boxes.shape)
            assert_elementwise(res["pred_box_tensor"], ref_boxes, f"sigma {s} boxes")
            assert_elementwise(res["pred_score"], ref_scores, f"sigma {s} scores")
    finally:
        with torch.no_grad():
            model.cls_head.bias -= float(shift)
