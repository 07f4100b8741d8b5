"""CPU tests of the host side: argument checks of the C ABI before any HIP call (its headers, tables and exports: tests/test_abi_cpu.py), ops refuse CPU tensors
(no fallback), pose algebra / config / anchors / plugin names match the reference-generated golden vectors."""
import os
import sys

import numpy as np
import pytest
import torch

from coalign_amd import hip, ops
from coalign_amd.config import builtin_config, load_yaml
from coalign_amd.detector import MODEL_REGISTRY, build_model
from coalign_amd import pose
from coalign_amd.postprocess import build_postprocessor

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = torch.from_numpy


def test_argument_validation_without_a_gpu():
    """Shape / pointer checks happen before any HIP call, so they can be exercised on a CPU-only machine."""
    import ctypes
    lib = hip.lib()
    null = ctypes.c_void_p(0)
    assert lib.coalign_warp_fuse(null, 2, 64, 8, 8, null, (ctypes.c_int32 * 1)(2), 1, 0, null, 8, 8, null) == -1   # NULL pointers
    assert lib.coalign_warp_fuse(null, 2, -1, 8, 8, null, (ctypes.c_int32 * 1)(2), 1, 0, null, 8, 8, null) == -2    # bad shape
    assert lib.coalign_warp_fuse(null, 2, 64, 8, 8, null, (ctypes.c_int32 * 1)(2), 1, 7, null, 8, 8, null) == -3    # unknown mode
    assert lib.coalign_nms_rotated(null, 8, 3, null, null, 5, null, 0.15, 5000, null, null, null, 0, null) == -3     # top > 4096
    assert lib.coalign_pillar_scatter_workspace_bytes(5, 200, 704) >= 5 * 200 * 704 * 4
    assert lib.coalign_nms_rotated_workspace_bytes(1000, 1000) >= 1000 * 16 * 8
    # round 5's entry points: the frame-record pillar launch, the SplitMap convolution, the up-sampling heads' SplitMap epilogue
    d3 = (ctypes.c_double * 3)(0.4, 0.4, 4.0)
    one = ctypes.c_void_p(16)                                # (a non-NULL, 16-byte aligned token: none of these calls gets as far as touching memory)
    assert lib.coalign_pillar_encode_sparse_frame(null, 100, 32, one, 64, 1, d3, d3, 2, 200, 704, one, one, one, null) == -1          # no frame record
    assert lib.coalign_pillar_encode_sparse_frame(one, 100, 33, one, 64, 1, d3, d3, 2, 200, 704, one, one, one, null) == -2           # P > 32
    assert lib.coalign_pillar_encode_sparse_frame(ctypes.c_void_p(20), 100, 32, one, 64, 1, d3, d3, 2, 200, 704, one, one, one, null) == -2      # record not 8-byte aligned
    assert lib.coalign_conv3x3_sp(null, one, one, null, 0, one, 1, 1, 64, 64, 8, 8, 1, 0, null, null, 0, null) == -1                    # no input map
    assert lib.coalign_conv3x3_sp(one, one, one, null, 0, one, 1, 1, 24, 64, 8, 8, 1, 0, null, null, 0, null) == -3                     # Cin % 16: unsupported
    assert lib.coalign_conv3x3_sp(one, one, one, null, 0, one, 3, 1, 64, 64, 8, 8, 1, 0, null, null, 0, null) == -3                     # unknown output kind
    assert lib.coalign_conv3x3_sp(one, one, one, null, 0, one, 1, 1, 64, 1088, 8, 8, 1, 0, null, null, 0, null) == -3                   # Cout > 1024: its bias / scale words exceed the LDS
    assert lib.coalign_conv3x3_sp(one, one, one, null, 0, one, 1, 0, 64, 1024, 8, 8, 1, 0, null, null, 0, null) == 0                    # Cout 1024, no images: nothing to do
    assert lib.coalign_sp_map_bytes(5, 256, 25, 88) == 5 * 256 * 25 * 88 * 4 and lib.coalign_sp_map_bytes(5, 24, 25, 88) == 0
    assert lib.coalign_pointwise_conv_emu_sp(one, one, one, one, 1, 64, 8, 8, 1, 120, 1, 128, 384, 0, 1, 1, null, null) == -3          # Cout % 16
    assert lib.coalign_pointwise_conv_emu_sp(one, one, one, one, 1, 64, 8, 8, 1, 128, 1, 128, 384, 8, 1, 1, null, null) == -3          # c_off % 16
    assert lib.coalign_pointwise_conv_emu_sp(one, one, one, one, 1, 64, 8, 8, 1, 128, 2, 128, 384, 0, 1, 1, null, null) == -2          # M_padded != Cout * up * up
    # round 6's entry points: the strided SplitMap convolution (dense / sparse canvas), the sp16 row packer, the two-output form of the stride-1 kernel
    assert lib.coalign_conv3x3_sp_s2(null, one, one, one, 1, 64, 64, 8, 8, 1, null, null) == -1                                         # no input map
    assert lib.coalign_conv3x3_sp_s2(one, one, one, one, 1, 24, 64, 8, 8, 1, null, null) == -3                                          # Cin % 16
    assert lib.coalign_conv3x3_sp_s2(one, one, one, one, 1, 64, 96, 8, 8, 1, null, null) == -3                                          # Cout % 64
    assert lib.coalign_conv3x3_sp_s2(one, one, one, one, 1, 64, 64, 0, 8, 1, null, null) == -2                                          # empty map
    assert lib.coalign_conv3x3_sp_s2(one, one, one, one, 0, 64, 64, 8, 8, 1, null, null) == 0                                           # no images: nothing to do
    assert lib.coalign_conv3x3_sp_s2_sparse(one, 10, null, one, one, one, one, 1, 64, 64, 8, 8, 1, null, null) == -1                    # no stamps
    assert lib.coalign_conv3x3_sp_s2_sparse(one, -1, one, one, one, one, one, 1, 64, 64, 8, 8, 1, null, null) == -2                     # negative row count
    assert lib.coalign_conv3x3_sp_s2_sparse(one, 10, one, one, one, one, one, 1, 16, 64, 8, 8, 1, null, null) == -3                     # Cin < 32 on the sparse route
    assert lib.coalign_conv3x3_sp_s2_sparse(one, 10, ctypes.c_void_p(20), one, one, one, one, 1, 64, 64, 8, 8, 1, null, null) == -3     # stamps not 8-byte aligned
    assert lib.coalign_sp_pack_rows(null, 10, null, 64, one, null, null) == -1 and lib.coalign_sp_pack_rows(one, 10, null, 24, one, null, null) == -3
    assert lib.coalign_sp_pack_rows(one, 0, null, 64, one, null, null) == 0 and lib.coalign_sp_rows_bytes(100, 64) == 100 * 64 * 4 and lib.coalign_sp_rows_bytes(100, 24) == 0
    assert lib.coalign_conv3x3_sp_both(one, one, one, null, 0, one, null, 1, 64, 64, 8, 8, 1, 0, null, null, 0, null) == -1            # no SplitMap output
    assert lib.coalign_conv3x3_sp_s2_skip(one, one, one, null, one, one, 1, 64, 64, 8, 8, 1, null, null) == -1                          # no skip weights
    assert lib.coalign_conv3x3_sp_s2_skip(one, one, one, one, one, one, 1, 64, 576, 8, 8, 1, null, null) == -3                         # Cout > 512 on the fused form
    assert lib.coalign_conv3x3_sp_s2_skip_sparse(one, 10, one, one, one, one, one, one, null, 1, 64, 64, 8, 8, 1, null, null) == -1     # no skip map
    assert lib.coalign_conv1x1_sp_weight_bytes(64, 128) == 128 * 64 * 4 + 16 + 128 * 8 and lib.coalign_conv1x1_sp_weight_bytes(24, 128) == 0
    assert lib.coalign_heads_sp(null, one, one, one, 1, 256, 20, 8, 8, null) == -1 and lib.coalign_heads_sp(one, one, one, one, 1, 256, 40, 8, 8, null) == -3      # no map; more than 32 head channels
    assert lib.coalign_heads_sp(one, one, one, one, 1, 250, 20, 8, 8, null) == -3 and lib.coalign_heads_sp(one, one, one, one, 0, 256, 20, 8, 8, null) == 0
    assert lib.coalign_conv3x3_sp_both(one, one, one, null, 0, one, ctypes.c_void_p(24), 1, 64, 64, 8, 8, 1, 0, null, null, 0, null) == -3      # ... not 16-byte aligned
    # the fusion entry points' refusals that fusion.py's routes rely on (group / row / per-scale arguments are host arrays the entry points read)
    i32 = lambda *v: (ctypes.c_int32 * len(v))(*v)                                                                    # noqa: E731
    fuse_rows = lambda n, C, groups, rows: lib.coalign_warp_fuse_rows(one, n, C, 8, 8, one, groups, len(groups), rows, 0, one, 8, 8, null)  # noqa: E731
    assert fuse_rows(4, 257, i32(4), None) == -3                                 # C > 256
    assert fuse_rows(9, 64, i32(9), None) == -3                                  # a frame of 9 agents
    assert fuse_rows(7, 64, i32(4, 2), None) == -2                               # group_len does not sum to n_total
    assert fuse_rows(6, 64, i32(4, 2), i32(0, 2, 2, 1, 1, 0)) == -2              # a row repeated inside the first frame
    assert fuse_rows(6, 64, i32(4, 2), i32(3, 0, 2, 1, 2, 0)) == -2              # a row outside its frame
    vp = lambda k: (ctypes.c_void_p * k)(*([16] * k))                                                               # noqa: E731
    fuse_nhwc = lambda k, C, n: lib.coalign_warp_fuse_nhwc(k, vp(k), i32(*[C] * k), i32(*[8] * k), i32(*[8] * k), vp(k), i32(*[8] * k),  # noqa: E731
                                                           i32(*[8] * k), n, one, None, 0, null)
    assert fuse_nhwc(1, 96, 4) == -3                                             # C not in {64, 128, 256}
    assert fuse_nhwc(1, 64, 9) == -3                                             # 9 agents
    assert fuse_nhwc(4, 64, 4) == -2                                             # 4 scales
    from coalign_amd import fusion
    aff = torch.zeros(1, 4, 4, 2, 3, dtype=torch.float64)
    assert fusion.fuse_multiscale([torch.zeros(4, 96, 8, 8).contiguous(memory_format=torch.channels_last)], [4], aff, ops.FUSE_ATT) is None    # no channels-last device map: the caller falls back
    assert fusion.fuse_multiscale([torch.zeros(4, 64, 8, 8)], [4], aff, ops.FUSE_MAX) is None


def test_ops_have_no_cpu_fallback():
    with pytest.raises(hip.CoalignHipError):
        ops.warp_fuse(torch.zeros(1, 4, 8, 8), torch.zeros(1, 2, 3, dtype=torch.float64), [1], ops.FUSE_ATT)
    with pytest.raises(hip.CoalignHipError):
        ops.scatter_to_bev(torch.zeros(3, 64), torch.zeros(3, 4, dtype=torch.int32), 1, 8, 8)
    model = build_model(builtin_config("mini_coalign")).eval()
    from coalign_amd.synthetic import make_frame
    with pytest.raises(hip.CoalignHipError):
        model(make_frame(builtin_config("mini_coalign"), 2, pillars_per_agent=10))


def test_pose_algebra_matches_reference(golden):
    g = golden("pose.npz")
    for p, w in zip(g["poses"], g["x_to_world"]):
        np.testing.assert_allclose(pose.x_to_world(p), w, rtol=0, atol=1e-15)
    np.testing.assert_allclose(pose.get_pairwise_transformation(g["poses"], 5), g["pairwise"], rtol=0, atol=1e-13)
    pt = T(g["pairwise"])[None]
    before = pt.clone()
    np.testing.assert_allclose(pose.normalize_pairwise_tfm(pt, 200, 704, 0.4).numpy(), g["normalized_200x704"], rtol=0, atol=1e-15)
    np.testing.assert_allclose(pose.normalize_pairwise_tfm(pt, 32, 64, 0.4).numpy(), g["normalized_32x64"], rtol=0, atol=1e-15)
    assert torch.equal(pt, before) and pose.normalize_pairwise_tfm(pt, 32, 64, 0.4).dtype == torch.float64
    assert np.array_equal(pose.get_pairwise_transformation(g["poses"], 5, proj_first=True), np.tile(np.eye(4), (5, 5, 1, 1)))
    # the host-side form FramePipeline stages with its frame record (numpy, written into a pinned view): the torch route's bits, golden included, batch > 1 too
    for H, W, key in ((200, 704, "normalized_200x704"), (32, 64, "normalized_32x64")):
        assert np.array_equal(pose.normalize_pairwise_np(g["pairwise"][None], H, W, 0.4), pose.normalize_pairwise_tfm(pt, H, W, 0.4).numpy())
        np.testing.assert_allclose(pose.normalize_pairwise_np(g["pairwise"][None], H, W, 0.4), g[key], rtol=0, atol=1e-15)
    rq = np.random.RandomState(5)
    many = np.stack([pose.get_pairwise_transformation([[rq.randn() * 40, rq.randn() * 15, rq.randn(), rq.randn() * 3, rq.randn() * 90, rq.randn() * 3] for _ in range(4)], 5) for _ in range(3)])
    out = np.full(many.shape[:-2] + (2, 3), np.nan)
    assert pose.normalize_pairwise_np(many, 100, 252, 0.4, out=out) is out and np.array_equal(out, pose.normalize_pairwise_tfm(T(many), 100, 252, 0.4).numpy())
    rs = np.random.RandomState(303)
    n = pose.generate_noise(0.2, 0.2, rng=rs)
    rs2 = np.random.RandomState(303)
    xy, yaw = rs2.normal(0, 0.2, size=2), rs2.normal(0, 0.2, size=1)
    assert np.array_equal(n, np.array([xy[0], xy[1], 0, 0, yaw[0], 0]))


def test_anchors_and_derived_config_match_reference(golden):
    import hashlib
    g = golden("anchors.npz")
    for tag, cfg in (("opv2v_coalign", "opv2v_coalign"), ("opv2v_late", "opv2v_pointpillar_late"),
                     ("dairv2x_coalign", "dairv2x_coalign"), ("mini", "mini_coalign")):
        h = builtin_config(cfg)
        a = build_postprocessor(h["postprocess"], False).generate_anchor_box()
        assert hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest() == g[tag + "_sha256"].tobytes()
        assert np.array_equal(np.asarray(h["model"]["args"]["point_pillar_scatter"]["grid_size"]), g[tag + "_grid_size"])
        assert [h["postprocess"]["anchor_args"][k] for k in "WHD"] == list(g[tag + "_WHD"])


def test_unchanged_reference_yamls_load_and_build(tmp_path):
    """Three of the reference's hypes yamls as load_yaml read them (tests/golden/reference_yamls.json, tests/golden/make_reference_yamls.py) against the shipped configs."""
    import json
    p = tmp_path / "optimizer.yaml"
    p.write_text("optimizer:\n  core_method: Adam\n  lr: 0.002\n  args:\n    eps: 1e-10\n    weight_decay: 1e-4\n")
    eps = load_yaml(str(p))["optimizer"]["args"]["eps"]
    assert isinstance(eps, float) and eps == 1e-10                          # float resolver fix ("1e-10" parses as float)
    golden = json.load(open(os.path.join(REPO, "tests", "golden", "reference_yamls.json")))
    for rel, cfg in (("opv2v/lidar_only_with_noise/coalign/pointpillar_coalign.yaml", "opv2v_coalign"),
                     ("opv2v/lidar_only_with_noise/pointpillar_single.yaml", "opv2v_pointpillar_late"),
                     ("dairv2x/lidar_only_with_noise/coalign/pointpillar_coalign.yaml", "dairv2x_coalign")):
        ref, mine = golden[rel], builtin_config(cfg)
        ref["model"]["args"]["point_pillar_scatter"]["grid_size"] = np.asarray(ref["model"]["args"]["point_pillar_scatter"]["grid_size"], dtype=np.int64)
        assert ref["optimizer_eps"] == 1e-10
        assert ref["model"]["core_method"] == mine["model"]["core_method"]
        ra, ma = ref["model"]["args"], mine["model"]["args"]
        for k in ("voxel_size", "lidar_range", "anchor_number", "pillar_vfe", "base_bev_backbone", "shrink_header", "dir_args"):
            assert ra[k] == ma[k], (cfg, k)
        assert np.array_equal(ra["point_pillar_scatter"]["grid_size"], ma["point_pillar_scatter"]["grid_size"])
        rp, mp = ref["postprocess"], mine["postprocess"]
        for k in ("anchor_args", "target_args", "order", "nms_thresh", "gt_range", "dir_args"):
            assert rp[k] == mp[k], (cfg, k)
        build_model(ref)                                                     # the unchanged yaml drives the plugin classes


def test_kernel_routes_of_every_config():
    """coalign_amd.routes.plan: (a) the configs behind the five BASELINE workloads leave NO 3x3 / skip / head layer on a library fallback, run
    the one-launch channels-last fusion and the matrix-core pillar encoder; a config built to fall off the fast path (Cout % 64 != 0,
    distance feature, 96-channel scale) is reported, not silent.  (b) the committed walk over the reference's hypes_yaml/**/pointpillar*.yaml
    (tests/golden/yaml_routes.json: 15 yamls of the hot-path families, 22 of other families) is reproduced when the checkout is present."""
    import copy
    import glob
    import json
    from coalign_amd.routes import plan, summary
    for cfg in ("opv2v_coalign", "dairv2x_coalign", "opv2v_pointpillar_late", "opv2v_pointpillar_uncertainty", "lss_coalign_fusion"):
        h = builtin_config(cfg)
        if "core_method" not in h.get("model", {}) or h["model"]["core_method"] not in ("point_pillar_baseline_multiscale", "point_pillar_coalign", "point_pillar", "point_pillar_uncertainty"):
            continue                                   # cfg 5 ships only its fusion step
        p = plan(h)
        assert p["outside_hot_path"] is None and p["fallbacks"] == [], (cfg, p["fallbacks"])
        assert p["pillar"].startswith("matrix-core"), cfg
        assert all(not r.startswith("MIOpen") for r in p["layers"].values()), cfg
        if p["fusion"] is not None:
            assert p["fusion"].startswith("warp_fuse_nhwc"), cfg
    odd = copy.deepcopy(builtin_config("opv2v_coalign"))
    odd["model"]["args"]["base_bev_backbone"]["num_filters"] = [64, 96, 256]
    odd["model"]["args"]["att"]["feat_dim"] = [64, 96, 256]
    odd["model"]["args"]["pillar_vfe"]["with_distance"] = True
    p = plan(odd)
    assert "fusion" in p["fallbacks"] and any("layer1" in n for n in p["fallbacks"]) and p["pillar"].startswith("fp32 VALU")
    table = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "yaml_routes.json")))
    hot = {k: v for k, v in table.items() if not v.get("outside_hot_path")}
    assert len(table) == 37 and len(hot) == 15 and all(v["fallbacks"] == [] for v in hot.values())
    base = "/root/reference/opencood/hypes_yaml/"
    if os.path.isdir(base):
        for path in sorted(glob.glob(base + "**/pointpillar*.yaml", recursive=True)):
            try:
                got = summary(plan(load_yaml(path)))
            except Exception as e:      # noqa: BLE001
                got = {"outside_hot_path": f"{type(e).__name__}: {str(e)[:120]}"}
            assert got == table[path[len(base):]], path


def test_state_dict_names_match_reference(golden):
    for cfg, gname in (("mini_coalign", "model_mini.npz"), ("mini_pointpillar_late", "late_mini.npz")):
        g = golden(gname)
        sd = build_model(builtin_config(cfg)).state_dict()
        assert list(sd.keys()) == [str(k) for k in g["state_keys"]]
        assert [v.numel() for v in sd.values()] == list(g["state_numel"])
    full = build_model(builtin_config("opv2v_coalign"))
    assert sum(p.numel() for p in full.parameters()) == 12901524            # SURVEY §2a [probe]


def test_opencood_alias_install_resolves_plugin_names():
    if os.path.isdir("/root/reference") and "/root/reference" in sys.path:
        pytest.skip("a real opencood checkout is on sys.path in this process")
    from coalign_amd import opencood_compat
    report = opencood_compat.install()
    assert set(report.values()) <= {"synthetic", "patched"}
    import importlib
    for core_method in ("point_pillar_baseline_multiscale", "point_pillar_coalign", "point_pillar"):
        lib = importlib.import_module("opencood.models." + core_method)
        target = core_method.replace("_", "").lower()
        hits = [c for n, c in lib.__dict__.items() if n.lower() == target or (core_method == "point_pillar_coalign" and n == "CoAlign")]
        assert hits and hits[0] is MODEL_REGISTRY[core_method]
    from opencood.models.fuse_modules.fusion_in_one import AttFusion, MaxFusion, regroup  # noqa: F401
    from opencood.utils.box_utils import nms_rotated  # noqa: F401
    from opencood.data_utils.post_processor import build_postprocessor as bp  # noqa: F401
    from opencood.tools.train_utils import create_model
    assert create_model(builtin_config("mini_coalign")).__class__.__name__ == "PointPillarBaselineMultiscale"


def test_delta_to_boxes3d_matches_reference(golden):
    from coalign_amd.postprocess import VoxelPostprocessor
    g = golden("postprocess.npz")
    out = VoxelPostprocessor.delta_to_boxes3d(T(g["i_reg"]), T(g["anchors"]))
    np.testing.assert_allclose(out.numpy(), g["i_delta_boxes"], rtol=1e-6, atol=1e-6)


def test_synthetic_frame_contract():
    from coalign_amd.synthetic import make_frame
    h = builtin_config("opv2v_coalign")
    f = make_frame(h, [2, 3], pillars_per_agent=500, seed=1)
    pl = f["processed_lidar"]
    assert pl["voxel_features"].shape == (2500, 32, 4) and pl["voxel_features"].dtype == torch.float32
    assert pl["voxel_coords"].dtype == torch.int32 and pl["voxel_num_points"].dtype == torch.int32
    assert f["pairwise_t_matrix"].shape == (2, 5, 5, 4, 4) and f["pairwise_t_matrix"].dtype == torch.float64
    c = pl["voxel_coords"].long()
    key = (c[:, 0] * 200 + c[:, 2]) * 704 + c[:, 3]
    assert key.unique().numel() == 2500                                      # distinct cells per agent
    pad = torch.arange(32)[None, :] >= pl["voxel_num_points"][:, None]
    assert float(pl["voxel_features"][pad].abs().sum()) == 0.0               # zero padded
    assert int(pl["voxel_num_points"].min()) >= 1 and int(pl["voxel_num_points"].max()) <= 32


def test_box_alignment_graph_construction_matches_reference(golden):
    """Host half of next-3 (coalign_amd/box_align.py, no GPU needed): clusters, landmarks, edges and information matrices equal
    the graph the reference hands to g2o; the hard-case rules return None where the reference returns the noisy poses."""
    import numpy as np
    from coalign_amd import box_align
    from tests.test_oracle_golden import BOX_ALIGN_CASES, box_align_inputs
    g = golden("box_align.npz")
    for tag in BOX_ALIGN_CASES:
        corners, noisy, unc, flags = box_align_inputs(g, tag)
        graph = box_align.build_pose_graph(corners, noisy, unc, **flags)
        if int(g[f"{tag}_solved"]) == 0:
            assert graph is None
            assert np.array_equal(box_align._refined(None, None, noisy), g[f"{tag}_refined"])
            continue
        graph.check()
        n = graph.n_agents
        assert np.array_equal(graph.kinds, g[f"{tag}_kinds"])
        assert np.array_equal(graph.edge_agent, g[f"{tag}_edge_agent"]) and np.array_equal(graph.edge_landmark, g[f"{tag}_edge_landmark"])
        assert np.array_equal(graph.vertices[:n], g[f"{tag}_vertices"][:n])                       # agents: exact
        np.testing.assert_allclose(graph.vertices[n:], g[f"{tag}_vertices"][n:], rtol=0, atol=1e-4)  # landmarks: float32 world frame
        np.testing.assert_allclose(graph.edge_meas, g[f"{tag}_edge_meas"], rtol=0, atol=1e-12)
        np.testing.assert_allclose(graph.edge_info, g[f"{tag}_edge_info"], rtol=1e-12, atol=0)


def dataset_scenario(g, tag):
    """Rebuild the in-memory scenario of tests/golden/dataset.npz (see make_golden.py: memory_scenario)."""
    from collections import OrderedDict
    sc = OrderedDict()
    for c, cid in enumerate(g[f"{tag}_cav_ids"]):
        veh = OrderedDict()
        for vid, row in zip(g[f"{tag}_veh_ids{c}"], g[f"{tag}_veh{c}"]):
            veh[int(vid)] = {"location": row[0:3].tolist(), "angle": row[3:6].tolist(), "extent": row[6:9].tolist(), "center": row[9:12].tolist()}
        sc[str(cid)] = {"ego": c == 0, "params": {"lidar_pose": g[f"{tag}_pose{c}"].tolist(), "vehicles": veh}, "lidar_np": g[f"{tag}_lidar{c}"]}
    return sc


def check_batch_against_reference(batch, g, tag, exact_voxels=True, xyz_atol=0.0):
    """``xyz_atol`` > 0: the clouds were projected on the host before voxelisation (proj_first), so x, y, z of the pillars' points are float32 4-term matrix products
    whose rounding follows the host's BLAS kernel (MKL's AVX-512, AVX2 and SSE4.2 kernels differ by up to 1.5e-5 on this golden); they are held to ``xyz_atol``,
    everything else stays bit-exact."""
    import numpy as np
    ego = batch["ego"]
    assert [str(c) for c in ego["cav_id_list"]] == [str(c) for c in g[f"{tag}_cav_id_list"]]
    assert ego["record_len"].tolist() == g[f"{tag}_record_len"].tolist()
    np.testing.assert_allclose(ego["lidar_pose"].numpy(), g[f"{tag}_lidar_pose"], rtol=0, atol=1e-12)
    np.testing.assert_allclose(ego["lidar_pose_clean"].numpy(), g[f"{tag}_lidar_pose_clean"], rtol=0, atol=0)
    np.testing.assert_allclose(ego["pairwise_t_matrix"].numpy(), g[f"{tag}_pairwise_t_matrix"], rtol=0, atol=1e-9)
    assert [int(i) for i in ego["object_ids"]] == g[f"{tag}_object_ids"].tolist()
    assert np.array_equal(ego["object_bbx_mask"].numpy(), g[f"{tag}_object_bbx_mask"])
    np.testing.assert_allclose(ego["object_bbx_center"].numpy(), g[f"{tag}_object_bbx_center"], rtol=0, atol=1e-9)
    assert np.array_equal(ego["transformation_matrix"].numpy(), g[f"{tag}_transformation_matrix"])
    pl = {k: v.cpu().numpy() for k, v in ego["processed_lidar"].items()}
    assert np.array_equal(pl["voxel_coords"], g[f"{tag}_voxel_coords"]) and np.array_equal(pl["voxel_num_points"], g[f"{tag}_voxel_num_points"])
    feats, want = pl["voxel_features"], g[f"{tag}_voxel_features"]
    if xyz_atol == 0.0:
        assert np.array_equal(feats, want)
    else:
        assert feats.shape == want.shape and np.array_equal(feats[..., 3:], want[..., 3:])
        np.testing.assert_allclose(feats[..., :3], want[..., :3], rtol=0, atol=xyz_atol)


def test_batch_dict_producer_matches_reference_dataset(golden):
    """next-4 on the host: IntermediateFusionBatcher (pose noise, comm-range cut, pairwise transforms, ground-truth boxes, id de-dup,
    collate) against the reference's IntermediateFusionDataset.__getitem__ + collate_batch_test run on the same in-memory scenario;
    the voxeliser is injected (oracle here, the device kernel in the GPU twin of this test)."""
    import numpy as np
    import torch
    from oracle import coalign_oracle as oracle
    from coalign_amd.config import builtin_config
    from coalign_amd.dataset import IntermediateFusionBatcher

    class OracleVoxels:
        def __init__(self, p):
            self.p = p

        def preprocess_clouds(self, clouds, ego_filter=False, filter_range=None):
            a = self.p["args"]
            per = [oracle.points_to_voxel(oracle.mask_ego_points(c) if ego_filter else c, a["voxel_size"], self.p["cav_lidar_range"],
                                          a["max_points_per_voxel"], a["max_voxel_test"]) for c in clouds]
            f, c, n = oracle.collate_voxels(per)
            return {"voxel_features": torch.from_numpy(f), "voxel_coords": torch.from_numpy(c), "voxel_num_points": torch.from_numpy(n)}

    g = golden("dataset.npz")
    h = builtin_config("opv2v_coalign")
    h.pop("box_align", None)
    batcher = IntermediateFusionBatcher(h, train=False, device="cpu", preprocessor=OracleVoxels(h["preprocess"]))
    for tag in ("a", "b"):
        np.random.seed(int(g[f"{tag}_np_seed"]))
        check_batch_against_reference(batcher(dataset_scenario(g, tag)), g, tag)
    assert len(g["a_cav_id_list"]) == 3 and int(g["a_n_cav"]) == 4          # one cav was beyond comm_range


def test_dataset_side_branches_match_reference(golden):
    """Laplace pose noise (pose_utils.py:19-21, 77-105) and proj_first = True (intermediate_fusion_dataset.py:43-44, 104: clouds projected
    into the ego frame before the voxeliser, identity pairwise matrices) against the reference's dataset class on the same scenario and numpy
    seed: poses, pairwise matrices, ground truth and -- through the injected oracle voxeliser -- the very same pillars."""
    import copy
    import numpy as np
    import torch
    from oracle import coalign_oracle as oracle
    from coalign_amd.config import builtin_config
    from coalign_amd.dataset import IntermediateFusionBatcher

    class OracleVoxels:
        def __init__(self, p):
            self.p = p

        def preprocess_clouds(self, clouds, ego_filter=False, filter_range=None):
            a = self.p["args"]
            per = [oracle.points_to_voxel(oracle.mask_ego_points(c) if ego_filter else c, a["voxel_size"], self.p["cav_lidar_range"],
                                          a["max_points_per_voxel"], a["max_voxel_test"]) for c in clouds]
            f, c, n = oracle.collate_voxels(per)
            return {"voxel_features": torch.from_numpy(f), "voxel_coords": torch.from_numpy(c), "voxel_num_points": torch.from_numpy(n)}

    g = golden("dataset_branches.npz")
    gg = {f"c_{k}": g[k] for k in g.files}
    gg["c_cav_id_list"] = g["cav_ids"]                                   # nobody out of range in this scenario
    gg["c_transformation_matrix"] = np.identity(4, dtype=np.float32)
    h = copy.deepcopy(builtin_config("opv2v_coalign"))
    h.pop("box_align", None)
    h.setdefault("fusion", {}).setdefault("args", {})["proj_first"] = True
    h["noise_setting"] = {"add_noise": True, "args": {"pos_std": 0.3, "rot_std": 0.4, "pos_mean": 0.0, "rot_mean": 0.0, "laplace": True}}
    batcher = IntermediateFusionBatcher(h, train=False, device="cpu", preprocessor=OracleVoxels(h["preprocess"]))
    np.random.seed(int(g["np_seed"]))
    batch = batcher(dataset_scenario(gg, "c"))
    # the terms each projected coordinate sums stay below 128 m here: two float32 evaluations of the 4-term sum differ by at most ~6 unit roundoffs of that
    check_batch_against_reference(batch, gg, "c", xyz_atol=6 * 2.0 ** -24 * 128)
    pw = batch["ego"]["pairwise_t_matrix"].numpy()
    assert np.array_equal(pw, np.tile(np.eye(4), pw.shape[:3] + (1, 1)))
    assert float(np.abs(g["lidar_pose"] - g["lidar_pose_clean"]).max()) > 0.01      # the noise really was drawn


def test_split_bf16_weight_image_layout_and_exactness():
    """ops.pack_conv3x3_emu_weight (entry point (9b)): the image is [Cout/64][Cin/8][5 steps][terms][2 k-groups][64][8] bf16 + 16 zero
    bytes, tap = 2 * step + k-group with a zero tenth tap; the three terms of the 3-way split add up to the fp32 weight EXACTLY, the
    two terms of the 2-way split to within 2^-16 relative."""
    from coalign_amd import hip, ops
    gen = torch.Generator().manual_seed(5)
    w = torch.randn(128, 16, 3, 3, generator=gen) * torch.logspace(-3, 3, 128).view(-1, 1, 1, 1)
    for terms in (3, 2):
        img = ops.pack_conv3x3_emu_weight(w, terms)
        assert img.dtype == torch.uint8 and img.numel() == hip.lib().coalign_conv3x3_emu_weight_bytes(16, 128, terms)
        assert int(img[-16:].sum()) == 0
        t = img[:-16].view(torch.bfloat16).reshape(2, 2, 5, terms, 2, 64, 8).double()          # [g, chunk, step, term, kgroup, cout, cin]
        total = t.sum(dim=3)                                                                    # [g, chunk, step, kgroup, cout, cin]
        taps = total.permute(0, 4, 1, 5, 2, 3).reshape(128, 16, 10)                             # [cout, cin, tap = 2 * step + kgroup]
        assert float(taps[..., 9].abs().max()) == 0.0
        want = w.reshape(128, 16, 9).double()
        if terms == 3:
            assert torch.equal(taps[..., :9], want)
        else:
            assert float(((taps[..., :9] - want).abs() / want.abs().clamp_min(1e-30)).max()) <= 2.0 ** -16
    with pytest.raises(ValueError):
        ops.pack_conv3x3_emu_weight(torch.zeros(60, 16, 3, 3), 3)
    assert hip.lib().coalign_conv3x3_emu_weight_bytes(16, 128, 4) == 0


def test_split_bf16_tap_major_weight_image_layout_and_exactness():
    """The tap-major image (COALIGN_LAYOUT_W_TAPMAJOR, the detector's stride-1 layers): [Cout/64][Cin/16][9 taps][terms][2 channel halves]
    [64][8] bf16 + 16 zero bytes -- no zero tap, so 9/10 of the tap-pair image; the 3-way terms add up to the fp32 weight exactly; Cin must be
    a multiple of 16; the size functions of the C ABI agree with the packer."""
    from coalign_amd import hip, ops
    L = hip.lib()
    gen = torch.Generator().manual_seed(6)
    w = torch.randn(128, 32, 3, 3, generator=gen) * torch.logspace(-3, 3, 128).view(-1, 1, 1, 1)
    for terms in (3, 2):
        img = ops.pack_conv3x3_emu_weight(w, terms, tap_major=True)
        assert img.dtype == torch.uint8 and img.numel() == L.coalign_conv3x3_emu_weight_bytes_ex(32, 128, terms, 1)
        assert (img.numel() - 16) * 10 == (L.coalign_conv3x3_emu_weight_bytes(32, 128, terms) - 16) * 9
        assert L.coalign_conv3x3_emu_weight_bytes_ex(32, 128, terms, 0) == L.coalign_conv3x3_emu_weight_bytes(32, 128, terms)
        assert int(img[-16:].sum()) == 0
        t = img[:-16].view(torch.bfloat16).reshape(2, 2, 9, terms, 2, 64, 8).double()          # [g, interval, tap, term, half, cout, cin]
        total = t.sum(dim=3)                                                                    # [g, interval, tap, half, cout, cin]
        got = total.permute(0, 4, 1, 3, 5, 2).reshape(128, 32, 9)                               # [cout, cin = 16 * interval + 8 * half + i, tap]
        want = w.reshape(128, 32, 9).double()
        if terms == 3:
            assert torch.equal(got, want)
        else:
            assert float(((got - want).abs() / want.abs().clamp_min(1e-30)).max()) <= 2.0 ** -16
    with pytest.raises(ValueError):
        ops.pack_conv3x3_emu_weight(torch.zeros(64, 24, 3, 3), 3, tap_major=True)              # Cin % 16
    assert L.coalign_conv3x3_emu_weight_bytes_ex(24, 64, 3, 1) == 0
    assert L.coalign_conv3x3_emu_workspace_bytes_ex(0, 64, 64, 100, 352, 3, 4) == 0             # nothing to do, no device needed


def test_pipeline_helpers_on_cpu():
    """pad_pillars (pure tensor code) and the pipeline's refusal to run without the GPU (no CPU fallback anywhere in the product)."""
    from coalign_amd.pipeline import FramePipeline, pad_pillars
    from coalign_amd.hip import CoalignHipError
    pl = {"voxel_features": torch.randn(10, 32, 4), "voxel_coords": torch.randint(0, 5, (10, 4)).int(), "voxel_num_points": torch.randint(1, 33, (10,)).int()}
    out = pad_pillars(pl, 16)
    assert out["voxel_features"].shape == (16, 32, 4) and out["voxel_coords"].shape == (16, 4) and out["voxel_num_points"].shape == (16,)
    assert torch.equal(out["voxel_features"][:10], pl["voxel_features"]) and bool((out["voxel_coords"][10:] == -1).all())
    assert float(out["voxel_features"][10:].abs().sum()) == 0.0 and bool((out["voxel_num_points"][10:] == 1).all())
    assert pad_pillars(out, 16) is out                                    # already a multiple: untouched
    h = builtin_config("mini_coalign")
    model = build_model(h).eval()
    pp = build_postprocessor(h["postprocess"], False)
    with pytest.raises(CoalignHipError):
        FramePipeline(model, pp, pp.generate_anchor_box(), lanes=2)


def test_pcdet_api_surface_and_citations():
    """Row N's host mirror exposes the four functions callers import from iou3d_nms_utils, and refuses CPU tensors."""
    from coalign_amd import pcdet
    from coalign_amd.hip import CoalignHipError
    for name in ("boxes_iou_bev", "boxes_iou3d_gpu", "nms_gpu", "nms_normal_gpu"):
        assert callable(getattr(pcdet, name))
    with pytest.raises(CoalignHipError):
        pcdet.nms_gpu(torch.zeros(3, 7), torch.zeros(3), 0.1)
    keep, none = pcdet.nms_gpu(torch.zeros(0, 7), torch.zeros(0), 0.1)       # empty input never reaches the device
    assert keep.numel() == 0 and none is None


def test_library_is_built_without_packed_fp32_instructions():
    """build.py: -fno-slp-vectorize on every source (the packed-fp32 hazard of profiles/round3/README.md); the flag must not get lost."""
    from coalign_amd import build
    assert "-fno-slp-vectorize" in build.FLAGS and "-fno-vectorize" in build.FLAGS
    assert "-ffp-contract=off" in build.FLAGS
    # the kernel the finding was made on, and the file whose encoder was written for v_pk_fma_f32 in round 2: ISA checked
    assert build.packed_fp32_count("warp_fuse_nhwc.hip") == 0
    assert build.packed_fp32_count("pillar_scatter.hip") == 0


def test_pointwise_emu_weight_image_layout():
    """ops.pack_pointwise_emu_weight against the indexing documented in include/coalign_amd.h: lane l of (row tile, step, term) holds term
    `term` of W[16 step + 8 (l // 32) + j][32 tile + l % 32]; the three terms add up to the fp32 weight exactly."""
    import torch
    from coalign_amd import ops
    g = torch.Generator().manual_seed(5)
    Cin, M = 48, 96
    w = torch.randn(Cin, M, generator=g)
    img = ops.pack_pointwise_emu_weight(w)
    assert tuple(img.shape) == (M // 32, Cin // 16, 3, 64, 8) and img.dtype == torch.int16
    h = w.to(torch.bfloat16); r1 = w - h.float(); m = r1.to(torch.bfloat16); lo = (r1 - m.float()).to(torch.bfloat16)
    assert float((h.float() + m.float() + lo.float() - w).abs().max()) == 0.0
    terms = [t.view(torch.int16) for t in (h, m, lo)]
    for tile in range(M // 32):
        for step in range(Cin // 16):
            for t in range(3):
                for lane in (0, 7, 31, 32, 45, 63):
                    k0, mm = 16 * step + 8 * (lane // 32), 32 * tile + lane % 32
                    assert img[tile, step, t, lane].tolist() == terms[t][k0: k0 + 8, mm].tolist()


def test_xcd_order_of_the_convolution_workgroups_is_a_permutation():
    """conv3x3_emu.hip: hardware workgroup b (on XCD b % 8) works as logical id k * q + min(k, r) + j (k = b % 8, j = b // 8, q = n // 8, r = n % 8): XCD k
    gets the k-th contiguous share of the ids.  Restated here: a permutation of range(n) for every grid size, shares contiguous and ordered."""
    for n in list(range(1, 70)) + [132, 192, 240, 242, 256, 462, 495, 512, 1000]:
        q, r = n // 8, n % 8
        ids = [(b % 8) * q + min(b % 8, r) + b // 8 for b in range(n)]
        assert sorted(ids) == list(range(n)), n
        for k in range(8):
            mine = [ids[b] for b in range(k, n, 8)]
            assert mine == list(range(mine[0], mine[0] + len(mine))) if mine else True
            if k and mine:
                prev = [ids[b] for b in range(k - 1, n, 8)]
                assert prev[-1] + 1 == mine[0], (n, k)


def test_product_library_reads_no_laboratory_switch():
    """ablation / debug / geometry switches live behind -DCOALIGN_LAB (coalign_amd/build.py --lab, loaded with COALIGN_LAB=1 by
    tools/ and the variant tests).  The PRODUCT library contains the names of exactly two environment variables -- the documented encoder / legacy
    selectors -- and the laboratory library contains the experiment switches."""
    import re
    from coalign_amd import build
    names = lambda path: set(re.findall(rb"COALIGN_[A-Z0-9_]+", open(path, "rb").read()))
    status = {b"COALIGN_OK", b"COALIGN_ERR_BAD_SHAPE", b"COALIGN_ERR_HIP", b"COALIGN_ERR_NULL_POINTER", b"COALIGN_ERR_UNSUPPORTED", b"COALIGN_ERR_WORKSPACE"}
    assert names(build.LIB_PATH) - status == {b"COALIGN_PILLAR_MFMA", b"COALIGN_NMS_LEGACY"}
    if not os.path.exists(build.LAB_LIB_PATH):
        build.build(lab=True)
    lab = names(build.LAB_LIB_PATH)
    assert {b"COALIGN_EMU_STACK", b"COALIGN_EMU_TAPK_ROWS", b"COALIGN_PILLAR_DEBUG", b"COALIGN_WINO_ABL", b"COALIGN_PW_PB"} <= lab


def test_load_saved_model_matches_reference(golden, tmp_path):
    """``load_saved_model`` (opencood/tools/train_utils.py:29-74; SURVEY section 2 row 16, section 8b "Weights"): which checkpoint of a training folder is chosen, the
    returned epoch, strict=False semantics and the failure cases equal what the REFERENCE'S OWN function did on the same folder layouts
    (tests/golden/checkpoint.npz, written by tests/golden/make_checkpoint_golden.py); then a real detector round trip through a ``net_epoch_bestval_at*.pth`` file."""
    from coalign_amd.detector import load_saved_model
    g = golden("checkpoint.npz")
    initial = float(g["initial"])

    class Tiny(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.marker = torch.nn.Parameter(torch.full((1,), initial))
            self.other = torch.nn.Parameter(torch.full((2,), initial))

    for name in [str(n) for n in g["layouts"]]:
        d = tmp_path / name
        d.mkdir()
        files = [str(f) for f in g[f"{name}.files"] if str(f)]
        for i, n in enumerate(files):                                 # the generator's populate(): marker 100 + i per .pth file, an unknown key, `other` missing
            if n.endswith(".pth"):
                torch.save({"marker": torch.full((1,), float(100 + i)), "not_in_the_model": torch.zeros(3)}, str(d / n))
            else:
                (d / n).write_text("x")
        m = Tiny()
        raised = str(g[f"{name}.raised"])
        if raised:
            with pytest.raises(AssertionError):
                load_saved_model(str(d), m)
            assert float(m.marker.item()) == initial
            continue
        epoch, m2 = load_saved_model(str(d), m)
        assert m2 is m
        assert epoch == int(g[f"{name}.epoch"]), name
        assert float(m.marker.item()) == float(g[f"{name}.marker"]), name
        assert float(m.other[0].item()) == float(g[f"{name}.other"]), name
    with pytest.raises(AssertionError, match=str(g["missing_folder.message"])):
        load_saved_model("/nonexistent/coalign/folder", Tiny())
    # ---- the detector itself: a checkpoint under the reference's best-validation name, loaded into a differently initialised model, through the opencood alias
    from coalign_amd.synthetic import fill_parameters_
    h = builtin_config("mini_coalign")
    src, dst = build_model(h), build_model(h)
    fill_parameters_(src, seed=5)
    fill_parameters_(dst, seed=6)
    ck = tmp_path / "trained"
    ck.mkdir()
    torch.save(src.state_dict(), str(ck / "net_epoch_bestval_at31.pth"))
    torch.save(dst.state_dict(), str(ck / "net_epoch40.pth"))        # a later plain epoch must NOT win over the best-validation file
    if not (os.path.isdir("/root/reference") and "/root/reference" in sys.path):
        from coalign_amd import opencood_compat
        opencood_compat.install()
        from opencood.tools.train_utils import load_saved_model as aliased
        assert aliased is load_saved_model
    epoch, out = load_saved_model(str(ck), dst)
    assert epoch == 31 and out is dst
    a, b = src.state_dict(), dst.state_dict()
    assert list(a) == list(b) and all(torch.equal(a[k], b[k]) for k in a)


def test_skip_weight_image_layout_and_values():
    """Round 6 (include/coalign_amd.h (9g)): ``ops.pack_conv1x1_sp_weight`` -- [Cout / 64][Cin / 16][2 terms][2 channel halves][64 cout][8 cin] fp16 sp16 pairs of the
    per-output-channel scaled weights, 16 zero bytes, [Cout] 2^-k_c, [Cout] 2^k_c: the pairs decode to the weights rounded to 22 significant bits."""
    torch.manual_seed(3)
    co, ci = 128, 48
    w = torch.randn(co, ci, 1, 1) * torch.logspace(-4, 1, co).reshape(co, 1, 1, 1)      # channel scales over five decades: the per-channel power of two matters
    w[5] = 0.0                                                                            # a dead channel
    img = ops.pack_conv1x1_sp_weight(w)
    assert img.dtype == torch.uint8 and img.numel() == hip.lib().coalign_conv1x1_sp_weight_bytes(ci, co) == co * ci * 4 + 16 + co * 8
    body = img[: co * ci * 4].view(torch.float16).reshape(co // 64, ci // 16, 2, 2, 64, 8).float()
    assert int(img[co * ci * 4: co * ci * 4 + 16].sum()) == 0
    inv = img[co * ci * 4 + 16: co * ci * 4 + 16 + co * 4].view(torch.float32)
    scale = img[co * ci * 4 + 16 + co * 4:].view(torch.float32)
    assert torch.equal(inv * scale, torch.ones(co)) and bool((torch.frexp(scale)[0] == 0.5).all())          # exact powers of two
    val = body[:, :, 0] + body[:, :, 1] / 1024.0                                          # [g, interval, half, cout, cin]
    got = val.permute(0, 3, 1, 2, 4).reshape(co, ci) * inv.reshape(co, 1)                 # channel = 16 * interval + 8 * half + cin
    ws = w.reshape(co, ci) * scale.reshape(co, 1)
    want = ((ws.contiguous().view(torch.int32) + 2) & -4).view(torch.float32) * inv.reshape(co, 1)
    assert torch.equal(got, want)
    amax = (w.reshape(co, ci).abs() * scale.reshape(co, 1)).amax(dim=1)
    live = w.reshape(co, ci).abs().amax(dim=1) > 0
    assert bool(((amax[live] >= 2.0 ** 13) & (amax[live] < 2.0 ** 14)).all())             # every channel's largest weight in [2^13, 2^14): both terms normal fp16 numbers


def test_csrc_has_one_copy_of_each_shared_piece():
    """csrc: the LDS-DMA statement, the dynamic-LDS attribute call, swap32, Geom and misaligned each exist in ONE file (common.h; Geom beside make_taps in
    warp_taps.h) -- a fix to one of them is made once.  Comments that mention a name do not count."""
    import glob
    import re
    from coalign_amd import build
    code = {}
    for path in sorted(glob.glob(os.path.join(build.CSRC, "*"))):
        if os.path.isfile(path):
            text = open(path, encoding="utf-8").read()
            code[os.path.basename(path)] = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", text, flags=re.S))
    assert set(build.SOURCES + build.LAB_ONLY_SOURCES) <= set(code)

    def files(pattern):
        return sorted(name for name, text in code.items() if re.search(pattern, text, flags=re.S))

    def count(pattern):
        return sum(len(re.findall(pattern, text)) for text in code.values())

    assert files(r"asm volatile\([^;]*global_load_lds") == ["common.h"]
    assert count(r"asm volatile\([^;]*global_load_lds") == 1
    assert files(r"hipFuncSetAttribute\(") == ["common.h"]
    assert files(r"\bvoid swap32\(") == ["common.h"]
    assert files(r"\bstruct Geom\b") == ["warp_taps.h"] and count(r"\bstruct Geom\b") == 1
    assert files(r"\bbool misaligned\(") == ["common.h"] and count(r"\b\w[\w:<>\*& ]* misaligned\([^;{)]*\)\s*\{") == 1
    assert count(r"\bmisaligned16\b") == 0


def test_conv3x3_sp_has_one_kernel_body_and_no_laboratory_issue_modes():
    """csrc/conv3x3_sp.hip: the LDS-DMA issue schedule is a constant of the tile geometry; the six measured-and-rejected issue modes, their dispatch tables
    and the host-only laboratory switches of the file are gone (DESIGN.md section 8 keeps their numbers).  The whole text counts, comments included."""
    import re
    from coalign_amd import build
    text = open(os.path.join(build.CSRC, "conv3x3_sp.hip"), encoding="utf-8").read()
    for name in ("PAIRED", "LOADERS", "loader_here", "kDefaultMode", "launch_mode"):
        assert not re.search(r"\b%s\b" % name, text), name
    for name in ("COALIGN_SP_SLOTS", "COALIGN_SP_BALANCE", "COALIGN_SP_CT32", "COALIGN_SP_FRONT"):
        assert name not in text, name
