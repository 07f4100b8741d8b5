"""The pose-robust V2VNet, host side (no GPU): the extension header include/coalign_amd_v2v_robust.h against the product library and ``hip.V2VR_SIGNATURES``,
argument validation before any HIP call, the parts of ``coalign_amd.v2v_robust`` and ``V2VNetFusion(agg_operator='weight')`` against the reference's recorded
outputs (tests/golden/v2v_robust.npz, written by tests/golden/make_v2v_robust_golden.py) and the float64 restatement of tests/v2v_robust_reference.py, the constant
intersection, the identities of ``forward_reduced`` one by one, the noise contract of ``PointPillarV2VNetRobust``, its refusals, and both walks of ``routes.plan``."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import abi_headers
from conftest import assert_elementwise
from coalign_amd import hip, ops, pose, routes, v2v_robust
from coalign_amd.config import builtin_config
from coalign_amd.detector import BASELINE_REGISTRY, MODEL_REGISTRY, PointPillarV2VNetRobust, build_model
from coalign_amd.fusion import V2VNetFusion
from coalign_amd.pose import generate_noise_torch, get_pairwise_transformation_torch, normalize_pairwise_tfm
from coalign_amd.synthetic import v2v_parameters_, v2v_robust_parameters_
from v2v_robust_cases import case, errors, hypes_for, maps_for, model_for, poses_for
from v2v_robust_reference import attention_f64, fuse_weight_f64, normalize_f64, pairwise_f64, pose_regression_f64, weighted_em_f64, intersection_f64

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NULL, ONE = ctypes.c_void_p(0), ctypes.c_void_p(16)      # (a non-NULL, 16-byte aligned token: none of these calls gets as far as touching memory)
HEADER = "coalign_amd_v2v_robust.h"
NAMES = {"coalign_v2vr_pool_act", "coalign_v2vr_score_head", "coalign_v2vr_pose_head_workspace_bytes", "coalign_v2vr_pose_head", "coalign_v2vr_pairwise",
         "coalign_v2vr_consistency", "coalign_v2vr_aggregate"}
CONFIGS = ("opv2v_pointpillar_v2vnet_robust", "mini_pointpillar_v2vnet_robust")
AFFINE = {"H": 24, "W": 40, "downsample_rate": 2, "discrete_ratio": 0.4}
# The golden comparison runs the same float32 torch operations as the reference on the same inputs; what may differ is how a convolution over n stacked maps
# and over one map order their sums: a few float32 roundings (2^-24 each) through four layers.
GOLDEN_RTOL, GOLDEN_FLOOR = 1e-5, 1e-6


def test_header_table_and_library_agree():
    """The header declares exactly ``NAMES``, the keys of ``hip.V2VR_SIGNATURES`` (types, counts and exports: tests/test_abi_cpu.py); every declaration's comment
    cites the reference lines it replaces; build.py lists the header and the source."""
    text = open(abi_headers.path(HEADER)).read()
    declared = abi_headers.declarations(HEADER)
    assert set(declared) == set(hip.V2VR_SIGNATURES) == abi_headers.names(HEADER) == NAMES
    comments = re.findall(r"/\*.*?\*/", text, flags=re.S)
    for name in declared:
        last = [c for c in comments if c in text[:text.index(name + "(")]][-1]
        assert re.search(r"(v2v_robust_module|v2v_fuse|transformation_utils)\.py:\d+-\d+", last), name
    src = open(os.path.join(REPO, "coalign_amd", "build.py")).read()
    assert '"coalign_amd_v2v_robust.h"' in src and '"v2v_robust.hip"' in src


def _pool(a=ONE, e=NULL, P=4, n=2, C=64, H=6, W=6, kind=1, out=ONE, flag=NULL):
    return hip.lib().coalign_v2vr_pool_act(a, e, P, n, C, H, W, kind, out, flag, NULL)


def _score(y=ONE, n=2, L=5, h=64, H=6, W=6, w=ONE, b=ONE, alpha=ONE, scores=ONE, weight=ONE):
    return hip.lib().coalign_v2vr_score_head(y, n, L, h, H, W, w, b, alpha, scores, weight, NULL)


def _head(y=ONE, n=2, L=5, h=64, H4=2, W4=2, p=ONE, T=ONE, corr=ONE, Tn=ONE, ws=ONE, wbytes=None):
    lib = hip.lib()
    return lib.coalign_v2vr_pose_head(y, n, L, h, H4, W4, p, p, p, p, p, p, T, corr, Tn, ws, lib.coalign_v2vr_pose_head_workspace_bytes(n, h) if wbytes is None else wbytes, NULL)


def _pairwise(poses=ONE, n=2, L=5, H=24, W=24, dx=19.2, dy=19.2, pw=ONE, af=ONE):
    return hip.lib().coalign_v2vr_pairwise(poses, n, L, H, W, dx, dy, pw, af, NULL)


def _consistency(poses=ONE, Tn=ONE, n=2, L=5, H=24, W=24, dx=19.2, dy=19.2, out=ONE, pw=ONE, af=ONE):
    return hip.lib().coalign_v2vr_consistency(poses, Tn, n, L, H, W, dx, dy, out, pw, af, NULL)


def _agg(a=ONE, e=ONE, x=ONE, n=2, R=2, C=64, H=5, W=7, theta=ONE, weight=ONE, L=5, kind=1, out=ONE, flag=NULL):
    return hip.lib().coalign_v2vr_aggregate(a, e, x, n, R, C, H, W, theta, weight, L, kind, out, flag, NULL)


def test_argument_validation_without_a_gpu():
    """NULL -1; negative counts, maps below 2 x 2, L < n, maps of 2^31 values -2; n > 8, L > 16, C = 24, hidden = 32, unaligned pointers, an unknown output kind -3;
    a short workspace -4; nothing to do is OK without a launch: all before any HIP call (token pointers, no GPU)."""
    for arg in ("a", "out"):
        assert _pool(**{arg: NULL}) == -1, arg
    for arg in ("y", "w", "b", "alpha", "scores", "weight"):
        assert _score(**{arg: NULL}) == -1, arg
    for arg in ("y", "p", "T", "corr", "Tn", "ws"):
        assert _head(**{arg: NULL}) == -1, arg
    for arg in ("poses", "pw", "af"):
        assert _pairwise(**{arg: NULL}) == -1, arg
    for arg in ("poses", "Tn", "out", "pw", "af"):
        assert _consistency(**{arg: NULL}) == -1, arg
    for arg in ("a", "e", "x", "theta", "weight", "out"):
        assert _agg(**{arg: NULL}) == -1, arg
    for bad in (dict(P=-1), dict(H=1), dict(W=1), dict(C=0), dict(e=ONE, P=5, n=2), dict(e=ONE, n=0), dict(P=64, C=1024, H=2048, W=2048)):
        assert _pool(**bad) == -2, bad
    for fn in (_score, _head, _pairwise, _consistency):
        for bad in (dict(n=0), dict(n=-1), dict(n=3, L=2), dict(L=0)):
            assert fn(**bad) == -2, (fn.__name__, bad)
        assert fn(n=9, L=9) == -3 and fn(L=17) == -3, fn.__name__
    for bad in (dict(H=1), dict(W=1), dict(h=0), dict(n=8, L=8, h=1024, H=2048, W=2048)):
        assert _score(**bad) == -2, bad
    for bad in (dict(H4=1), dict(W4=1), dict(h=-64)):
        assert _head(**bad) == -2, bad
    for bad in (dict(H=0), dict(W=0), dict(dx=0.0), dict(dy=-1.0)):
        assert _pairwise(**bad) == -2 and _consistency(**bad) == -2, bad
    for bad in (dict(n=-1), dict(R=3), dict(C=0), dict(H=0), dict(L=1), dict(L=0), dict(n=8, R=8, L=8, C=512, H=2048, W=2048)):
        assert _agg(**bad) == -2, bad
    assert _pool(C=24) == -3 and _pool(kind=2) == -3 and _score(h=32) == -3 and _score(h=1088) == -3 and _head(h=96) == -3 and _agg(n=9, L=9) == -3 and _agg(C=24) == -3
    assert _agg(kind=7) == -3 and _agg(L=17) == -3
    for fn, arg, p in ((_pool, "a", 8), (_pool, "e", 4), (_pool, "out", 20), (_pool, "flag", 2), (_score, "y", 8), (_score, "w", 4), (_score, "alpha", 2), (_score, "scores", 6),
                       (_head, "y", 8), (_head, "p", 4), (_head, "T", 12), (_head, "ws", 8), (_pairwise, "poses", 12), (_pairwise, "af", 4), (_consistency, "Tn", 4),
                       (_consistency, "out", 20), (_agg, "a", 8), (_agg, "theta", 12), (_agg, "weight", 2), (_agg, "out", 4)):
        assert fn(**{arg: ctypes.c_void_p(p)}) == -3, (fn.__name__, arg)
    assert _head(wbytes=0) == -4 and _head(wbytes=hip.lib().coalign_v2vr_pose_head_workspace_bytes(2, 64) - 1) == -4
    assert hip.lib().coalign_v2vr_pose_head_workspace_bytes(2, 64) == (2 * 4 * 64 + 4 * 4) * 4 and hip.lib().coalign_v2vr_pose_head_workspace_bytes(9, 64) == 0
    assert _pool(P=0) == 0 and _pool(P=0, a=NULL, out=NULL) == 0 and _agg(n=0, R=0) == 0 and _agg(R=0, a=NULL) == 0
    assert ops.v2vr_shape_ok(64, 64, 8, 8) and ops.v2vr_shape_ok(256, 256, 5, 5) and not ops.v2vr_shape_ok(64, 32, 2) and not ops.v2vr_shape_ok(24, 64, 2)
    assert not ops.v2vr_shape_ok(64, 64, 9, 9) and not ops.v2vr_shape_ok(64, 64, 6, 5) and not ops.v2vr_shape_ok(64, 64, 2, 17) and not ops.v2vr_shape_ok(64, 1088, 2)


def test_ops_refuse_cpu_tensors():
    x = torch.zeros(4, 64, 6, 6).contiguous(memory_format=torch.channels_last)
    d = lambda *s: torch.zeros(*s, dtype=torch.float64)      # noqa: E731
    with pytest.raises(hip.CoalignHipError):
        ops.v2vr_pool_act(x)
    with pytest.raises(hip.CoalignHipError):
        ops.v2vr_score_head(x, 2, 5, torch.zeros(64), torch.zeros(1), torch.zeros(1))
    with pytest.raises(hip.CoalignHipError):
        ops.v2vr_pairwise(d(2, 3), 5, 24, 24, 19.2, 19.2)
    with pytest.raises(hip.CoalignHipError):
        ops.v2vr_consistency(d(2, 3), d(5, 5, 4, 4), 24, 24, 19.2, 19.2)
    with pytest.raises(hip.CoalignHipError):
        ops.v2vr_aggregate(x, x[:2], x[:2], d(2, 2, 2, 3), torch.zeros(5, 5))
    with pytest.raises(TypeError):
        ops.v2vr_pose_head(x, 2, 5, (), d(5, 5, 4, 4))


# ---- the reference's recorded outputs ------------------------------------------------------------------------------------------------------------------------
def _golden_modules(g):
    C = g["x"].shape[1]
    reg, att = v2v_robust.PoseRegressionWraper(2 * C, 16, AFFINE), v2v_robust.AttentionWrapper(2 * C, 16, AFFINE, True)
    fus = V2VNetFusion({"num_iteration": 2, "in_channels": C, "gru_flag": True, "agg_operator": "weight", "conv_gru": {"H": 24, "W": 40, "num_layers": 1, "kernel_size": [[3, 3]]}})
    for tag, m in (("reg", reg), ("att", att), ("fus", fus)):
        keys = [str(k) for k in g[tag + "_keys"]]
        assert keys == list(m.state_dict().keys()), tag
        m.load_state_dict({k: torch.from_numpy(g[f"{tag}.{k}"]) for k in keys})
        m.eval()
    return reg, att, fus


def test_parts_reproduce_the_references_recorded_outputs(golden):
    """``PoseRegressionWraper``, ``get_intersection``, ``weighted_em``, ``AttentionWrapper`` and ``V2VNetFusion(weight=...)``, each fed the reference's own recorded
    input of that part, against the reference's recorded output; the weights are the ones ``v2v_robust_parameters_`` / ``v2v_parameters_`` regenerate."""
    g = golden("v2v_robust.npz")
    reg, att, fus = _golden_modules(g)
    t = lambda k: torch.from_numpy(g[k])      # noqa: E731
    x, poses, rl = t("x"), t("poses"), [int(v) for v in g["record_len"]]
    with torch.no_grad():
        T = get_pairwise_transformation_torch(poses, 5, rl, dof=3)
        assert_elementwise(T, t("T"), "get_pairwise_transformation_torch", GOLDEN_RTOL, GOLDEN_FLOOR)
        for route in (reg.forward_torch, reg.forward_reduced):
            corr, T_new = route(x, rl, t("T"))
            assert_elementwise(corr, t("corr"), "pose_corr", GOLDEN_RTOL, GOLDEN_FLOOR)
            assert_elementwise(T_new, t("T_new"), "T_new", GOLDEN_RTOL, GOLDEN_FLOOR)
        inter = v2v_robust.get_intersection(t("T_new")[0], AFFINE)
        assert torch.equal(inter, t("intersection")) and inter.unique().tolist() == [0.009999999776482582]
        fixed = v2v_robust.weighted_em(poses[:3], t("T_new")[0], inter)
        print("weighted_em vs the reference:", float((fixed - t("fixed")[:3]).abs().max()))
        assert float((fixed - t("fixed")[:3]).abs().max()) <= 1e-5      # (the reference's own EM moves by 1.2e-5 under 2e-7 relative input noise; same operations here)
        for route in (att.forward_torch, att.forward_reduced):
            scores, weight = route(x, rl, t("T_fixed"))
            assert_elementwise(scores, t("scores"), "scores", GOLDEN_RTOL, GOLDEN_FLOOR)
            assert_elementwise(weight, t("weight"), "weight", GOLDEN_RTOL, GOLDEN_FLOOR)
        A = normalize_pairwise_tfm(t("T_fixed"), 24, 40, 0.4, 2)
        for route in (fus.forward_torch, fus.forward_reduced, fus):
            assert_elementwise(route(x, rl, A, t("weight")), t("fused"), "fused", GOLDEN_RTOL, 1e-5)
    regen = v2v_robust.PoseRegressionWraper(32, 16, AFFINE)
    v2v_robust_parameters_(regen, seed=50)
    assert all(torch.equal(a, b) for a, b in zip(regen.state_dict().values(), reg.state_dict().values()))


def test_model_state_dict_names_match_the_reference(golden):
    g = golden("v2v_robust.npz")
    h = builtin_config("opv2v_pointpillar_v2vnet_robust")
    h["model"]["args"]["point_pillar_scatter"]["grid_size"] = [704, 200, 1]
    sd = build_model(h).state_dict()
    assert list(sd.keys()) == [str(k) for k in g["model_state_keys"]]
    assert [v.numel() for v in sd.values()] == g["model_state_numel"].tolist()
    assert "attention_net.alpha" in sd and float(sd["attention_net.alpha"]) == pytest.approx(0.15)
    h["model"]["args"]["robust"]["learnable_alpha"] = False
    m = build_model(h)
    assert m.attention_net.alpha == 0.35 and "attention_net.alpha" not in m.state_dict()


def test_the_yardstick_agrees_with_the_references_recorded_outputs(golden):
    """tests/v2v_robust_reference.py, written independently of the module, against the reference's float32 results: within float32's own error of them."""
    g = golden("v2v_robust.npz")
    reg, att, fus = _golden_modules(g)
    state = {**{"pose_reg_net." + k: v for k, v in reg.state_dict().items()}, **{"attention_net." + k: v for k, v in att.state_dict().items()},
             **{"fusion_net." + k: v for k, v in fus.state_dict().items()}}
    t = lambda k: torch.from_numpy(g[k])      # noqa: E731
    x, poses = t("x")[:3], t("poses")[:3]
    T = pairwise_f64(poses, 5)
    corr, T_new = pose_regression_f64(state, x, T, AFFINE)
    assert_elementwise(corr, t("corr")[0, :3, :3], "yardstick corr", 1e-4, 1e-5)
    fixed = weighted_em_f64(poses, T_new, intersection_f64(T_new, AFFINE))
    assert float((fixed - t("fixed")[:3].double()).abs().max()) <= 1e-4
    T_fixed = pairwise_f64(fixed, 5)
    scores, weight = attention_f64(state, x, T_fixed, AFFINE)
    assert_elementwise(scores, t("scores")[0], "yardstick scores", 1e-4, 1e-5)
    assert_elementwise(weight, t("weight")[0], "yardstick weight", 1e-4, 1e-5)
    fused = fuse_weight_f64(state, x, normalize_f64(T_fixed, 24, 40, 2, 0.4), {"num_iteration": 2, "gru_flag": True, "conv_gru": {"num_layers": 1}}, weight)
    assert_elementwise(fused, t("fused")[0], "yardstick fused", 1e-4, 1e-5)


# ---- the constant intersection and the identities, one by one ---------------------------------------------------------------------------------------------------
def test_the_intersection_is_constant_whatever_the_poses():
    for seed in range(4):
        g = torch.Generator().manual_seed(seed)
        poses = (torch.rand(5, 3, generator=g) - 0.5) * torch.tensor([60.0, 60.0, 360.0])
        T = get_pairwise_transformation_torch(poses, 5, [5], dof=3)[0]
        inter = v2v_robust.get_intersection(T, AFFINE)
        assert inter.shape == (5, 5) and torch.equal(inter, torch.full((5, 5), 0.01)) and torch.equal(inter, v2v_robust.constant_intersection(T))


def _f64_case(n=3, H=24, W=25, seed=3):
    m, args, _ = model_for(H, W, seed=seed)
    m = m.double()
    x, poses = maps_for(n + 1, H, W, seed).double(), torch.cat([poses_for(n, seed), torch.zeros(1, 3)]).double()
    return m, x, poses, [n, 1]


def test_identity_a_and_b_pose_regression():
    """(a) the split first convolution, (b) pooling before LeakyReLU and the mean of the pooled cropped map: float64, 1e-10 of ``forward_torch``."""
    m, x, poses, rl = _f64_case()
    T = get_pairwise_transformation_torch(poses, 8, rl, dof=3)
    with torch.no_grad():
        full, red = m.pose_reg_net.forward_torch(x, rl, T), m.pose_reg_net.forward_reduced(x, rl, T)
    for a, b in zip(full, red):
        assert float((a - b).abs().max()) <= 1e-10 and float(a.abs().max()) > 0.1
    net = m.pose_reg_net.pose_regression.model
    v = torch.randn(2, 64, 9, 11, dtype=torch.float64) * 3
    assert torch.equal(net[2](net[1](v)), net[1](net[2](v)))                      # lrelu(maxpool(v)) = maxpool(lrelu(v)) bit for bit


def test_identity_a_and_b_attention():
    """(a) the split first convolution, (b) MaxPool 2 + global max = the max over the floor-cropped map: float64, 1e-10 of ``forward_torch``; odd map sizes."""
    m, x, poses, rl = _f64_case(H=25, W=27)
    T = get_pairwise_transformation_torch(poses, 8, rl, dof=3)
    with torch.no_grad():
        full, red = m.attention_net.forward_torch(x, rl, T), m.attention_net.forward_reduced(x, rl, T)
    for a, b in zip(full, red):
        assert float((a - b).abs().max()) <= 1e-10 and float(a.abs().max()) > 0.1
    assert bool((full[0][0, 3:] == 0).all()) and bool((full[0][1, 1:] == 0).all())


def test_identity_c_one_warp_serves_attention_and_fusion():
    """(c) with equal normalisations the attention's theta IS the fusion's: the same SplitMap serves both (float64, 1e-10); with unequal ones the model's kernel
    route is off."""
    m, x, poses, rl = _f64_case()
    T = get_pairwise_transformation_torch(poses, 8, rl, dof=3)
    H, W = x.shape[2:]
    assert m.one_normalisation()
    own = m.attention_net._thetas(T[0], m.H, m.W, H, W)
    assert float((own - m._fusion_affine(T, H, W)[0]).abs().max()) <= 1e-10 and float((own - m.pose_reg_net._thetas(T[0], H, W, H, W)).abs().max()) <= 1e-10
    m.fusion_downsample_rate = 4
    assert not m.one_normalisation() and not m.float().kernel_route(64, 3)


def test_identity_d_the_em_needs_no_warp():
    """(d) ``weighted_em`` with ``get_intersection`` and with the constant: the same poses (float64, 1e-10), and they differ from the input."""
    m, x, poses, rl = _f64_case()
    T = get_pairwise_transformation_torch(poses, 8, rl, dof=3)
    with torch.no_grad():
        _, T_new = m.pose_reg_net.forward_torch(x, rl, T)
        a = v2v_robust.weighted_em(poses[:3], T_new[0], v2v_robust.get_intersection(T_new[0], m.affine_parameter))
        b = v2v_robust.weighted_em(poses[:3], T_new[0], v2v_robust.constant_intersection(T_new[0]))
    assert float((a - b).abs().max()) <= 1e-10 and float((a - poses[:3]).abs().max()) > 0.05


@pytest.mark.parametrize("stage", [0, 1, 2])
def test_forward_reduced_is_forward_torch(stage):
    m, x, poses, rl = _f64_case()
    with torch.no_grad():
        full, red = m.forward_torch(x, rl, poses, stage), m.forward_reduced(x, rl, poses, stage)
    assert set(full) == set(red)
    for k, v in full.items():
        if torch.is_tensor(v):
            assert float((v - red[k]).abs().max()) <= 1e-10 * max(1.0, float(v.abs().max())), k


def test_weighted_fusion_routes_and_refusals():
    """``agg_operator: weight``: ``forward_reduced`` is ``forward_torch`` (float64, 1e-12) and both are the yardstick's loop; without a weight every route raises
    ``ValueError``; other names still raise as before; ``rows`` is refused."""
    args = {"num_iteration": 2, "in_channels": 8, "gru_flag": True, "agg_operator": "weight", "conv_gru": {"H": 6, "W": 7, "num_layers": 1, "kernel_size": [[3, 3]]}}
    m = V2VNetFusion(args).double().eval()
    v2v_parameters_(m, seed=3)
    g = torch.Generator().manual_seed(4)
    x = torch.randn(4, 8, 6, 7, generator=g, dtype=torch.float64)
    T = get_pairwise_transformation_torch(torch.tensor([[0.0, 0, 0], [1.0, 0.5, 10], [-1.0, 0.3, -20], [0.0, 0, 0]], dtype=torch.float64), 5, [3, 1], dof=3)
    A = normalize_pairwise_tfm(T, 6, 7, 0.4, 2)
    w = torch.rand(2, 5, 5, generator=g, dtype=torch.float64)
    with torch.no_grad():
        full, red = m.forward_torch(x, [3, 1], A, w), m.forward_reduced(x, [3, 1], A, w)
        assert float((full - red).abs().max()) <= 1e-12 * float(full.abs().max())
        ref = fuse_weight_f64({"fusion_net." + k: v for k, v in m.state_dict().items()}, x[:3], A[0], args, w[0])
        assert float((full[0] - ref).abs().max()) <= 1e-6 * float(ref.abs().max())          # (the yardstick samples at float32 positions)
        for fn in (m, m.forward_torch, m.forward_reduced):
            with pytest.raises(ValueError):
                fn(x, [3, 1], A)
        with pytest.raises(ValueError):
            m.forward_kernels(x, [3, 1], A)
        with pytest.raises(NotImplementedError):
            m(x, [3, 1], A, w, rows=[0])
    m.agg_operator = "sum"
    for fn in (m, m.forward_torch, m.forward_reduced):
        with pytest.raises(ValueError):
            fn(x, [3, 1], A, w)
    with pytest.raises(ValueError):
        m.kernel_route(64, 1)
    m.agg_operator = "weight"
    assert m.kernel_route(64, 1) == V2VNetFusion(dict(args, agg_operator="max")).eval().kernel_route(64, 1)


# ---- the model ---------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", CONFIGS)
def test_build_model_constructs_the_model(cfg):
    """``build_model`` answered ``KeyError`` for this family before it existed."""
    hypes = builtin_config(cfg)
    model = build_model(hypes)
    assert isinstance(model, PointPillarV2VNetRobust) and BASELINE_REGISTRY["point_pillar_v2vnet_robust"] is PointPillarV2VNetRobust
    assert "point_pillar_v2vnet_robust" not in MODEL_REGISTRY and model.fusion_net.agg_operator == "weight" and model.stage == 2
    from coalign_amd import opencood_compat
    opencood_compat.install()
    import importlib
    assert importlib.import_module("opencood.models.point_pillar_v2vnet_robust").PointPillarV2VNetRobust is PointPillarV2VNetRobust
    assert importlib.import_module("opencood.models.sub_modules.v2v_robust_module").WeightedEM is v2v_robust.weighted_em
    hypes["model"]["args"]["compression"] = 4
    assert build_model(hypes).naive_compressor.encoder[0].in_channels == 256


def test_noise_contract():
    """Zeros for ``pose_noise`` reproduce ``eval_forward``; the caller's ``lidar_pose`` is unchanged; every stage returns the reference's keys; without the key the
    noise is drawn (two calls differ) and a seed repeats it."""
    H, W = 24, 24
    x, rl = maps_for(4, H, W), [3, 1]
    lidar_pose = torch.zeros(4, 6)
    lidar_pose[:, [0, 1, 4]] = torch.cat([poses_for(3, 5), torch.zeros(1, 3)])
    before = lidar_pose.clone()
    keys = {0: {"stage", "scores", "choice", "cls_preds", "reg_preds"}, 1: {"stage", "pairwise_corr", "pairwise_t_matrix"},
            2: {"stage", "scores", "cls_preds", "reg_preds", "pairwise_corr", "pairwise_t_matrix"}}
    with torch.no_grad():
        for stage in (0, 1, 2):
            m, _, _ = model_for(H, W, stage)
            torch.manual_seed(7)
            a = m.train_forward(x, rl, lidar_pose)
            torch.manual_seed(7)
            b = m.train_forward(x, rl, lidar_pose)
            c = m.train_forward(x, rl, lidar_pose)
            assert set(a) == keys[stage] and a["stage"] == stage and torch.equal(lidar_pose, before)
            probe = "pairwise_t_matrix" if stage else "cls_preds"
            assert torch.equal(a[probe], b[probe]) and not torch.equal(a[probe], c[probe])
            if stage == 0:
                assert a["choice"].shape == (4, 1) and set(a["choice"].flatten().tolist()) <= {0, 1}
        zero = m.train_forward(x, rl, lidar_pose, noise=torch.zeros(4, 6))
        ev = m.eval_forward(x, rl, lidar_pose)
        assert set(ev) == {"stage", "scores", "cls_preds", "reg_preds", "pairwise_t_matrix"}
        for k in ("scores", "cls_preds", "reg_preds"):
            assert torch.equal(zero[k], ev[k]), k
        assert not torch.equal(ev["pairwise_t_matrix"], zero["pairwise_t_matrix"])      # eval_forward returns the REGRESSED matrices, train_forward the noisy ones
        assert torch.equal(lidar_pose, before)


def test_noise_statistics_match_generate_noise_torch():
    """4000 seeded draws of ``noise_generator``: the position noise is N(0, 0.4) and the yaw entry a von Mises sample of concentration (180 / (pi 4))^2 -- in radians --
    each mean and standard deviation within 5 sigma of its sampling error; the other entries are zero.  The same bounds hold for ``generate_noise_torch`` itself."""
    m, _, _ = model_for(24, 24)
    N = 4000
    kappa = (180 / (np.pi * 4)) ** 2
    yaw_std = 1 / np.sqrt(kappa) * (1 + 1 / (4 * kappa))                      # var = 1 / kappa + 1 / (2 kappa^2) + ..: 0.0698 rad for a 4 degree standard deviation
    for draw in (lambda: m.noise_generator(torch.zeros(N, 6), all_strong=True)[0], lambda: generate_noise_torch(torch.zeros(N, 6), 0.4, 4)):
        torch.manual_seed(11)
        noise = draw()
        assert noise.shape == (N, 6) and bool((noise[:, [2, 3, 5]] == 0).all())
        for col, std in ((0, 0.4), (1, 0.4), (4, yaw_std)):
            v = noise[:, col].double()
            assert abs(float(v.mean())) <= 5 * std / np.sqrt(N), (col, float(v.mean()))
            assert abs(float(v.std()) - std) <= 5 * std / np.sqrt(2 * N), (col, float(v.std()), std)
    torch.manual_seed(12)
    mixed, choice = m.noise_generator(torch.zeros(N, 6), all_strong=False)
    weak = mixed[choice.flatten() == 1]
    assert 0.4 < float(choice.float().mean()) < 0.6 and float(weak[:, :2].abs().max()) < 0.06 and float(mixed[choice.flatten() == 0][:, 0].std()) > 0.3


def test_refusals():
    m, _, _ = model_for(24, 24)
    lidar_pose = torch.zeros(2, 6)
    with torch.no_grad():
        for shape in ((2, 64, 24, 25), (2, 64, 25, 24)):
            with pytest.raises(NotImplementedError):
                m.train_forward(torch.zeros(*shape), [2], lidar_pose)
        for H, W in ((23, 24), (24, 23), (16, 32)):
            small, _, _ = model_for(H, W)
            for route in (small.forward_torch, small.forward_reduced, small.forward_kernels):
                with pytest.raises(NotImplementedError):
                    route(torch.zeros(2, 64, H, W), [2], torch.zeros(2, 3))
        one = m.forward_torch(maps_for(1, 24, 24), [1], torch.tensor([[1.0, 2.0, 3.0]]))      # one agent passes through everywhere
    assert torch.equal(one["lidar_pose_corrected"], torch.tensor([[1.0, 2.0, 3.0]])) and float(one["scores"][0, 0, 0]) > 0 and bool((one["scores"][0].flatten()[1:] == 0).all())
    h = hypes_for(24, 24)
    h["model"]["args"]["v2vfusion"]["agg_operator"] = "sum"
    with pytest.raises(ValueError):
        build_model(h).eval().forward_torch(maps_for(2, 24, 24), [2], torch.zeros(2, 3))
    assert not m.train().kernel_route(64, 2) and m.eval().kernel_route(64, 2) and not m.kernel_route(64, 9) and not m.kernel_route(48, 2)
    m.force_torch = True
    assert not m.kernel_route(64, 2)


def test_float32_route_error_against_the_yardstick_is_the_recorded_e32():
    """E32, the error of the float32 ``forward_torch`` route against the float64 yardstick, is what bounds the kernel route on the GPU (4 x E32,
    tests/test_v2v_robust_gpu.py): one case re-measured here stays within the recorded worst case."""
    from test_v2v_robust_gpu import E32
    m, _, _ = model_for(25, 41)
    args, state, x, poses, ref, _ = case(25, 41, 3)
    with torch.no_grad():
        got = m.forward_torch(x, [3], poses)
    e = errors(got, ref, 3)
    print("E32 at 25 x 41, 3 agents:", e)
    for k, v in e.items():
        assert v <= E32[k], (k, v)


def test_routes_plan_both_walks():
    for cfg in CONFIGS:
        h = builtin_config(cfg)
        h["model"]["args"]["point_pillar_scatter"]["grid_size"] = [704, 200, 1] if cfg.startswith("opv2v") else [112, 56, 1]
        p = routes.plan(h)
        assert p["outside_hot_path"] == "model family 'point_pillar_v2vnet_robust' is not part of the CoAlign hot path" and p["layers"] == {}
        p = routes.plan(h, baselines=True)
        assert p["outside_hot_path"] is None and p["fusion"] == routes.V2VR
        L = p["layers"]
        for k in (0, 3, 6):
            assert L[f"pose_reg_net.pose_regression.model.{k}"].startswith(routes.SP), k
        assert L["pose_reg_net.pose_regression.model.9"].startswith(routes.SP_S2)
        for k in (14, 16, 18):
            assert L[f"pose_reg_net.pose_regression.model.{k}"].startswith("v2vr_pose_head")
        assert L["attention_net.attention_net.model.0"].startswith(routes.SP) and L["attention_net.attention_net.model.3"].startswith(routes.SP)
        assert L["attention_net.attention_net.model.8"].startswith("v2vr_score_head") and L["fusion_net.msg_cnn"].startswith(routes.SP)
        assert "fusion" not in p["fallbacks"] and not [f for f in p["fallbacks"] if f.startswith(("pose_reg_net", "attention_net", "fusion_net"))]
    h = builtin_config("mini_pointpillar_v2vnet_robust")
    h["model"]["args"]["point_pillar_scatter"]["grid_size"] = [112, 56, 1]
    h["model"]["args"]["robust"]["hidden_dim"] = 48
    p = routes.plan(h, baselines=True)
    assert p["fusion"].startswith(routes.V2VR_TORCH) and "fusion" in p["fallbacks"] and p["layers"]["attention_net.attention_net.model.8"].startswith(routes.ROCBLAS.split(" (")[0])
