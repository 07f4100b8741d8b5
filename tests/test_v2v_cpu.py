"""V2VNet's message passing, host side (no GPU): the extension header include/coalign_amd_v2v.h against the product library and ``hip.V2V_SIGNATURES``, argument
validation before any HIP call, ``fusion.V2VNetFusion`` against the reference's recorded output (tests/golden/v2v_fuse.npz, written by
tests/golden/make_v2v_golden.py) and against float64, the three identities of ``forward_reduced``, the sliced GRU weights, and the ``point_pillar_baseline``
model: construction, names, alias, route plan, forward."""
import copy
import ctypes
import os
import re

import pytest
import torch

import abi_headers
from conftest import assert_elementwise
from coalign_amd import hip, ops
from coalign_amd.config import builtin_config
from coalign_amd.detector import BASELINE_REGISTRY, MODEL_REGISTRY, PointPillarBaseline, build_model
from coalign_amd.fusion import AttFusion, DiscoFusion, MaxFusion, V2VNetFusion
from coalign_amd.synthetic import fill_parameters_, v2v_parameters_
from v2v_reference import assert_not_degenerate, make_thetas, v2v_fuse_f64

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NULL, ONE = ctypes.c_void_p(0), ctypes.c_void_p(16)      # (a non-NULL, 16-byte aligned token: none of these calls gets as far as touching memory)
HEADER = "coalign_amd_v2v.h"
CONFIGS = ("opv2v_pointpillar_v2vnet", "mini_pointpillar_v2vnet")
GOLDEN_ARGS = {"num_iteration": 2, "in_channels": 16, "gru_flag": True, "agg_operator": "max", "conv_gru": {"H": 9, "W": 14, "num_layers": 1, "kernel_size": [[3, 3]]}}


def test_v2v_header_table_and_library_agree():
    """include/coalign_amd_v2v.h declares exactly the keys of ``hip.V2V_SIGNATURES`` (types, counts and exports: tests/test_abi_cpu.py); the header includes
    coalign_amd.h and cites the reference lines."""
    text = open(abi_headers.path(HEADER)).read()
    assert '#include "coalign_amd.h"' in text
    declared = abi_headers.declarations(HEADER)
    assert set(declared) == set(hip.V2V_SIGNATURES) == abi_headers.names(HEADER) == {"coalign_v2v_warp_split", "coalign_v2v_aggregate", "coalign_v2v_gate"}
    comments = re.findall(r"/\*.*?\*/", text, flags=re.S)
    for name in declared:
        last = [c for c in comments if c in text[:text.index(name + "(")]][-1]
        assert "fusion_in_one.py:173-293" in last, name


def test_build_lists_the_new_header_and_source():
    src = open(os.path.join(REPO, "coalign_amd", "build.py")).read()
    assert '"coalign_amd_v2v.h"' in src and '"v2v_fuse.hip"' in src


def _warp(x=ONE, n=3, R=3, C=64, H=9, W=14, theta=ONE, y=ONE, flag=NULL):
    return hip.lib().coalign_v2v_warp_split(x, n, R, C, H, W, theta, y, flag, NULL)


def _agg(a=ONE, e=ONE, x=ONE, n=3, R=3, C=64, H=9, W=14, theta=ONE, agg=0, kind=1, out=ONE, flag=NULL):
    return hip.lib().coalign_v2v_aggregate(a, e, x, n, R, C, H, W, theta, agg, kind, out, flag, NULL)


def _gate(y=ONE, R=3, Ch=64, H=9, W=14, kind=0, out=ONE, flag=NULL):
    return hip.lib().coalign_v2v_gate(y, R, Ch, H, W, kind, out, flag, NULL)


def test_v2v_argument_validation_without_a_gpu():
    """NULL -1; negative counts, C / H / W < 1, R > n, maps of 2^31 floats -2; n > 8, C = 24, another agg / out_kind, unaligned pointers -3; n = 0 and R = 0 are OK
    without a launch: all before any HIP call (token pointers, no GPU)."""
    for arg in ("x", "theta", "y"):
        assert _warp(**{arg: NULL}) == -1, arg
    for arg in ("a", "e", "x", "theta", "out"):
        assert _agg(**{arg: NULL}) == -1, arg
    for arg in ("y", "out"):
        assert _gate(**{arg: NULL}) == -1, arg
    for bad in (dict(n=-1), dict(R=-1), dict(C=0), dict(H=0), dict(W=0), dict(H=-2), dict(C=-16), dict(n=2, R=3)):
        assert _warp(**bad) == -2 and _agg(**bad) == -2, bad
    for bad in (dict(R=-1), dict(Ch=0), dict(H=0), dict(W=-3)):
        assert _gate(**bad) == -2, bad
    for bad in (dict(n=9, R=1), dict(n=64, R=64), dict(C=24), dict(C=100), dict(C=8)):
        assert _warp(**bad) == -3 and _agg(**bad) == -3, bad
    assert _gate(Ch=24) == -3 and _gate(kind=2) == -3 and _agg(agg=2) == -3 and _agg(kind=5) == -3 and _agg(agg=-1) == -3
    for fn in (_warp, _agg):
        assert fn(n=0, R=0) == 0 and fn(n=3, R=0) == 0 and fn(n=0, R=0, x=NULL, theta=NULL) == 0
    assert _gate(R=0) == 0 and _gate(R=0, y=NULL, out=NULL) == 0
    assert _warp(n=8, R=8, C=64, H=1024, W=1024) == -2 and _agg(n=8, R=8, C=64, H=1024, W=1024) == -2      # R n C H W = 2^32 floats
    assert _warp(n=1, R=1, C=16, H=46341, W=46341) == -2 and _gate(R=1, Ch=16, H=46341, W=46341) == -2
    assert _warp(x=ctypes.c_void_p(20)) == -3 and _warp(y=ctypes.c_void_p(8)) == -3 and _warp(theta=ctypes.c_void_p(12)) == -3 and _warp(flag=ctypes.c_void_p(18)) == -3
    assert _agg(a=ctypes.c_void_p(4)) == -3 and _agg(e=ctypes.c_void_p(24)) == -3 and _agg(out=ctypes.c_void_p(8)) == -3 and _agg(theta=ctypes.c_void_p(4)) == -3
    assert _gate(y=ctypes.c_void_p(8)) == -3 and _gate(out=ctypes.c_void_p(4)) == -3
    assert ops.v2v_shape_ok(64, 8) and ops.v2v_shape_ok(16, 1) and not ops.v2v_shape_ok(24, 2) and not ops.v2v_shape_ok(64, 9) and not ops.v2v_shape_ok(64, 0)


def test_v2v_ops_refuse_cpu_tensors():
    x = torch.zeros(2, 16, 3, 3).contiguous(memory_format=torch.channels_last)
    th = torch.zeros(2, 2, 2, 3, dtype=torch.float64)
    with pytest.raises(hip.CoalignHipError):
        ops.v2v_warp_split(x, th)
    with pytest.raises(hip.CoalignHipError):
        ops.v2v_aggregate(torch.cat([x, x]), x, x, th)
    with pytest.raises(hip.CoalignHipError):
        ops.v2v_gate(torch.zeros(2, 32, 3, 3).contiguous(memory_format=torch.channels_last))


@pytest.fixture(scope="module")
def recorded(golden):
    g = golden("v2v_fuse.npz")
    m = V2VNetFusion(copy.deepcopy(GOLDEN_ARGS))
    state = {str(k): torch.from_numpy(g["sd." + str(k)]) for k in g["state_keys"]}
    m.load_state_dict(state, strict=True)                                  # the reference's parameter names
    return g, m.eval(), state


def test_v2v_fusion_reproduces_the_reference_recording(recorded):
    """``V2VNetFusion`` loaded from the reference's ``state_dict`` gives the reference's recorded output on the CPU (``forward`` = the op-by-op route there, and
    ``forward_reduced``); the float64 restatement agrees with both, and the recorded case is one in which every stage matters."""
    g, m, state = recorded
    x, rl, A = torch.from_numpy(g["x"]), torch.from_numpy(g["record_len"]), torch.from_numpy(g["affine"])
    with torch.no_grad():
        got, red = m(x, rl, A), m.forward_reduced(x, rl, A)
    assert_elementwise(got, torch.from_numpy(g["out"]), "V2VNetFusion on the CPU vs the reference's recording")
    assert_elementwise(red, torch.from_numpy(g["out"]), "forward_reduced (float32) vs the reference's recording")
    off = 0
    for b, n in enumerate(rl.tolist()):
        trace = {}
        ref = v2v_fuse_f64(state, x[off:off + n], A[b, :n, :n], GOLDEN_ARGS, trace=trace)
        assert_not_degenerate(state, x[off:off + n], A[b, :n, :n], GOLDEN_ARGS, ref, trace, f"frame {b}")
        assert_elementwise(torch.from_numpy(g["out"][b]), ref, f"the reference's recording vs float64, frame {b}")
        assert_elementwise(got[b], ref, f"V2VNetFusion vs float64, frame {b}")
        off += n


def _module(C, K, layers, gru, agg, seed=0):
    m = V2VNetFusion({"num_iteration": K, "in_channels": C, "gru_flag": gru, "agg_operator": agg, "conv_gru": {"H": 6, "W": 7, "num_layers": layers, "kernel_size": [[3, 3]] * layers}})
    v2v_parameters_(m, seed=seed)
    return m.double().eval()


@pytest.mark.parametrize("agg", ["max", "avg"])
@pytest.mark.parametrize("K", [1, 2, 3])
@pytest.mark.parametrize("layers,gru", [(1, True), (2, True), (1, False)])
def test_forward_reduced_equals_forward_torch_in_float64(agg, K, layers, gru):
    """The three identities are exact: in float64 ``forward_reduced`` equals the reference's loops within 1e-12 of the scale (rounding order only), for batches of
    one to four agents with every receiver row of the affine matrix filled."""
    m = _module(8, K, layers, gru, agg, seed=K)
    for groups in ([1], [2, 3], [4]):
        x = torch.randn(sum(groups), 8, 6, 7, dtype=torch.float64, generator=torch.Generator().manual_seed(7 + len(groups)))
        A = torch.eye(2, 3, dtype=torch.float64).repeat(len(groups), 5, 5, 1, 1)
        for b, n in enumerate(groups):
            A[b, :n, :n] = make_thetas(n, 6, 7, seed=b)
        with torch.no_grad():
            full, red = m.forward_torch(x, groups, A), m.forward_reduced(x, groups, A)
        assert full.shape == (len(groups), 8, 6, 7)
        worst = float((full - red).abs().max()) / float(full.abs().max())
        assert worst <= 1e-12, (groups, worst)


def test_a_wrong_agg_operator_raises_like_the_reference():
    m = _module(8, 1, 1, True, "sum")
    x, A = torch.zeros(1, 8, 6, 7, dtype=torch.float64), torch.eye(2, 3, dtype=torch.float64).repeat(1, 5, 5, 1, 1)
    for fn in (m, m.forward_torch, m.forward_reduced):
        with pytest.raises(ValueError):
            fn(x, [1], A)
    with pytest.raises(ValueError):
        m.kernel_route(64, 1)
    with pytest.raises(NotImplementedError):
        _module(8, 1, 1, True, "max")(x, [1], A, rows=[0])


def test_sliced_gru_weights_are_the_stated_rows_and_columns():
    """``ConvGRUCell.reduced``: rows [hidden, 2 hidden) of conv_gates stacked on conv_can, the first ``input_dim`` input columns, biases alike; ``reduced_weights``
    splits msg_cnn at column C; the kernel route's images are cached until a parameter changes."""
    m = _module(8, 2, 2, True, "max").float()
    for k, cell in enumerate(m.conv_gru.cell_list):
        inp, hid = (16, 8) if k == 0 else (8, 8)
        w, b = cell.reduced()
        assert cell.input_dim == inp and cell.hidden_dim == hid and w.shape == (2 * hid, inp, 3, 3) and b.shape == (2 * hid,)
        assert torch.equal(w[:hid], cell.conv_gates.weight[hid:, :inp]) and torch.equal(w[hid:], cell.conv_can.weight[:, :inp])
        assert torch.equal(b[:hid], cell.conv_gates.bias[hid:]) and torch.equal(b[hid:], cell.conv_can.bias)
    wn, we, bm, cells = m.reduced_weights()
    assert torch.equal(wn, m.msg_cnn.weight[:, :8]) and torch.equal(we, m.msg_cnn.weight[:, 8:]) and bm is m.msg_cnn.bias and len(cells) == 2


@pytest.mark.parametrize("cfg", CONFIGS)
def test_build_model_constructs_the_baseline(cfg):
    """``build_model`` constructs ``point_pillar_baseline`` from both shipped yamls (a KeyError before this model existed) and their max / att / disconet variants;
    v2xvit is refused at construction."""
    hypes = builtin_config(cfg)
    model = build_model(hypes)
    C = hypes["model"]["args"]["shrink_header"]["dim"][-1]
    assert isinstance(model, PointPillarBaseline) and BASELINE_REGISTRY["point_pillar_baseline"] is PointPillarBaseline and "point_pillar_baseline" not in MODEL_REGISTRY
    assert isinstance(model.fusion_net, V2VNetFusion) and model.out_channel == C and model.fusion_net.msg_cnn.in_channels == 2 * C
    for method, extra, kind in (("max", {}, MaxFusion), ("att", {"att": {"feat_dim": C}}, AttFusion), ("disconet", {"disconet": {"feat_dim": C}}, DiscoFusion)):
        h = builtin_config(cfg)
        h["model"]["args"].update(fusion_method=method, **extra)
        assert isinstance(build_model(h).fusion_net, kind), method
    for method in ("v2xvit", "when2comm", "nothing"):
        h = builtin_config(cfg)
        h["model"]["args"]["fusion_method"] = method
        with pytest.raises(NotImplementedError):
            build_model(h)
    h = builtin_config(cfg)
    h["model"]["args"]["base_bev_backbone"]["resnet"] = True
    h["model"]["args"]["compression"] = 4
    m = build_model(h)
    assert type(m.backbone).__name__ == "ResNetBEVBackbone" and m.compression and m.naive_compressor.encoder[0].in_channels == C


def test_state_dict_names_match_the_reference(golden):
    g = golden("v2v_fuse.npz")
    sd = build_model(builtin_config("opv2v_pointpillar_v2vnet")).state_dict()
    assert list(sd.keys()) == [str(k) for k in g["model_state_keys"]]
    assert [v.numel() for v in sd.values()] == list(g["model_state_numel"])
    assert list(V2VNetFusion(copy.deepcopy(GOLDEN_ARGS)).state_dict().keys()) == [str(k) for k in g["state_keys"]]


def test_opencood_alias_resolves_the_model():
    import sys
    if os.path.isdir("/root/reference") and "/root/reference" in sys.path:
        pytest.skip("a real opencood checkout is on sys.path in this process")
    import importlib
    from coalign_amd import opencood_compat
    opencood_compat.install()
    assert importlib.import_module("opencood.models.point_pillar_baseline").PointPillarBaseline is PointPillarBaseline
    from opencood.models.fuse_modules.fusion_in_one import V2VNetFusion as V
    assert V is V2VNetFusion


def test_route_plan_names_the_v2vnet_route():
    """``plan(h, baselines=True)`` names the kernel route, lists msg_cnn / conv_gates / conv_can / mlp under the kernels that serve them and the OPV2V config's strided
    shrink convolution as a fallback; the default ``plan(h)`` reports the family as outside the hot path; a width the route does not take is named with its reason."""
    from coalign_amd.routes import SP, V2V, plan
    for cfg in CONFIGS:
        h = builtin_config(cfg)
        assert plan(h) == {"model": "point_pillar_baseline", "outside_hot_path": "model family 'point_pillar_baseline' is not part of the CoAlign hot path", "layers": {}, "fallbacks": []}
        p = plan(h, baselines=True)
        assert p["outside_hot_path"] is None and p["fusion"] == V2V and V2V.startswith("v2v_warp_split + conv3x3_sp + v2v_aggregate")
        for name in ("fusion_net.msg_cnn", "fusion_net.conv_gru.cell_list.0.conv_gates", "fusion_net.conv_gru.cell_list.0.conv_can"):
            assert p["layers"][name].startswith(SP), name
        assert p["layers"]["fusion_net.mlp"].startswith("pointwise")
        strided = "shrink_conv.layers.0.double_conv.0"
        assert p["fallbacks"] == ([strided] if cfg.startswith("opv2v") else [])
        if cfg.startswith("opv2v"):
            assert p["layers"][strided].startswith("MIOpen") and "strided" in p["layers"][strided]
    odd = builtin_config("mini_pointpillar_v2vnet")
    odd["model"]["args"]["shrink_header"]["dim"] = [48]
    odd["model"]["args"]["v2vnet"]["in_channels"] = 48
    p = plan(odd, baselines=True)
    assert "fusion" in p["fallbacks"] and p["fusion"].startswith("V2VNetFusion op by op") and "48 channels" in p["fusion"]
    assert "fusion_net.msg_cnn" in p["fallbacks"] and "fusion_net.mlp" in p["fallbacks"]
    native = plan(builtin_config("mini_pointpillar_v2vnet"), terms=0, baselines=True)
    assert native["fusion"].startswith("V2VNetFusion op by op") and "not in force" in native["fusion"]


def test_kernel_route_conditions():
    m = V2VNetFusion({"num_iteration": 2, "in_channels": 64, "gru_flag": True, "agg_operator": "max", "conv_gru": {"H": 4, "W": 4, "num_layers": 1, "kernel_size": [[3, 3]]}})
    assert not m.kernel_route(64, 3)                                         # training mode
    m.eval()
    assert m.kernel_route(64, 1) and m.kernel_route(64, 8) and not m.kernel_route(64, 9) and not m.kernel_route(128, 2)
    m.force_torch = True
    assert not m.kernel_route(64, 3)
    wide = V2VNetFusion({"num_iteration": 1, "in_channels": 576, "gru_flag": True, "agg_operator": "avg", "conv_gru": {"H": 4, "W": 4, "num_layers": 1, "kernel_size": [[3, 3]]}}).eval()
    assert not wide.kernel_route(576, 2)                                     # 2C beyond conv3x3_sp's 1024 channels
    k5 = V2VNetFusion({"num_iteration": 1, "in_channels": 64, "gru_flag": True, "agg_operator": "avg", "conv_gru": {"H": 4, "W": 4, "num_layers": 1, "kernel_size": [[5, 5]]}}).eval()
    assert not k5.kernel_route(64, 2)


class _CpuEncoder(torch.nn.Module):
    """Stands in for the pillar encoder + scatter (HIP only) on the CPU: a fixed random canvas per agent."""

    def __init__(self, ny, nx):
        super().__init__()
        self.ny, self.nx = ny, nx

    def forward(self, batch):
        n = sum(batch["record_len"])
        batch["spatial_features"] = torch.randn(n, 64, self.ny, self.nx, generator=torch.Generator().manual_seed(5))
        return batch


def test_forward_on_the_cpu():
    """The mini model's forward on the CPU (op-by-op fusion; the HIP pillar encoder replaced by a stand-in canvas): the reference's three outputs, and the second
    agent is seen through the off-ego affine rows."""
    hypes = builtin_config("mini_pointpillar_v2vnet")
    model = build_model(hypes)
    fill_parameters_(model, seed=3)
    v2v_parameters_(model.fusion_net, seed=3)
    model.eval()
    model.pillar_vfe, model.scatter = torch.nn.Identity(), _CpuEncoder(model.scatter.ny, model.scatter.nx)
    pair = torch.eye(4, dtype=torch.float64).repeat(1, 5, 5, 1, 1)
    pair[0, 0, 1, 0, 3], pair[0, 1, 0, 0, 3], pair[0, 2, 1, 1, 3] = 1.3, -1.3, 0.9
    batch = {"processed_lidar": {"voxel_features": torch.zeros(1, 32, 4), "voxel_coords": torch.zeros(1, 4, dtype=torch.int32), "voxel_num_points": torch.ones(1, dtype=torch.int32)},
             "record_len": torch.tensor([3]), "pairwise_t_matrix": pair}
    with torch.no_grad():
        out = model(batch)
        pair2 = pair.clone()
        pair2[0, 2, 1, 1, 3] = 2.1                                           # agent 2's view of agent 1: reaches the ego only through the second iteration
        out2 = model(dict(batch, pairwise_t_matrix=pair2))
    H, W = model.scatter.ny // 2, model.scatter.nx // 2
    assert set(out) == {"cls_preds", "reg_preds", "dir_preds"}
    assert out["cls_preds"].shape == (1, 2, H, W) and out["reg_preds"].shape == (1, 14, H, W) and out["dir_preds"].shape == (1, 4, H, W)
    assert all(bool(torch.isfinite(v).all()) for v in out.values())
    assert not torch.equal(out["reg_preds"], out2["reg_preds"])
