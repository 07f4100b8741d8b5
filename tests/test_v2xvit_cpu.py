"""V2X-ViT's fusion, host side (no GPU): the extension header include/coalign_amd_v2x.h against the product library and ``hip.V2X_SIGNATURES``, argument validation
before any HIP call, ``fusion.V2XViTFusion`` against the reference's recorded outputs (tests/golden/v2xvit_fuse.npz, written by tests/golden/make_v2xvit_golden.py)
and the reference's parameter names, what the reference's identity STTF and ROI mask were found to do, the identities of ``forward_reduced`` in float64, and the
``point_pillar_baseline`` model with ``fusion_method: v2xvit``: construction, names, route plan, refusals."""
import copy
import ctypes
import os

import numpy as np
import pytest
import torch

import abi_headers
from conftest import assert_elementwise
from coalign_amd import hip, ops
from coalign_amd.config import builtin_config
from coalign_amd.detector import PointPillarBaseline, build_model
from coalign_amd.fusion import V2XViTFusion
from coalign_amd.synthetic import v2xvit_parameters_
from coalign_amd.v2xvit import HGTCavAttention, PreNorm, STTF, agent_attention_reduced, folded_agent_attention
from v2v_reference import make_thetas
from v2xvit_reference import ARGS_A, ARGS_B, SEED_A, SEED_B, agent_attention_f64, args, examine, inputs, weight_checksum

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NULL, ONE = ctypes.c_void_p(0), ctypes.c_void_p(16)      # (a non-NULL, 16-byte aligned token: none of these calls gets as far as touching memory)
HEADER = "coalign_amd_v2x.h"
CONFIGS = ("opv2v_pointpillar_v2xvit", "mini_pointpillar_v2xvit")


def test_v2x_header_table_and_library_agree():
    """include/coalign_amd_v2x.h declares exactly the keys of ``hip.V2X_SIGNATURES`` (types, counts and exports: tests/test_abi_cpu.py) and cites the reference;
    build.py lists the header and the source."""
    text = open(abi_headers.path(HEADER)).read()
    assert '#include "coalign_amd.h"' in text and "hmsa.py:7-151" in text
    declared = abi_headers.declarations(HEADER)
    assert set(declared) == set(hip.V2X_SIGNATURES) == abi_headers.names(HEADER) == {"coalign_v2x_param_bytes", "coalign_v2x_workspace_bytes", "coalign_v2x_agent_attention"}
    src = open(os.path.join(REPO, "coalign_amd", "build.py")).read()
    assert '"coalign_amd_v2x.h"' in src and '"v2x_attn.hip"' in src


def _att(x=ONE, n=3, R=3, C=256, H=5, W=7, theta=ONE, params=ONE, pbytes=None, out=ONE, ws=ONE, wbytes=None):
    L = hip.lib()
    pbytes = L.coalign_v2x_param_bytes(C) if pbytes is None else pbytes
    wbytes = L.coalign_v2x_workspace_bytes(n, C, H, W) if wbytes is None else wbytes
    return L.coalign_v2x_agent_attention(x, n, R, C, H, W, theta, params, pbytes, out, ws, wbytes, NULL)


def test_v2x_argument_validation_without_a_gpu():
    """NULL -1 (theta may be NULL: the maps are read in place); negative counts, R > n, C / H / W < 1, a map of 2^31 floats, a wrong image size, a short workspace -2;
    n > 8, a C that is neither 64 nor 256, 1 < R < n, unaligned pointers -3; n = 0 and R = 0 are OK without a launch: all before any HIP call (token pointers)."""
    L = hip.lib()
    for arg in ("x", "params", "out", "ws"):
        assert _att(**{arg: NULL}) == -1, arg
    for bad in (dict(n=-1, R=-1), dict(R=-1), dict(n=2, R=3), dict(C=0), dict(H=0), dict(W=0), dict(H=-2), dict(C=-64)):
        assert _att(**bad, pbytes=1, wbytes=1) == -2, bad
    for bad in (dict(n=9, R=9), dict(n=9, R=1), dict(C=32), dict(C=128), dict(C=96), dict(C=512), dict(n=3, R=2), dict(n=8, R=5)):
        assert _att(**bad, pbytes=1, wbytes=1) == -3, bad
    assert _att(n=0, R=0) == 0 and _att(n=0, R=0, x=NULL, params=NULL, out=NULL, ws=NULL) == 0 and _att(n=3, R=0, x=NULL) == 0
    assert _att(n=1, R=1, C=64, H=8192, W=4096, wbytes=1 << 40) == -2                         # C H W = 2^31
    assert _att(pbytes=L.coalign_v2x_param_bytes(256) - 4) == -2 and _att(C=64, pbytes=L.coalign_v2x_param_bytes(256)) == -2
    assert _att(wbytes=L.coalign_v2x_workspace_bytes(3, 256, 5, 7) - 4) == -2 and _att(n=5, R=5, wbytes=L.coalign_v2x_workspace_bytes(3, 256, 5, 7)) == -2
    for arg, p in (("x", 20), ("out", 8), ("params", 4), ("ws", 24), ("theta", 12)):
        assert _att(**{arg: ctypes.c_void_p(p)}) == -3, arg
    assert L.coalign_v2x_param_bytes(256) == 16 * 32 * 2048 + 16 * 256 and L.coalign_v2x_param_bytes(64) == 4 * 8 * 2048 + 16 * 64
    assert L.coalign_v2x_param_bytes(128) == 0 and L.coalign_v2x_param_bytes(0) == 0
    assert L.coalign_v2x_workspace_bytes(5, 256, 48, 176) == 5 * 48 * 176 * 768 * 4
    assert L.coalign_v2x_workspace_bytes(9, 256, 4, 4) == 0 and L.coalign_v2x_workspace_bytes(0, 256, 4, 4) == 0 and L.coalign_v2x_workspace_bytes(2, 48, 4, 4) == 0


def test_shape_predicate_and_cpu_refusal():
    ok = ops.v2x_attn_shape_ok
    assert ok(256, 8, 32, 5) and ok(64, 2, 32, 1) and ok(256, 8, 32, 8)
    assert not ok(256, 8, 32, 9) and not ok(256, 8, 32, 0) and not ok(256, 4, 64, 2) and not ok(128, 4, 32, 2) and not ok(32, 2, 16, 2) and not ok(64, 8, 32, 2)
    with pytest.raises(hip.CoalignHipError):
        ops.v2x_agent_attention(torch.zeros(2, 3, 3, 64), None, torch.zeros(16, dtype=torch.uint8))


def test_parameter_image_layout():
    """``pack_v2x_weights``: the size the library states, the biases at the end as float32, an operand of the first row tile where the header says; None outside fp16."""
    g = torch.Generator().manual_seed(0)
    C = 64
    wqkv, bqkv, wa, ba = torch.randn(3 * C, C, generator=g), torch.randn(3 * C, generator=g), torch.randn(C, C, generator=g), torch.randn(C, generator=g)
    img = ops.pack_v2x_weights(wqkv, bqkv, wa, ba)
    assert img.dtype == torch.uint8 and img.numel() == hip.lib().coalign_v2x_param_bytes(C)
    assert torch.equal(img[-4 * C * 4:].view(torch.float32), torch.cat([bqkv, ba]))
    tiles = 3 * C // 32
    step, tile, lane = 2, 4, 37                                                  # lane (r = 5, half = 1): W[32 tile + 5][16 step + 8 .. 16 step + 15]
    piece = img[((step * tiles + tile) * 64 + lane) * 32:][:32].view(torch.float16)
    hi, lo = ops._sp16_pair(wqkv[32 * tile + 5, 16 * step + 8:16 * step + 16])
    assert torch.equal(piece[:8], hi) and torch.equal(piece[8:], lo)
    big = wqkv.clone()
    big[3, 3] = 1e5
    assert ops.pack_v2x_weights(big, bqkv, wa, ba) is None
    with pytest.raises(ValueError):
        ops.pack_v2x_weights(torch.zeros(96, 32), torch.zeros(96), torch.zeros(32, 32), torch.zeros(32))


@pytest.fixture(scope="module")
def recorded(golden):
    g = golden("v2xvit_fuse.npz")
    m = V2XViTFusion(copy.deepcopy(ARGS_A))
    state = {str(k): torch.from_numpy(g["sd." + str(k)]) for k in g["state_keys"]}
    m.load_state_dict(state, strict=True)                                  # the reference's parameter names
    return g, m.eval()


def test_state_names_and_numels_are_the_references(recorded):
    """The fusion's and the whole model's ``state_dict`` names, order and numels equal the reference's, unread parameters included; ``relative_indices`` is no buffer."""
    g, m = recorded
    sd = m.state_dict()
    assert list(sd.keys()) == [str(k) for k in g["state_keys"]] and [v.numel() for v in sd.values()] == list(g["state_numel"])
    assert any(k.endswith("prior_feed.weight") for k in sd) and any(k.endswith("q_linears.1.weight") for k in sd) and not any("relative_indices" in k for k in sd)
    rte = V2XViTFusion(args(32, 2, 16, [4, 2, 1], [8, 16, 32], [2, 4, 8], "naive", 1, use_rte=True)).state_dict()
    assert list(rte.keys()) == [str(k) for k in g["rte_state_keys"]] and [v.numel() for v in rte.values()] == list(g["rte_state_numel"])
    assert any(k.endswith("rte.emb.emb.weight") for k in rte)
    model = build_model(builtin_config("opv2v_pointpillar_v2xvit")).state_dict()
    assert list(model.keys()) == [str(k) for k in g["model_state_keys"]] and [v.numel() for v in model.values()] == list(g["model_state_numel"])
    pw = m.fusion_net.encoder.layers[0][0].layers[0][1].fn.pwmsa[0]
    assert torch.is_tensor(pw.relative_indices) and "relative_indices" not in dict(pw.named_buffers())


def test_forward_torch_reproduces_the_reference_recordings(recorded):
    """Case A (state loaded from the fixture) and case B (dim 256, split attention; weights and map regenerated from their seeds and checked against the recorded
    checksums): ``forward`` (= ``forward_torch`` on the CPU) and ``forward_reduced`` give the reference's output within float32 round-off."""
    g, m = recorded
    x, rl, A = torch.from_numpy(g["a.x"]), torch.from_numpy(g["a.record_len"]), torch.from_numpy(g["a.affine"])
    xs, _, As = inputs(32, SEED_A + 100)
    assert torch.equal(xs, x) and torch.equal(As, A)
    with torch.no_grad():
        e1 = assert_elementwise(m(x, rl, A), torch.from_numpy(g["a.out"]), "case A: V2XViTFusion on the CPU vs the reference's recording")
        e2 = assert_elementwise(m.forward_reduced(x, rl, A), torch.from_numpy(g["a.out"]), "case A: forward_reduced (float32) vs the reference's recording")
    mb = V2XViTFusion(copy.deepcopy(ARGS_B))
    v2xvit_parameters_(mb, seed=SEED_B)
    mb.eval()
    x, rl, A = inputs(256, SEED_B + 100)
    assert np.allclose(weight_checksum(mb), g["b.weight_checksum"], rtol=1e-12, atol=0) and torch.equal(A, torch.from_numpy(g["b.affine"]))
    assert np.allclose([float(x.double().sum()), float(x.double().abs().sum())], g["b.x_checksum"], rtol=1e-12, atol=0)
    with torch.no_grad():
        e3 = assert_elementwise(mb(x, rl, A), torch.from_numpy(g["b.out"]), "case B: V2XViTFusion on the CPU vs the reference's recording")
        e4 = assert_elementwise(mb.forward_reduced(x, rl, A), torch.from_numpy(g["b.out"]), "case B: forward_reduced (float32) vs the reference's recording")
    print(f"worst error / scale: A {e1:.2e} (reduced {e2:.2e}), B {e3:.2e} (reduced {e4:.2e})")


def test_the_recorded_cases_see_every_block():
    """float64: most softmax rows of the agent attention are neither uniform nor saturated, and every block, taken out, moves the output by more than 1e-2 of its scale."""
    for a, seed, C in ((ARGS_A, SEED_A, 32), (ARGS_B, SEED_B, 256)):
        share, moved = examine(a, seed, *inputs(C, seed + 100), f"dim {C}")
        assert share > 0.5 and moved > 1e-2


def test_identity_sttf_and_roi_mask_findings(golden):
    """What the reference itself does with the identity correction matrix, at the three yamls' map shapes and one odd shape: the ROI mask IS the agent mask; STTF is
    NOT bit-identical to its input (a few 1e-5 of the scale at the yamls' shapes).  ``STTF.positions`` restates both and agrees; the restated resample equals the
    reference's output on the recorded probe bit for bit."""
    g = golden("v2xvit_fuse.npz")
    table = g["identity_findings"]
    assert [tuple(int(v) for v in r[:2]) for r in table] == [(48, 176), (48, 128), (80, 80), (7, 13)]
    for h, w, vs, ds, identical, dev, roi_is_mask in table:
        sttf = STTF({"voxel_size": [vs, vs, 4], "downsample_rate": int(ds)})
        _, ident, ones, roi = sttf.positions(int(h), int(w))
        assert ident == bool(identical) and ones == bool(roi_is_mask), (h, w)
        assert bool(roi_is_mask) and not bool(identical) and 0 < dev < 1e-4, (h, w, dev)
        assert sttf.roi_mask(int(h), int(w), "cpu", torch.float32) is None
    sttf = STTF({"voxel_size": [0.4, 0.4, 4], "downsample_rate": 4})
    probe = torch.from_numpy(g["sttf_probe_in"])
    out = sttf(probe)
    assert torch.equal(out, torch.from_numpy(g["sttf_probe_out"])) and torch.equal(out[:, 0], probe[:, 0]) and not torch.equal(out[:, 1:], probe[:, 1:])


def _double_module(a, seed):
    m = V2XViTFusion(copy.deepcopy(a))
    v2xvit_parameters_(m, seed=seed)
    return m.double().eval()


@pytest.mark.parametrize("fold_norm", [False, True], ids=["relations_and_scale", "plus_layernorm"])
@pytest.mark.parametrize("case", ["naive_depth2", "split_attn", "two_blocks_rte"])
def test_forward_reduced_equals_forward_torch_in_float64(case, fold_norm):
    """The identities are exact: in float64 ``forward_reduced`` equals ``forward_torch`` within 1e-10 of the scale, for batches with padding, one agent alone and five
    agents, with the relation / scale folds alone and with LayerNorm folded too; also with two fusion blocks per layer and RTE (which no yaml uses)."""
    a = {"naive_depth2": ARGS_A, "split_attn": ARGS_B,
         "two_blocks_rte": args(32, 2, 16, [4, 2, 1], [8, 16, 32], [2, 4, 8], "naive", 2, use_rte=True)}[case]
    a = copy.deepcopy(a)
    if case == "two_blocks_rte":
        a["transformer"]["encoder"]["num_blocks"] = 2
    C = a["transformer"]["encoder"]["cav_att_config"]["dim"]
    m = _double_module(a, seed=7)
    for groups in ([1], [3, 1], [5]) if C < 256 else ([2, 1],):
        x = torch.randn(sum(groups), C, 8, 16, dtype=torch.float64, generator=torch.Generator().manual_seed(7 + len(groups)))
        A = torch.eye(2, 3, dtype=torch.float64).repeat(len(groups), 5, 5, 1, 1)
        for b, n in enumerate(groups):
            A[b, :n, :n] = make_thetas(n, 8, 16, seed=b)
        with torch.no_grad():
            full, red = m.forward_torch(x, groups, A), m.forward_reduced(x, groups, A, fold_norm=fold_norm)
        assert full.shape == (len(groups), C, 8, 16)
        worst = float((full - red).abs().max()) / float(full.abs().max())
        assert worst <= 1e-10, (case, groups, worst)


def test_folded_layer_against_the_float64_restatement():
    """One agent-attention layer: ``agent_attention_reduced`` on the folded projection (both fold depths, R = n and R = 1) equals tests/v2xvit_reference.py's
    restatement from the unfolded parameters within 1e-10 of the scale; the folded query rows carry the scale, the key rows ``relation_att[0]``."""
    layer = PreNorm(64, HGTCavAttention(64, heads=2, dim_head=32))
    v2xvit_parameters_(layer, seed=3)
    layer = layer.double().eval()
    x = torch.randn(3, 5, 7, 64, dtype=torch.float64, generator=torch.Generator().manual_seed(3))
    ref = agent_attention_f64(layer.state_dict(), x, None, 2)
    with torch.no_grad():
        own = layer(x[None], mask=torch.ones(1, 1, 1, 1, 3))[0] + x
        assert float((own - ref).abs().max()) <= 1e-10 * float(ref.abs().max())
        for fold_norm in (False, True):
            for R in (3, 1):
                got = agent_attention_reduced(x, R, layer.norm, layer.fn, fold_norm)
                assert got.shape == (R, 5, 7, 64) and float((got - ref[:R]).abs().max()) <= 1e-10 * float(ref.abs().max()), (fold_norm, R)
        wqkv, bqkv, wa, ba = folded_agent_attention(layer.norm, layer.fn, False)
    att = layer.fn
    assert torch.allclose(wqkv[:64], att.q_linears[0].weight * 32 ** -0.5, rtol=1e-14, atol=0) and torch.equal(wa, att.a_linears[0].weight)
    assert torch.allclose(wqkv[64:96], att.relation_att[0, 0] @ att.k_linears[0].weight[:32], rtol=1e-12, atol=1e-15)
    assert torch.allclose(wqkv[128:160], att.relation_msg[0, 0].t() @ att.v_linears[0].weight[:32], rtol=1e-12, atol=1e-15)


def test_dropout_acts_in_training_mode_only():
    m = V2XViTFusion(copy.deepcopy(ARGS_A))
    v2xvit_parameters_(m, seed=1)
    x, rl, A = inputs(32, 5)
    assert sum(isinstance(k, torch.nn.Dropout) for k in m.modules()) == 2 * (1 + 3 + 2)
    with torch.no_grad():
        m.eval()
        e1, e2 = m(x, rl, A), m(x, rl, A)
        m.train()
        torch.manual_seed(0)
        t1 = m(x, rl, A)
        t2 = m(x, rl, A)
    assert torch.equal(e1, e2) and not torch.equal(t1, t2) and not torch.equal(t1, e1)
    assert not m.kernel_route(32) and not V2XViTFusion(copy.deepcopy(ARGS_B)).kernel_route(256)      # training mode


def test_kernel_route_conditions():
    mk = lambda *a, **k: V2XViTFusion(args(*a, **k)).eval()      # noqa: E731
    m = mk(256, 8, 32, [16, 8, 4], [16, 32, 64], [4, 8, 16], "split_attn", 3)
    assert m.kernel_route(256, 1) and m.kernel_route(256, 8) and m.kernel_route(256, 5, (48, 176)) and not m.kernel_route(256, 9) and not m.kernel_route(64, 2)
    m.force_torch = True
    assert not m.kernel_route(256, 2)
    assert mk(64, 2, 32, [4, 2, 1], [16, 32, 64], [2, 4, 8], "naive", 2).kernel_route(64, 3)
    assert not mk(32, 2, 16, [4, 2, 1], [8, 16, 32], [2, 4, 8], "naive", 2).kernel_route(32, 3)
    assert "4 heads x 64" in mk(256, 4, 64, [16, 8, 4], [16, 32, 64], [4, 8, 16], "split_attn", 1).kernel_shape_reason(256)
    plain = args(64, 2, 32, [4, 2, 1], [16, 32, 64], [2, 4, 8], "naive", 1)
    plain["transformer"]["encoder"]["cav_att_config"]["use_hetero"] = False
    assert not V2XViTFusion(plain).eval().kernel_route(64, 2)
    x, rl, A = inputs(32, 5)
    with pytest.raises(NotImplementedError):
        mk(32, 2, 16, [4, 2, 1], [8, 16, 32], [2, 4, 8], "naive", 1)(x, rl, A, rows=[0, 1, 2, 3])


@pytest.mark.parametrize("cfg", CONFIGS)
def test_build_model_constructs_the_baseline(cfg):
    """``build_model`` constructs ``point_pillar_baseline`` with ``fusion_method: v2xvit`` from both shipped yamls (NotImplementedError before this fusion existed);
    a config without the ``v2xvit`` section, ``when2comm`` and unknown names stay refused."""
    hypes = builtin_config(cfg)
    model = build_model(hypes)
    enc = hypes["model"]["args"]["v2xvit"]["transformer"]["encoder"]
    assert isinstance(model, PointPillarBaseline) and isinstance(model.fusion_net, V2XViTFusion)
    assert model.out_channel == enc["cav_att_config"]["dim"] and len(model.fusion_net.fusion_net.encoder.layers) == enc["depth"]
    assert model.fusion_net.kernel_shape_reason(model.out_channel, 5) is None
    h = builtin_config(cfg)
    del h["model"]["args"]["v2xvit"]
    with pytest.raises(NotImplementedError, match="v2xvit.*section"):
        build_model(h)
    for method in ("when2comm", "nothing"):
        h = builtin_config(cfg)
        h["model"]["args"]["fusion_method"] = method
        with pytest.raises(NotImplementedError):
            build_model(h)


def test_route_plan_names_the_v2xvit_route():
    """``plan(h, baselines=True)`` names the kernel route and lists the transformer's linears under what serves them; the default ``plan(h)`` reports the family as
    outside the hot path; a config off the kernel's shapes is reported with its reason."""
    from coalign_amd.routes import V2X, plan
    for cfg in CONFIGS:
        h = builtin_config(cfg)
        assert plan(h) == {"model": "point_pillar_baseline", "outside_hot_path": "model family 'point_pillar_baseline' is not part of the CoAlign hot path", "layers": {}, "fallbacks": []}
        p = plan(h, baselines=True)
        assert p["outside_hot_path"] is None and p["fusion"] == V2X and V2X.startswith("v2x_agent_attention") and "library kernels" in V2X and "fusion" not in p["fallbacks"]
        pre = "fusion_net.fusion_net.encoder."
        att = pre + "layers.0.0.layers.0.0.fn."
        for name in ("q_linears.0", "k_linears.0", "v_linears.0", "a_linears.0"):
            assert p["layers"][att + name].startswith("v2x_agent_attention") and att + name not in p["fallbacks"], name
        for name in (att + "q_linears.1", att + "a_linears.1", pre + "prior_feed"):
            assert p["layers"][name].startswith("never read") and name not in p["fallbacks"], name
        for name in (pre + "layers.0.0.layers.0.1.fn.pwmsa.0.to_qkv", pre + "layers.0.1.fn.net.0"):
            assert p["layers"][name].startswith("rocBLAS") and "torch op" in p["layers"][name] and name in p["fallbacks"], name
    odd = builtin_config("mini_pointpillar_v2xvit")
    odd["model"]["args"]["v2xvit"]["transformer"]["encoder"]["cav_att_config"].update(heads=4, dim_head=16)
    p = plan(odd, baselines=True)
    assert "fusion" in p["fallbacks"] and p["fusion"].startswith("V2XViTFusion op by op in PyTorch (") and "4 heads x 16" in p["fusion"]
    assert "fusion_net.fusion_net.encoder.layers.0.0.layers.0.0.fn.q_linears.0" in p["fallbacks"]


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
    """The mini model's forward on the CPU (op-by-op fusion; the HIP pillar encoder replaced by a stand-in canvas): the reference's three outputs, and the second agent
    is seen through the ego's affine row."""
    from coalign_amd.synthetic import fill_parameters_
    hypes = builtin_config("mini_pointpillar_v2xvit")
    model = build_model(hypes)
    fill_parameters_(model, seed=3)
    v2xvit_parameters_(model.fusion_net, seed=3)
    model.eval()
    model.pillar_vfe, model.scatter = torch.nn.Identity(), _CpuEncoder(model.scatter.ny, model.scatter.nx)
    pair = torch.eye(4, dtype=torch.float64).repeat(1, 5, 5, 1, 1)
    pair[0, 0, 1, 0, 3] = 1.3
    batch = {"processed_lidar": {"voxel_features": torch.zeros(1, 32, 4), "voxel_coords": torch.zeros(1, 4, dtype=torch.int32), "voxel_num_points": torch.ones(1, dtype=torch.int32)},
             "record_len": torch.tensor([3]), "pairwise_t_matrix": pair}
    with torch.no_grad():
        out = model(batch)
        pair2 = pair.clone()
        pair2[0, 0, 1, 0, 3] = 2.1
        out2 = model(dict(batch, pairwise_t_matrix=pair2))
    H, W = model.scatter.ny // 2, model.scatter.nx // 2
    assert out["cls_preds"].shape == (1, 2, H, W) and out["reg_preds"].shape == (1, 14, H, W) and out["dir_preds"].shape == (1, 4, H, W)
    assert all(bool(torch.isfinite(v).all()) for v in out.values()) and not torch.equal(out["reg_preds"], out2["reg_preds"])
