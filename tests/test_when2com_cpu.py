"""When2com's handshake fusion, host side (no GPU): the extension header include/coalign_amd_w2c.h against the product library and ``hip.W2C_SIGNATURES``, argument
validation before any HIP call, ``fusion.When2comFusion`` against the reference's recorded output, logits and weights (tests/golden/when2com_fuse.npz, written by
tests/golden/make_when2com_golden.py) and against the float64 restatement of tests/when2com_reference.py, the identities of ``forward_reduced``, the parameter
image's layout, the examination that the yardstick SEES the heads, and the ``point_pillar_baseline`` model: construction, names, alias, route plan."""
import copy
import ctypes
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import abi_headers
from conftest import assert_elementwise
from coalign_amd import fusion, hip, ops, routes
from coalign_amd.config import builtin_config
from coalign_amd.detector import PointPillarBaseline, build_model
from coalign_amd.fusion import When2comFusion
from coalign_amd.synthetic import when2com_parameters_
from when2com_reference import (adaptive_pool_f64, assert_sees_the_heads, parameter_checksums, score_f64, state_f64, weighted_warp_f64, when2com_fuse_f64)

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NULL, ONE = ctypes.c_void_p(0), ctypes.c_void_p(16)      # (a non-NULL, 16-byte aligned token: none of these calls gets as far as touching memory)
HEADER = "coalign_amd_w2c.h"
NAMES = {"coalign_w2c_workspace_bytes", "coalign_w2c_score", "coalign_w2c_fuse"}
CONFIGS = ("opv2v_pointpillar_when2com", "mini_pointpillar_when2com")
GOLDEN_ARGS = {"in_channels": 16, "H": 9, "W": 14, "query_size": 32, "key_size": 1024}
PARAM_BYTES = 4 * ops.W2C_PARAM_FLOATS


def test_w2c_header_table_and_library_agree():
    """include/coalign_amd_w2c.h declares exactly ``NAMES``, the keys of ``hip.W2C_SIGNATURES`` (types, counts and exports: tests/test_abi_cpu.py); every
    declaration's comment cites the reference lines it replaces; the header's image size is the one ``ops`` packs; build.py lists the header and the source."""
    text = open(abi_headers.path(HEADER)).read()
    assert '#include "coalign_amd.h"' in text
    declared = abi_headers.declarations(HEADER)
    assert set(declared) == set(hip.W2C_SIGNATURES) == abi_headers.names(HEADER) == NAMES
    comments = re.findall(r"/\*.*?\*/", text, flags=re.S)
    for name in declared:
        last = [c for c in comments if c in text[:text.index(name + "(")]][-1]
        assert "fusion_in_one.py:354-431" in last, name
    assert "when2com_fuse.py:253-270" in text and "when2com_fuse.py:342-363" in text
    floats = int(eval(re.search(r"#define COALIGN_W2C_PARAM_FLOATS (\(.*\))", text).group(1), {"__builtins__": {}}))
    assert floats == ops.W2C_PARAM_FLOATS == 2 * 256 * 4480 + 2 * 256 + 2 * (256 * 128 + 128) + 2 * (128 * 128 + 128)
    assert hip.lib().coalign_w2c_workspace_bytes() == 2 * 16 * 8 * 256 * 4
    src = open(os.path.join(REPO, "coalign_amd", "build.py")).read()
    assert '"coalign_amd_w2c.h"' in src and '"w2c_fuse.hip"' in src


def _score(key=ONE, kc=128, query=ONE, n=3, h=7, w=22, params=ONE, pbytes=PARAM_BYTES, weights=ONE, logits=NULL, ws=ONE, wbytes=None):
    L = hip.lib()
    return L.coalign_w2c_score(key, kc, query, n, h, w, params, pbytes, weights, logits, ws, L.coalign_w2c_workspace_bytes() if wbytes is None else wbytes, NULL)


def _fuse(x=ONE, n=3, C=64, H=9, W=14, theta=ONE, weights=ONE, out=ONE):
    return hip.lib().coalign_w2c_fuse(x, n, C, H, W, theta, weights, out, NULL)


def test_w2c_argument_validation_without_a_gpu():
    """NULL -1; negative counts, sizes < 1, a wrong image size, maps of 2^31 values -2; n > 8, C = 24, unaligned pointers -3; a short workspace -4; n = 0 is OK
    without a launch: all before any HIP call (token pointers, no GPU; every call here is one the entry point refuses or has nothing to do for)."""
    for arg in ("key", "query", "params", "weights", "ws"):
        assert _score(**{arg: NULL}) == -1, arg
    for arg in ("x", "theta", "weights", "out"):
        assert _fuse(**{arg: NULL}) == -1, arg
    for bad in (dict(n=-1), dict(h=0), dict(w=0), dict(h=-3), dict(pbytes=PARAM_BYTES - 4), dict(pbytes=0), dict(n=8, h=2048, w=2048), dict(kc=0), dict(kc=-128), dict(n=8, kc=256, h=1024, w=1024)):
        assert _score(**bad) == -2, bad
    for bad in (dict(n=-1), dict(C=0), dict(H=0), dict(W=-1), dict(C=-16), dict(n=8, C=64, H=2048, W=2048), dict(n=1, C=16, H=46341, W=46341)):
        assert _fuse(**bad) == -2, bad
    assert _score(n=9) == -3 and _score(kc=64) == -3 and _score(kc=136) == -3 and _fuse(n=9) == -3 and _fuse(C=24) == -3 and _fuse(C=8) == -3
    for arg, p in (("key", 8), ("query", 24), ("params", 4), ("ws", 8), ("weights", 18), ("logits", 6)):
        assert _score(**{arg: ctypes.c_void_p(p)}) == -3, arg
    for arg, p in (("x", 20), ("out", 8), ("theta", 12), ("weights", 2)):
        assert _fuse(**{arg: ctypes.c_void_p(p)}) == -3, arg
    assert _score(wbytes=hip.lib().coalign_w2c_workspace_bytes() - 1) == -4 and _score(wbytes=0) == -4
    assert _score(n=0) == 0 and _score(n=0, key=NULL, params=NULL, ws=NULL) == 0 and _fuse(n=0) == 0 and _fuse(n=0, x=NULL, out=NULL) == 0
    assert ops.w2c_shape_ok(64, 8) and ops.w2c_shape_ok(16, 1) and not ops.w2c_shape_ok(24, 2) and not ops.w2c_shape_ok(64, 9) and not ops.w2c_shape_ok(64, 0)


def test_w2c_ops_validate_before_any_hip_call():
    """CPU tensors are refused by every wrapper; ``pack_w2c_weights`` checks its shapes and lays the image out as the header says."""
    x = torch.zeros(2, 16, 3, 3).contiguous(memory_format=torch.channels_last)
    with pytest.raises(hip.CoalignHipError):
        ops.w2c_fuse(x, torch.zeros(2, 2, 3, dtype=torch.float64), torch.ones(2))
    sm = ops.SplitMap(torch.zeros(2, 8, 4, 2, 2, 8, dtype=torch.float16))
    with pytest.raises(hip.CoalignHipError):
        ops.w2c_score(sm, ops.SplitMap(sm.data[:1]), torch.zeros(ops.W2C_PARAM_FLOATS))
    with pytest.raises(TypeError):
        ops.w2c_score(x, x, torch.zeros(4))
    g = torch.Generator().manual_seed(0)
    net = lambda: (torch.randn(256, 4480, generator=g), torch.randn(256, generator=g), torch.randn(128, 256, generator=g), torch.randn(128, generator=g),      # noqa: E731
                   torch.randn(128, 128, generator=g).double(), torch.randn(128, generator=g).double())
    k, q = net(), net()
    img = ops.pack_w2c_weights(k, q)
    assert img.dtype == torch.float32 and img.numel() == ops.W2C_PARAM_FLOATS
    o = 2 * 256 * 4480
    assert torch.equal(img[:256 * 4480].view(256, 4480), k[0]) and torch.equal(img[256 * 4480:o].view(256, 4480), q[0])
    assert torch.equal(img[o:o + 256], k[1]) and torch.equal(img[o + 256:o + 512], q[1])
    o += 512
    assert torch.equal(img[o:o + 32768].view(256, 128), k[2].t()) and torch.equal(img[o + 32768:o + 32896], k[3])
    o += 32896
    assert torch.equal(img[o:o + 32768].view(256, 128), q[2].t()) and torch.equal(img[o + 32768:o + 32896], q[3])
    o += 32896
    assert torch.equal(img[o:o + 16384].view(128, 128), k[4].t().float()) and torch.equal(img[o + 16384:o + 16512], k[5].float())
    o += 16512
    assert torch.equal(img[o:o + 16384].view(128, 128), q[4].t().float()) and torch.equal(img[o + 16384:o + 16512], q[5].float()) and o + 16512 == img.numel()
    with pytest.raises(ValueError):
        ops.pack_w2c_weights(k[:5], q)
    with pytest.raises(ValueError):
        ops.pack_w2c_weights((k[0][:, :100],) + k[1:], q)


@pytest.fixture(scope="module")
def recorded(golden):
    """(fixture, the module with the regenerated parameters).  The fixture holds no parameter tensor: a checksum mismatch FAILS here."""
    g = golden("when2com_fuse.npz")
    m = When2comFusion(copy.deepcopy(GOLDEN_ARGS))
    when2com_parameters_(m, seed=int(g["seed"]))
    sums = parameter_checksums(m)
    assert list(sums.keys()) == [str(k) for k in g["param_names"]]
    assert [v[0] for v in sums.values()] == g["param_numel"].tolist()
    got = np.array([[v[1], v[2]] for v in sums.values()])
    assert np.allclose(got, g["param_sums"], rtol=1e-12, atol=1e-12), "when2com_parameters_ no longer draws the recorded parameters"
    return g, m.eval()


def test_state_dict_names_equal_the_references(recorded):
    g, m = recorded
    keys = [str(k) for k in g["state_keys"]]
    assert list(m.state_dict().keys()) == keys
    assert keys[0] == "query_key_net.conv1.cbr_unit.0.weight" and keys[-1] == "attention_net.linear_out.bias" and len(keys) == 67
    assert (m.feat_H, m.feat_W, m.query_size, m.key_size, m.in_channels) == (9, 14, 32, 1024, 16)


def test_forward_torch_reproduces_the_reference(recorded):
    """Output, per-frame logits and weights of the reference itself; float32 against float32 of another build of the same operations."""
    g, m = recorded
    x, A, groups = torch.from_numpy(g["x"]), torch.from_numpy(g["affine"]), g["record_len"].tolist()
    details = []
    with torch.no_grad():
        out = m(x, torch.tensor(groups), A)
        again = m.forward_torch(x, groups, A, details)
    assert torch.equal(out, again) and out.shape == (2, 16, 9, 14)
    assert_elementwise(out, torch.from_numpy(g["out"]), "forward_torch vs the reference's output", rtol=1e-5, floor=1e-6)
    logits, weights = torch.cat([d[0] for d in details]), torch.cat([d[1] for d in details])
    assert_elementwise(logits, torch.from_numpy(g["logits"]), "logits vs the reference's", rtol=1e-5, floor=1e-6)
    assert_elementwise(weights, torch.from_numpy(g["weights"]), "weights vs the reference's", rtol=1e-5, floor=1e-6)
    assert float(weights[3]) == 1.0                                                         # the one-agent frame
    with pytest.raises(NotImplementedError):
        m(x, groups, A, rows=[0, 1, 2, 3])


def test_float64_restatement_agrees_with_the_reference(recorded):
    g, m = recorded
    x, A = torch.from_numpy(g["x"]), torch.from_numpy(g["affine"])
    sd = state_f64(m.state_dict())
    off = 0
    for b, n in enumerate(g["record_len"].tolist()):
        ref, logits, w = when2com_fuse_f64(sd, x[off:off + n], A[b, 0, :n])
        assert_elementwise(torch.from_numpy(g["out"][b]), ref, f"the reference's output vs float64, frame {b}")
        assert_elementwise(torch.from_numpy(g["weights"][off:off + n]), w, f"the reference's weights vs float64, frame {b}")
        off += n


def _as_f64(m):
    return copy.deepcopy(m).double()


def test_forward_reduced_is_exact_in_float64(recorded):
    """Identities (a) - (d) together: ``forward_reduced`` against ``forward_torch`` in float64 to 1e-10 of the scale, logits and weights included."""
    g, m = recorded
    m64 = _as_f64(m)
    x, A, groups = torch.from_numpy(g["x"]).double(), torch.from_numpy(g["affine"]), g["record_len"].tolist()
    dt, dr = [], []
    with torch.no_grad():
        want, got = m64.forward_torch(x, groups, A, dt), m64.forward_reduced(x, groups, A, dr)
    scale = float(want.abs().max())
    assert float((got - want).abs().max()) <= 1e-10 * scale
    assert float((dr[0][0] - dt[0][0]).abs().max()) <= 1e-10 * float(dt[0][0].abs().max()) and float((dr[0][1] - dt[0][1]).abs().max()) <= 1e-10
    assert dr[1][0] is None and float(dr[1][1]) == 1.0                                      # (d): the one-agent frame's heads are not run


def test_each_identity_in_float64(recorded):
    g, m = recorded
    m64 = _as_f64(m)
    gen = torch.Generator().manual_seed(3)
    with torch.no_grad():
        # (a) BatchNorm and the bias folded into weight and shift, stride kept
        for block, cin, stride in ((m64.query_key_net.conv1, 16, 1), (m64.query_key_net.conv3, 256, 2), (m64.key_net.conv1, 256, 2)):
            x = torch.randn(2, cin, 7, 9, generator=gen, dtype=torch.float64)
            w, s, st = block.folded()
            want = block(x)
            assert st == stride and float((F.relu(F.conv2d(x, w, s, stride=st, padding=1)) - want).abs().max()) <= 1e-10 * float(want.abs().max())
        # (b) the two linears as one 128 x 128 matrix: key_size and query_size vanish
        for which, net, lin in (("key", m64.key_net, m64.attention_net.linear_feat), ("query", m64.query_net, m64.attention_net.linear_context)):
            T, tb = m64.folded_tail(which)
            h = torch.randn(5, 128, generator=gen, dtype=torch.float64)
            want = lin(net.fc[4](h))
            assert T.shape == (128, 128) and T.dtype == torch.float64 and float((h @ T.t() + tb - want).abs().max()) <= 1e-10 * float(want.abs().max())
        # (c) the query block on the ego's map alone = row 0 of the query block on every map
        maps = torch.randn(3, 256, 6, 8, generator=gen, dtype=torch.float64).abs()
        assert torch.equal(m64.query_net(maps[:1]), m64.query_net(maps)[:1]) or float((m64.query_net(maps[:1]) - m64.query_net(maps)[:1]).abs().max()) <= 1e-10 * float(m64.query_net(maps).abs().max())
        # (d) a softmax over one logit is 1 whatever the logit
        x = torch.randn(1, 16, 9, 14, generator=gen, dtype=torch.float64)
        th = torch.tensor([[[1.0, 0.1, 0.2], [-0.1, 1.0, 0.05]]], dtype=torch.float64)
        fused, logits, w = m64.frame_torch(x, th)
        assert float(w) == 1.0 and float((fused - F.grid_sample(x, F.affine_grid(th, [1, 16, 9, 14], align_corners=False), align_corners=False)).abs().max()) <= 1e-10
    assert float((adaptive_pool_f64(maps) - F.adaptive_avg_pool2d(maps, (5, 7))).abs().max()) <= 1e-12        # the restatement's bins are PyTorch's


def test_the_yardstick_sees_the_heads(recorded):
    """On the parity inputs every frame with n >= 2 has softmax weights in [0.02, 0.98], one at least 0.05 off 1 / n.  A head that flattened the pooled map with the
    channel fastest, or pooled to a transposed (7 x 5) grid, moves the float64 output by more than 1e-2 of its scale -- measured here: 1.5e-1 and 1.0 of the
    scale, over a thousand times the parity bound -- so the comparison cannot pass such a kernel."""
    g, m = recorded
    x, A = torch.from_numpy(g["x"]), torch.from_numpy(g["affine"])
    sd = state_f64(m.state_dict())
    w = torch.from_numpy(g["weights"])
    assert_sees_the_heads(w[:3], "frame 0")
    ref, _, w0 = when2com_fuse_f64(sd, x[:3], A[0, 0, :3])
    scale = float(ref.abs().max())
    for order in ("ijc", "cji"):
        other, _, w1 = when2com_fuse_f64(sd, x[:3], A[0, 0, :3], order=order)
        moved = float((other - ref).abs().max()) / scale
        print(f"flatten order {order}: output moves by {moved:.3e} of the scale, weights {w0.tolist()} -> {w1.tolist()}")
        assert moved > 1e-2, (order, moved)


def test_score_restatement_matches_the_module_heads(recorded):
    """``score_f64`` (the yardstick of the score kernel's GPU test) on given conv1 outputs equals the module's own heads in float64, at map sizes below, at and above
    the pool grid."""
    g, m = recorded
    m64, sd = _as_f64(m), state_f64(m.state_dict())
    gen = torch.Generator().manual_seed(5)
    with torch.no_grad():
        for h, w in ((2, 2), (2, 4), (5, 7), (7, 22), (13, 44)):
            key, query = torch.randn(3, 128, h, w, generator=gen, dtype=torch.float64).abs(), torch.randn(1, 128, h, w, generator=gen, dtype=torch.float64).abs()
            keys, q = m64.key_net.fc(m64.key_net.avgp(key).view(-1, 4480)).unsqueeze(0), m64.query_net.fc(m64.query_net.avgp(query).view(-1, 4480)).unsqueeze(0)
            want = m64.attention_net.logits(q, keys).reshape(-1)
            logits, wts = score_f64(sd, key, query)
            assert float((logits - want).abs().max()) <= 1e-10 * float(want.abs().max()) and float((wts - torch.softmax(want, 0)).abs().max()) <= 1e-10
    assert float((weighted_warp_f64(torch.ones(2, 1, 3, 3), torch.tensor([[[1.0, 0, 0], [0, 1.0, 0]]] * 2, dtype=torch.float64), torch.tensor([0.25, 0.75])) - 1).abs().max()) <= 1e-6      # (float32 sampling positions: the identity row is not exact)


@pytest.mark.parametrize("cfg", CONFIGS)
def test_build_model_constructs_the_baseline(cfg, golden):
    """``build_model`` constructs ``point_pillar_baseline`` with ``fusion_method: when2comm`` from both new yamls (NotImplementedError before this fusion existed);
    with the ``when2comm`` section deleted it is still refused, by a message naming the section; unknown names stay refused.  The full-size model's ``state_dict``
    names and sizes equal the reference's."""
    hypes = builtin_config(cfg)
    model = build_model(hypes)
    sect = hypes["model"]["args"]["when2comm"]
    assert isinstance(model, PointPillarBaseline) and isinstance(model.fusion_net, When2comFusion)
    assert model.fusion_net.in_channels == sect["in_channels"] == model.out_channel and (sect["query_size"], sect["key_size"]) == (32, 1024)
    assert "this project's choice" in open(os.path.join(REPO, "coalign_amd", "configs", cfg + ".yaml")).read()
    if cfg.startswith("opv2v"):
        g = golden("when2com_fuse.npz")
        sd = model.state_dict()
        assert list(sd.keys()) == [str(k) for k in g["model_state_keys"]]
        assert [v.numel() for v in sd.values()] == g["model_state_numel"].tolist()
    h = builtin_config(cfg)
    del h["model"]["args"]["when2comm"]
    with pytest.raises(NotImplementedError, match="when2comm.*section"):
        build_model(h)
    h = builtin_config(cfg)
    h["model"]["args"]["fusion_method"] = "nothing"
    with pytest.raises(NotImplementedError):
        build_model(h)


def test_opencood_alias_resolves():
    from coalign_amd import opencood_compat
    opencood_compat.install()
    import importlib
    mod = importlib.import_module("opencood.models.fuse_modules.fusion_in_one")
    assert mod.When2commFusion is fusion.When2comFusion is When2comFusion


@pytest.mark.parametrize("cfg", CONFIGS)
def test_route_plan(cfg):
    """``plan(hypes, baselines=True)``: the six convolutions under conv3x3_sp / conv3x3_sp_s2, the fc stacks and attention linears under w2c_score, ``linear_out`` as
    never read, nothing of the fusion under ``fallbacks``; without the SplitMap arithmetic the op-by-op route with its reason.  The default ``plan(hypes)`` still
    reports the family as outside the hot path."""
    hypes = builtin_config(cfg)
    p = routes.plan(hypes, baselines=True)
    L = p["layers"]
    assert p["fusion"] == routes.W2C and "fusion" not in p["fallbacks"] and not [n for n in p["fallbacks"] if n.startswith("fusion_net.")]
    for name in ("query_key_net.conv1", "query_key_net.conv2", "query_key_net.conv4"):
        assert L[f"fusion_net.{name}.cbr_unit.0"].startswith(routes.SP), name
    for name in ("query_key_net.conv3", "query_key_net.conv5", "key_net.conv1", "query_net.conv1"):
        assert L[f"fusion_net.{name}.cbr_unit.0"].startswith(routes.SP_S2), name
    for name in ("key_net.fc.0", "key_net.fc.2", "key_net.fc.4", "query_net.fc.0", "query_net.fc.2", "query_net.fc.4", "attention_net.linear_feat", "attention_net.linear_context"):
        assert L["fusion_net." + name].startswith(routes.W2C_SCORE), name
    assert L["fusion_net.attention_net.linear_out"] == routes.W2C_UNREAD
    counts = routes.summary(p)["routes"]
    assert counts["w2c_score"] == 8 and counts["conv3x3_sp_s2"] >= 4 and counts["never read"] == 1
    q = routes.plan(hypes, terms=3, baselines=True)
    assert q["fusion"].startswith(routes.W2C_TORCH) and "SplitMap arithmetic" in q["fusion"] and "fusion" in q["fallbacks"]
    assert "fusion_net.key_net.fc.0" in q["fallbacks"] and "fusion_net.query_key_net.conv1.cbr_unit.0" in q["fallbacks"]
    assert "fusion_net.attention_net.linear_out" not in q["fallbacks"]
    d = routes.plan(hypes)
    assert d["outside_hot_path"] is not None and d["layers"] == {}


def test_kernel_route_decision():
    m = When2comFusion(copy.deepcopy(GOLDEN_ARGS)).eval()
    assert m.kernel_route(16, 1) and m.kernel_route(16, 8) and m.kernel_shape_reason(16, 3) is None
    assert not m.kernel_route(16, 9) and "agents" in m.kernel_shape_reason(16, 9)
    assert not m.kernel_route(32, 2) and "channels" in m.kernel_shape_reason(32, 2)
    assert not m.kernel_route(16, 2, terms=3) and "SplitMap" in m.kernel_shape_reason(16, 2, terms=3)
    m.force_torch = True
    assert not m.kernel_route(16, 2)
    m.force_torch = False
    assert not m.train().kernel_route(16, 2)
    m24 = When2comFusion(dict(GOLDEN_ARGS, in_channels=24)).eval()
    assert not m24.kernel_route(24, 2) and "C % 16" in m24.kernel_shape_reason(24, 2)
