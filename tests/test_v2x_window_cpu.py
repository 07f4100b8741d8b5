"""V2X-ViT's pyramid window attention, host side (no GPU): the extension header include/coalign_amd_v2x_window.h against the product library and
``hip.V2X_WINDOW_SIGNATURES``, argument validation before any HIP call, the identities of ``v2xvit.window_attention_reduced`` in float64 against the module and
against the float64 restatement of tests/v2x_window_reference.py, the parameter image's layout, the examination that the yardstick SEES the block, and the route plan
with the switch on and off."""
import copy
import ctypes
import os

import pytest
import torch

import abi_headers
from coalign_amd import hip, ops, routes, v2xvit
from coalign_amd.config import builtin_config
from coalign_amd.fusion import V2XViTFusion
from coalign_amd.synthetic import v2xvit_parameters_
from coalign_amd.v2xvit import PreNorm, PyramidWindowAttention, folded_window_attention, window_attention_reduced
from v2x_window_reference import window_attention_f64
from v2xvit_reference import args

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NULL, ONE = ctypes.c_void_p(0), ctypes.c_void_p(16)      # (a non-NULL, 16-byte aligned token: none of these calls gets as far as touching memory)
HEADER = "coalign_amd_v2x_window.h"
NAMES = {"coalign_v2x_window_param_bytes", "coalign_v2x_window_workspace_bytes", "coalign_v2x_window_attention"}
WINDOWS, DIM_HEADS = [4, 8, 16], [16, 32, 64]
CONFIGS = ("opv2v_pointpillar_v2xvit", "mini_pointpillar_v2xvit")


def _param_bytes(C, fuse):
    return (C // 16) * (12 * C // 32) * 2048 + (12 * C + 1236) * 4 + ((7 * C * C + 2 * C) * 4 if fuse else 0)


def test_window_header_table_and_library_agree():
    """include/coalign_amd_v2x_window.h declares exactly ``NAMES``, the keys of ``hip.V2X_WINDOW_SIGNATURES`` (types, counts and exports: tests/test_abi_cpu.py) and
    cites the reference; build.py lists the header and the source."""
    text = open(abi_headers.path(HEADER)).read()
    assert '#include "coalign_amd.h"' in text and "mswin.py:19-121" in text and "split_attn.py:6-63" in text and "base_transformer.py:7-14" in text
    assert "v2xvit_basic.py:118-122" in text
    declared = abi_headers.declarations(HEADER)
    assert set(declared) == set(hip.V2X_WINDOW_SIGNATURES) == abi_headers.names(HEADER) == NAMES
    src = open(os.path.join(REPO, "coalign_amd", "build.py")).read()
    assert '"coalign_amd_v2x_window.h"' in src and '"v2x_window.hip"' in src


def _win(x=ONE, n=3, C=256, H=16, W=32, fuse=0, params=ONE, pbytes=None, out=ONE, ws=ONE, wbytes=None):
    L = hip.lib()
    pbytes = L.coalign_v2x_window_param_bytes(C, fuse) if pbytes is None else pbytes
    wbytes = L.coalign_v2x_window_workspace_bytes(n, C, H, W) if wbytes is None else wbytes
    return L.coalign_v2x_window_attention(x, n, C, H, W, fuse, params, pbytes, out, ws, wbytes, NULL)


def test_window_argument_validation_without_a_gpu():
    """NULL -1; a negative n, C / H / W < 1, a map of 2^31 floats, a wrong image size, a short workspace -2; n > 8, a C that is neither 256 nor (naive) 64, a fuse
    method other than 0 / 1, H or W no multiple of 16, unaligned pointers -3; n = 0 is OK without a launch: all before any HIP call (token pointers).  The size
    queries: their values at 5 x 256 x 48 x 176, 0 for every refused shape."""
    L = hip.lib()
    for arg in ("x", "params", "out", "ws"):
        assert _win(**{arg: NULL}) == -1, arg
        assert _win(**{arg: NULL}, fuse=1) == -1, arg
    for bad in (dict(n=-1), dict(C=0), dict(H=0), dict(W=0), dict(H=-16), dict(C=-64), dict(W=-32)):
        assert _win(**bad, pbytes=1, wbytes=1) == -2, bad
    for bad in (dict(n=9), dict(C=32), dict(C=128), dict(C=96), dict(C=512), dict(H=24), dict(W=40), dict(H=8), dict(C=64, fuse=1), dict(fuse=2), dict(fuse=-1), dict(C=128, fuse=1)):
        assert _win(**bad, pbytes=1, wbytes=1) == -3, bad
    assert _win(n=0) == 0 and _win(n=0, x=NULL, params=NULL, out=NULL, ws=NULL) == 0 and _win(n=0, fuse=1, x=NULL) == 0
    assert _win(n=1, C=64, H=8192, W=4096, wbytes=1 << 42) == -2                               # C H W = 2^31
    assert _win(pbytes=_param_bytes(256, 0) - 4) == -2 and _win(pbytes=_param_bytes(256, 1)) == -2 and _win(fuse=1, pbytes=_param_bytes(256, 0)) == -2
    assert _win(C=64, pbytes=_param_bytes(256, 0)) == -2
    assert _win(wbytes=L.coalign_v2x_window_workspace_bytes(3, 256, 16, 32) - 4) == -2 and _win(n=5, wbytes=L.coalign_v2x_window_workspace_bytes(3, 256, 16, 32)) == -2
    for arg, p in (("x", 20), ("out", 8), ("params", 4), ("ws", 24)):
        assert _win(**{arg: ctypes.c_void_p(p)}) == -3, arg
    for C, fuse in ((256, 0), (256, 1), (64, 0)):
        assert L.coalign_v2x_window_param_bytes(C, fuse) == _param_bytes(C, fuse), (C, fuse)
    for C, fuse in ((64, 1), (128, 0), (0, 0), (256, 2), (256, -1), (512, 1)):
        assert L.coalign_v2x_window_param_bytes(C, fuse) == 0, (C, fuse)
    n, C, HW = 5, 256, 48 * 176
    assert L.coalign_v2x_window_workspace_bytes(n, C, 48, 176) == 4 * (n * HW * 9 * C + n * HW * 3 * C + n * 3 * (HW // 16) * C + n * 3 * C) == 527170560
    assert L.coalign_v2x_window_workspace_bytes(1, 64, 16, 16) == 4 * (256 * 12 * 64 + 3 * 16 * 64 + 3 * 64)
    for bad in ((9, 256, 16, 16), (0, 256, 16, 16), (2, 48, 16, 16), (2, 128, 16, 16), (2, 256, 24, 16), (2, 256, 16, 8), (2, 256, 0, 16), (1, 64, 8192, 4096)):
        assert L.coalign_v2x_window_workspace_bytes(*bad) == 0, bad


def test_shape_predicate_and_cpu_refusal():
    ok = ops.v2x_window_shape_ok
    assert ok(256, [16, 8, 4], DIM_HEADS, WINDOWS, "split_attn", True, 5, (48, 176)) and ok(256, [16, 8, 4], DIM_HEADS, WINDOWS, "naive", True, 8)
    assert ok(64, [4, 2, 1], DIM_HEADS, WINDOWS, "naive", True, 1, (16, 16))
    assert not ok(64, [4, 2, 1], DIM_HEADS, WINDOWS, "split_attn", True) and not ok(256, [16, 8, 4], DIM_HEADS, WINDOWS, "split_attn128", True)
    assert not ok(256, [16, 8, 4], DIM_HEADS, [2, 4, 8], "naive", True) and not ok(256, [4, 8, 16], [64, 32, 16], [16, 8, 4], "naive", True)
    assert not ok(256, [8, 8, 4], DIM_HEADS, WINDOWS, "naive", True) and not ok(128, [8, 4, 2], DIM_HEADS, WINDOWS, "naive", True)
    assert not ok(256, [16, 8, 4], DIM_HEADS, WINDOWS, "naive", False) and not ok(256, [16, 8, 4], DIM_HEADS, WINDOWS, "naive", True, 9)
    assert not ok(256, [16, 8, 4], DIM_HEADS, WINDOWS, "naive", True, 0) and not ok(256, [16, 8, 4], DIM_HEADS, WINDOWS, "naive", True, 2, (24, 32))
    with pytest.raises(hip.CoalignHipError):
        ops.v2x_window_attention(torch.zeros(2, 16, 16, 64), torch.zeros(16, dtype=torch.uint8), "naive")


def _layer(C, fuse, seed, dtype=torch.float64):
    layer = PreNorm(C, PyramidWindowAttention(C, [C // d for d in DIM_HEADS], DIM_HEADS, 0.1, WINDOWS, True, fuse))
    v2xvit_parameters_(layer, seed=seed)
    return layer.to(dtype).eval()


@pytest.fixture(scope="module")
def layers64():
    return {(C, fuse): _layer(C, fuse, seed=C + 1) for C, fuse in ((64, "naive"), (256, "split_attn"))}


@pytest.mark.parametrize("hw", [(16, 32), (32, 48)], ids=["16x32", "32x48"])
@pytest.mark.parametrize("config", [(64, "naive"), (256, "split_attn")], ids=["C64_naive", "C256_split_attn"])
def test_window_attention_reduced_is_exact_in_float64(layers64, config, hw):
    """The identities are exact: in float64 ``window_attention_reduced`` equals the module's own ``x + pw(x)`` and the restatement from the unfolded parameters within
    1e-10 of the scale, for one map and three; three maps equal their single-map results (every map is on its own)."""
    C, fuse = config
    layer = layers64[config]
    for n in (1, 3):
        x = torch.randn(n, *hw, C, dtype=torch.float64, generator=torch.Generator().manual_seed(10 * n + hw[0]))
        with torch.no_grad():
            own = x + layer(x[None])[0]
            red = window_attention_reduced(x, layer.norm, layer.fn)
            ref = window_attention_f64(layer.state_dict(), x, WINDOWS, [C // d for d in DIM_HEADS], fuse)
            scale = float(own.abs().max())
            assert red.shape == own.shape == ref.shape == (n, *hw, C)
            assert float((red - own).abs().max()) <= 1e-10 * scale and float((red - ref).abs().max()) <= 1e-10 * scale and float((own - ref).abs().max()) <= 1e-10 * scale
            assert float((own - x).abs().max()) > 0.05 * scale                       # (the block is no bystander)
            if n == 3:
                assert float((red[1:2] - window_attention_reduced(x[1:2], layer.norm, layer.fn)).abs().max()) <= 1e-10 * scale


def test_folded_projection_carries_the_scales_and_layernorm():
    layer = _layer(64, "naive", seed=5)
    with torch.no_grad():
        wqkv, bqkv, wout, bout, pos = folded_window_attention(layer.norm, layer.fn)
    g, beta = layer.norm.weight, layer.norm.bias
    assert wqkv.shape == (9 * 64, 64) and bqkv.shape == (9 * 64,) and wout.shape == (3, 64, 64) and bout.shape == (3, 64) and [tuple(p.shape) for p in pos] == [(7, 7), (15, 15), (31, 31)]
    for b, att in enumerate(layer.fn.pwmsa):
        w = att.to_qkv.weight
        assert torch.allclose(wqkv[192 * b:192 * b + 64], w[:64] * g * DIM_HEADS[b] ** -0.5, rtol=1e-13, atol=0)
        assert torch.allclose(wqkv[192 * b + 64:192 * b + 192], w[64:] * g, rtol=1e-13, atol=0)
        assert torch.allclose(bqkv[192 * b + 64:192 * b + 192], w[64:] @ beta, rtol=1e-12, atol=1e-15)
        assert torch.equal(wout[b], att.to_out[0].weight) and torch.equal(bout[b], att.to_out[0].bias) and torch.equal(pos[b], att.pos_embedding)
    # the cache follows the parameters
    x = torch.randn(1, 16, 16, 64, dtype=torch.float64, generator=torch.Generator().manual_seed(0))
    with torch.no_grad():
        before = window_attention_reduced(x, layer.norm, layer.fn)
        layer.fn.pwmsa[2].pos_embedding.mul_(2.0)
        after = window_attention_reduced(x, layer.norm, layer.fn)
        assert float((after - (x + layer(x[None])[0])).abs().max()) <= 1e-10 * float(after.abs().max()) and not torch.equal(before, after)


def test_parameter_image_layout():
    """``pack_v2x_window_weights``: the size the library states, an operand of the stacked projection and of an output projection where the header says, the biases and
    the three position tables after them, the split attention's transposed float32 matrices at the end; None outside fp16."""
    L = hip.lib()
    for C, fuse in ((64, "naive"), (256, "split_attn")):
        layer = _layer(C, fuse, seed=2, dtype=torch.float32)
        sa = layer.fn.split_attn if fuse == "split_attn" else None
        split = None if sa is None else (sa.fc1.weight, sa.bn1.weight, sa.bn1.bias, sa.fc2.weight)
        with torch.no_grad():
            wqkv, bqkv, wout, bout, pos = folded_window_attention(layer.norm, layer.fn)
            img = ops.pack_v2x_window_weights(wqkv, bqkv, wout, bout, pos, split=split)
        assert img.dtype == torch.uint8 and img.numel() == L.coalign_v2x_window_param_bytes(C, ops.V2X_WINDOW_FUSE[fuse]) == _param_bytes(C, sa is not None)
        tiles = 9 * C // 32
        step, tile, lane = 2, tiles - 3, 37                                       # lane (r = 5, half = 1): W[32 tile + 5][16 step + 8 .. 16 step + 15]
        piece = img[((step * tiles + tile) * 64 + lane) * 32:][:32].view(torch.float16)
        hi, lo = ops._sp16_pair(wqkv[32 * tile + 5, 16 * step + 8:16 * step + 16])
        assert torch.equal(piece[:8], hi) and torch.equal(piece[8:], lo)
        one = (C // 16) * (C // 32) * 2048                                        # bytes of one output projection's image
        base = (C // 16) * tiles * 2048 + 2 * one                                 # branch 2's
        piece = img[base + ((1 * (C // 32) + 1) * 64 + 3) * 32:][:32].view(torch.float16)      # step 1, tile 1, lane (r = 3, half = 0)
        hi, lo = ops._sp16_pair(wout[2][32 + 3, 16:24])
        assert torch.equal(piece[:8], hi) and torch.equal(piece[8:], lo)
        fl = img[(C // 16) * (12 * C // 32) * 2048:].view(torch.float32)
        assert torch.equal(fl[:9 * C], bqkv) and torch.equal(fl[9 * C:12 * C], bout.reshape(-1))
        assert torch.equal(fl[12 * C:12 * C + 49], pos[0].reshape(-1)) and torch.equal(fl[12 * C + 49:12 * C + 274], pos[1].reshape(-1))
        assert torch.equal(fl[12 * C + 274:12 * C + 1235], pos[2].reshape(-1)) and float(fl[12 * C + 1235]) == 0.0
        assert float(fl[12 * C + 274 + 3 * 31 + 7]) == float(layer.fn.pwmsa[2].pos_embedding[3, 7].detach())
        if sa is not None:
            sp = fl[12 * C + 1236:]
            assert sp.numel() == 7 * C * C + 2 * C
            assert torch.equal(sp[:3 * C * C].view(3, C, C), wout.transpose(1, 2)) and torch.equal(sp[3 * C * C:4 * C * C].view(C, C), sa.fc1.weight.t())
            assert torch.equal(sp[4 * C * C:4 * C * C + C], sa.bn1.weight) and torch.equal(sp[4 * C * C + C:4 * C * C + 2 * C], sa.bn1.bias)
            assert torch.equal(sp[4 * C * C + 2 * C:].view(C, 3 * C), sa.fc2.weight.t())
        big = wqkv.clone()
        big[3, 3] = 1e5
        assert ops.pack_v2x_window_weights(big, bqkv, wout, bout, pos, split=split) is None
        bigo = wout.clone()
        bigo[1, 0, 0] = -7e4
        assert ops.pack_v2x_window_weights(wqkv, bqkv, bigo, bout, pos, split=split) is None
    with pytest.raises(ValueError):
        ops.pack_v2x_window_weights(torch.zeros(9 * 32, 32), torch.zeros(9 * 32), torch.zeros(3, 32, 32), torch.zeros(3, 32), pos)
    with pytest.raises(ValueError):      # (C = 64 has no split attention)
        ops.pack_v2x_window_weights(torch.zeros(9 * 64, 64), torch.zeros(9 * 64), torch.zeros(3, 64, 64), torch.zeros(3, 64), pos, split=split)


def test_the_yardstick_sees_the_block(layers64):
    """Under ``v2xvit_parameters_``, float64: most softmax rows of every branch are neither uniform nor saturated (the share rule of ``v2xvit_reference.examine`` over the rows of the three
    branches together, with 1 / keys for the uniform row; per branch the median row's top weight is at least three times the uniform one); the split weights lie strictly inside (0, 1) and are not the naive 1 / 3; transposing the relative-position index, or swapping the
    head / channel split of one branch, moves the output by far more than the GPU test's bound (1e-4)."""
    for (C, fuse), layer in layers64.items():
        heads = [C // d for d in DIM_HEADS]
        x = torch.randn(2, 32, 48, C, dtype=torch.float64, generator=torch.Generator().manual_seed(C))
        probe = {}
        ref = window_attention_f64(layer.state_dict(), x, WINDOWS, heads, fuse, probe=probe)
        scale = float(ref.abs().max())
        good = [((top > 1.0 / keys + 0.05) & (top < 0.95)).double() for keys, top in probe["top"]]
        share = float(torch.cat(good).mean())                                # over the softmax rows of the three branches together
        print(C, fuse, "share of window softmax rows neither uniform nor saturated", round(share, 3), "per branch", [round(float(g.mean()), 3) for g in good])
        assert share > 0.5, (C, share)
        for keys, top in probe["top"]:
            # per branch, free of the number of keys (the rule's margin of 0.05 above uniform is 13 x uniform for 256 keys, which a row of 256 scores of order
            # one rarely reaches): the median row's top weight is several times the uniform one, and no branch is saturated
            assert float(top.median()) > 3.0 / keys and float(top.median()) < 0.95, (C, keys, float(top.median()))
        if fuse == "split_attn":
            a = probe["a"]
            assert a.shape == (2, 3, C) and float(a.min()) > 0.0 and float(a.max()) < 1.0 and float((a - 1 / 3).abs().max()) > 0.05
            assert torch.allclose(a.sum(dim=1), torch.ones(2, C, dtype=torch.float64), rtol=0, atol=1e-12)
        moved = {"transposed position index": float((window_attention_f64(layer.state_dict(), x, WINDOWS, heads, fuse, transpose_pos=True) - ref).abs().max()) / scale}
        for b in range(3):
            if heads[b] > 1:      # (one head of all channels has no other split)
                moved[f"head / channel split of branch {b}"] = float((window_attention_f64(layer.state_dict(), x, WINDOWS, heads, fuse, channel_major_heads=b) - ref).abs().max()) / scale
        print(C, fuse, {k: round(v, 4) for k, v in moved.items()})
        assert min(moved.values()) > 100 * 1e-4, moved


def test_route_plan_with_the_switch_on_and_off(monkeypatch):
    """Off (the default): ``plan`` is what it was -- ``routes.V2X``, the window attention's linears under rocBLAS in ``fallbacks``.  On: the new constant
    ``routes.V2X_WINDOW``, which names ``v2x_window_attention`` and still says the feed-forward is torch ops; ``pwmsa.*.to_qkv``, ``pwmsa.*.to_out.0``,
    ``split_attn.fc1`` / ``fc2`` listed under the kernel and outside ``fallbacks``."""
    assert v2xvit.V2X_WINDOW_KERNELS is (os.environ.get("COALIGN_V2X_WINDOW", "0") != "0")
    monkeypatch.setattr(v2xvit, "V2X_WINDOW_KERNELS", False)
    off = {cfg: routes.plan(builtin_config(cfg), baselines=True) for cfg in CONFIGS}
    monkeypatch.setattr(v2xvit, "V2X_WINDOW_KERNELS", True)
    on = {cfg: routes.plan(builtin_config(cfg), baselines=True) for cfg in CONFIGS}
    assert "v2x_window_attention" in routes.V2X_WINDOW and routes.V2X_WINDOW.startswith("v2x_agent_attention") and "feed-forward is still torch ops" in routes.V2X_WINDOW
    pre = "fusion_net.fusion_net.encoder.layers.0."
    for cfg in CONFIGS:
        p, q = off[cfg], on[cfg]
        assert p["fusion"] == routes.V2X and q["fusion"] == routes.V2X_WINDOW and "fusion" not in q["fallbacks"]
        window = [n for n in p["layers"] if ".pwmsa." in n or ".split_attn." in n]
        assert window and all(p["layers"][n].startswith("rocBLAS") and n in p["fallbacks"] for n in window)
        assert all(q["layers"][n].startswith("v2x_window_attention") and n not in q["fallbacks"] for n in window)
        for leaf in ("0.layers.0.1.fn.pwmsa.0.to_qkv", "0.layers.0.1.fn.pwmsa.2.to_out.0") + (("0.layers.0.1.fn.split_attn.fc1", "0.layers.0.1.fn.split_attn.fc2") if cfg.startswith("opv2v") else ()):
            assert pre + leaf in window, leaf
        rest = [n for n in p["layers"] if n not in window]
        assert all(p["layers"][n] == q["layers"][n] for n in rest) and [n for n in p["fallbacks"] if n not in window] == q["fallbacks"]
        assert q["layers"][pre + "1.fn.net.0"].startswith("rocBLAS") and pre + "1.fn.net.0" in q["fallbacks"]      # the feed-forward stays a library kernel
        assert {k: v for k, v in p.items() if k not in ("fusion", "layers", "fallbacks")} == {k: v for k, v in q.items() if k not in ("fusion", "layers", "fallbacks")}


def test_window_kernel_reason():
    mk = lambda *a, **k: V2XViTFusion(args(*a, **k)).eval()      # noqa: E731
    m = mk(256, 8, 32, [16, 8, 4], DIM_HEADS, WINDOWS, "split_attn", 3)
    assert m.window_kernels is v2xvit.V2X_WINDOW_KERNELS
    m.window_kernels = False
    assert "switched off" in m.window_kernel_reason(256, (48, 176))
    m.window_kernels = True
    assert m.window_kernel_reason(256) is None and m.window_kernel_reason(256, (48, 176)) is None
    assert "multiples of 16" in m.window_kernel_reason(256, (48, 168)) and "multiples of 16" in m.window_kernel_reason(256, (8, 16))
    m64 = mk(64, 2, 32, [4, 2, 1], DIM_HEADS, WINDOWS, "naive", 2)
    m64.window_kernels = True
    assert m64.window_kernel_reason(64, (16, 32)) is None
    old = mk(64, 2, 32, [4, 2, 1], DIM_HEADS, [2, 4, 8], "naive", 2)
    old.window_kernels = True
    assert "[2, 4, 8]" in old.window_kernel_reason(64)
    heads = mk(256, 8, 32, [8, 8, 4], DIM_HEADS, WINDOWS, "naive", 1)
    heads.window_kernels = True
    assert "[8, 8, 4]" in heads.window_kernel_reason(256)
    a = args(256, 8, 32, [16, 8, 4], DIM_HEADS, WINDOWS, "naive", 1)
    a["transformer"]["encoder"]["pwindow_att_config"]["relative_pos_embedding"] = False
    norel = V2XViTFusion(a).eval()
    norel.window_kernels = True
    assert "relative_pos_embedding" in norel.window_kernel_reason(256)
    a = args(256, 8, 32, [16, 8, 4], DIM_HEADS, WINDOWS, "split_attn128", 1)
    s128 = V2XViTFusion(a).eval()
    s128.window_kernels = True
    assert "split_attn128" in s128.window_kernel_reason(256)
    # the op-by-op route and forward_reduced on the CPU do not look at the switch
    x = torch.randn(2, 64, 16, 32, generator=torch.Generator().manual_seed(1))
    A = torch.eye(2, 3, dtype=torch.float64).repeat(1, 5, 5, 1, 1)
    v2xvit_parameters_(m64, seed=1)
    with torch.no_grad():
        on = m64(x, [2], A)
        m64.window_kernels = False
        assert torch.equal(on, m64(x, [2], A))
