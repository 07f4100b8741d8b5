"""V2X-ViT's feed-forward block, host side (no GPU): the extension header include/coalign_amd_v2x_ffn.h against the product library and ``hip.V2X_FFN_SIGNATURES``,
argument refusals before any HIP call, the identity of ``v2xvit.feed_forward_reduced`` in float64 against the module and against the float64 restatement of
tests/v2x_ffn_reference.py, the parameter image decoded lane by lane against a numpy statement of the layout, the packer's static range guarantee, the examination
that the yardstick SEES the activation, the switch, and the route plan with the switch on and off."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import abi_headers
from conftest import assert_elementwise
from coalign_amd import build, hip, ops, routes, v2xvit
from coalign_amd.config import builtin_config
from coalign_amd.fusion import V2XViTFusion
from coalign_amd.synthetic import v2xvit_parameters_
from coalign_amd.v2xvit import FeedForward, PreNorm, feed_forward_reduced, folded_feed_forward
from v2v_reference import student_t
from v2x_ffn_reference import feed_forward_f64
from v2xvit_reference import args

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NULL, ONE, TWO = ctypes.c_void_p(0), ctypes.c_void_p(16), ctypes.c_void_p(1 << 20)      # (non-NULL, 16-byte aligned tokens: none of these calls gets as far as touching memory)
HEADER = "coalign_amd_v2x_ffn.h"
NAMES = {"coalign_v2x_ffn_param_bytes", "coalign_v2x_feed_forward"}
SHAPES = ((64, 64), (64, 256), (256, 256), (256, 512))
WINDOWS, DIM_HEADS = [4, 8, 16], [16, 32, 64]
CONFIGS = ("opv2v_pointpillar_v2xvit", "mini_pointpillar_v2xvit")


def _param_bytes(C, M):
    return 2 * (C // 16) * (M // 32) * 2048 + 4 * (M + C)


def test_ffn_header_table_and_library_agree():
    """The header declares exactly ``NAMES``, the keys of ``hip.V2X_FFN_SIGNATURES`` (types, counts and exports: tests/test_abi_cpu.py); every declaration cites the
    reference lines it replaces; build.py lists the source."""
    text = open(abi_headers.path(HEADER)).read()
    assert '#include "coalign_amd.h"' in text
    declared = abi_headers.declarations(HEADER)
    assert set(declared) == set(hip.V2X_FFN_SIGNATURES) == abi_headers.names(HEADER) == NAMES
    comments = re.findall(r"/\*.*?\*/", text, flags=re.S)
    for name in declared:
        last = [c for c in comments if c in text[:text.index(name + "(")]][-1]
        assert "base_transformer.py:7-14" in last and "base_transformer.py:17-29" in last, name
    assert "v2xvit_basic.py:179" in [c for c in comments if c in text[:text.index("coalign_v2x_feed_forward(")]][-1]
    assert '"v2x_ffn.hip"' in open(os.path.join(REPO, "coalign_amd", "build.py")).read() and "v2x_ffn.hip" in build.SOURCES
    assert int(re.search(r"#define COALIGN_V2X_FFN_MAX_HIDDEN (\d+)", text).group(1)) == ops.V2X_FFN_MAX_HIDDEN


def _ffn(x=ONE, tokens=175, C=256, M=256, params=ONE, pbytes=None, out=TWO):
    L = hip.lib()
    pbytes = L.coalign_v2x_ffn_param_bytes(C, M) if pbytes is None else pbytes
    return L.coalign_v2x_feed_forward(x, tokens, C, M, params, pbytes, out, NULL)


def test_ffn_argument_refusals_without_a_gpu():
    """NULL and misaligned pointers -1; negative sizes, 2^31 values, a wrong image size -2; C = 128, M = 48, M = 544 and their like, out == x -3; tokens = 0 is OK
    without a launch: all before any HIP call (token pointers).  The size query: its values, 0 for every refused pair."""
    L = hip.lib()
    for arg in ("x", "params", "out"):
        assert _ffn(**{arg: NULL}) == -1, arg
    for arg, p in (("x", 20), ("out", 8), ("params", 4)):
        assert _ffn(**{arg: ctypes.c_void_p(p)}) == -1, arg
    for bad in (dict(tokens=-1), dict(C=0), dict(M=0), dict(C=-64), dict(M=-32)):
        assert _ffn(**bad, pbytes=1) == -2, bad
    for bad in (dict(C=128), dict(C=32), dict(C=512), dict(M=48), dict(M=544), dict(M=16), dict(M=100), dict(C=128, M=48)):
        assert _ffn(**bad, pbytes=1) == -3, bad
    assert _ffn(out=ONE) == -3 and _ffn(C=64, M=96, out=ONE) == -3                             # out == x
    assert _ffn(tokens=0) == 0 and _ffn(tokens=0, x=NULL, params=NULL, out=NULL) == 0 and _ffn(tokens=0, out=ONE) == 0
    assert _ffn(tokens=1 << 23) == -2 and _ffn(tokens=(1 << 23) - 1, pbytes=1) == -2           # 2^31 values; one token fewer gets as far as the image's size
    assert _ffn(tokens=1 << 22, C=64, M=512) == -2 and _ffn(tokens=1 << 22, C=256, M=512) == -2
    assert _ffn(pbytes=_param_bytes(256, 256) - 4) == -2 and _ffn(pbytes=_param_bytes(256, 512)) == -2 and _ffn(C=64, M=64, pbytes=_param_bytes(256, 256)) == -2
    for C in (64, 256):
        for M in range(32, 513, 32):
            assert L.coalign_v2x_ffn_param_bytes(C, M) == _param_bytes(C, M), (C, M)
    assert L.coalign_v2x_ffn_param_bytes(256, 256) == 512 * 1024 + 2048                        # both matrices as sp16 operands: 512 KB
    for C, M in ((128, 64), (0, 64), (64, 0), (64, 48), (64, 544), (256, 16), (-64, 64), (64, -32), (512, 512)):
        assert L.coalign_v2x_ffn_param_bytes(C, M) == 0, (C, M)
    assert all(ops.v2x_ffn_shape_ok(C, M) for C, M in SHAPES) and ops.v2x_ffn_shape_ok(64, 96)
    assert not any(ops.v2x_ffn_shape_ok(C, M) for C, M in ((128, 64), (64, 48), (64, 544), (256, 0), (64, 16)))
    with pytest.raises(hip.CoalignHipError):
        ops.v2x_feed_forward(torch.zeros(4, 64), torch.zeros(16, dtype=torch.uint8))


def _layer(C, M, seed, dtype=torch.float64):
    layer = PreNorm(C, FeedForward(C, M, 0.3))
    v2xvit_parameters_(layer, seed=seed)
    return layer.to(dtype).eval()


@pytest.fixture(scope="module")
def layers64():
    return {(C, M): _layer(C, M, seed=C + M) for C, M in SHAPES}


@pytest.mark.parametrize("shape", [(64, 64), (256, 256)], ids=["C64_M64", "C256_M256"])
def test_feed_forward_reduced_is_exact_in_float64(layers64, shape):
    """The fold is exact: in float64 ``feed_forward_reduced`` equals the module's own ``x + ff(x)`` and the restatement from the unfolded parameters within 1e-10 of the
    scale; the cache follows the parameters."""
    C, M = shape
    layer = _layer(C, M, seed=7)
    x = torch.randn(3, 5, 7, C, dtype=torch.float64, generator=torch.Generator().manual_seed(C))
    with torch.no_grad():
        own = x + layer(x)
        red = feed_forward_reduced(x, layer.norm, layer.fn)
        ref = feed_forward_f64(layer.state_dict(), x)
        scale = float(own.abs().max())
        assert red.shape == own.shape == ref.shape == x.shape
        assert float((red - own).abs().max()) <= 1e-10 * scale and float((red - ref).abs().max()) <= 1e-10 * scale
        assert float((own - x).abs().max()) > 0.05 * scale                       # (the block is no bystander)
        w1, b1, w2, b2 = folded_feed_forward(layer.norm, layer.fn)
        assert w1.dtype == torch.float64 and w1.shape == (M, C) and b1.shape == (M,) and w2.shape == (C, M) and b2.shape == (C,)
        assert torch.allclose(w1, layer.fn.net[0].weight * layer.norm.weight, rtol=1e-14, atol=0)
        assert torch.allclose(b1, layer.fn.net[0].weight @ layer.norm.bias + layer.fn.net[0].bias, rtol=1e-12, atol=1e-15)
        layer.norm.weight.mul_(1.5)
        after = feed_forward_reduced(x, layer.norm, layer.fn)
        assert float((after - (x + layer(x))).abs().max()) <= 1e-10 * float(after.abs().max()) and not torch.equal(red, after)


def _decode(img, R, K):
    """The header's layout restated in numpy: bytes of [K / 16 steps][R / 32 row tiles][64 lanes][8 h | 8 l] fp16 -> W [R, K] float64, lane (r = lane & 31,
    half = lane >> 5) of (step, tile) holding W[32 tile + r][16 step + 8 half + j] as h + l 2^-10."""
    raw = np.frombuffer(img.tobytes(), dtype=np.float16).astype(np.float64)
    tiles = R // 32
    W = np.full((R, K), np.nan)
    for s in range(K // 16):
        for t in range(tiles):
            for lane in range(64):
                piece = raw[((s * tiles + t) * 64 + lane) * 16:][:16]
                r, half = lane & 31, lane >> 5
                W[32 * t + r, 16 * s + 8 * half:16 * s + 8 * half + 8] = piece[:8] + piece[8:] * 2.0 ** -10
    return W


@pytest.mark.parametrize("shape", [(64, 96), (256, 256)], ids=["C64_M96", "C256_M256"])
def test_parameter_image_decodes_to_the_folded_weights(layers64, shape):
    """``pack_v2x_ffn_weights``: the size the library states; W1' then W2 in the lane order of the header, every element within 22 bits of the folded float64 weight;
    b1' and b2 after them as float32."""
    C, M = shape
    layer = _layer(C, M, seed=3)
    w1, b1, w2, b2 = folded_feed_forward(layer.norm, layer.fn)
    img = ops.pack_v2x_ffn_weights(w1, b1, w2, b2)
    assert img.dtype == torch.uint8 and img.numel() == hip.lib().coalign_v2x_ffn_param_bytes(C, M) == _param_bytes(C, M)
    raw = img.numpy()
    one = (C // 16) * (M // 32) * 2048
    for got, want in ((_decode(raw[:one], M, C), w1.float().double().numpy()), (_decode(raw[one:2 * one], C, M), w2.float().double().numpy())):      # (the packer's float32 input)
        assert not np.isnan(got).any()                                           # every element has its lane
        assert (np.abs(got - want) <= 2.0 ** -22 * np.abs(want) + 2.0 ** -34).all()
        assert np.abs(got - want).max() > 0                                      # (22 bits, not 53)
    fl = torch.from_numpy(raw[2 * one:].copy()).view(torch.float32)
    assert torch.equal(fl[:M], b1.float()) and torch.equal(fl[M:], b2.float()) and fl.numel() == M + C


def test_packer_refuses_what_could_leave_the_fp16_range():
    """None for a folded weight of 1e5 in either matrix, and for a row of W1' whose static bound ||W1'_r||_2 sqrt(C) + |b1'_r| reaches 65504 although every
    weight is far inside the range -- through the weights or through the bias alone; a row just inside is packed."""
    layer = _layer(64, 64, seed=5)
    w1, b1, w2, b2 = folded_feed_forward(layer.norm, layer.fn)
    assert ops.pack_v2x_ffn_weights(w1, b1, w2, b2) is not None
    big = w1.clone(); big[3, 3] = 1e5
    assert ops.pack_v2x_ffn_weights(big, b1, w2, b2) is None
    big = w2.clone(); big[0, 5] = -1e5
    assert ops.pack_v2x_ffn_weights(w1, b1, big, b2) is None
    row = w1.clone(); row[7] = 1024.0                                           # ||row||_2 sqrt(C) = 1024 * 8 * 8 = 65536
    assert ops.pack_v2x_ffn_weights(row, b1, w2, b2) is None
    row[7] = 1000.0                                                             # 64000 + |b1'_7| < 65504
    assert ops.pack_v2x_ffn_weights(row, b1, w2, b2) is not None
    bias = b1.clone(); bias[9] = -65504.0
    assert ops.pack_v2x_ffn_weights(w1, bias, w2, b2) is None
    nan = w2.clone(); nan[1, 1] = float("nan")
    assert ops.pack_v2x_ffn_weights(w1, b1, nan, b2) is None
    with pytest.raises(ValueError):
        ops.pack_v2x_ffn_weights(torch.zeros(48, 64), torch.zeros(48), torch.zeros(64, 48), torch.zeros(64))
    with pytest.raises(ValueError):
        ops.pack_v2x_ffn_weights(torch.zeros(64, 128), torch.zeros(64), torch.zeros(128, 64), torch.zeros(128))
    # the module keeps the torch ops for such a layer
    m = V2XViTFusion(args(64, 2, 32, [4, 2, 1], DIM_HEADS, WINDOWS, "naive", 2)).eval()
    v2xvit_parameters_(m, seed=1)
    m.ffn_kernels = True
    assert m.ffn_kernel_reason(64) is None and len(m.packed_ffn()) == 2
    with torch.no_grad():
        m.fusion_net.encoder.layers[1][1].fn.net[0].weight[0, 0] = 1e5
    assert m.packed_ffn() is None and "fp16 range" in m.ffn_kernel_reason(64)


@pytest.mark.parametrize("shape", SHAPES, ids=[f"C{C}_M{M}" for C, M in SHAPES])
def test_the_yardstick_sees_the_activation(layers64, shape):
    """175 tokens, float64, under ``v2xvit_parameters_``: the pre-activations reach past |z| = 3 with most inside (-3, 3) (the non-linear part of GELU is exercised);
    the block moves the output by 15 - 100 % of its scale at input scales 1 and 1e-2 (least for Student-t maps at scale 1, whose tails set the scale) and by under
    1 % at 1e2; the float32 op-by-op layer holds the GPU test's bound everywhere (at most 6.8e-7 of the scale); a restatement with the tanh approximation of GELU
    fails that bound at input scale 1e-2 (1.6e-4 .. 2.2e-4 of the scale against a bound of at most 1.1e-4), one with ReLU fails it by 0.02 .. 0.2 of the scale."""
    C, M = shape
    layer = layers64[shape]
    state = layer.state_dict()
    f32 = _layer(C, M, seed=C + M, dtype=torch.float32)
    for k, (kind, scale) in enumerate((("gauss", 1.0), ("student", 1.0), ("gauss", 1e-2), ("student", 1e2), ("gauss", 1e2), ("student", 1e-2))):
        x = (torch.randn((5, 5, 7, C), generator=torch.Generator().manual_seed(50 + k)) * scale) if kind == "gauss" else student_t((5, 5, 7, C), 50 + k, scale=scale)
        probe = {}
        ref = feed_forward_f64(state, x, probe=probe)
        s = float(ref.abs().max())
        z = probe["z"].abs()
        moved = float((ref - x.double()).abs().max()) / s
        with torch.no_grad():
            e32 = assert_elementwise(f32(x) + x, ref, f"{shape} {kind} x{scale}: float32 op-by-op layer vs float64")
        print(f"{shape} {kind} x{scale}: max |z| {float(z.max()):.2f}, inside (-3, 3) {float((z < 3).double().mean()):.4f}, block moves {moved:.3f} of the scale, float32 layer {e32:.2e}")
        assert float(z.max()) > 3.0 and float((z < 3).double().mean()) > 0.9
        assert moved > 0.1 if scale <= 1.0 else moved < 0.01
        relu = float((feed_forward_f64(state, x, act="relu") - ref).abs().max()) / s
        if scale <= 1.0:
            print(f"    ReLU restatement: {relu:.3f} of the scale")
            assert relu > 1000 * 1e-5, relu                                      # a thousand times the bound's floor
            with pytest.raises(AssertionError):
                assert_elementwise(feed_forward_f64(state, x, act="relu"), ref)
        if scale == 1e-2:
            tanh = feed_forward_f64(state, x, act="gelu_tanh")
            print(f"    tanh-GELU restatement: {float((tanh - ref).abs().max()) / s:.2e} of the scale")
            with pytest.raises(AssertionError):
                assert_elementwise(tanh, ref)


def test_switch_follows_the_environment_and_defaults_to_off(monkeypatch):
    src = open(os.path.join(REPO, "coalign_amd", "v2xvit.py")).read()
    assert 'V2X_FFN_KERNELS = os.environ.get("COALIGN_V2X_FFN", "0") != "0"' in src                # unset: "0" -> off
    assert v2xvit.V2X_FFN_KERNELS is (os.environ.get("COALIGN_V2X_FFN", "0") != "0")
    a = args(64, 2, 32, [4, 2, 1], DIM_HEADS, WINDOWS, "naive", 2)
    for value in (False, True):
        monkeypatch.setattr(v2xvit, "V2X_FFN_KERNELS", value)
        m = V2XViTFusion(a).eval()
        assert m.ffn_kernels is value and (m.ffn_kernel_reason(64) is None) is value
    monkeypatch.setattr(v2xvit, "V2X_FFN_KERNELS", False)
    m = V2XViTFusion(a).eval()
    assert "switched off" in m.ffn_kernel_reason(64)
    m.ffn_kernels = True
    assert m.ffn_kernel_reason(64) is None and "128 channels" in m.ffn_kernel_reason(128)
    a48 = args(64, 2, 32, [4, 2, 1], DIM_HEADS, WINDOWS, "naive", 2)
    a48["transformer"]["encoder"]["feed_forward"]["mlp_dim"] = 48
    m48 = V2XViTFusion(a48).eval()
    m48.ffn_kernels = True
    assert "48" in m48.ffn_kernel_reason(64)
    # the op-by-op route on the CPU does not look at the switch
    x = torch.randn(2, 64, 16, 32, generator=torch.Generator().manual_seed(1))
    A = torch.eye(2, 3, dtype=torch.float64).repeat(1, 5, 5, 1, 1)
    v2xvit_parameters_(m, seed=1)
    with torch.no_grad():
        on = m(x, [2], A)
        m.ffn_kernels = False
        assert torch.equal(on, m(x, [2], A))


def test_route_plan_with_the_switch_on_and_off(monkeypatch):
    """Off (the default): ``plan`` returns the existing constants -- ``routes.V2X``, or ``routes.V2X_WINDOW`` with the window switch -- and lists both feed-forward
    linears under rocBLAS in ``fallbacks``.  On: ``routes.V2X_FFN`` / ``routes.V2X_WINDOW_FFN``, the ``.net.0`` / ``.net.3`` linears named under ``v2x_feed_forward``
    and outside ``fallbacks``; every other line as it was."""
    plans = {}
    for window in (False, True):
        for ffn in (False, True):
            monkeypatch.setattr(v2xvit, "V2X_WINDOW_KERNELS", window)
            monkeypatch.setattr(v2xvit, "V2X_FFN_KERNELS", ffn)
            plans[window, ffn] = {cfg: routes.plan(builtin_config(cfg), baselines=True) for cfg in CONFIGS}
    assert routes.V2X_FFN.startswith("v2x_agent_attention + v2x_feed_forward") and "torch ops" in routes.V2X_FFN
    assert all(k in routes.V2X_WINDOW_FFN for k in ("v2x_agent_attention", "v2x_window_attention", "v2x_feed_forward")) and "torch ops" not in routes.V2X_WINDOW_FFN
    assert len({routes.V2X, routes.V2X_WINDOW, routes.V2X_FFN, routes.V2X_WINDOW_FFN}) == 4
    pre = "fusion_net.fusion_net.encoder.layers."
    for cfg in CONFIGS:
        for window in (False, True):
            p, q = plans[window, False][cfg], plans[window, True][cfg]
            assert p["fusion"] == (routes.V2X_WINDOW if window else routes.V2X) and q["fusion"] == (routes.V2X_WINDOW_FFN if window else routes.V2X_FFN)
            assert "fusion" not in q["fallbacks"]
            ffn = [n for n in p["layers"] if ".fn.net." in n]
            depth = len(ffn) // 2
            assert len(ffn) == 2 * depth and depth >= 1 and all(n.startswith(pre) and n.rsplit(".", 1)[-1] in ("0", "3") for n in ffn)
            assert all(p["layers"][n].startswith("rocBLAS") and n in p["fallbacks"] for n in ffn)
            assert all(q["layers"][n].startswith("v2x_feed_forward") and n not in q["fallbacks"] for n in ffn)
            assert pre + "0.1.fn.net.0" in ffn and pre + "0.1.fn.net.3" in ffn
            rest = [n for n in p["layers"] if n not in ffn]
            assert all(p["layers"][n] == q["layers"][n] for n in rest) and [n for n in p["fallbacks"] if n not in ffn] == q["fallbacks"]
            assert {k: v for k, v in p.items() if k not in ("fusion", "layers", "fallbacks")} == {k: v for k, v in q.items() if k not in ("fusion", "layers", "fallbacks")}
        if cfg.startswith("opv2v"):      # both switches: no linear of an encoder layer is left to the library
            left = [n for n in plans[True, True][cfg]["fallbacks"] if n.startswith(pre)]
            assert left == [], left
