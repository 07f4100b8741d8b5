"""V2X-ViT's three kernels at their range, softmax and tile limits on the GPU: ``ops.v2x_agent_attention`` (csrc/v2x_attn.hip), ``ops.v2x_window_attention``
(csrc/v2x_window.hip) and ``ops.v2x_feed_forward`` (csrc/v2x_ffn.hip) on the cases of tests/v2x_limit_cases.py against the float64 restatements of
tests/v2xvit_reference.py, tests/v2x_window_reference.py and tests/v2x_ffn_reference.py.

The bound is ``token_bound <= 1``: the project's element-wise bound (rtol 1e-4, floor 1e-5) with the floor's scale taken per token.  Every kernel case first holds the
float32 op-by-op layer, on the same GPU and the same inputs, to that bound (tests/test_v2x_limits_cpu.py holds it to half of it on the CPU); both errors and their
ratio are printed.  One call per kernel goes through the C ABI into NaN-poisoned output and workspace buffers: every output element must be written, and the bits must
equal the ``ops`` call (nothing of the result depends on what the buffers held).  No bound is widened."""
import copy

import pytest
import torch

import v2x_limit_cases as lc
from conftest import assert_elementwise
from coalign_amd import hip, ops
from coalign_amd.fusion import V2XViTFusion
from coalign_amd.synthetic import v2xvit_parameters_
from coalign_amd.v2xvit import folded_agent_attention, folded_feed_forward, folded_window_attention
from v2v_reference import make_thetas
from v2xvit_reference import args

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ARGS_W64 = args(64, 2, 32, [4, 2, 1], lc.DIM_HEADS, lc.WINDOWS, "naive", 2)
_ON_GPU = {}


def _placed(kind, key, variant):
    """-> (the float32 layer on the CPU, a copy on the GPU, its parameter image on the GPU), made once per layer."""
    k = (kind, key, variant)
    if k not in _ON_GPU:
        if kind == "agent":
            layer = lc.agent_layer(key, variant)
            with torch.no_grad():
                image = ops.pack_v2x_weights(*folded_agent_attention(layer.norm, layer.fn, True))
        elif kind == "window":
            layer = lc.window_layer(key, variant)
            pw = layer.fn
            sa = pw.split_attn if pw.fuse_mehod == "split_attn" else None
            with torch.no_grad():
                image = ops.pack_v2x_window_weights(*folded_window_attention(layer.norm, pw), split=None if sa is None else (sa.fc1.weight, sa.bn1.weight, sa.bn1.bias, sa.fc2.weight))
        else:
            layer = lc.ffn_layer(*key, variant)
            with torch.no_grad():
                image = ops.pack_v2x_ffn_weights(*folded_feed_forward(layer.norm, layer.fn))
        assert image is not None, k
        _ON_GPU[k] = (layer, copy.deepcopy(layer).to(DEV), image.to(DEV))
    return _ON_GPU[k]


def _report(what, e_torch, e_kernel):
    print(f"{what}: of the per-token bound, kernel {e_kernel:.3f}, float32 op-by-op layer {e_torch:.3f}, ratio {e_kernel / max(e_torch, 1e-30):.2f}")
    assert e_torch <= 1.0, (what, "float32 op-by-op layer", e_torch)
    assert e_kernel <= 1.0, (what, "kernel", e_kernel)


# ---- agent attention -------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("group", lc.AGENT_GROUPS)
@pytest.mark.parametrize("C", [64, 256])
def test_agent_attention_against_the_float64_layer(C, group):
    """counts: every n = 1 .. 8 with R in {n, 1} on 5 x 7, in place and warped.  maps: 1 x 1, 1 x 31, 32 x 1, 1 x 33, 33 x 1 at n = 3.  planted: LayerNorm's edge
    tokens in the ego's and in a sender's map.  scales: eight agents from 1e-3 to 1e3.  q16: saturated softmax rows.  edge: the value projection's static bound at
    0.98 x 65504 with the aligned token (n = 1: o = v')."""
    worst = 0.0
    for case in lc.agent_cases(C, group):
        layer, gpu_layer, image = _placed("agent", C, case.variant)
        ref = lc.agent_reference(layer, case)
        e_torch = lc.token_bound(lc.agent_op_by_op(gpu_layer, lc.agent_warped_f64(case).float().to(DEV)), ref)
        xd = case.x.to(DEV)
        th = None if case.theta is None else case.theta.to(DEV)
        for R in case.receivers:
            got = ops.v2x_agent_attention(xd, th, image, receivers=R)
            assert got.shape == (R,) + tuple(case.x.shape[1:])
            e_kernel = lc.token_bound(got, ref[:R])
            _report(f"agent attention C={C} {case.name} R={R}", e_torch, e_kernel)
            worst = max(worst, e_kernel)
    print(f"agent attention C={C} {group}: worst kernel error {worst:.3f} of the per-token bound")


@pytest.mark.parametrize("C", [64, 256])
def test_agent_attention_writes_every_element_whatever_the_buffers_held(C):
    """n = 3 on 5 x 7 (a partial tile) under a warp, R = 3 and R = 1, through the C ABI: output and workspace are all NaN before the call."""
    _, _, image = _placed("agent", C, "base")
    L = hip.lib()
    n, H, W = 3, 5, 7
    x = torch.randn(n, H, W, C, generator=torch.Generator().manual_seed(C)).to(DEV)
    th = make_thetas(n, H, W, seed=n)[0].to(DEV).contiguous()
    for R in (3, 1):
        want = ops.v2x_agent_attention(x, th, image, receivers=R)
        out = torch.full((R, H, W, C), float("nan"), device=DEV)
        ws_bytes = int(L.coalign_v2x_workspace_bytes(n, C, H, W))
        ws = torch.full((ws_bytes // 4,), float("nan"), device=DEV)
        rc = L.coalign_v2x_agent_attention(ops._ptr(x), n, R, C, H, W, ops._ptr(th), ops._ptr(image), image.numel(), ops._ptr(out), ops._ptr(ws), ws_bytes, ops._stream())
        torch.cuda.synchronize()
        assert rc == 0
        assert bool(torch.isfinite(out).all()) and torch.equal(out, want), (C, R)


# ---- window attention ------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("config,group", lc.WINDOW_PARAMS)
def test_window_attention_against_the_float64_layer(config, group):
    """counts: n in {3, 4, 6, 7} on 16 x 16.  columns: 48 x 16 and 16 x 48 (one column, one row of 16-windows).  planted: LayerNorm's edge tokens.  q12: saturated
    rows under the online softmax.  pos30: a position table that dominates the scores.  fc2x40 (split attention): nearly one-hot branch weights.  edge: every
    branch's value projection at 0.98 x 65504 with windows of aligned tokens (o_b = v_b)."""
    C, fuse = lc.WINDOW_CONFIGS[config]
    worst = 0.0
    for case in lc.window_cases(config, group):
        layer, gpu_layer, image = _placed("window", config, case.variant)
        xd = case.x.to(DEV)
        ref = lc.window_reference(layer, config, xd)                  # (float64 torch ops on the GPU)
        e_torch = lc.token_bound(lc.window_op_by_op(gpu_layer, xd), ref)
        got = ops.v2x_window_attention(xd, image, fuse)
        assert got.shape == xd.shape
        e_kernel = lc.token_bound(got, ref)
        _report(f"window attention {config} {case.name}", e_torch, e_kernel)
        worst = max(worst, e_kernel)
    print(f"window attention {config} {group}: worst kernel error {worst:.3f} of the per-token bound")


@pytest.mark.parametrize("config", list(lc.WINDOW_CONFIGS))
def test_window_attention_writes_every_element_whatever_the_buffers_held(config):
    """n = 3 on 16 x 32 through the C ABI: the output and all four parts of the workspace (projections, attention outputs, partial sums, branch weights) are NaN
    before the call."""
    C, fuse = lc.WINDOW_CONFIGS[config]
    _, _, image = _placed("window", config, "base")
    L = hip.lib()
    n, H, W = 3, 16, 32
    x = torch.randn(n, H, W, C, generator=torch.Generator().manual_seed(C)).to(DEV)
    want = ops.v2x_window_attention(x, image, fuse)
    out = torch.full((n, H, W, C), float("nan"), device=DEV)
    ws_bytes = int(L.coalign_v2x_window_workspace_bytes(n, C, H, W))
    ws = torch.full((ws_bytes // 4,), float("nan"), device=DEV)
    rc = L.coalign_v2x_window_attention(ops._ptr(x), n, C, H, W, ops.V2X_WINDOW_FUSE[fuse], ops._ptr(image), image.numel(), ops._ptr(out), ops._ptr(ws), ws_bytes, ops._stream())
    torch.cuda.synchronize()
    assert rc == 0
    assert bool(torch.isfinite(out).all()) and torch.equal(out, want), config


# ---- feed-forward ----------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("group", lc.FFN_GROUPS)
@pytest.mark.parametrize("shape", lc.FFN_SHAPES, ids=[f"C{C}_M{M}" for C, M in lc.FFN_SHAPES])
def test_feed_forward_against_the_float64_layer(shape, group):
    """(C, M): one row tile for four wavefronts (M = 32), the last M below and the first above the 64 KB of dynamic LDS at C = 64 (416 | 448; at C = 256 224 here,
    256 in tests/test_v2x_ffn_gpu.py), the largest tile of the <64> instantiation (512).  tokens: 31, 32, 33, 64.  planted: LayerNorm's edge tokens.  edge: the first
    linear's static bound at 0.98 x 65504 with the aligned token and its negative, in the first and in the partial tile."""
    C, M = shape
    worst = 0.0
    for case in lc.ffn_cases(C, M, group):
        layer, gpu_layer, image = _placed("ffn", shape, case.variant)
        xd = case.x.to(DEV)
        ref = lc.ffn_reference(layer, xd)
        e_torch = lc.token_bound(lc.ffn_op_by_op(gpu_layer, xd), ref)
        got = ops.v2x_feed_forward(xd, image)
        assert got.shape == xd.shape
        e_kernel = lc.token_bound(got, ref)
        _report(f"feed-forward C={C} M={M} {case.name}", e_torch, e_kernel)
        worst = max(worst, e_kernel)
    print(f"feed-forward C={C} M={M} {group}: worst kernel error {worst:.3f} of the per-token bound")


@pytest.mark.parametrize("shape", [(64, 448), (256, 224)], ids=["C64_M448", "C256_M224"])
def test_feed_forward_writes_every_element_whatever_the_buffer_held(shape):
    """33 tokens (a partial tile) through the C ABI into an output of NaN."""
    C, M = shape
    _, _, image = _placed("ffn", shape, "base")
    L = hip.lib()
    x = torch.randn(33, C, generator=torch.Generator().manual_seed(M)).to(DEV)
    want = ops.v2x_feed_forward(x, image)
    out = torch.full((33, C), float("nan"), device=DEV)
    rc = L.coalign_v2x_feed_forward(ops._ptr(x), 33, C, M, ops._ptr(image), image.numel(), ops._ptr(out), ops._stream())
    torch.cuda.synchronize()
    assert rc == 0
    assert bool(torch.isfinite(out).all()) and torch.equal(out, want), shape


# ---- the module --------------------------------------------------------------------------------------------------------------------------------------------------------
def test_module_keeps_the_torch_route_for_an_unpackable_agent_attention_layer():
    """``V2XViTFusion``, C = 64, all three kernel switches on, the value projection of the second agent-attention layer at a static bound of 1.05 x 65504: the reason
    is reported, ``ops.v2x_agent_attention`` is not called, the output equals the float64 route; the same module before the change runs the kernels."""
    m = V2XViTFusion(copy.deepcopy(ARGS_W64))
    v2xvit_parameters_(m, seed=64)
    m = m.eval().to(DEV)
    m.window_kernels = m.ffn_kernels = True
    x = torch.randn(4, 64, 16, 32, generator=torch.Generator().manual_seed(108))
    rl = torch.tensor([3, 1])
    A = torch.zeros(2, 5, 5, 2, 3, dtype=torch.float64)
    A[..., 0, 0] = A[..., 1, 1] = 1.0
    A[0, :3, :3] = make_thetas(3, 16, 32, seed=108)

    def run():
        seen = []
        real = ops.v2x_agent_attention
        ops.v2x_agent_attention = lambda *a_, **k_: (seen.append(1), real(*a_, **k_))[1]
        try:
            with torch.no_grad():
                return m(x.to(DEV), rl, A.to(DEV)), len(seen)
        finally:
            ops.v2x_agent_attention = real
    assert m.kernel_weight_reason() is None and m.window_kernel_reason(64, (16, 32)) is None and m.ffn_kernel_reason(64) is None
    _, calls = run()
    assert calls == 4                                                 # two frames x two layers
    lc.scale_agent_values_(m.fusion_net.encoder.layers[1][0].layers[0][0], lc.OUTSIDE)
    reason = m.kernel_weight_reason()
    assert reason is not None and "or the static bound of an attention output" in reason and m.packed() is None
    assert m.window_kernel_reason(64, (16, 32)) is None and m.ffn_kernel_reason(64) is None and m.kernel_route(64, 3, (16, 32))
    line, fallback, _ = m.plan_fusion(64)
    assert fallback and reason in line
    got, calls = run()
    assert calls == 0
    with torch.no_grad():
        ref = copy.deepcopy(m).cpu().double().forward_torch(x.double(), rl, A)
    e = assert_elementwise(got, ref, "the torch route of a module with an unpackable agent-attention layer vs its float64 route")
    print(f"module, one agent-attention layer at 1.05 x 65504: torch route at {e:.2e} of the scale from float64; reason: {reason}")
