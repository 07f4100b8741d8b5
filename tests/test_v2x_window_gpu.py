"""V2X-ViT's pyramid window attention on the GPU (csrc/v2x_window.hip through the C ABI): ``ops.v2x_window_attention`` against the float64 restatement of one layer
(tests/v2x_window_reference.py) on one 16-window and on 2 x 3 of them, one to eight maps, naive and split attention, across input scales; the independence of the
maps and the fixed reduction order bit for bit; its argument contract on real buffers; ``V2XViTFusion`` with ``window_kernels`` set against float64, under a graph
capture, and on a geometry the kernel refuses; the model (``mini_pointpillar_v2xvit.yaml``) eagerly and through ``FramePipeline``.

The bound is ``assert_elementwise`` at its defaults (rtol 1e-4, floor 1e-5 of the scale).  Every kernel case first holds the float32 op-by-op layer, on the same
GPU and the same inputs, to that bound: the inputs never ask of the kernel what float32 itself cannot do.  Both errors are printed.  (On exactly these shapes,
scales and weights the float32 op-by-op layer on the CPU is within 8.3e-7 of the scale.  The block moves the output by about 20 % of its scale at input scale 1,
by 100 % at 1e-2 and by less than 1 % at 1e2: there the case tests the residual path and LayerNorm's range, not the attention.)"""
import copy

import pytest
import torch

from conftest import assert_elementwise
from coalign_amd import hip, ops
from coalign_amd.config import builtin_config
from coalign_amd.detector import build_model, to_device
from coalign_amd.fusion import V2XViTFusion
from coalign_amd.inference import inference_intermediate_fusion
from coalign_amd.pipeline import FramePipeline
from coalign_amd.postprocess import build_postprocessor
from coalign_amd.synthetic import fill_parameters_, make_frame, v2xvit_parameters_
from coalign_amd.v2xvit import PreNorm, PyramidWindowAttention, folded_window_attention
from v2v_reference import make_thetas, student_t
from v2x_window_reference import window_attention_f64
from v2xvit_reference import args

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
WINDOWS, DIM_HEADS = [4, 8, 16], [16, 32, 64]
CONFIGS = {"C64_naive": (64, "naive"), "C256_naive": (256, "naive"), "C256_split_attn": (256, "split_attn")}
ARGS_A64 = args(64, 2, 32, [4, 2, 1], DIM_HEADS, [2, 4, 8], "naive", 2)          # windows the kernel does not take
ARGS_W64 = args(64, 2, 32, [4, 2, 1], DIM_HEADS, WINDOWS, "naive", 2)
ARGS_W256 = args(256, 8, 32, [16, 8, 4], DIM_HEADS, WINDOWS, "split_attn", 1)


def _heads(C):
    return [C // d for d in DIM_HEADS]


def _image(layer):
    pw = layer.fn
    sa = pw.split_attn if pw.fuse_mehod == "split_attn" else None
    with torch.no_grad():
        return ops.pack_v2x_window_weights(*folded_window_attention(layer.norm, pw), split=None if sa is None else (sa.fc1.weight, sa.bn1.weight, sa.bn1.bias, sa.fc2.weight))


@pytest.fixture(scope="module")
def layers():
    """config -> (PreNorm(PyramidWindowAttention) on the GPU in float32, its state, its parameter image on the GPU), made once."""
    out = {}
    for name, (C, fuse) in CONFIGS.items():
        layer = PreNorm(C, PyramidWindowAttention(C, _heads(C), DIM_HEADS, 0.1, WINDOWS, True, fuse))
        v2xvit_parameters_(layer, seed=C + len(fuse))
        layer.eval()
        out[name] = (copy.deepcopy(layer).to(DEV), {k: v.clone() for k, v in layer.state_dict().items()}, _image(layer).to(DEV))
    return out


def _maps(kind, scale, shape, seed):
    if kind == "gauss":
        return torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale
    return student_t(shape, seed, scale=scale)


@pytest.mark.parametrize("n", [1, 2, 5, 8])
@pytest.mark.parametrize("hw", [(16, 16), (32, 48)], ids=["16x16", "32x48"])
@pytest.mark.parametrize("config", list(CONFIGS))
def test_kernel_against_the_float64_layer(layers, config, hw, n):
    """16 x 16 is one 16-window, four 8-windows and sixteen 4-windows; 32 x 48 is 2 x 3 of the big windows: unequal counts in the two directions, windows on every
    edge.  Gaussian and Student-t maps at scales 1e-2, 1, 1e2.  The float64 yardstick runs on the GPU too (float64 torch ops)."""
    H, W = hw
    C, fuse = CONFIGS[config]
    gpu_layer, state, image = layers[config]
    worst_kernel = worst_torch = 0.0
    for k, (kind, scale) in enumerate((("gauss", 1.0), ("student", 1.0), ("gauss", 1e-2), ("student", 1e2), ("gauss", 1e2), ("student", 1e-2))):
        xd = _maps(kind, scale, (n, H, W, C), 1000 * n + 10 * H + k).to(DEV)
        ref = window_attention_f64(state, xd, WINDOWS, _heads(C), fuse)
        what = f"{config} {H}x{W} n={n} {kind} x{scale}"
        with torch.no_grad():
            plain = gpu_layer(xd[None])[0] + xd
        e_torch = assert_elementwise(plain, ref, what + ": float32 op-by-op layer vs float64")
        got = ops.v2x_window_attention(xd, image, fuse)
        assert got.shape == (n, H, W, C)
        e_kernel = assert_elementwise(got, ref, what + ": kernel vs float64")
        print(f"{what}: error / scale, kernel {e_kernel:.3e}, float32 op-by-op layer {e_torch:.3e}")
        worst_kernel, worst_torch = max(worst_kernel, e_kernel), max(worst_torch, e_torch)
    print(f"{config} {H}x{W} n={n}: worst error / scale, kernel {worst_kernel:.3e}, float32 op-by-op layer {worst_torch:.3e}")


def test_maps_are_independent_and_the_reduction_order_is_fixed(layers):
    """fuse = 0: the result for five maps equals the five single-map results bit for bit.  fuse = 1: two calls on the same input are equal bit for bit (the pooled sums
    are reduced in a fixed order), and a map's result does not depend on its neighbours either."""
    for config, H, W in (("C64_naive", 32, 48), ("C256_naive", 16, 16)):
        C, fuse = CONFIGS[config]
        x = torch.randn(5, H, W, C, generator=torch.Generator().manual_seed(3)).to(DEV)
        whole = ops.v2x_window_attention(x, layers[config][2], fuse)
        for i in range(5):
            assert torch.equal(whole[i:i + 1], ops.v2x_window_attention(x[i:i + 1].contiguous(), layers[config][2], fuse)), (config, i)
    image = layers["C256_split_attn"][2]
    x = torch.randn(5, 32, 48, 256, generator=torch.Generator().manual_seed(4)).to(DEV)
    first, second = ops.v2x_window_attention(x, image, "split_attn"), ops.v2x_window_attention(x, image, "split_attn")
    assert torch.equal(first, second)
    assert torch.equal(first[2:3], ops.v2x_window_attention(x[2:3].contiguous(), image, "split_attn"))


def test_argument_contract_on_real_buffers(layers):
    """Every status code before a launch, with real device buffers: a canary output stays untouched by every refused call; n = 0 returns OK without a launch."""
    image = layers["C64_naive"][2]
    image256 = layers["C256_split_attn"][2]
    L = hip.lib()
    n, H, W, C = 3, 16, 32, 64
    x = torch.randn(n, H, W, C, device=DEV)
    out = torch.full((n, H, W, C), 7.0, device=DEV)
    ws = torch.empty(L.coalign_v2x_window_workspace_bytes(n, 256, H, W) // 4, device=DEV)      # (large enough for C = 256 too)
    wb64 = L.coalign_v2x_window_workspace_bytes(n, C, H, W)
    stream = ops._stream()

    def call(x_=x, n_=n, C_=C, H_=H, W_=W, fuse_=0, image_=image, pb=None, out_=out, ws_=ws, wb=None):
        return L.coalign_v2x_window_attention(ops._ptr(x_), n_, C_, H_, W_, fuse_, ops._ptr(image_), image.numel() if pb is None else pb, ops._ptr(out_), ops._ptr(ws_),
                                              ws.numel() * 4 if wb is None else wb, stream)
    assert call(x_=None) == -1 and call(image_=None) == -1 and call(out_=None) == -1 and call(ws_=None) == -1
    assert call(n_=-1) == -2 and call(H_=0) == -2 and call(W_=-16) == -2 and call(pb=image.numel() - 32) == -2 and call(wb=wb64 - 4) == -2
    assert call(pb=image256.numel(), image_=image256) == -2                                     # the C = 256 split-attention image for a C = 64 call
    assert call(n_=9) == -3 and call(C_=128) == -3 and call(H_=24) == -3 and call(W_=40) == -3 and call(fuse_=1) == -3 and call(fuse_=2) == -3
    assert call(x_=x.view(-1)[1:]) == -3 and call(out_=out.view(-1)[2:]) == -3
    assert call(n_=0) == 0 and call(n_=0, x_=None, out_=None) == 0
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    assert call() == 0
    torch.cuda.synchronize()
    assert bool((out != 7.0).any()) and bool(torch.isfinite(out).all())
    with pytest.raises(ValueError):
        ops.v2x_window_attention(torch.randn(2, 24, 32, 64, device=DEV), image, "naive")
    with pytest.raises(ValueError):
        ops.v2x_window_attention(torch.randn(2, 16, 16, 64, device=DEV), image, "split_attn")
    with pytest.raises(ValueError):
        ops.v2x_window_attention(torch.randn(2, 16, 16, 128, device=DEV), image, "naive")


def _float64_fusion(m, x, rl, A):
    """The module's own op-by-op route in float64 on the CPU: tests/test_v2xvit_cpu.py pins that route to the reference's recordings."""
    with torch.no_grad():
        return copy.deepcopy(m).cpu().double().forward_torch(x.double(), rl, A)


# The warps of the module cases.  Whether float32 itself holds the bound on a 16 x 32 batch depends on the warps: where a sampling position lands within float32's
# resolution of a pixel border, a border token of nearly zero norm changes and LayerNorm amplifies that.  On the CPU, float32 ``forward_torch`` against float64 over
# the seeds 100 .. 111 of ``make_thetas`` is either 1e-6 .. 8e-6 of the scale (seven seeds) or 2e-5 .. 7e-5 with elements outside the bound (five seeds), for all
# three modules alike; 108 is of the first kind for all three (worst element at 0.13 / 0.07 / 0.08 of its bound).  Chosen by float32's own error, not by the kernel's.
BATCH_SEED = 108


def _batch(C, seed, H=16, W=32):
    """record_len [3, 1] padded to five agents on an H x W map: a shift, a rotation, an agent half outside (make_thetas)."""
    x = torch.randn(4, C, H, W, generator=torch.Generator().manual_seed(seed))
    A = torch.zeros(2, 5, 5, 2, 3, dtype=torch.float64)
    A[..., 0, 0] = A[..., 1, 1] = 1.0
    A[0, :3, :3] = make_thetas(3, H, W, seed=seed)
    return x, torch.tensor([3, 1]), A


@pytest.mark.parametrize("case", ["W64_naive_depth2", "W256_split_attn", "A64_windows_2_4_8"])
def test_module_window_kernels_against_float64(case):
    """``V2XViTFusion`` with ``window_kernels`` set on a 16 x 32 batch: against its own op-by-op route in float64, the float32 op-by-op route on the same GPU held to the
    bound first.  With windows [2, 4, 8] the module reports a reason, runs the torch ops for the window attention and still equals the float64 route."""
    a, seed, C = {"W64_naive_depth2": (ARGS_W64, 64, 64), "W256_split_attn": (ARGS_W256, 41, 256), "A64_windows_2_4_8": (ARGS_A64, 64, 64)}[case]
    m = V2XViTFusion(copy.deepcopy(a))
    v2xvit_parameters_(m, seed=seed)
    m = m.eval().to(DEV)
    assert m.window_kernels is False and "switched off" in m.window_kernel_reason(C, (16, 32))
    m.window_kernels = True
    x, rl, A = _batch(C, BATCH_SEED)
    ref = _float64_fusion(m, x, rl, A)
    assert m.kernel_route(C, 3, (16, 32))
    reason = m.window_kernel_reason(C, (16, 32))
    if case.startswith("A64"):
        assert reason is not None and "[2, 4, 8]" in reason
    else:
        assert reason is None and "multiples of 16" in m.window_kernel_reason(C, (8, 16))
    seen = []
    real = ops.v2x_window_attention
    ops.v2x_window_attention = lambda *a_, **k_: (seen.append(1), real(*a_, **k_))[1]
    try:
        with torch.no_grad():
            got = m(x.to(DEV), rl, A.to(DEV))
    finally:
        ops.v2x_window_attention = real
    assert len(seen) == (0 if reason is not None else 2 * len(m.fusion_net.encoder.layers))      # two frames, one fusion block per layer
    with torch.no_grad():
        m.force_torch = True
        plain = m(x.to(DEV), rl, A.to(DEV))
        m.force_torch = False
    e_torch = assert_elementwise(plain, ref, case + ": float32 op-by-op route vs float64")
    e_kernel = assert_elementwise(got, ref, case + ": kernel route with window kernels vs float64")
    print(f"{case}: worst error / scale, kernel route {e_kernel:.3e}, float32 op-by-op route {e_torch:.3e}")


def test_forward_under_graph_capture():
    m = V2XViTFusion(copy.deepcopy(ARGS_W64))
    v2xvit_parameters_(m, seed=9)
    m = m.eval().to(DEV)
    m.window_kernels = True
    x, _, A = _batch(64, 9)
    x, A, groups = x[:3].contiguous(memory_format=torch.channels_last).to(DEV), A[:1].to(DEV), [3]
    assert m.window_kernel_reason(64, (16, 32)) is None
    with torch.no_grad():
        m(x, groups, A)                                                     # (parameter images packed, grids and indices placed: before the capture)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = m(x, groups, A)
        for seed in (1, 2):
            fresh = torch.randn(3, 64, 16, 32, generator=torch.Generator().manual_seed(seed)).to(DEV)
            x.copy_(fresh)
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(out, m(fresh.contiguous(memory_format=torch.channels_last), groups, A)), seed


def test_model_heads_and_detections():
    """``mini_pointpillar_v2xvit.yaml`` (16 x 32 map, windows 4 / 8 / 16, naive), 3 agents, the switch on: the heads against the same model with its fusion on the
    op-by-op route; detections of ``inference_intermediate_fusion`` equal those of ``FramePipeline`` (eager lanes and captured frames), bit for bit."""
    h = builtin_config("mini_pointpillar_v2xvit")
    model = build_model(h)
    fill_parameters_(model, seed=0, cls_bias=-1.0)
    v2xvit_parameters_(model.fusion_net, seed=2)
    with torch.no_grad():
        model.reg_head.weight.mul_(0.01); model.reg_head.bias.zero_(); model.cls_head.weight.mul_(0.05)
    model = model.to(DEV).eval()
    model.fusion_net.window_kernels = True
    anchors = torch.from_numpy(build_postprocessor(h["postprocess"], False).generate_anchor_box())
    frames = [to_device(make_frame(h, 3, pillars_per_agent=150, seed=40 + i, spread_xy=(4.0, 2.0), spread_yaw=45.0), DEV) for i in range(4)]
    assert model.fusion_net.kernel_route(model.out_channel, 3, (16, 32)) and model.fusion_net.window_kernel_reason(model.out_channel, (16, 32)) is None
    with torch.no_grad():
        got = model(frames[0])
        model.fusion_net.force_torch = True
        want = model(frames[0])
        model.fusion_net.force_torch = False
    for k in ("cls_preds", "reg_preds", "dir_preds"):
        print(k, assert_elementwise(got[k], want[k], f"{k}: kernel-route fusion with window kernels vs op-by-op fusion"))
    pp = build_postprocessor(h["postprocess"], False)
    eye = torch.eye(4, device=DEV)
    want = []
    for f in frames:
        r = inference_intermediate_fusion({"ego": dict(f, anchor_box=anchors.to(DEV), transformation_matrix=eye)}, model, pp)
        want.append((r["pred_box_tensor"], r["pred_score"]))
    assert sum(0 if b is None else b.shape[0] for b, _ in want) > 0
    for graph in (False, True):
        pipe = FramePipeline(model, build_postprocessor(h["postprocess"], False), anchors, lanes=2, result_lag=1, graph=graph, device=DEV)
        try:
            got = pipe.run(frames)
        finally:
            pipe.close()
        for i, ((gb, gs), (wb, ws)) in enumerate(zip(got, want)):
            assert (gb is None) == (wb is None), (graph, i)
            if wb is not None:
                assert torch.equal(gb, wb) and torch.equal(gs, ws), (graph, i)
