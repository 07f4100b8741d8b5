"""V2X-ViT's feed-forward block on the GPU (csrc/v2x_ffn.hip through the C ABI): ``ops.v2x_feed_forward`` against the float64 restatement of one layer
(tests/v2x_ffn_reference.py) at every (C, mlp_dim) corner of the kernel, on 1, 35, 175 and 1024 tokens, across input scales; the independence of the tokens and of
the view bit for bit; its argument contract on real buffers; ``V2XViTFusion`` with ``ffn_kernels`` set (alone and with ``window_kernels``) against float64, on a
hidden width the kernel refuses, and under a graph capture; the model (``mini_pointpillar_v2xvit.yaml``) eagerly and through ``FramePipeline``.

The bound is ``assert_elementwise`` at its defaults (rtol 1e-4, floor 1e-5 of the scale), as for the two sibling kernels.  Every kernel case first holds the float32
op-by-op layer, on the same GPU and the same inputs, to that bound: the inputs never ask of the kernel what float32 itself cannot do.  Both errors are printed.
(tests/test_v2x_ffn_cpu.py examines the yardstick on the CPU, 175 tokens at (C, mlp_dim) up to (256, 512) and these scales: the float32 op-by-op layer is within 6.8e-7
of the scale of float64; pre-activations reach |z| = 3.9 .. 4.9 with 99.6 % inside (-3, 3); the block moves the output by 15 - 100 % of its scale at input scales 1 and
1e-2 and by less than 1 % at 1e2: there the case tests the residual path and LayerNorm's range.)  Measured on the MI355X: DESIGN.md section 8g-2."""
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
from coalign_amd.v2xvit import FeedForward, PreNorm, folded_feed_forward
from v2v_reference import make_thetas, student_t
from v2x_ffn_reference import feed_forward_f64
from v2xvit_reference import args

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
WINDOWS, DIM_HEADS = [4, 8, 16], [16, 32, 64]
CONFIGS = {"C64_M64": (64, 64), "C64_M96": (64, 96), "C256_M256": (256, 256), "C256_M512": (256, 512)}      # (64, 96): three row tiles on four wavefronts
SHAPES = {"1x1x1": (1, 1, 1), "1x5x7": (1, 5, 7), "5x5x7": (5, 5, 7), "8x8x16": (8, 8, 16)}                  # 1 token; 35 (a tail of 3); 175 (tiles straddle maps); 1024
KINDS = (("gauss", 1.0), ("student", 1.0), ("gauss", 1e-2), ("student", 1e2), ("gauss", 1e2), ("student", 1e-2))
ARGS_W64 = args(64, 2, 32, [4, 2, 1], DIM_HEADS, WINDOWS, "naive", 2)
ARGS_W256 = args(256, 8, 32, [16, 8, 4], DIM_HEADS, WINDOWS, "split_attn", 1)


def _image(layer):
    return ops.pack_v2x_ffn_weights(*folded_feed_forward(layer.norm, layer.fn))


@pytest.fixture(scope="module")
def layers():
    """config -> (PreNorm(FeedForward) on the GPU in float32, its state, its parameter image on the GPU), made once."""
    out = {}
    for name, (C, M) in CONFIGS.items():
        layer = PreNorm(C, FeedForward(C, M, 0.3))
        v2xvit_parameters_(layer, seed=C + M)
        layer.eval()
        out[name] = (copy.deepcopy(layer).to(DEV), {k: v.clone() for k, v in layer.state_dict().items()}, _image(layer).to(DEV))
    return out


def _maps(kind, scale, shape, seed):
    if kind == "gauss":
        return torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale
    return student_t(shape, seed, scale=scale)


@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("config", list(CONFIGS))
def test_kernel_against_the_float64_layer(layers, config, shape):
    """Gaussian and Student-t maps at scales 1e-2, 1, 1e2.  The float64 yardstick runs on the GPU too (float64 torch ops)."""
    n, H, W = SHAPES[shape]
    C, M = CONFIGS[config]
    gpu_layer, state, image = layers[config]
    worst_kernel = worst_torch = 0.0
    for k, (kind, scale) in enumerate(KINDS):
        xd = _maps(kind, scale, (n, H, W, C), 1000 * n + 10 * H + k).to(DEV)
        ref = feed_forward_f64(state, xd)
        what = f"{config} {shape} {kind} x{scale}"
        with torch.no_grad():
            plain = gpu_layer(xd) + xd
        e_torch = assert_elementwise(plain, ref, what + ": float32 op-by-op layer vs float64")
        got = ops.v2x_feed_forward(xd, image)
        assert got.shape == (n, H, W, C) and got.data_ptr() != xd.data_ptr()
        e_kernel = assert_elementwise(got, ref, what + ": kernel vs float64")
        print(f"{what}: error / scale, kernel {e_kernel:.3e}, float32 op-by-op layer {e_torch:.3e}")
        worst_kernel, worst_torch = max(worst_kernel, e_kernel), max(worst_torch, e_torch)
    print(f"{config} {shape}: worst error / scale, kernel {worst_kernel:.3e}, float32 op-by-op layer {worst_torch:.3e}")


def test_tokens_are_independent_and_the_result_is_reproducible(layers):
    """Five maps equal their five single-map results bit for bit (35 tokens a map: every tile of the whole straddles or is cut differently from the single maps');
    two calls are equal bit for bit; the same tokens viewed as [1, 1, T, C] give the same bits."""
    for config in ("C64_M96", "C256_M256"):
        C, _ = CONFIGS[config]
        image = layers[config][2]
        x = torch.randn(5, 5, 7, C, generator=torch.Generator().manual_seed(3)).to(DEV)
        whole = ops.v2x_feed_forward(x, image)
        for i in range(5):
            assert torch.equal(whole[i:i + 1], ops.v2x_feed_forward(x[i:i + 1].contiguous(), image)), (config, i)
        assert torch.equal(whole, ops.v2x_feed_forward(x, image)), config
        assert torch.equal(whole.reshape(1, 1, 175, C), ops.v2x_feed_forward(x.reshape(1, 1, 175, C), image)), config


def test_argument_contract_on_real_buffers(layers):
    """Every status code before a launch, with real device buffers: a canary output stays untouched by every refused call; tokens = 0 returns OK without a launch."""
    image = layers["C64_M64"][2]
    image256 = layers["C256_M256"][2]
    L = hip.lib()
    T, C, M = 35, 64, 64
    x = torch.randn(T, C, device=DEV)
    out = torch.full((T, C), 7.0, device=DEV)
    stream = ops._stream()

    def call(x_=x, T_=T, C_=C, M_=M, image_=image, pb=None, out_=out):
        return L.coalign_v2x_feed_forward(ops._ptr(x_), T_, C_, M_, ops._ptr(image_), image.numel() if pb is None else pb, ops._ptr(out_), stream)
    assert call(x_=None) == -1 and call(image_=None) == -1 and call(out_=None) == -1
    assert call(x_=x.view(-1)[1:]) == -1 and call(out_=out.view(-1)[2:]) == -1 and call(image_=image[4:]) == -1      # misaligned
    assert call(T_=-1) == -2 and call(C_=0) == -2 and call(M_=-32) == -2 and call(pb=image.numel() - 4) == -2
    assert call(pb=image256.numel(), image_=image256) == -2                                     # the (256, 256) image for a (64, 64) call
    assert call(C_=128) == -3 and call(M_=48) == -3 and call(M_=544) == -3 and call(M_=16) == -3
    assert call(out_=x) == -3
    assert call(T_=0) == 0 and call(T_=0, x_=None, out_=None) == 0
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    assert call() == 0
    torch.cuda.synchronize()
    assert bool((out != 7.0).any()) and bool(torch.isfinite(out).all())
    with pytest.raises(ValueError):
        ops.v2x_feed_forward(torch.randn(4, 128, device=DEV), image)
    with pytest.raises(ValueError):
        ops.v2x_feed_forward(torch.randn(4, 256, device=DEV), image)                           # the (64, 64) image for 256 channels
    with pytest.raises(ValueError):
        ops.v2x_feed_forward(torch.randn(4, 64, device=DEV)[:, ::2], image)


def _float64_fusion(m, x, rl, A):
    """The module's own op-by-op route in float64 on the CPU: tests/test_v2xvit_cpu.py pins that route to the reference's recordings."""
    with torch.no_grad():
        return copy.deepcopy(m).cpu().double().forward_torch(x.double(), rl, A)


BATCH_SEED = 108      # the warps of tests/test_v2x_window_gpu.py's module cases: chosen there by float32's own error, not by a kernel's


def _batch(C, seed, H=16, W=32):
    """record_len [3, 1] padded to five agents on an H x W map: a shift, a rotation, an agent half outside (make_thetas)."""
    x = torch.randn(4, C, H, W, generator=torch.Generator().manual_seed(seed))
    A = torch.zeros(2, 5, 5, 2, 3, dtype=torch.float64)
    A[..., 0, 0] = A[..., 1, 1] = 1.0
    A[0, :3, :3] = make_thetas(3, H, W, seed=seed)
    return x, torch.tensor([3, 1]), A


def _spied(m, x, rl, A):
    """-> (the module's output, calls of ops.v2x_feed_forward, calls of ops.v2x_window_attention)"""
    seen = {"ffn": 0, "win": 0}
    real_f, real_w = ops.v2x_feed_forward, ops.v2x_window_attention
    ops.v2x_feed_forward = lambda *a_, **k_: (seen.__setitem__("ffn", seen["ffn"] + 1), real_f(*a_, **k_))[1]
    ops.v2x_window_attention = lambda *a_, **k_: (seen.__setitem__("win", seen["win"] + 1), real_w(*a_, **k_))[1]
    try:
        with torch.no_grad():
            got = m(x.to(DEV), rl, A.to(DEV))
    finally:
        ops.v2x_feed_forward, ops.v2x_window_attention = real_f, real_w
    return got, seen["ffn"], seen["win"]


@pytest.mark.parametrize("window", [False, True], ids=["ffn_alone", "ffn_and_window"])
@pytest.mark.parametrize("case", ["W64_naive_depth2", "W256_split_attn"])
def test_module_ffn_kernels_against_float64(case, window):
    """``V2XViTFusion`` with ``ffn_kernels`` set on a 16 x 32 batch, alone and together with ``window_kernels``: against its own op-by-op route in float64, the float32
    op-by-op route on the same GPU held to the bound first."""
    a, seed, C = {"W64_naive_depth2": (ARGS_W64, 64, 64), "W256_split_attn": (ARGS_W256, 41, 256)}[case]
    m = V2XViTFusion(copy.deepcopy(a))
    v2xvit_parameters_(m, seed=seed)
    m = m.eval().to(DEV)
    assert m.ffn_kernels is False and "switched off" in m.ffn_kernel_reason(C)
    m.ffn_kernels, m.window_kernels = True, window
    x, rl, A = _batch(C, BATCH_SEED)
    ref = _float64_fusion(m, x, rl, A)
    assert m.kernel_route(C, 3, (16, 32)) and m.ffn_kernel_reason(C) is None
    got, n_ffn, n_win = _spied(m, x, rl, A)
    depth = len(m.fusion_net.encoder.layers)
    assert n_ffn == 2 * depth and n_win == (2 * depth if window else 0)      # two frames, one feed-forward and one fusion block per layer
    with torch.no_grad():
        m.force_torch = True
        plain = m(x.to(DEV), rl, A.to(DEV))
        m.force_torch = False
    e_torch = assert_elementwise(plain, ref, case + ": float32 op-by-op route vs float64")
    e_kernel = assert_elementwise(got, ref, case + ": kernel route with the feed-forward kernel vs float64")
    print(f"{case} window_kernels={window}: worst error / scale, kernel route {e_kernel:.3e}, float32 op-by-op route {e_torch:.3e}")


def test_module_refuses_a_hidden_width_of_48():
    """mlp_dim = 48: the module reports a reason, runs the torch ops for the feed-forward and equals the switch-off result bit for bit."""
    a = copy.deepcopy(ARGS_W64)
    a["transformer"]["encoder"]["feed_forward"]["mlp_dim"] = 48
    m = V2XViTFusion(a)
    v2xvit_parameters_(m, seed=64)
    m = m.eval().to(DEV)
    x, rl, A = _batch(64, BATCH_SEED)
    off, n_ffn, _ = _spied(m, x, rl, A)
    assert n_ffn == 0
    m.ffn_kernels = True
    reason = m.ffn_kernel_reason(64)
    assert reason is not None and "48" in reason and m.kernel_route(64, 3, (16, 32))
    on, n_ffn, _ = _spied(m, x, rl, A)
    assert n_ffn == 0 and torch.equal(on, off)


def test_forward_under_graph_capture():
    m = V2XViTFusion(copy.deepcopy(ARGS_W64))
    v2xvit_parameters_(m, seed=9)
    m = m.eval().to(DEV)
    m.ffn_kernels = m.window_kernels = True
    x, _, A = _batch(64, 9)
    x, A, groups = x[:3].contiguous(memory_format=torch.channels_last).to(DEV), A[:1].to(DEV), [3]
    assert m.ffn_kernel_reason(64) is None and m.window_kernel_reason(64, (16, 32)) is None
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
    """``mini_pointpillar_v2xvit.yaml`` (C = 64, mlp_dim = 64, 16 x 32 map), 3 agents: with the feed-forward kernel alone and with both switches the heads against the
    same model with its fusion on the op-by-op route; with both switches the detections of ``inference_intermediate_fusion`` equal those of ``FramePipeline`` (eager
    lanes and captured frames), bit for bit."""
    h = builtin_config("mini_pointpillar_v2xvit")
    model = build_model(h)
    fill_parameters_(model, seed=0, cls_bias=-1.0)
    v2xvit_parameters_(model.fusion_net, seed=2)
    with torch.no_grad():
        model.reg_head.weight.mul_(0.01); model.reg_head.bias.zero_(); model.cls_head.weight.mul_(0.05)
    model = model.to(DEV).eval()
    anchors = torch.from_numpy(build_postprocessor(h["postprocess"], False).generate_anchor_box())
    frames = [to_device(make_frame(h, 3, pillars_per_agent=150, seed=40 + i, spread_xy=(4.0, 2.0), spread_yaw=45.0), DEV) for i in range(4)]
    with torch.no_grad():
        model.fusion_net.force_torch = True
        want = model(frames[0])
        model.fusion_net.force_torch = False
    for window in (False, True):
        model.fusion_net.ffn_kernels, model.fusion_net.window_kernels = True, window
        assert model.fusion_net.kernel_route(model.out_channel, 3, (16, 32)) and model.fusion_net.ffn_kernel_reason(model.out_channel) is None
        with torch.no_grad():
            got = model(frames[0])
        for k in ("cls_preds", "reg_preds", "dir_preds"):
            print(k, window, assert_elementwise(got[k], want[k], f"{k}: kernel-route fusion with the feed-forward kernel (window {window}) vs op-by-op fusion"))
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
