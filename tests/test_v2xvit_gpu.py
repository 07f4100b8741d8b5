"""V2X-ViT's fusion on the GPU (csrc/v2x_attn.hip through the C ABI): ``ops.v2x_agent_attention`` against the float64 restatement of one agent-attention layer
(tests/v2xvit_reference.py) at one to eight agents, all and one receiver, with and without the warp, on maps that are no multiple of the pixel tile, across input
scales; its argument contract on real buffers; the module's kernel route against float64 on the recorded cases' shapes; and the model
(``mini_pointpillar_v2xvit.yaml``) eagerly and through ``FramePipeline``.

The bound is ``assert_elementwise`` at its defaults (rtol 1e-4, floor 1e-5 of the scale).  Every kernel case first holds the float32 op-by-op layer, on the same
GPU and the same inputs, to that bound: the inputs never ask of the kernel what float32 itself cannot do.  Both errors are printed."""
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
from coalign_amd.v2xvit import HGTCavAttention, PreNorm, folded_agent_attention
from v2v_reference import make_thetas, student_t
from v2xvit_reference import ARGS_B, SEED_B, agent_attention_f64, args, inputs

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ARGS_A64 = args(64, 2, 32, [4, 2, 1], [16, 32, 64], [2, 4, 8], "naive", 2)      # case A's structure at a width the kernel takes


@pytest.fixture(scope="module")
def layers():
    """C -> (PreNorm(HGTCavAttention) on the CPU in float32, its state, its parameter image on the GPU), made once."""
    out = {}
    for C in (64, 256):
        layer = PreNorm(C, HGTCavAttention(C, heads=C // 32, dim_head=32))
        v2xvit_parameters_(layer, seed=C)
        layer.eval()
        with torch.no_grad():
            image = ops.pack_v2x_weights(*folded_agent_attention(layer.norm, layer.fn, True))
        out[C] = (layer, {k: v.clone() for k, v in layer.state_dict().items()}, image.to(DEV))
    return out


def _maps(kind, scale, shape, seed):
    if kind == "gauss":
        return torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale
    return student_t(shape, seed, scale=scale)


@pytest.mark.parametrize("hw", [(5, 7), (8, 16)], ids=["5x7", "8x16"])
@pytest.mark.parametrize("C", [64, 256])
def test_kernel_against_the_float64_layer(layers, C, hw):
    """n in {1, 2, 3, 5, 8}, R in {n, 1}, theta NULL and real warps (the last sender half outside; from four agents on, one wholly outside), Gaussian and Student-t maps
    at scales 1e-2, 1, 1e2.  5 x 7 = 35 pixels is a partial 32-pixel tile and n H W a multiple of nothing; 8 x 16 fills four tiles."""
    H, W = hw
    layer, state, image = layers[C]
    gpu_layer = copy.deepcopy(layer).to(DEV)
    worst_kernel = worst_torch = 0.0
    for n in (1, 2, 3, 5, 8):
        theta = make_thetas(n, H, W, seed=n)[0]
        for k, (kind, scale) in enumerate((("gauss", 1.0), ("student", 1.0), ("gauss", 1e-2), ("student", 1e2), ("gauss", 1e2), ("student", 1e-2))):
            x = _maps(kind, scale, (n, H, W, C), 100 * n + k)
            xd = x.to(DEV)
            for th in (None, theta):
                ref = agent_attention_f64(state, x, th, C // 32)
                what = f"C={C} {H}x{W} n={n} {kind} x{scale} {'warp' if th is not None else 'in place'}"
                with torch.no_grad():
                    xw = xd if th is None else ops.warp_fuse_nhwc([xd.permute(0, 3, 1, 2)], th.to(DEV), ops.FUSE_NONE)[0].permute(0, 2, 3, 1)
                    plain = gpu_layer(xw[None], mask=torch.ones(1, 1, 1, 1, n, device=DEV))[0] + xw
                e_torch = assert_elementwise(plain, ref, what + ": float32 op-by-op layer vs float64")
                for R in sorted({n, 1}):
                    got = ops.v2x_agent_attention(xd, None if th is None else th.to(DEV), image, receivers=R)
                    assert got.shape == (R, H, W, C)
                    e_kernel = assert_elementwise(got, ref[:R], what + f" R={R}: kernel vs float64")
                    worst_kernel, worst_torch = max(worst_kernel, e_kernel), max(worst_torch, e_torch)
    print(f"C={C} {H}x{W}: worst error / scale, kernel {worst_kernel:.3e}, float32 op-by-op layer {worst_torch:.3e}")


def test_a_sender_wholly_outside_contributes_layernorm_of_zero(layers):
    """All senders but the ego warped wholly outside: keys and values are LayerNorm(0) = beta, as in the reference (not dropped, not zero)."""
    layer, state, image = layers[64]
    x = torch.randn(3, 5, 7, 64, generator=torch.Generator().manual_seed(1))
    th = torch.tensor([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0]], dtype=torch.float64).repeat(3, 1, 1)
    th[1:, 0, 2] = 5.0
    ref = agent_attention_f64(state, x, th, 2)
    alone = agent_attention_f64(state, x[:1], th[:1], 2)
    assert float((ref[0] - alone[0]).abs().max()) > 1e-2 * float(ref.abs().max())
    assert_elementwise(ops.v2x_agent_attention(x.to(DEV), th.to(DEV), image), ref, "senders wholly outside")


def test_argument_contract_on_real_buffers(layers):
    """Every status code before a launch, with real device buffers: a canary output stays untouched by every refused call; n = 0 returns OK without a launch."""
    _, _, image = layers[64]
    L = hip.lib()
    n, H, W, C = 3, 5, 7, 64
    x = torch.randn(n, H, W, C, device=DEV)
    out = torch.full((n, H, W, C), 7.0, device=DEV)
    ws = torch.empty(L.coalign_v2x_workspace_bytes(n, C, H, W) // 4, device=DEV)
    stream = ops._stream()

    def call(x_=x, n_=n, R_=n, C_=C, H_=H, W_=W, image_=image, pb=None, out_=out, ws_=ws, wb=None):
        return L.coalign_v2x_agent_attention(ops._ptr(x_), n_, R_, C_, H_, W_, None, ops._ptr(image_), image.numel() if pb is None else pb, ops._ptr(out_), ops._ptr(ws_),
                                             ws.numel() * 4 if wb is None else wb, stream)
    assert call(x_=None) == -1 and call(image_=None) == -1 and call(out_=None) == -1 and call(ws_=None) == -1
    assert call(n_=-1, R_=-1) == -2 and call(n_=2, R_=3) == -2 and call(H_=0) == -2 and call(pb=image.numel() - 32) == -2 and call(wb=ws.numel() * 4 - 4) == -2
    assert call(n_=9, R_=9) == -3 and call(C_=128) == -3 and call(R_=2) == -3 and call(x_=x.view(-1)[1:]) == -3
    assert call(n_=0, R_=0) == 0 and call(R_=0) == 0
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    assert call() == 0
    torch.cuda.synchronize()
    assert bool((out != 7.0).any()) and bool(torch.isfinite(out).all())
    with pytest.raises(ValueError):
        ops.v2x_agent_attention(x, None, image, receivers=2)
    with pytest.raises(ValueError):
        ops.v2x_agent_attention(torch.randn(2, 4, 4, 128, device=DEV), None, image)


def _float64_fusion(m, x, rl, A):
    """The module's own op-by-op route in float64 on the CPU: tests/test_v2xvit_cpu.py pins that route to the reference's recordings."""
    with torch.no_grad():
        return copy.deepcopy(m).cpu().double().forward_torch(x.double(), rl, A)


@pytest.mark.parametrize("case", ["A64_naive_depth2", "B_split_attn"])
def test_module_kernel_route_against_float64(case):
    """The recorded cases' batch (record_len [3, 1] padded to five, a shift, a rotation, an agent half outside) on the kernel route: against float64, with the float32
    op-by-op route on the same GPU held to the same bound first; ``forward_reduced`` on the GPU alike."""
    a, seed, C = (ARGS_A64, 64, 64) if case.startswith("A") else (ARGS_B, SEED_B, 256)
    m = V2XViTFusion(copy.deepcopy(a))
    v2xvit_parameters_(m, seed=seed)
    m = m.eval().to(DEV)
    x, rl, A = inputs(C, seed + 100)
    ref = _float64_fusion(m, x, rl, A)
    assert m.kernel_route(C, 3, (8, 16))
    with torch.no_grad():
        got = m(x.to(DEV), rl, A.to(DEV))
        red = m.forward_reduced(x.to(DEV), rl, A.to(DEV))
        m.force_torch = True
        plain = m(x.to(DEV), rl, A.to(DEV))
        m.force_torch = False
    e_torch = assert_elementwise(plain, ref, case + ": float32 op-by-op route vs float64")
    e_kernel = assert_elementwise(got, ref, case + ": kernel route vs float64")
    e_red = assert_elementwise(red, ref, case + ": forward_reduced (float32, GPU) vs float64")
    print(f"{case}: worst error / scale, kernel route {e_kernel:.3e}, float32 op-by-op route {e_torch:.3e}, forward_reduced {e_red:.3e}")
    with pytest.raises(NotImplementedError):
        m(x.to(DEV), rl, A.to(DEV), rows=[0, 1, 2, 3])


def test_unsupported_width_takes_the_torch_route():
    a = args(32, 2, 16, [4, 2, 1], [8, 16, 32], [2, 4, 8], "naive", 1)
    m = V2XViTFusion(a)
    v2xvit_parameters_(m, seed=5)
    m = m.eval().to(DEV)
    assert not m.kernel_route(32, 3)
    x, rl, A = inputs(32, 5)
    with torch.no_grad():
        out = m(x.to(DEV), rl, A.to(DEV))
    assert_elementwise(out, _float64_fusion(m, x, rl, A), "dim 32 (torch route on the GPU) vs float64")


def test_forward_under_graph_capture():
    m = V2XViTFusion(copy.deepcopy(ARGS_A64))
    v2xvit_parameters_(m, seed=9)
    m = m.eval().to(DEV)
    x, rl, A = inputs(64, 9)
    x, A, groups = x[:3].contiguous(memory_format=torch.channels_last).to(DEV), A[:1].to(DEV), [3]
    with torch.no_grad():
        m(x, groups, A)                                                     # (parameter images packed, grids and indices placed: before the capture)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = m(x, groups, A)
        for seed in (1, 2):
            fresh = torch.randn(3, 64, 8, 16, generator=torch.Generator().manual_seed(seed)).to(DEV)
            x.copy_(fresh)
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(out, m(fresh.contiguous(memory_format=torch.channels_last), groups, A)), seed


def _mini_world(n_frames):
    h = builtin_config("mini_pointpillar_v2xvit")
    model = build_model(h)
    fill_parameters_(model, seed=0, cls_bias=-1.0)
    v2xvit_parameters_(model.fusion_net, seed=2)
    with torch.no_grad():
        model.reg_head.weight.mul_(0.01); model.reg_head.bias.zero_(); model.cls_head.weight.mul_(0.05)
    model = model.to(DEV).eval()
    anchors = torch.from_numpy(build_postprocessor(h["postprocess"], False).generate_anchor_box())
    frames = [to_device(make_frame(h, 3, pillars_per_agent=150, seed=40 + i, spread_xy=(4.0, 2.0), spread_yaw=45.0), DEV) for i in range(n_frames)]
    return h, model, anchors, frames


def test_model_heads_and_detections():
    """``mini_pointpillar_v2xvit.yaml``, 3 agents: the heads of the kernel-route fusion against the same model with its fusion on the op-by-op route; detections of
    ``inference_intermediate_fusion`` equal those of ``FramePipeline`` (eager lanes and captured frames), bit for bit."""
    h, model, anchors, frames = _mini_world(4)
    assert model.fusion_net.kernel_route(model.out_channel, 3, (16, 32))
    with torch.no_grad():
        got = model(frames[0])
        model.fusion_net.force_torch = True
        want = model(frames[0])
        model.fusion_net.force_torch = False
    assert set(got) == {"cls_preds", "reg_preds", "dir_preds"}
    for k in ("cls_preds", "reg_preds", "dir_preds"):
        print(k, assert_elementwise(got[k], want[k], f"{k}: kernel-route fusion vs op-by-op fusion"))
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
