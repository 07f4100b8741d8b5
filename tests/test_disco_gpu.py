"""DiscoNet's pixel-weight fusion on the GPU (csrc/disco_fuse.hip through the C ABI): the kernel against the float64 restatement of tests/disco_reference.py at
every channel class, agent count and at map sizes that are no multiple of its 32-pixel tile; across activation scales; against the module's own op-by-op route;
under graph capture; and at model level (``mini_pointpillar_disconet.yaml``), eagerly and through ``FramePipeline``.

Weights come from ``synthetic.disco_parameters_``: every parity test first asserts on the float64 side that the MLP is visible in the result
(``assert_not_degenerate``: most logits positive, softmax weights that differ between agents).

Measured on the MI355X, worst |error| / max |reference| over the cases of ``test_kernel_against_float64``: see DESIGN.md, "DiscoNet's pixel-weight fusion"."""
import math

import pytest
import torch

from conftest import assert_elementwise
from coalign_amd import ops
from coalign_amd.config import builtin_config
from coalign_amd.detector import build_model, to_device
from coalign_amd.fusion import DiscoFusion
from coalign_amd.inference import inference_intermediate_fusion
from coalign_amd.pipeline import FramePipeline
from coalign_amd.postprocess import build_postprocessor
from coalign_amd.synthetic import disco_parameters_, fill_parameters_, make_frame
from disco_reference import assert_not_degenerate, disco_fuse_f64, warp_f64

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SIZES = ((1, 1), (5, 7), (13, 37))


def thetas(n, H, W):
    """One affine per agent, mixed: identity (the ego), a sub-pixel shift, an agent pushed wholly outside the map (its all-zero row still takes its softmax share), a
    30 degree rotation, an agent half outside; agents 5 .. 7 repeat shift / rotation / half-outside with other parameters."""
    th = torch.zeros(n, 2, 3, dtype=torch.float64)
    th[:, 0, 0] = th[:, 1, 1] = 1.0

    def rot(deg, tx, ty):
        c, s = math.cos(math.radians(deg)), math.sin(math.radians(deg))
        return torch.tensor([[c, -s * H / W, tx], [s * W / H, c, ty]], dtype=torch.float64)
    kinds = [None,
             torch.tensor([[1, 0, 2 * 0.37 / W], [0, 1, -2 * 0.21 / H]], dtype=torch.float64),
             torch.tensor([[1, 0, 3.0], [0, 1, 0.25]], dtype=torch.float64),
             rot(30.0, 0.05, -0.03),
             torch.tensor([[1, 0, 1.0], [0, 1, 0.0]], dtype=torch.float64),
             torch.tensor([[1, 0, -2 * 1.6 / W], [0, 1, 2 * 0.8 / H]], dtype=torch.float64),
             rot(-30.0, -0.2, 0.1),
             torch.tensor([[1, 0, 0.0], [0, 1, -1.0]], dtype=torch.float64)]
    for j in range(1, n):
        th[j] = kinds[j]
    return th


def fusion_module(C, seed, input_scale=1.0):
    m = DiscoFusion(C)
    disco_parameters_(m.pixel_weight_layer, seed=seed, input_scale=input_scale)
    return m.eval()


def run_kernel(m, x, th):
    """The launch itself, through ``ops.disco_fuse`` -> ctypes -> ``coalign_disco_fuse``: -> [C, H, W] on the host."""
    md = m.to(DEV)
    image = md.pixel_weight_layer.packed()
    assert image is not None and image.is_cuda
    out = ops.disco_fuse(x.to(DEV).contiguous(memory_format=torch.channels_last), th.to(DEV), image)
    torch.cuda.synchronize()
    return out[0].cpu()


def affine_of(th, L=8):
    A = torch.zeros(1, L, L, 2, 3, dtype=torch.float64)
    A[0, 0, :th.shape[0]] = th
    return A


@pytest.mark.parametrize("n", [1, 2, 3, 5, 8])
@pytest.mark.parametrize("C", [32, 64, 256, 384])
def test_kernel_against_float64(C, n):
    for H, W in SIZES:
        m = fusion_module(C, seed=7)
        x = torch.randn(n, C, H, W, generator=torch.Generator().manual_seed(100 * C + 10 * n + H))
        th = thetas(n, H, W)
        ref, s, a = disco_fuse_f64(m.state_dict(), x, th)
        assert_not_degenerate(s, a, (C, n, H, W))
        if n >= 3:
            assert not bool(warp_f64(x[2:3], th[2:3]).any())                # the agent outside the map: an all-zero row ...
            assert float(a[2].min()) > 0.0                                  # ... with a softmax share of its own
        got = run_kernel(m, x, th)
        with torch.no_grad():
            route = m.forward_torch(x.to(DEV), [n], affine_of(th).to(DEV))[0].cpu()
        scale = float(ref.abs().max())
        print(f"disco_fuse C={C} n={n} {H}x{W}: kernel {float((got.double() - ref).abs().max()) / scale:.3e}, fp32 torch route "
              f"{float((route.double() - ref).abs().max()) / scale:.3e} of the scale")
        assert_elementwise(got, ref, f"kernel vs float64, C={C} n={n} {H}x{W}")


@pytest.mark.parametrize("scale", [1e-2, 1.0, 1e2])
def test_activation_scales(scale):
    """Maps at 1e-2, 1 and 1e2 times a Student-t draw (heavy tails), the first layer's weights scaled the other way: the sp16 operand split keeps its accuracy over the
    range and produces no inf / NaN."""
    C, n, H, W = 256, 3, 5, 7
    m = fusion_module(C, seed=11, input_scale=scale)
    g = torch.Generator().manual_seed(31)
    t = torch.randn(n, C, H, W, generator=g) / torch.sqrt(torch._standard_gamma(torch.full((n, C, H, W), 2.0), generator=g) / 2.0)      # Student-t, 4 degrees of freedom
    x = (scale * t).float()
    assert bool(torch.isfinite(x).all())
    th = thetas(n, H, W)
    ref, s, a = disco_fuse_f64(m.state_dict(), x, th)
    assert_not_degenerate(s, a, scale)
    got = run_kernel(m, x, th)
    assert bool(torch.isfinite(got).all())
    print(f"disco_fuse at activation scale {scale:g}: kernel {float((got.double() - ref).abs().max()) / float(ref.abs().max()):.3e} of the scale, max |x| {float(x.abs().max()):.3g}")
    assert_elementwise(got, ref, f"kernel vs float64 at activation scale {scale:g}")


@pytest.mark.parametrize("C,groups", [(64, [3, 1]), (256, [2, 5]), (96, [1])])
def test_module_kernel_route_equals_its_torch_route(C, groups):
    H, W = 9, 14
    m = fusion_module(C, seed=5).to(DEV)
    N = sum(groups)
    x = torch.randn(N, C, H, W, generator=torch.Generator().manual_seed(C)).to(DEV)
    A = torch.zeros(len(groups), 8, 8, 2, 3, dtype=torch.float64)
    for b, n in enumerate(groups):
        A[b, 0, :n] = thetas(n, H, W)
    A = A.to(DEV)
    with torch.no_grad():
        want = m.forward_torch(x, groups, A)
        got = m(x, torch.tensor(groups), A)
    assert got.shape == want.shape == (len(groups), C, H, W)
    assert_elementwise(got, want, f"DiscoFusion.forward (kernel) vs forward_torch, C={C} groups={groups}")
    # a negative last bias: part of the logits is clamped by the last ReLU (the weights of disco_parameters_ keep every logit positive)
    with torch.no_grad():
        m.pixel_weight_layer.conv1_4.bias.fill_(-10.0)
        logits = m.pixel_weight_layer(torch.cat((x[:1], x[:1]), dim=1))
        assert 0.05 < float((logits == 0).float().mean()) < 0.95
        assert_elementwise(m(x, torch.tensor(groups), A), m.forward_torch(x, groups, A), f"clamped logits, C={C} groups={groups}")
    # one agent: the softmax weight is 1 and the result IS the warp of the ego map -- the blend of coalign_warp_fuse_nhwc, bit for bit
    th = torch.tensor([[[0.9, 0.1, 0.05], [-0.1, 0.9, -0.02]]], dtype=torch.float64)
    if C in (64, 256):
        xc = x[:1].contiguous(memory_format=torch.channels_last)
        assert torch.equal(ops.disco_fuse(xc, th.to(DEV), m.pixel_weight_layer.packed()), ops.warp_fuse_nhwc([xc], th.to(DEV), ops.FUSE_NONE)[0])


def test_forward_under_graph_capture():
    C, groups, H, W = 256, [3], 13, 37
    m = fusion_module(C, seed=9).to(DEV)
    x = torch.randn(3, C, H, W, device=DEV).contiguous(memory_format=torch.channels_last)
    A = affine_of(thetas(3, H, W)).to(DEV)
    with torch.no_grad():
        m(x, groups, A)                                                     # (weight image packed, LDS limit raised: before the capture)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = m(x, groups, A)
        for seed in (1, 2):
            fresh = torch.randn(3, C, H, W, generator=torch.Generator().manual_seed(seed)).to(DEV)
            x.copy_(fresh)
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(out, m(fresh.contiguous(memory_format=torch.channels_last), groups, A)), seed


def _mini_world(n_frames):
    h = builtin_config("mini_pointpillar_disconet")
    model = build_model(h)
    fill_parameters_(model, seed=0, cls_bias=-1.0)
    disco_parameters_(model.fusion_net.pixel_weight_layer, seed=2)
    with torch.no_grad():
        model.reg_head.weight.mul_(0.01); model.reg_head.bias.zero_(); model.cls_head.weight.mul_(0.05)
    model = model.to(DEV).eval()
    anchors = torch.from_numpy(build_postprocessor(h["postprocess"], False).generate_anchor_box())
    frames = [to_device(make_frame(h, 3, pillars_per_agent=150, seed=40 + i, spread_xy=(4.0, 2.0), spread_yaw=45.0), DEV) for i in range(n_frames)]
    return h, model, anchors, frames


def test_model_heads_and_detections():
    """``mini_pointpillar_disconet.yaml``, 3 agents: the heads of the HIP route against the same model with its fusion on the op-by-op route; detections of
    ``inference_intermediate_fusion`` equal those of ``FramePipeline`` (eager lanes and captured frames), bit for bit."""
    h, model, anchors, frames = _mini_world(4)
    with torch.no_grad():
        got = model(frames[0])
        model.fusion_net.force_torch = True
        want = model(frames[0])
        model.fusion_net.force_torch = False
    assert set(got) == {"feature", "cls_preds", "reg_preds", "dir_preds"}
    for k in ("feature", "cls_preds", "reg_preds", "dir_preds"):
        assert_elementwise(got[k], want[k], f"{k}: HIP fusion vs op-by-op fusion")
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


def test_unsupported_width_takes_the_torch_route():
    m = fusion_module(48, seed=3).to(DEV)
    assert not m.kernel_route(48)
    x = torch.randn(2, 48, 5, 7, device=DEV)
    A = affine_of(thetas(2, 5, 7)).to(DEV)
    with torch.no_grad():
        out = m(x, [2], A)
        assert_elementwise(out, m.forward_torch(x, [2], A), "C = 48")
    ref, _, _ = disco_fuse_f64(m.state_dict(), x.cpu(), thetas(2, 5, 7))
    assert_elementwise(out[0], ref, "C = 48 vs float64")
