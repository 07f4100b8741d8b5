"""V2VNet's message passing on the GPU (csrc/v2v_fuse.hip through the C ABI, the convolutions on conv3x3_sp): the three kernels bit for bit against the project's
own warp / pack kernels and torch arithmetic, the gate against float64, the module's kernel route against the float64 restatement of tests/v2v_reference.py at one
to eight agents and at map sizes that are no multiple of any tile; across activation scales; against the module's own op-by-op route; under graph capture; and at
model level (``mini_pointpillar_v2vnet.yaml``), eagerly and through ``FramePipeline``.

Weights come from ``synthetic.v2v_parameters_``: every parity test first asserts on the float64 side that every stage is visible in the result
(``assert_not_degenerate``).  Measured on the MI355X: see DESIGN.md, "V2VNet's message passing"."""
import pytest
import torch

from conftest import assert_elementwise
from coalign_amd import ops
from coalign_amd.config import builtin_config
from coalign_amd.detector import build_model, to_device
from coalign_amd.fusion import V2VNetFusion
from coalign_amd.inference import inference_intermediate_fusion
from coalign_amd.pipeline import FramePipeline
from coalign_amd.postprocess import build_postprocessor
from coalign_amd.synthetic import fill_parameters_, make_frame, v2v_parameters_
from v2v_reference import assert_not_degenerate, make_thetas, student_t, v2v_fuse_f64

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SIZES = ((1, 1), (5, 7), (13, 37))


def nhwc(t):
    """-> the same logical [N, C, H, W] tensor in dense [N, H, W, C] memory (what ``contiguous(memory_format=channels_last)`` does not promise for 1 x 1 maps)."""
    return t.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)


def project_warp(x, th):
    """The project's own warp of the n maps x by th [n, 2, 3]: ``warp_fuse_nhwc`` (FUSE_NONE), whose taps and blend csrc/warp_taps.h holds.  A 1 x 1 map is at the
    same time NCHW memory, which that op's layout predicate does not take: there the NCHW kernel ``warp_fuse`` (the same expressions, csrc/warp_fuse.hip) stands in."""
    if x.shape[2] * x.shape[3] > 1:
        return ops.warp_fuse_nhwc([x], th, ops.FUSE_NONE)[0]
    return ops.warp_fuse(x, th, [x.shape[0]], ops.FUSE_NONE)


def v2v_args(C, H, W, K=2, layers=1, gru=True, agg="max"):
    return {"num_iteration": K, "in_channels": C, "gru_flag": gru, "agg_operator": agg, "conv_gru": {"H": H, "W": W, "num_layers": layers, "kernel_size": [[3, 3]] * layers}}


def fusion_module(args, seed, input_scale=1.0):
    m = V2VNetFusion(args)
    v2v_parameters_(m, seed=seed, input_scale=input_scale)
    return m.eval()


def affine_of(thetas, L=8):
    """[n, n, 2, 3] per frame -> normalized_affine_matrix [B, L, L, 2, 3]."""
    A = torch.zeros(len(thetas), L, L, 2, 3, dtype=torch.float64)
    A[..., 0, 0] = A[..., 1, 1] = 1.0
    for b, th in enumerate(thetas):
        A[b, :th.shape[0], :th.shape[0]] = th
    return A


@pytest.mark.parametrize("C", [64, 256])
def test_warp_split_is_the_projects_warp_and_pack_bit_for_bit(C):
    for H, W in SIZES:
        for n in (1, 2, 3, 5, 8):
            x = nhwc(torch.randn(n, C, H, W, generator=torch.Generator().manual_seed(C + n + H)).to(DEV))
            th = make_thetas(n, H, W, seed=n).to(DEV)
            for R in sorted({n, 1}):
                got = ops.v2v_warp_split(x, th[:R])
                assert got.shape == (R * n, C, H, W)
                for i in range(R):
                    want = ops.SplitMap.pack(project_warp(x, th[i]))
                    assert torch.equal(got.data[i * n:(i + 1) * n], want.data), (C, H, W, n, R, i)


@pytest.mark.parametrize("agg", ["max", "avg"])
@pytest.mark.parametrize("C", [64, 256])
def test_aggregate_is_the_stated_arithmetic(C, agg):
    """(a + e) * mask, then max over j -- bit for bit -- or the sum in order of j divided by n; the masks are the project's own warp of a map of ones; both output
    forms.  The mean is held to 2 ulp, not to the bit: the kernel divides (correctly rounded), torch may multiply by a rounded reciprocal (two roundings, 1.5 ulp from
    the quotient).  In the SplitMap that is 2 units of the pair's 22 bits plus the 2^-34 a pair keeps of a value below 2^-14."""
    for H, W in SIZES:
        for n in (1, 2, 3, 5, 8):
            g = torch.Generator().manual_seed(3 * C + n + W)
            th = make_thetas(n, H, W, seed=10 + n).to(DEV)
            x = nhwc(torch.randn(n, C, H, W, generator=g).to(DEV))
            ones = nhwc(torch.ones(n, 64, H, W, device=DEV))
            for R in sorted({n, 1}):
                a = nhwc(torch.randn(R * n, C, H, W, generator=g).to(DEV))
                e = nhwc(torch.randn(R, C, H, W, generator=g).to(DEV))
                mask = torch.stack([project_warp(ones, th[i])[:, :1] for i in range(R)])      # [R, n, 1, H, W]
                m = (a.view(R, n, C, H, W) + e.unsqueeze(1)) * mask
                if agg == "max":
                    want = m.max(dim=1)[0]
                else:
                    want = m[:, 0]
                    for j in range(1, n):
                        want = want + m[:, j]
                    want = want / torch.full((), float(n), device=DEV)
                plain = ops.v2v_aggregate(a, e, x, th[:R], agg, gru=False)
                split = ops.v2v_aggregate(a, e, x, th[:R], agg, gru=True)
                assert plain.shape == (R, C, H, W) and split.shape == (R, 2 * C, H, W) and ops.nhwc_memory(plain)
                what = (C, agg, H, W, n, R)
                if agg == "max":
                    assert torch.equal(plain, x[:R] + want), what
                    assert torch.equal(split.data, ops.SplitMap.pack(nhwc(torch.cat([x[:R], want], dim=1))).data), what
                else:
                    assert bool(((split.dense_reference()[:, C:] - want).abs() <= 2.0 ** -20 * want.abs() + 2.0 ** -32).all()), what
                    assert bool(((plain - (x[:R] + want)).abs() <= 2.0 ** -22 * (x[:R].abs() + want.abs()) + 1e-30).all()), what
                assert torch.equal(split.dense_reference()[:, :C], ops.SplitMap.pack(x[:R]).dense_reference()), what


def test_gate_against_float64():
    """sigmoid(b) * tanh(c) over -30 .. 30 with +-0, every (b, c) sign combination, against float64; float32 and SplitMap outputs."""
    Ch, H, W = 64, 5, 7
    g = torch.Generator().manual_seed(5)
    y = (torch.rand(3, 2 * Ch, H, W, generator=g) - 0.5) * 60.0
    y[0, :, 0, 0] = torch.linspace(-30, 30, 2 * Ch)
    y[0, :Ch, 0, 1], y[0, Ch:, 0, 1] = torch.linspace(-30, 30, Ch), torch.linspace(30, -30, Ch)
    y[1] = (torch.rand(2 * Ch, H, W, generator=g) - 0.5) * 4.0                  # the range the gates live in
    y[2, :, 1, 1], y[2, :, 1, 2], y[2, 0, 1, 3], y[2, Ch, 1, 3] = 0.0, -0.0, -0.0, 0.0
    ref = torch.sigmoid(y[:, :Ch].double()) * torch.tanh(y[:, Ch:].double())
    yd = nhwc(y.to(DEV))
    got = ops.v2v_gate(yd).cpu()
    sp = ops.v2v_gate(yd, out_split=True)
    assert bool(torch.isfinite(got).all()) and got.shape == (3, Ch, H, W) and sp.shape == (3, Ch, H, W)
    ulp = torch.exp2(torch.floor(torch.log2(ref.abs().clamp_min(2.0 ** -126))) - 23)
    print(f"v2v_gate: worst error {float(((got.double() - ref).abs() / ulp).max()):.2f} ulp, {float((got.double() - ref).abs().max()):.3e} absolute")
    assert_elementwise(got, ref, "v2v_gate (float32) vs float64")
    assert_elementwise(sp.dense_reference(), ref, "v2v_gate (SplitMap) vs float64")
    assert torch.equal(sp.data, ops.SplitMap.pack(nhwc(got.to(DEV))).data)


def check_against_float64(args, groups, H, W, seed, scale=1.0, input_scale=1.0, what=""):
    """The module's ``forward`` (kernel route) against ``v2v_fuse_f64`` per frame; prints the fp32 ``forward_torch`` route's error beside the kernel's."""
    C = args["in_channels"]
    m = fusion_module(args, seed=seed, input_scale=input_scale)
    x = student_t((sum(groups), C, H, W), seed=100 * seed + H, scale=scale) if what.startswith("scale") else torch.randn(sum(groups), C, H, W, generator=torch.Generator().manual_seed(100 * seed + H))
    thetas = [make_thetas(n, H, W, seed=seed + b) for b, n in enumerate(groups)]
    A = affine_of(thetas)
    state = {k: v.clone() for k, v in m.state_dict().items()}
    md = m.to(DEV)
    assert md.kernel_route(C, max(groups))
    with torch.no_grad():
        got = md(x.to(DEV), torch.tensor(groups), A.to(DEV))
        route = md.forward_torch(x.to(DEV), groups, A.to(DEV))
    torch.cuda.synchronize()
    assert got.shape == (len(groups), C, H, W) and bool(torch.isfinite(got).all())
    off, worst = 0, 0.0
    for b, n in enumerate(groups):
        trace = {}
        ref = v2v_fuse_f64(state, x[off:off + n], thetas[b], args, trace=trace)
        assert_not_degenerate(state, x[off:off + n], thetas[b], args, ref, trace, (what, b))
        s = float(ref.abs().max())
        ek, et = float((got[b].cpu().double() - ref).abs().max()) / s, float((route[b].cpu().double() - ref).abs().max()) / s
        print(f"v2v {what} frame {b} (n={n}, {H}x{W}, C={C}): kernel route {ek:.3e}, fp32 torch route {et:.3e} of the scale")
        assert_elementwise(route[b], ref, f"fp32 forward_torch vs float64: {what} frame {b}")
        assert_elementwise(got[b], ref, f"kernel route vs float64: {what} frame {b}")
        worst = max(worst, ek)
        off += n
    assert not ops.sp_range_exceeded(DEV)
    return worst


@pytest.mark.parametrize("agg", ["max", "avg"])
@pytest.mark.parametrize("n", [1, 2, 3, 5, 8])
def test_module_against_float64(n, agg):
    for H, W in SIZES:
        check_against_float64(v2v_args(64, H, W, agg=agg), [n], H, W, seed=n, what=f"{agg} n={n}")


@pytest.mark.parametrize("case", ["C256", "two_layers", "no_gru", "one_iteration", "three_iterations", "batch"])
def test_module_against_float64_more(case):
    H, W = 5, 7
    kw = {"C256": dict(C=256), "two_layers": dict(layers=2), "no_gru": dict(gru=False, agg="avg"), "one_iteration": dict(K=1), "three_iterations": dict(K=3), "batch": {}}[case]
    C = kw.pop("C", 64)
    check_against_float64(v2v_args(C, H, W, **kw), [3, 1] if case == "batch" else [3], H, W, seed=21, what=case)


@pytest.mark.parametrize("scale", [1e-2, 1.0, 1e2])
def test_activation_scales(scale):
    """Student-t maps (heavy tails) at 1e-2, 1 and 1e2: finite, no SplitMap range report, and inside the same bound.  Two modules, because the GRU's outputs are
    below one whatever the input's magnitude: one iteration WITH the GRU and ``input_scale`` compensating (every kernel sees the scaled values, the gate its
    calibrated range), and two iterations WITHOUT it (max, sum and the convolutions are positively homogeneous: the scale travels through both iterations)."""
    H, W = 5, 7
    check_against_float64(v2v_args(64, H, W, K=1), [3], H, W, seed=31, scale=scale, input_scale=scale, what=f"scale {scale:g}, GRU, 1 iteration")
    check_against_float64(v2v_args(64, H, W, gru=False), [3], H, W, seed=32, scale=scale, what=f"scale {scale:g}, no GRU, 2 iterations")


@pytest.mark.parametrize("groups", [[3, 1], [2, 5]])
def test_module_kernel_route_equals_its_torch_route(groups):
    C, H, W = 64, 9, 14
    m = fusion_module(v2v_args(C, H, W), seed=5).to(DEV)
    x = torch.randn(sum(groups), C, H, W, generator=torch.Generator().manual_seed(C)).to(DEV)          # NCHW memory: forward converts
    A = affine_of([make_thetas(n, H, W, seed=40 + n) for n in groups]).to(DEV)
    with torch.no_grad():
        want = m.forward_torch(x, groups, A)
        got = m(x, torch.tensor(groups), A)
        red = m.forward_reduced(x, groups, A)
    assert got.shape == want.shape == (len(groups), C, H, W)
    assert_elementwise(got, want, f"V2VNetFusion.forward (kernel) vs forward_torch, groups={groups}")
    assert_elementwise(red, want, f"forward_reduced vs forward_torch, groups={groups}")
    with pytest.raises(NotImplementedError):
        m(x, groups, A, rows=list(range(sum(groups))))


def test_unsupported_width_takes_the_torch_route():
    H, W = 5, 7
    args = v2v_args(48, H, W)
    m = fusion_module(args, seed=3)
    state = {k: v.clone() for k, v in m.state_dict().items()}
    m = m.to(DEV)
    assert not m.kernel_route(48, 2)
    x, th = torch.randn(2, 48, H, W, generator=torch.Generator().manual_seed(48)), make_thetas(2, H, W, seed=3)
    with torch.no_grad():
        out = m(x.to(DEV), [2], affine_of([th]).to(DEV))
    trace = {}
    ref = v2v_fuse_f64(state, x, th, args, trace=trace)
    assert_not_degenerate(state, x, th, args, ref, trace, "C = 48")
    assert_elementwise(out[0], ref, "C = 48 vs float64")


def test_forward_under_graph_capture():
    C, groups, H, W = 64, [3], 13, 37
    m = fusion_module(v2v_args(C, H, W), seed=9).to(DEV)
    x = nhwc(torch.randn(3, C, H, W, device=DEV))
    A = affine_of([make_thetas(3, H, W, seed=9)]).to(DEV)
    with torch.no_grad():
        m(x, groups, A)                                                     # (weight images packed, workspaces and the range word made: before the capture)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = m(x, groups, A)
        for seed in (1, 2):
            fresh = torch.randn(3, C, H, W, generator=torch.Generator().manual_seed(seed)).to(DEV)
            x.copy_(fresh)
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(out, m(nhwc(fresh), groups, A)), seed


def _mini_world(n_frames):
    h = builtin_config("mini_pointpillar_v2vnet")
    model = build_model(h)
    fill_parameters_(model, seed=0, cls_bias=-1.0)
    v2v_parameters_(model.fusion_net, seed=2)
    with torch.no_grad():
        model.reg_head.weight.mul_(0.01); model.reg_head.bias.zero_(); model.cls_head.weight.mul_(0.05)
    model = model.to(DEV).eval()
    anchors = torch.from_numpy(build_postprocessor(h["postprocess"], False).generate_anchor_box())
    frames = [to_device(make_frame(h, 3, pillars_per_agent=150, seed=40 + i, spread_xy=(4.0, 2.0), spread_yaw=45.0), DEV) for i in range(n_frames)]
    return h, model, anchors, frames


def test_model_heads_and_detections():
    """``mini_pointpillar_v2vnet.yaml``, 3 agents: the heads of the HIP fusion against the same model with its fusion on the op-by-op route; detections of
    ``inference_intermediate_fusion`` equal those of ``FramePipeline`` (eager lanes and captured frames), bit for bit."""
    h, model, anchors, frames = _mini_world(4)
    assert model.fusion_net.kernel_route(model.out_channel, 3)
    with torch.no_grad():
        got = model(frames[0])
        model.fusion_net.force_torch = True
        want = model(frames[0])
        model.fusion_net.force_torch = False
    assert set(got) == {"cls_preds", "reg_preds", "dir_preds"}
    for k in ("cls_preds", "reg_preds", "dir_preds"):
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
