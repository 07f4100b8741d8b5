"""When2com's handshake fusion on the GPU (csrc/w2c_fuse.hip through the C ABI, the convolutions on conv3x3_sp / conv3x3_sp_s2): the score kernel against float64
computed from the very SplitMaps it reads, at map sizes below, at and above the 5 x 7 pool grid; the fuse kernel against float64 with given weights and, one-hot,
against the project's own warp bit for bit; the module's kernel route against the float64 restatement of tests/when2com_reference.py at one to eight agents, at odd
map sizes, in batches and across activation scales; against its own op-by-op route; under graph capture; and at model level (``mini_pointpillar_when2com.yaml``),
eagerly and through ``FramePipeline``.

Weights come from ``synthetic.when2com_parameters_``; every module-level parity test first asserts on the float64 side that the softmax over the agents is
neither uniform nor one-hot (``assert_sees_the_heads``), and holds the fp32 op-by-op route on the same device to the bound before the kernel route.  The bound is
the project's: element-wise rtol 1e-4 + 1e-5 of the output's scale against float64.  Measured on the MI355X: see DESIGN.md section 8h."""
import pytest
import torch
import torch.nn.functional as F

from conftest import assert_elementwise
from coalign_amd import ops
from coalign_amd.config import builtin_config
from coalign_amd.detector import build_model, to_device
from coalign_amd.fusion import When2comFusion
from coalign_amd.inference import inference_intermediate_fusion
from coalign_amd.pipeline import FramePipeline
from coalign_amd.postprocess import build_postprocessor
from coalign_amd.synthetic import fill_parameters_, make_frame, when2com_parameters_
from v2v_reference import make_thetas, student_t
from when2com_reference import assert_sees_the_heads, score_f64, state_f64, weighted_warp_f64, when2com_fuse_f64

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
POOL_SIZES = ((2, 2), (2, 4), (5, 7), (7, 22), (13, 44))      # below the 5 x 7 grid (bins repeat), equal to it, overlapping bins, 13 x 44 (overlapping rows too)


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)


def w2c_args(C, H, W):
    return {"in_channels": C, "H": H, "W": W, "query_size": 32, "key_size": 1024}


_MODULES = {}


def fusion_module(C, H, W, seed, input_scale=1.0, gain=0.2):
    """(module on the CPU in eval mode, its state as float64); built once per key: the module has six million parameters.  ``gain``: the attention linears' gain
    (the logits go with its square); the cases below choose 0.2 or 0.07 so that, on the float64 side, no softmax is uniform or one-hot."""
    key = (C, H, W, seed, input_scale, gain)
    if key not in _MODULES:
        m = When2comFusion(w2c_args(C, H, W))
        when2com_parameters_(m, seed=seed, input_scale=input_scale, attention_gain=gain)
        _MODULES[key] = (m.eval(), state_f64(m.state_dict()))
    return _MODULES[key]


def affine_of(thetas, L=8):
    """[n, n, 2, 3] per frame -> normalized_affine_matrix [B, L, L, 2, 3]."""
    A = torch.zeros(len(thetas), L, L, 2, 3, dtype=torch.float64)
    A[..., 0, 0] = A[..., 1, 1] = 1.0
    for b, th in enumerate(thetas):
        A[b, :th.shape[0], :th.shape[0]] = th
    return A


def head_maps(n, h, w, seed):
    """Key maps [n, 128, h, w] and the query map as SplitMaps: non-negative (they follow a ReLU), of order one, different between agents."""
    g = torch.Generator().manual_seed(seed)
    key = torch.randn(n, 128, h, w, generator=g).abs() * (0.5 + torch.rand(n, 1, 1, 1, generator=g))
    query = torch.randn(1, 128, h, w, generator=g).abs()
    return ops.SplitMap.pack(nhwc(key.to(DEV))), ops.SplitMap.pack(nhwc(query.to(DEV)))


def torch_heads(m, key, query):
    """The fp32 op-by-op heads on the device, on the dense maps."""
    keys, q = m.key_net.fc(m.key_net.avgp(key).view(-1, 4480)).unsqueeze(0), m.query_net.fc(m.query_net.avgp(query).view(-1, 4480)).unsqueeze(0)
    logits = m.attention_net.logits(q, keys).reshape(-1)
    return logits, torch.softmax(logits, dim=0)


@pytest.mark.parametrize("n", [1, 2, 5, 8])
def test_score_against_float64(n):
    """``w2c_score`` against float64 computed from ``dense_reference()`` of the same SplitMaps, every pool regime; the fp32 op-by-op heads first."""
    m, sd = fusion_module(16, 9, 14, seed=30)
    md = When2comFusion(w2c_args(16, 9, 14)).eval()
    md.load_state_dict(m.state_dict())
    md = md.to(DEV)
    params = md.packed()[2]
    for h, w in POOL_SIZES:
        key, query = head_maps(n, h, w, seed=100 * n + h)
        kd, qd = key.dense_reference(), query.dense_reference()
        ref_l, ref_w = score_f64(sd, kd.cpu(), qd.cpu())
        with torch.no_grad():
            tl, tw = torch_heads(md, kd, qd)
            got_w, got_l = ops.w2c_score(key, query, params, return_logits=True)
            again_w, again_l = ops.w2c_score(key, query, params, return_logits=True)
        what = f"n={n}, {h}x{w}"
        el, et = float((got_l.cpu().double() - ref_l).abs().max()), float((tl.cpu().double() - ref_l).abs().max())
        print(f"w2c_score {what}: logits {[round(float(v), 3) for v in ref_l]}, |logit error| kernel {el:.3e}, fp32 torch {et:.3e}; "
              f"weight error kernel {float((got_w.cpu().double() - ref_w).abs().max()):.3e}, fp32 torch {float((tw.cpu().double() - ref_w).abs().max()):.3e}")
        assert_elementwise(tl, ref_l, f"fp32 torch logits vs float64: {what}")
        assert_elementwise(tw, ref_w, f"fp32 torch weights vs float64: {what}")
        assert_elementwise(got_l, ref_l, f"w2c_score logits vs float64: {what}")
        assert_elementwise(got_w, ref_w, f"w2c_score weights vs float64: {what}")
        assert abs(float(got_w.sum()) - 1.0) < 1e-6 and bool((got_w >= 0).all())
        assert torch.equal(got_w, again_w) and torch.equal(got_l, again_l), what            # a fixed summation order: the same bits twice


def test_score_key_vectors_do_not_depend_on_the_agent_count():
    """Five agents' logits equal, bit for bit, those of five single-agent calls with the same query: agent j's key vector never looks at n."""
    m, _ = fusion_module(16, 9, 14, seed=30)
    params = ops.pack_w2c_weights(*[tuple(t.to(DEV) for t in head) for head in m.reduced_weights()[2]])
    for h, w in ((2, 4), (7, 22)):
        key, query = head_maps(5, h, w, seed=7 + h)
        _, together = ops.w2c_score(key, query, params, return_logits=True)
        for j in range(5):
            w1, alone = ops.w2c_score(ops.SplitMap(key.data[j:j + 1]), query, params, return_logits=True)
            assert torch.equal(alone, together[j:j + 1]), (h, w, j)
            assert float(w1) == 1.0


@pytest.mark.parametrize("C", [64, 256])
def test_fuse_against_float64(C):
    """``w2c_fuse`` against float64 with given weights; one agent is warped half outside the map (``make_thetas``).  One-hot weights: the project's own warp of that
    agent (``warp_fuse_nhwc`` in its no-fusion mode), equal element for element."""
    for H, W in ((9, 14), (16, 32)):
        for n in (1, 2, 5, 8):
            g = torch.Generator().manual_seed(C + 10 * n + H)
            x = torch.randn(n, C, H, W, generator=g)
            th = make_thetas(n, H, W, seed=n)[0]
            wts = torch.softmax(torch.randn(n, generator=g), dim=0).float()
            ref = weighted_warp_f64(x, th, wts)
            xd = nhwc(x.to(DEV))
            route = (wts.to(DEV).view(-1, 1, 1, 1) * F.grid_sample(x.to(DEV), F.affine_grid(th.to(DEV), [n, C, H, W], align_corners=False).float(), align_corners=False)).sum(0)
            got = ops.w2c_fuse(xd, th.to(DEV), wts.to(DEV))
            assert got.shape == (1, C, H, W) and ops.nhwc_memory(got)
            assert_elementwise(route, ref, f"fp32 torch weighted warp vs float64: C={C}, {H}x{W}, n={n}")
            assert_elementwise(got[0], ref, f"w2c_fuse vs float64: C={C}, {H}x{W}, n={n}")
            warped = ops.warp_fuse_nhwc([xd], th.to(DEV), ops.FUSE_NONE)[0]
            for k in sorted({0, n - 1, n // 2}):
                hot = torch.zeros(n, device=DEV)
                hot[k] = 1.0
                assert torch.equal(ops.w2c_fuse(xd, th.to(DEV), hot)[0], warped[k]), (C, H, W, n, k)


def check_against_float64(C, groups, H, W, seed, scale=1.0, input_scale=1.0, what="", gain=0.07):
    """The module's kernel route against ``when2com_fuse_f64`` per frame, the fp32 ``forward_torch`` route on the same device first; prints both errors."""
    m, sd = fusion_module(C, H, W, seed, input_scale, gain)
    shape = (sum(groups), C, H, W)
    x = student_t(shape, seed=100 * seed + H, scale=scale) if what.startswith("scale") else torch.randn(shape, generator=torch.Generator().manual_seed(100 * seed + H))
    thetas = [make_thetas(n, H, W, seed=seed + b) for b, n in enumerate(groups)]
    A = affine_of(thetas)
    md = When2comFusion(w2c_args(C, H, W)).eval()
    md.load_state_dict(m.state_dict())
    md = md.to(DEV)
    assert md.kernel_route(C, max(groups)) and md.kernel_shape_reason(C, max(groups)) is None
    details = []
    with torch.no_grad():
        got = md.forward_kernels(x.to(DEV), groups, A.to(DEV), details)
        route = md.forward_torch(x.to(DEV), groups, A.to(DEV))
    torch.cuda.synchronize()
    assert got.shape == (len(groups), C, H, W) and bool(torch.isfinite(got).all())
    off, worst = 0, 0.0
    for b, n in enumerate(groups):
        ref, logits, w = when2com_fuse_f64(sd, x[off:off + n], thetas[b][0])
        assert_sees_the_heads(w, (what, b))
        s = float(ref.abs().max())
        ek, et = float((got[b].cpu().double() - ref).abs().max()) / s, float((route[b].cpu().double() - ref).abs().max()) / s
        ew = float((details[b][1].cpu().double() - w).abs().max())
        print(f"when2com {what} frame {b} (n={n}, {H}x{W}, C={C}): kernel route {ek:.3e}, fp32 torch route {et:.3e} of the scale; logits {[round(float(v), 2) for v in logits]}, "
              f"weights {[round(float(v), 3) for v in w]}, kernel weight error {ew:.3e}")
        assert_elementwise(route[b], ref, f"fp32 forward_torch vs float64: {what} frame {b}")
        assert_elementwise(got[b], ref, f"kernel route vs float64: {what} frame {b}")
        worst = max(worst, ek)
        off += n
    assert not ops.sp_range_exceeded(DEV)
    return worst


@pytest.mark.parametrize("n", [1, 2, 3, 5, 8])
def test_module_against_float64(n):
    check_against_float64(64, [n], 16, 32, seed=n, what=f"n={n}")


@pytest.mark.parametrize("case", ["odd_25x44", "C256", "batch_3_1", "batch_2_5"])
def test_module_against_float64_more(case):
    """25 x 44: the odd sizes 25 -> 13 -> 7 -> 4 and 44 -> 22 -> 11 -> 6 pass through every strided layer; C = 256 with five agents; two batches."""
    C, groups, H, W, seed = {"odd_25x44": (64, [3], 25, 44, 11), "C256": (256, [5], 16, 32, 12), "batch_3_1": (64, [3, 1], 16, 32, 13), "batch_2_5": (64, [2, 5], 16, 32, 14)}[case]
    check_against_float64(C, groups, H, W, seed=seed, what=case, gain=0.2 if case in ("odd_25x44", "batch_3_1") else 0.07)


@pytest.mark.parametrize("scale", [1e-2, 1.0, 1e2])
def test_activation_scales(scale):
    """Student-t maps (heavy tails) at 1e-2, 1 and 1e2 with ``input_scale`` compensating in the first convolution: the warp, the split and the weighted sum see the
    scaled values, the logits -- quadratic in the feature scale -- stay of order one.  Finite, no SplitMap range report, inside the same bound."""
    check_against_float64(64, [3], 16, 32, seed=21, scale=scale, input_scale=scale, what=f"scale {scale:g}")


def test_one_agent_frame_is_the_warp_of_its_map():
    C, H, W = 64, 9, 14
    m, _ = fusion_module(C, H, W, seed=5)
    md = When2comFusion(w2c_args(C, H, W)).eval()
    md.load_state_dict(m.state_dict())
    md = md.to(DEV)
    x = nhwc(torch.randn(1, C, H, W, generator=torch.Generator().manual_seed(1)).to(DEV))
    th = torch.tensor([[[1.0, 0.05, 0.21], [-0.04, 1.0, -0.13]]], dtype=torch.float64)
    A = affine_of([th[None]]).to(DEV)
    with torch.no_grad():
        got = md(x, [1], A)
    assert torch.equal(got, ops.warp_fuse_nhwc([x], th.to(DEV), ops.FUSE_NONE)[0])
    assert not torch.equal(got, x)                                                      # (the ego is warped too: the row is not the identity here)


def test_unsupported_width_takes_the_torch_route():
    C, H, W = 24, 9, 14
    m, sd = fusion_module(C, H, W, seed=3, gain=0.2)
    md = When2comFusion(w2c_args(C, H, W)).eval()
    md.load_state_dict(m.state_dict())
    md = md.to(DEV)
    assert not md.kernel_route(C, 2) and "C % 16" in md.kernel_shape_reason(C, 2)
    assert "agents" in When2comFusion(w2c_args(32, H, W)).eval().kernel_shape_reason(32, 9)
    x, th = torch.randn(2, C, H, W, generator=torch.Generator().manual_seed(24)), make_thetas(2, H, W, seed=3)
    with torch.no_grad():
        out = md(x.to(DEV), [2], affine_of([th]).to(DEV))
    ref, _, w = when2com_fuse_f64(sd, x, th[0])
    assert_sees_the_heads(w, "C = 24")
    assert_elementwise(out[0], ref, "C = 24 vs float64")


@pytest.mark.parametrize("groups", [[3, 1], [2, 5]])
def test_module_kernel_route_equals_its_torch_route(groups, monkeypatch):
    C, H, W = 64, 9, 14
    m, _ = fusion_module(C, H, W, seed=5)
    md = When2comFusion(w2c_args(C, H, W)).eval()
    md.load_state_dict(m.state_dict())
    md = md.to(DEV)
    x = torch.randn(sum(groups), C, H, W, generator=torch.Generator().manual_seed(C)).to(DEV)          # NCHW memory: forward converts
    A = affine_of([make_thetas(n, H, W, seed=40 + n) for n in groups]).to(DEV)
    launches, fuse = [], ops.w2c_fuse
    monkeypatch.setattr(ops, "w2c_fuse", lambda *a: launches.append(1) or fuse(*a))
    with torch.no_grad():
        want = md.forward_torch(x, groups, A)
        got = md(x, torch.tensor(groups), A)
        assert len(launches) == len(groups)                                             # one fuse launch per frame: the kernel route ran
        red = md.forward_reduced(x, groups, A)
        md.force_torch = True
        forced = md(x, groups, A)
        md.force_torch = False
        assert len(launches) == len(groups)                                             # ... and force_torch keeps off it
    assert got.shape == want.shape == (len(groups), C, H, W)
    assert_elementwise(forced, want, f"force_torch vs forward_torch, groups={groups}")      # (the library's convolutions do not repeat to the bit between two calls)
    assert_elementwise(got, want, f"When2comFusion.forward (kernel) vs forward_torch, groups={groups}")
    assert_elementwise(red, want, f"forward_reduced vs forward_torch, groups={groups}")
    with pytest.raises(NotImplementedError):
        md(x, groups, A, rows=list(range(sum(groups))))


def test_forward_under_graph_capture():
    C, groups, H, W = 64, [3], 13, 37
    m, _ = fusion_module(C, H, W, seed=9)
    md = When2comFusion(w2c_args(C, H, W)).eval()
    md.load_state_dict(m.state_dict())
    md = md.to(DEV)
    x = nhwc(torch.randn(3, C, H, W, device=DEV))
    A = affine_of([make_thetas(3, H, W, seed=9)]).to(DEV)
    with torch.no_grad():
        md(x, groups, A)                                                    # (weight images packed, workspaces and the range word made: before the capture)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = md(x, groups, A)
        for seed in (1, 2):
            fresh = torch.randn(3, C, H, W, generator=torch.Generator().manual_seed(seed)).to(DEV)
            x.copy_(fresh)
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(out, md(nhwc(fresh), groups, A)), seed


def _mini_world(n_frames):
    h = builtin_config("mini_pointpillar_when2com")
    model = build_model(h)
    fill_parameters_(model, seed=0, cls_bias=-1.0)
    when2com_parameters_(model.fusion_net, seed=2)
    with torch.no_grad():
        model.reg_head.weight.mul_(0.01); model.reg_head.bias.zero_(); model.cls_head.weight.mul_(0.05)
    model = model.to(DEV).eval()
    anchors = torch.from_numpy(build_postprocessor(h["postprocess"], False).generate_anchor_box())
    frames = [to_device(make_frame(h, 3, pillars_per_agent=150, seed=40 + i, spread_xy=(4.0, 2.0), spread_yaw=45.0), DEV) for i in range(n_frames)]
    return h, model, anchors, frames


def test_model_heads_and_detections():
    """``mini_pointpillar_when2com.yaml``, 3 agents: the heads of the HIP fusion against the same model with its fusion on the op-by-op route; detections of
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
