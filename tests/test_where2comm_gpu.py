"""Where2comm on the GPU (csrc/w2comm.hip through the C ABI): the mask kernel against float64 with ``torch.equal`` -- every test's inputs come from
``where2comm_reference.mask_case``, which asserts in float64 that the masks are mixed and that no smoothed confidence lies within 2e-5 of the threshold --; the
masked fusion kernel's two exact properties (all-ones masks = ``warp_fuse_nhwc``; 0 / 1 masks = ``warp_fuse_nhwc`` on maps multiplied beforehand), with ``rows``, and
against float64; the module's kernel route against its op-by-op route and float64, single and multi scale, and under graph capture; the model
(``mini_pointpillar_where2comm.yaml``) eagerly and through ``FramePipeline``.  The bound against float64 is the project's: element-wise rtol 1e-4 + 1e-5 of the
output's scale, with the fp32 op-by-op route on the same device held to it first."""
import copy

import pytest
import torch

from conftest import assert_elementwise
from coalign_amd import ops
from coalign_amd.backbone import ResNetBEVBackbone
from coalign_amd.config import builtin_config
from coalign_amd.detector import build_model, to_device
from coalign_amd.fusion import Where2commFusion
from coalign_amd.inference import inference_intermediate_fusion
from coalign_amd.pipeline import FramePipeline
from coalign_amd.postprocess import build_postprocessor
from coalign_amd.synthetic import fill_parameters_, make_frame
from coalign_amd.where2comm import AttenFusion, MaxFusion, _warp_torch
from v2v_reference import make_thetas, student_t
from where2comm_reference import check_mask_inputs, mask_case, masks_f64, rate_of, single_scale_masks, where2comm_levels_f64

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LEVELS = ((64, 16, 32), (128, 8, 16), (256, 4, 8))
MODES = {"ATTEN": ops.FUSE_ATT, "MAX": ops.FUSE_MAX}


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)


def dev(t):
    return None if t is None else t.to(DEV)


# ---- the mask kernel -------------------------------------------------------------------------------------------------------------------------------------------------
def run_masks(n_total, A, H, W, k, groups, levels, bias=0.0, seed=50):
    psm, w, b, thre = mask_case(n_total, A, H, W, k, bias=bias, seed=seed)          # asserts the two conditions in float64
    masks, rates = ops.w2comm_masks(dev(psm), groups, dev(w), dev(b), thre, levels=levels)
    want, want_rates = masks_f64(psm, groups, w, b, thre, levels=levels)
    assert len(masks) == levels
    for l, (g, r) in enumerate(zip(masks, want)):
        assert g.dtype == torch.uint8 and tuple(g.shape) == (n_total, H >> l, W >> l)
        assert torch.equal(g.cpu(), r), (l, int((g.cpu() != r).sum()))
    assert torch.equal(rates.cpu(), want_rates), (rates.cpu().tolist(), want_rates.tolist())
    assert float(rate_of(rates.cpu())) == float(rate_of(want_rates))


@pytest.mark.parametrize("k", [0, 3, 5])
@pytest.mark.parametrize("H,W,levels", [(3, 4, 1), (9, 14, 3), (16, 32, 3), (25, 88, 3)])
def test_masks_sizes_and_kernels(H, W, levels, k):
    """3 x 4 is smaller than the 5 x 5 kernel; 9 x 14 pools to 4 x 7 and 2 x 3 (floor); 25 x 88 spans two tiles across; frames of 3, 1 and 2 agents."""
    run_masks(6, 2, H, W, k, [3, 1, 2], levels, bias=0.02 if k else 0.0)


@pytest.mark.parametrize("A", [1, 2, 3])
@pytest.mark.parametrize("groups", [[1], [2], [3, 1, 2], [8]])
@pytest.mark.parametrize("levels", [1, 3])
def test_masks_anchors_groups_levels(A, groups, levels):
    run_masks(sum(groups), A, 9, 14, 5, groups, levels, bias=-0.015, seed=60)


@pytest.mark.parametrize("k", [1, 7, 9])
def test_masks_other_kernel_sizes(k):
    """Every odd size up to the kernel's limit of 9 (a 9 x 9 kernel on 9 x 14 covers the map's whole height)."""
    run_masks(4, 2, 9, 14, k, [3, 1], 3, bias=0.01)


def test_masks_two_tiles_down():
    """More rows than a tile has (32): the second tile row's halo reads the first's pixels."""
    run_masks(2, 2, 41, 70, 5, [2], 3)


# ---- the fusion kernel -----------------------------------------------------------------------------------------------------------------------------------------------
def fuse_inputs(shapes, n, seed):
    g = torch.Generator().manual_seed(seed)
    xs = [nhwc(student_t((n, C, H, W), seed + i).to(DEV)) for i, (C, H, W) in enumerate(shapes)]
    masks = [(torch.rand(n, H, W, generator=g) < 0.55).to(torch.uint8).to(DEV) for _, H, W in shapes]
    theta = make_thetas(n, shapes[0][1], shapes[0][2], seed=seed)[0].to(DEV)
    return xs, masks, theta


def torch_fuse(xs, masks, theta, mode):
    """The fp32 op-by-op route on the device: x * mask, warp, fuse (the module's own parts)."""
    out = []
    for x, mk in zip(xs, masks):
        v = _warp_torch(x * mk.unsqueeze(1).float(), theta)
        out.append((AttenFusion(x.shape[1]) if mode == "ATTEN" else MaxFusion())(v).unsqueeze(0))
    return out


@pytest.mark.parametrize("mode", ["ATTEN", "MAX"])
@pytest.mark.parametrize("n", [1, 2, 5, 8])
@pytest.mark.parametrize("shapes", [LEVELS, ((64, 9, 14),), ((128, 9, 14),), ((256, 9, 14),)], ids=["three-levels", "odd-64", "odd-128", "odd-256"])
def test_fuse_exact_properties_rows_and_float64(shapes, n, mode):
    xs, masks, theta = fuse_inputs(shapes, n, seed=7 * n + len(shapes))
    ones = [torch.ones_like(m) for m in masks]
    plain = ops.warp_fuse_nhwc(xs, theta, MODES[mode])
    got1 = ops.w2comm_fuse_nhwc(xs, ones, theta, MODES[mode])
    for a, b in zip(got1, plain):
        assert torch.equal(a, b), "all-ones masks must give warp_fuse_nhwc's bits"
    pre = ops.warp_fuse_nhwc([nhwc(x * m.unsqueeze(1).float()) for x, m in zip(xs, masks)], theta, MODES[mode])
    got = ops.w2comm_fuse_nhwc(xs, masks, theta, MODES[mode])
    for a, b, p in zip(got, pre, plain):
        assert torch.equal(a, b), "0 / 1 masks must give warp_fuse_nhwc's bits on the maps multiplied beforehand"
        assert n == 1 or not torch.equal(a, p)                                        # (the masks are seen)
    rows = [(3 * i + 1) % n for i in range(n)] if n in (2, 5, 8) else list(range(n))          # a permutation: 3 is coprime to 2, 5 and 8
    inv = sorted(range(n), key=lambda r: rows[r])                                    # physical row r holds logical agent inv[r]
    routed = ops.w2comm_fuse_nhwc([nhwc(x[inv]) for x in xs], [m[inv].contiguous() for m in masks], theta, MODES[mode], rows=rows)
    for a, b in zip(routed, got):
        assert torch.equal(a, b), "rows"
    ref = where2comm_levels_f64([x.cpu() for x in xs], [m.cpu() for m in masks], [n], theta.cpu().unsqueeze(0).unsqueeze(0), mode)
    for t, a, r in zip(torch_fuse(xs, masks, theta, mode), got, ref):
        assert_elementwise(t, r, f"fp32 op by op vs float64, {mode}, n={n}")
        assert_elementwise(a, r, f"w2comm_fuse_nhwc vs float64, {mode}, n={n}")


# ---- the module ------------------------------------------------------------------------------------------------------------------------------------------------------
def affine_of(thetas, L=8):
    A = torch.zeros(len(thetas), L, L, 2, 3, dtype=torch.float64)
    A[..., 0, 0] = A[..., 1, 1] = 1.0
    for b, th in enumerate(thetas):
        A[b, :th.shape[0], :th.shape[0]] = th
    return A


def module_of(mode, multi_scale, thre, C=64):
    args = {"voxel_size": [0.4, 0.4, 4], "downsample_rate": 1, "multi_scale": multi_scale, "agg_operator": {"mode": mode, "feature_dim": C},
            "communication": {"thre": thre, "gaussian_smooth": {"k_size": 5, "c_sigma": 1.0}}}
    if multi_scale:
        args.update(layer_nums=[1, 1, 1], num_filters=[64, 128, 256])
    return Where2commFusion(args).eval().to(DEV)


def count_calls(monkeypatch, name):
    calls, fn = [], getattr(ops, name)
    monkeypatch.setattr(ops, name, lambda *a, **k: calls.append(1) or fn(*a, **k))
    return calls


@pytest.mark.parametrize("mode", ["ATTEN", "MAX"])
def test_module_single_scale(mode, monkeypatch):
    C, H, W, groups = 64, 9, 14, [3, 1]
    psm, w, b, thre = mask_case(4, 2, H, W, 5, seed=70)
    m = module_of(mode, False, thre)
    x = student_t((4, C, H, W), 71).to(DEV)                                           # NCHW memory: fuse converts
    A = affine_of([make_thetas(n, H, W, seed=40 + n) for n in groups]).to(DEV)
    fuse_calls, mask_calls = count_calls(monkeypatch, "w2comm_fuse_nhwc"), count_calls(monkeypatch, "w2comm_masks")
    with torch.no_grad():
        got, rate, extra = m.fuse(x, dev(psm), groups, A)
        assert len(fuse_calls) == len(groups) and len(mask_calls) == 1 and extra == {}      # the kernel route ran: one mask launch, one fusion launch per frame
        want, want_rate, _ = m.forward_torch(x, dev(psm), groups, A)
        m.force_torch = True
        forced, _, _ = m.fuse(x, dev(psm), groups, A)
        assert len(fuse_calls) == len(groups)
    masks, rates = masks_f64(psm, groups, w, b, thre)
    ref = where2comm_levels_f64([x.cpu()], [single_scale_masks(masks[0], groups)], groups, A.cpu(), mode)[0]
    assert_elementwise(want, ref, f"forward_torch vs float64, {mode}")
    assert_elementwise(forced, ref, f"force_torch vs float64, {mode}")
    assert_elementwise(got, ref, f"kernel route vs float64, {mode}")
    assert_elementwise(got, want, f"kernel route vs forward_torch, {mode}")
    assert rate.dim() == 0 and rate.is_cuda and float(rate) == float(want_rate) == float(rate_of(rates))


def level_maps(n, seed):
    return [nhwc(student_t((n, C, H, W), seed + i).to(DEV)) for i, (C, H, W) in enumerate(LEVELS)]


def decode_backbone():
    cfg = {"layer_nums": [1, 1, 1], "layer_strides": [1, 2, 2], "num_filters": [64, 128, 256], "upsample_strides": [1, 2, 4], "num_upsample_filter": [32, 32, 32]}
    bb = ResNetBEVBackbone(cfg, 64)
    fill_parameters_(bb, seed=3)
    return bb.eval()


@pytest.mark.parametrize("mode", ["ATTEN", "MAX"])
def test_module_multi_scale(mode, monkeypatch):
    """The levels enter through the internal entry point (``feats``), as the model hands them over; the backbone serves the up-sampling heads."""
    groups = [3, 1]
    psm, w, b, thre = mask_case(4, 2, 16, 32, 5, seed=72)
    m = module_of(mode, True, thre)
    bb = decode_backbone()
    bbd = copy.deepcopy(bb).to(DEV)
    xs = level_maps(4, 73)
    A = affine_of([make_thetas(n, 16, 32, seed=50 + n) for n in groups]).to(DEV)
    fuse_calls = count_calls(monkeypatch, "w2comm_fuse_nhwc")
    with torch.no_grad():
        levels, rate = m.fuse(None, dev(psm), groups, A, bbd, feats=xs, decode=False)
        assert isinstance(levels, list) and len(fuse_calls) == len(groups)
        got, rate2, _ = m.fuse(None, dev(psm), groups, A, bbd, feats=xs)
        want, want_rate, _ = m.forward_torch(None, dev(psm), groups, A, bbd, feats=xs)
    masks, rates = masks_f64(psm, groups, w, b, thre, levels=3)
    ref = where2comm_levels_f64([x.cpu() for x in xs], masks, groups, A.cpu(), mode)
    for l, (a, r) in enumerate(zip(levels, ref)):
        assert_elementwise(a, r, f"level {l} vs float64, {mode}")
    with torch.no_grad():
        ref_out = bb.double().decode_multiscale_feature(ref)
    assert tuple(got.shape) == (2, 96, 16, 32)
    assert_elementwise(want, ref_out, f"forward_torch vs float64, {mode}")
    assert_elementwise(got, ref_out, f"kernel route vs float64, {mode}")
    assert_elementwise(got, want, f"kernel route vs forward_torch, {mode}")
    assert float(rate) == float(rate2) == float(want_rate) == float(rate_of(rates))


def test_module_without_communication_is_the_plain_fusion():
    args = {"voxel_size": [0.4, 0.4, 4], "downsample_rate": 1, "multi_scale": True, "agg_operator": {"mode": "ATTEN", "feature_dim": 64}, "layer_nums": [1, 1, 1],
            "num_filters": [64, 128, 256]}
    m = Where2commFusion(args).eval().to(DEV)
    xs = level_maps(3, 75)
    A = affine_of([make_thetas(3, 16, 32, seed=5)]).to(DEV)
    levels, rate = m.fuse(None, None, [3], A, decode_backbone().to(DEV), feats=xs, decode=False)
    for a, b in zip(levels, ops.warp_fuse_nhwc(xs, A[0, 0, :3], ops.FUSE_ATT)):
        assert torch.equal(a, b)
    assert rate.dtype == torch.int64 and int(rate) == 0 and rate.is_cuda


@pytest.mark.parametrize("multi_scale", [False, True])
def test_module_under_graph_capture(multi_scale):
    groups = [3]
    H, W = (16, 32) if multi_scale else (9, 14)
    psm, _, _, thre = mask_case(3, 2, H, W, 5, seed=76)
    m = module_of("ATTEN", multi_scale, thre)
    bb = decode_backbone().to(DEV) if multi_scale else None
    xs = level_maps(3, 77) if multi_scale else [nhwc(student_t((3, 64, H, W), 77).to(DEV))]
    A = affine_of([make_thetas(3, H, W, seed=9)]).to(DEV)
    p = dev(psm)

    def run():
        if multi_scale:
            lv, rate = m.fuse(None, p, groups, A, bb, feats=xs, decode=False)
            return [*lv, rate]
        out, rate, _ = m.fuse(xs[0], p, groups, A)
        return [out, rate]

    with torch.no_grad():
        run()
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            outs = run()
        for seed in (1, 2):
            for x in xs:
                x.copy_(nhwc(student_t(tuple(x.shape), 100 * seed + x.shape[1]).to(DEV)))
            p.copy_(2 * torch.randn(p.shape, generator=torch.Generator().manual_seed(seed)).to(DEV) - 2)
            graph.replay()
            torch.cuda.synchronize()
            for a, b in zip(outs, run()):
                assert torch.equal(a, b), seed


# ---- the model -------------------------------------------------------------------------------------------------------------------------------------------------------
def _mini_world(n_frames):
    """``mini_pointpillar_where2comm.yaml`` with synthetic weights and the first ``n_frames`` synthetic frames (seeds from 40 on) whose single-agent logits meet the
    mask tests' two conditions in float64 at the yaml's threshold."""
    h = builtin_config("mini_pointpillar_where2comm")
    model = build_model(h)
    fill_parameters_(model, seed=0, cls_bias=-1.0)
    comm = model.fusion_net.naive_communication
    comm.init_gaussian_filter(5, 1.0)                                                 # (fill_parameters_ fills by name: the filter is the reference's formula again)
    with torch.no_grad():
        model.reg_head.weight.mul_(0.01); model.reg_head.bias.zero_(); model.cls_head.weight.mul_(0.05)
    model = model.to(DEV).eval()
    anchors = torch.from_numpy(build_postprocessor(h["postprocess"], False).generate_anchor_box())
    frames = []
    w, b = comm.gaussian_filter.weight.detach().cpu().reshape(5, 5), comm.gaussian_filter.bias.detach().cpu()
    for seed in range(40, 104):
        f = to_device(make_frame(h, 3, pillars_per_agent=150, seed=seed, spread_xy=(4.0, 2.0), spread_yaw=45.0), DEV)
        with torch.no_grad():
            psm = model.encode(f)[0][-1]
        try:
            check_mask_inputs(psm.cpu(), w, b, comm.thre)
        except AssertionError:
            continue
        frames.append(f)
        if len(frames) == n_frames:
            break
    assert len(frames) == n_frames, "too few synthetic frames with mixed, decided masks at the config's threshold"
    return h, model, anchors, frames, (w, b, comm.thre)


def test_model_heads_rates_and_detections(monkeypatch):
    h, model, anchors, frames, (w, b, thre) = _mini_world(4)
    assert model.kernel_route(3)
    fuse_calls = count_calls(monkeypatch, "w2comm_fuse_nhwc")
    with torch.no_grad():
        feats, affine = model.encode(frames[0])
        got = model(frames[0])
        assert len(fuse_calls) == 1                                                    # the kernel route ran
        model.fusion_net.force_torch = True
        want = model(frames[0])
        model.fusion_net.force_torch = False
        assert len(fuse_calls) == 1
    assert set(got) == {"cls_preds", "reg_preds", "dir_preds", "comm_rates"}
    *maps, psm = feats
    assert tuple(psm.shape[2:]) == tuple(maps[0].shape[2:]) == (16, 32)
    # the float64 side from the encoder's maps on: masks, fusion of the three levels, up-sampling heads, shrink header, heads
    masks, rates = masks_f64(psm.cpu(), [3], w, b, thre, levels=3)
    fused = where2comm_levels_f64([m.cpu() for m in maps], masks, [3], affine.cpu(), "ATTEN")
    ref = copy.deepcopy(model).cpu().double().eval()
    with torch.no_grad():
        x = ref.shrink_conv(ref.backbone.decode_multiscale_feature(fused))
        ref_out = {"cls_preds": ref.cls_head(x), "reg_preds": ref.reg_head(x), "dir_preds": ref.dir_head(x)}
    for k in ("cls_preds", "reg_preds", "dir_preds"):
        assert_elementwise(want[k], ref_out[k], f"{k}: op-by-op fusion vs float64")
        assert_elementwise(got[k], ref_out[k], f"{k}: HIP fusion vs float64")
    assert got["comm_rates"].dim() == 0 and got["comm_rates"].is_cuda
    assert float(got["comm_rates"]) == float(want["comm_rates"]) == float(rate_of(rates))
    assert 0.2 <= float(got["comm_rates"]) <= 0.8
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
