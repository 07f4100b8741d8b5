"""The pose-robust V2VNet on the GPU (csrc/v2v_robust.hip through the C ABI, the convolutions on conv3x3_sp / conv3x3_sp_s2): the pooling tail and the weighted
aggregation bit for bit against torch arithmetic, the two heads against float64 of the same inputs, the EM kernel against the float64 yardstick of
tests/v2v_robust_reference.py, the model's kernel route per stage and end to end against the yardstick and against its own op-by-op route, under graph capture, and at
model level (``mini_pointpillar_v2vnet_robust.yaml``).

Shapes: C = hidden = 64, one to eight agents, maps of 24 x 24 (the minimum) and 25 x 41 (floor cropping at every pooling, no multiple of any tile).  Weights come from
``synthetic.v2v_robust_parameters_``; every parity test first asserts on the float64 side that every part is visible (``assert_robust_not_degenerate``).

Bounds.  Maps computed from the yardstick's own thetas and weights: the project's V2VNet bound, rtol 1e-4 + 1e-5 of the scale (``assert_elementwise``).  Quantities that
pass through learned poses or the EM: 4 x E32, where E32 is the error of the float32 ``forward_torch`` route against the float64 yardstick on the same cases,
measured on the CPU (worst of the ten cases; tests/test_v2v_robust_cpu.py re-measures one).  The margin of 4 covers other summation orders and the 22-bit
convolution operands; it stays two orders of magnitude under the non-degeneracy guards.  Measured on the MI355X: see DESIGN.md section 8i."""
import pytest
import torch
import torch.nn.functional as F

from conftest import assert_elementwise
from coalign_amd import ops
from coalign_amd.config import builtin_config
from coalign_amd.detector import build_model, to_device
from coalign_amd.inference import inference_intermediate_fusion
from coalign_amd.postprocess import build_postprocessor
from coalign_amd.synthetic import fill_parameters_, make_frame, v2v_robust_parameters_
from v2v_reference import make_thetas
from v2v_robust_cases import AGENTS, MAX_CAV, SIZES, case, errors, maps_for, model_for, poses_for
from v2v_robust_reference import (assert_robust_not_degenerate, fuse_weight_f64, normalize_f64, pairwise_f64, robust_frame_f64, tfm_f64, weighted_em_f64)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
POOL_SIZES = ((2, 2), (5, 7), (13, 37))

# E32: max |float32 forward_torch - float64 yardstick| over the ten cases (SIZES x AGENTS), CPU.  Poses in m / degrees, scores and weights absolute, head maps
# relative to the yardstick's largest magnitude.  Beside each line: the worst figure of the kernel route and of ``forward_torch`` measured on the MI355X, same cases.
E32 = {
    "pairwise_corr": 4.45e-6,           # kernel route 1.85e-6, forward_torch on the GPU 3.96e-6
    "lidar_pose_corrected": 8.18e-6,    # kernel route 6.41e-7, forward_torch on the GPU 9.32e-6
    "scores": 1.88e-6,                  # kernel route 6.88e-7, forward_torch on the GPU 2.33e-6
    "weight": 6.84e-7,                  # kernel route 2.67e-7, forward_torch on the GPU 8.62e-7
    "cls_preds": 1.86e-7,               # kernel route 1.21e-7, forward_torch on the GPU 1.92e-7
    "reg_preds": 8.55e-7,               # kernel route 4.80e-7, forward_torch on the GPU 8.47e-7
}
MARGIN = 4.0
BOUNDS = {k: MARGIN * v for k, v in E32.items()}


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)


def lrelu(t):
    return F.leaky_relu(t, 0.01)


def test_pool_act_is_the_stated_arithmetic_bit_for_bit():
    """lrelu(max_pool2d(a + e)) -- with e, without, both output kinds, one to three agents; signed zeros, blocks of negative values only and a block of equal
    values are planted in every map."""
    C = 64
    for H, W in POOL_SIZES:
        for n in (1, 2, 3):
            g = torch.Generator().manual_seed(H + 10 * n)
            a = torch.randn(n * n, C, H, W, generator=g)
            e = torch.randn(n, C, H, W, generator=g)
            a[:, 0::4, :2, :2] = -a[:, 0::4, :2, :2].abs() - 0.5            # negative-only blocks (the ego term below is zeroed there)
            a[:, 1::4, 0, 0], a[:, 1::4, 0, 1], a[:, 1::4, 1, 0], a[:, 1::4, 1, 1] = -0.0, 0.0, -0.0, -1.0
            a[:, 2::4, 0, 0], a[:, 2::4, 0, 1], a[:, 2::4, 1, 0], a[:, 2::4, 1, 1] = 0.0, -0.0, -2.0, 0.0
            a[:, 3::4, :2, :2] = 0.25
            e[:, :, :2, :2] = 0.0
            a, e = nhwc(a.to(DEV)), nhwc(e.to(DEV))
            for ego in (e, None):
                v = a if ego is None else (a.view(n, n, C, H, W) + ego.unsqueeze(1)).flatten(0, 1)
                want = nhwc(lrelu(F.max_pool2d(v, 2)))
                assert bool((want[:, 0::4, 0, 0] < 0).all()) and want.shape == (n * n, C, H // 2, W // 2)
                sp = ops.v2vr_pool_act(a, ego, n)
                plain = ops.v2vr_pool_act(a, ego, n, out_split=False)
                assert sp.shape == want.shape and ops.nhwc_memory(plain)
                assert torch.equal(plain.view(torch.int32), want.view(torch.int32)), (H, W, n, ego is None)      # (bit patterns: -0.0 is not +0.0)
                assert torch.equal(sp.data, ops.SplitMap.pack(want).data), (H, W, n, ego is None)


def test_aggregate_is_the_torch_loop_bit_for_bit():
    """(a + e) * mask * w_ij summed in order of j, both output kinds; a sender wholly outside the map (n >= 4) and a zero weight are included."""
    C = 64
    for H, W in ((5, 7), (13, 37)):
        for n in AGENTS:
            g = torch.Generator().manual_seed(3 * n + W)
            th = make_thetas(n, H, W, seed=10 + n).to(DEV)
            x = nhwc(torch.randn(n, C, H, W, generator=g).to(DEV))
            ones = nhwc(torch.ones(n, 64, H, W, device=DEV))
            wt = torch.rand(MAX_CAV, MAX_CAV, generator=g).to(DEV)
            wt[0, n - 1] = 0.0
            for R in sorted({n, 1}):
                a = nhwc(torch.randn(R * n, C, H, W, generator=g).to(DEV))
                e = nhwc(torch.randn(R, C, H, W, generator=g).to(DEV))
                mask = torch.stack([ops.warp_fuse_nhwc([ones], th[i], ops.FUSE_NONE)[0][:, :1] for i in range(R)])
                m = (a.view(R, n, C, H, W) + e.unsqueeze(1)) * mask
                want = m[:, 0] * wt[:R, 0].view(R, 1, 1, 1)
                for j in range(1, n):
                    want = want + m[:, j] * wt[:R, j].view(R, 1, 1, 1)
                plain = ops.v2vr_aggregate(a, e, x, th[:R], wt, gru=False)
                split = ops.v2vr_aggregate(a, e, x, th[:R], wt, gru=True)
                assert torch.equal(plain, x[:R] + want), (H, W, n, R)
                assert torch.equal(split.data, ops.SplitMap.pack(nhwc(torch.cat([x[:R], want], dim=1))).data), (H, W, n, R)
            if n >= 4:
                assert bool((mask[0, n - 2] == 0).all())


def test_score_head_against_float64():
    """The cropped global max, LeakyReLU, the linear layer, the sigmoid and the weights against float64 of the same inputs.  Bound: the max is exact; the h-term
    dot product in float32 errs by at most h 2^-24 sum |w m|, the sigmoid's slope is at most 1 / 4, plus its own and the division's roundings."""
    h = 64
    for H, W in ((4, 4), (5, 7), (12, 20)):
        for n, L in ((1, 5), (3, 5), (8, 8)):
            g = torch.Generator().manual_seed(H + n)
            y = torch.randn(n * n, h, H, W, generator=g) * 2
            y[0, :8] = -y[0, :8].abs()                                      # channels whose maximum is negative: the LeakyReLU's other branch
            y[:, :, H // 2 * 2:, :] += 50.0                                 # rows and columns the pooling crops must not be seen
            y[:, :, :, W // 2 * 2:] += 50.0
            w, b, alpha = torch.randn(h, generator=g) * 0.1, torch.tensor([0.05]), torch.tensor([0.15])
            scores, weight = ops.v2vr_score_head(nhwc(y.to(DEV)), n, L, w.to(DEV), b.to(DEV), alpha.to(DEV))
            z = lrelu(y.double()[:, :, :H // 2 * 2, :W // 2 * 2].amax(dim=(2, 3)))
            ref = torch.zeros(L, L, dtype=torch.float64)
            ref[:n, :n] = torch.sigmoid(z @ w.double() + b.double()).view(n, n)
            bound = (h * 2.0 ** -24 * (z.abs() @ w.abs().double()).max() + 2.0 ** -22) / 4 + 2.0 ** -23
            assert float((scores.cpu().double() - ref).abs().max()) <= float(bound), (H, W, n)
            assert bool((scores.cpu()[n:] == 0).all()) and bool((scores.cpu()[:, n:] == 0).all())
            wref = ref / (ref.sum(dim=1, keepdim=True) + 0.15 + 1e-4)
            assert float((weight.cpu().double() - wref).abs().max()) <= float(bound) * 4 + 2.0 ** -22, (H, W, n)


def test_pose_head_against_float64():
    """LeakyReLU, MaxPool 2, the mean, three linears and pose_to_tfm(corr) @ T against float64 of the same inputs (the SplitMap's values): the project's bound for
    float32 kernels against float64, rtol 1e-4 + 1e-5 of the scale; T_new from the kernel's OWN corr to 1e-12."""
    h = 64
    for H4, W4 in ((2, 2), (3, 5), (4, 7)):
        for n, L in ((1, 5), (3, 5), (8, 8)):
            g = torch.Generator().manual_seed(H4 + n)
            y4 = ops.SplitMap.pack(nhwc((torch.randn(n * n, h, H4, W4, generator=g) * 2).to(DEV)))
            fc = [torch.randn(h, h, generator=g) / 8, torch.randn(h, generator=g) * 0.1, torch.randn(h, h, generator=g) / 8, torch.randn(h, generator=g) * 0.1,
                  torch.randn(3, h, generator=g) / 8, torch.randn(3, generator=g) * 0.1]
            T = pairwise_f64(poses_for(n, n), L)
            corr, T_new = ops.v2vr_pose_head(y4, n, L, tuple(t.to(DEV) for t in fc), T.to(DEV))
            d = [t.double() for t in fc]
            z = F.max_pool2d(lrelu(y4.dense_reference().cpu().double()), 2).mean(dim=(2, 3))
            z = lrelu(lrelu(z @ d[0].t() + d[1]) @ d[2].t() + d[3]) @ d[4].t() + d[5]
            assert_elementwise(corr.cpu()[:n, :n].reshape(n * n, 3), z, "v2vr_pose_head vs float64")
            want = torch.eye(4, dtype=torch.float64).repeat(L, L, 1, 1)
            want[:n, :n] = (tfm_f64(corr.cpu()[:n, :n].reshape(n * n, 3)) @ T[:n, :n].reshape(n * n, 4, 4)).view(n, n, 4, 4)
            assert float((T_new.cpu() - want).abs().max()) <= 1e-12
            assert bool((corr.cpu()[n:] == 0).all()) and bool((corr.cpu()[:, n:] == 0).all())


def _synthetic_t_new(n, L, seed, noise=True):
    """(noisy poses [n, 3], T' [L, L, 4, 4]): the pairwise matrices of the TRUE poses, each perturbed by an independent small rigid motion (a regression's residual)."""
    g = torch.Generator().manual_seed(seed)
    true = poses_for(n, seed).double()
    noisy = true.clone()
    T_new = pairwise_f64(true, L)
    if noise:
        noisy[:, :2] += torch.randn(n, 2, generator=g, dtype=torch.float64) * 0.4
        noisy[:, 2] += torch.randn(n, generator=g, dtype=torch.float64) * 4.0
        for i in range(n):
            for j in range(n):
                if i != j:
                    T_new[i, j] = tfm_f64(torch.randn(1, 3, generator=g, dtype=torch.float64) * torch.tensor([0.05, 0.05, 0.5]))[0] @ T_new[i, j]
    return noisy, T_new


def test_pairwise_and_consistency_against_the_yardstick():
    """``v2vr_pairwise`` against the float64 solve (1e-12); the whole EM in one launch against ``weighted_em_f64`` on synthetic T' under strong noise (0.4 m, 4
    degrees) for two to eight agents, one agent, and a scene without noise (T' consistent: corrected = input) -- all within 4 x E32 of the corrected poses."""
    H, W, den = 25, 41, 0.8
    bound = BOUNDS["lidar_pose_corrected"]
    for n in AGENTS:
        for noise in (True, False):
            noisy, T_new = _synthetic_t_new(n, MAX_CAV, 20 + n, noise)
            T, theta = ops.v2vr_pairwise(noisy.to(DEV), MAX_CAV, H, W, den * W, den * H)
            want = pairwise_f64(noisy, MAX_CAV)
            assert float((T.cpu() - want).abs().max()) <= 1e-12 and float((theta.cpu() - normalize_f64(want, H, W, 2, 0.4)).abs().max()) <= 1e-12
            fixed, T_fixed, theta_fixed = ops.v2vr_consistency(noisy.to(DEV), T_new.to(DEV), H, W, den * W, den * H)
            ref = weighted_em_f64(noisy, T_new, torch.full((MAX_CAV, MAX_CAV), 0.01, dtype=torch.float64))
            err = float((fixed.cpu() - ref).abs().max())
            print(f"v2vr_consistency n = {n}, noise {noise}: |kernel - yardstick| {err:.3e}, moved {float((ref - noisy).abs().max()):.3f}")
            assert err <= bound, (n, noise, err)
            if n > 1 and noise:
                assert float((ref - noisy).abs().max()) > 100 * bound                          # the EM does move the poses
            if n == 1 or not noise:
                assert float((fixed.cpu() - noisy).abs().max()) <= bound, (n, noise)
            want = pairwise_f64(fixed.cpu(), MAX_CAV)
            assert float((T_fixed.cpu() - want).abs().max()) <= 1e-12 and float((theta_fixed.cpu() - normalize_f64(want, H, W, 2, 0.4)).abs().max()) <= 1e-12


def _on_device(H, W, stage=2):
    m, args, state = model_for(H, W, stage)
    return m.to(DEV), args, state


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_fusion_and_heads_with_the_yardsticks_own_thetas_and_weights(size):
    """The weighted message passing and the 1 x 1 mlp given the yardstick's OWN affines and weights: the V2VNet bound."""
    H, W = size
    m, _, _ = _on_device(H, W)
    for n in AGENTS:
        args, state, x, poses, ref, trace = case(H, W, n)
        assert_robust_not_degenerate(state, args, x, poses, ref, trace, BOUNDS, what=(H, W, n))
        theta = normalize_f64(ref["pairwise_t_matrix_corrected"], H, W, 2, 0.4)
        with torch.no_grad():
            got = m.fusion_net(nhwc(x.to(DEV)), [n], theta.unsqueeze(0).to(DEV), ref["weight"].float().unsqueeze(0).to(DEV))
        assert_elementwise(got[0], ref["fused"], f"fusion {H} x {W}, {n} agents")


@pytest.mark.parametrize("stage", [0, 1, 2])
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_kernel_route_against_the_yardstick_and_the_torch_route(size, stage):
    """``forward_kernels`` per stage against the float64 yardstick (4 x E32 per quantity) and against ``forward_torch`` on the GPU (5 x E32: the kernel route's
    4 plus the float32 route's own 1), one to eight agents; every figure is printed before it is asserted."""
    H, W = size
    m, _, _ = _on_device(H, W, stage)
    for n in AGENTS:
        args, state, x, poses, ref, trace = case(H, W, n, stage)
        if stage != 1:
            assert_robust_not_degenerate(state, args, x, poses, ref, trace, BOUNDS, what=(H, W, n, stage))
        elif n > 1:
            assert float(ref["pairwise_corr"].abs().min()) > 100 * BOUNDS["pairwise_corr"]
        assert m.kernel_route(64, n)
        with torch.no_grad():
            got = m.forward_kernels(nhwc(x.to(DEV)), [n], poses.to(DEV))
            slow = m.forward_torch(x.to(DEV), [n], poses.to(DEV))
        e, s = errors(got, ref, n), errors(slow, ref, n)
        print(f"{H} x {W}, {n} agents, stage {stage}: kernels {({k: f'{v:.2e}' for k, v in e.items()})}  forward_torch on the GPU {({k: f'{v:.2e}' for k, v in s.items()})}")
        wanted = {0: {"scores", "weight", "cls_preds", "reg_preds"}, 1: {"pairwise_corr"}, 2: set(E32)}[stage]
        assert set(e) == wanted
        for k, v in e.items():
            assert v <= BOUNDS[k], (H, W, n, stage, k, v, BOUNDS[k])
        for k in wanted:
            a, b = got[k].float(), slow[k].float()
            d = float((a - b).abs().max()) / (float(b.abs().max()) if k.endswith("_preds") else 1.0)
            assert d <= (MARGIN + 1) * E32[k], (H, W, n, stage, k, d)


def test_chain_under_graph_capture():
    """From the shrunk maps and the poses to the head outputs, captured once on one stream and replayed on two other frames: equal to the eager results bit for
    bit -- nothing in the chain returns to the host."""
    H, W, n = 25, 41, 3
    m, _, _ = _on_device(H, W)
    x, p = nhwc(maps_for(n, H, W).to(DEV)), poses_for(n, 3).to(DEV)
    with torch.no_grad():
        m.forward_kernels(x, [n], p)                                        # (weight images packed, workspaces and the range word made: before the capture)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = m.forward_kernels(x, [n], p)
        for seed in (1, 2):
            fx, fp = maps_for(n, H, W, seed).to(DEV), poses_for(n, 3 + seed).to(DEV)
            x.copy_(fx)
            p.copy_(fp)
            graph.replay()
            torch.cuda.synchronize()
            eager = m.forward_kernels(nhwc(fx), [n], fp)
            for k in ("pairwise_corr", "lidar_pose_corrected", "scores", "weight", "cls_preds", "reg_preds"):
                assert torch.equal(out[k], eager[k]), (seed, k)


def test_model_level_detections_and_head_maps():
    """``mini_pointpillar_v2vnet_robust.yaml`` eagerly through ``inference_intermediate_fusion`` with a fixed ``pose_noise``: the detections of the kernel route
    equal those of a second run; its head maps lie within the map bound (4 x E32) of the yardstick fed the same shrunk maps."""
    h = builtin_config("mini_pointpillar_v2vnet_robust")
    model = build_model(h)
    fill_parameters_(model, seed=0, cls_bias=-1.0)
    v2v_robust_parameters_(model, seed=2)
    with torch.no_grad():
        model.reg_head.weight.mul_(0.01); model.reg_head.bias.zero_(); model.cls_head.weight.mul_(0.05)
    state = {k: v.clone() for k, v in model.state_dict().items()}
    model = model.to(DEV).eval()
    pp = build_postprocessor(h["postprocess"], False)
    anchors = torch.from_numpy(pp.generate_anchor_box())
    frame = make_frame(h, 3, pillars_per_agent=300, seed=41, spread_xy=(4.0, 2.0), spread_yaw=15.0, with_poses=True)
    g = torch.Generator().manual_seed(5)
    frame["pose_noise"] = torch.zeros(3, 6)
    frame["pose_noise"][:, :2] = torch.randn(3, 2, generator=g) * 0.4
    batch = {"ego": dict(to_device(frame, DEV), transformation_matrix=torch.eye(4, device=DEV), anchor_box=anchors.to(DEV))}
    assert model.kernel_route(model.out_channel, 3)
    with torch.no_grad():
        first = inference_intermediate_fusion(batch, model, pp)
        second = inference_intermediate_fusion(batch, model, pp)
        x = model.encode(batch["ego"])
        got = model(batch["ego"])
    assert first["pred_box_tensor"] is not None and first["pred_box_tensor"].shape[0] > 0
    assert torch.equal(first["pred_box_tensor"], second["pred_box_tensor"]) and torch.equal(first["pred_score"], second["pred_score"])
    noisy = (frame["lidar_pose"] + frame["pose_noise"])[:, [0, 1, 4]]
    ref = robust_frame_f64(state, h["model"]["args"], x.float().cpu(), noisy, 2)
    e = errors(got, ref, 3)
    print("mini_pointpillar_v2vnet_robust, 3 agents:", {k: f"{v:.2e}" for k, v in e.items()})
    for k in ("cls_preds", "reg_preds", "scores"):
        assert e[k] <= BOUNDS[k], (k, e[k])
