"""The pose-robust V2VNet restated in float64 (not the code under test): the yardstick of tests/test_v2v_robust_cpu.py and tests/test_v2v_robust_gpu.py.

The reference's UNREDUCED computation (models/point_pillar_v2vnet_robust.py:205-267, sub_modules/v2v_robust_module.py, fuse_modules/v2v_fuse.py:51-166), one frame:

    T_ij    = T_j^-1 T_i of pose_to_tfm(noisy poses)                          (a linear solve per pair)
    corr_ij = PoseRegression([warp(x_j, theta_ij) | x_i])                     the full 2C -> h convolution per pair, every LeakyReLU before its pooling
    T'_ij   = pose_to_tfm(corr_ij) @ T_ij
    poses'  = WeightedEM(poses, T', intersection)                             the intersection from an actual warp of a map of zeros, + 0.01
    s_ij    = Attention([warp(x_j, theta'_ij) | x_i]);  w_ij = s_ij / (sum_j s_ij + alpha + 1e-4)
    fused   = V2VNet message passing with agg_i = sum_j m_ij w_ij, then the 1 x 1 heads

Everything after the sampling positions of the warp (tests/disco_reference.py: float32 positions) is float64.  None of the identities of ``coalign_amd.v2v_robust``
is used: no split first convolution, no pooling before the activation, no cropped maximum, no constant intersection, no shared warp.
"""
import math

import torch
import torch.nn.functional as F

from disco_reference import warp_f64

SLOPE = 0.01


def _sd(state: dict, prefix: str) -> dict:
    return {k[len(prefix):]: v.detach().cpu().double() for k, v in state.items() if k.startswith(prefix) and torch.is_tensor(v) and v.is_floating_point()}


def tfm_f64(poses: torch.Tensor) -> torch.Tensor:
    """[n, 3] (x, y, yaw in degrees) -> [n, 4, 4] float64."""
    p = poses.detach().cpu().double()
    T = torch.eye(4, dtype=torch.float64).repeat(p.shape[0], 1, 1)
    yaw = p[:, 2] * math.pi / 180.0
    T[:, 0, 0], T[:, 0, 1], T[:, 1, 0], T[:, 1, 1] = torch.cos(yaw), -torch.sin(yaw), torch.sin(yaw), torch.cos(yaw)
    T[:, 0, 3], T[:, 1, 3] = p[:, 0], p[:, 1]
    return T


def pairwise_f64(poses: torch.Tensor, L: int) -> torch.Tensor:
    """[n, 3] -> [L, L, 4, 4]: entry [i, j] = T_j^-1 T_i, identity elsewhere."""
    t = tfm_f64(poses)
    out = torch.eye(4, dtype=torch.float64).repeat(L, L, 1, 1)
    for i in range(t.shape[0]):
        for j in range(t.shape[0]):
            if i != j:
                out[i, j] = torch.linalg.solve(t[j], t[i])
    return out


def normalize_f64(T: torch.Tensor, H: int, W: int, downsample_rate: float, discrete_ratio: float) -> torch.Tensor:
    """[.., 4, 4] -> [.., 2, 3] in affine_grid's normalised coordinates."""
    T = T.double()
    m = torch.zeros(T.shape[:-2] + (2, 3), dtype=torch.float64)
    m[..., 0, 0], m[..., 0, 1], m[..., 0, 2] = T[..., 0, 0], T[..., 0, 1] * H / W, T[..., 0, 3] / (downsample_rate * discrete_ratio * W) * 2
    m[..., 1, 0], m[..., 1, 1], m[..., 1, 2] = T[..., 1, 0] * W / H, T[..., 1, 1], T[..., 1, 3] / (downsample_rate * discrete_ratio * H) * 2
    return m


def _pair_inputs(x: torch.Tensor, theta: torch.Tensor, i: int) -> torch.Tensor:
    n = x.shape[0]
    return torch.cat([warp_f64(x, theta[i, :n]), x[i:i + 1].expand(n, -1, -1, -1)], dim=1)


def regression_net_f64(sd: dict, cat: torch.Tensor) -> torch.Tensor:
    """PoseRegression.model on [N, 2C, H, W] float64, layer by layer in the reference's order."""
    y = cat
    for k, stride in ((0, 1), (3, 1), (6, 1), (9, 2)):
        y = F.max_pool2d(F.leaky_relu(F.conv2d(y, sd[f"model.{k}.weight"], sd[f"model.{k}.bias"], stride=stride, padding=1), SLOPE), 2)
    y = y.mean(dim=(2, 3))
    y = F.leaky_relu(y @ sd["model.14.weight"].t() + sd["model.14.bias"], SLOPE)
    y = F.leaky_relu(y @ sd["model.16.weight"].t() + sd["model.16.bias"], SLOPE)
    return y @ sd["model.18.weight"].t() + sd["model.18.bias"]


def attention_net_f64(sd: dict, cat: torch.Tensor) -> torch.Tensor:
    """Attention.model on [N, 2C, H, W] float64 -> [N]."""
    y = cat
    for k in (0, 3):
        y = F.max_pool2d(F.leaky_relu(F.conv2d(y, sd[f"model.{k}.weight"], sd[f"model.{k}.bias"], padding=1), SLOPE), 2)
    y = y.amax(dim=(2, 3))
    return torch.sigmoid(y @ sd["model.8.weight"].t() + sd["model.8.bias"]).flatten()


def pose_regression_f64(state: dict, x: torch.Tensor, T: torch.Tensor, cfg: dict):
    """One frame: x [n, C, H, W], T [L, L, 4, 4] -> (corr [n, n, 3], T_new [L, L, 4, 4])."""
    sd = _sd(state, "pose_reg_net.pose_regression.")
    x = x.detach().cpu().double()
    n, _, H, W = x.shape
    theta = normalize_f64(T, H, W, cfg["downsample_rate"], cfg["discrete_ratio"])
    corr = torch.stack([regression_net_f64(sd, _pair_inputs(x, theta, i)) for i in range(n)])
    T_new = torch.eye(4, dtype=torch.float64).repeat(T.shape[0], T.shape[1], 1, 1)
    for i in range(n):
        T_new[i, :n] = tfm_f64(corr[i]) @ T[i, :n].double()
    return corr, T_new


def _xycs(M: torch.Tensor) -> torch.Tensor:
    return torch.stack([M[..., 0, 3], M[..., 1, 3], M[..., 0, 0], M[..., 1, 0]], dim=-1)


def _xycs_tfm(v: torch.Tensor) -> torch.Tensor:
    T = torch.eye(4, dtype=torch.float64)
    T[0, 0], T[0, 1], T[1, 0], T[1, 1], T[0, 3], T[1, 3] = v[2], -v[3], v[3], v[2], v[0], v[1]
    return T


def intersection_f64(T_new: torch.Tensor, cfg: dict) -> torch.Tensor:
    """get_intersection as written: the warp of a map of ZEROS, summed, / (H W), + 0.01."""
    L = T_new.shape[0]
    H, W = cfg["H"], cfg["W"]
    theta = normalize_f64(T_new, H, W, cfg["downsample_rate"], cfg["discrete_ratio"])
    zeros = torch.zeros(L, 1, H, W, dtype=torch.float64)
    return torch.stack([warp_f64(zeros, theta[i]).sum(dim=(1, 2, 3)) / (H * W) for i in range(L)]) + 0.01


def weighted_em_f64(poses: torch.Tensor, T_new: torch.Tensor, intersection: torch.Tensor, rounds: int = 10, steps: int = 15) -> torch.Tensor:
    """WeightedEM of one frame in float64 throughout: poses [n, 3], T_new [L, L, 4, 4] -> [n, 3]."""
    poses, T_new = poses.detach().cpu().double(), T_new.detach().cpu().double()
    n = poses.shape[0]
    if n == 1:
        return poses.clone()
    tf = tfm_f64(poses)
    weight = torch.ones(n, n, dtype=torch.float64)
    eye = torch.eye(4, dtype=torch.float64)
    for _ in range(rounds):
        mus, sigmas = [], []
        for i in range(n):
            ids = [k for k in range(n) if k != i]
            rel = torch.cat([T_new[i, ids], torch.linalg.inv(T_new[ids, i])])
            samples = _xycs(torch.cat([tf[ids], tf[ids]]) @ rel)
            w = torch.cat([weight[i, ids], weight[i, ids]])
            mu = samples.median(0).values
            Sigma = eye.clone()
            for _ in range(steps):
                d = mu[None] - samples
                eta = 6.0 / (2.0 + ((d @ torch.linalg.inv(Sigma)) * d).sum(1))
                mu = (w * eta) @ samples / (w * eta).sum()
                d = mu[None] - samples
                Sigma = (eta[:, None, None] * d[:, :, None] * d[:, None, :]).sum(0) / d.shape[0] + 0.05 * eye
            mus.append(mu)
            sigmas.append(Sigma)
        weight = torch.zeros(n, n, dtype=torch.float64)
        for i in range(n):
            Si, logdet = torch.linalg.inv(sigmas[i]), torch.logdet(sigmas[i])
            for j in range(n):
                if i != j:
                    est = _xycs(torch.stack([_xycs_tfm(mus[j]) @ T_new[i, j], _xycs_tfm(mus[i]) @ torch.linalg.inv(T_new[i, j])]))
                    d = est - mus[i]
                    logt = math.lgamma(3.0) - (math.lgamma(1.0) + 2.0 * (math.log(2.0) + math.log(math.pi)) + 0.5 * logdet) - 3.0 * torch.log(1 + ((d @ Si) * d).sum(1) / 2.0)
                    weight[i, j] = 120.0 * intersection[i, j] / (120.0 - logt.sum())
    mu = torch.stack(mus)
    return torch.stack([mu[:, 0], mu[:, 1], torch.rad2deg(torch.atan2(mu[:, 3], mu[:, 2]))], dim=1)


def attention_f64(state: dict, x: torch.Tensor, T: torch.Tensor, cfg: dict):
    """One frame -> (scores [L, L], weight [L, L])."""
    sd = _sd(state, "attention_net.attention_net.")
    alpha = float(state["attention_net.alpha"]) if "attention_net.alpha" in state else float(cfg.get("alpha", 0.35))
    x = x.detach().cpu().double()
    n, _, H, W = x.shape
    L = T.shape[0]
    theta = normalize_f64(T, H, W, cfg["downsample_rate"], cfg["discrete_ratio"])
    scores = torch.zeros(L, L, dtype=torch.float64)
    for i in range(n):
        scores[i, :n] = attention_net_f64(sd, _pair_inputs(x, theta, i))
    return scores, scores / (scores.sum(dim=1, keepdim=True) + alpha + 1e-4)


def fuse_weight_f64(state: dict, x: torch.Tensor, theta: torch.Tensor, args: dict, weight: torch.Tensor, trace=None) -> torch.Tensor:
    """V2VNetFusion with agg_operator 'weight', one frame, unreduced: x [n, C, H, W], theta [>= n, >= n, 2, 3], weight [>= n, >= n] -> [C, H, W]."""
    sd = _sd(state, "fusion_net.")
    x = x.detach().cpu().double()
    n, C, H, W = x.shape
    th, wt = theta.detach().cpu().double(), weight.detach().cpu().double()
    layers = args["conv_gru"]["num_layers"]
    masks = torch.stack([warp_f64(torch.ones(n, 1, H, W, dtype=torch.float64), th[i, :n]) for i in range(n)])
    if trace is not None:
        trace["masks"] = masks[:, :, 0]
    for _ in range(args["num_iteration"]):
        new = []
        for i in range(n):
            m = F.conv2d(_pair_inputs(x, th, i), sd["msg_cnn.weight"], sd["msg_cnn.bias"], padding=1) * masks[i]
            agg = (m * wt[i, :n].view(-1, 1, 1, 1)).sum(dim=0)
            if args["gru_flag"]:
                inp = torch.cat([x[i], agg], dim=0).unsqueeze(0)
                for k in range(layers):
                    p = f"conv_gru.cell_list.{k}."
                    hid = sd[p + "conv_can.weight"].shape[0]
                    h = torch.zeros(1, hid, H, W, dtype=torch.float64)
                    gates = F.conv2d(torch.cat([inp, h], dim=1), sd[p + "conv_gates.weight"], sd[p + "conv_gates.bias"], padding=1)
                    reset, update = torch.sigmoid(gates[:, :hid]), torch.sigmoid(gates[:, hid:])
                    cnm = torch.tanh(F.conv2d(torch.cat([inp, reset * h], dim=1), sd[p + "conv_can.weight"], sd[p + "conv_can.bias"], padding=1))
                    inp = (1 - update) * h + update * cnm
                new.append(inp[0])
            else:
                new.append(x[i] + agg)
        x = torch.stack(new)
    return (x[0].permute(1, 2, 0) @ sd["mlp.weight"].t() + sd["mlp.bias"]).permute(2, 0, 1)


def heads_f64(state: dict, fused: torch.Tensor) -> dict:
    out = {}
    for k in ("cls", "reg"):
        w, b = state[f"{k}_head.weight"].detach().cpu().double(), state[f"{k}_head.bias"].detach().cpu().double()
        out[f"{k}_preds"] = torch.einsum("oc,chw->ohw", w.flatten(1), fused) + b.view(-1, 1, 1)
    return out


def robust_frame_f64(state: dict, args: dict, x: torch.Tensor, poses3: torch.Tensor, stage: int = 2, zero_weight_of=None, trace=None) -> dict:
    """One frame of train_forward after the noise: x [n, C, H, W], poses3 [n, 3] (noisy) -> the stage's outputs in float64, every intermediate included.
    ``zero_weight_of`` (an agent index): that sender's weights are zeroed before the fusion (the non-degeneracy guard)."""
    cfg, L = args["robust"], args["max_cav"]
    fcfg = {"downsample_rate": args["v2vfusion"]["downsample_rate"], "discrete_ratio": args["v2vfusion"]["voxel_size"][0]}
    n, _, H, W = x.shape
    L = max(L, n)
    poses3 = poses3.detach().cpu().double()
    T = pairwise_f64(poses3, L)
    out = {"pairwise_t_matrix": T, "poses": poses3}
    if stage in (1, 2):
        out["pairwise_corr"], out["pairwise_t_matrix_new"] = pose_regression_f64(state, x, T, cfg)
    if stage == 1:
        return out
    if stage == 2:
        out["lidar_pose_corrected"] = weighted_em_f64(poses3, out["pairwise_t_matrix_new"], intersection_f64(out["pairwise_t_matrix_new"], cfg))
        T = pairwise_f64(out["lidar_pose_corrected"], L)
        out["pairwise_t_matrix_corrected"] = T
    out["scores"], out["weight"] = attention_f64(state, x, T, cfg)
    weight = out["weight"].clone()
    if zero_weight_of is not None:
        weight[:, zero_weight_of] = 0
    out["fused"] = fuse_weight_f64(state, x, normalize_f64(T, H, W, fcfg["downsample_rate"], fcfg["discrete_ratio"]), args["v2vfusion"], weight, trace)
    return dict(out, **heads_f64(state, out["fused"]))


def assert_robust_not_degenerate(state: dict, args: dict, x: torch.Tensor, poses3: torch.Tensor, ref: dict, trace: dict, bounds: dict, what="", rtol=1e-4, floor=1e-5) -> None:
    """The case must SEE every part (run on the float64 side before every parity assertion; ``ref`` and ``trace`` from ``robust_frame_f64`` of the same case).
    With more than one agent: the scores lie in (0.1, 0.9) and any two pairs differ by more than twice the scores' bound (``bounds['scores']``); |pose_corr| and |corrected - noisy| each exceed 100 x their bound
    (``bounds['pairwise_corr']``, ``bounds['lidar_pose_corrected']``); zeroing agent 1's weight moves the fused map by more than 10 x the map bound; the masks hold
    fractions, zeros and ones."""
    n = x.shape[0]
    if n == 1:
        return
    s = ref["scores"][:n, :n]
    assert bool(((s > 0.1) & (s < 0.9)).all()), (what, "scores outside (0.1, 0.9)", s)
    flat = s.flatten().sort().values
    assert float((flat[1:] - flat[:-1]).min()) > 2 * bounds["scores"], (what, "two pairs share a score to within the comparison bound: swapping them would pass", s)
    if "pairwise_corr" in ref:
        c = ref["pairwise_corr"].abs().amax(dim=-1)                             # per pair: its largest component
        assert float(c.min()) > 100 * bounds["pairwise_corr"], (what, "a pair's pose correction is invisible", float(c.min()))
    if "lidar_pose_corrected" in ref:
        d = (ref["lidar_pose_corrected"] - ref["poses"]).abs().max(dim=1).values
        assert float(d.min()) > 100 * bounds["lidar_pose_corrected"], (what, "the EM leaves an agent's pose where it was", d)
    scale = float(ref["fused"].abs().max())
    without = robust_frame_f64(state, args, x, poses3, stage=2 if "lidar_pose_corrected" in ref else 0, zero_weight_of=1)
    assert float((ref["fused"] - without["fused"]).abs().max()) > 10 * (rtol + floor) * scale, (what, "agent 1's weight is invisible")
    m = trace["masks"]
    assert bool((m == 0).any()) and bool(((m - 1).abs() < 1e-12).any()) and bool(((m > 1e-6) & (m < 1 - 1e-6)).any()), (what, "masks: 0, 1 and fractions must all occur")
