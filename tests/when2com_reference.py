"""When2com's handshake fusion restated in float64 (not the code under test): the yardstick of tests/test_when2com_gpu.py and tests/test_when2com_cpu.py.

The reference's UNFOLDED arithmetic (When2commFusion.forward, fuse_modules/fusion_in_one.py:354-431; policy_net4, km_generator_v2, AdditiveAttentin,
fuse_modules/when2com_fuse.py:133-363), one frame, from the ``state_dict``:

    v_j   = warp(x_j, theta_j)                                 every agent, the ego included; the warp of tests/disco_reference.py (float32 sampling positions)
    m_j   = five blocks relu(bn(conv(.) + bias)) on v_j        C -> 512 -> 256 -> (stride 2) 256 -> 256 -> (stride 2) 256, BatchNorm in eval mode, eps = 1e-5
    key_j = fc(pool(relu(bn(conv_s2(m_j)))))                   256 -> 128 block, a 5 x 7 adaptive average pool with explicit bins, flattened (channel, row, column),
                                                               Linear 4480 -> 256, ReLU, 256 -> 128, ReLU, 128 -> key_size;  query likewise from m_0 with query_net
    l_j   = <linear_feat(key_j), linear_context(query)>        the two linears applied one after the other, nothing folded
    out   = sum_j softmax_j(l_j) v_j

None of the identities of ``When2comFusion.forward_reduced`` is used here.
"""
import torch
import torch.nn.functional as F

from disco_reference import EPS, warp_f64

POOL = (5, 7)


def cbr_f64(sd: dict, prefix: str, x: torch.Tensor, stride: int) -> torch.Tensor:
    y = F.conv2d(x, sd[prefix + ".cbr_unit.0.weight"], sd[prefix + ".cbr_unit.0.bias"], stride=stride, padding=1)
    scale = sd[prefix + ".cbr_unit.1.weight"] / torch.sqrt(sd[prefix + ".cbr_unit.1.running_var"] + EPS)
    y = (y - sd[prefix + ".cbr_unit.1.running_mean"].view(1, -1, 1, 1)) * scale.view(1, -1, 1, 1) + sd[prefix + ".cbr_unit.1.bias"].view(1, -1, 1, 1)
    return torch.relu(y)


def adaptive_pool_f64(x: torch.Tensor, out_hw=POOL) -> torch.Tensor:
    """AdaptiveAvgPool2d by its definition: bin i covers rows floor(i h / oh) .. ceil((i + 1) h / oh) - 1 (overlapping when oh does not divide h, repeating when
    h < oh), likewise for the columns; the mean of the bin."""
    n, c, h, w = x.shape
    oh, ow = out_hw
    out = torch.zeros(n, c, oh, ow, dtype=x.dtype)
    for i in range(oh):
        ys, ye = (i * h) // oh, -((-(i + 1) * h) // oh)
        for j in range(ow):
            xs, xe = (j * w) // ow, -((-(j + 1) * w) // ow)
            out[:, :, i, j] = x[:, :, ys:ye, xs:xe].mean(dim=(2, 3))
    return out


def flatten_pool(p: torch.Tensor, order: str = "cij") -> torch.Tensor:
    """[n, 128, 5, 7] -> [n, 4480].  ``cij`` is the reference's order; ``ijc`` (channel fastest) and ``cji`` (the 5 x 7 grid transposed) are the two mistakes a
    kernel's pooling can make, kept here so that a test can show the yardstick tells them apart."""
    if order == "cij":
        return p.reshape(p.shape[0], -1)
    if order == "ijc":
        return p.permute(0, 2, 3, 1).reshape(p.shape[0], -1)
    if order == "cji":
        return p.permute(0, 1, 3, 2).reshape(p.shape[0], -1)
    raise ValueError(order)


def head_f64(sd: dict, net: str, feat: torch.Tensor, order: str = "cij") -> torch.Tensor:
    """km_generator_v2 after its conv1: feat [n, 128, h, w] -> [n, out_size]."""
    p = flatten_pool(adaptive_pool_f64(feat), order)
    h = torch.relu(p @ sd[net + ".fc.0.weight"].t() + sd[net + ".fc.0.bias"])
    h = torch.relu(h @ sd[net + ".fc.2.weight"].t() + sd[net + ".fc.2.bias"])
    return h @ sd[net + ".fc.4.weight"].t() + sd[net + ".fc.4.bias"]


def score_f64(sd: dict, key_maps: torch.Tensor, query_map: torch.Tensor, order: str = "cij"):
    """The heads on given conv1 outputs: key_maps [n, 128, h, w], query_map [1, 128, h, w] -> (logits [n], weights [n]) float64."""
    keys, query = head_f64(sd, "key_net", key_maps.double(), order), head_f64(sd, "query_net", query_map.double(), order)
    kf = keys @ sd["attention_net.linear_feat.weight"].t() + sd["attention_net.linear_feat.bias"]
    qf = query @ sd["attention_net.linear_context.weight"].t() + sd["attention_net.linear_context.bias"]
    logits = kf @ qf[0]
    return logits, torch.softmax(logits, dim=0)


def state_f64(state: dict) -> dict:
    return {k.split("fusion_net.")[-1]: v.detach().cpu().double() for k, v in state.items() if v.is_floating_point()}


def when2com_fuse_f64(state: dict, x: torch.Tensor, theta: torch.Tensor, order: str = "cij"):
    """One frame: x [n, C, H, W], theta [n, 2, 3] (the ego's row) -> (fused [C, H, W], logits [n], weights [n]) float64."""
    sd = state_f64(state)
    v = warp_f64(x, theta)
    m = v
    for name, stride in (("conv1", 1), ("conv2", 1), ("conv3", 2), ("conv4", 1), ("conv5", 2)):
        m = cbr_f64(sd, "query_key_net." + name, m, stride)
    logits, w = score_f64(sd, cbr_f64(sd, "key_net.conv1", m, 2), cbr_f64(sd, "query_net.conv1", m[:1], 2), order)
    return (w.view(-1, 1, 1, 1) * v).sum(0), logits, w


def weighted_warp_f64(x: torch.Tensor, theta: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
    """sum_j w_j warp(x_j, theta_j) with given weights -> [C, H, W] float64."""
    return (w.detach().cpu().double().view(-1, 1, 1, 1) * warp_f64(x, theta)).sum(0)


def parameter_checksums(module) -> dict:
    """name -> (numel, float64 sum, float64 sum of squares) of every floating-point tensor of the ``state_dict``: what the fixture stores in place of 24 MB of weights."""
    return {k: (v.numel(), float(v.double().sum()), float((v.double() ** 2).sum())) for k, v in module.state_dict().items() if v.is_floating_point()}


def assert_sees_the_heads(weights: torch.Tensor, what="") -> None:
    """With more than one agent every softmax weight lies in [0.02, 0.98] and at least one is 0.05 off 1 / n: neither uniform (the heads invisible) nor one-hot
    (every agent but one invisible)."""
    n = weights.numel()
    if n < 2:
        return
    w = weights.detach().cpu().double()
    assert float(w.min()) >= 0.02 and float(w.max()) <= 0.98, (what, "saturated softmax", w.tolist())
    assert float((w - 1.0 / n).abs().max()) >= 0.05, (what, "uniform softmax", w.tolist())
