"""DiscoNet's pixel-weight fusion restated in float64 (not the code under test): the yardstick of tests/test_disco_gpu.py and tests/test_disco_cpu.py.

    xw_j = warp(x_j, theta_j)                  every agent, the ego included; bilinear, zero padding, align_corners=False, sampled at the float32 positions the
                                               reference's float64 -> float32 grid and float32 un-normalise give (the positions are part of the semantics)
    s_j  = relu(conv1_4(relu(bn1_3(conv1_3(relu(bn1_2(conv1_2(relu(bn1_1(conv1_1([xw_j | x_0]))))))))))),  BatchNorm in eval mode, eps = 1e-5
    out  = sum_j softmax_j(s_j) xw_j

Everything after the sampling positions is float64: tap weights, blend, the four layers from the UNFOLDED ``state_dict``, softmax, weighted sum.
"""
import torch

EPS = 1e-5


def warp_f64(x: torch.Tensor, theta: torch.Tensor) -> torch.Tensor:
    """x [n, C, H, W], theta [n, 2, 3] -> [n, C, H, W] float64."""
    x, th = x.detach().cpu().double(), theta.detach().cpu().double()
    n, C, H, W = x.shape
    xs = (2.0 * torch.arange(W, dtype=torch.float64) + 1.0) / W - 1.0
    ys = (2.0 * torch.arange(H, dtype=torch.float64) + 1.0) / H - 1.0
    yy, xx = torch.meshgrid(ys, xs, indexing="ij")
    gx = (th[:, 0, 0, None, None] * xx + th[:, 0, 1, None, None] * yy + th[:, 0, 2, None, None]).float()      # the float64 grid, cast to float32
    gy = (th[:, 1, 0, None, None] * xx + th[:, 1, 1, None, None] * yy + th[:, 1, 2, None, None]).float()
    ix = ((gx + 1.0) * (W / 2.0) - 0.5).double()                                                             # float32 un-normalise: the sampling position
    iy = ((gy + 1.0) * (H / 2.0) - 0.5).double()
    x0, y0 = torch.floor(ix), torch.floor(iy)
    tx, ty = ix - x0, iy - y0
    x0, y0 = x0.long(), y0.long()
    flat = x.reshape(n, C, H * W)
    out = torch.zeros(n, C, H, W, dtype=torch.float64)
    for dy, dx, wgt in ((0, 0, (1 - ty) * (1 - tx)), (0, 1, (1 - ty) * tx), (1, 0, ty * (1 - tx)), (1, 1, ty * tx)):
        xi, yi = x0 + dx, y0 + dy
        ok = (xi >= 0) & (xi < W) & (yi >= 0) & (yi < H)
        idx = (yi.clamp(0, H - 1) * W + xi.clamp(0, W - 1)).view(n, 1, -1).expand(n, C, -1)
        out = out + torch.gather(flat, 2, idx).view(n, C, H, W) * (wgt * ok.double()).unsqueeze(1)
    return out


def logits_f64(state: dict, cat: torch.Tensor) -> torch.Tensor:
    """PixelWeightLayer on cat [n, 2C, H, W] float64 from its state_dict (names conv1_1 .. conv1_4, bn1_1 .. bn1_3) -> [n, H, W]."""
    sd = {k.split("pixel_weight_layer.")[-1]: v.detach().cpu().double() for k, v in state.items() if v.is_floating_point()}      # (DiscoFusion's or the layer's own names)
    h = cat
    for i in (1, 2, 3, 4):
        w = sd[f"conv1_{i}.weight"].flatten(1)
        h = torch.einsum("oc,nchw->nohw", w, h) + sd[f"conv1_{i}.bias"].view(1, -1, 1, 1)
        if i < 4:
            scale = sd[f"bn1_{i}.weight"] / torch.sqrt(sd[f"bn1_{i}.running_var"] + EPS)
            h = (h - sd[f"bn1_{i}.running_mean"].view(1, -1, 1, 1)) * scale.view(1, -1, 1, 1) + sd[f"bn1_{i}.bias"].view(1, -1, 1, 1)
        h = torch.relu(h)
    return h[:, 0]


def disco_fuse_f64(state: dict, x: torch.Tensor, theta: torch.Tensor):
    """One frame.  -> (fused [C, H, W] float64, logits [n, H, W], softmax weights [n, H, W])."""
    xw = warp_f64(x, theta)
    n = xw.shape[0]
    ego = x[:1].detach().cpu().double().expand(n, -1, -1, -1)
    s = logits_f64(state, torch.cat((xw, ego), dim=1))
    a = torch.softmax(s, dim=0)
    return (a.unsqueeze(1) * xw).sum(0), s, a


def assert_not_degenerate(s: torch.Tensor, a: torch.Tensor, what="") -> None:
    """The MLP must be visible in the result: at least half of the (pixel, agent) logits positive; with more than one agent, at least a quarter of the pixels with
    softmax weights that differ by more than 0.1 between agents."""
    assert float((s > 0).double().mean()) >= 0.5, (what, "share of positive logits", float((s > 0).double().mean()))
    if a.shape[0] > 1:
        spread = (a.max(0).values - a.min(0).values) > 0.1
        assert float(spread.double().mean()) >= 0.25, (what, "share of pixels with distinct weights", float(spread.double().mean()))
