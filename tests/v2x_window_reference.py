"""V2X-ViT's pyramid window attention for the tests: ONE ``PreNorm(PyramidWindowAttention)`` layer with its residual restated in float64 from the UNFOLDED
``state_dict`` (not the code under test, none of the folds of ``v2xvit.folded_window_attention``) -- the yardstick of ``ops.v2x_window_attention`` in
tests/test_v2x_window_gpu.py and of ``v2xvit.window_attention_reduced`` in tests/test_v2x_window_cpu.py.

The layer (PyramidWindowAttention over BaseWindowAttention, sub_modules/mswin.py:19-121, SplitAttn with RadixSoftmax, split_attn.py:6-63, under PreNorm,
base_transformer.py:7-14, and the residual of v2xvit_basic.py:118-122), per map, branch b with windows of ws x ws tokens and m heads:

    y      = LayerNorm(x), eps = 1e-5
    q, k, v = to_qkv_b(y) cut in three, each cut into m heads of consecutive channels
    att    = softmax_j( q_i . k_j / sqrt(dim_head) + pos_b[xj - xi + ws - 1][yj - yi + ws - 1] )      tokens i = xi ws + yi, j = xj ws + yj of one window, x the row
    out_b  = to_out_b( concat_heads( sum_j att_ij v_j ) )
    naive:      out = x + (out_0 + out_1 + out_2) / 3
    split_attn: gap = mean_HW(out_0 + out_1 + out_2);  a = softmax_b( fc2(relu(LayerNorm(fc1(gap)))) viewed [3, C] );  out = x + sum_b a_b * out_b

It runs on the device of ``x`` (float64 either way).  ``probe`` collects what the examination of tests/test_v2x_window_cpu.py looks at; ``transpose_pos`` and
``channel_major_heads`` are deliberately WRONG variants that examination uses to show the yardstick tells them apart.
"""
import torch


def _relative_bias(pos: torch.Tensor, ws: int, transposed: bool) -> torch.Tensor:
    """[ws^2, ws^2]: entry (i, j) = pos[xj - xi + ws - 1][yj - yi + ws - 1]."""
    t = torch.arange(ws * ws, device=pos.device)
    row, col = t // ws, t % ws
    dr, dc = row[None, :] - row[:, None] + ws - 1, col[None, :] - col[:, None] + ws - 1
    return pos[dc, dr] if transposed else pos[dr, dc]


def window_attention_f64(state: dict, x: torch.Tensor, windows, heads, fuse: str, probe: dict = None, transpose_pos: bool = False, channel_major_heads: int = None) -> torch.Tensor:
    """state: the ``state_dict`` of ``PreNorm(C, PyramidWindowAttention(...))``; x [n, H, W, C] -> x + layer, [n, H, W, C] float64 on x's device."""
    dev = x.device
    sd = {k: v.detach().to(device=dev, dtype=torch.float64) for k, v in state.items()}
    x = x.detach().double()
    n, H, W, C = x.shape
    mu = x.mean(dim=-1, keepdim=True)
    var = ((x - mu) ** 2).mean(dim=-1, keepdim=True)
    y = (x - mu) / torch.sqrt(var + 1e-5) * sd["norm.weight"] + sd["norm.bias"]
    outs = []
    for b, (ws, m) in enumerate(zip(windows, heads)):
        w = sd[f"fn.pwmsa.{b}.to_qkv.weight"]
        inner = w.shape[0] // 3
        dh = inner // m
        nh, nw = H // ws, W // ws
        swapped = channel_major_heads == b

        def cut(t):      # [n, H, W, inner] -> [n, nh, nw, m, ws ws, dh]
            if swapped:
                t = t.reshape(n, nh, ws, nw, ws, dh, m).transpose(-1, -2)
            else:
                t = t.reshape(n, nh, ws, nw, ws, m, dh)
            return t.permute(0, 1, 3, 5, 2, 4, 6).reshape(n, nh, nw, m, ws * ws, dh)
        proj = y @ w.t()
        q, k, v = cut(proj[..., :inner]), cut(proj[..., inner:2 * inner]), cut(proj[..., 2 * inner:])
        scores = q @ k.transpose(-1, -2) / dh ** 0.5 + _relative_bias(sd[f"fn.pwmsa.{b}.pos_embedding"], ws, transpose_pos)
        att = torch.softmax(scores, dim=-1)
        if probe is not None:
            probe.setdefault("top", []).append((ws * ws, att.max(dim=-1)[0].flatten()))
        o = (att @ v).reshape(n, nh, nw, m, ws, ws, dh).permute(0, 1, 4, 2, 5, 3, 6)      # n nh ws nw ws m dh
        if swapped:
            o = o.transpose(-1, -2)
        o = o.reshape(n, H, W, inner)
        outs.append(o @ sd[f"fn.pwmsa.{b}.to_out.0.weight"].t() + sd[f"fn.pwmsa.{b}.to_out.0.bias"])
    if fuse == "naive":
        return x + (outs[0] + outs[1] + outs[2]) / 3
    assert fuse == "split_attn"
    gap = (outs[0] + outs[1] + outs[2]).mean(dim=(1, 2))                                      # [n, C]
    h = gap @ sd["fn.split_attn.fc1.weight"].t()
    hm = h.mean(dim=-1, keepdim=True)
    hv = ((h - hm) ** 2).mean(dim=-1, keepdim=True)
    h = torch.relu((h - hm) / torch.sqrt(hv + 1e-5) * sd["fn.split_attn.bn1.weight"] + sd["fn.split_attn.bn1.bias"])
    a = torch.softmax((h @ sd["fn.split_attn.fc2.weight"].t()).reshape(n, 3, C), dim=1)
    if probe is not None:
        probe["a"] = a
    return x + sum(a[:, b, None, None, :] * outs[b] for b in range(3))
