"""V2VNet's message passing restated in float64 (not the code under test): the yardstick of tests/test_v2v_gpu.py and tests/test_v2v_cpu.py.

The reference's UNREDUCED loops (V2VNetFusion.forward, fuse_modules/fusion_in_one.py:197-293, with ConvGRUCell.forward, sub_modules/convgru.py:48-70), one frame:

    mask_ij = warp(ones, theta_ij)                               every receiver i and sender j; the warp of tests/disco_reference.py (float32 sampling positions)
    per iteration, for EVERY agent i:
        m_ij  = msg_cnn([warp(x_j, theta_ij) | x_i]) * mask_ij   the full 2C -> C convolution per pair, bias included
        agg_i = max_j m_ij  |  mean_j m_ij
        x_i'  = ConvGRU([x_i | agg_i]) with a zero hidden state: both full convolutions over [input | h = 0], reset gate and (1 - z) h + z tanh(.) as written
              | x_i + agg_i  without the GRU
    out = mlp(x_0) after the last iteration

Everything after the sampling positions is float64.  None of the three identities of ``V2VNetFusion.forward_reduced`` is used here.
"""
import math

import torch
import torch.nn.functional as F

from disco_reference import warp_f64


def make_thetas(n: int, H: int, W: int, seed: int = 0, outside: bool = True) -> torch.Tensor:
    """normalized affine rows [n, n, 2, 3] float64 for ALL receivers: identity on the diagonal; off it a rotation of up to 25 degrees (with the aspect terms of a
    normalised matrix) and a sub-pixel-odd shift; receiver 0 sees its LAST sender half outside the map (n >= 2) and, with ``outside`` and n >= 4, sender n - 2
    wholly outside (mask exactly zero)."""
    g = torch.Generator().manual_seed(1000 + seed)
    th = torch.zeros(n, n, 2, 3, dtype=torch.float64)
    for i in range(n):
        for j in range(n):
            if i == j:
                th[i, j, 0, 0] = th[i, j, 1, 1] = 1.0
                continue
            ang = float((torch.rand((), generator=g) - 0.5) * 2 * math.radians(25))
            sx, sy = [float(v) for v in (torch.rand(2, generator=g) - 0.5) * 0.5]
            c, s = math.cos(ang), math.sin(ang)
            th[i, j] = torch.tensor([[c, -s * H / W, sx], [s * W / H, c, sy]], dtype=torch.float64)
    if n >= 2:
        th[0, n - 1] = torch.tensor([[1.0, 0.0, 1.03], [0.0, 1.0, 0.01]], dtype=torch.float64)      # the right half of the ego grid falls outside this sender
    if outside and n >= 4:
        th[0, n - 2] = torch.tensor([[1.0, 0.0, 3.1], [0.0, 1.0, 0.2]], dtype=torch.float64)        # wholly outside
    return th


def student_t(shape, seed: int, scale: float = 1.0, df: float = 4.0) -> torch.Tensor:
    """Heavy-tailed float32 maps (Student-t, 4 degrees of freedom), as the backbone's activations are."""
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(shape, generator=g, dtype=torch.float64)
    chi = sum(torch.randn(shape, generator=g, dtype=torch.float64) ** 2 for _ in range(int(df))) / df
    return (z / chi.sqrt() * scale).float()


def v2v_fuse_f64(state: dict, x: torch.Tensor, theta_full: torch.Tensor, args: dict, iterations=None, trace=None) -> torch.Tensor:
    """One frame: x [n, C, H, W], theta_full [n, n, 2, 3] -> the fused map [C, H, W] float64.  ``iterations`` overrides args['num_iteration'];
    ``trace`` (a dict) receives 'masks' [n, n, H, W], 'argmax' (the winning sender per element of the ego's first aggregation) and 'update_gates' (every cell's)."""
    sd = {k.split("fusion_net.")[-1]: v.detach().cpu().double() for k, v in state.items()}
    x = x.detach().cpu().double()
    n, C, H, W = x.shape
    th = theta_full.detach().cpu().double()
    K = args["num_iteration"] if iterations is None else iterations
    layers = args["conv_gru"]["num_layers"]
    ones = torch.ones(n, 1, H, W, dtype=torch.float64)
    masks = torch.stack([warp_f64(ones, th[i]) for i in range(n)])                     # [n (receiver), n (sender), 1, H, W]
    if trace is not None:
        trace["masks"], trace["update_gates"] = masks[:, :, 0], []
    for it in range(K):
        new = []
        for i in range(n):
            cat = torch.cat([warp_f64(x, th[i]), x[i:i + 1].expand(n, -1, -1, -1)], dim=1)
            m = F.conv2d(cat, sd["msg_cnn.weight"], sd["msg_cnn.bias"], padding=1) * masks[i]
            if args["agg_operator"] == "max":
                agg, arg = m.max(dim=0)
                if trace is not None and it == 0 and i == 0:
                    trace["argmax"] = arg
            elif args["agg_operator"] == "avg":
                agg = m.mean(dim=0)
            else:
                raise ValueError("agg_operator has wrong value")
            if args["gru_flag"]:
                inp = torch.cat([x[i], agg], dim=0).unsqueeze(0)
                for k in range(layers):
                    p = f"conv_gru.cell_list.{k}."
                    hid = sd[p + "conv_can.weight"].shape[0]
                    h = torch.zeros(1, hid, H, W, dtype=torch.float64)
                    pad = sd[p + "conv_can.weight"].shape[-1] // 2
                    gates = F.conv2d(torch.cat([inp, h], dim=1), sd[p + "conv_gates.weight"], sd[p + "conv_gates.bias"], padding=pad)
                    reset, update = torch.sigmoid(gates[:, :hid]), torch.sigmoid(gates[:, hid:])
                    cnm = torch.tanh(F.conv2d(torch.cat([inp, reset * h], dim=1), sd[p + "conv_can.weight"], sd[p + "conv_can.bias"], padding=pad))
                    inp = (1 - update) * h + update * cnm
                    if trace is not None:
                        trace["update_gates"].append(update.flatten())
                new.append(inp[0])
            else:
                new.append(x[i] + agg)
        x = torch.stack(new)
    return (x[0].permute(1, 2, 0) @ sd["mlp.weight"].t() + sd["mlp.bias"]).permute(2, 0, 1)


def assert_not_degenerate(state: dict, x: torch.Tensor, theta_full: torch.Tensor, args: dict, ref: torch.Tensor, trace: dict, what="", rtol=1e-4, floor=1e-5) -> None:
    """The case must SEE every stage (run before every parity assertion; ``ref`` and ``trace`` from ``v2v_fuse_f64`` of the same case).  With more than one agent: masks strictly between 0 and 1, exactly 0 and exactly 1 all
    occur; the arg-max sender varies over the pixels (max); zeroing a non-ego agent changes the output by more than ten times the bound (an error in that agent's
    path is of the order of its contribution, which then lies outside the bound).  With the GRU: most update gates lie in (0.1, 0.9).  Always:
    K iterations differ from K - 1 by more than a hundred times the comparison bound (rtol + floor of the scale)."""
    n = x.shape[0]
    scale = float(ref.abs().max())
    bound = (rtol + floor) * scale
    assert scale > 0 and bool(torch.isfinite(ref).all()), what
    fewer = v2v_fuse_f64(state, x, theta_full, args, iterations=args["num_iteration"] - 1)
    assert float((ref - fewer).abs().max()) > 100 * bound, (what, "the last iteration is invisible", float((ref - fewer).abs().max()) / scale)
    if args["gru_flag"]:
        z = torch.cat(trace["update_gates"])
        share = float(((z > 0.1) & (z < 0.9)).double().mean())
        assert share > 0.5, (what, "share of unsaturated update gates", share)
    if n > 1:
        m = trace["masks"]
        one = (m - 1).abs() < 1e-12
        single = x.shape[2] * x.shape[3] == 1      # (one pixel per pair: the n * n masks of a 1 x 1 map hold a zero only where a sender lies wholly outside)
        assert (single or bool((m == 0).any())) and bool(one.any()) and bool(((m > 1e-6) & (m < 1 - 1e-6)).any()), (what, "masks: 0, 1 and fractions must all occur")
        if args["agg_operator"] == "max" and x.shape[2] * x.shape[3] > 1:
            wins = torch.bincount(trace["argmax"].flatten(), minlength=n).double() / trace["argmax"].numel()
            assert int((wins > 0.05).sum()) >= 2, (what, "one sender wins the max everywhere", wins.tolist())
        x0 = x.clone()
        x0[1] = 0
        without = v2v_fuse_f64(state, x0, theta_full, args)
        assert float((ref - without).abs().max()) > 10 * bound, (what, "agent 1 is invisible", float((ref - without).abs().max()) / scale)
