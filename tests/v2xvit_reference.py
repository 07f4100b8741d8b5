"""V2X-ViT's fusion for the tests: the recorded cases of tests/golden/v2xvit_fuse.npz (shared with tests/golden/make_v2xvit_golden.py, which records the reference's
output on them), the examination that a case SEES every block, and ONE agent-attention layer restated in float64 (not the code under test) -- the yardstick of
``ops.v2x_agent_attention`` in tests/test_v2xvit_gpu.py.

The layer (HGTCavAttention.forward, sub_modules/hmsa.py:110-151, under PreNorm, base_transformer.py:7-14, and the residual of v2xvit_basic.py:118-122; all agents of
type 0), per pixel, from the UNFOLDED ``state_dict``:

    xw_j  = warp(x_j, theta_j)  (tests/disco_reference.py: float32 sampling positions)  |  x_j
    y_j   = LayerNorm(xw_j), eps = 1e-5
    q, k, v = the type-0 linears of y, split into heads
    att   = softmax_j( q_i^T relation_att[0] k_j / sqrt(dim_head) )
    out_i = xw_i + a_linear( concat_heads( sum_j att_ij relation_msg[0]^T v_j ) )

Everything after the sampling positions is float64; none of the folds of ``v2xvit.folded_agent_attention`` is used.
"""
import copy

import numpy as np
import torch

from disco_reference import warp_f64
from v2v_reference import make_thetas

H, W = 8, 16


def args(dim, heads, dim_head, pheads, pdim_head, windows, fuse, depth, use_rte=False):
    return {"transformer": {"encoder": {
        "num_blocks": 1, "depth": depth, "use_roi_mask": True, "use_RTE": use_rte, "RTE_ratio": 0,
        "cav_att_config": {"dim": dim, "use_hetero": True, "use_RTE": use_rte, "RTE_ratio": 0, "heads": heads, "dim_head": dim_head, "dropout": 0.3},
        "pwindow_att_config": {"dim": dim, "heads": pheads, "dim_head": pdim_head, "dropout": 0.3, "window_size": windows, "relative_pos_embedding": True, "fusion_method": fuse},
        "feed_forward": {"mlp_dim": dim, "dropout": 0.3},
        "sttf": {"voxel_size": [0.4, 0.4, 4], "downsample_rate": 4}}}}


ARGS_A = args(32, 2, 16, [4, 2, 1], [8, 16, 32], [2, 4, 8], "naive", 2)
ARGS_B = args(256, 8, 32, [16, 8, 4], [16, 32, 64], [2, 4, 8], "split_attn", 1)
SEED_A, SEED_B = 40, 41


def affines(L=5):
    """normalized_affine_matrix [2, L, L, 2, 3] float64: frame 0's three agents with every receiver row filled (row 0: identity, a rotation with a shift, the last
    agent half outside); identity elsewhere."""
    A = torch.zeros(2, L, L, 2, 3, dtype=torch.float64)
    A[..., 0, 0] = A[..., 1, 1] = 1.0
    A[0, :3, :3] = make_thetas(3, H, W, seed=40)
    return A


def inputs(C, seed):
    return torch.randn(4, C, H, W, generator=torch.Generator().manual_seed(seed)), torch.tensor([3, 1]), affines()


def weight_checksum(module):
    sd = module.state_dict()
    return np.array([float(sum(v.double().sum() for v in sd.values())), float(sum(v.double().abs().sum() for v in sd.values()))])


def examine(a, seed, x, rl, A, what):
    """float64 (this package's restatement: the reference's STTF mixes float32 grids with the map's dtype and runs in float32 only): the softmax of the agent
    attention is neither uniform nor saturated; each block, taken out, moves the output."""
    from coalign_amd.fusion import V2XViTFusion
    from coalign_amd.synthetic import v2xvit_parameters_
    m = V2XViTFusion(copy.deepcopy(a))
    v2xvit_parameters_(m, seed=seed)
    m = m.double().eval()
    tops = []
    hooks = [mod.register_forward_hook(lambda _m, _i, o: tops.append(o[0, :, :, :, :3, :3].max(dim=-1)[0].flatten()))      # frame 0: three real agents
             for n, mod in m.named_modules() if n.endswith("fn.attend")]
    with torch.no_grad():
        ref = m(x.double(), rl, A)
    for h in hooks:
        h.remove()
    top = torch.cat(tops)
    share = float(((top > 1 / 3 + 0.05) & (top < 0.95)).double().mean())
    assert share > 0.5, (what, "share of softmax rows neither uniform nor saturated", share)
    scale = float(ref.abs().max())
    moved = {}
    for kind, pick in (("agent attention", lambda layer: layer[0].layers[0][0]), ("window attention", lambda layer: layer[0].layers[0][1]), ("feed-forward", lambda layer: layer[1])):
        for d, layer in enumerate(m.fusion_net.encoder.layers):
            pre = pick(layer)
            saved = pre.forward
            pre.forward = lambda t, **k: torch.zeros_like(t)
            with torch.no_grad():
                out = m(x.double(), rl, A)
            pre.forward = saved
            moved[f"{kind} {d}"] = float((out - ref).abs().max()) / scale
    assert min(moved.values()) > 100 * 1.1e-4, (what, moved)
    print(what, "share of unsaturated softmax rows", round(share, 3), "output moved by", {k: round(v, 3) for k, v in moved.items()})
    return share, min(moved.values())


def agent_attention_f64(state: dict, x: torch.Tensor, theta, heads: int) -> torch.Tensor:
    """state: the ``state_dict`` of ``PreNorm(dim, HGTCavAttention)``; x [n, H, W, C]; theta [n, 2, 3] or None -> x + attention, [n, H, W, C] float64, every receiver."""
    sd = {k: v.detach().cpu().double() for k, v in state.items()}
    x = x.detach().cpu().double()
    if theta is not None:
        x = warp_f64(x.permute(0, 3, 1, 2), theta).permute(0, 2, 3, 1)
    n, Hh, Ww, C = x.shape
    mu = x.mean(dim=-1, keepdim=True)
    var = ((x - mu) ** 2).mean(dim=-1, keepdim=True)
    y = (x - mu) / torch.sqrt(var + 1e-5) * sd["norm.weight"] + sd["norm.bias"]

    def lin(name):
        return (y @ sd[f"fn.{name}.0.weight"].t() + sd[f"fn.{name}.0.bias"]).reshape(n, Hh, Ww, heads, -1)
    q, k, v = lin("q_linears"), lin("k_linears"), lin("v_linears")
    dh = q.shape[-1]
    A, M = sd["fn.relation_att"][0], sd["fn.relation_msg"][0]                # [heads, dh, dh]
    ak = torch.einsum("mpq,jhwmq->jhwmp", A, k)
    att = torch.softmax(torch.einsum("ihwmp,jhwmp->hwmij", q, ak) / dh ** 0.5, dim=-1)
    mv = torch.einsum("mpc,jhwmp->jhwmc", M, v)
    o = torch.einsum("hwmij,jhwmc->ihwmc", att, mv).reshape(n, Hh, Ww, -1)
    return x + o @ sd["fn.a_linears.0.weight"].t() + sd["fn.a_linears.0.bias"]
