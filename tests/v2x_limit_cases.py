"""The limit cases of V2X-ViT's three kernels (csrc/v2x_attn.hip, csrc/v2x_window.hip, csrc/v2x_ffn.hip), shared by tests/test_v2x_limits_cpu.py (the float32 op-by-op
layer on the CPU must stay within HALF of the bound on every one of them: no case asks of a kernel what float32 cannot do) and tests/test_v2x_limits_gpu.py (the
kernels against the float64 restatements of tests/v2xvit_reference.py, tests/v2x_window_reference.py and tests/v2x_ffn_reference.py).

``token_bound`` is the project's element-wise bound (rtol 1e-4, floor 1e-5) with the floor's scale taken PER TOKEN: a whole-tensor scale lets one token of mean 1e4
set a floor of 0.1 for every unit token of the map, and LayerNorm's edge tokens or agents of mixed scale then hide behind it.

``plant`` writes LayerNorm's edge tokens into a map.  The layer builders start from ``synthetic.v2xvit_parameters_`` (deep copies; the cached originals stay as they
are) and push one thing to its end: saturated softmax rows (queries x 16 / x 12), a position table that dominates the scores (x 30), nearly one-hot branch weights
(``split_attn.fc2`` x 40), and a value projection whose static bound -- max_r ||w_r||_2 sqrt(C) + |b_r| over the folded rows, what ``ops.pack_v2x*_weights`` guarantee to
stay below 65504 -- lands at 0.98 (packed) or 1.05 (refused) of 65504.  ``aligned_token`` is the token that comes within a few per cent of that bound; random tokens
reach 0.2 - 0.4 of it."""
import copy
import functools
import math
import zlib
from collections import namedtuple

import torch

from coalign_amd.synthetic import v2xvit_parameters_
from coalign_amd.v2xvit import (FeedForward, HGTCavAttention, PreNorm, PyramidWindowAttention, folded_agent_attention, folded_feed_forward,
                                folded_window_attention)
from disco_reference import warp_f64
from v2v_reference import make_thetas
from v2x_ffn_reference import feed_forward_f64
from v2x_window_reference import window_attention_f64
from v2xvit_reference import agent_attention_f64

EDGE = 65504.0                                                       # the largest finite fp16
INSIDE, OUTSIDE = 0.98, 1.05                                          # the static bound of the range-edge layers, as fractions of EDGE
WINDOWS, DIM_HEADS = [4, 8, 16], [16, 32, 64]
WINDOW_CONFIGS = {"C64_naive": (64, "naive"), "C256_naive": (256, "naive"), "C256_split_attn": (256, "split_attn")}
# (64, 416) | (64, 448) and (256, 224) | (256, 256, in tests/test_v2x_ffn_gpu.py) straddle the 64 KB of dynamic LDS: 32 (4 C + 16 + 4 M + 16) bytes; M = 32 is one row
# tile for four wavefronts; (64, 512) the largest tile of the <64> instantiation
FFN_SHAPES = ((64, 32), (64, 416), (64, 448), (64, 512), (256, 32), (256, 224))
AGENT_SCALES = (1e-2, 1e2, 1.0, 1e-3, 1e3, 1.0, 30.0, 0.1)

Case = namedtuple("Case", "name variant x theta receivers", defaults=(None, (None,)))


def token_bound(got: torch.Tensor, ref: torch.Tensor) -> float:
    """got, ref [..., C] -> the worst |got - ref| / (1e-4 |ref| + 1e-5 max_c |ref[token]|) over the elements; at most 1 means inside.  A non-finite element of ``got``,
    or an error where the bound is zero, gives inf."""
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    assert got.shape == ref.shape, (tuple(got.shape), tuple(ref.shape))
    assert bool(torch.isfinite(ref).all())
    if not bool(torch.isfinite(got).all()):
        return math.inf
    err = (got - ref).abs()
    bound = 1e-4 * ref.abs() + 1e-5 * ref.abs().amax(dim=-1, keepdim=True)
    ratio = torch.where(err > 0, err / bound.clamp(min=1e-300), torch.zeros_like(err))
    return float(ratio.max()) if ratio.numel() else 0.0


def _gen(*key) -> torch.Generator:
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()) & 0x7FFFFFFF)


def _randn(*shape, key) -> torch.Tensor:
    return torch.randn(*shape, generator=_gen(*key))


def _one_channel(C, g):
    t = torch.zeros(C)
    t[int(torch.randint(C, (), generator=g))] = 1e3
    return t


# LayerNorm's edge tokens.  (Dropped on purpose: 3 + 1e-3 randn -- the float32 op-by-op layer itself reaches 1.3 - 1.9 of the per-token bound on it with range-edge
# feed-forward weights -- and an offset of 100, where it reaches 0.5.)
PLANTED = (("constant 3.0 (variance 0)", lambda C, g: torch.full((C,), 3.0)),
           ("all zero", lambda C, g: torch.zeros(C)),
           ("10 + randn", lambda C, g: 10.0 + torch.randn(C, generator=g)),
           ("30 + randn", lambda C, g: 30.0 + torch.randn(C, generator=g)),
           ("one channel at 1e3, the rest 0", _one_channel),
           ("randn x 1e-3 (variance below eps)", lambda C, g: torch.randn(C, generator=g) * 1e-3),
           ("randn x 1e3", lambda C, g: torch.randn(C, generator=g) * 1e3))
TINY = 5                                                              # the index of the token whose variance is below LayerNorm's eps


def plant(x: torch.Tensor, g: torch.Generator, agent: int = 0, only=None) -> torch.Tensor:
    """x [n, H >= 2, W >= 7, C]: the tokens of ``PLANTED`` (all, or those whose index is in ``only``) into row 1 of map ``agent``, token k at column k.  In place."""
    C = x.shape[-1]
    assert x.dim() == 4 and x.shape[1] >= 2 and x.shape[2] >= len(PLANTED)
    for k, (_, make) in enumerate(PLANTED):
        t = make(C, g)                                                # (every token is drawn, so that a token does not depend on ``only``)
        if only is None or k in only:
            x[agent, 1, k] = t.to(x.dtype)
    return x


def static_bound(w: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """w [rows, C], b [rows] (folded onto yhat = (x - mean) / sqrt(var + eps)) -> per row ||w_r||_2 sqrt(C) + |b_r| in float64: sum yhat^2 <= C and Cauchy-Schwarz."""
    w, b = w.detach().double(), b.detach().double()
    return (w * w).sum(dim=1).sqrt() * math.sqrt(w.shape[1]) + b.abs()


def aligned_token(w: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """The token that drives the worst row r of (w, b) towards its static bound: 2.5 sqrt(C) times w_r made mean-free and normalised, with the sign of b_r.  LayerNorm
    maps it to sqrt(C) times that direction (its variance 6.25 dwarfs eps)."""
    r = int(static_bound(w, b).argmax())
    u = w[r].detach().double() - w[r].detach().double().mean()
    sign = -1.0 if float(b[r]) < 0 else 1.0
    return (2.5 * math.sqrt(w.shape[1]) * sign * u / u.norm()).float()


# ---- the folded value rows of a layer (float64) ----------------------------------------------------------------------------------------------------------------
def agent_value_rows(layer):
    d = copy.deepcopy(layer).double()
    wqkv, bqkv, _, _ = folded_agent_attention(d.norm, d.fn, True)
    C = wqkv.shape[1]
    return wqkv[2 * C:].detach(), bqkv[2 * C:].detach()


def window_value_rows(layer, b):
    d = copy.deepcopy(layer).double()
    wqkv, bqkv = folded_window_attention(d.norm, d.fn)[:2]
    C = wqkv.shape[1]
    return wqkv[3 * C * b + 2 * C:3 * C * (b + 1)].detach(), bqkv[3 * C * b + 2 * C:3 * C * (b + 1)].detach()


def ffn_hidden_rows(layer):
    d = copy.deepcopy(layer).double()
    w1, b1, _, _ = folded_feed_forward(d.norm, d.fn)
    return w1.detach(), b1.detach()


# ---- layers ------------------------------------------------------------------------------------------------------------------------------------------------------
def _window_heads(C):
    return [C // d for d in DIM_HEADS]


@functools.lru_cache(maxsize=None)
def _agent_base(C):
    layer = PreNorm(C, HGTCavAttention(C, heads=C // 32, dim_head=32))
    v2xvit_parameters_(layer, seed=C)
    return layer.eval()


@functools.lru_cache(maxsize=None)
def _window_base(config):
    C, fuse = WINDOW_CONFIGS[config]
    layer = PreNorm(C, PyramidWindowAttention(C, _window_heads(C), DIM_HEADS, 0.1, WINDOWS, True, fuse))
    v2xvit_parameters_(layer, seed=C + len(fuse))
    return layer.eval()


@functools.lru_cache(maxsize=None)
def _ffn_base(C, M):
    layer = PreNorm(C, FeedForward(C, M, 0.3))
    v2xvit_parameters_(layer, seed=C + M)
    return layer.eval()


def scale_agent_values_(layer, frac):
    """v_linears[0] (weight and bias: the folded v' rows and their bias are linear in both) scaled so that the static bound of |v'| is ``frac`` x 65504.  In place."""
    s = frac * EDGE / float(static_bound(*agent_value_rows(layer)).max())
    with torch.no_grad():
        layer.fn.v_linears[0].weight.mul_(s)
        layer.fn.v_linears[0].bias.mul_(s)
    return layer


def scale_window_values_(layer, frac):
    """The v third of every branch's bias-free ``to_qkv`` scaled so that the static bound of every branch's |v| is ``frac`` x 65504.  In place."""
    for b, att in enumerate(layer.fn.pwmsa):
        s = frac * EDGE / float(static_bound(*window_value_rows(layer, b)).max())
        inner = att.to_qkv.weight.shape[0] // 3
        with torch.no_grad():
            att.to_qkv.weight[2 * inner:].mul_(s)
    return layer


def scale_ffn_hidden_(layer, frac):
    """The first linear (weight and bias) scaled so that the static bound of the hidden pre-activations is ``frac`` x 65504.  In place."""
    s = frac * EDGE / float(static_bound(*ffn_hidden_rows(layer)).max())
    with torch.no_grad():
        layer.fn.net[0].weight.mul_(s)
        layer.fn.net[0].bias.mul_(s)
    return layer


@functools.lru_cache(maxsize=None)
def agent_layer(C, variant="base"):
    """PreNorm(HGTCavAttention) in float32 on the CPU, eval mode.  Cached: callers copy before they change or move it."""
    layer = copy.deepcopy(_agent_base(C))
    with torch.no_grad():
        if variant == "q16":                                          # logits to +-80: more than half the rows with a top weight above 0.999
            layer.fn.q_linears[0].weight.mul_(16.0)
            layer.fn.q_linears[0].bias.mul_(16.0)
        elif variant in ("edge", "outside"):
            scale_agent_values_(layer, INSIDE if variant == "edge" else OUTSIDE)
        else:
            assert variant == "base", variant
    return layer


@functools.lru_cache(maxsize=None)
def window_layer(config, variant="base"):
    """PreNorm(PyramidWindowAttention) in float32 on the CPU, eval mode.  Cached: callers copy before they change or move it."""
    layer = copy.deepcopy(_window_base(config))
    with torch.no_grad():
        if variant == "q12":                                          # a quarter to a half of the rows with a top weight above 0.99
            for att in layer.fn.pwmsa:
                att.to_qkv.weight[:att.to_qkv.weight.shape[0] // 3].mul_(12.0)
        elif variant == "pos30":                                      # entries to +-54: the table dominates the scores
            for att in layer.fn.pwmsa:
                att.pos_embedding.mul_(30.0)
        elif variant == "fc2x40":                                     # nearly one-hot branch weights
            layer.fn.split_attn.fc2.weight.mul_(40.0)
        elif variant in ("edge", "outside"):
            scale_window_values_(layer, INSIDE if variant == "edge" else OUTSIDE)
        else:
            assert variant == "base", variant
    return layer


@functools.lru_cache(maxsize=None)
def ffn_layer(C, M, variant="base"):
    """PreNorm(FeedForward) in float32 on the CPU, eval mode.  Cached: callers copy before they change or move it."""
    layer = copy.deepcopy(_ffn_base(C, M))
    if variant in ("edge", "outside"):
        scale_ffn_hidden_(layer, INSIDE if variant == "edge" else OUTSIDE)
    else:
        assert variant == "base", variant
    return layer


# ---- the cases ---------------------------------------------------------------------------------------------------------------------------------------------------
AGENT_GROUPS = ("counts", "maps", "planted", "scales", "q16", "edge")
WINDOW_GROUPS = ("counts", "columns", "planted", "q12", "pos30", "fc2x40", "edge")
FFN_GROUPS = ("tokens", "planted", "edge")
WINDOW_PARAMS = [(config, group) for config, (_, fuse) in WINDOW_CONFIGS.items() for group in WINDOW_GROUPS if group != "fc2x40" or fuse == "split_attn"]


def _both(n, H, W):
    return ((None, "in place"), (make_thetas(n, H, W, seed=n)[0], "warp"))


def agent_cases(C, group):
    """-> [Case]: x [n, H, W, C] float32, theta [n, 2, 3] float64 or None, the receiver counts to run."""
    out = []
    if group == "counts":                                             # every n: 4, 6 and 7 leave -inf slots behind the live ones as 1, 2, 3 and 5 do, 8 leaves none
        for n in range(1, 9):
            x = _randn(n, 5, 7, C, key=("agent", C, "counts", n))
            for th, how in _both(n, 5, 7):
                out.append(Case(f"n={n} 5x7 {how}", "base", x, th, tuple(sorted({n, 1}))))
    elif group == "maps":                                             # H W = 1, 31, 32, 33 around the 32-pixel tile; W = 1 and H = 1 under a warp
        for H, W in ((1, 1), (1, 31), (32, 1), (1, 33), (33, 1)):
            x = _randn(3, H, W, C, key=("agent", C, "maps", H, W))
            for th, how in _both(3, H, W):
                out.append(Case(f"n=3 {H}x{W} {how}", "base", x, th, (1, 3)))
    elif group == "planted":
        for agent, who in ((0, "the ego's map"), (1, "a sender's map")):
            x = plant(_randn(3, 5, 7, C, key=("agent", C, "planted", agent)), _gen("agent", C, "plant", agent), agent)
            out.append(Case(f"n=3 5x7 planted tokens in {who}", "base", x, None, (1, 3)))
    elif group == "scales":
        x = _randn(8, 5, 7, C, key=("agent", C, "scales")) * torch.tensor(AGENT_SCALES)[:, None, None, None]
        for th, how in _both(8, 5, 7):
            out.append(Case(f"n=8 5x7 agents at scales {AGENT_SCALES} {how}", "base", x, th, (1, 8)))
    elif group == "q16":
        for n in (3, 8):
            x = _randn(n, 5, 7, C, key=("agent", C, "q16", n))
            for th, how in _both(n, 5, 7):
                out.append(Case(f"q x 16 n={n} 5x7 {how}", "q16", x, th, tuple(sorted({n, 1}))))
    elif group == "edge":                                             # with n = 1 the attention output IS v' of the token
        tok = aligned_token(*agent_value_rows(agent_layer(C, "edge")))
        for n in (1, 3):
            x = _randn(n, 5, 7, C, key=("agent", C, "edge", n))
            x[0, 0, 0] = tok
            x[0, 4, 6] = tok                                          # the last pixel of the partial tile
            out.append(Case(f"static bound at {INSIDE} x 65504, n={n} 5x7, aligned token in agent 0", "edge", x, None, tuple(sorted({n, 1}))))
    else:
        raise KeyError(group)
    return out


def window_cases(config, group):
    """-> [Case]: x [n, H, W, C] float32 (theta and receivers unused)."""
    C, fuse = WINDOW_CONFIGS[config]
    out = []
    if group == "counts":
        for n in (3, 4, 6, 7):
            out.append(Case(f"n={n} 16x16", "base", _randn(n, 16, 16, C, key=("window", config, "counts", n))))
    elif group == "columns":                                          # one window column / one window row of the 16-windows
        for H, W in ((48, 16), (16, 48)):
            out.append(Case(f"n=1 {H}x{W}", "base", _randn(1, H, W, C, key=("window", config, "columns", H))))
    elif group == "planted":
        x = plant(_randn(2, 16, 16, C, key=("window", config, "planted")), _gen("window", config, "plant"))
        out.append(Case("n=2 16x16 planted tokens in map 0", "base", x))
    elif group in ("q12", "pos30", "fc2x40"):
        assert group != "fc2x40" or fuse == "split_attn", (config, group)
        out.append(Case(f"{group} n=2 16x16", group, _randn(2, 16, 16, C, key=("window", config, group))))
    elif group == "edge":
        layer = window_layer(config, "edge")
        x = _randn(2, 16, 16, C, key=("window", config, "edge"))
        x[0, 4:8, 8:12] = aligned_token(*window_value_rows(layer, 0))       # one whole 4-window of equal tokens: its o_0 IS v_0 of the token
        x[1] = aligned_token(*window_value_rows(layer, 2))                   # a whole map of equal tokens: every o_b IS v_b of the token
        out.append(Case(f"static bound at {INSIDE} x 65504, n=2 16x16, a 4-window and a map of aligned tokens", "edge", x))
    else:
        raise KeyError(group)
    return out


def ffn_cases(C, M, group):
    """-> [Case]: x [tokens, C] or [n, H, W, C] float32."""
    out = []
    if group == "tokens":
        for T in (31, 32, 33, 64):
            out.append(Case(f"{T} tokens", "base", _randn(T, C, key=("ffn", C, M, "tokens", T))))
    elif group == "planted":
        x = plant(_randn(2, 5, 7, C, key=("ffn", C, M, "planted")), _gen("ffn", C, M, "plant"))
        out.append(Case("2x5x7 planted tokens", "base", x))
    elif group == "edge":                                             # z = +-|w yhat| + b: one of the two signs is the large positive pre-activation GELU passes on
        tok = aligned_token(*ffn_hidden_rows(ffn_layer(C, M, "edge")))
        x = _randn(33, C, key=("ffn", C, M, "edge"))
        x[0], x[1], x[31], x[32] = tok, -tok, -tok, tok
        out.append(Case(f"static bound at {INSIDE} x 65504, 33 tokens, the aligned token and its negative", "edge", x))
    else:
        raise KeyError(group)
    return out


# ---- one layer three ways: float64 restatement, float32 op by op (any device) ---------------------------------------------------------------------------------------
def agent_reference(layer, case):
    return agent_attention_f64(layer.state_dict(), case.x, case.theta, case.x.shape[-1] // 32)


def agent_warped_f64(case) -> torch.Tensor:
    """The maps the layer sees, float64 on the CPU: the restatement's warp (float32 sampling positions)."""
    if case.theta is None:
        return case.x.double()
    return warp_f64(case.x.permute(0, 3, 1, 2), case.theta).permute(0, 2, 3, 1)


def agent_op_by_op(layer, xw: torch.Tensor) -> torch.Tensor:
    """xw [n, H, W, C] (already warped) on the layer's device and in its dtype -> xw + attention, every receiver: the module's own forward."""
    with torch.no_grad():
        return layer(xw[None], mask=torch.ones(1, 1, 1, 1, xw.shape[0], device=xw.device))[0] + xw


def window_reference(layer, config, x):
    C, fuse = WINDOW_CONFIGS[config]
    return window_attention_f64(layer.state_dict(), x, WINDOWS, _window_heads(C), fuse)


def window_op_by_op(layer, x):
    with torch.no_grad():
        return layer(x[None])[0] + x


def ffn_reference(layer, x):
    return feed_forward_f64(layer.state_dict(), x)


def ffn_op_by_op(layer, x):
    with torch.no_grad():
        return layer(x) + x
