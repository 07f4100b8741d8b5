"""A float64 restatement of one ``PreNorm(FeedForward)`` layer of V2X-ViT with its residual, from the UNFOLDED parameters (base_transformer.py:7-29 and the residual
of v2xvit_basic.py:179): the yardstick of tests/test_v2x_ffn_cpu.py and tests/test_v2x_ffn_gpu.py.  ``act`` swaps the activation, for the examination that the
yardstick sees it."""
import math

import torch


def _activation(z: torch.Tensor, act: str) -> torch.Tensor:
    if act == "gelu":                                    # the exact one: 0.5 z (1 + erf(z / sqrt 2))
        return 0.5 * z * (1.0 + torch.erf(z / math.sqrt(2.0)))
    if act == "gelu_tanh":
        return 0.5 * z * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (z + 0.044715 * z ** 3)))
    if act == "relu":
        return z.clamp(min=0.0)
    raise ValueError(act)


def feed_forward_f64(state: dict, x: torch.Tensor, act: str = "gelu", probe: dict = None) -> torch.Tensor:
    """state: the ``state_dict`` of ``PreNorm(dim, FeedForward)``; x [..., C] on any device -> x + net(LayerNorm(x)) in float64 on x's device."""
    sd = {k: v.detach().to(device=x.device, dtype=torch.float64) for k, v in state.items()}
    x = x.detach().double()
    mean = x.mean(dim=-1, keepdim=True)
    var = ((x - mean) ** 2).mean(dim=-1, keepdim=True)
    y = (x - mean) / torch.sqrt(var + 1e-5) * sd["norm.weight"] + sd["norm.bias"]
    z = y @ sd["fn.net.0.weight"].t() + sd["fn.net.0.bias"]
    if probe is not None:
        probe["z"] = z
    return x + _activation(z, act) @ sd["fn.net.3.weight"].t() + sd["fn.net.3.bias"]
