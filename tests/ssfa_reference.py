"""Float64 restatements of the SSFA neck (opencood/models/sub_modules/cia_ssd_utils.py:6-55) for tests/test_ssfa_cpu.py and tests/test_ssfa_gpu.py: the
transposed convolution from its scatter definition (no ``F.conv_transpose2d``: that is the thing under test on the torch route), the two-way softmax blend, the
whole module, and the closed formula that fills a module's parameters for the golden fixture (tests/golden/make_ssfa_golden.py imports it from here)."""
import math

import torch
import torch.nn as nn


def deconv_f64(x, w, b=None):
    """ConvTranspose2d(3, stride 2, padding 1, output_padding 1) in float64, tap by tap: out[co, 2y - 1 + ky, 2x - 1 + kx] += x[ci, y, x] w[ci, co, ky, kx].
    x [N, Ci, h, w], w [Ci, Co, 3, 3], b [Co] or None -> [N, Co, 2h, 2w]."""
    N, Ci, h, wd = x.shape
    xd, wt = x.double(), w.double()
    out = torch.zeros((N, w.shape[1], 2 * h, 2 * wd), dtype=torch.float64, device=x.device)
    for ky in range(3):
        for kx in range(3):
            y0, x0 = (1 if ky == 0 else 0), (1 if kx == 0 else 0)          # the first input row / column whose target lies inside the map
            t = torch.einsum("io,nihw->nohw", wt[:, :, ky, kx], xd[:, :, y0:, x0:])
            ys, xs = 2 * y0 - 1 + ky, 2 * x0 - 1 + kx
            out[:, :, ys:ys + 2 * (h - y0):2, xs:xs + 2 * (wd - x0):2] += t
    return out if b is None else out + b.double().view(1, -1, 1, 1)


def blend_f64(a, b, wa, wb, ba, bb):
    """The softmax blend of cia_ssd_utils.py:50-53 in float64 -> (y, p)."""
    ad, bd = a.double(), b.double()
    la = torch.einsum("c,nchw->nhw", wa.double().reshape(-1), ad) + float(ba)
    lb = torch.einsum("c,nchw->nhw", wb.double().reshape(-1), bd) + float(bb)
    p = torch.sigmoid(la - lb).unsqueeze(1)
    return ad * p + bd * (1.0 - p), p


def _bn(seq, i):
    bn = seq[i]
    s = bn.weight.double() / torch.sqrt(bn.running_var.double() + bn.eps)
    return s, bn.bias.double() - bn.running_mean.double() * s


def _conv_f64(x, conv, bn_s, bn_b, relu=True):
    k, s = conv.kernel_size[0], conv.stride[0]
    p = conv.padding[0]
    xp = torch.nn.functional.pad(x, (p, p, p, p))
    N, _, H, W = xp.shape
    Ho, Wo = (H - k) // s + 1, (W - k) // s + 1
    out = torch.zeros((N, conv.out_channels, Ho, Wo), dtype=torch.float64, device=x.device)
    wt = conv.weight.double()
    for ky in range(k):
        for kx in range(k):
            out += torch.einsum("oc,nchw->nohw", wt[:, :, ky, kx], xp[:, :, ky:ky + s * (Ho - 1) + 1:s, kx:kx + s * (Wo - 1) + 1:s])
    out = out * bn_s.view(1, -1, 1, 1) + bn_b.view(1, -1, 1, 1)
    return torch.relu(out) if relu else out


def ssfa_f64(m, x):
    """``second.SSFA.forward`` of the eval-mode module ``m`` in float64, every convolution tap by tap, BatchNorm from its running statistics."""
    x = x.double()
    with torch.no_grad():
        def seq(block, y, first=0, relu_last=True):
            mods = list(block)
            i = first
            while i < len(mods):
                conv = mods[i]
                relu = i + 2 < len(mods) and isinstance(mods[i + 2], nn.ReLU)
                s, b = _bn(mods, i + 1)
                if isinstance(conv, nn.ConvTranspose2d):
                    y = deconv_f64(y, conv.weight) * s.view(1, -1, 1, 1) + b.view(1, -1, 1, 1)
                    y = torch.relu(y) if relu else y
                else:
                    y = _conv_f64(y, conv, s, b, relu)
                i += 3 if relu else 2
            return y
        x0 = seq(m.bottom_up_block_0, torch.nn.functional.pad(x, (1, 1, 1, 1)), first=1)
        x1 = seq(m.bottom_up_block_1, x0)
        t0, t1 = seq(m.trans_0, x0), seq(m.trans_1, x1)
        m0 = seq(m.deconv_block_0, t1) + t0
        m1 = seq(m.deconv_block_1, t1)
        o0, o1 = seq(m.conv_0, m0), seq(m.conv_1, m1)
        la, lb = seq(m.w_0, o0), seq(m.w_1, o1)
        p = torch.sigmoid(la - lb)
        return o0 * p + o1 * (1.0 - p)


# ---- the closed formula of the golden fixture ----------------------------------------------------------------------------------------------------------------
def _name_phase(name: str) -> float:
    return (sum((i + 1) * ord(c) for i, c in enumerate(name)) % 997) / 997.0


def formula_values(name: str, shape, dtype=torch.float64) -> torch.Tensor:
    """The values of the parameter or buffer ``name``: a function of the name and the flat index alone (no RNG).  Weights are sized so that activations keep their
    scale through the module (a sine of an irrational multiple of the index, divided by sqrt(fan-in)); BatchNorm scales lie in [0.75, 1.25], shifts and running
    means in [-0.1, 0.1], running variances in [0.5, 1.5] (positive); ``num_batches_tracked`` is 0."""
    n = 1
    for s in shape:
        n *= int(s)
    if name.endswith("num_batches_tracked"):
        return torch.zeros(tuple(shape), dtype=torch.int64)
    i = torch.arange(n, dtype=torch.float64)
    wave = torch.sin(i * (math.sqrt(2.0) + _name_phase(name)) + 7.0 * _name_phase(name))
    if name.endswith("running_var"):
        v = 1.0 + 0.5 * wave
    elif name.endswith("running_mean") or name.endswith(".bias"):
        v = 0.1 * wave
    elif len(shape) == 1:                                         # BatchNorm weight
        v = 1.0 + 0.25 * wave
    else:                                                         # convolution weight [a, b, k, k]: fan-in = the other channel count x taps (an upper estimate for the transposed layers)
        fan = max(int(shape[0]), int(shape[1])) * int(shape[2]) * int(shape[3])
        v = wave * math.sqrt(3.0 / fan)
    return v.reshape(tuple(shape)).to(dtype)


def fill_by_formula_(module: nn.Module) -> nn.Module:
    with torch.no_grad():
        for name, t in module.state_dict().items():
            t.copy_(formula_values(name, t.shape).to(t.dtype))
    return module


def formula_input(shape=(1, 128, 4, 6)) -> torch.Tensor:
    n = 1
    for s in shape:
        n *= s
    i = torch.arange(n, dtype=torch.float64)
    return (torch.sin(i * math.sqrt(3.0)) + 0.25 * torch.cos(i * 0.0137)).reshape(shape)
