"""Float64 restatement of Where2comm (opencood/models/fuse_modules/where2comm_attn.py:174-341, opencood/models/comm_modules/where2comm.py:9-78) for the tests, and
the inputs of the mask tests.

A mask is a threshold of a continuous value, so it can be compared bit for bit only where no value lies near the threshold.  Every mask test therefore takes its
logits and its threshold from ``mask_case`` / ``check_mask_inputs``, which ASSERT in float64 that (a) every agent's mask has between 20 % and 80 % ones before the
even-agent override and (b) no pixel's smoothed confidence lies within ``MARGIN`` = 2e-5 of the threshold: more than ten times the fp32 error of a 25-tap sum of
values <= 1 (25 x 2^-24 = 1.5e-6)."""
import numpy as np
import torch
import torch.nn.functional as F

MARGIN = 2e-5


def gaussian_weight(k, sigma=1.0):
    """Communication.init_gaussian_filter (where2comm.py:24-32) -> float32 [k, k] (the reference stores float32)."""
    c = k // 2
    x, y = np.mgrid[0 - c: k - c, 0 - c: k - c]
    return torch.Tensor(1 / (2 * np.pi * sigma) * np.exp(-(np.square(x) + np.square(y)) / (2 * np.square(sigma))))


def smoothed_f64(psm, weight=None, bias=None):
    """where2comm.py:52-57 in float64: [n, A, H, W] logits -> [n, H, W]."""
    conf = psm.double().sigmoid().max(dim=1)[0].unsqueeze(1)
    if weight is not None:
        k = weight.shape[-1]
        conf = F.conv2d(conf, weight.double().reshape(1, 1, k, k), None if bias is None else bias.double().reshape(1), padding=(k - 1) // 2)
    return conf[:, 0]


def check_mask_inputs(psm, weight, bias, thre):
    """The two conditions of every mask test, in float64 -> (smoothed, the masks before the override, as bool)."""
    s = smoothed_f64(psm, weight, bias)
    thre32 = float(np.float32(thre))          # the comparison runs against the float32 value of the threshold
    margin = float((s - thre32).abs().min())
    assert margin >= MARGIN, f"a smoothed confidence lies within {margin:.2e} of the threshold: the mask is not decided in fp32"
    on = s > thre32
    frac = on.flatten(1).double().mean(dim=1)
    assert bool((frac >= 0.2).all()) and bool((frac <= 0.8).all()), f"masks not mixed: fractions of ones {frac.tolist()}"
    return s, on


def mask_case(n_total, A, H, W, k, bias=0.0, seed=50):
    """Logits ``2 randn - 2`` and a threshold in the widest gap of the smoothed confidences' middle fifth -> (psm, weight or None, bias or None, thre), at the first
    seed from ``seed`` on at which the two conditions hold (asserted).  The threshold is an input like any other; it is chosen so that both hold at every shape,
    anchor count and kernel size."""
    weight = gaussian_weight(k) if k > 0 else None
    b = torch.tensor([bias], dtype=torch.float32) if k > 0 else None
    for s in range(seed, seed + 64):
        psm = 2 * torch.randn(n_total, A, H, W, generator=torch.Generator().manual_seed(s)) - 2
        v = smoothed_f64(psm, weight, b).flatten().sort()[0]
        lo, hi = int(0.4 * v.numel()), max(int(0.6 * v.numel()), int(0.4 * v.numel()) + 2)
        gaps = v[lo + 1:hi] - v[lo:hi - 1]
        i = int(gaps.argmax())
        thre = float(np.float32(0.5 * float(v[lo + i] + v[lo + i + 1])))
        try:
            check_mask_inputs(psm, weight, b, thre)
        except AssertionError:
            continue
        return psm, weight, b, thre
    raise AssertionError(f"no seed in {seed}..{seed + 63} gives mixed, decided masks at {(n_total, A, H, W, k)}")


def masks_f64(psm, groups, weight, bias, thre, levels=1):
    """-> (masks per level, uint8 [n, H >> l, W >> l], after the even-agent override; rates float32 [B], count / (H W) as the reference's fp32 division gives it)."""
    s = smoothed_f64(psm, weight, bias)
    on = s > float(np.float32(thre))
    H, W = on.shape[1:]
    rates, off = [], 0
    out = on.clone()
    for n in groups:
        rates.append(torch.tensor(float(on[off].sum()), dtype=torch.float32) / (H * W))          # where2comm.py:63 (an integer count is exact in fp32)
        out[off:off + n:2] = True                                                                   # where2comm.py:71
        off += n
    masks = [out.to(torch.uint8)]
    for _ in range(1, levels):
        masks.append(F.max_pool2d(masks[-1].double().unsqueeze(1), kernel_size=2)[:, 0].to(torch.uint8))      # where2comm_attn.py:274
    return masks, torch.stack(rates)


def single_scale_masks(mask, groups):
    """where2comm_attn.py:334 indexes the masks of ALL agents (where2comm.py:77) by the FRAME: frame b's agents are all masked by the batch's agent number b."""
    return torch.cat([mask[b:b + 1].expand(n, *mask.shape[1:]) for b, n in enumerate(groups)], dim=0)


def rate_of(rates):
    """sum(communication_rates) / B in the reference's order (where2comm.py:76), fp32."""
    return sum(rates.unbind(0)) / rates.numel()


def warp_f64(x, theta):
    """warp_affine_simple with the grid cast to float32 like the reference's ``.to(src)`` on an fp32 map, sampled in float64."""
    grid = F.affine_grid(theta.double(), list(x.shape), align_corners=False).float().double()
    return F.grid_sample(x.double(), grid, align_corners=False)


def fuse_f64(x, theta, mode, dim=None):
    """AttenFusion / MaxFusion (where2comm_attn.py:44-61) of ONE frame's warped maps in float64 -> [C, H, W]."""
    v = warp_f64(x, theta)
    if mode == "MAX":
        return v.max(dim=0)[0]
    n, C, H, W = v.shape
    q = v.reshape(n, C, -1).permute(2, 0, 1)
    score = torch.bmm(q, q.transpose(1, 2)) / np.sqrt(C if dim is None else dim)
    return torch.bmm(F.softmax(score, -1), q).permute(1, 2, 0).reshape(n, C, H, W)[0]


def where2comm_levels_f64(xs, masks, groups, affine, mode):
    """Per level: fuse(warp(x * mask)) of every frame in float64 -> list of [B, C_l, H_l, W_l].  ``masks``: per level uint8 [n, H_l, W_l], or None."""
    out = []
    for l, x in enumerate(xs):
        xm = x.double() if masks is None else x.double() * masks[l].double().unsqueeze(1)
        frames, off = [], 0
        for b, n in enumerate(groups):
            frames.append(fuse_f64(xm[off:off + n], affine[b, 0, :n], mode))
            off += n
        out.append(torch.stack(frames))
    return out
