"""The shared cases of tests/test_v2v_robust_cpu.py and tests/test_v2v_robust_gpu.py: a ``PointPillarV2VNetRobust`` at C = hidden = 64 on a map of the wanted
size with ``synthetic.v2v_robust_parameters_``, maps, noisy poses, and the float64 yardstick's result for them -- each computed once per process and never modified.

Poses: the ego at the origin, the others within +-4 m and +-15 degrees, every agent with strong position noise (0.4 m).  The map covers 0.8 m per cell, so the
warps shift by a few cells: masks with fractions, zeros and ones."""
import functools

import torch

from coalign_amd.config import builtin_config
from coalign_amd.detector import build_model
from coalign_amd.synthetic import fill_parameters_, v2v_robust_parameters_
from v2v_robust_reference import robust_frame_f64

SIZES = ((24, 24), (25, 41))          # the minimum; floor cropping at every pooling and no multiple of any tile
AGENTS = (1, 2, 3, 5, 8)
MAX_CAV = 8
SEED = 2                              # of the weights, the maps and the poses: chosen so that the yardstick satisfies every non-degeneracy guard in all cases


def hypes_for(H: int, W: int, stage: int = 2) -> dict:
    h = builtin_config("mini_pointpillar_v2vnet_robust")
    a = h["model"]["args"]
    a["robust"].update(H=H, W=W)
    a["v2vfusion"]["conv_gru"].update(H=H, W=W)
    a["stage"], a["max_cav"] = stage, MAX_CAV
    return h


def model_for(H: int, W: int, stage: int = 2, seed: int = SEED):
    """-> (model in eval mode on the CPU, its args, a copy of its state_dict)."""
    h = hypes_for(H, W, stage)
    m = build_model(h)
    fill_parameters_(m, seed=seed)
    v2v_robust_parameters_(m, seed=seed)
    return m.eval(), h["model"]["args"], {k: v.clone() for k, v in m.state_dict().items()}


def poses_for(n: int, seed: int) -> torch.Tensor:
    """[n, 3] float32 noisy poses (x, y, yaw in degrees)."""
    g = torch.Generator().manual_seed(seed)
    p = torch.zeros(n, 3)
    p[1:, :2] = (torch.rand(n - 1, 2, generator=g) - 0.5) * 8.0
    p[1:, 2] = (torch.rand(n - 1, generator=g) - 0.5) * 30
    p[:, :2] += torch.randn(n, 2, generator=g) * 0.4
    return p


def maps_for(n: int, H: int, W: int, seed: int = SEED) -> torch.Tensor:
    return torch.randn(n, 64, H, W, generator=torch.Generator().manual_seed(1000 * seed + n))


@functools.lru_cache(maxsize=None)
def case(H: int, W: int, n: int, stage: int = 2, seed: int = SEED):
    """-> (args, state_dict, x [n, 64, H, W], poses [n, 3], yardstick dict, trace) of one frame."""
    _, args, state = model_for(H, W, stage, seed)
    x, poses = maps_for(n, H, W, seed), poses_for(n, n + seed)
    trace = {}
    ref = robust_frame_f64(state, args, x, poses, stage, trace=trace)
    return args, state, x, poses, ref, trace


QUANTITIES = ("pairwise_corr", "lidar_pose_corrected", "scores", "weight", "cls_preds", "reg_preds")


def errors(got: dict, ref: dict, n: int, frame: int = 0) -> dict:
    """max |got - ref| per quantity of one frame (maps: relative to the yardstick's largest magnitude)."""
    out = {}
    for k in QUANTITIES:
        if k not in got or k not in ref:
            continue
        r = ref[k]
        g = got[k].detach().cpu().double()
        if k in ("scores", "weight"):
            g = g[frame, :r.shape[0], :r.shape[1]]
        elif k == "pairwise_corr":
            g = g[frame, :n, :n]
        elif k in ("cls_preds", "reg_preds"):
            g = g[frame]
        e = float((g - r).abs().max())
        out[k] = e / float(r.abs().max()) if k in ("cls_preds", "reg_preds") else e
    return out
