"""Helpers shared by the SplitMap GPU tests (tests/test_round5_gpu.py, tests/test_s2_gpu.py, tests/test_sp_limits_gpu.py)."""
import torch

from coalign_amd import ops

DEV = "cuda:0"


def round22(x):
    return ((x.contiguous().view(torch.int32) + 2) & -4).view(torch.float32)


def assert_split_map_holds(sm, want, what=""):
    """A SplitMap holds `want` rounded to 22 significant bits: exactly for |value| >= 2^-13, to an absolute 2^-33 below (csrc/common.h)."""
    got, w22 = sm.dense(), round22(want)
    big = want.abs() >= 2.0 ** -13
    assert torch.equal(got[big], w22[big]), what
    if bool((~big).any()):
        assert float((got[~big] - want[~big]).abs().max()) <= 2.0 ** -33, what


def sparse_canvas(n_agents, ny, nx, pillars, seed, count_below_capacity=False):
    """A SparseCanvas from the one-launch pillar op on random pillars (duplicate cells included: the larger row wins)."""
    from coalign_amd.config import builtin_config
    from coalign_amd.detector import build_model
    from coalign_amd.synthetic import fill_parameters_, make_frame
    h = builtin_config("opv2v_coalign")
    model = build_model(h)
    fill_parameters_(model, seed=seed)
    model = model.to(DEV).eval()
    margs = h["model"]["args"]
    pl = make_frame(h, n_agents, pillars_per_agent=pillars, seed=seed)["processed_lidar"]
    pfn = model.pillar_vfe.pfn_layers[0]
    bn = (pfn.norm.weight, pfn.norm.bias, pfn.norm.running_mean, pfn.norm.running_var)
    gx, gy, _ = [int(v) for v in margs["point_pillar_scatter"]["grid_size"]]
    assert (gy, gx) == (ny, nx)
    count_dev = None
    vf, npts, coords = pl["voxel_features"].to(DEV), pl["voxel_num_points"].to(DEV), pl["voxel_coords"].to(DEV)
    if count_below_capacity:
        count_dev = torch.tensor([vf.shape[0] - 1234], dtype=torch.int32, device=DEV)
    return ops.pillar_encode_sparse(vf, npts, coords, pfn.linear.weight, None, bn, 1e-3, True, margs["voxel_size"], margs["lidar_range"][:3], n_agents, ny, nx, canvas_cache={},
                                    count_dev=count_dev)
