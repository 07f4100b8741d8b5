"""The yardstick of the pillar-encoder limit tests: ``PillarVFE`` (opencood/models/sub_modules/pillar_vfe.py:31-53,105-155) evaluated on the CPU from the float32
inputs, in float64 (``pfn_f64``) or, operation by operation in the reference's order, in float32 (``pfn_f32``: the reference's own arithmetic for the flag sets
``oracle.pillar_vfe`` does not cover; tests/test_pillar_limits_cpu.py pins it to goldens recorded from the reference itself).

Any P and C, ``use_absolute_xyz`` on or off, ``with_distance`` on or off, eval BatchNorm (``norm.*`` in the state dict) or a Linear bias (``linear.bias``).
What both precisions share with the reference and with every kernel:
  * the cell centre is FORMED IN FLOAT32, coord * voxel + (voxel / 2 + range_min) with the offset rounded to float32 once (pillar_vfe.py:84-89,123-132), and
    only then widened: the centre is an input of the arithmetic, not part of its rounding error;
  * the mean divides the sum over ALL P slots by ``voxel_num_points`` (:118-120);
  * the distance is taken of the raw point, the padding mask is applied afterwards (:139-149);
  * padded rows (slot >= num_points) stay in the max: they contribute relu(BN(0)) or relu(bias) (:46).
Pillars are evaluated in chunks of at most 8192, so the [M, P, C] intermediate stays below ~130 MB at P = 32, C = 64.
"""
import torch

PREFIX = "pillar_vfe.pfn_layers.0."
CHUNK = 8192
BN_EPS = 1e-3                     # pillar_vfe.py:25


def cell_centres(coords, voxel_size, lidar_range):
    """[M, 3] float32 (x, y, z) centres as the reference forms them: float32 coordinate times the float32 voxel size plus the float32 offset."""
    f32 = lambda v: torch.tensor(float(v), dtype=torch.float32)
    vs, r = voxel_size, lidar_range
    cd = coords
    return torch.stack([cd[:, 3].float() * f32(vs[0]) + f32(vs[0] / 2 + r[0]), cd[:, 2].float() * f32(vs[1]) + f32(vs[1] / 2 + r[1]),
                        cd[:, 1].float() * f32(vs[2]) + f32(vs[2] / 2 + r[2])], 1)


def _pfn(vf, npts, coords, sd, voxel_size, lidar_range, use_absolute_xyz, with_distance, dtype, prefix):
    w = sd[prefix + "linear.weight"].to(dtype)
    use_norm = prefix + "norm.weight" in sd
    cin = (4 if use_absolute_xyz else 1) + 6 + (1 if with_distance else 0)
    assert vf.dtype == torch.float32 and vf.dim() == 3 and vf.shape[2] == 4 and w.shape[1] == cin, (tuple(vf.shape), tuple(w.shape), cin)
    M, P = vf.shape[0], vf.shape[1]
    ctr_all = cell_centres(coords, voxel_size, lidar_range)
    slots = torch.arange(P, dtype=torch.int32)[None, :]
    out = torch.empty((M, w.shape[0]), dtype=dtype)
    for m0 in range(0, M, CHUNK):
        v = vf[m0:m0 + CHUNK].to(dtype)
        n = npts[m0:m0 + CHUNK]
        xyz = v[:, :, :3]
        mean = xyz.sum(dim=1, keepdim=True) / n.to(dtype).view(-1, 1, 1)
        feats = [v if use_absolute_xyz else v[:, :, 3:], xyz - mean, xyz - ctr_all[m0:m0 + CHUNK].to(dtype)[:, None, :]]
        if with_distance:
            feats.append(torch.norm(xyz, 2, 2, keepdim=True))
        f = torch.cat(feats, dim=-1)
        f = f * (n.int().view(-1, 1) > slots).to(dtype)[..., None]
        x = f @ w.t()
        if use_norm:
            x = (x - sd[prefix + "norm.running_mean"].to(dtype)) / torch.sqrt(sd[prefix + "norm.running_var"].to(dtype) + BN_EPS) * sd[prefix + "norm.weight"].to(dtype) \
                + sd[prefix + "norm.bias"].to(dtype)
        elif prefix + "linear.bias" in sd:
            x = x + sd[prefix + "linear.bias"].to(dtype)
        out[m0:m0 + CHUNK] = torch.relu(x).max(dim=1).values
    return out


def pfn_f64(voxel_features, voxel_num_points, voxel_coords, sd, voxel_size, lidar_range, use_absolute_xyz=True, with_distance=False, prefix=PREFIX):
    """-> [M, C] float64: the exact value of the reference's formula on these float32 inputs (up to float64 rounding, 1e-16 of the scale)."""
    return _pfn(voxel_features, voxel_num_points, voxel_coords, sd, voxel_size, lidar_range, use_absolute_xyz, with_distance, torch.float64, prefix)


def pfn_f32(voxel_features, voxel_num_points, voxel_coords, sd, voxel_size, lidar_range, use_absolute_xyz=True, with_distance=False, prefix=PREFIX):
    """-> [M, C] float32: the same operations in the reference's order in float32 -- what the reference itself computes on a CPU."""
    return _pfn(voxel_features, voxel_num_points, voxel_coords, sd, voxel_size, lidar_range, use_absolute_xyz, with_distance, torch.float32, prefix)
