"""Float64 restatement of Lift-Splat's frustum pooling (test infrastructure): the cell of every frustum point and the pooled BEV map, in numpy, from the
reference's formulas -- ``get_geometry`` (opencood/models/lift_splat_shoot.py:80-102), ``voxel_pooling``'s index line and bounds test (:126, :133-135), the
softmax x feature product of ``CamEncode.forward`` (sub_modules/lss_submodule.py:134-136) and the channel order of ``torch.cat(final.unbind(dim=2), 1)``.
Plus the seeded cases the CPU and GPU tests share, computed once per process."""
import functools

import numpy as np
import torch

from coalign_amd.lss import LiftSplat
from coalign_amd.synthetic import make_camera_rig

CAMS = ("rots", "trans", "intrins", "post_rots", "post_trans")
GOLDEN_GRID = {"xbound": [-4.0, 4.8, 0.4], "ybound": [-3.2, 3.2, 0.4], "zbound": [-2, 4, 3.0], "ddiscr": [2, 12, 6], "mode": "LID"}
GOLDEN_AUG = {"final_dim": [48, 64]}
# (xbound, ybound, zbound, ddiscr) of the small grids the tests use beside the fixture's: 7 x 5 cells of 2 m (the step divides exactly), one cell that takes everything
GRID_7X5 = ((-7, 7, 2.0), (-5, 5, 2.0), (-10, 10, 20.0), (2, 12, 6))
GRID_7X5_D8 = GRID_7X5[:3] + ((2, 12, 8),)
GRID_ONE_CELL = ((-100, 100, 200), (-100, 100, 200), (-10, 10, 20.0), (2, 12, 8))


def grid_conf(x=(-4.0, 4.8, 0.4), y=(-3.2, 3.2, 0.4), z=(-2, 4, 3.0), ddiscr=(2, 12, 6)):
    return {"xbound": list(x), "ybound": list(y), "zbound": list(z), "ddiscr": list(ddiscr), "mode": "LID"}


def splat(grid=None, final_dim=(48, 64), downsample=8) -> LiftSplat:
    return LiftSplat(grid or grid_conf(), {"final_dim": list(final_dim)}, downsample)


def _inv3(a):
    """[..., 3, 3] float64 by the adjugate; a singular matrix gives inf / NaN (no exception)."""
    with np.errstate(all="ignore"):
        adj = np.empty_like(a)
        for i in range(3):
            for j in range(3):
                r = [k for k in range(3) if k != j]
                c = [k for k in range(3) if k != i]
                adj[..., i, j] = (-1.0) ** (i + j) * (a[..., r[0], c[0]] * a[..., r[1], c[1]] - a[..., r[0], c[1]] * a[..., r[1], c[0]])
        det = (a[..., 0, :] * adj[..., :, 0]).sum(-1)
        return adj / det[..., None, None]


def scaled_coordinates(rig, xs, ys, ds, lower, dx):
    """float64 v = (g - lower) / dx of every frustum point, [M, D, fH, fW, 3], from the float32 inputs."""
    f = {k: np.asarray(rig[k], dtype=np.float32).astype(np.float64) for k in CAMS}
    M = f["trans"].reshape(-1, 3).shape[0]
    R, K, PR = (f[k].reshape(M, 3, 3) for k in ("rots", "intrins", "post_rots"))
    T, PT = f["trans"].reshape(M, 3), f["post_trans"].reshape(M, 3)
    xs, ys, ds = (np.asarray(v, dtype=np.float32).astype(np.float64) for v in (xs, ys, ds))
    D, fH, fW = len(ds), len(ys), len(xs)
    fr = np.stack(np.broadcast_arrays(xs[None, None, :], ys[None, :, None], ds[:, None, None]), -1)      # [D, fH, fW, 3]
    with np.errstate(all="ignore"):
        p = fr[None] - PT[:, None, None, None, :]
        p = np.einsum("mij,mdhwj->mdhwi", _inv3(PR), p)
        p = np.concatenate([p[..., :2] * p[..., 2:3], p[..., 2:3]], -1)
        g = np.einsum("mij,mdhwj->mdhwi", np.einsum("mij,mjk->mik", R, _inv3(K)), p) + T[:, None, None, None, :]
        return (g - np.asarray(lower, dtype=np.float32).astype(np.float64)) / np.asarray(dx, dtype=np.float32).astype(np.float64)


def cells_f64(v, n):
    """v [M, D, fH, fW, 3] -> int32 cell (z ny + y) nx + x or -1: truncation TOWARDS ZERO, the bounds test, non-finite or >= 2^31 dropped."""
    nx, ny, nz = (int(k) for k in n)
    with np.errstate(all="ignore"):
        ok = np.abs(v) < 2.0 ** 31
        i = np.trunc(np.where(ok, v, -1.0)).astype(np.int64)
    kept = ok.all(-1) & (i[..., 0] >= 0) & (i[..., 0] < nx) & (i[..., 1] >= 0) & (i[..., 1] < ny) & (i[..., 2] >= 0) & (i[..., 2] < nz)
    return np.where(kept, (i[..., 2] * ny + i[..., 1]) * nx + i[..., 0], -1).astype(np.int32)


def distance_to_integer(v):
    """min over the points with finite coordinates of |v - round(v)|."""
    w = v[np.isfinite(v)]
    return float(np.abs(w - np.round(w)).min()) if w.size else 1.0


def near_boundary(v, band=1e-3):
    """[M, D, fH, fW] bool: a coordinate within ``band`` of an integer (where float32 and float64 geometry may disagree on the cell)."""
    with np.errstate(all="ignore"):
        return (np.abs(v - np.round(v)) <= band).any(-1) | ~np.isfinite(v).all(-1)


def pool_f64(depth_logit, x_img, cell, A, n):
    """The pooled map in float64: out[a, z C + c, y, x] = sum over the points of the cell of softmax_d(logit) * x_img.  depth_logit [M, D, fH, fW],
    x_img [M, C, fH, fW], cell [M, D, fH, fW] -> float64 [A, nz C, ny, nx]."""
    nx, ny, nz = (int(k) for k in n)
    lg = np.asarray(depth_logit, dtype=np.float64)
    x = np.asarray(x_img, dtype=np.float64)
    M, D, fH, fW = lg.shape
    C = x.shape[1]
    e = np.exp(lg - lg.max(1, keepdims=True))
    prob = e / e.sum(1, keepdims=True)
    vol = prob[:, :, :, :, None] * x.transpose(0, 2, 3, 1)[:, None]                 # [M, D, fH, fW, C]
    cell = np.asarray(cell).reshape(M, D, fH, fW).astype(np.int64)
    agent = np.broadcast_to((np.arange(M) // (M // A))[:, None, None, None], cell.shape)
    kept = cell >= 0
    out = np.zeros((A * nz * ny * nx, C))
    np.add.at(out, (agent[kept] * (nz * ny * nx) + cell[kept]), vol[kept])
    return torch.from_numpy(out.reshape(A, nz, ny, nx, C).transpose(0, 1, 4, 2, 3).reshape(A, nz * C, ny, nx).copy())


def rig_tensors(rig, device=None):
    return [rig[k] if device is None else rig[k].to(device) for k in CAMS]


@functools.lru_cache(maxsize=None)
def case(A, N, seed, grid_key=None, final_dim=(48, 64)):
    """A seeded rig on a grid, with everything the tests compare against, computed once: (splat module, rig, v, cells).  ``grid_key``: a tuple
    (xbound, ybound, zbound, ddiscr) of tuples, None for the golden fixture's grid."""
    sp = splat(grid_conf(*grid_key) if grid_key else None, final_dim)
    rig = make_camera_rig(A, N, final_dim, seed=seed)
    v = scaled_coordinates(rig, *sp.axes, sp.lower, sp.cell_size)
    return sp, rig, v, cells_f64(v, sp.nx)


def features(M, C, D, fH, fW, seed, logit_scale=3.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(M, D, fH, fW, generator=g) * logit_scale, torch.randn(M, C, fH, fW, generator=g)


def skewed_cells(M=4, D=8, fH=6, fW=8, nx=7, ny=5, nz=1, long=700, seed=3):
    """Hand-made cells of one agent (int32 [M, D, fH, fW]): cell (3, 2) of the 7 x 5 grid holds ``long`` points (more than one chunk), each of its eight
    neighbours 1 .. 5, everything else is dropped -- the skew the chunk rule exists for, at the smallest size."""
    rs = np.random.RandomState(seed)
    cell = np.full(M * D * fH * fW, -1, np.int32)
    free = rs.permutation(cell.size)
    centre = 2 * nx + 3
    cell[free[:long]] = centre
    at = long
    for k, (dy, dx) in enumerate((dy, dx) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (dy, dx) != (0, 0)):
        n = 1 + k % 5
        cell[free[at:at + n]] = centre + dy * nx + dx
        at += n
    return cell.reshape(M, D, fH, fW)
