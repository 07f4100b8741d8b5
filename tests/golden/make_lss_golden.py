#!/usr/bin/env python
"""Generate tests/golden/lss_pool.npz by IMPORTING THE REFERENCE ITSELF (build container only: needs /root/reference; the ``.npz`` travels, this script's
import does not).  Usage:  python tests/golden/make_lss_golden.py

What is pinned: the reference's ``LiftSplatShoot.create_frustum``, ``.get_geometry`` and ``.voxel_pooling`` (opencood/models/lift_splat_shoot.py:65-169), called
UNBOUND on a stand-in object that carries the attributes they read (the class's constructor moves tensors to CUDA and builds the EfficientNet trunk, so it is
not constructed), with ``gen_dx_bx`` / ``depth_discretization`` of opencood/utils/camera_utils.py.  The case: grid x [-4.0, 4.8, 0.4], y [-3.2, 3.2, 0.4],
z [-2, 4, 3.0] (22 x 16 x 2 cells), depth bins [2, 12, 6] LID, a 48 x 64 image at downsample 8 (a 6 x 8 feature map), 2 agents x 3 cameras (1 728 frustum points),
C = 8, the rig of ``coalign_amd.synthetic.make_camera_rig`` with seed 5.  Stored: the camera tensors, the frustum's axes, the reference's float32 geometry, its
cell indices and kept mask, the logits and features, the ``voxel_pooling`` output.  Only data goes into the fixture.

The generator ASSERTS what makes the fixture worth having (float64 scaled coordinates v of tests/lss_reference.py): at least 10 kept points with a coordinate in
(-1, 0) (the fold of ``.long()``), at least 10 % of the points dropped, a cell fed by two cameras, at most 1 % of the points within 1e-3 of a cell boundary, none
within 1e-6.

Third-party modules the reference imports at module scope but that are absent here are replaced by inert stubs; torchvision's stub carries a real ``Normalize``
class (camera_utils.py subclasses it) and callables for ``Compose`` / ``ToTensor`` / ``ToPILImage``; the fusion names lss_submodule.py imports and this snapshot of
fusion_in_one.py lacks are set to None on the imported module.  No reference file is touched.
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, HERE)

from make_disco_golden import _Inert, import_reference  # noqa: E402  (puts the repository and the reference on sys.path)


def stub_torchvision():
    if "torchvision" in sys.modules and not isinstance(sys.modules["torchvision"], _Inert):
        return
    tv, tr = _Inert("torchvision"), _Inert("torchvision.transforms")

    class Normalize:
        def __init__(self, mean, std, inplace=False):
            self.mean, self.std = mean, std

        def __call__(self, tensor):
            return tensor

    tr.Normalize = Normalize
    tr.Compose = tr.ToTensor = tr.ToPILImage = lambda *a, **k: None
    tv.transforms = tr
    sys.modules["torchvision"], sys.modules["torchvision.transforms"] = tv, tr


def reference_classes():
    stub_torchvision()
    fio = import_reference("opencood.models.fuse_modules.fusion_in_one")
    for name in ("MaxFusion", "AttFusion", "V2VNetFusion", "V2XViTFusion", "When2commFusion", "Where2commFusion", "DiscoFusion"):
        if not hasattr(fio, name):
            setattr(fio, name, None)
    cu = import_reference("opencood.utils.camera_utils")
    lss = import_reference("opencood.models.lift_splat_shoot")
    return cu, lss.LiftSplatShoot


def main():
    import lss_reference as R
    from coalign_amd.synthetic import make_camera_rig
    cu, LSS = reference_classes()
    grid, aug, down = R.GOLDEN_GRID, R.GOLDEN_AUG, 8
    dx, bx, nx = cu.gen_dx_bx(grid["xbound"], grid["ybound"], grid["zbound"])
    ns = types.SimpleNamespace(grid_conf=grid, data_aug_conf=aug, downsample=down, dx=dx, bx=bx, nx=nx, use_quickcumsum=True)
    ns.frustum = LSS.create_frustum(ns)
    D, fH, fW, _ = ns.frustum.shape
    A, N, C = 2, 3, 8
    rig = make_camera_rig(A, N, aug["final_dim"], seed=5)
    cams = [rig[k] for k in R.CAMS]
    g = torch.Generator().manual_seed(5)
    logit = torch.randn(A * N, D, fH, fW, generator=g) * 3.0
    feat = torch.randn(A * N, C, fH, fW, generator=g)
    with torch.no_grad():
        geom = LSS.get_geometry(ns, *cams)
        idx = ((geom - (bx - dx / 2.)) / dx).long().view(-1, 3)                                   # voxel_pooling's own line, for the fixture's cells
        kept = (idx[:, 0] >= 0) & (idx[:, 0] < nx[0]) & (idx[:, 1] >= 0) & (idx[:, 1] < nx[1]) & (idx[:, 2] >= 0) & (idx[:, 2] < nx[2])
        vol = torch.softmax(logit, 1).unsqueeze(1) * feat.unsqueeze(2)                             # CamEncode.forward, lss_submodule.py:134-136
        vol = vol.view(A, N, C, D, fH, fW).permute(0, 1, 3, 4, 5, 2)                               # get_cam_feats, lift_splat_shoot.py:111-112
        out = LSS.voxel_pooling(ns, geom, vol)
    nxi = [int(v) for v in nx]
    assert nxi == [22, 16, 2] and tuple(out.shape) == (A, C * 2, 16, 22), (nxi, out.shape)
    cell = torch.where(kept, (idx[:, 2] * nxi[1] + idx[:, 1]) * nxi[0] + idx[:, 0], torch.full_like(idx[:, 0], -1)).to(torch.int32)

    xs, ys, ds = ns.frustum[0, 0, :, 0], ns.frustum[0, :, 0, 1], ns.frustum[:, 0, 0, 2]
    v = R.scaled_coordinates(rig, xs, ys, ds, (bx - dx / 2.).numpy(), dx.numpy())
    c64 = R.cells_f64(v, nxi)
    k64 = c64 >= 0
    fold = int((k64 & ((v > -1) & (v < 0)).any(-1)).sum())
    dropped = 1.0 - float(k64.mean())
    cam = np.broadcast_to(np.arange(A * N)[:, None, None, None], c64.shape)
    key = (cam // N) * (nxi[0] * nxi[1] * nxi[2]) + c64
    two = max(len(set(cam[k64][key[k64] == k])) for k in np.unique(key[k64]))
    near = float(R.near_boundary(v, 1e-3).mean())
    nearest = R.distance_to_integer(v)
    mism = int((cell.numpy().reshape(c64.shape) != c64)[~R.near_boundary(v, 1e-3)].sum())
    ref64 = R.pool_f64(logit, feat, cell.numpy(), A, nxi)
    err = float((out.double() - ref64).abs().max() / ref64.abs().max())
    print(f"kept {int(k64.sum())} of {k64.size}, folded (-1, 0): {fold}, dropped {dropped:.2%}, cameras in the busiest shared cell {two}, within 1e-3 of an integer "
          f"{near:.2%}, nearest {nearest:.2e}, fp32 / float64 cell mismatches outside the band {mism}, cumsum error {err:.2e} of the scale")
    assert fold >= 10 and dropped >= 0.10 and two >= 2 and near <= 0.01 and nearest > 1e-6 and mism == 0
    fixture = {**{k: rig[k].numpy() for k in R.CAMS}, "xs": xs.numpy(), "ys": ys.numpy(), "ds": ds.numpy(), "dx": dx.numpy(), "bx": bx.numpy(),
               "nx": nx.numpy(), "geom": geom.numpy(), "cell": cell.numpy(), "kept": kept.numpy(), "depth_logit": logit.numpy(), "x_img": feat.numpy(),
               "out": out.numpy()}
    path = os.path.join(HERE, "lss_pool.npz")
    np.savez_compressed(path, **fixture)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
