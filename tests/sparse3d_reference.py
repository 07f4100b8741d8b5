"""An independent float64 restatement of the sparse 3-D trunk BY DENSE ``F.conv3d`` (no site lists, no searchsorted, no kernels): scatter the rows to
[N, C, D, H, W], convolve, relu(scale y + shift), multiply by the site mask.  The mask of a submanifold layer is its input's; a strided layer's is
``conv3d(mask, ones, stride, padding) > 0``.  Rows whose coordinates lie outside the grid are ignored."""
import torch
import torch.nn.functional as F


def scatter(features, indices, shape, batch, count=None):
    """rows [:count] -> (dense [N, C, D, H, W] float64, mask [N, 1, D, H, W] float64)."""
    n = indices.shape[0] if count is None else int(count)
    idx = indices[:n].long().cpu()
    f = features[:n].double().cpu()
    D, H, W = shape
    hi = torch.tensor([batch, D, H, W])
    ok = ((idx >= 0) & (idx < hi)).all(dim=1)
    idx, f = idx[ok], f[ok]
    dense = torch.zeros((batch, D, H, W, f.shape[1]), dtype=torch.float64)
    mask = torch.zeros((batch, D, H, W, 1), dtype=torch.float64)
    dense[idx[:, 0], idx[:, 1], idx[:, 2], idx[:, 3]] = f
    mask[idx[:, 0], idx[:, 1], idx[:, 2], idx[:, 3]] = 1.0
    return dense.permute(0, 4, 1, 2, 3).contiguous(), mask.permute(0, 4, 1, 2, 3).contiguous()


def bn_affine(bn):
    scale = bn.weight.detach().double().cpu() / torch.sqrt(bn.running_var.detach().double().cpu() + bn.eps)
    return scale, bn.bias.detach().double().cpu() - bn.running_mean.detach().double().cpu() * scale


def layer(dense, mask, weight, scale, shift, kernel, stride, padding, subm):
    """One conv + batch norm + ReLU layer; weight [Cout, kd, kh, kw, Cin].  -> (dense, mask) of the output."""
    w = weight.detach().double().cpu().permute(0, 4, 1, 2, 3).contiguous()
    y = F.conv3d(dense, w, stride=stride, padding=padding)
    if not subm:
        mask = (F.conv3d(mask, torch.ones((1, 1, *kernel), dtype=torch.float64), stride=stride, padding=padding) > 0).double()
    return torch.relu(y * scale.view(1, -1, 1, 1, 1) + shift.view(1, -1, 1, 1, 1)) * mask, mask


def sequential(seq, dense, mask):
    """A (conv, BatchNorm1d, ReLU) SparseSequential of coalign_amd.sparse3d, or a nest of them."""
    mods = list(seq)
    if hasattr(mods[0], "kernel_size"):
        conv, bn = mods[0], mods[1]
        scale, shift = bn_affine(bn)
        return layer(dense, mask, conv.weight, scale, shift, conv.kernel_size, conv.stride, conv.padding, conv.subm)
    for m in mods:
        dense, mask = sequential(m, dense, mask)
    return dense, mask


def backbone(bb, features, indices, batch):
    """VoxelBackBone8x of coalign_amd.sparse3d on the dense route -> (dense [N, C, D, H, W], mask) of conv_out."""
    dense, mask = scatter(features, indices, bb.sparse_shape, batch)
    for name in ("conv_input", "conv1", "conv2", "conv3", "conv4", "conv_out"):
        dense, mask = sequential(getattr(bb, name), dense, mask)
    return dense, mask


def sites(mask):
    """The active cells as (batch, z, y, x) int32 rows, ascending in the linear cell index."""
    return torch.nonzero(mask[:, 0] > 0).to(torch.int32)


def height_compression(dense):
    N, C, D, H, W = dense.shape
    return dense.reshape(N, C * D, H, W)
