"""An independent float64 restatement of the sparse 3-D trunk BY DENSE ``F.conv3d`` (no site lists, no searchsorted, no kernels): scatter the rows to
[N, C, D, H, W], convolve, relu(scale y + shift), multiply by the site mask.  The mask of a submanifold layer is its input's; a strided layer's is
``conv3d(mask, ones, stride, padding) > 0``.  Rows whose coordinates lie outside the grid are ignored.

Second half (``key_*``, ``KeyTensor``): the same layers restated over SORTED CELL KEYS, still float64, for grids no dense tensor can hold (the OPV2V grid of five
agents has 461.8 M cells, the largest grid the kernels take 2^31 - 1).  A site set is a sorted int64 vector of linear cell indices ((b D + z) H + y) W + x; a layer is
out[r] = relu(scale (sum over the taps, ascending, of W[tap] . in[find(key of the tap's input cell)]) + shift) with ``find`` = ``searchsorted``; a strided layer's
sites are the unique reachable cells, ascending, cut to ``site_capacity`` -- a dropped site is absent for every later layer and for to-dense.  Nothing of the grid's
size is allocated.  tests/test_sparse3d_limits_cpu.py holds it to the dense half on every case of tests/sparse3d_cases.py."""
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


# ---- the same layers over sorted cell keys: nothing of the grid's size is allocated ------------------------------------------------------------------------------
class KeyTensor:
    """keys: sorted int64 [S] linear cell indices; feats: float64 [S, C] (row i belongs to keys[i]); shape (D, H, W); batch; ``full``: the sites a strided layer
    reached before the cut to its capacity (None for any other tensor); ``pre``: the layer's pre-activation scale y + shift (None for an input)."""

    def __init__(self, keys, feats, shape, batch, full=None, pre=None):
        self.keys, self.feats, self.shape, self.batch, self.full, self.pre = keys, feats, tuple(int(v) for v in shape), int(batch), full, pre

    def coords(self):
        return key_coords(self.keys, self.shape)


def key_of(idx, shape, batch):
    """int64 coordinates [.., 4] -> (inside, linear cell index)."""
    D, H, W = shape
    b, z, y, x = idx.unbind(-1)
    ok = (b >= 0) & (b < batch) & (z >= 0) & (z < D) & (y >= 0) & (y < H) & (x >= 0) & (x < W)
    return ok, ((b * D + z) * H + y) * W + x


def key_coords(keys, shape):
    """keys -> (batch, z, y, x) int64 rows."""
    D, H, W = shape
    return torch.stack([keys // (D * H * W), keys // (H * W) % D, keys // W % H, keys % W], dim=1)


def key_scatter(features, indices, shape, batch, count=None):
    """The list as the kernels see it -- any row order, rows at or past ``count`` unused, rows outside the grid no sites -> (KeyTensor, row_site): row_site int64
    [count] is the place of each list row among the sorted keys, -1 for a row outside the grid.  Cells are unique among the rows in use."""
    n = indices.shape[0] if count is None else int(count)
    idx = indices[:n].long().cpu()
    f = features[:n].double().cpu()
    ok, key = key_of(idx, shape, batch)
    rows = torch.nonzero(ok).flatten()
    skeys, order = torch.sort(key[rows])
    assert skeys.numel() < 2 or bool((skeys[1:] > skeys[:-1]).all()), "the rows in use name a cell twice"
    row_site = torch.full((n,), -1, dtype=torch.int64)
    row_site[rows[order]] = torch.arange(rows.numel())
    return KeyTensor(skeys, f[rows[order]], shape, batch), row_site


def out_shape(shape, kernel, stride, padding):
    return tuple((n + 2 * p - k) // s + 1 for n, k, s, p in zip(shape, kernel, stride, padding))


def key_strided_sites(t, kernel, stride, padding):
    """The cells of the output grid that some site of ``t`` reaches: o = (i + p - kappa) / s where the division is exact and o lies inside; unique, ascending."""
    oshape = out_shape(t.shape, kernel, stride, padding)
    c = t.coords()
    s, p = torch.tensor([1, *stride]), torch.tensor([0, *padding])
    found = []
    for kz in range(kernel[0]):
        for ky in range(kernel[1]):
            for kx in range(kernel[2]):
                num = c + p - torch.tensor([0, kz, ky, kx])
                o = torch.div(num, s, rounding_mode="floor")
                ok, key = key_of(o, oshape, t.batch)
                found.append(key[ok & (num >= 0).all(dim=1) & (num % s == 0).all(dim=1)])
    return torch.unique(torch.cat(found)), oshape


def key_gather_sum(t, out_keys, oshape, weight, kernel, stride, padding, feats=None):
    """sum over the taps, ascending (kz, ky, kx), of weight[:, kz, ky, kx, :] . in[o s - p + kappa] for the output cells ``out_keys`` -> float64 [S_out, Cout].
    ``feats``: other per-site rows than ``t.feats`` (the bound of the mixed-scale test sums |x| this way)."""
    w = weight.detach().double().cpu()
    f = t.feats if feats is None else feats
    acc = torch.zeros((out_keys.numel(), w.shape[0]), dtype=torch.float64)
    if t.keys.numel() == 0 or out_keys.numel() == 0:
        return acc
    base = key_coords(out_keys, oshape) * torch.tensor([1, *stride]) - torch.tensor([0, *padding])
    for kz in range(kernel[0]):
        for ky in range(kernel[1]):
            for kx in range(kernel[2]):
                ok, key = key_of(base + torch.tensor([0, kz, ky, kx]), t.shape, t.batch)
                pos = torch.searchsorted(t.keys, key).clamp_(max=t.keys.numel() - 1)
                hit = ok & (t.keys[pos] == key)
                if bool(hit.any()):
                    acc[hit] += f[pos[hit]] @ w[:, kz, ky, kx, :].t()
    return acc


def key_layer(t, weight, scale, shift, kernel, stride, padding, subm, site_capacity=None):
    """One conv + batch norm + ReLU layer on a KeyTensor; weight [Cout, kd, kh, kw, Cin], ``scale`` None for a weight that is folded already."""
    if subm:
        keys, oshape, full = t.keys, t.shape, None
    else:
        keys, oshape = key_strided_sites(t, kernel, stride, padding)
        full = keys.numel()
        if site_capacity is not None:
            keys = keys[:int(site_capacity)]
    y = key_gather_sum(t, keys, oshape, weight, kernel, stride, padding)
    pre = (y if scale is None else y * scale.view(1, -1)) + shift.double().view(1, -1)
    return KeyTensor(keys, torch.relu(pre), oshape, t.batch, full, pre)


def key_sequential(seq, t, levels=None):
    """A (conv, BatchNorm1d, ReLU) SparseSequential of coalign_amd.sparse3d, or a nest of them; ``levels`` collects the KeyTensor behind every layer."""
    mods = list(seq)
    if hasattr(mods[0], "kernel_size"):
        conv, bn = mods[0], mods[1]
        scale, shift = bn_affine(bn)
        t = key_layer(t, conv.weight, scale, shift, conv.kernel_size, conv.stride, conv.padding, conv.subm, conv.site_capacity)
        if levels is not None:
            levels.append(t)
        return t
    for m in mods:
        t = key_sequential(m, t, levels)
    return t


def key_backbone(bb, features, indices, batch, count=None, capacities=None):
    """VoxelBackBone8x on keys -> (KeyTensor of conv_out, [the KeyTensor behind each of the 12 layers]); every strided layer cut to ``bb.site_capacity`` as
    ``VoxelBackBone8x.forward`` has it, or, with ``capacities="as set"``, to the ``site_capacity`` its own module carries."""
    assert capacities in (None, "as set")
    for _, m in bb.sparse_convs():
        if capacities is None:
            m.site_capacity = bb.site_capacity
    t, _ = key_scatter(features, indices, bb.sparse_shape, batch, count)
    levels = []
    for name in ("conv_input", "conv1", "conv2", "conv3", "conv4", "conv_out"):
        t = key_sequential(getattr(bb, name), t, levels)
    return t, levels


def key_height_compression(t):
    """The occupied pixels of HeightCompression's map and their channel vectors: (pix int64 [P, 3] = (batch, y, x), ascending, values float64 [P, C D], channel
    c D + d; zero where (pixel, d) is no site)."""
    D = t.shape[0]
    c = t.coords()
    pix, inv = torch.unique(c[:, [0, 2, 3]], dim=0, return_inverse=True)
    C = t.feats.shape[1]
    vals = torch.zeros((pix.shape[0], C, D), dtype=torch.float64)
    if c.shape[0]:
        vals[inv, :, c[:, 1]] = t.feats
    return pix, vals.reshape(pix.shape[0], C * D)
