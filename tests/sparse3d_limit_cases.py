"""The cases of the sparse 3-D trunk's limit tests (tests/test_sparse3d_limits_cpu.py: the key-based reference against the dense one, the torch-op route on the big
grids; tests/test_sparse3d_limits_gpu.py: the kernels): grids from the last single-pass size of the prefix count to the largest grid the kernels take, with sites
seeded ON the edges of the index's units; layers whose folded weights put every output channel on its own scale; the per-channel bound.

The site index counts in three units: a 32-cell bitmap WORD, a 1024-word (32 768-cell) BLOCK of ``sp3d_block_sums`` / ``sp3d_word_prefix``, and a 256-block
(8 388 608-cell) PASS of ``sp3d_scan_sums``, whose carry only exists above 256 blocks.  ``sites`` puts a 3 x 3 x 3 block and a short plane on cell 0, on the last
cell, and on both sides of the first word, block and pass edge, of the second pass edge and of the first batch item's edge -- for the grid itself and for the grid
of the stride-2 layer behind it --, then adds random clusters, and shuffles the list."""
from collections import namedtuple

import torch
import torch.nn as nn

import sparse3d_cases as cases
import sparse3d_reference as ref
from coalign_amd import sparse3d

WORD, BLOCK, PASS = 32, 32 * 1024, 256 * 32 * 1024
BOUND = 3e-6                     # of the channel's own scale: the project's bound for sp16 kernels (tests/test_sp_limits_gpu.py, tests/test_lss_bev_gpu.py)
SMALL_W = 2.0 ** -14             # below it an UNSCALED sp16 pair keeps an absolute 2^-34 only (csrc/common.h)
PAIR_ABS = 2.0 ** -33            # ... doubled: the worst case per such weight, times |x|
ZERO_CH = 3                      # the all-zero output channel of a mixed-scale layer

# name -> (batch, sparse shape): exactly 256 blocks, one pass | 257 blocks, the first carry | the OPV2V grid of five agents, 14 094 blocks, 56 passes (its second
# level, 5 x (21, 400, 1408), has 1 805 blocks, 8 passes) | 2 146 959 360 cells, 65 520 blocks, 256 passes, just under INT32_MAX
GRIDS = {"blocks_256": (2, (64, 256, 256)), "blocks_257": (2, (64, 256, 257)), "opv2v_5_agents": (5, (41, 800, 2816)), "below_int32_max": (1, (64, 8192, 4095))}
LAYER_GRIDS = ("blocks_256", "blocks_257", "below_int32_max")
REFUSED = [(1, (64, 8192, 4096)), (4, (128, 2048, 2048)), (1, (64, 8192, 4097)), (24, (41, 800, 2816))]      # 2^31 cells exactly, twice; one row more; the OPV2V grid of 24 agents
SUBM_LAYER, STRIDED_LAYER = (16, 16, True, 3, 1, 1), (16, 32, False, *cases.K3S2P1)

Case = cases.Case


def cells(batch, shape):
    return batch * shape[0] * shape[1] * shape[2]


def blocks_and_passes(batch, shape):
    words = -(-cells(batch, shape) // WORD)
    blocks = -(-words // 1024)
    return blocks, -(-blocks // 256)


def edge_cells(batch, shape):
    """The linear cell indices the clusters are centred on."""
    total, item = cells(batch, shape), shape[0] * shape[1] * shape[2]
    out = [0, total - 1]
    for e in (WORD, BLOCK, PASS, 2 * PASS, item):
        if 0 < e < total:
            out += [e - 1, e]
    return sorted(set(out))


def _cluster(centre, shape, batch, plane=True):
    """A 3 x 3 x 3 block around ``centre`` = (b, z, y, x) and a 2 x 5 plane beside it, cut to the grid: every site has a neighbour."""
    b, z, y, x = (int(v) for v in centre)
    rows = [[b, z + dz, y + dy, x + dx] for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1)]
    if plane:
        rows += [[b, z, y + dy, x + dx] for dy in (2, 3) for dx in (-2, -1, 0, 1, 2)]
    t = torch.tensor(rows, dtype=torch.int64)
    ok, _ = ref.key_of(t, shape, batch)
    return t[ok]


def sites(batch, shape, seed, random_clusters=24, extra=()):
    """int32 [M, 4], unique cells in SHUFFLED order."""
    g = torch.Generator().manual_seed(seed)
    parts = [_cluster(c, shape, batch) for c in ref.key_coords(torch.tensor(edge_cells(batch, shape)), shape)]
    oshape = ref.out_shape(shape, (3, 3, 3), (2, 2, 2), (1, 1, 1))                                # the edges of the next level's index, reached from here
    hi = torch.tensor([batch - 1, shape[0] - 1, shape[1] - 1, shape[2] - 1])
    for c in ref.key_coords(torch.tensor(edge_cells(batch, oshape)), oshape):
        parts.append(_cluster(torch.minimum(c * torch.tensor([1, 2, 2, 2]), hi), shape, batch, plane=False))
    centres = torch.randint(0, cells(batch, shape), (random_clusters,), generator=g)
    parts += [_cluster(c, shape, batch) for c in ref.key_coords(centres, shape)]
    if len(extra):
        parts.append(torch.tensor(extra, dtype=torch.int64).reshape(-1, 4))
    rows = torch.unique(torch.cat(parts), dim=0)
    return rows[torch.randperm(rows.shape[0], generator=g)].to(torch.int32)


def _build():
    out = {}
    for i, (name, (batch, shape)) in enumerate(GRIDS.items()):
        D, H, W = shape
        if name == "blocks_257":
            # a count below the capacity (the rows behind it repeat live cells and carry NaN features) and rows outside the grid in interior lines: without the range
            # check (0, 3, 5, W) is cell (0, 3, 6, 0), (0, 3, 5, -1) is (0, 3, 4, W - 1), (0, 3, H, 4) is (0, 4, 0, 4) and (1, -1, 5, 5) is (0, D - 1, 5, 5), all live here
            live = [[0, 3, 6, 0], [0, 3, 6, 1], [0, 3, 4, W - 1], [0, 3, 4, W - 2], [0, 4, 0, 4], [0, 4, 1, 4], [0, D - 1, 5, 5], [0, D - 1, 5, 6], [1, 0, 5, 5], [1, 0, 5, 6]]
            bad = torch.tensor([[0, 3, 5, W], [0, 3, 5, -1], [0, 3, H, 4], [1, -1, 5, 5]], dtype=torch.int32)
            s = sites(batch, shape, 40 + i, extra=live)
            s = torch.cat([s[:100], bad[:2], s[100:], bad[2:]])
            out[name] = Case(name, "limits", shape, batch, torch.cat([s, s[:37]]), s.shape[0])
        else:
            out[name] = Case(name, "limits", shape, batch, sites(batch, shape, 40 + i))
    return out


CASES = _build()


def voxels(case, points=5, seed=0):
    """processed_lidar on a case's sites, in the list's (shuffled) order: 1 .. ``points`` points per voxel, unused slots zero."""
    g = torch.Generator().manual_seed(seed)
    M = case.indices.shape[0]
    num = torch.randint(1, points + 1, (M,), generator=g).to(torch.int32)
    feats = torch.randn((M, points, 4), generator=g)
    feats[..., 3] = torch.rand((M, points), generator=g)
    feats = feats * (torch.arange(points).view(1, -1, 1) < num.view(-1, 1, 1))
    return {"voxel_features": feats, "voxel_coords": case.indices.clone(), "voxel_num_points": num}


# ---- operands and bounds ------------------------------------------------------------------------------------------------------------------------------------------
def round22(x):
    """float32 -> 22 significant bits, ties away from zero: ``sp16_round`` of csrc/common.h, what an sp16 pair holds of a normal value."""
    return ((x.contiguous().view(torch.int32) + 2) & -4).view(torch.float32)


def folded(layer):
    """(weight [Cout, kd, kh, kw, Cin], shift [Cout]) of conv + eval batch norm in float32, by the expression of ``sparse3d._fold`` -- the operands the kernel
    route's image is made from; rounded to 22 bits where the layer runs on sp16 pairs (Cin >= 16)."""
    conv, bn = layer[0], layer[1]
    with torch.no_grad():
        scale = bn.weight * (1.0 / torch.sqrt(bn.running_var + bn.eps))
        shift = (bn.bias - bn.running_mean * scale).float()
        w = (conv.weight * scale.view(-1, 1, 1, 1, 1)).float()
    return (w if conv.in_channels == 4 else round22(w)).cpu(), shift.cpu()


def channel_error(got, want, pre, extra=None):
    """max over channels of max over rows of (|got - want| - extra) / the channel's scale (max |pre-activation| over the rows); rows [R, C]."""
    scale = pre.abs().amax(dim=0)
    err = (got.double() - want).abs()
    if extra is not None:
        err = (err - extra).clamp_min(0.0)
    err = err.amax(dim=0)
    return float(torch.where(scale > 0, err / scale.clamp_min(1e-300), err).max()) if err.numel() else 0.0


def assert_rows_close(got, want, pre, what, extra=None):
    """Every element within BOUND of its CHANNEL's scale (max |pre-activation| of the channel over the rows), + ``extra`` [R, C] where a caller derives one."""
    scale = pre.abs().amax(dim=0, keepdim=True)
    bad = (got.double() - want).abs() > BOUND * scale + (0.0 if extra is None else extra)
    worst = channel_error(got, want, pre, extra)
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} elements outside {BOUND:g} of their channel's scale; worst channel {worst:.3e}"
    return worst


def check_layer(case, layer, feats, out, rows, compare, what, operands=None):
    """``out``: the layer's SparseTensor3d with ``rows`` rows in use.  Sites, their order and the count exactly as the key-based reference has them; values through
    ``compare(got, want, pre, what)``.  ``operands``: (folded weight, shift) when the reference is to read the kernel's own 22-bit operands."""
    conv = layer[0]
    t, row_site = ref.key_scatter(feats, case.indices, case.shape, case.batch, case.count)
    if operands is None:
        want = ref.key_sequential(layer, t)
    else:
        want = ref.key_layer(t, operands[0], None, operands[1], conv.kernel_size, conv.stride, conv.padding, conv.subm, conv.site_capacity)
    got_idx, got_f = out.indices[:rows].cpu(), out.features[:rows].cpu()
    assert not bool(torch.isnan(got_f).any()), what
    if conv.subm:
        n_in = row_site.numel()
        assert rows == n_in and torch.equal(got_idx, case.indices[:n_in]), what                     # same sites, same row order
        live = row_site >= 0
        assert not bool(got_f[~live].any()), what                                                  # a row outside the grid answers zero
        compare(got_f[live], want.feats[row_site[live]], want.pre[row_site[live]], what)
    else:
        assert tuple(out.spatial_shape) == want.shape, what
        keep = want.keys.numel()
        assert rows == keep, (what, rows, keep)
        assert torch.equal(got_idx.long(), want.coords()), what                                    # ascending in the linear cell index
        overflow = int(out.status.cpu()[0]) & 1 if out.status is not None else 0
        assert overflow == int(want.full > keep), what
        compare(got_f, want.feats, want.pre, what)
    return want


# ---- one layer whose folded weight puts every output channel on its own scale ------------------------------------------------------------------------------------
def mixed_scale_layer(cin, cout, subm, kernel, stride, padding, seed, lo=-20, hi=6):
    """(conv, BatchNorm1d, ReLU), eval: an ordinary convolution weight, and a batch norm whose WEIGHT carries the channel scales 2^lo ... 2^hi, randomly permuted,
    channel ZERO_CH zero -- so the FOLDED weight (``sparse3d._fold``) has rows on those scales and one all-zero row.  running_mean = 0 and running_var = 1 - eps: the
    fold's scale is bn.weight, its shift bn.bias, which sits on the channel's scale too (``mixed_layer`` of tests/test_lss_bev_gpu.py, through the fold)."""
    g = torch.Generator().manual_seed(seed)
    layer = cases.make_layer(cin, cout, subm, kernel, stride, padding, seed)
    conv, bn = layer[0], layer[1]
    cs = (2.0 ** torch.linspace(lo, hi, cout, dtype=torch.float64)).float()[torch.randperm(cout, generator=g)]
    with torch.no_grad():
        conv.weight.copy_(torch.randn(conv.weight.shape, generator=g) / (conv.taps * cin) ** 0.5)
        bn.weight.copy_(cs)
        bn.weight[ZERO_CH] = 0.0
        bn.bias.copy_(torch.randn(cout, generator=g) * cs)
        bn.running_mean.zero_()
        bn.running_var.fill_(1.0 - bn.eps)
    return layer


def mixed_scale_features(case, cin, seed, lo=-6, hi=7):
    """[capacity, Cin] float32, input channel c on scale 2^lo ... 2^hi (a trunk's input holds coordinates up to 140 beside intensities in [0, 1])."""
    g = torch.Generator().manual_seed(seed)
    cs = (2.0 ** torch.linspace(lo, hi, cin, dtype=torch.float64)).float()[torch.randperm(cin, generator=g)]
    return torch.randn((case.indices.shape[0], cin), generator=g) * cs


def small_weight_allowance(case, layer, feats, w):
    """A [rows in use, Cout] float64: 2^-33 x the sum of |x| over the terms of each element whose folded |w| is below 2^-14 -- what an sp16 pair WITHOUT a per-channel
    power of two may lose (2^-34 absolute per such weight, doubled); list order for a submanifold layer, site order for a strided one."""
    conv = layer[0]
    t, row_site = ref.key_scatter(feats, case.indices, case.shape, case.batch, case.count)
    mask = ((w.abs() < SMALL_W) & (w != 0)).double()
    if conv.subm:
        keys, oshape = t.keys, t.shape
    else:
        keys, oshape = ref.key_strided_sites(t, conv.kernel_size, conv.stride, conv.padding)
    a = PAIR_ABS * ref.key_gather_sum(t, keys, oshape, mask, conv.kernel_size, conv.stride, conv.padding, feats=t.feats.abs())
    return a[row_site[row_site >= 0]] if conv.subm else a


def ordinary_layer():
    """The (16, 32, 3) submanifold layer of the bit-equality fixture tests/golden/sp3d_conv_bits.npz: every folded |w| at least 2^-7, far above 2^-14, so the
    weight image's per-channel power of two changes no bit of the result."""
    g = torch.Generator().manual_seed(77)
    layer = cases.make_layer(16, 32, True, 3, 1, 1, 77)
    with torch.no_grad():
        w = torch.rand(layer[0].weight.shape, generator=g) * 0.18 + 0.02
        layer[0].weight.copy_(w * (torch.randint(0, 2, w.shape, generator=g) * 2 - 1))
    return layer
