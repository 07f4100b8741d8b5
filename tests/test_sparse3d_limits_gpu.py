"""The sparse 3-D trunk's kernels (csrc/sparse_conv3d.hip) at their full-grid, scan-pass and channel-scale limits, on the MI355X, against the key-based float64
reference of tests/sparse3d_reference.py (no tensor of the grid's size):

* one submanifold and one stride-2 layer on grids of exactly 256 word blocks (the last single-pass size of ``sp3d_scan_sums``), of 257 (the first carry) and of
  2 146 959 360 cells (just under the ``N D H W <= INT32_MAX`` limit), sites seeded on every edge of the index's units -- sites, order and device count exact,
  values within 3e-6 of each output channel's own scale;
* the whole backbone + to-dense on the OPV2V grid of five agents (14 094 blocks, 56 passes; its second level 8 passes), then level by level;
* every matrix-core combination on folded weights whose output channels sit on scales 2^-20 ... 2^6, input channels on 2^-6 ... 2^7: 3e-6 of the channel's scale,
  the zero channel exactly relu(shift); an ordinary layer bit for bit what the weight image without the per-channel power of two gave;
* the levels behind a capacity overflow, the status word only ever OR-ed; ``sp3d_mean_vfe`` at num_points of 0, 1 and above T, M around the workgroup size."""
import copy

import pytest
import torch

import sparse3d_cases as cases
import sparse3d_limit_cases as limits
import sparse3d_reference as ref
import test_sparse3d_limits_cpu as shared
from conftest import assert_elementwise
from coalign_amd import ops, sparse3d

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
BOUND = limits.BOUND


@pytest.fixture(autouse=True)
def _kernel_route(monkeypatch):
    monkeypatch.setenv("COALIGN_SP3D", "1")


def _on_device(case, feats, status=None):
    count = None if case.count is None else torch.tensor([case.count], dtype=torch.int32, device=DEV)
    return sparse3d.SparseTensor3d(feats.to(DEV), case.indices.to(DEV), case.shape, case.batch, count,
                                   torch.zeros(1, dtype=torch.int32, device=DEV) if status is None else status)


def _layers_of(seq):
    """The (conv, BatchNorm1d, ReLU) runs of a SparseSequential nest, in order."""
    if isinstance(seq[0], sparse3d._SparseConvBase):
        yield seq
    else:
        for m in seq:
            yield from _layers_of(m)


# ---- grid size ------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spec", [limits.SUBM_LAYER, limits.STRIDED_LAYER], ids=["subm_16_16", "s2p1_16_32"])
@pytest.mark.parametrize("name", limits.LAYER_GRIDS)
def test_layers_on_the_big_grids(name, spec):
    """subm: ``sp3d_index_build`` + ``sp3d_perm`` on a shuffled list, ``sp3d_neighbors`` and a (16, 16, 3) submanifold layer -- its ranks come from ``sp3d_scan_sums``'
    per-block offsets alone, so without the carry between passes the 257-block grid fails here and the 256-block grid does not.  s2p1: ``sp3d_mark_strided`` +
    ``sp3d_enumerate`` and a (16, 32, 3) stride-2 padding-1 layer, whose device count is the scan's total.  The grid's index (0.55 GB on the largest) lives in the test
    that builds it and is freed with it."""
    case = limits.CASES[name]
    cin, cout, subm, k, s, p = spec
    feats = limits.round22(cases.features(case, cin, seed=3))                          # the 22-bit values an sp16 pair holds: the kernel's own operands
    x = _on_device(case, feats)
    layer = cases.make_layer(cin, cout, subm, k, s, p, seed=cin + cout).to(DEV)
    assert layer[0].kernel_reason(x) is None
    with torch.no_grad():
        out = layer(x)
    assert out.count is not None and out.count.is_cuda
    rows = int(out.count.item())
    what = f"{name} {'subm' if subm else 'strided'}"
    worst = []
    want = limits.check_layer(case, layer, feats, out, rows, lambda g, w, pre, wh: worst.append(limits.assert_rows_close(g, w, pre, wh)), what,
                              operands=limits.folded(layer))
    blocks, passes = limits.blocks_and_passes(out.batch_size, out.spatial_shape)
    print(f"\n{what}: {rows} rows on {out.batch_size} x {tuple(out.spatial_shape)} ({blocks} blocks, {passes} passes), worst channel error {worst[0]:.2e} (bound {BOUND:g})")
    assert want.keys.numel() >= 300 and int(out.status.item()) == 0
    assert x._index.numel() == ops.sp3d_index_bytes(case.batch, case.shape, case.indices.shape[0])
    del x, out
    torch.cuda.empty_cache()


def test_backbone_and_to_dense_on_the_opv2v_grid():
    """The deployed grid, five agents: output sites and count exact, the map equal to the reference at every occupied pixel and zero elsewhere, written into a
    NaN-poisoned buffer; then the twelve layers one by one, each level's site list against the reference's, so that a wrong level is not masked by the next.
    Values: ``assert_elementwise``'s defaults, the bound of the existing whole-backbone test (twelve float32 layers against one float64 chain)."""
    case, bb, vox, t, levels = shared.opv2v_backbone()
    bb = copy.deepcopy(bb).to(DEV)
    d = {k: v.to(DEV) for k, v in vox.items()}
    d["batch_size"] = case.batch
    with torch.no_grad():
        d = bb(sparse3d.MeanVFE({}, 4)(d))
    out = d["encoded_spconv_tensor"]
    assert all(m.kernel_reason() is None for _, m in bb.sparse_convs())
    rows = int(out.count.item())
    assert out.spatial_shape == t.shape and rows == t.keys.numel() > 100 and torch.equal(out.indices[:rows].cpu().long(), t.coords())
    assert int(bb.last_status.item()) == 0
    poisoned = torch.full((case.batch, 64 * t.shape[0], t.shape[1], t.shape[2]), float("nan"), device=DEV).contiguous(memory_format=torch.channels_last)
    got = ops.sp3d_to_dense(out.features, out.count, out._index, out.batch_size, out.spatial_shape, out=poisoned)
    assert got is poisoned and not bool(torch.isnan(got).any())
    pix, vals = ref.key_height_compression(t)
    on = pix.to(DEV)
    worst = assert_elementwise(got[on[:, 0], :, on[:, 1], on[:, 2]], vals, "map at the occupied pixels")
    assert int(torch.count_nonzero(got.abs().amax(dim=1))) <= pix.shape[0]
    counts = []
    x = sparse3d.SparseTensor3d(sparse3d.MeanVFE({}, 4)({"voxel_features": vox["voxel_features"].to(DEV), "voxel_num_points": vox["voxel_num_points"].to(DEV)})["voxel_features"],
                                vox["voxel_coords"].to(DEV), bb.sparse_shape, case.batch, None, torch.zeros(1, dtype=torch.int32, device=DEV))
    _, row_site = ref.key_scatter(torch.zeros(case.indices.shape[0], 1), case.indices, case.shape, case.batch)
    i = 0
    for name in ("conv_input", "conv1", "conv2", "conv3", "conv4", "conv_out"):
        for seq in _layers_of(getattr(bb, name)):
            with torch.no_grad():
                x = seq(x)
            lv, n = levels[i], int(x.count.item())
            assert x.spatial_shape == lv.shape and n == lv.keys.numel(), (i, n, lv.keys.numel())
            if seq[0].subm and i < 2:                                                # level 0 keeps the list's shuffled order
                assert torch.equal(x.indices[:n].cpu(), case.indices)
                assert_elementwise(x.features[:n].cpu(), lv.feats[row_site], f"layer {i}")
            else:
                assert torch.equal(x.indices[:n].cpu().long(), lv.coords()), i
                assert_elementwise(x.features[:n].cpu(), lv.feats, f"layer {i}")
            if not seq[0].subm:
                counts.append(n)
            i += 1
    assert i == 12 and int(x.status.item()) == 0
    print(f"\nOPV2V grid x 5: {case.indices.shape[0]} voxels -> {counts} sites per strided level, {pix.shape[0]} occupied pixels, map worst {worst:.2e} of the scale")


# ---- per-channel precision ------------------------------------------------------------------------------------------------------------------------------------------
def _tile_edge_case(rows):
    return next(c for c in cases.CASES if c.name == f"rows_{rows}")


@pytest.mark.parametrize("rows", (65, 257))
@pytest.mark.parametrize("combo", cases.COMBOS, ids=lambda c: f"{c[0]}_{c[1]}_k{''.join(map(str, sparse3d._triple(c[2])))}")
def test_mixed_channel_scales_against_float64(combo, rows, monkeypatch):
    """Output channels of the FOLDED weight on scales 2^-20 ... 2^6 (through ``bn.weight``, so ``sparse3d._fold`` is in the path), one all-zero; input channels on
    2^-6 ... 2^7.  Every element within 3e-6 of its channel's scale (max |pre-activation| over the rows) of the float64 sum over the 22-bit operands -- WITHOUT the
    allowance A = 2^-33 x sum of |x| over the terms whose folded |w| is below 2^-14, which a weight image without a per-channel power of two needed (measured before
    ``pack_sp3d_weights`` scaled its rows: worst channel 1.8e-4 ... 1.3e-3 without A, 3.5e-7 beyond it; since then 3.5e-7 without it); both figures and the float32 torch-op route's
    are printed.  The zero channel is exactly relu(shift).  (4, 16, 3) is fp32 vector arithmetic and has no pair to lose: the same bound."""
    cin, cout, kernel = combo
    case = _tile_edge_case(rows)
    geo = (True, 3, 1, 1) if kernel == 3 else (False, *cases.K311)
    layer = limits.mixed_scale_layer(cin, cout, *geo, seed=cin + cout).to(DEV)
    feats = limits.mixed_scale_features(case, cin, seed=rows)
    feats = feats if cin == 4 else limits.round22(feats)
    w, shift = limits.folded(layer)
    assert float(w[limits.ZERO_CH].abs().max()) == 0.0 and int((w.abs().amax(dim=(1, 2, 3, 4)) < limits.SMALL_W).sum()) >= 3      # the zero row and rows wholly below 2^-14
    allowance = limits.small_weight_allowance(case, layer, feats, w)
    kept = {}
    with torch.no_grad():
        out = layer(_on_device(case, feats))
        limits.check_layer(case, layer, feats, out, int(out.count.item()), lambda g, wnt, pre, wh: kept.update(kernel=(g, wnt, pre)), "kernel route", operands=(w, shift))
        monkeypatch.setenv("COALIGN_SP3D", "0")
        other = layer(_on_device(case, feats))
        limits.check_layer(case, layer, feats, other, other.rows(), lambda g, wnt, pre, wh: kept.update(torch=(g, wnt, pre)), "torch-op route", operands=(w, shift))
    got, want, pre = kept["kernel"]
    assert got.shape[0] >= 60 and allowance.shape == got.shape
    e_plain, e_less_a, e_torch = limits.channel_error(got, want, pre), limits.channel_error(got, want, pre, allowance), limits.channel_error(*kept["torch"])
    print(f"\nsp3d_conv {combo} on {got.shape[0]} rows: worst channel error {e_plain:.2e} of the channel's scale, {e_less_a:.2e} beyond A (bound {BOUND:g}); "
          f"float32 torch-op route {e_torch:.2e}")
    assert torch.equal(got[:, limits.ZERO_CH], torch.relu(shift[limits.ZERO_CH]).expand(got.shape[0])), combo
    limits.assert_rows_close(got, want, pre, f"{combo} on {rows} rows")


def test_an_ordinary_layer_keeps_the_bits_of_the_unscaled_image(golden):
    """Scaling a weight row by a power of two is exact in fp16 and fp32 away from underflow, so a layer whose folded weights are all normal as sp16 pairs computes
    the SAME BITS with and without the image's per-channel power of two.  tests/golden/sp3d_conv_bits.npz holds a (16, 32, 3) submanifold layer on 257 rows and the
    output of the kernel as it was before the image had its tail (tests/golden/make_sp3d_conv_bits.py, run at that commit)."""
    z = golden("sp3d_conv_bits.npz")
    w, shift, feats, idx = (torch.from_numpy(z[k]) for k in ("weight", "shift", "feats", "indices"))
    batch, shape = int(z["batch"]), tuple(int(v) for v in z["shape"])
    assert tuple(w.shape) == (32, 27, 16) and float(w.abs().min()) >= 2.0 ** -7                    # every pair normal, its low half included
    n = idx.shape[0]
    idx, count = idx.to(DEV), torch.tensor([n], dtype=torch.int32, device=DEV)
    index = ops.sp3d_index_build(idx, count, batch, shape)
    nbr = ops.sp3d_neighbors(idx, count, batch, shape, index, n, shape, 3, 1, 1)
    y = ops.sp3d_conv(feats.to(DEV), nbr, count, 32, ops.pack_sp3d_weights(w).to(DEV), shift.to(DEV))
    assert torch.equal(y.cpu(), torch.from_numpy(z["out"]))


# ---- chained overflow -----------------------------------------------------------------------------------------------------------------------------------------------
def _run_blocks(bb, vox, batch, status):
    """The backbone's blocks in ``VoxelBackBone8x.forward``'s order with every layer's ``site_capacity`` AS IT IS SET (forward gives all layers one value; the sites
    of these voxels shrink from level to level, so one value cannot spare the first strided level and cut the second) -> (the tensor behind each layer, the map)."""
    mean = sparse3d.MeanVFE({}, 4)({"voxel_features": vox["voxel_features"].to(DEV), "voxel_num_points": vox["voxel_num_points"].to(DEV)})["voxel_features"]
    x = sparse3d.SparseTensor3d(mean, vox["voxel_coords"].to(DEV), bb.sparse_shape, batch, None, status)
    outs = []
    with torch.no_grad():
        for name in ("conv_input", "conv1", "conv2", "conv3", "conv4", "conv_out"):
            for seq in _layers_of(getattr(bb, name)):
                x = seq(x)
                outs.append(x)
        return outs, sparse3d.HeightCompression({"feature_num": 128}).compress(x)


def _against_levels(outs, dense, levels, what):
    for i, (x, lv) in enumerate(zip(outs, levels)):
        if i < 2:
            continue                                                                 # (level 0: the input's own list)
        n = int(x.count.item())
        assert n == lv.keys.numel() and torch.equal(x.indices[:n].cpu().long(), lv.coords()), (what, i, n, lv.keys.numel())
        assert_elementwise(x.features[:n].cpu(), lv.feats, f"{what} layer {i}")
    pix, vals = ref.key_height_compression(levels[-1])
    on = pix.to(DEV)
    assert_elementwise(dense[on[:, 0], :, on[:, 1], on[:, 2]], vals, what + " map")
    assert int(torch.count_nonzero(dense.abs().amax(dim=1))) <= pix.shape[0], what


def test_the_levels_behind_a_capacity_overflow():
    """The second strided level (conv3) exceeds its capacity, the first does not: the bitmap of that level still holds bits whose rank is past the capacity, and
    every later level and the dense map must equal the reference with the same cut.  Bit 0 of the caller's status word is set and the word's other bits stay; a
    second run with ample capacity on the SAME word clears nothing, and on a fresh word sets nothing."""
    shape = (41, 64, 64)
    bb = cases.seed_backbone_(sparse3d.VoxelBackBone8x({"num_features_out": 64}, 4, [shape[2], shape[1], shape[0] - 1]), 5).eval()
    vox = cases.voxels(shape, 2, seed=6)
    mean = vox["voxel_features"].double().sum(dim=1) / vox["voxel_num_points"].clamp(min=1).view(-1, 1).double()
    _, free = ref.key_backbone(bb, mean, vox["voxel_coords"], 2)
    full2 = free[5].full
    cap = full2 - 200
    assert free[2].full > full2 > cap > free[8].full > free[11].full                # the cut bites at conv3 alone
    for n, m in bb.sparse_convs():
        m.site_capacity = None if n.startswith("conv2") else cap
    _, cut = ref.key_backbone(bb, mean, vox["voxel_coords"], 2, capacities="as set")
    assert cut[5].keys.numel() == cap and cut[5].full == full2 and cut[8].keys.numel() < free[8].keys.numel()      # the dropped sites are missed behind it
    bb = bb.to(DEV)
    status = torch.tensor([4], dtype=torch.int32, device=DEV)                       # a bit of the caller's own
    outs, dense = _run_blocks(bb, vox, 2, status)
    assert int(status.item()) == 5 and all(o.status is status for o in outs)
    _against_levels(outs, dense, cut, "cut at conv3")
    for _, m in bb.sparse_convs():
        m.site_capacity = None
    outs, dense = _run_blocks(bb, vox, 2, status)
    assert int(status.item()) == 5                                                  # only ever OR-ed: nothing cleared
    _against_levels(outs, dense, free, "ample capacity")
    fresh = torch.zeros(1, dtype=torch.int32, device=DEV)
    _run_blocks(bb, vox, 2, fresh)
    assert int(fresh.item()) == 0


# ---- MeanVFE --------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", (4, 5))
@pytest.mark.parametrize("M", (0, 1, 3, 255, 256, 257))
def test_mean_vfe_edges(M, C):
    """num_points of 0 (divides by 1), 1, and T + 3 (sums the T slots, divides by T + 3, as mean_vfe.py:26-30 does), every slot filled whatever the count says;
    against float64 within (T + 1) 2^-24 of sum |v| / max(n, 1): T - 1 float32 additions of partial sums no larger than sum |v|, one division."""
    T = 5
    g = torch.Generator().manual_seed(10 * M + C)
    v = torch.randn((M, T, C), generator=g) * 3.0
    n = torch.tensor([0, T + 3, 1, 2, T, 3][:M] + [int(a) for a in torch.randint(0, T + 4, (max(M - 6, 0),), generator=g)], dtype=torch.int32)
    got = ops.sp3d_mean_vfe(v.to(DEV), n.to(DEV)).cpu()
    assert tuple(got.shape) == (M, C)
    div = n.clamp(min=1).view(-1, 1).double()
    want = v.double().sum(dim=1) / div
    bound = (T + 1) * 2.0 ** -24 * v.double().abs().sum(dim=1) / div
    assert bool(((got.double() - want).abs() <= bound).all()), float(((got.double() - want).abs() - bound).max())
    if M >= 2:
        assert torch.equal(got[0], v[0, 0] + v[0, 1] + v[0, 2] + v[0, 3] + v[0, 4])                # n = 0: the plain sum, slot order
        assert torch.equal(got[1], (v[1, 0] + v[1, 1] + v[1, 2] + v[1, 3] + v[1, 4]) / float(T + 3))
