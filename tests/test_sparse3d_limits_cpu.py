"""The sparse 3-D trunk's limit suite without a GPU: the key-based float64 reference of tests/sparse3d_reference.py (``key_*``: sorted cell keys + searchsorted, no
tensor of the grid's size) equals the dense one on EVERY case and layer combination of tests/sparse3d_cases.py -- sites exactly, values to 1e-12 of the scale, both
being float64 --, and the torch-op route (CPU tensors, float64) equals it on the big grids of tests/sparse3d_limit_cases.py, up to 2^31 - 1 - 524 287 cells."""
import functools

import pytest
import torch

import sparse3d_cases as cases
import sparse3d_limit_cases as limits
import sparse3d_reference as ref
from coalign_amd import sparse3d


def _close64(got, want, what):
    scale = max(float(want.abs().max()), 1e-300) if want.numel() else 1.0
    err = float((got.detach().double() - want).abs().max()) if want.numel() else 0.0
    assert err <= 1e-12 * scale, f"{what}: {err / scale:.3e} of the scale"


@pytest.mark.parametrize("group", cases.GROUPS)
@pytest.mark.parametrize("combo", cases.COMBOS, ids=lambda c: f"{c[0]}_{c[1]}_k{''.join(map(str, sparse3d._triple(c[2])))}")
def test_key_reference_equals_the_dense_reference(combo, group):
    cin, cout, kernel = combo
    ran = 0
    for case in cases.of_group(group):
        for subm, k, s, p in cases.geometries(case, kernel):
            layer = cases.make_layer(cin, cout, subm, k, s, p, seed=cin + cout, site_capacity=case.site_capacity).double()
            feats = cases.features(case, cin, seed=3)
            what = f"{case.name} {'subm' if subm else 'strided'} {k}/{s}/{p}"
            dense, mask = cases.reference(case, layer, feats)
            want_sites = ref.sites(mask).long()
            t, row_site = ref.key_scatter(feats, case.indices, case.shape, case.batch, case.count)
            got = ref.key_sequential(layer, t)
            n_in = case.indices.shape[0] if case.count is None else case.count
            ok = ((case.indices[:n_in] >= 0) & (case.indices[:n_in] < torch.tensor([case.batch, *case.shape]))).all(dim=1)
            assert torch.equal(row_site >= 0, ok), what                                            # out-of-range rows are no sites
            assert torch.equal(t.coords()[row_site[ok]], case.indices[:n_in][ok].long()), what     # ... and every other row finds its own cell
            full = want_sites.shape[0]
            keep = full if (subm or case.site_capacity is None) else min(full, case.site_capacity)
            assert got.shape == tuple(dense.shape[2:]), what
            assert torch.equal(got.coords(), want_sites[:keep]), what                              # sites exact, ascending, cut to the capacity
            if not subm:
                assert got.full == full and (case.n_out is None or full == case.n_out), what
            i = got.coords()
            _close64(got.feats, dense[i[:, 0], :, i[:, 1], i[:, 2], i[:, 3]], what)
            if group == "to_dense" and keep == full:
                pix, vals = ref.key_height_compression(got)
                want = ref.height_compression(dense)
                occupied = torch.nonzero(mask[:, 0].sum(dim=1) > 0)
                assert torch.equal(pix, occupied), what
                _close64(vals, want[pix[:, 0], :, pix[:, 1], pix[:, 2]], what + " dense")
            ran += 1
    assert ran > 0 or (group == "strided")


def test_key_backbone_equals_the_dense_backbone():
    """All twelve layers chained, and the cut of a strided level carried through the levels behind it (the dense reference has no cut: compared without one)."""
    shape = (41, 64, 64)
    bb = cases.seed_backbone_(sparse3d.VoxelBackBone8x({"num_features_out": 64}, 4, [shape[2], shape[1], shape[0] - 1]), 5).eval().double()
    vox = cases.voxels(shape, 2, seed=6)
    mean = vox["voxel_features"].double().sum(dim=1) / vox["voxel_num_points"].clamp(min=1).view(-1, 1).double()
    dense, mask = ref.backbone(bb, mean, vox["voxel_coords"], 2)
    perm = torch.randperm(mean.shape[0], generator=torch.Generator().manual_seed(1))                # the list order is the caller's
    t, levels = ref.key_backbone(bb, mean[perm], vox["voxel_coords"][perm], 2)
    assert len(levels) == 12 and [lv.shape for lv in levels][-1] == tuple(dense.shape[2:])
    assert torch.equal(t.coords(), ref.sites(mask).long()) and t.keys.numel() > 50
    i = t.coords()
    _close64(t.feats, dense[i[:, 0], :, i[:, 1], i[:, 2], i[:, 3]], "backbone")
    pix, vals = ref.key_height_compression(t)
    _close64(vals, ref.height_compression(dense)[pix[:, 0], :, pix[:, 1], pix[:, 2]], "backbone dense")


def test_big_grid_cases_sit_on_the_edges_they_name():
    """Every case holds a few hundred to a few thousand unique sites with both sides of every edge of its grid among them, and every site has a neighbour."""
    assert [limits.blocks_and_passes(*limits.GRIDS[n]) for n in limits.GRIDS] == [(256, 1), (257, 2), (14094, 56), (65520, 256)]
    assert limits.blocks_and_passes(5, (21, 400, 1408)) == (1805, 8)                             # the OPV2V grid's second level is still multi-pass
    assert limits.cells(*limits.GRIDS["below_int32_max"]) == 2146959360 < 2 ** 31 - 1
    assert all(limits.cells(b, s) >= 2 ** 31 for b, s in limits.REFUSED) and [limits.cells(b, s) for b, s in limits.REFUSED[:2]] == [2 ** 31] * 2
    for name, case in limits.CASES.items():
        n = case.indices.shape[0] if case.count is None else case.count
        t, row_site = ref.key_scatter(torch.zeros(case.indices.shape[0], 1), case.indices, case.shape, case.batch, case.count)
        assert 300 <= t.keys.numel() <= 5000, (name, t.keys.numel())
        listed = ref.key_of(case.indices[:n].long(), case.shape, case.batch)[1]
        assert int((listed[1:] < listed[:-1]).sum()) > n // 4, name                                # the list is shuffled
        for c in limits.edge_cells(case.batch, case.shape):
            assert bool((t.keys == c).any()), (name, c)
        total = limits.cells(case.batch, case.shape)
        wanted = [0, total - 1, 31, 32, 32767, 32768, case.shape[0] * case.shape[1] * case.shape[2] - 1, case.shape[0] * case.shape[1] * case.shape[2]]
        wanted += [c for c in (8388607, 8388608, 16777215, 16777216) if c < total]
        assert all(bool((t.keys == c).any()) for c in wanted if 0 <= c < total), name
        ones = torch.ones((1, 3, 3, 3, 1), dtype=torch.float64)
        near = ref.key_gather_sum(ref.KeyTensor(t.keys, torch.ones((t.keys.numel(), 1), dtype=torch.float64), case.shape, case.batch), t.keys, case.shape, ones,
                                  (3, 3, 3), (1, 1, 1), (1, 1, 1))
        assert float(near.min()) >= 2.0, name                                                      # itself and at least one neighbour
    c257 = limits.CASES["blocks_257"]
    assert c257.count is not None and c257.count < c257.indices.shape[0]
    assert int((ref.key_scatter(torch.zeros(c257.indices.shape[0], 1), c257.indices, c257.shape, c257.batch, c257.count)[1] < 0).sum()) == 4


def _decode_image(img, cout, taps, cin):
    """The weight image of ``ops.pack_sp3d_weights`` back to (h + 2^-10 l [Cout, taps Cin] float64 -- the scaled rows as the pairs hold them --, 2^k_c [Cout])."""
    rows, K = (cout + 31) // 32 * 32, taps * cin
    pairs = img[:K // 16 * (rows // 32) * 2048].view(torch.float16).reshape(K // 16, rows // 32, 2, 32, 2, 8)      # [step][tile][half][r][h | l][j]
    value = pairs[..., 0, :].double() + pairs[..., 1, :].double() / 1024.0
    value = value.permute(1, 3, 0, 2, 4).reshape(rows, K)                                                          # [tile, r, step, half, j]
    tail = img[K // 16 * (rows // 32) * 2048:].view(torch.float32)
    assert tail.numel() == rows and not bool(value[cout:].any()) and bool((tail[cout:] == 1).all())
    return value[:cout], tail[:cout]


@pytest.mark.parametrize("combo", cases.COMBOS[1:], ids=lambda c: f"{c[0]}_{c[1]}_k{''.join(map(str, sparse3d._triple(c[2])))}")
def test_weight_image_scales_every_row_by_its_own_power_of_two(combo):
    """Rows on scales 2^-20 ... 2^6 and one zero row: the pairs hold the row divided by 2^k_c with its largest |w| in [1, 2), the tail holds 2^k_c (1 for the zero row
    and behind Cout), and pair x tail is the weight rounded to 22 bits wherever the SCALED weight is at least 2^-13 -- i.e. down to 2^-14 of the row's largest, whatever
    the row's scale -- and within 2^-34 2^k_c below that.  The image's size is what the library asks for."""
    from coalign_amd import hip, ops
    cin, cout, kernel = combo
    taps = 27 if kernel == 3 else 3
    layer = limits.mixed_scale_layer(cin, cout, kernel == 3, *((3, 1, 1) if kernel == 3 else cases.K311), seed=cin + cout)
    w, _ = limits.folded(layer)                                                   # rounded to 22 bits
    w = w.reshape(cout, taps * cin)
    img = ops.pack_sp3d_weights(w.reshape(cout, taps, cin))
    assert img.dtype == torch.uint8 and img.numel() == hip.lib().coalign_sp3d_weight_bytes(cin, cout, taps)
    value, tail = _decode_image(img, cout, taps, cin)
    top = w.abs().amax(dim=1)
    assert float(tail[limits.ZERO_CH]) == 1.0 and not bool(value[limits.ZERO_CH].any())
    live = top > 0
    assert bool((torch.log2(tail.double()) == torch.floor(torch.log2(top.double().clamp_min(1e-300))))[live].all())
    assert 1.0 <= float(value[live].abs().amax(dim=1).min()) and float(value.abs().max()) < 2.0
    back = value * tail.double().view(-1, 1)
    normal = value.abs() >= 2.0 ** -13                                             # (the last of a pair's 22 bits is 2^-21 of the value's power of two: fp16 holds it, times 2^10, from 2^-13 on)
    assert bool((back == w.double())[normal].all()) and int(normal.sum()) > 0.99 * int(live.sum()) * w.shape[1]
    assert bool(((back - w.double()).abs() <= 2.0 ** -34 * tail.double().view(-1, 1)).all())
    assert float(top[live].min()) < 2.0 ** -19                                     # the rows an unscaled image held to 2^-34 absolute


def test_grids_of_2_to_the_31_cells_are_refused_on_the_host():
    """``ops.sp3d_index_bytes`` refuses with ValueError before anything is allocated or launched (there is no GPU here); the largest case's index is 0.55 GB."""
    from coalign_amd import ops
    for batch, shape in limits.REFUSED:
        with pytest.raises(ValueError):
            ops.sp3d_index_bytes(batch, shape, 1000)
    batch, shape = limits.GRIDS["below_int32_max"]
    words = limits.cells(batch, shape) // 32
    assert ops.sp3d_index_bytes(batch, shape, 1024) == 8 * words + 256 * -(-(65520 + 1) * 4 // 256) + 4096
    assert ops.sp3d_index_bytes(1, (1, 1, 2 ** 31 - 1), 1) > 0                                      # INT32_MAX itself is inside


@pytest.mark.parametrize("spec", [limits.SUBM_LAYER, limits.STRIDED_LAYER], ids=["subm_16_16", "s2p1_16_32"])
@pytest.mark.parametrize("name", limits.LAYER_GRIDS)
def test_torch_route_on_the_big_grids(name, spec):
    case = limits.CASES[name]
    cin, cout, subm, k, s, p = spec
    layer = cases.make_layer(cin, cout, subm, k, s, p, seed=cin + cout).double()
    feats = cases.features(case, cin, seed=3)
    count = None if case.count is None else torch.tensor([case.count], dtype=torch.int32)
    x = sparse3d.SparseTensor3d(feats.double(), case.indices, case.shape, case.batch, count, torch.zeros(1, dtype=torch.int32))
    assert layer[0].kernel_reason(x) is not None                                                    # CPU tensors: the torch-op route
    with torch.no_grad():
        out = layer(x)
    want = limits.check_layer(case, layer, feats, out, out.rows(), lambda got, ref_f, pre, what: _close64(got, ref_f, what), f"{name} {spec}")
    assert want.keys.numel() >= 300


@functools.lru_cache(maxsize=None)
def opv2v_backbone():
    """The backbone and voxels of the OPV2V-grid case and the key-based reference of all its levels, computed once (tests/test_sparse3d_limits_gpu.py shares them)."""
    case = limits.CASES["opv2v_5_agents"]
    bb = sparse3d.VoxelBackBone8x({"num_features_out": 64}, 4, [case.shape[2], case.shape[1], case.shape[0] - 1], site_capacity=4 * case.indices.shape[0])
    bb = cases.seed_backbone_(bb, 5).eval()
    vox = limits.voxels(case, seed=8)
    mean = vox["voxel_features"].double().sum(dim=1) / vox["voxel_num_points"].clamp(min=1).view(-1, 1).double()
    t, levels = ref.key_backbone(bb, mean, vox["voxel_coords"], case.batch)
    assert all(lv.full is None or lv.full <= bb.site_capacity for lv in levels)                    # the capacity cuts nothing here
    return case, bb, vox, t, levels


def test_torch_route_backbone_on_the_opv2v_grid(monkeypatch):
    monkeypatch.setenv("COALIGN_SP3D", "0")
    case, bb, vox, t, levels = opv2v_backbone()
    bb = bb.double()
    try:
        d = {"voxel_features": vox["voxel_features"].double(), "voxel_coords": vox["voxel_coords"], "voxel_num_points": vox["voxel_num_points"], "batch_size": case.batch}
        with torch.no_grad():
            d = sparse3d.HeightCompression({"feature_num": 128})(bb(sparse3d.MeanVFE({}, 4)(d)))
    finally:
        bb.float()
    out = d["encoded_spconv_tensor"]
    assert out.spatial_shape == t.shape == (2, 100, 352) and out.rows() == t.keys.numel() > 100
    assert torch.equal(out.indices.long(), t.coords())
    _close64(out.features, t.feats, "conv_out")
    for name, lv in zip(("x_conv1", "x_conv2", "x_conv3", "x_conv4"), (levels[1], levels[4], levels[7], levels[10])):
        got = d["multi_scale_3d_features"][name]
        assert got.spatial_shape == lv.shape and got.rows() == lv.keys.numel(), name
        if name != "x_conv1":                                                                       # (level 0 keeps the list's shuffled order)
            assert torch.equal(got.indices.long(), lv.coords()), name
            _close64(got.features, lv.feats, name)
    pix, vals = ref.key_height_compression(t)
    m = d["spatial_features"]
    assert tuple(m.shape) == (5, 128, 100, 352)
    _close64(m[pix[:, 0], :, pix[:, 1], pix[:, 2]], vals, "map")
    assert int(torch.count_nonzero(m.abs().amax(dim=1))) <= pix.shape[0]
