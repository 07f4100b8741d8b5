"""The sparse 3-D trunk's kernels on the MI355X (include_ext/coalign_amd_sparse3d.h, csrc/sparse_conv3d.hip): every layer combination on every case of
tests/sparse3d_cases.py against the dense float64 restatement -- sites and order exact, the device count the reference's, values within ``assert_elementwise``'s
defaults (rtol 1e-4, floor 1e-5 of the scale) --, the whole backbone + to-dense, determinism, graph replay onto another site set, an empty agent, the model against
its torch-op route, and stage 1 downstream of it."""
import functools

import pytest
import torch

import sparse3d_cases as cases
import sparse3d_reference as ref
from conftest import assert_elementwise
from coalign_amd import ops, sparse3d
from coalign_amd.config import builtin_config
from coalign_amd.detector import build_model, to_device
from coalign_amd.postprocess import build_postprocessor

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
BACKBONE_SHAPE = (41, 64, 64)                                  # grid_size (64, 64, 40)


@pytest.fixture(autouse=True)
def _kernel_route(monkeypatch):
    monkeypatch.setenv("COALIGN_SP3D", "1")


def _on_device(case, feats):
    count = None if case.count is None else torch.tensor([case.count], dtype=torch.int32, device=DEV)
    return sparse3d.SparseTensor3d(feats.to(DEV), case.indices.to(DEV), case.shape, case.batch, count, torch.zeros(1, dtype=torch.int32, device=DEV))


@pytest.mark.parametrize("group", cases.GROUPS)
@pytest.mark.parametrize("combo", cases.COMBOS, ids=lambda c: f"{c[0]}_{c[1]}_k{''.join(map(str, sparse3d._triple(c[2])))}")
def test_kernel_route_equals_the_dense_reference(combo, group):
    cin, cout, kernel = combo
    for case in cases.of_group(group):
        for subm, k, s, p in cases.geometries(case, kernel):
            layer = cases.make_layer(cin, cout, subm, k, s, p, seed=cin + cout, site_capacity=case.site_capacity).to(DEV)
            feats = cases.features(case, cin, seed=3)
            x = _on_device(case, feats)
            assert layer[0].kernel_reason(x) is None
            with torch.no_grad():
                out = layer(x)
            assert out.count is not None and out.count.is_cuda                       # the count lives on the device
            what = f"{case.name} {'subm' if subm else 'strided'} {k}/{s}/{p}"
            rows = int(out.count.item())
            dense, _ = cases.check(case, layer, feats, out, rows, assert_elementwise, what)
            if group == "to_dense":
                want = ref.height_compression(dense)
                poisoned = torch.full(want.shape, float("nan"), device=DEV).contiguous(memory_format=torch.channels_last)
                got = ops.sp3d_to_dense(out.features, out.count, out._index, out.batch_size, out.spatial_shape, out=poisoned)
                assert got is poisoned and not bool(torch.isnan(got).any()), what   # every element written
                if rows == 0:
                    assert not bool(got.any()), what
                else:
                    assert_elementwise(got, want, what + " dense")
                i = out.indices[:rows].long()
                D = out.spatial_shape[0]
                for r in range(min(rows, 5)):                                       # channel c D + d, spelled out
                    b, z, y, xx = (int(v) for v in i[r])
                    assert torch.equal(got[b, z::D, y, xx], out.features[r]), what


@functools.lru_cache(maxsize=None)
def _backbone(seed=5):
    bb = sparse3d.VoxelBackBone8x({"num_features_out": 64}, 4, [BACKBONE_SHAPE[2], BACKBONE_SHAPE[1], BACKBONE_SHAPE[0] - 1])
    return cases.seed_backbone_(bb, seed).eval().to(DEV)


def _trunk(bb, vox, batch):
    """MeanVFE -> backbone -> HeightCompression on the device -> (map, the backbone's output tensor)."""
    d = {k: v.to(DEV) for k, v in vox.items()}
    d["batch_size"] = batch
    with torch.no_grad():
        d = sparse3d.HeightCompression({"feature_num": 128})(bb(sparse3d.MeanVFE({}, 4)(d)))
    return d["spatial_features"], d["encoded_spconv_tensor"]


def _trunk_reference(bb, vox, batch):
    mean = vox["voxel_features"].double().sum(dim=1) / vox["voxel_num_points"].clamp(min=1).view(-1, 1).double()
    dense, mask = ref.backbone(bb, mean, vox["voxel_coords"], batch)
    return ref.height_compression(dense), ref.sites(mask)


def test_whole_backbone_and_to_dense():
    bb = _backbone()
    vox = cases.voxels(BACKBONE_SHAPE, 2, seed=6)
    want, want_sites = _trunk_reference(bb, vox, 2)
    got, t = _trunk(bb, vox, 2)
    assert all(m.kernel_reason() is None for _, m in bb.sparse_convs())
    assert tuple(got.shape) == (2, 128, 8, 8) == tuple(want.shape) and got.is_contiguous(memory_format=torch.channels_last)
    rows = int(t.count.item())
    assert rows == want_sites.shape[0] > 50 and torch.equal(t.indices[:rows].cpu(), want_sites)
    assert int(bb.last_status.item()) == 0
    worst = assert_elementwise(got, want, "backbone + to-dense")
    print(f"backbone (41, 64, 64) x 2: {vox['voxel_coords'].shape[0]} voxels -> {rows} sites, worst {worst:.3e} of the scale")
    again, _ = _trunk(bb, vox, 2)                                                    # determinism: no atomics on floats, a fixed tap order
    assert torch.equal(again, got)


def test_an_empty_agent_among_full_ones():
    bb = _backbone()
    vox = cases.voxels(BACKBONE_SHAPE, 3, seed=7, empty=(1,))
    assert not bool((vox["voxel_coords"][:, 0] == 1).any())
    want, _ = _trunk_reference(bb, vox, 3)
    got, _ = _trunk(bb, vox, 3)
    assert not bool(got[1].any()) and bool(got[0].any()) and bool(got[2].any())
    assert_elementwise(got, want, "empty agent")


def test_graph_replay_onto_another_site_set():
    """One capture, replayed onto same-shape buffers that hold a DIFFERENT site set: counts are read on the device, so the replay equals the eager run bit for bit."""
    bb = _backbone()
    a, b = cases.voxels(BACKBONE_SHAPE, 2, seed=8), cases.voxels(BACKBONE_SHAPE, 2, seed=9)
    M = min(a["voxel_coords"].shape[0], b["voxel_coords"].shape[0])
    a, b = {k: v[:M] for k, v in a.items()}, {k: v[:M] for k, v in b.items()}
    assert not torch.equal(a["voxel_coords"], b["voxel_coords"])
    eager_a, eager_b = _trunk(bb, a, 2)[0].clone(), _trunk(bb, b, 2)[0].clone()
    assert not torch.equal(eager_a, eager_b)
    static = {k: v.to(DEV).clone() for k, v in a.items()}
    static["batch_size"] = 2

    def body():
        d = dict(static)
        with torch.no_grad():
            return sparse3d.HeightCompression({"feature_num": 128})(bb(sparse3d.MeanVFE({}, 4)(d)))["spatial_features"]

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        body()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = body()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager_a)
    for k in ("voxel_features", "voxel_coords", "voxel_num_points"):
        static[k].copy_(b[k].to(DEV))
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager_b)


@functools.lru_cache(maxsize=None)
def _mini_model():
    h = builtin_config("second/mini_second_uncertainty")
    model = cases.seed_backbone_(build_model(h), 2).eval().to(DEV)
    vox = cases.voxels(model.spconv_block.sparse_shape, 2, seed=4)
    return h, model, vox


def test_model_kernel_route_equals_its_torch_route(monkeypatch):
    _, model, vox = _mini_model()
    data = to_device({"processed_lidar": vox, "record_len": torch.tensor([2])}, DEV)
    with torch.no_grad():
        got = model(data)
        monkeypatch.setenv("COALIGN_SP3D", "0")
        assert all(m.kernel_reason() == "COALIGN_SP3D=0" for _, m in model.spconv_block.sparse_convs())
        want = model(data)
    assert set(got) == {"cls_preds", "reg_preds", "unc_preds", "dir_preds"}
    for k in got:
        assert tuple(got[k].shape[2:]) == (16, 32)
        assert_elementwise(got[k], want[k], f"model {k}")


def test_stage1_downstream_of_the_second_model():
    """The model's head maps through ``post_process_stage1_device``: the store's kept boxes equal ``post_process_stage1``'s lists."""
    import test_stage1_batched_gpu as s1
    h, model, vox = _mini_model()
    pp = build_postprocessor(h["postprocess"], False)
    anchors = pp.generate_anchor_box()
    a1 = torch.from_numpy(anchors)
    assert anchors.shape[:3] == (16, 32, 2)
    data = to_device({"processed_lidar": vox, "record_len": torch.tensor([2])}, DEV)
    saved = (model.cls_head.weight.clone(), model.cls_head.bias.clone())
    with torch.no_grad():
        try:
            model.cls_head.weight.mul_(30.0)                                         # (xavier with gain 0.1 leaves the logits within 1e-2 of each other)
            v = torch.unique(model(data)["cls_preds"]).flip(0)                       # distinct logits, descending: the cells of empty regions tie
            model.cls_head.bias.add_(-1.386 - float(v[19] + v[20]) / 2)              # the 20 highest distinct logits pass the score threshold of 0.2 (logit -1.386)
            heads = model(data)
        finally:
            model.cls_head.weight.copy_(saved[0])
            model.cls_head.bias.copy_(saved[1])
    assert 0 < int((heads["cls_preds"] > -1.386).sum()) < 200
    ref_c, ref_u = s1._reference(pp, heads, a1)
    assert sum(len(c) for c in ref_c) > 0
    store = ops.Stage1Store(DEV, 3)
    s1._poison(store)
    assert pp.post_process_stage1_device(heads, a1, store) is store and store.n_agents == 2
    s1._check(store, ref_c, ref_u, "SecondSSFAUncertainty -> post_process_stage1_device")
