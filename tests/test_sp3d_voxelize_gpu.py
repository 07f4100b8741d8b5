"""Raw clouds -> the sparse trunk's input tensor on the MI355X: ``coalign_sp3d_voxelize`` (``ops.sp3d_voxelize`` / ``sparse3d.voxel_sites``) on every case of
tests/sp3d_voxelize_cases.py against the oracle's chain -- features, indices, count, cloud counts and status bits exactly --, the emitted site index against
``ops.sp3d_index_build``, the OPV2V grid that ``ops.voxelize`` refuses, one captured graph replayed on another frame, and the SECOND model from ``voxel_sites`` against
the same model from the oracle's ``processed_lidar``."""
import numpy as np
import pytest
import torch

import sp3d_voxelize_cases as cases
import sparse3d_cases
from coalign_amd import hip, ops, second, sparse3d
from coalign_amd.config import builtin_config
from coalign_amd.detector import build_model, to_device

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


@pytest.fixture(autouse=True)
def _kernel_route(monkeypatch):
    monkeypatch.setenv("COALIGN_SP3D", "1")


def _index_agrees(got):
    """``sp3d_neighbors`` and ``sp3d_to_dense`` on the emitted index equal those on ``sp3d_index_build(indices, count)``."""
    n, shape, cap = got.batch_size, got.spatial_shape, got.capacity
    rows = int(got.count.cpu()[0])
    built = ops.sp3d_index_build(got.indices, got.count, n, shape)
    assert got._index.numel() == built.numel() == ops.sp3d_index_bytes(n, shape, cap)
    a = ops.sp3d_neighbors(got.indices, got.count, n, shape, got._index, cap, shape, 3, 1, 1)
    b = ops.sp3d_neighbors(got.indices, got.count, n, shape, built, cap, shape, 3, 1, 1)
    assert torch.equal(a[:, :rows], b[:, :rows])
    assert rows == 0 or bool((a[13, :rows] == torch.arange(rows, device=DEV, dtype=torch.int32)).all())          # the centre tap of a site is its own row: rank = row
    feats = torch.where(torch.arange(cap, device=DEV).unsqueeze(1) < rows, got.features, torch.full_like(got.features, float("nan")))
    da, db = ops.sp3d_to_dense(feats, got.count, got._index, n, shape), ops.sp3d_to_dense(feats, got.count, built, n, shape)
    assert torch.equal(da.view(torch.int32), db.view(torch.int32)) and not bool(torch.isnan(da).any())
    return da


@pytest.mark.parametrize("name", cases.TINY)
def test_kernels_equal_the_oracle_on_the_tiny_grid(name):
    case = cases.CASES[name]
    got = cases.sites(case, device=DEV)
    assert got._index is not None and got.features.is_cuda
    want = cases.check(case, got)
    dense = _index_agrees(got)
    assert int((dense != 0).any(dim=1).sum()) <= len(want.features)
    if name == "all_invalid":
        assert int(got.count.cpu()[0]) == 0 and not bool(dense.any())
    again = cases.sites(case, device=DEV)                                                  # two eager runs: the same bits
    rows = int(got.count.cpu()[0])
    assert torch.equal(again.features[:rows].view(torch.int32), got.features[:rows].view(torch.int32)) and torch.equal(again.indices[:rows], got.indices[:rows])


@pytest.mark.parametrize("name", ["point_order", "max_voxels", "every_cell", "sixteen_clouds"])
def test_capacity_cut_keeps_the_first_rows(name):
    case = cases.CASES[name]
    kept = len(cases.reference(name).features)
    below = cases.sites(case, kept - 1, device=DEV)
    cases.check(case, below, kept - 1)
    _index_agrees(below)
    exact = cases.sites(case, kept, device=DEV)
    cases.check(case, exact, kept)
    _index_agrees(exact)


def test_the_grid_the_dense_voxeliser_refuses():
    case = cases.CASES["opv2v_grid"]
    got = cases.sites(case, device=DEV)
    want = cases.check(case, got)
    assert 6000 < len(want.features) and tuple(got.spatial_shape) == (41, 800, 2816)
    pts, off = cases.concatenated(case)
    with pytest.raises((ValueError, hip.CoalignHipError)):
        ops.voxelize(torch.from_numpy(pts).to(DEV), off.tolist(), case.voxel_size, case.lidar_range, 5, 70000)


def test_offsets_are_read_on_the_device_and_clamped():
    case = cases.CASES["point_order"]
    pts, off = cases.concatenated(case)
    n0 = int(off[1])
    for offsets in ([0, n0, n0 - 5, len(pts) + 9], [-3, n0, 1 << 30], [4, n0, len(pts) - 2]):
        args = (case.voxel_size, case.lidar_range, case.shape, case.max_points, case.max_voxels, len(pts))
        got = sparse3d.voxel_sites(torch.from_numpy(pts).to(DEV), torch.tensor(offsets, dtype=torch.int32, device=DEV), *args)
        want = sparse3d._voxel_sites_torch(torch.from_numpy(pts), torch.tensor(offsets, dtype=torch.int32), *args, False, None)
        n = int(want[2])
        assert int(got.count.cpu()[0]) == n and torch.equal(got.indices[:n].cpu(), want[1][:n]) and torch.equal(got.features[:n].cpu(), want[0][:n])
        assert torch.equal(got.cloud_counts.cpu(), want[3])


def test_graph_replay_on_another_frame():
    """One capture at P_cap; the replay sees other points and other offsets and equals the eager call on that frame, bit for bit."""
    a, b = cases.CASES["point_order"], cases.CASES["empty_first_middle_last"]
    pa, oa = cases.concatenated(a)
    b_clouds = b.clouds[1:3] if len(b.clouds) != 2 else b.clouds                       # two clouds, as the capture has: [small, empty]
    pb = np.concatenate(b_clouds).astype(np.float32)
    ob = np.asarray([0, len(b_clouds[0]), len(pb)], dtype=np.int32)
    P_cap = len(pa) + 37
    args = (a.voxel_size, a.lidar_range, a.shape, a.max_points, a.max_voxels, P_cap)
    points = torch.full((P_cap, 4), 0.55, device=DEV)                                  # the slack past offsets[-1] holds VALID points: they belong to no cloud
    offsets = torch.zeros(3, dtype=torch.int32, device=DEV)

    def load(p, o):
        points[: len(p)].copy_(torch.from_numpy(p))
        points[len(p):] = 0.55
        offsets.copy_(torch.from_numpy(o))

    def eager():
        x = sparse3d.voxel_sites(points, offsets, *args)
        return x.features.clone(), x.indices.clone(), x.count.clone(), x.cloud_counts.clone(), x.status.clone()

    load(pa, oa)
    eager_a = eager()
    load(pb, ob)
    eager_b = eager()
    assert int(eager_a[2]) == 9 and int(eager_b[2]) == 3
    load(pa, oa)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        sparse3d.voxel_sites(points, offsets, *args)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = sparse3d.voxel_sites(points, offsets, *args)
    for frame, want in ((None, eager_a), ((pb, ob), eager_b), ((pa, oa), eager_a)):
        if frame is not None:
            load(*frame)
        out.status.zero_()
        graph.replay()
        torch.cuda.synchronize()
        n = int(want[2])
        assert int(out.count) == n and torch.equal(out.indices[:n], want[1][:n]) and torch.equal(out.features[:n].view(torch.int32), want[0][:n].view(torch.int32))
        assert torch.equal(out.cloud_counts, want[3]) and torch.equal(out.status, want[4])
        dense = ops.sp3d_to_dense(out.features, out.count, out._index, 2, a.shape)
        assert int((dense != 0).any(dim=1).sum()) > 0


@pytest.mark.parametrize("ssfa", ["0", "1"])
def test_model_from_voxel_sites_equals_the_model_from_the_oracles_voxels(ssfa, monkeypatch):
    """``mini_second_uncertainty`` on the kernels: the dense map and the head maps from ``voxel_sites`` are those from the oracle's ``processed_lidar``, bit for bit --
    ``sp3d_conv`` adds taps per output row in a fixed order and a skipped tap adds zeros, so the row order cannot show.  With the neck on torch ops (``COALIGN_SSFA=0``)
    MIOpen's 3 x 3 convolutions are asked for their deterministic solvers: by default the SAME map through the SAME ``nn.Conv2d`` twice differs in the last bit
    (measured: 3e-8 per layer, 6e-8 behind the neck, 4e-9 in the head maps, equal dense maps in front), which no input can be held to."""
    monkeypatch.setenv("COALIGN_SSFA", ssfa)
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)
    model = sparse3d_cases.seed_backbone_(build_model(builtin_config("second/mini_second_uncertainty")), 2).eval().to(DEV)
    clouds = cases.model_clouds(model, 5)
    host = to_device({"processed_lidar": cases.oracle_lidar(model, clouds), "record_len": torch.tensor([2])}, DEV)
    sites = second.lidar_from_points(model, clouds, capacity=4096)
    assert sites["voxel_sites"]._index is not None and sites["voxel_sites"].features.is_cuda
    assert int(sites["voxel_counts"][-1]) == host["processed_lidar"]["voxel_coords"].shape[0] <= 4096
    with torch.no_grad():
        want_bev, want = model.bev_features(host), model(host)
        monkeypatch.setattr(second, "_batch_size", lambda *a, **k: pytest.fail("_batch_size was called"))
        got_bev, got = model.bev_features({"processed_lidar": sites}), model({"processed_lidar": sites})
    assert float(want_bev.abs().max()) > 0 and torch.equal(got_bev, want_bev)
    assert set(got) == set(want) == {"cls_preds", "reg_preds", "unc_preds", "dir_preds"}
    for k in want:
        assert torch.equal(got[k], want[k]), k
