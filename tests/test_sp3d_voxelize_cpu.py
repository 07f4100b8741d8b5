"""Raw clouds -> the sparse trunk's input tensor, without a GPU: the torch-op route of ``sparse3d.voxel_sites`` on every case of tests/sp3d_voxelize_cases.py against the
oracle's chain (exactly), every refusal of ``coalign_sp3d_voxelize`` before the first HIP call, the new header against its table and the library, and the SECOND model
on the CPU reading ``voxel_sites`` against the same model reading the oracle's ``processed_lidar``."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import sp3d_voxelize_cases as cases
import sparse3d_cases
from coalign_amd import build, hip, ops, preprocess, second, sparse3d
from coalign_amd.config import builtin_config
from coalign_amd.detector import build_model
from oracle import coalign_oracle as oracle

NULL, ONE = ctypes.c_void_p(0), ctypes.c_void_p(4096)      # (never dereferenced: every refusal below comes before the first HIP call)
HEADER = "coalign_amd_sp3d_voxelize.h"
CITES = ("sp_voxel_preprocessor.py:62-147", "mean_vfe.py:26-30", "pcd_utils.py:41-88")


# ---- the reference itself ----------------------------------------------------------------------------------------------------------------------------------------
def test_the_cases_hold_what_they_name():
    w = cases.reference("point_order")
    assert len(w.features) == 6 + 3 and w.cloud_counts.tolist() == [6, 3, 9]
    c = cases.CASES["point_order"]
    v, co, n = oracle.points_to_voxel(c.clouds[0], c.voxel_size, c.lidar_range, c.max_points, c.max_voxels)
    assert sorted(n.tolist()) == [1, 2, 5, 5, 5, 5]
    v2, co2, n2 = oracle.points_to_voxel_python(c.clouds[0], c.voxel_size, c.lidar_range, c.max_points, c.max_voxels)
    assert np.array_equal(v, v2) and np.array_equal(co, co2) and np.array_equal(n, n2)
    assert cases.reference("max_voxels").cloud_counts.tolist() == [6, 4, 10] and cases.reference("max_voxels").reached
    assert cases.reference("max_voxels_exactly").cloud_counts.tolist() == [9, 4, 13] and cases.reference("max_voxels_exactly").reached
    assert cases.reference("max_voxels_1").cloud_counts.tolist() == [1, 1, 2]
    assert cases.reference("all_invalid").cloud_counts.tolist() == [0, 0, 0]
    assert cases.reference("every_cell").cloud_counts.tolist() == [1920, 1920, 3840] and not cases.reference("every_cell").reached
    assert cases.reference("empty_first_middle_last").cloud_counts.tolist() == [0, 3, 0, 3, 0, 6]
    e, ee, er = cases.reference("edges"), cases.reference("edges_ego"), cases.reference("edges_range")
    assert 0 < len(ee.features) < len(e.features) and 0 < len(er.features) < len(e.features)
    big = cases.reference("opv2v_grid")
    assert 6000 < len(big.features) < 7013 and (big.indices[:, 1:] < np.asarray(cases.OPV2V_SHAPE)).all()
    for name in cases.CASES:
        idx = cases.reference(name).indices
        assert (np.diff(cases.linear_cell(idx, cases.CASES[name].shape)) > 0).all(), name


# ---- the torch-op route ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(cases.CASES))
def test_torch_route_equals_the_oracle(name):
    case = cases.CASES[name]
    got = cases.sites(case)
    assert got._index is None
    cases.check(case, got)


@pytest.mark.parametrize("name", ["point_order", "max_voxels", "every_cell"])
def test_torch_route_capacity(name):
    case = cases.CASES[name]
    kept = len(cases.reference(name).features)
    cases.check(case, cases.sites(case, kept - 1), kept - 1)
    cases.check(case, cases.sites(case, kept), kept)


def test_torch_route_offsets_are_clamped_and_a_decreasing_pair_is_an_empty_cloud():
    case = cases.CASES["point_order"]
    pts, off = cases.concatenated(case)
    n0 = int(off[1])
    for offsets, clouds in (([0, n0, n0 - 5, len(pts) + 9], [pts[:n0], pts[:0], pts[n0:]]), ([-3, n0, 1 << 30], [pts[:n0], pts[n0:]]), ([4, n0, len(pts) - 2], [pts[4:n0], pts[n0:-2]])):
        got = sparse3d.voxel_sites(torch.from_numpy(pts), torch.tensor(offsets, dtype=torch.int32), case.voxel_size, case.lidar_range, case.shape, case.max_points,
                                   case.max_voxels, len(pts))
        want = sparse3d.voxel_sites(torch.from_numpy(np.concatenate(clouds)), torch.tensor(np.concatenate([[0], np.cumsum([len(c) for c in clouds])]), dtype=torch.int32),
                                    case.voxel_size, case.lidar_range, case.shape, case.max_points, case.max_voxels, len(pts))
        n = int(want.count)
        assert int(got.count) == n and torch.equal(got.indices[:n], want.indices[:n]) and torch.equal(got.features[:n], want.features[:n])
        assert torch.equal(got.cloud_counts, want.cloud_counts)


def test_voxel_sites_refuses_a_shape_that_does_not_hold_the_grid():
    case = cases.CASES["point_order"]
    pts, off = cases.concatenated(case)
    for shape in ((9, 12, 19), (9, 11, 20), (7, 12, 20)):
        with pytest.raises(ValueError):
            sparse3d.voxel_sites(torch.from_numpy(pts), torch.from_numpy(off), case.voxel_size, case.lidar_range, shape, 5, 100, 100)
    assert int(sparse3d.voxel_sites(torch.from_numpy(pts), torch.from_numpy(off), case.voxel_size, case.lidar_range, (8, 12, 20), 5, 100, 100).count) == 9


def test_route_text(monkeypatch):
    monkeypatch.delenv("COALIGN_SP3D", raising=False)
    assert sparse3d.voxel_sites_route_text() == (sparse3d.VOXEL_SITES_KERNEL_TEXT if sparse3d.VOXEL_SITES_KERNEL_DEFAULT else sparse3d.voxel_sites_route_text())
    monkeypatch.setenv("COALIGN_SP3D", "1")
    assert sparse3d.voxel_sites_route_text() == sparse3d.VOXEL_SITES_KERNEL_TEXT and "coalign_sp3d_voxelize" in sparse3d.VOXEL_SITES_KERNEL_TEXT
    monkeypatch.setenv("COALIGN_SP3D", "0")
    assert sparse3d.voxel_sites_route_text() == f"{sparse3d.VOXEL_SITES_TORCH_TEXT} (COALIGN_SP3D=0)"
    hypes = builtin_config("second/opv2v_second_uncertainty")
    assert list(sparse3d.plan(hypes))[0] == "vfe" and "voxel_sites" not in sparse3d.plan(hypes) and not any("voxel" in k for k in second.plan(hypes))


# ---- the ABI -----------------------------------------------------------------------------------------------------------------------------------------------------
def test_header_table_and_library_agree():
    assert HEADER in build.OPEN_HEADERS and list(hip.OPEN_HEADERS) == list(build.OPEN_HEADERS) and hip.OPEN_HEADERS[HEADER] is hip.SP3D_VOXELIZE_SIGNATURES
    assert sorted(os.listdir(build.OPEN_INCLUDE)) == sorted(build.OPEN_HEADERS)
    src = open(os.path.join(build.OPEN_INCLUDE, HEADER)).read()
    text = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", src, flags=re.S))
    assert '#include "coalign_amd.h"' in text
    assert set(re.findall(r"\b(coalign_[a-z0-9_]+)\s*\(", text)) == set(hip.SP3D_VOXELIZE_SIGNATURES) == {"coalign_sp3d_voxelize_workspace_bytes", "coalign_sp3d_voxelize"}
    lib = hip.lib()
    assert lib.coalign_abi_version() == 2
    comments = re.findall(r"/\*.*?\*/", src, flags=re.S)
    for name, (res, args) in hip.SP3D_VOXELIZE_SIGNATURES.items():
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == args, name
        last = [c for c in comments if c in src[:src.index(name + "(")]][-1]
        assert CITES[0] in last, name
    last = [c for c in comments if c in src[:src.index("coalign_sp3d_voxelize(")]][-1]
    assert all(c in last for c in CITES)
    assert "ASCENDING LINEAR CELL INDEX" in src and "REFUSED" in src                     # the header says the row order and what an empty call gets
    assert int(re.search(r"#define COALIGN_SP3D_STATUS_MAX_VOXELS (\d+)u", src).group(1)) == ops.SP3D_STATUS_MAX_VOXELS == 2 != ops.SP3D_STATUS_OVERFLOW
    assert int(re.search(r"#define COALIGN_SP3D_VOXELIZE_MAX_POINTS (\d+)", src).group(1)) == ops.SP3D_VOXELIZE_MAX_POINTS >= 8
    assert int(re.search(r"#define COALIGN_SP3D_VOXELIZE_MAX_CLOUDS (\d+)", src).group(1)) == ops.SP3D_VOXELIZE_MAX_CLOUDS == 16
    kernel = open(os.path.join(build.CSRC, "sparse_conv3d.hip")).read()
    assert "getenv" not in kernel and len(re.findall(r"\bstruct Index\b", kernel)) == 1
    for k in ("sp3d_block_sums", "sp3d_scan_sums", "sp3d_word_prefix", "sp3d_mark", "vox_mark", "vox_first", "vox_round", "vox_head_count", "vox_cut", "vox_emit"):
        assert len(re.findall(r"__global__[^\n]*\bvoid " + k + r"\(", kernel)) == 1, k          # the site-index kernels exist once
    assert not re.search(r"atomic(Add|Min|Max)\s*\(\s*\(?\s*float", kernel)


def test_entry_point_refuses_before_any_hip_call():
    L = hip.lib()
    vs, rg, fr = (ctypes.c_double * 3)(0.1, 0.1, 0.1), (ctypes.c_double * 6)(0, 0, 0, 2.0, 1.2, 0.8), (ctypes.c_double * 6)(0, 0, 0, 1, 1, 1)
    big = 1 << 40

    def vx(points=ONE, offsets=ONE, P=100, n=2, vs=vs, rg=rg, D=9, H=12, W=20, T=5, mv=10, flags=0, fr=None, feat=ONE, idx=ONE, count=ONE, cc=ONE, cap=50, index=ONE,
           ib=big, status=ONE, ws=ONE, wb=big):
        return L.coalign_sp3d_voxelize(points, offsets, P, n, vs, rg, D, H, W, T, mv, flags, fr, feat, idx, count, cc, cap, index, ib, status, ws, wb, NULL)

    for kw in (dict(P=0), dict(P=-1), dict(P=(1 << 27) + 1), dict(cap=0), dict(cap=-4), dict(n=0), dict(mv=0), dict(T=0), dict(W=19), dict(H=13), dict(D=7),
               dict(rg=(ctypes.c_double * 6)(0, 0, 0, 0.04, 1.2, 0.8), W=1), dict(rg=(ctypes.c_double * 6)(0, 0, 0, 2.0, 1.2, 7000.0), D=70001),
               dict(rg=(ctypes.c_double * 6)(-140.8, -40, -3, 140.8, 40, 1), D=64, H=800, W=2816, n=16), dict(vs=(ctypes.c_double * 3)(0.1, 0.0, 0.1)),
               dict(vs=(ctypes.c_double * 3)(0.1, float("nan"), 0.1))):
        assert vx(**kw) == -2, kw
    for kw in (dict(n=17), dict(T=9), dict(T=64), dict(flags=4), dict(flags=-1)):
        assert vx(**kw) == -3, kw
    assert vx(T=8, n=16, D=8, points=NULL) == -1 and vx(T=1, n=1, mv=1, cap=1, P=1, status=NULL) == -1      # (the limits themselves pass the shape and support checks)
    index_need = L.coalign_sp3d_index_workspace_bytes(2, 9, 12, 20, 50)
    ws_need = L.coalign_sp3d_voxelize_workspace_bytes(100, 2, 5)
    assert index_need > 0 and ws_need >= (2 + 5) * 100 * 4
    assert vx(ib=index_need - 1) == -4 and vx(wb=ws_need - 1) == -4 and vx(ib=0) == -4 and vx(wb=0) == -4
    for kw in (dict(points=NULL), dict(offsets=NULL), dict(vs=None), dict(rg=None), dict(feat=NULL), dict(idx=NULL), dict(count=NULL), dict(cc=NULL), dict(index=NULL),
               dict(status=NULL), dict(ws=NULL), dict(flags=2), dict(points=ctypes.c_void_p(4104)), dict(feat=ctypes.c_void_p(4100)), dict(idx=ctypes.c_void_p(4104)),
               dict(index=ctypes.c_void_p(4112 - 8)), dict(ws=ctypes.c_void_p(4100)), dict(offsets=ctypes.c_void_p(4098)), dict(count=ctypes.c_void_p(4097)),
               dict(cc=ctypes.c_void_p(4098)), dict(status=ctypes.c_void_p(4099))):
        assert vx(**kw) == -1, kw
    assert vx(flags=2, fr=fr, points=NULL) == -1 and vx(flags=3, fr=fr, ib=0) == -4     # (with a filter range the flag passes; the next check answers)
    for args in ((0, 2, 5), (-1, 2, 5), ((1 << 27) + 1, 2, 5), (100, 0, 5), (100, 17, 5), (100, 2, 0), (100, 2, 9)):
        assert L.coalign_sp3d_voxelize_workspace_bytes(*args) == 0, args
    assert L.coalign_sp3d_voxelize_workspace_bytes(1, 1, 1) > 0 and L.coalign_sp3d_voxelize_workspace_bytes(1 << 27, 16, 8) > (1 << 27) * 40
    with pytest.raises(hip.CoalignHipError):
        ops.sp3d_voxelize(torch.zeros(4, 4), torch.tensor([0, 4], dtype=torch.int32), (0.1, 0.1, 0.1), (0, 0, 0, 2.0, 1.2, 0.8), (9, 12, 20), 5, 10, 4)


# ---- the model ---------------------------------------------------------------------------------------------------------------------------------------------------
def test_model_from_voxel_sites_equals_the_model_from_the_oracles_voxels(monkeypatch):
    """``mini_second_uncertainty`` on the CPU: ``voxel_sites`` from the clouds and the oracle's ``processed_lidar`` from the same clouds give the same dense map and
    the same head maps.  ``_batch_size`` is not asked when the sites come with their own batch size."""
    model = sparse3d_cases.seed_backbone_(build_model(builtin_config("second/mini_second_uncertainty")), 2).eval()
    clouds = cases.model_clouds(model, 5)
    host = cases.oracle_lidar(model, clouds)
    assert host["voxel_coords"].shape[0] > 1000 and int(host["voxel_num_points"].max()) > 1
    sites = second.lidar_from_points(model, clouds, device="cpu")
    assert set(sites) == {"voxel_sites", "voxel_counts"} and isinstance(sites["voxel_sites"], sparse3d.SparseTensor3d)
    assert sites["voxel_sites"].capacity == 2 * 70000 and tuple(sites["voxel_sites"].spatial_shape) == tuple(model.spconv_block.sparse_shape)
    assert int(sites["voxel_counts"][-1]) == host["voxel_coords"].shape[0] == int(sites["voxel_sites"].count)
    by_hypes = second.lidar_from_points(builtin_config("second/mini_second_uncertainty"), clouds, device="cpu")
    assert torch.equal(by_hypes["voxel_sites"].indices, sites["voxel_sites"].indices) and torch.equal(by_hypes["voxel_sites"].features, sites["voxel_sites"].features)
    with torch.no_grad():
        want_bev = model.bev_features({"processed_lidar": host, "record_len": torch.tensor([2])})
        want = model({"processed_lidar": host, "record_len": torch.tensor([2])})
        monkeypatch.setattr(second, "_batch_size", lambda *a, **k: pytest.fail("_batch_size was called"))
        got_bev = model.bev_features({"processed_lidar": sites})
        got = model({"processed_lidar": sites})
    assert float(want_bev.abs().max()) > 0
    assert torch.equal(got_bev, want_bev)
    assert list(got) == list(want)
    for k in want:
        assert torch.equal(got[k], want[k]), k


def test_preprocess_clouds_keeps_its_refusal_and_gains_the_sites_method():
    h = builtin_config("second/opv2v_second_uncertainty")
    pre = preprocess.SpVoxelPreprocessor(h["preprocess"], False, "cpu")
    clouds = cases.CASES["opv2v_grid"].clouds
    out = pre.preprocess_clouds_sites(clouds, capacity=8000)
    assert out["voxel_sites"].capacity == 8000 and tuple(out["voxel_sites"].spatial_shape) == cases.OPV2V_SHAPE
    want = cases.reference("opv2v_grid")
    n = int(out["voxel_sites"].count)
    assert n == len(want.features) and torch.equal(out["voxel_sites"].indices[:n], torch.from_numpy(want.indices.copy()))
    assert torch.equal(out["voxel_counts"], torch.from_numpy(want.cloud_counts.copy()))
    assert hip.lib().coalign_voxelize_capacity(7013, 2, (ctypes.c_double * 3)(*cases.OPV2V_VOXEL), (ctypes.c_double * 6)(*cases.OPV2V_RANGE), 70000) == -1      # the dense voxeliser refuses this grid, as before
