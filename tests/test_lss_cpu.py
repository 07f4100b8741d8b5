"""Lift-Splat's frustum pooling and the camera model, host side (no GPU): the float64 restatement of tests/lss_reference.py against the fixture made from the
reference (tests/golden/make_lss_golden.py), ``LiftSplat``'s torch routes against the restatement, the properties of the inverted index, the extension header
include/coalign_amd_lss.h against the product library and ``hip.LSS_SIGNATURES``, argument refusals before any HIP call, the switch, the yaml parser and
``build_model`` of the camera configs with a forward through the torch route."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import abi_headers
from conftest import assert_elementwise
from coalign_amd import build, hip, lss, ops
from coalign_amd.config import YAML_PARSERS, builtin_config
from coalign_amd.detector import CAMERA_REGISTRY, MODEL_REGISTRY, build_model
from coalign_amd.synthetic import fill_parameters_, make_camera_frame
import lss_reference as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NULL, ONE, TWO = ctypes.c_void_p(0), ctypes.c_void_p(16), ctypes.c_void_p(1 << 20)      # (non-NULL, aligned tokens: none of these calls gets as far as touching memory)
HEADER = "coalign_amd_lss.h"
NAMES = {"coalign_lss_cells", "coalign_lss_depth_prob", "coalign_lss_pool"}
NZ1 = ((-4.0, 4.8, 0.4), (-3.2, 3.2, 0.4), (-10, 10, 20.0), (2, 12, 6))


# ---- the restatement against the reference ------------------------------------------------------------------------------------------------------------------
def test_restatement_matches_the_reference_fixture(golden):
    """Cells: equal to the reference's float32 cells for every point outside the 1e-3 band around a cell boundary (mismatches printed; 0 on this case).  The
    map: summed in float64 with the fixture's OWN cells, it holds the element-wise bound against ``voxel_pooling``'s output (its cumsum error: ~5e-7 of the scale)."""
    g = golden("lss_pool.npz")
    rig = {k: g[k] for k in R.CAMS}
    lower = g["bx"] - g["dx"] / np.float32(2.0)
    v = R.scaled_coordinates(rig, g["xs"], g["ys"], g["ds"], lower, g["dx"])
    cell = R.cells_f64(v, g["nx"])
    ref_cell = g["cell"].reshape(cell.shape)
    assert np.array_equal(ref_cell >= 0, g["kept"].reshape(cell.shape))
    band = R.near_boundary(v, 1e-3)
    mism = int((cell != ref_cell).sum())
    print(f"float64 / reference cells: {mism} of {cell.size} differ, {int(band.sum())} points inside the 1e-3 band, nearest boundary {R.distance_to_integer(v):.2e}")
    assert np.array_equal(cell[~band], ref_cell[~band]) and float(band.mean()) <= 0.01
    fold = ((v > -1) & (v < 0)).any(-1) & (cell >= 0)
    assert int(fold.sum()) >= 10 and float((cell < 0).mean()) >= 0.10
    pooled = R.pool_f64(g["depth_logit"], g["x_img"], g["cell"], 2, g["nx"])
    err = assert_elementwise(pooled, torch.from_numpy(g["out"]), "float64 sum over the reference's cells vs voxel_pooling")
    print(f"voxel_pooling vs float64: {err:.2e} of the scale")
    # the module's restatements of the reference's helpers give the fixture's constants bit for bit
    sp = R.splat()
    assert sp.nx == [int(k) for k in g["nx"]] == [22, 16, 2]
    assert np.array_equal(sp.dx.numpy(), g["dx"]) and np.array_equal(sp.bx.numpy(), g["bx"]) and np.array_equal(np.float32(sp.lower), lower)
    assert all(np.array_equal(a.numpy(), g[k]) for a, k in zip(sp.axes, ("xs", "ys", "ds")))
    cams = [torch.from_numpy(g[k]) for k in R.CAMS]
    assert_elementwise(sp.get_geometry(*cams), torch.from_numpy(g["geom"]), "get_geometry", rtol=1e-5, floor=1e-6)
    idx, kept = sp.voxel_indices(torch.from_numpy(g["geom"]))
    assert np.array_equal(kept.numpy(), g["kept"])
    assert np.array_equal(sp.cells_float64(*cams).numpy(), cell)


# ---- the module against the restatement --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nz", [1, 2])
def test_torch_routes_against_float64(nz):
    """``forward_torch`` (index_add) and ``forward_reference_ops`` (argsort, cumsum, difference) against the float64 sum over the float64 cells; the rig is one on
    which no point changes its cell between the float32 and the float64 geometry (asserted)."""
    sp, rig, v, cell = R.case(2, 3, 5, None if nz == 2 else NZ1)
    cams = R.rig_tensors(rig)
    assert sp.nx[2] == nz
    idx, kept = sp.voxel_indices(sp.get_geometry(*cams))
    c32 = torch.where(kept, (idx[:, 2] * sp.nx[1] + idx[:, 1]) * sp.nx[0] + idx[:, 0], torch.full_like(idx[:, 0], -1))
    assert np.array_equal(c32.numpy(), cell.reshape(-1))
    logit, x = R.features(6, 8, sp.D, sp.fH, sp.fW, seed=11)
    ref = R.pool_f64(logit, x, cell, 2, sp.nx)
    assert tuple(ref.shape) == (2, nz * 8, 16, 22) and float((ref != 0).double().mean()) > 0.1
    for name in ("forward_torch", "forward_reference_ops", "forward"):
        got = getattr(sp, name)(logit, x, *cams)
        print(f"nz = {nz} {name}: {assert_elementwise(got, ref, name):.2e} of the scale")


def test_channel_order_truncated_nx_and_the_fold():
    sp, rig, v, cell = R.case(2, 3, 5)
    cams = R.rig_tensors(rig)
    logit, x = R.features(6, 8, sp.D, sp.fH, sp.fW, seed=12)
    got = sp.forward_torch(logit, x, *cams)
    ref = R.pool_f64(logit, x, cell, 2, sp.nx)
    assert_elementwise(got, ref, "z C + c")
    swapped = ref.view(2, 2, 8, 16, 22).transpose(1, 2).reshape(2, 16, 16, 22)              # c nz + z
    assert float((got.double() - swapped).abs().max()) > 0.1 * float(ref.abs().max())
    # slice z of the map is channels [z C, (z + 1) C): pooling with the other slice's points dropped leaves it unchanged
    only0 = R.pool_f64(logit, x, np.where(cell < 22 * 16, cell, -1), 2, sp.nx)
    assert torch.equal(only0[:, :8], ref[:, :8]) and float(only0[:, 8:].abs().max()) == 0.0 and float(ref[:, 8:].abs().max()) > 0
    # nx = LongTensor([(hi - lo) / step]) truncates
    assert [int(k) for k in lss.gen_dx_bx([-4.8, 4.8, 0.4], [-3.2, 3.2, 0.4], [-2, 4, 3.0])[2]] == [23, 16, 2]
    assert [int(k) for k in lss.gen_dx_bx([-48, 48, 0.4], [-48, 48, 0.4], [-10, 10, 20.0])[2]] == [240, 240, 1]
    # .long() truncates towards zero: coordinates in (-1, 0) land in index 0 and are kept; with floor they would be dropped
    fold = ((v > -1) & (v < 0)).any(-1) & (cell >= 0)
    assert int(fold.sum()) >= 10
    x_of, y_of = cell % 22, (cell // 22) % 16
    assert bool((((v[..., 0] < 0) & fold) <= (x_of == 0)).all()) and bool((((v[..., 1] < 0) & fold) <= (y_of == 0)).all())
    floored = R.pool_f64(logit, x, np.where(fold, -1, cell), 2, sp.nx)
    assert float((floored - ref).abs().max()) > 0.01 * float(ref.abs().max())
    with pytest.raises(AssertionError):
        assert_elementwise(got, floored)


# ---- the index ------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["golden_grid", "one_cell", "skewed"])
def test_index_properties(which):
    """``order`` is a permutation of the kept points, ascending inside every list; the lists partition the kept points by their cell; the chunks tile every list,
    none longer than 512 points; ``long_cells`` names exactly the lists longer than a chunk; ``points`` addresses the feature row and the probability."""
    if which == "golden_grid":
        sp, rig, v, cell = R.case(2, 3, 5)
    elif which == "one_cell":
        sp, rig, v, cell = R.case(1, 4, 7, ((-100, 100, 200), (-100, 100, 200), (-10, 10, 20.0), (2, 12, 8)))
    A, N = (2, 3) if which == "golden_grid" else (1, 4)
    if which == "skewed":
        cell = R.skewed_cells()
        sp = R.splat(R.grid_conf(*R.GRID_7X5_D8))
        assert sp.nx == [7, 5, 1] and cell.shape == (4, sp.D, sp.fH, sp.fW)
        ix = ops.build_lss_index(torch.from_numpy(cell), A, N, *sp.nx)
    else:
        ix = sp.build_index(*R.rig_tensors(rig))
        assert np.array_equal(sp.cells_float64(*R.rig_tensors(rig)).numpy(), cell)
    nx, ny, nz = sp.nx
    flat = cell.reshape(-1).astype(np.int64)
    kept = np.nonzero(flat >= 0)[0]
    order, starts, points = ix.order.numpy(), ix.starts.numpy().astype(np.int64), ix.points.numpy().astype(np.int64)
    assert np.array_equal(np.sort(order), kept) and len(order) == ix.n_points == starts[-1] and starts[0] == 0 and len(starts) == ix.cells + 1 == A * nx * ny * nz + 1
    assert (np.diff(starts) >= 0).all()
    per_agent = N * sp.D * sp.fH * sp.fW
    c = flat[order]
    key = (((order // per_agent) * ny + (c // nx) % ny) * nx + c % nx) * nz + c // (nx * ny)
    lens = np.diff(starts)
    assert np.array_equal(key, np.repeat(np.arange(ix.cells), lens))                       # list k holds exactly the points of cell k ...
    assert np.array_equal(np.bincount(key, minlength=ix.cells), lens)                      # ... all of them
    inside = np.ones(len(order), bool)
    inside[starts[:-1][lens > 0]] = False
    assert (np.diff(order)[inside[1:]] > 0).all()                                          # ascending inside every list
    m, rem = order // (sp.D * sp.fH * sp.fW), order % (sp.D * sp.fH * sp.fW)
    assert np.array_equal(points[:, 0], m * sp.fH * sp.fW + rem % (sp.fH * sp.fW)) and np.array_equal(points[:, 1], points[:, 0] * sp.D + rem // (sp.fH * sp.fW))
    chunks = ix.chunks()
    assert all(0 < e - b <= ops.LSS_CHUNK for _, b, e in chunks)
    assert [b for _, b, _ in chunks] == sorted(b for _, b, _ in chunks) and all(starts[k] <= b and e <= starts[k + 1] for k, b, e in chunks)
    assert [e for _, _, e in chunks[:-1]] == [b for _, b, _ in chunks[1:]] and chunks[0][1] == 0 and chunks[-1][2] == len(order)      # they tile the points
    assert np.array_equal(ix.long_cells.numpy(), np.nonzero(lens > ops.LSS_CHUNK)[0])
    print(f"{which}: {len(order)} kept of {flat.size}, {int((lens > 0).sum())} occupied cells of {ix.cells}, longest list {int(lens.max())}, {len(chunks)} chunks, {ix.long_cells.numel()} long lists")
    if which == "one_cell":
        assert len(order) == flat.size == 1536 and lens.tolist() == [1536] and len(chunks) == 3
    if which == "skewed":
        assert int(lens.max()) == 700 and int(((lens >= 1) & (lens <= 5)).sum()) == 8 and len(chunks) == 10 and ix.long_cells.tolist() == [17]


def test_index_cache_follows_the_rig():
    sp, rig, _, _ = R.case(2, 3, 5)
    sp = R.splat()
    cams = R.rig_tensors(rig)
    a = sp.index_for(*cams)
    assert sp.index_for(*[t.clone() for t in cams]) is a and sp.index_builds == 1
    moved = [t.clone() for t in cams]
    moved[1][1, 2, 0] += 0.25
    b = sp.index_for(*moved)
    assert b is not a and sp.index_builds == 2 and not torch.equal(a.order, b.order)
    assert sp.index_for(*moved) is b and sp.index_builds == 2
    # reference_cells: the lists are made of the reference's float32 cells (on this rig the same cells, hence the same lists)
    sp.reference_cells = True
    c = sp.build_index(*cams)
    idx, kept = sp.voxel_indices(sp.get_geometry(*cams))
    assert c.n_points == int(kept.sum()) and torch.equal(c.order, a.order) and torch.equal(c.starts, a.starts) and torch.equal(c.points, a.points)


# ---- header, table, library ------------------------------------------------------------------------------------------------------------------------------
def test_lss_header_table_and_library_agree():
    """The header declares exactly ``NAMES``, the keys of ``hip.LSS_SIGNATURES`` (types, counts and exports: tests/test_abi_cpu.py); every declaration's comment
    cites the reference lines it replaces; build.py lists the source; the source reads no environment variable."""
    text = open(abi_headers.path(HEADER)).read()
    assert '#include "coalign_amd.h"' in text
    declared = abi_headers.declarations(HEADER)
    assert set(declared) == set(hip.LSS_SIGNATURES) == abi_headers.names(HEADER) == NAMES
    comments = re.findall(r"/\*.*?\*/", text, flags=re.S)
    cites = {"coalign_lss_cells": ("lift_splat_shoot.py:80-102", "lift_splat_shoot.py:65-78", "lift_splat_shoot.py:126", "lift_splat_shoot.py:133-135", "camera_utils.py:129-134",
                                   "camera_utils.py:187-196", "undefined"),
             "coalign_lss_depth_prob": ("lss_submodule.py:66-67", "lss_submodule.py:134-135"),
             "coalign_lss_pool": ("lss_submodule.py:134-136", "lift_splat_shoot.py:116-169", "lift_splat_shoot.py:167")}
    for name in declared:
        last = [c for c in comments if c in text[:text.index(name + "(")]][-1]
        assert all(c in last for c in cites[name]), name
    assert '"lss_pool.hip"' in open(os.path.join(REPO, "coalign_amd", "build.py")).read() and "lss_pool.hip" in build.SOURCES
    assert int(re.search(r"#define COALIGN_LSS_CHUNK (\d+)", text).group(1)) == ops.LSS_CHUNK == 512
    assert int(re.search(r"#define COALIGN_LSS_MAX_DEPTH (\d+)", text).group(1)) == ops.LSS_MAX_DEPTH
    kernel = open(os.path.join(REPO, "coalign_amd", "csrc", "lss_pool.hip")).read()
    assert "getenv" not in kernel and "lab_env" not in kernel and "atomic" not in re.sub(r"/\*.*?\*/", "", kernel, flags=re.S).replace("no atomics", "")
    for k in ("lss_cells", "lss_depth_prob", "lss_pool"):
        assert re.search(r"__global__[^\n]*\bvoid " + k + r"\(", kernel), k


def _cells(**kw):
    a = dict(rots=ONE, trans=ONE, intrins=ONE, post_rots=ONE, post_trans=ONE, A=2, N=3, xs=ONE, ys=ONE, ds=ONE, D=6, fH=6, fW=8, lower=(-4.0, -3.2, -2.0), dx=(0.4, 0.4, 3.0),
             nx=22, ny=16, nz=2, cell=TWO)
    a.update(kw)
    return hip.lib().coalign_lss_cells(a["rots"], a["trans"], a["intrins"], a["post_rots"], a["post_trans"], a["A"], a["N"], a["xs"], a["ys"], a["ds"], a["D"], a["fH"], a["fW"],
                                       *a["lower"], *a["dx"], a["nx"], a["ny"], a["nz"], a["cell"], NULL)


def _prob(logit=ONE, M=6, D=6, fH=6, fW=8, cl=0, prob=TWO):
    return hip.lib().coalign_lss_depth_prob(logit, M, D, fH, fW, cl, prob, NULL)


def _pool(**kw):
    a = dict(x=ONE, prob=ONE, rows=288, C=64, D=6, points=ONE, n_points=700, starts=ONE, cells=704, long_cells=ONE, n_long=1, out=TWO)
    a.update(kw)
    return hip.lib().coalign_lss_pool(a["x"], a["prob"], a["rows"], a["C"], a["D"], a["points"], a["n_points"], a["starts"], a["cells"], a["long_cells"], a["n_long"], a["out"], NULL)


def test_lss_argument_refusals_without_a_gpu():
    """NULL and misaligned pointers -1, impossible sizes -2, shapes outside the kernels -3, empty work 0 without a launch: all before any HIP call."""
    for arg in ("rots", "trans", "intrins", "post_rots", "post_trans", "xs", "ys", "ds", "cell"):
        assert _cells(**{arg: NULL}) == -1 and _cells(**{arg: ctypes.c_void_p(18)}) == -1, arg
    for bad in (dict(A=0), dict(N=0), dict(D=0), dict(fH=-1), dict(fW=0), dict(nx=0), dict(ny=-3), dict(nz=0), dict(A=1 << 15, N=1 << 10, D=128), dict(nx=1 << 12, ny=1 << 12, nz=1 << 8),
                dict(dx=(0.0, 0.4, 3.0)), dict(dx=(0.4, -0.4, 3.0)), dict(dx=(0.4, 0.4, float("inf"))), dict(dx=(float("nan"), 0.4, 3.0)), dict(lower=(float("nan"), 0.0, 0.0)),
                dict(lower=(0.0, float("-inf"), 0.0))):
        assert _cells(**bad) == -2, bad
    assert _prob(logit=NULL) == -1 and _prob(prob=NULL) == -1 and _prob(logit=ctypes.c_void_p(6)) == -1
    assert _prob(M=-1) == -2 and _prob(D=0) == -2 and _prob(M=1 << 12, D=128, fH=64, fW=64) == -2
    assert _prob(D=129) == -3 and _prob(cl=2) == -3 and _prob(cl=-1) == -3
    assert _prob(M=0) == 0 and _prob(M=0, logit=NULL, prob=NULL) == 0 and _prob(fH=0) == 0
    for arg, mis in (("x", 8), ("prob", 2), ("points", 4), ("starts", 2), ("long_cells", 2), ("out", 8)):
        assert _pool(**{arg: NULL}) == -1 and _pool(**{arg: ctypes.c_void_p(mis)}) == -1, arg
    for bad in (dict(rows=-1), dict(n_points=-1), dict(cells=-1), dict(n_long=-1), dict(n_long=705), dict(D=0), dict(C=0), dict(rows=1 << 25, D=64), dict(rows=0)):
        assert _pool(**bad) == -2, bad
    for bad in (dict(C=32), dict(C=96), dict(C=256), dict(D=129), dict(C=8)):
        assert _pool(**bad) == -3, bad
    assert _pool(cells=0, n_long=0) == 0 and _pool(cells=0, n_long=0, out=NULL, starts=NULL) == 0
    assert _pool(n_points=0, x=NULL, prob=NULL, points=NULL, out=NULL) == -1 and _pool(n_long=0, long_cells=NULL, out=NULL) == -1      # (what remains required)
    assert ops.lss_shape_ok(64, 1) and ops.lss_shape_ok(128, 128) and not any(ops.lss_shape_ok(C, D) for C, D in ((32, 6), (256, 6), (64, 0), (64, 129)))
    sp, rig, _, _ = R.case(2, 3, 5)
    ix = sp.build_index(*R.rig_tensors(rig))
    with pytest.raises(hip.CoalignHipError):
        ops.lss_pool(torch.zeros(6, 6, 6, 8), torch.zeros(6, 64, 6, 8), ix)
    with pytest.raises(hip.CoalignHipError):
        ops.lss_cells(*R.rig_tensors(rig), *sp.axes, sp.lower, sp.cell_size, sp.nx, 3)


def test_switch_defaults_to_on_and_the_cpu_takes_the_torch_route(monkeypatch):
    src = open(os.path.join(REPO, "coalign_amd", "lss.py")).read()
    assert 'LSS_POOL = os.environ.get("COALIGN_LSS_POOL", "1") != "0"' in src
    assert lss.LSS_POOL is (os.environ.get("COALIGN_LSS_POOL", "1") != "0")
    sp = R.splat()
    logit, x = R.features(6, 64, sp.D, sp.fH, sp.fW, seed=3)
    monkeypatch.setattr(lss, "LSS_POOL", True)
    assert sp.kernel_reason(logit, x) == "not on the GPU"
    monkeypatch.setattr(lss, "LSS_POOL", False)
    assert "COALIGN_LSS_POOL=0" in sp.kernel_reason(logit, x)


# ---- the model ------------------------------------------------------------------------------------------------------------------------------------------------
def test_build_model_of_the_camera_configs():
    """State-dict names of the heads, ``bevencode`` and ``camencode``; output keys with the ``_single`` heads; a CPU forward through the torch route; the full-size config builds with the reference's grid; the parser table; refusals."""
    assert "load_lift_splat_shoot_params" in YAML_PARSERS and CAMERA_REGISTRY["lift_splat_shoot_intermediate"] is lss.LiftSplatShootIntermediate
    assert "lift_splat_shoot_intermediate" not in MODEL_REGISTRY
    h = builtin_config("camera/mini_lss_coalign")
    assert h["postprocess"]["anchor_args"]["W"] == 32 and h["postprocess"]["anchor_args"]["H"] == 16 and h["postprocess"]["anchor_args"]["vd"] == 4
    model = build_model(h).eval()
    assert isinstance(model, lss.LiftSplatShootIntermediate) and model.splat.nx == [32, 16, 1] and (model.D, model.splat.fH, model.splat.fW) == (6, 6, 8)
    keys = list(model.state_dict().keys())
    for k in ("camencode.depth_head.weight", "camencode.depth_head.bias", "camencode.image_head.weight", "camencode.image_head.bias", "bevencode.conv1.weight",
              "bevencode.bn1.running_mean", "bevencode.layer1.0.conv1.weight", "bevencode.layer1.1.bn2.weight", "bevencode.layer2.0.downsample.0.weight",
              "bevencode.layer2.0.downsample.1.running_var", "bevencode.layer3.1.conv2.weight", "bevencode.up_layer1.conv.0.weight", "bevencode.up_layer1.conv.4.bias",
              "bevencode.up_layer2.conv.3.weight", "bevencode.down_layer.0.bias", "bevencode.down_layer.2.weight", "cls_head.weight", "reg_head.bias", "dir_head.weight",
              "cls_head_before_fusion.weight", "reg_head_before_fusion.weight", "dir_head_before_fusion.bias"):
        assert k in keys, k
    assert not any("splat" in k or "fuse_module" in k or "layer1.0.downsample" in k for k in keys)
    sd = model.state_dict()
    assert tuple(sd["camencode.depth_head.weight"].shape) == (6, 512, 1, 1) and tuple(sd["camencode.image_head.weight"].shape) == (64, 512, 1, 1)
    assert tuple(sd["bevencode.conv1.weight"].shape) == (64, 64, 7, 7) and tuple(sd["bevencode.up_layer2.conv.0.weight"].shape) == (256, 384, 3, 3)
    assert not any(p.requires_grad for p in model.camencode.parameters())
    fill_parameters_(model, seed=1)
    frame = make_camera_frame(h, 2, seed=5)
    with torch.no_grad():
        out = model(frame)
    assert list(out.keys()) == ["cls_preds", "reg_preds", "depth_items", "dir_preds", "cls_preds_single", "reg_preds_single", "dir_preds_single"] and out["depth_items"] is None
    assert tuple(out["cls_preds"].shape) == (1, 2, 8, 16) and tuple(out["reg_preds"].shape) == (1, 14, 8, 16) and tuple(out["dir_preds"].shape) == (1, 4, 8, 16)
    assert tuple(out["cls_preds_single"].shape) == (2, 2, 8, 16) and tuple(out["reg_preds_single"].shape) == (2, 14, 8, 16) and tuple(out["dir_preds_single"].shape) == (2, 4, 8, 16)
    assert all(bool(torch.isfinite(v).all()) for v in out.values() if v is not None) and model.splat.index_builds == 0      # (the torch route builds no index)
    # the pooled map feeds the result: other camera features, other predictions
    other = dict(frame, image_inputs=dict(frame["image_inputs"], trunk_features=frame["image_inputs"]["trunk_features"].flip(0)))
    with torch.no_grad():
        assert not torch.equal(model(other)["cls_preds"], out["cls_preds"])
    full = builtin_config("camera/opv2v_lss_coalign")
    m = build_model(full)
    assert m.splat.nx == [240, 240, 1] and (m.D, m.splat.fH, m.splat.fW, m.camC) == (48, 60, 80, 128) and tuple(m.bevencode.conv1.weight.shape) == (64, 128, 7, 7)
    assert "model" not in builtin_config("lss_coalign_fusion")                               # the fusion-only config stays as it was
    bad = builtin_config("camera/mini_lss_coalign")
    bad["model"]["args"]["use_depth_gt"] = True
    with pytest.raises(NotImplementedError):
        build_model(bad)
    bad["model"]["args"]["use_depth_gt"] = False
    bad["model"]["args"]["fusion_args"]["core_method"] = "att"
    with pytest.raises(NotImplementedError):
        build_model(bad)


def test_an_injected_encoder_reads_the_images():
    """With ``camencode=`` an encoder that has ``get_eff_features`` the model reads ``image_inputs['imgs']`` (the first three channels, cameras flattened)."""
    class Trunk(lss.CamHeads):
        def get_eff_features(self, x):
            assert tuple(x.shape) == (6, 3, 48, 64)
            return torch.nn.functional.avg_pool2d(x, 8).repeat(1, 171, 1, 1)[:, :512]
    h = builtin_config("camera/mini_lss_coalign")
    model = lss.LiftSplatShootIntermediate(h["model"]["args"], camencode=Trunk(6, 64)).eval()
    fill_parameters_(model, seed=2)
    frame = make_camera_frame(h, 2, seed=6)
    del frame["image_inputs"]["trunk_features"]
    frame["image_inputs"]["imgs"] = torch.randn(2, 3, 4, 48, 64, generator=torch.Generator().manual_seed(1))
    with torch.no_grad():
        out = model(frame)
    assert tuple(out["cls_preds"].shape) == (1, 2, 8, 16) and bool(torch.isfinite(out["reg_preds"]).all())
