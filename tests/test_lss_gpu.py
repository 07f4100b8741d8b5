"""Lift-Splat's frustum pooling on the GPU (csrc/lss_pool.hip): ``ops.lss_cells`` against the float64 restatement of tests/lss_reference.py and the reference's
fixture, ``ops.lss_pool`` against the float64 sum at every channel count, agent and camera count, height-slice count and grid the kernel's paths differ on, the
long-list split, the written-everywhere property, the softmax's range, bitwise reproducibility (twice, under a captured graph, with a rebuilt index), the input
layouts, and the camera model with the kernel route against the torch route."""
import numpy as np
import pytest
import torch

from conftest import assert_elementwise
from coalign_amd import lss, ops
from coalign_amd.config import builtin_config
from coalign_amd.detector import build_model, to_device
from coalign_amd.inference import inference_intermediate_fusion
from coalign_amd.postprocess import build_postprocessor
from coalign_amd.synthetic import fill_parameters_, make_camera_frame
import lss_reference as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
GRID_22X16_NZ1 = ((-4.0, 4.8, 0.4), (-3.2, 3.2, 0.4), (-10, 10, 20.0), (2, 12, 6))
GRID_1X1 = ((-100, 100, 200), (-100, 100, 200), (-10, 10, 20.0), (2, 12, 6))
Z2 = (-2, 4, 3.0)
RIGS = ((2, 3, 5), (1, 1, 21), (5, 4, 22), (1, 4, 23))      # (A, N, seed): the fixture's rig and three more


def _with_nz(grid, nz):
    return grid if nz == 1 else (grid[0], grid[1], Z2, grid[3])


def _cells(sp, rig):
    return ops.lss_cells(*R.rig_tensors(rig, DEV), *(a.to(DEV) for a in sp.axes), sp.lower, sp.cell_size, sp.nx, rig["trans"].shape[1])


def _pool(sp, rig, logit, x, cell=None):
    """The kernel route on the kernel's own cells (or on given ones) -> (map on the host, the cells as numpy)."""
    A, N = rig["trans"].shape[:2]
    cell = _cells(sp, rig) if cell is None else cell
    ix = ops.build_lss_index(cell, A, N, *sp.nx)
    return ops.lss_pool(logit.to(DEV), x.to(DEV), ix), cell.cpu().numpy()


# ---- cells ------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("A,N,seed", RIGS, ids=[f"A{a}_N{n}" for a, n, _ in RIGS])
def test_cells_equal_the_float64_restatement(A, N, seed):
    """Exactly equal on every point, at nz = 2 (the fixture's grid): no float64 coordinate of these rigs is within 1e-6 of an integer (asserted first), and two
    float64 evaluations differ by far less."""
    sp, rig, v, cell = R.case(A, N, seed)
    assert R.distance_to_integer(v) > 1e-6
    got = _cells(sp, rig)
    assert got.dtype == torch.int32 and tuple(got.shape) == (A * N, sp.D, sp.fH, sp.fW)
    assert np.array_equal(got.cpu().numpy(), cell)
    assert 0.1 < float((cell >= 0).mean()) < 0.9 and int((((v > -1) & (v < 0)).any(-1) & (cell >= 0)).sum()) >= 5      # (kept, dropped and folded points all occur)


def test_cells_against_the_reference_fixture_and_a_singular_camera(golden):
    g = golden("lss_pool.npz")
    sp, rig, v, cell = R.case(2, 3, 5)
    assert all(np.array_equal(rig[k].numpy(), g[k]) for k in R.CAMS)
    got = _cells(sp, rig).cpu().numpy()
    band = R.near_boundary(v, 1e-3)
    ref = g["cell"].reshape(got.shape)
    print(f"kernel / reference float32 cells: {int((got != ref).sum())} of {got.size} differ, {int(band.sum())} points inside the 1e-3 band")
    assert np.array_equal(got[~band], ref[~band])
    for kind in ("zero", "rank2"):                              # a singular intrinsic matrix: its camera's points are all dropped, the others untouched
        broken = {k: t.clone() for k, t in rig.items()}
        broken["intrins"][1, 0] = 0.0 if kind == "zero" else torch.tensor([[400.0, 0.0, 320.0], [0.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
        out = _cells(sp, broken).cpu().numpy()
        assert (out[3] == -1).all() and np.array_equal(np.delete(out, 3, 0), np.delete(cell, 3, 0)) and (cell[3] >= 0).any(), kind
        assert np.array_equal(R.cells_f64(R.scaled_coordinates(broken, *sp.axes, sp.lower, sp.cell_size), sp.nx), out)


# ---- the pooled map against float64 -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 4])
@pytest.mark.parametrize("A", [1, 2, 5])
@pytest.mark.parametrize("C", [64, 128])
def test_pool_against_float64(C, A, N):
    """nz in {1, 2} on the 22 x 16, 1 x 1 and 7 x 5 grids with the 6 x 8 x 6 frustum: the kernel route and ``forward_torch`` against the float64 sum over the
    kernel's own cells, element-wise."""
    logit, x = R.features(A * N, C, 6, 6, 8, seed=100 + C + 10 * A + N)
    for gname, grid in (("22x16", GRID_22X16_NZ1), ("1x1", GRID_1X1), ("7x5", R.GRID_7X5)):
        for nz in (1, 2):
            sp, rig, v, _ = R.case(A, N, 30 + A + N, _with_nz(grid, nz))
            got, cell = _pool(sp, rig, logit, x)
            nx, ny, _ = sp.nx
            assert tuple(got.shape) == (A, nz * C, ny, nx) and sp.nx[2] == nz and got.permute(0, 2, 3, 1).is_contiguous()
            ref = R.pool_f64(logit, x, cell, A, sp.nx)
            assert float(ref.abs().max()) > 0
            e_k = assert_elementwise(got, ref, f"lss_pool {gname} nz {nz}")
            on_dev = R.splat(R.grid_conf(*_with_nz(grid, nz))).to(DEV)
            e_t = float((on_dev.forward_torch(logit.to(DEV), x.to(DEV), *R.rig_tensors(rig, DEV)).double().cpu() - ref).abs().max() / ref.abs().max())
            print(f"C {C} A {A} N {N} grid {gname} nz {nz}: {int((cell >= 0).sum())} of {cell.size} points kept; kernel {e_k:.2e}, forward_torch {e_t:.2e} of the scale")


@pytest.mark.parametrize("D", [1, 48, 128])
def test_pool_depth_bins(D):
    sp, rig, v, _ = R.case(2, 4, 41, ((-4.0, 4.8, 0.4), (-3.2, 3.2, 0.4), Z2, (2, 12, D)))
    assert sp.D == D
    logit, x = R.features(8, 64, D, 6, 8, seed=D)
    got, cell = _pool(sp, rig, logit, x)
    ref = R.pool_f64(logit, x, cell, 2, sp.nx)
    print(f"D {D}: {int((cell >= 0).sum())} points kept, kernel {assert_elementwise(got, ref, f'D {D}'):.2e} of the scale")


@pytest.mark.parametrize("C", [64, 128])
def test_one_cell_takes_everything_and_a_skewed_grid(C):
    """All 1 536 points in ``out[0, :, 0, 0]`` (three chunks of 512, the workgroup route); and hand-made cells with one list of 700 points beside lists of
    1 .. 5 (both routes in one launch)."""
    sp, rig, v, cell = R.case(1, 4, 7, R.GRID_ONE_CELL)
    assert sp.nx == [1, 1, 1] and (cell == 0).all() and cell.size == 1536
    logit, x = R.features(4, C, 8, 6, 8, seed=C)
    got, kcell = _pool(sp, rig, logit, x)
    assert np.array_equal(kcell, cell) and tuple(got.shape) == (1, C, 1, 1)
    ix = ops.build_lss_index(torch.from_numpy(cell), 1, 4, 1, 1, 1)
    assert ix.long_cells.tolist() == [0] and len(ix.chunks()) == 3
    ref = R.pool_f64(logit, x, cell, 1, sp.nx)
    print(f"one cell, C {C}: kernel {assert_elementwise(got, ref, 'one cell'):.2e} of the scale")
    skew = R.skewed_cells()
    sp7 = R.splat(R.grid_conf(*R.GRID_7X5_D8))
    rig7 = R.case(1, 4, 7, R.GRID_7X5_D8)[1]
    got, _ = _pool(sp7, rig7, logit, x, cell=torch.from_numpy(skew).to(DEV))
    ref = R.pool_f64(logit, x, skew, 1, sp7.nx)
    assert int((ref[0, 0] != 0).sum()) == 9
    print(f"skewed, C {C}: kernel {assert_elementwise(got, ref, 'skewed'):.2e} of the scale")
    assert float(got[0, :, 0, 0].abs().max()) == 0.0


def test_every_element_is_written():
    """The grid moved 1 km away: nothing is inside, and a map pre-filled with NaN comes back all zeros.  On the fixture's case no NaN survives either."""
    far = ((1000.0, 1008.8, 0.4), (-3.2, 3.2, 0.4), Z2, (2, 12, 6))
    for grid in (far, None):
        sp, rig, v, cell = R.case(2, 3, 5, grid)
        logit, x = R.features(6, 128, 6, 6, 8, seed=9)
        ix = ops.build_lss_index(_cells(sp, rig), 2, 3, *sp.nx)
        out = torch.full((2, sp.nx[1], sp.nx[0], sp.nx[2] * 128), float("nan"), device=DEV).permute(0, 3, 1, 2)      # (the far grid has 21 columns: 8.8 / 0.4 truncates)
        got = ops.lss_pool(logit.to(DEV), x.to(DEV), ix, out=out)
        assert got.data_ptr() == out.data_ptr() and bool(torch.isfinite(out).all())
        if grid is far:
            assert ix.n_points == 0 and (cell < 0).all() and float(out.abs().max()) == 0.0
        else:
            assert_elementwise(out, R.pool_f64(logit, x, cell, 2, sp.nx), "into a NaN-filled map")


def test_softmax_range():
    """Logits of +-80 and more, and a row with one logit 60 above the rest: finite and inside the element-wise bound."""
    sp, rig, v, cell = R.case(2, 3, 5)
    logit, x = R.features(6, 64, 6, 6, 8, seed=13)
    wide = logit * (80.0 / 3.0)
    assert float(wide.abs().max()) > 200
    hot = logit.clone()
    hot[:, 2] += 60.0
    for name, lg in (("+-80", wide), ("one-hot", hot)):
        got, kcell = _pool(sp, rig, lg, x)
        assert bool(torch.isfinite(got).all())
        print(f"{name}: kernel {assert_elementwise(got, R.pool_f64(lg, x, kcell, 2, sp.nx), name):.2e} of the scale")
    prob = ops.lss_depth_prob(hot.to(DEV)).cpu()
    assert tuple(prob.shape) == (6 * 48, 6) and float((prob.sum(1) - 1).abs().max()) < 1e-6 and float(prob[:, 2].min()) > 0.999


def test_reproducible_bits_graph_replay_and_a_rebuilt_index():
    sp, rig, v, cell = R.case(5, 4, 22)
    logit, x = (t.to(DEV) for t in R.features(20, 128, 6, 6, 8, seed=17))
    x = x.contiguous(memory_format=torch.channels_last)
    ix = ops.build_lss_index(_cells(sp, rig), 5, 4, *sp.nx)
    first = ops.lss_pool(logit, x, ix)
    assert torch.equal(first, ops.lss_pool(logit, x, ix))
    again = ops.build_lss_index(_cells(sp, rig), 5, 4, *sp.nx)
    assert again is not ix and torch.equal(again.points, ix.points) and torch.equal(again.starts, ix.starts) and torch.equal(first, ops.lss_pool(logit, x, again))
    assert_elementwise(first, R.pool_f64(logit.cpu(), x.cpu(), cell, 5, sp.nx), "A 5 N 4")
    static = torch.full_like(first, float("nan"))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.lss_pool(logit, x, ix, out=static)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.lss_pool(logit, x, ix, out=static)                  # the frame path: two launches, no allocation of the library's own
    static.fill_(float("nan"))
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(static, first)
    x.copy_(x.flip(0))                                          # new inputs in the captured buffers
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(static, ops.lss_pool(logit, x, ix)) and not torch.equal(static, first)


def test_layouts_give_equal_bits():
    sp, rig, v, cell = R.case(2, 3, 5)
    logit, x = (t.to(DEV) for t in R.features(6, 128, 6, 6, 8, seed=19))
    ix = ops.build_lss_index(_cells(sp, rig), 2, 3, *sp.nx)
    plain = ops.lss_pool(logit, x, ix)
    cl = torch.channels_last
    assert x.is_contiguous() and not x.contiguous(memory_format=cl).is_contiguous()
    for lg in (logit, logit.contiguous(memory_format=cl)):
        for xx in (x, x.contiguous(memory_format=cl)):
            assert torch.equal(plain, ops.lss_pool(lg, xx, ix))
    assert torch.equal(ops.lss_depth_prob(logit), ops.lss_depth_prob(logit.contiguous(memory_format=cl)))
    with pytest.raises(ValueError):
        ops.lss_pool(logit[:5], x, ix)
    with pytest.raises(Exception):
        ops.lss_pool(logit, x[:, :32], ix)


# ---- the model ----------------------------------------------------------------------------------------------------------------------------------------------
def test_camera_model_kernel_route_against_the_torch_route(monkeypatch):
    """``camera/mini_lss_coalign`` with non-default BatchNorm statistics and 2 agents: every head of the kernel route against ``COALIGN_LSS_POOL=0``, element-wise (the
    rig is one on which float32 and float64 geometry agree on every cell: asserted); boxes out of ``inference_intermediate_fusion``; the index is reused on a
    second frame of the same rig and rebuilt when one ``trans`` changes."""
    h = builtin_config("camera/mini_lss_coalign")
    model = build_model(h)
    fill_parameters_(model, seed=1)
    model = model.to(DEV).eval()
    frame = to_device(make_camera_frame(h, 2, seed=5), DEV)
    cams = [frame["image_inputs"][k] for k in R.CAMS]
    sp = model.splat
    idx, kept = sp.voxel_indices(sp.get_geometry(*cams))
    c32 = torch.where(kept, (idx[:, 2] * sp.nx[1] + idx[:, 1]) * sp.nx[0] + idx[:, 0], torch.full_like(idx[:, 0], -1))
    assert torch.equal(c32.int().cpu(), sp.cells_float64(*cams).reshape(-1).cpu()) and 0.2 < float(kept.float().mean()) < 0.9
    feats = model.camera_features(frame["image_inputs"])
    monkeypatch.setattr(lss, "LSS_POOL", True)
    assert sp.kernel_reason(*feats) is None and "C = 8" in sp.kernel_reason(feats[0], feats[1][:, :8])
    with torch.no_grad():
        on = model(frame)
        assert sp.index_builds == 1
        second = dict(frame, image_inputs=dict(frame["image_inputs"], trunk_features=frame["image_inputs"]["trunk_features"].flip(0)))
        on2 = model(second)
        assert sp.index_builds == 1 and not torch.equal(on2["cls_preds"], on["cls_preds"])
        moved = dict(frame["image_inputs"], trans=frame["image_inputs"]["trans"].clone())
        moved["trans"][1, 2, 0] += 0.5
        model(dict(frame, image_inputs=moved))
        assert sp.index_builds == 2
        model(frame)
        assert sp.index_builds == 3
        monkeypatch.setattr(lss, "LSS_POOL", False)
        assert "COALIGN_LSS_POOL=0" in sp.kernel_reason(*feats)
        off = model(frame)
        assert sp.index_builds == 3
    assert list(on.keys()) == ["cls_preds", "reg_preds", "depth_items", "dir_preds", "cls_preds_single", "reg_preds_single", "dir_preds_single"]
    for k in on:
        if k != "depth_items":
            print(f"{k}: kernel route vs torch route {assert_elementwise(on[k], off[k], k):.2e} of the scale")
    monkeypatch.setattr(lss, "LSS_POOL", True)
    post = build_postprocessor(h["postprocess"], False)
    with torch.no_grad():
        model.cls_head.bias.add_(3.0)
    batch = {"ego": dict(frame, transformation_matrix=torch.eye(4, device=DEV), anchor_box=torch.from_numpy(post.generate_anchor_box()).to(DEV))}
    res = inference_intermediate_fusion(batch, model, post)
    assert res["pred_box_tensor"] is not None and res["pred_box_tensor"].shape[1:] == (8, 3) and len(res["pred_score"]) == len(res["pred_box_tensor"]) > 0
