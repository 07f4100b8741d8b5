"""NaiveCompressor's encoder on the sparse canvas (include/coalign_amd_narrow_sparse.h; csrc/conv3x3_narrow.hip, input kind 2) on the MI355X.

Kernel level, through the C ABI: ``coalign_conv3x3_sp_narrow_sparse`` on (sp16 rows, stamps, state) against input kind 1 of ``coalign_conv3x3_sp_narrow`` on the
densified canvas in channels-last memory -- the same products in the same order, so ``SplitMap.data`` is compared with ``torch.equal``.  The grids are small and
each names what it can break: 32 x 64 is exactly 2 x 2 tiles (16 x 32 output pixels per tile), 37 x 75 leaves partial tiles on both edges and exercises the
640-group DMA padding of the 18 x 34 patch, 5 x 131 has fewer rows than a tile, 1 x 1 is a single pixel.

Model and pipeline level: ``mini_coalign`` with ``compression: 4``, two agents, 150 pillars each.
"""
import copy
import ctypes

import pytest
import torch

from coalign_amd import backbone as bb
from coalign_amd import detector, hip, ops
from coalign_amd import pipeline as pl_mod
from coalign_amd.config import builtin_config
from coalign_amd.detector import build_model, to_device
from coalign_amd.postprocess import build_postprocessor
from coalign_amd.synthetic import fill_parameters_, make_frame
from conftest import assert_elementwise
from sp_helpers import assert_split_map_holds

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BOUND = 3e-6                     # of the channel's own scale: DESIGN.md section 8a's kernel-level bound


# ------------------------------------------------------------------------------------------------ helpers
def _ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _layer(cin, cout, seed):
    """Weights, bias and the narrow weight image of a (cin -> cout) layer; negative and positive biases, so that ReLU cuts some empty pixels and keeps others."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    w = torch.randn((cout, cin, 3, 3), generator=g, device=DEV) * (1.0 / (9 * cin) ** 0.5)
    b = torch.randn(cout, generator=g, device=DEV) * 0.1
    return w, b, ops.pack_conv3x3_narrow_weight(w)


def _kind1(dense, img, b, cout, relu):
    """The yardstick: input kind 1 (channels-last float32) of the existing kernel, through the C ABI."""
    N, C, H, W = dense.shape
    x = dense.permute(0, 2, 3, 1).contiguous()
    out = ops.SplitMap.empty(N, cout, H, W, dense.device)
    hip.check(hip.lib().coalign_conv3x3_sp_narrow(_ptr(x), ops.NARROW_IN_NHWC, _ptr(img), _ptr(b), _ptr(out.data), N, C, cout, H, W, int(relu), None, _stream()), "kind 1")
    return out


def _kind2_status(rows, m_rows, stamps, state, shape, img, b, cout, relu, out):
    N, C, H, W = shape
    return hip.lib().coalign_conv3x3_sp_narrow_sparse(ops._rows_ptr(rows), int(m_rows), _ptr(stamps), _ptr(state), _ptr(img), _ptr(b), _ptr(out.data), N, C, cout, H, W,
                                                      int(relu), None, _stream())


def _kind2(sc, img, b, cout, relu, rows=None, m_rows=None):
    """The new symbol through the C ABI on a SparseCanvas (``rows``: its packed rows when the caller has prepared them)."""
    rows = ops.sp_pack_rows(sc) if rows is None else rows
    N, C, H, W = sc.shape
    out = ops.SplitMap.empty(N, cout, H, W, sc.device)
    hip.check(_kind2_status(rows, rows.shape[0] if m_rows is None else m_rows, sc.stamps, sc.state, sc.shape, img, b, cout, relu, out), "kind 2")
    return out


def _mini_on_grid(ny, nx):
    """A deep-copied mini_coalign whose lidar range spans ``ny x nx`` cells of its 0.4 m voxels."""
    h = copy.deepcopy(builtin_config("mini_coalign"))
    rng = [-0.2 * nx, -0.2 * ny, -3.0, 0.2 * nx, 0.2 * ny, 1.0]
    h["preprocess"]["cav_lidar_range"] = list(rng)
    h["model"]["args"]["lidar_range"] = list(rng)
    h["model"]["args"]["point_pillar_scatter"]["grid_size"] = [nx, ny, 1]
    return h


_ENCODER = {}


def _pillar_args():
    """The mini model's PFN layer (one weight set for every grid)."""
    if not _ENCODER:
        model = build_model(builtin_config("mini_coalign"))
        fill_parameters_(model, seed=2)
        _ENCODER["pfn"] = model.to(DEV).eval().pillar_vfe.pfn_layers[0]
    pfn = _ENCODER["pfn"]
    return pfn.linear.weight, None, (pfn.norm.weight, pfn.norm.bias, pfn.norm.running_mean, pfn.norm.running_var), 1e-3, True


def _pillars(h, n_agents, pillars, seed, duplicates=17, agents_with_pillars=None):
    """Pillar arrays of ``n_agents`` agents (``agents_with_pillars`` of them non-empty) on the grid of ``h``; ``duplicates`` cells per frame appear twice with
    different content, rows shuffled so that the winning (larger) row of a cell sits anywhere."""
    live = n_agents if agents_with_pillars is None else agents_with_pillars
    pl = make_frame(h, live, pillars_per_agent=pillars, seed=seed)["processed_lidar"]
    vf, npts, coords = pl["voxel_features"], pl["voxel_num_points"], pl["voxel_coords"].to(torch.int32)
    M = vf.shape[0]
    k = min(duplicates, M)
    if k:
        vf, npts, coords = torch.cat([vf, vf[M - k:].flip(0) * 0.5]), torch.cat([npts, npts[M - k:].flip(0)]), torch.cat([coords, coords[:k]])
    perm = torch.randperm(vf.shape[0], generator=torch.Generator().manual_seed(seed))
    return vf[perm].contiguous().to(DEV), npts[perm].to(torch.int32).contiguous().to(DEV), coords[perm].contiguous().to(DEV)


def _encode(ny, nx, n_agents, pillars, seed, canvas_cache=None, count_below=0, agents_with_pillars=None):
    """-> (canvas_cache, SparseCanvas) of the one-launch pillar op on this grid.  The cache is returned because a second encode through it overwrites the stamps."""
    h = _mini_on_grid(ny, nx)
    margs = h["model"]["args"]
    vf, npts, coords = _pillars(h, n_agents, pillars, seed, agents_with_pillars=agents_with_pillars)
    cache = {} if canvas_cache is None else canvas_cache
    count_dev = torch.tensor([vf.shape[0] - count_below], dtype=torch.int32, device=DEV) if count_below else None
    w, bias, bn, eps, absxyz = _pillar_args()
    sc = ops.pillar_encode_sparse(vf, npts, coords, w, bias, bn, eps, absxyz, margs["voxel_size"], margs["lidar_range"][:3], n_agents, ny, nx, canvas_cache=cache, count_dev=count_dev)
    return cache, sc


GRIDS = {(32, 64): (2, 600), (37, 75): (3, 450), (5, 131): (2, 300), (1, 1): (3, 1)}      # grid -> (agents, pillars per agent)
_CANVASES = {}


def _canvas(grid):
    """One encoder-made canvas per grid with its dense form (shared: nothing below writes to them, and each grid has a stamp map of its own)."""
    if grid not in _CANVASES:
        n, m = GRIDS[grid]
        _, sc = _encode(grid[0], grid[1], n, m, seed=grid[0] + grid[1])
        dense = sc.dense()
        assert float(dense.abs().max()) > 0 and sc.feats.shape[0] > n * m - 1      # (duplicates included)
        _CANVASES[grid] = (sc, dense)
    return _CANVASES[grid]


# ------------------------------------------------------------------------------------------------ kernel level
@pytest.mark.parametrize("grid", list(GRIDS), ids=lambda g: f"{g[0]}x{g[1]}")
@pytest.mark.parametrize("cout", [16, 32])
@pytest.mark.parametrize("relu", [True, False], ids=["relu", "linear"])
def test_sparse_kind_equals_the_channels_last_kind_on_encoder_made_canvases(grid, cout, relu):
    """Kind 2 on the rows and stamps the pillar op wrote == kind 1 on the densified canvas, bit for bit; ``ops.conv3x3_sp_narrow`` on the SparseCanvas launches the
    same thing."""
    sc, dense = _canvas(grid)
    w, b, img = _layer(64, cout, 10 * cout + relu)
    want = _kind1(dense, img, b, cout, relu)
    got = _kind2(sc, img, b, cout, relu)
    assert got.shape == (sc.shape[0], cout) + grid and torch.equal(got.data, want.data)
    via_op = ops.conv3x3_sp_narrow(sc, img, b, cout, relu)
    assert isinstance(via_op, ops.SplitMap) and torch.equal(via_op.data, want.data)
    assert float(got.dense().abs().max()) > 0
    if not relu:
        assert float(got.dense().min()) < 0
    assert not ops.sp_range_exceeded(DEV)


def test_stale_stamps_read_as_empty_and_a_stale_object_is_refused():
    """Frame A then frame B through ONE stamp map: a cell only A occupied holds A's stamp with an old tag and must read as empty -- the result is kind 1 on B's
    dense canvas.  The SparseCanvas object of A, kept across B's encode, is refused by the op."""
    ny, nx = 37, 75
    cache, sc_a = _encode(ny, nx, 2, 500, seed=1)
    cells_a = {tuple(c) for c in sc_a.coords.cpu().tolist()}
    dense_a = sc_a.dense()
    _, sc_b = _encode(ny, nx, 2, 300, seed=2, canvas_cache=cache)
    assert sc_b.stamps is sc_a.stamps and len(cache) == 1
    cells_b = {tuple(c) for c in sc_b.coords.cpu().tolist()}
    assert len(cells_a - cells_b) > 100                              # cells occupied only in A
    w, b, img = _layer(64, 32, 3)
    dense_b = sc_b.dense()
    want = _kind1(dense_b, img, b, 32, True)
    got = _kind2(sc_b, img, b, 32, True)
    assert torch.equal(got.data, want.data)
    assert not torch.equal(want.data, _kind1(dense_a + dense_b, img, b, 32, True).data)      # (A's cells would have shown)
    with pytest.raises(hip.CoalignHipError, match="stale SparseCanvas"):
        ops.conv3x3_sp_narrow(sc_a, img, b, 32, True)
    assert torch.equal(ops.conv3x3_sp_narrow(sc_b, img, b, 32, True).data, want.data)


def test_rows_past_the_device_side_count_are_never_referenced():
    """``count_dev`` below the arrays' capacity: the pillar op stamps no row at or past the count, ``sp_pack_rows`` leaves those rows alone -- filled with a large
    finite value (float32 rows before the pack, sp16 rows after it) they do not move the result."""
    ny, nx = 37, 75
    below = 123
    _, sc = _encode(ny, nx, 2, 500, seed=5, count_below=below)
    count = int(sc.count_dev.item())
    assert count == sc.feats.shape[0] - below
    dense = sc.dense()
    w, b, img = _layer(64, 16, 4)
    want = _kind1(dense, img, b, 16, True)
    sc.feats[count:] = 6.0e4
    rows = ops.sp_pack_rows(sc)
    rows[count:] = 6.0e4
    got = _kind2(sc, img, b, 16, True, rows=rows)
    assert torch.equal(got.data, want.data)
    live = (sc.stamps >> 32) == int(sc.state[0])
    assert int((sc.stamps[live] & 0xffffffff).max()) < count
    assert not ops.sp_range_exceeded(DEV)


def test_m_rows_guard_reads_rows_beyond_the_array_as_empty():
    """The C symbol with ``M_rows`` smaller than the real row count: every cell whose stamp names a row >= M_rows reads as zero (a guard: nothing is read past
    the M_rows rows) -- kind 1 on the dense canvas with those cells zeroed."""
    sc, dense = _canvas((37, 75))
    M = sc.feats.shape[0]
    m_rows = M - 200
    live = (sc.stamps >> 32) == int(sc.state[0])
    cut = (live & ((sc.stamps & 0xffffffff) >= m_rows)).view(sc.shape[0], 1, sc.ny, sc.nx)
    assert 100 < int(cut.sum()) <= 200
    w, b, img = _layer(64, 32, 6)
    want = _kind1(torch.where(cut, torch.zeros_like(dense), dense), img, b, 32, False)
    got = _kind2(sc, img, b, 32, False, rows=ops.sp_pack_rows(sc)[:m_rows], m_rows=m_rows)
    assert torch.equal(got.data, want.data)
    assert not torch.equal(got.data, _kind1(dense, img, b, 32, False).data)


@pytest.mark.parametrize("case", ["empty_frame", "empty_agent"])
def test_empty_frame_and_empty_agent(case):
    """M = 0, and one agent without pillars: the empty maps equal kind 1 on the all-zero canvas, which is relu(bias) everywhere."""
    ny, nx = 19, 40
    w, b, img = _layer(64, 16, 8)
    if case == "empty_frame":
        _, sc = _encode(ny, nx, 2, 0, seed=3)
        assert sc.feats.shape[0] == 0
        dense = torch.zeros((2, 64, ny, nx), device=DEV)
    else:
        _, sc = _encode(ny, nx, 2, 200, seed=3, agents_with_pillars=1)
        dense = sc.dense()
        assert float(dense[0].abs().max()) > 0 and float(dense[1].abs().max()) == 0
    want = _kind1(dense, img, b, 16, True)
    got = _kind2(sc, img, b, 16, True)
    assert torch.equal(got.data, want.data)
    empty = ops.SplitMap(got.data[1:2].contiguous()) if case == "empty_agent" else got
    n = 1 if case == "empty_agent" else 2
    assert_split_map_holds(empty, torch.relu(b).view(1, -1, 1, 1).expand(n, 16, ny, nx).contiguous(), case)
    assert float(torch.relu(b).max()) > 0 and float(b.min()) < 0


def _hand_built(C, seed, N=2, H=19, W=40, tag=7, fill=0.3):
    """feats [M, C], stamps (tag << 32) | row on ~30 % of the cells (rows in random order), stale stamps (tag - 1, valid rows) on others, state[0] = tag;
    -> (SparseCanvas, dense canvas built with torch indexing)."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    cells = N * H * W
    order = torch.randperm(cells, generator=g, device=DEV)
    M = int(fill * cells)
    live, stale = order[:M], order[M:M + M // 3]
    feats = torch.randn((M, C), generator=g, device=DEV)
    stamps = torch.zeros(cells, dtype=torch.int64, device=DEV)
    stamps[live] = (tag << 32) | torch.arange(M, device=DEV)
    stamps[stale] = ((tag - 1) << 32) | torch.arange(stale.numel(), device=DEV)
    state = torch.zeros(hip.lib().coalign_sparse_canvas_state_bytes() // 4, dtype=torch.int32, device=DEV)
    state[0] = tag
    dense = torch.zeros((cells, C), device=DEV)
    dense[live] = feats
    dense = dense.view(N, H, W, C).permute(0, 3, 1, 2)
    return ops.SparseCanvas(feats, stamps, state, None, N, C, H, W), dense


@pytest.mark.parametrize("C,cout", [(128, 32), (128, 16), (32, 16), (32, 32), (64, 32)])
def test_hand_built_canvases_at_other_channel_counts(C, cout):
    """Channel counts the encoder does not produce: C = 128 with Cout = 32 travels interval by interval (the weight image does not fit: Cin * Cout > 64 * 32) and
    prefetches the next tile's stamps across eight intervals; C = 128 / Cout = 16 and C = 64 are stationary with 8 and 4 intervals; C = 32 has the minimum of two."""
    sc, dense = _hand_built(C, seed=C + cout)
    w, b, img = _layer(C, cout, C * cout)
    for relu in (True, False):
        want = _kind1(dense, img, b, cout, relu)
        assert torch.equal(_kind2(sc, img, b, cout, relu).data, want.data), relu
    assert torch.equal(ops.conv3x3_sp_narrow(sc, img, b, cout, True).data, _kind1(dense, img, b, cout, True).data)
    sc.state[0] = 0                                                  # tag 0 is never current: every cell reads as empty
    assert torch.equal(_kind2(sc, img, b, cout, True).data, _kind1(torch.zeros_like(dense), img, b, cout, True).data)


def test_a_single_interval_layer_returns_the_documented_unsupported():
    """``Cin == 16``: a tile's stamps cannot be one interval ahead of its first DMA; the entry point returns COALIGN_ERR_UNSUPPORTED (-3) before any launch
    (include/coalign_amd_narrow_sparse.h), and the op raises."""
    sc, dense = _hand_built(16, seed=16)
    w, b, img = _layer(16, 16, 1)
    out = ops.SplitMap.empty(2, 16, 19, 40, DEV)
    assert _kind2_status(ops.sp_pack_rows(sc), sc.feats.shape[0], sc.stamps, sc.state, sc.shape, img, b, 16, True, out) == -3
    with pytest.raises(hip.CoalignHipError):
        ops.conv3x3_sp_narrow(sc, img, b, 16, True)
    assert _kind1(dense, img, b, 16, True).data.shape == out.data.shape          # (the dense kinds keep serving the shape)


def _conv64(x, w, b):
    """conv3x3(x, w, stride 1, pad 1) + b in float64 as nine matrix products (``conv64`` of tests/test_s2_gpu.py at stride 1, before the ReLU)."""
    N, Ci, H, W = x.shape
    xp = torch.nn.functional.pad(x.double(), (1, 1, 1, 1))
    out = torch.zeros((N, w.shape[0], H, W), dtype=torch.float64, device=x.device)
    for dy in range(3):
        for dx in range(3):
            out += torch.einsum("oc,nchw->nohw", w.double()[:, :, dy, dx], xp[:, :, dy:dy + H, dx:dx + W])
    return out + b.double().view(1, -1, 1, 1)


def test_sparse_kind_against_float64():
    """Every output channel within 3e-6 of its own scale (max |pre-activation| of the channel) of the float64 convolution of the float32 canvas, 37 x 75 grid."""
    sc, dense = _canvas((37, 75))
    w, b, img = _layer(64, 32, 12)
    pre = _conv64(dense, w, b)
    ref = torch.relu(pre)
    got = _kind2(sc, img, b, 32, True).dense().double()
    scale = pre.abs().amax(dim=(0, 2, 3))
    err = (got - ref).abs().amax(dim=(0, 2, 3)) / scale
    print(f"\nconv3x3_sp_narrow_sparse vs float64 on 3 x 64 x 37 x 75 -> 32: worst channel {float(err.max()):.2e} of its scale (bound {BOUND:g})")
    assert float(scale.min()) > 0 and float(err.max()) <= BOUND


# ------------------------------------------------------------------------------------------------ model and pipeline level
PILLAR_DENSE_OPS = [n for n in dir(ops) if n.startswith(("pillar_vfe_scatter", "pillar_encode_persistent", "pillar_encode_stream"))]


@pytest.fixture(scope="module")
def world():
    h = copy.deepcopy(builtin_config("mini_coalign"))
    h["model"]["args"]["compression"] = 4
    model = build_model(h)
    fill_parameters_(model, seed=0, cls_bias=-1.0)
    cpu_frame = make_frame(h, 2, pillars_per_agent=150, seed=3)
    from oracle import coalign_oracle as oracle
    with torch.no_grad():
        ref = oracle.coalign_forward({k: v.clone() for k, v in model.state_dict().items()}, h["model"]["args"], cpu_frame)
    model = model.to(DEV).eval()
    return {"hypes": h, "model": model, "frame": to_device(cpu_frame, DEV), "oracle": ref}


class _Spy:
    def __init__(self, monkeypatch):
        self.calls = []
        for name in ["conv3x3_sp_narrow", "conv3x3_sp_s2", "conv3x3_sp", "pillar_encode_sparse"] + PILLAR_DENSE_OPS:
            monkeypatch.setattr(ops, name, self._wrap(name, getattr(ops, name)))

    def _wrap(self, name, fn):
        def spy(*args, **kwargs):
            out = fn(*args, **kwargs)
            self.calls.append((name, args[0], out))
            return out
        return spy

    def of(self, name):
        return [c for c in self.calls if c[0] == name]


def test_forward_hands_the_compressor_a_sparse_canvas(world, monkeypatch):
    """One ``conv3x3_sp_narrow`` call whose input is a SparseCanvas, the one-launch pillar op and none of the dense-canvas pillar ops, and ``conv3x3_sp_s2`` reading
    the SplitMap the compressor's last layer returned."""
    model = world["model"]
    assert "pillar_vfe_scatter" in PILLAR_DENSE_OPS and "pillar_encode_stream" in PILLAR_DENSE_OPS
    assert detector.compressor_sparse_route(model) and not detector.sparse_canvas_route(model)
    with torch.no_grad():
        spy = _Spy(monkeypatch)
        out = model(world["frame"])
    assert all(bool(torch.isfinite(v).all()) for v in out.values())
    narrow = spy.of("conv3x3_sp_narrow")
    assert len(narrow) == 1 and isinstance(narrow[0][1], ops.SparseCanvas) and narrow[0][1].shape[1] == 64 and isinstance(narrow[0][2], ops.SplitMap)
    assert len(spy.of("pillar_encode_sparse")) == 1 and narrow[0][1] is spy.of("pillar_encode_sparse")[0][2]
    assert [c[0] for c in spy.calls if c[0] in PILLAR_DENSE_OPS] == []
    handed = spy.of("conv3x3_sp")[1][2]                              # the compressor's third layer
    s2 = spy.of("conv3x3_sp_s2")
    assert [c[0] for c in spy.calls][:4] == ["pillar_encode_sparse", "conv3x3_sp_narrow", "conv3x3_sp", "conv3x3_sp"]
    assert isinstance(handed, ops.SplitMap) and s2[0][1] is handed and isinstance(s2[0][2], tuple)      # (opener + skip in one launch)
    assert model.pillar_vfe.sparse_canvas is False                   # (encode restores the module's own setting)
    assert not ops.sp_range_exceeded(DEV)


def test_heads_match_the_oracle_and_the_dense_canvas_route(world, monkeypatch):
    """Suite tolerance (``assert_elementwise`` defaults) against the CPU oracle and against the same model with the selector off; with the selector off the heads
    are bit-equal to a forward whose ``compressor_sparse_route`` says no (today's route, exactly)."""
    model, frame = world["model"], world["frame"]
    with torch.no_grad():
        new = model(frame)
        monkeypatch.setattr(bb, "COMPRESS_SPARSE", False)
        assert not detector.compressor_sparse_route(model)
        spy = _Spy(monkeypatch)
        off = model(frame)
        assert torch.is_tensor(spy.of("conv3x3_sp_narrow")[0][1]) and spy.of("pillar_encode_sparse") == []
        monkeypatch.undo()
        assert detector.compressor_sparse_route(model)
        monkeypatch.setattr(detector, "compressor_sparse_route", lambda model, terms=None: False)
        parent = model(frame)
    for k in ("cls_preds", "reg_preds", "dir_preds"):
        e_o = assert_elementwise(new[k], world["oracle"][k], ("oracle", k))
        e_d = assert_elementwise(new[k], off[k], ("selector off", k))
        print(f"\nmini_coalign compression 4, {k}: sparse route {e_o:.2e} of the scale against the oracle, {e_d:.2e} against the dense-canvas route")
        assert torch.equal(off[k], parent[k]), k
        assert_elementwise(off[k], world["oracle"][k], ("oracle, selector off", k))


def _same(a, b):
    (ba, sa), (b2, s2) = a, b
    if ba is None or b2 is None:
        return ba is None and b2 is None
    return ba.shape == b2.shape and torch.equal(ba, b2) and torch.equal(sa, s2)


def test_compression_frames_go_through_frame_records(world):
    """FramePipeline in graph mode, one lane, three frames of different pillar counts inside one capacity bucket: every frame is read in place (no copy into the
    graph's buffers) and its detections equal the synchronous ``model(frame)`` + post-process bit for bit."""
    h = world["hypes"]
    model = build_model(h)
    fill_parameters_(model, seed=0, cls_bias=-1.0)
    with torch.no_grad():
        model.reg_head.weight.mul_(0.01); model.reg_head.bias.zero_(); model.cls_head.weight.mul_(0.05)      # (frames carry detections: tests/test_pipeline_slots_gpu.py)
    model = model.to(DEV).eval()
    pp = build_postprocessor(h["postprocess"], False)
    anchors = torch.from_numpy(pp.generate_anchor_box())
    frames = [to_device(make_frame(h, 2, pillars_per_agent=m, seed=60 + i, spread_xy=(4.0, 2.0), spread_yaw=45.0), DEV) for i, m in enumerate((150, 131, 144))]
    assert len({int(f["processed_lidar"]["voxel_features"].shape[0]) for f in frames}) == 3
    meta = {"ego": {"transformation_matrix": torch.eye(4, device=DEV), "anchor_box": anchors}}
    with torch.no_grad():
        want = [pp.post_process(meta, {"ego": model(f)}) for f in frames]
    assert sum(0 if b is None else b.shape[0] for b, _ in want) > 0
    pipe = pl_mod.FramePipeline(model, build_postprocessor(h["postprocess"], False), anchors, lanes=1, result_lag=0, graph=True, device=DEV)
    try:
        got = pipe.run(frames)
        assert pipe._records_ok and (pipe.frames_in_place, pipe.frames_copied) == (3, 0)
        assert all(s.record is not None for d in pipe._slots for s in d.values())
        for i, (g, w) in enumerate(zip(got, want)):
            assert _same(g, w), f"frame {i}"
    finally:
        pipe.close()


def test_encode_and_compressor_inside_a_captured_graph_replay_to_the_same_bits(world):
    """Pillar op -> sp_pack_rows -> narrow kernel on the sparse canvas -> decoder, captured by ``torch.cuda.graph``: replays reproduce eager bit for bit, also after
    the content of the input arrays changed (every replay is a new frame tag on the same stamp map)."""
    h, model = world["hypes"], world["model"]
    pls = [to_device(make_frame(h, 2, pillars_per_agent=150, seed=80 + i), DEV)["processed_lidar"] for i in range(2)]
    arrays = [(p["voxel_features"].float().contiguous(), p["voxel_num_points"].to(torch.int32).contiguous(), p["voxel_coords"].to(torch.int32).contiguous()) for p in pls]
    assert arrays[0][0].shape == arrays[1][0].shape and not torch.equal(arrays[0][2], arrays[1][2])
    vfe = model.pillar_vfe

    def body(vf, npts, coords):
        keep, vfe.sparse_canvas = vfe.sparse_canvas, True
        try:
            bd = model.scatter(vfe({"voxel_features": vf, "voxel_num_points": npts, "voxel_coords": coords, "record_len": [2]}))
        finally:
            vfe.sparse_canvas = keep
        assert isinstance(bd["spatial_features"], ops.SparseCanvas)
        return model.naive_compressor(bd["spatial_features"], out_split=True).data
    stream = torch.cuda.Stream(device=DEV)
    with torch.no_grad(), torch.cuda.stream(stream):
        eager = [body(*a).clone() for a in arrays]                   # (also the warm-up: weight images, folded parameters, the stamp map, the range word)
        assert not torch.equal(eager[0], eager[1])
        static = [t.clone() for t in arrays[0]]
        stream.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            out = body(*static)
        for i in (0, 1, 1, 0):
            for s, t in zip(static, arrays[i]):
                s.copy_(t)
            graph.replay()
            stream.synchronize()
            assert torch.equal(out, eager[i]), i
    torch.cuda.synchronize()
