"""Every pillar encoder at its run, shape and range limits against float64 (csrc/pillar_scatter.hip, csrc/pillar_sparse.hip; all through coalign_amd.ops / the C ABI).

Each case of tests/pillar_cases.py runs through EVERY entry point that accepts its flags and shape -- the NCHW op, the channels-last op, the persistent canvas, the
device-count stream form, the sparse encoder with a host count, a device count and a frame record; an entry that does not accept a case must refuse it the way it
documents.  Per entry: the feature rows against ``pfn_f64`` under the project's bound (``pillar_cases.assert_bound``), the canvas bit-equal to ``oracle.scatter`` of
those rows (the sparse forms densified through their stamps, as the consumers read them).  tests/test_pillar_limits_cpu.py proves on the CPU that the reference's
float32 arithmetic meets the same bound on every one of these inputs."""
import types

import pytest
import torch

from oracle import coalign_oracle as oracle
from coalign_amd import hip, ops
from tests import pillar_cases as pc
from tests.pillar_reference import BN_EPS, PREFIX
from tests.test_hip_parity import run_pillar
from tests.test_round3_gpu import _run_pillar
from tests.test_round4_gpu import _sparse_encode

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PAD = 5                       # rows of capacity beyond the count in the device-count forms (garbage the kernels must not touch)
BN_KEYS = ("norm.weight", "norm.bias", "norm.running_mean", "norm.running_var")
_REFS = {}


def _cus():
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def _refs(case):
    """(float64 yardstick, float32 reference) of a case: computed once, shared by all entries, never modified."""
    if case.name not in _REFS:
        _REFS.clear()
        _REFS[case.name] = (pc.want64(case), pc.ref32(case))
    return _REFS[case.name]


def _params(case):
    w = case.sd[PREFIX + "linear.weight"].to(DEV)
    bn = tuple(case.sd[PREFIX + k].to(DEV) for k in BN_KEYS) if case.use_norm else None
    bias = None if case.use_norm else case.sd[PREFIX + "linear.bias"].to(DEV)
    return w, bias, bn


def _dense_args(case, pl):
    w, bias, bn = _params(case)
    return (pl["voxel_features"].to(DEV), pl["voxel_num_points"].to(DEV), pl["voxel_coords"].to(DEV), w, bias, bn, BN_EPS, case.use_abs, case.with_dist, case.voxel_size, case.lidar_range[:3],
            case.n_agents, case.ny, case.nx)


def _padded(case):
    """Capacity-sized arrays: the case's pillars, then PAD rows of garbage (huge points, a count, the FIRST pillar's cell) that lie beyond the device-side count."""
    vf = torch.cat([case.vf, torch.full((PAD, case.P, 4), 1.0e3)])
    npts = torch.cat([case.npts, torch.full((PAD,), min(7, case.P), dtype=torch.int32)])
    coords = torch.cat([case.coords, case.coords[:1].expand(PAD, 4)])
    return {"voxel_features": vf.to(DEV), "voxel_num_points": npts.to(DEV), "voxel_coords": coords.to(DEV)}


def _model_shim(case):
    """What ``_sparse_encode`` reads of a model: the PFN layer's Linear weight and BatchNorm tensors on the device."""
    ns = types.SimpleNamespace
    pfn = ns(linear=ns(weight=case.sd[PREFIX + "linear.weight"].to(DEV)), norm=ns(weight=case.sd[PREFIX + "norm.weight"].to(DEV), bias=case.sd[PREFIX + "norm.bias"].to(DEV),
                                                                                  running_mean=case.sd[PREFIX + "norm.running_mean"].to(DEV),
                                                                                  running_var=case.sd[PREFIX + "norm.running_var"].to(DEV)))
    return ns(pillar_vfe=ns(pfn_layers=[pfn]))


def _sparse(case, pl, cache, count_dev=None, frame=None):
    if case.default_flags and frame is None:
        return _sparse_encode(_model_shim(case), case.margs, pl, case.n_agents, cache, count_dev=count_dev)
    w, bias, bn = _params(case)
    return ops.pillar_encode_sparse(pl["voxel_features"].to(DEV), pl["voxel_num_points"].to(DEV), pl["voxel_coords"].to(DEV), w, bias, bn, BN_EPS, case.use_abs,
                                    case.voxel_size, case.lidar_range[:3], case.n_agents, case.ny, case.nx, canvas_cache=cache, count_dev=count_dev, frame=frame)


def _densify(stamps, state, feats_cpu, case):
    """The canvas as the sparse consumers see it: a cell is occupied iff its stamp carries the tag of the last completed frame, and then names its row."""
    st = stamps.view(case.n_agents, case.ny, case.nx).cpu()
    occ = (st >> 32) == int(state[0].item())
    rows = (st & 0xFFFFFFFF)[occ]
    assert rows.numel() == 0 or int(rows.max()) < feats_cpu.shape[0]
    seen = torch.zeros(case.n_agents, case.ny, case.nx, feats_cpu.shape[1])
    seen[occ] = feats_cpu[rows]
    return seen.permute(0, 3, 1, 2)


def _check(case, label, feats, canvas):
    want, ref = _refs(case)
    M = case.M
    rows = feats[:M].cpu()
    assert rows.shape == (M, case.C), (case.name, label, tuple(feats.shape))
    pc.assert_bound(rows, want, ref, f"{case.name} {label}")
    assert torch.equal(canvas.contiguous().cpu(), oracle.scatter(rows, case.coords, case.n_agents, case.nx, case.ny)), (case.name, label, "canvas != scatter of the rows")


def run_every_entry(case):
    """-> the labels of the entries that ran.  Every other entry was asked too and refused the case as documented."""
    ran = []
    pl = case.pl
    P, C = case.P, case.C
    # ---- (1) NCHW: any P, any C, every flag
    feats, canvas = run_pillar(case.vf, case.npts, case.coords, case.sd, case.margs, case.n_agents) if case.default_flags else ops.pillar_vfe_scatter(*_dense_args(case, pl))
    _check(case, "nchw", feats, canvas)
    ran.append("nchw")
    # ---- (2) channels-last: P <= 32, C <= 64 (ops routes anything else, and the layout-ambiguous C == 1, to the NCHW entry: the C ABI's refusal is
    #      test_entry_points_refuse_what_they_document)
    if case.use_norm and not case.with_dist:
        feats, canvas = _run_pillar(pl, case.sd, case.margs, case.n_agents, True, use_abs=case.use_abs)
    else:
        feats, canvas = ops.pillar_vfe_scatter(*_dense_args(case, pl), channels_last=True)
    nhwc_ok = P <= 32 and 1 < C <= 64
    assert ops.is_channels_last(canvas) == nhwc_ok or C == 1, (case.name, "channels-last routing")
    _check(case, "nhwc", feats, canvas)
    ran.append("nhwc")
    # ---- (3) persistent canvas: additionally C % 4 == 0.  Twice through one cache: the second call clears exactly what the first one wrote
    cache = {}
    persistent_ok = nhwc_ok and C % 4 == 0
    for _ in range(2):
        feats, canvas = ops.pillar_vfe_scatter(*_dense_args(case, pl), channels_last=True, canvas_cache=cache)
    assert bool(cache) == persistent_ok, (case.name, "persistent routing")           # (refused shapes took the fresh-canvas entry: nothing was cached)
    if persistent_ok:
        _check(case, "persistent", feats, canvas)
        ran.append("persistent")
    # ---- (4) stream: the count on the device, capacity-sized arrays
    cap = _padded(case)
    cnt = torch.tensor([case.M], dtype=torch.int32, device=DEV)
    w, bias, bn = _params(case)
    stream_args = (cap["voxel_features"], cap["voxel_num_points"], cap["voxel_coords"], cnt, w, bias, bn, BN_EPS, case.use_abs, case.with_dist, case.voxel_size,
                   case.lidar_range[:3], case.n_agents, case.ny, case.nx)
    if P <= 32 and C <= 64 and C % 4 == 0:
        cache = {}
        for _ in range(2):
            feats, canvas = ops.pillar_encode_stream(*stream_args, cache, unique_cells=True, want_features=True)
        _check(case, "stream", feats, canvas)
        ran.append("stream")
    else:
        with pytest.raises(hip.CoalignHipError):
            ops.pillar_encode_stream(*stream_args, {}, unique_cells=True, want_features=True)
    # ---- (5-7) sparse: P <= 32, C <= 64; the entry has no distance flag at all (coalign_amd.h (1b): "with_distance configs use (1)"), so such a case cannot be put to it
    if case.with_dist:
        return ran
    if P > 32 or C > 64:
        with pytest.raises(hip.CoalignHipError):
            _sparse(case, pl, {})
        return ran
    sc = _sparse(case, pl, {})
    _check(case, "sparse", sc.feats, _densify(sc.stamps, sc.state, sc.feats.cpu(), case))
    sc = _sparse(case, cap, {}, count_dev=cnt)
    assert sc.feats.shape[0] == case.M + PAD
    _check(case, "sparse count_dev", sc.feats, _densify(sc.stamps, sc.state, sc.feats[:case.M].cpu(), case))
    blob, host = torch.zeros(4, dtype=torch.int64, device=DEV), torch.zeros(4, dtype=torch.int64).pin_memory()
    rec = ops.PillarFrameRecord(blob, host, case.M + PAD)
    dpl = {k: v.to(DEV) for k, v in pl.items()}
    assert ops.PillarFrameRecord.admits(dpl["voxel_features"], dpl["voxel_num_points"], dpl["voxel_coords"], torch.device(DEV))
    rec.set(dpl["voxel_features"], dpl["voxel_num_points"], dpl["voxel_coords"])
    blob.copy_(host, non_blocking=True)
    sc = _sparse(case, dpl, {}, frame=rec)
    torch.cuda.synchronize()
    assert sc.feats.shape[0] == case.M + PAD
    _check(case, "sparse frame record", sc.feats, _densify(sc.stamps, sc.state, sc.feats[:case.M].cpu(), case))
    return ran + ["sparse", "sparse count_dev", "sparse frame record"]


ALL_ENTRIES = ["nchw", "nhwc", "persistent", "stream", "sparse", "sparse count_dev", "sparse frame record"]


# ---------------------------------------------------------------------------------------------------------------- (a) small counts
@pytest.mark.parametrize("name", pc.names("a"))
def test_small_pillar_counts(name):
    """M = 1 .. 81 at P = 32, C = 64: one wavefront of the sparse kernel takes 1 .. 6 pairs, then its ``active`` partition splits them; one workgroup of the dense
    channels-last kernel takes runs of 1 .. 10 pairs per wavefront and a second workgroup starts at M = 81.  An odd M ends in a full pillar without a partner."""
    assert run_every_entry(pc.get_case(name)) == ALL_ENTRIES


# ---------------------------------------------------------------------------------------------------------------- (b) run lengths on the round boundaries
def test_run_lengths_hold_on_this_device():
    """The pillar counts of group b give their run lengths with the CU count THIS device reports (the sparse launcher sizes its grid by it)."""
    pc.check_run_lengths(_cus())


@pytest.mark.parametrize("name", pc.names("b"))
def test_run_lengths_on_the_round_boundaries(name):
    """A wavefront's run ends exactly on / one pair past an LDS round (sparse: rounds of 4, two issued up front, pairs grouped by 2; dense: rounds of 5), fills all
    32 record slots, and the count one pair above adds workgroups; each M also as M - 1, the odd tail inside the last group.  P = 8: padded point slots (P < 32)."""
    cus = _cus()
    case = pc.get_case(name, cus)
    r, kind = case.info["run"], case.info["kind"]
    blocks, lo, hi = pc.sparse_launch(case.M, cus)
    dblocks, drun = pc.dense_launch(case.M)
    if kind == "sparse":
        assert (lo, hi, blocks) == (r, r, 3 * cus) if r else (blocks > 3 * cus and hi <= pc.SPARSE_RUN_MAX), (name, blocks, lo, hi)
    else:
        assert (dblocks, drun) == (512, r) if r else (dblocks > 512 and drun <= pc.DENSE_RUN_MAX), (name, dblocks, drun)
    assert run_every_entry(case) == ALL_ENTRIES


# ---------------------------------------------------------------------------------------------------------------- (c) device counts far below the capacity
CANARY = 12345.0


@pytest.fixture(scope="module")
def capacity_world():
    cus = _cus()
    case = pc.get_case("c_capacity", cus)
    assert case.M == 12 * cus * 16
    w, bias, bn = _params(case)
    dev = {k: v.to(DEV) for k, v in case.pl.items()}
    return case, dev, ops.pillar_fold_params(w, bias, bn, BN_EPS, True), pc.want64(case), pc.ref32(case)


@pytest.mark.parametrize("form", ["count_dev", "frame_record"])
@pytest.mark.parametrize("count", [0, 1, 2, 11, 12, 13, -1, "capacity"])
def test_device_count_far_below_the_capacity(capacity_world, count, form):
    """Capacity 12 x CUs x 16 pillars, the count on the device: rows [0, count) against float64, the rows beyond keep the canary they were filled with, the stamps
    densify to the scatter of the valid rows, and the frame tag advances by exactly one per launch (count 0 included) with every arrival counter back at zero."""
    case, dev, folded, want, ref = capacity_world
    cap = case.M
    n = cap if count == "capacity" else cap - 1 if count == -1 else count
    L = hip.lib()
    feats = torch.full((cap, case.C), CANARY, device=DEV)
    stamps = torch.zeros(case.n_agents * case.ny * case.nx, dtype=torch.int64, device=DEV)
    state = torch.zeros(L.coalign_sparse_canvas_state_bytes() // 4, dtype=torch.int32, device=DEV)
    cnt = torch.tensor([n], dtype=torch.int32, device=DEV)
    words = torch.tensor([dev["voxel_features"].data_ptr(), dev["voxel_num_points"].data_ptr(), dev["voxel_coords"].data_ptr(), n], dtype=torch.int64, device=DEV)
    tail = (case.P, ops._ptr(folded), case.C, 1, ops._dbl3(case.voxel_size), ops._dbl3(case.lidar_range[:3]), case.n_agents, case.ny, case.nx, ops._ptr(feats), ops._ptr(stamps),
            ops._ptr(state), ops._stream())
    first = None
    for launch in (1, 2):
        if form == "count_dev":
            rc = L.coalign_pillar_encode_sparse(ops._ptr(dev["voxel_features"]), ops._ptr(dev["voxel_num_points"]), ops._ptr(dev["voxel_coords"]), cap, ops._ptr(cnt), *tail)
        else:
            rc = L.coalign_pillar_encode_sparse_frame(ops._ptr(words), cap, *tail)
        assert rc == 0, rc
        torch.cuda.synchronize()
        st = state.cpu()
        assert int(st[0]) == launch and int(st[1:].abs().sum()) == 0, (count, form, st[:2].tolist())
        assert bool((feats[n:] == CANARY).all()), (count, form, "rows beyond the count were written")
        rows = feats[:n].cpu()
        if n:
            pc.assert_bound(rows, want[:n], ref[:n], f"c count {n} {form} launch {launch}")
        assert torch.equal(_densify(stamps, state, rows, case), oracle.scatter(rows, case.coords[:n], case.n_agents, case.nx, case.ny))
        assert first is None or torch.equal(first, rows)
        first = rows


# ---------------------------------------------------------------------------------------------------------------- (d) shapes and flags
@pytest.mark.parametrize("name", [n for n in pc.names("d") if pc.table()[n]["use_abs"] and not pc.table()[n]["with_dist"] and pc.table()[n]["use_norm"]])
def test_shapes_with_the_default_flags(name):
    """P in 1 .. 65, C in 1 .. 128 at M = 41 with the product's flags (also run on the VALU route by tests/test_round3_gpu.py's subprocess test)."""
    _shape_case(name)


@pytest.mark.parametrize("name", [n for n in pc.names("d") if not (pc.table()[n]["use_abs"] and not pc.table()[n]["with_dist"] and pc.table()[n]["use_norm"])])
def test_shapes_and_flags(name):
    """The same shapes with use_absolute_xyz off, the distance feature on, a Linear bias instead of BatchNorm; 4 m and 5 m cells."""
    _shape_case(name)


def _shape_case(name):
    case = pc.get_case(name)
    P, C = case.P, case.C
    expect = ["nchw", "nhwc"]
    if P <= 32 and C <= 64 and C % 4 == 0:
        expect += (["persistent"] if C > 1 else []) + ["stream"]
    if P <= 32 and C <= 64 and not case.with_dist:
        expect += ALL_ENTRIES[4:]
    assert run_every_entry(case) == expect, name


def test_entry_points_refuse_what_they_document():
    """The C ABI's own answers to shapes outside an entry (the ops layer routes or raises before it gets there): COALIGN_ERR_UNSUPPORTED (-3) from the channels-last
    entry for P > 32 or C > 64, COALIGN_ERR_BAD_SHAPE (-2) from the persistent and the stream entry for P > 32, C > 64 or C % 4, and from the sparse encoder and its
    parameter fold for P > 32 or C > 64.  Nothing is launched: every refusal comes before the first kernel."""
    L = hip.lib()
    z = torch.zeros(4096, device=DEV)
    p = ops._ptr(z)
    vs, rm = ops._dbl3([0.4, 0.4, 4.0]), ops._dbl3([-3.2, -1.6, -3.0])
    ws = L.coalign_pillar_scatter_workspace_bytes(1, 8, 16)
    for P, C, persistent_rc, nhwc_rc in ((33, 64, -2, -3), (32, 65, -2, -3), (32, 63, -2, None), (32, 2, -2, None)):
        head = (p, p, p, 0, P, p, None, p, p, p, p, 1e-3, C, 1, 0, vs, rm, 1, 8, 16, p)
        if nhwc_rc is not None:
            assert L.coalign_pillar_vfe_scatter_nhwc(*head, p, p, ws, None) == nhwc_rc, (P, C)
        assert L.coalign_pillar_encode_persistent(*head, p, 0, p, p, None) == persistent_rc, (P, C)
        assert L.coalign_pillar_encode_stream(p, p, p, 1, p, P, p, None, p, p, p, p, 1e-3, C, 1, 0, vs, rm, 1, 8, 16, p, p, p, p, 1, None) == persistent_rc, (P, C)
    for P, C in ((33, 64), (32, 65)):
        assert L.coalign_pillar_encode_sparse(p, p, p, 1, None, P, p, C, 1, vs, rm, 1, 8, 16, p, p, p, None) == -2, (P, C)
    assert L.coalign_pillar_fold_params(p, None, p, p, p, p, 1e-3, 65, 1, p, None) == -2
    assert float(z.abs().sum()) == 0.0


# ---------------------------------------------------------------------------------------------------------------- (e) input range
@pytest.mark.parametrize("name", pc.names("e"))
def test_input_range(name):
    """Coinciding points (offsets to the mean exactly zero, low terms of the fp16 split zero or subnormal), points within 1e-4 m, points on the cell faces and the z
    ends of 4 m and 5 m cells, intensities 0 / 1 / 255, pillars in the four corners of the full range (|centre| ~ 140 m: the per-pillar bracket is large and cancels),
    channels whose summed weights vanish (with and without a BatchNorm shift) or span 2^-20 .. 1, negative BatchNorm scales on both kinds; at M = 41 and on a sparse
    round boundary.  All inside the range the encoders state; nothing beyond it is fed."""
    case = pc.get_case(name, _cus())
    w = case.sd[PREFIX + "linear.weight"]
    B = 4 if case.use_abs else 1
    summed = (w[:, 0:3] if case.use_abs else 0) + w[:, B:B + 3] + w[:, B + 3:B + 6]
    assert float(summed[3:5].abs().max()) == 0.0 and float(w[3:5, 3 if case.use_abs else 0].abs().max()) == 0.0          # the degenerate channels are what they claim
    assert float(case.sd[PREFIX + "norm.weight"][3]) < 0 < float(case.sd[PREFIX + "norm.weight"][4]) and float(case.sd[PREFIX + "norm.weight"][6]) < 0
    assert float(case.vf[:, :, 3].max()) == 255.0
    expect = ALL_ENTRIES
    assert run_every_entry(case) == expect
