"""Stage 1 of all agents in one pass on the MI355X (include/coalign_amd_stage1.h): ``post_process_stage1_device`` and the direct ``ops.stage1_boxes`` call
against ``post_process_stage1`` -- the host read-back on the per-agent kernels -- bit for bit: corners, uncertainties, counts and the status word.

Shapes: the mini stage-1 config with its range trimmed to a 15 x 31 x 2 head grid (930 anchors, no multiple of the 256-anchor decode block: with a wrong
segmentation a block would straddle two agents), the untrimmed 16 x 32 x 2 grid where every anchor passes (1024 candidates > NMS_TOP) and the DAIR 100 x 252 x 2
grid for the store overflow.  The launch count (count, emit, rank, mask, reduce: five for any number of agents) is the entry point's documented sequence; the
library keeps no launch bookkeeping to assert it with."""
import copy
import functools

import numpy as np
import pytest
import torch

from coalign_amd import box_align, ops
from coalign_amd.config import builtin_config, load_point_pillar_params
from coalign_amd.pose import generate_noise
from coalign_amd.postprocess import NMS_TOP, build_postprocessor
from tests.test_pose_correction_gpu import NORM, _heads, _objects, _plant, _scene_views, _stage1

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
KEPT = {1: [65], 2: [64, 1], 5: [63, 130, 0, 65, 1], 8: [1, 64, 128, 0, 63, 130, 65, 129]}      # kept boxes per slot: all different, a zero in a middle slot
# (eight slots need eight different counts: the issue's {0, 1, 63, 64, 65, 130} plus 128 and 129, the next 64-wide tile edge)


@functools.lru_cache(maxsize=None)
def _mini(trimmed: bool):
    h = copy.deepcopy(builtin_config("mini_pointpillar_uncertainty"))
    if trimmed:
        rng = [-12.4, -6.0, -3, 12.4, 6.0, 1]                       # 62 x 30 voxels of 0.4 m -> a 31 x 15 head grid
        h["preprocess"]["cav_lidar_range"] = rng
        h["model"]["args"]["lidar_range"] = rng
        h["postprocess"]["anchor_args"]["cav_lidar_range"] = rng
        h["postprocess"]["gt_range"] = rng
        h = load_point_pillar_params(h)
    pp = build_postprocessor(h["postprocess"], False)
    anchors = pp.generate_anchor_box()
    assert anchors.shape[:3] == ((15, 31, 2) if trimmed else (16, 32, 2))
    return pp, anchors, torch.from_numpy(anchors)


def _cells(anchors, k, rs, size=(1.56, 0.3, 0.6)):
    """``k`` small boxes on ``k`` different anchor cells (0.8 m apart: 0.6 x 0.3 m boxes do not overlap), yaw 0 or 90 degrees."""
    H, W = anchors.shape[:2]
    pick = rs.permutation(H * W)[:k]
    obj = np.zeros((k, 7))
    obj[:, 0], obj[:, 1] = anchors[pick // W, pick % W, 0, 0], anchors[pick // W, pick % W, 0, 1]
    obj[:, 2], obj[:, 3:6], obj[:, 6] = -1.0, size, rs.randint(0, 2, k) * (np.pi / 2)
    return obj


def _planted(anchors, object_lists, rs, udim=3, with_dir=False, logits=None):
    """Head maps of ``len(object_lists)`` agents (``_plant`` per agent).  ``logits[i]``: None = +4 at every planted anchor (equal scores), else a range the
    planted anchors' logits are drawn from."""
    parts = [_plant(obj, anchors, rs) for obj in object_lists]
    H, W, A, _ = anchors.shape
    cls = np.concatenate([p[0] for p in parts])
    for i, lg in enumerate(logits or []):
        if lg is not None:
            on = cls[i] > 0
            cls[i][on] = rs.uniform(lg[0], lg[1], int(on.sum())).astype(np.float32)
    heads = {"cls_preds": cls, "reg_preds": np.concatenate([p[1] for p in parts]),
             "unc_preds": rs.normal(-2.0, 0.3, (len(parts), A * max(udim, 1), H, W)).astype(np.float32)}
    if with_dir:
        heads["dir_preds"] = rs.normal(0, 1, (len(parts), A * 2, H, W)).astype(np.float32)
    return {k: torch.from_numpy(v).to(DEV) for k, v in heads.items()}


def _reference(pp, heads, a1):
    """``post_process_stage1`` -> (corners per agent, uncertainties per agent) as numpy, empty arrays when nothing passes anywhere."""
    n, udim = heads["cls_preds"].shape[0], heads["unc_preds"].shape[1] // heads["cls_preds"].shape[1]
    c, _, u = pp.post_process_stage1(heads, a1)
    if c is None:
        return [np.zeros((0, 8, 3), np.float32)] * n, [np.zeros((0, udim), np.float32)] * n
    return [x.cpu().numpy() for x in c], [x.cpu().numpy() for x in u]


def _direct(pp, heads, a1, store, unc="heads"):
    A, H, W = heads["cls_preds"].shape[1:]
    n = heads["cls_preds"].shape[0]
    ws = ops.stage1_workspace(n, A, H, W, NMS_TOP, DEV)
    da = pp.params["dir_args"]
    ops.stage1_boxes(heads["cls_preds"], heads["reg_preds"], heads.get("dir_preds"), heads["unc_preds"] if unc == "heads" else unc, pp._anchors_f32(a1, DEV), store, ws,
                     pp.params["target_args"]["score_threshold"], da["dir_offset"], da["num_bins"], pp.params["order"], pp.params["nms_thresh"], NMS_TOP)
    return ws


def _check(store, ref_c, ref_u, what, check_unc=True):
    torch.cuda.synchronize()
    n = len(ref_c)
    counts = store.count.cpu().numpy()
    want = [min(len(c), store.boxes) for c in ref_c]
    print(f"{what}: kept {[len(c) for c in ref_c]} store {list(counts[:n])} status {int(store.status[0])}")
    assert list(counts[:n]) == want, what
    assert int(store.status[0]) == (ops.ALIGN_STORE_OVERFLOW if any(len(c) > store.boxes for c in ref_c) else 0), what
    for i in range(n):
        assert np.array_equal(store.corners[i, : want[i]].cpu().numpy(), ref_c[i][: want[i]]), (what, i)
        if check_unc and store.udim:
            assert np.array_equal(store.unc[i, : want[i]].cpu().numpy(), ref_u[i][: want[i]]), (what, i)


def _poison(store):
    """Leave values no kernel writes in the store, so that a slot the pass did not write shows."""
    store.corners.fill_(float("nan"))
    store.unc.fill_(float("nan"))
    store.words.fill_(-7)


@pytest.mark.parametrize("n_agents", [1, 2, 5, 8])
def test_batched_pass_equals_the_per_agent_read_back(n_agents):
    """Per-agent kept counts across the 64-wide tile edges and the segment offsets, on the 15 x 31 x 2 grid; direction head present."""
    pp, anchors, a1 = _mini(True)
    rs = np.random.RandomState(10 + n_agents)
    heads = _planted(anchors, [_cells(anchors, k, rs) for k in KEPT[n_agents]], rs, with_dir=True)
    ref_c, ref_u = _reference(pp, heads, a1)
    assert [len(c) for c in ref_c] == KEPT[n_agents]
    store = ops.Stage1Store(DEV, 3)
    _poison(store)
    assert pp.post_process_stage1_device(heads, a1, store) is store and store.n_agents == n_agents
    _check(store, ref_c, ref_u, f"{n_agents} agents, post_process_stage1_device")
    assert (store.count[n_agents:] == -7).all()                                     # slots beyond the frame's agents are left as they are
    _poison(store)
    _direct(pp, heads, a1, store)
    _check(store, ref_c, ref_u, f"{n_agents} agents, ops.stage1_boxes")


def test_overlap_ties_and_the_top_cut():
    """One agent of heavily overlapping boxes with different scores (suppression across tile boundaries), one with equal scores (the index-descending tie rule),
    one empty, one of small boxes; then the 16 x 32 x 2 grid with every anchor of one agent passing: 1024 candidates, the ``top`` cut at 1000."""
    pp, anchors, a1 = _mini(True)
    rs = np.random.RandomState(3)
    big = (1.56, 1.6, 3.9)
    lists = [_cells(anchors, 300, rs, big), _cells(anchors, 5, rs), _cells(anchors, 0, rs), _cells(anchors, 300, rs, big)]
    heads = _planted(anchors, lists, rs, logits=[(0.5, 5.0), None, None, None])
    ref_c, ref_u = _reference(pp, heads, a1)
    assert 10 < len(ref_c[0]) < 250 and 10 < len(ref_c[3]) < 250 and len(ref_c[1]) == 5 and len(ref_c[2]) == 0
    store = ops.Stage1Store(DEV, 3)
    _poison(store)
    pp.post_process_stage1_device(heads, a1, store)
    _check(store, ref_c, ref_u, "overlap / ties")
    pp, anchors, a1 = _mini(False)
    heads = _planted(anchors, [_cells(anchors, 3, rs), _cells(anchors, 0, rs)], rs, with_dir=True)
    heads["cls_preds"][1] = torch.from_numpy(rs.uniform(-1.0, 4.0, (2, 16, 32)).astype(np.float32)).to(DEV)      # sigmoid(-1) = 0.27 > 0.2: every anchor passes
    heads["reg_preds"][1] = torch.from_numpy(rs.normal(0, 0.3, (14, 16, 32)).astype(np.float32)).to(DEV)
    ref_c, ref_u = _reference(pp, heads, a1)
    assert int((torch.sigmoid(heads["cls_preds"][1]) > 0.2).sum()) == 1024 > NMS_TOP and len(ref_c[1]) > 20
    _poison(store)
    pp.post_process_stage1_device(heads, a1, store)
    _check(store, ref_c, ref_u, "top cut")


@pytest.mark.parametrize("udim", [0, 2, 3])
@pytest.mark.parametrize("with_dir", [False, True])
def test_uncertainty_dimension_and_direction_head(udim, with_dir):
    pp, anchors, a1 = _mini(True)
    rs = np.random.RandomState(20 + udim)
    heads = _planted(anchors, [_cells(anchors, 70, rs), _cells(anchors, 9, rs)], rs, udim=udim, with_dir=with_dir)
    ref_c, ref_u = _reference(pp, heads, a1)          # (udim 0: the reference reads a one-channel map; only its corners and counts are compared)
    store = ops.Stage1Store(DEV, udim)
    _poison(store)
    _direct(pp, heads, a1, store, unc="heads" if udim else None)
    _check(store, ref_c, ref_u, f"udim {udim} dir {with_dir}", check_unc=udim > 0)
    if udim:
        _poison(store)
        pp.post_process_stage1_device(heads, a1, store)
        _check(store, ref_c, ref_u, f"udim {udim} dir {with_dir}, post_process_stage1_device")
    else:
        with pytest.raises(ValueError):
            _direct(pp, heads, a1, ops.Stage1Store(DEV, 3), unc=None)                 # the store's udim and the maps' disagree


def test_channel_slices_of_a_merged_heads_tensor_are_read_in_place():
    """A detector with merged heads returns cls / reg / dir / unc as channel slices of one [n, C, H, W] tensor: every agent's maps dense, the agents C * H * W floats
    apart.  The pass takes them through ``coalign_stage1_boxes_strided`` and gives what it gives on dense copies."""
    pp, anchors, a1 = _mini(True)
    rs = np.random.RandomState(31)
    dense = _planted(anchors, [_cells(anchors, 66, rs), _cells(anchors, 0, rs), _cells(anchors, 129, rs)], rs, with_dir=True, logits=[(0.5, 5.0)] * 3)
    names = ("cls_preds", "reg_preds", "dir_preds", "unc_preds")
    merged = torch.cat([dense[k] for k in names], dim=1)
    heads, c0 = {}, 0
    for k in names:
        heads[k] = merged[:, c0: c0 + dense[k].shape[1]]
        c0 += dense[k].shape[1]
    assert not heads["reg_preds"].is_contiguous() and heads["reg_preds"][0].is_contiguous()
    ref_c, ref_u = _reference(pp, dense, a1)
    store = ops.Stage1Store(DEV, 3)
    _poison(store)
    pp.post_process_stage1_device(heads, a1, store)
    _check(store, ref_c, ref_u, "channel slices")


def test_store_overflow_and_nothing_passes_through_the_corrector():
    """The DAIR 100 x 252 x 2 grid: an agent with more kept boxes than a slot holds (the 300-box crowd) -> the overflow bit, the first 256 equal, and ``correct``
    gives ``ALIGN_OUTSIDE_LIMITS | ALIGN_STORE_OVERFLOW`` with the noisy poses bit for bit; nothing passes in any agent -> counts 0, ``ALIGN_NO_BOXES``."""
    h1, pp1, anchors, a1 = _stage1()
    rs = np.random.RandomState(9)
    rngd = h1["postprocess"]["anchor_args"]["cav_lidar_range"]
    clean = [np.zeros(6), np.array([12.0, 3.0, 0, 0, 25.0, 0]), np.array([-9.0, -4.0, 0, 0, -30.0, 0])]
    views = _scene_views(clean, rs, rngd)
    gx, gy = np.meshgrid(np.arange(-90, 90, 6.0), np.arange(-31.5, 32, 7.0))
    crowd = _objects(np.stack([gx.ravel(), gy.ravel()], 1), np.zeros(gx.size))
    over = _heads([views[0], crowd, views[2]], anchors, rs)
    ref_c, _, ref_u = pp1.post_process_stage1(over, a1)
    ref_c, ref_u = [c.cpu().numpy() for c in ref_c], [u.cpu().numpy() for u in ref_u]
    corrector = box_align.PoseCorrector(dict(abandon_hard_cases=True, drop_hard_boxes=True), 5, device=DEV, **NORM)
    assert len(ref_c[1]) > corrector.store.boxes
    noisy = torch.from_numpy(np.array([p + generate_noise(0.2, 0.2, rng=rs) for p in clean])).to(DEV)
    _poison(corrector.store)
    store = pp1.post_process_stage1_device(over, a1, corrector.store)
    out = corrector.correct(store, noisy)
    torch.cuda.synchronize()
    assert int(out["status"][0]) == ops.ALIGN_OUTSIDE_LIMITS | ops.ALIGN_STORE_OVERFLOW and torch.equal(out["lidar_poses"], noisy)
    store = pp1.post_process_stage1_device(over, a1, corrector.store)              # (correct rewrote the status word: fill again for the comparison)
    _check(store, ref_c, ref_u, "store overflow")
    nothing = _heads([v[:0] for v in views], anchors, rs)
    store = pp1.post_process_stage1_device(nothing, a1, corrector.store)
    _check(store, [np.zeros((0, 8, 3), np.float32)] * 3, [np.zeros((0, 3), np.float32)] * 3, "nothing passes")
    out = corrector.correct(store, noisy)
    torch.cuda.synchronize()
    assert int(store.count[:3].sum()) == 0 and int(out["status"][0]) == ops.ALIGN_NO_BOXES and torch.equal(out["lidar_poses"], noisy)


def test_captured_pass_replays_bit_equal():
    """``ops.stage1_boxes`` captured in a ``torch.cuda.graph`` (workspace and anchors exist: no allocation, no synchronisation inside) and replayed three times
    with other planted maps equals the eager results bit for bit."""
    pp, anchors, a1 = _mini(True)
    rs = np.random.RandomState(5)
    inputs = [_planted(anchors, [_cells(anchors, k, rs) for k in ks], rs, with_dir=True, logits=[(0.5, 5.0)] * 3)
              for ks in ([64, 0, 130], [5, 65, 1], [300, 63, 64])]
    static = {k: v.clone() for k, v in inputs[0].items()}
    store = ops.Stage1Store(DEV, 3)
    stream = torch.cuda.Stream(device=DEV)
    eager = []
    with torch.cuda.stream(stream):
        for inp in inputs:
            _poison(store)
            pp.post_process_stage1_device(inp, a1, store)
            stream.synchronize()
            eager.append((store.corners.clone(), store.unc.clone(), store.words.clone()))
        for k in static:
            static[k].copy_(inputs[0][k])
        pp.post_process_stage1_device(static, a1, store)                             # warm-up on the static maps (their workspace exists from the eager calls)
        stream.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            pp.post_process_stage1_device(static, a1, store)
        for i in (1, 2, 0):
            for k in static:
                static[k].copy_(inputs[i][k])
            _poison(store)
            graph.replay()
            stream.synchronize()
            counts = eager[i][2][:3].tolist()
            assert torch.equal(store.words[:3], eager[i][2][:3]) and int(store.status[0]) == int(eager[i][2][8]), i
            for a, c in enumerate(counts):
                assert torch.equal(store.corners[a, :c], eager[i][0][a, :c]) and torch.equal(store.unc[a, :c], eager[i][1][a, :c]), (i, a)
    torch.cuda.synchronize()
