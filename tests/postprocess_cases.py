"""Helpers shared by tests/test_postprocess_cases_cpu.py and tests/test_postprocess_limits_gpu.py: seeded head outputs for the anchor decode
(csrc/decode.hip), a float64 restatement of the decode, and the lists of cases both files run.

A case is (cls [1, A, H, W], reg [1, 7A, H, W], dir [1, bins * A, H, W] | None, anchors [H, W, A, 7] float64, transform [4, 4] float32 | None) built from
(A, H, W, seed, density, options).  ``reference(spec)`` evaluates a case once with the float32 oracle (``oracle.decode_candidates`` + its two filters)
and with ``decode_f64`` and caches both; nothing here touches the GPU.

Two conditions keep the comparisons free of legitimate one-rounding flips:
  * score margin -- no sigmoid(cls) within 16 * 6e-8 of the threshold (``tests/test_hip_parity.py::_margin_ok``): a logit inside is MOVED to
    logit(thr) +- 0.01, never dropped;
  * discontinuity -- ``limit_period`` is ``v - floor(v / period + offset) * period``: a candidate whose floor argument lies within 1e-5 (about 100 float32
    roundings of it) of an integer may legitimately land one period away; it is left out of the VALUE comparisons only (never out of selection,
    order, index, score or keep flag), and at most 1 % of a case's candidates may be.
The keep flag has the same kind of edge (an extent within a rounding of 6, a z within a rounding of -3 / 1); ``keep_slack`` measures the distance
and the CPU file asserts that no case sits on it.
"""
import functools
import math
from collections import namedtuple

import numpy as np
import torch

from oracle import coalign_oracle as oracle

THR = 0.2
MARGIN = 16 * 6e-8                     # _margin_ok of tests/test_hip_parity.py
NEAR_INTEGER = 1e-5                    # the discontinuity condition
MAX_LEFT_OUT = 0.01                    # ... and its cap
KEEP_SLACK = 64 * 6e-8                 # keep-flag edges: relative to the candidate's scale
SCORE_RTOL = 3e-7                      # the existing decode tolerances (tests/test_hip_parity.py::test_decode_candidates_vs_oracle)
BOX7_TOL = dict(rtol=2e-6, atol=2e-6)
CORNER_TOL = dict(rtol=2e-6, atol=4e-6)
RANGE = [-140.8, -40.0, -3.0, 140.8, 40.0, 1.0]
YAWS = {1: [0], 2: [0, 90], 3: [0, 60, 120]}
TWO_PI_F32 = float(np.float32(2 * np.pi))
EXP_MAX = 88.72                        # log(FLT_MAX)

Spec = namedtuple("Spec", "A H W seed density order use_dir num_bins dir_offset transform tie_dir nonfinite")
Case = namedtuple("Case", "spec cls reg dir anchors transform passing")
Ref = namedtuple("Ref", "case idx scores box7 corners keep f64")


def spec(A, H, W, seed, density, order="hwl", use_dir=True, num_bins=2, dir_offset=0.7853, transform="none", tie_dir=False, nonfinite=None):
    return Spec(A, H, W, seed, density, order, use_dir, num_bins, dir_offset, transform, tie_dir, nonfinite)


def spec_id(s):
    d = s.density if isinstance(s.density, str) else f"{s.density:g}"
    parts = [f"{s.A}x{s.H}x{s.W}", d, f"s{s.seed}"]
    base = spec(s.A, s.H, s.W, s.seed, s.density)
    parts += [s.order] * (s.order != base.order) + ["nodir"] * (not s.use_dir) + [f"bins{s.num_bins}"] * (s.num_bins != 2)
    parts += [f"off{s.dir_offset:g}"] * (s.dir_offset != base.dir_offset) + [s.transform] * (s.transform != "none") + ["tie"] * s.tie_dir
    parts += [s.nonfinite] * (s.nonfinite is not None)
    return "-".join(parts)


# ------------------------------------------------------------------------------------------------ inputs
def anchors_for(A, H, W, order="hwl"):
    """oracle.generate_anchor_box over the OPV2V range at feature stride 1: [H, W, A, 7] float64."""
    args = dict(W=W, H=H, r=YAWS[A], vw=0.4, vh=0.4, cav_lidar_range=RANGE, feature_stride=1, l=3.9, w=1.6, h=1.56)
    return torch.from_numpy(oracle.generate_anchor_box(args, order))


def transform_of(kind):
    """None | identity | a rigid pose with a large translation | a general matrix without a zero entry (the last row is read by neither side).
    The translations keep x and y away from 0, so no projected coordinate is a small difference of large terms."""
    if kind == "none":
        return None
    if kind == "identity":
        return torch.eye(4)
    if kind == "rigid":
        c, s = math.cos(math.radians(30.0)), math.sin(math.radians(30.0))
        return torch.tensor([[c, -s, 0.0, 300.0], [s, c, 0.0, -250.0], [0.0, 0.0, 1.0, 0.3], [0.0, 0.0, 0.0, 1.0]], dtype=torch.float32)
    if kind == "rigid_b":
        c, s = math.cos(math.radians(-75.0)), math.sin(math.radians(-75.0))
        return torch.tensor([[c, -s, 0.0, -320.0], [s, c, 0.0, 280.0], [0.0, 0.0, 1.0, -0.2], [0.0, 0.0, 0.0, 1.0]], dtype=torch.float32)
    if kind == "general":
        return torch.tensor([[0.9, -0.3, 0.05, 300.0], [0.3, 0.9, -0.04, -250.0], [0.002, -0.003, 0.98, 0.1], [0.01, 0.02, 0.03, 1.5]], dtype=torch.float32)
    if kind == "near":                 # a neighbour a few metres away (the whole-chain cases on the mini range)
        c, s = math.cos(math.radians(12.0)), math.sin(math.radians(12.0))
        return torch.tensor([[c, -s, 0.0, 1.5], [s, c, 0.0, -0.8], [0.0, 0.0, 1.0, 0.05], [0.0, 0.0, 0.0, 1.0]], dtype=torch.float32)
    if kind == "near_b":
        c, s = math.cos(math.radians(-40.0)), math.sin(math.radians(-40.0))
        return torch.tensor([[c, -s, 0.0, -2.0], [s, c, 0.0, 1.1], [0.0, 0.0, 1.0, -0.05], [0.0, 0.0, 0.0, 1.0]], dtype=torch.float32)
    raise ValueError(kind)


def passing_mask(density, total, rs):
    """Which flat anchors (h, w, anchor order: what a thread of decode.hip indexes) pass the score threshold."""
    m = np.zeros(total, dtype=bool)
    lane = np.arange(total) % 256
    if density == "none":
        pass
    elif density == "all":
        m[:] = True
    elif density == "first":
        m[0] = True
    elif density == "last":
        m[-1] = True
    elif density == "seam":            # the last lane of wave 0 and the first lane of wave 1 of every block
        m[(lane == 63) | (lane == 64)] = True
    elif density == "blocks":          # block 0, block 256 and the very last anchor (the 257-block shapes)
        assert total > 256 * 256
        m[[3, 200, 255, 256 * 256, total - 1]] = True
        m[256 * 256 + 1: total - 1: 97] = True
    else:
        m = rs.uniform(size=total) < float(density)
    return m


def make_case(s, anchors=None):
    """The head outputs of one agent.  cls: |logit - logit(thr)| ~ |randn| on the side ``passing_mask`` asks for, then the margin rule;
    reg ~ 0.3 * randn; dir ~ randn (``tie_dir``: every bin of an anchor holds the same value; a quarter of them only the first two)."""
    A, H, W = s.A, s.H, s.W
    total = A * H * W
    rs = np.random.RandomState(s.seed)
    passing = passing_mask(s.density, total, rs)
    t0 = math.log(THR / (1 - THR))
    flat = t0 + np.where(passing, 1.0, -1.0) * np.abs(rs.randn(total))
    inside = np.abs(1.0 / (1.0 + np.exp(-flat.astype(np.float32).astype(np.float64))) - THR) <= MARGIN
    flat = np.where(inside, t0 + np.where(passing, 0.01, -0.01), flat)
    cls = torch.from_numpy(flat.astype(np.float32)).view(H, W, A).permute(2, 0, 1).contiguous()[None]
    reg = torch.from_numpy((0.3 * rs.randn(1, 7 * A, H, W)).astype(np.float32))
    dirp = None
    if s.use_dir:
        d = rs.randn(A, s.num_bins, H, W).astype(np.float32)
        if s.tie_dir:
            d[:] = d[:, :1]
            if s.num_bins > 2:
                d[:, 2:, ::2, ::2] -= 1.0
        dirp = torch.from_numpy(d.reshape(1, A * s.num_bins, H, W))
    if s.nonfinite is not None:
        put_nonfinite(s.nonfinite, cls, reg, passing, A, H, W)
    anchors = anchors_for(A, H, W, s.order) if anchors is None else anchors
    assert tuple(anchors.shape) == (H, W, A, 7)
    # the keep-edge rule, like the margin rule: a candidate within a few roundings of an edge of the sanity filters (tens per 65 536 candidates)
    # is MOVED off it -- its z and size deltas become 0, a plain anchor-sized box well inside every limit -- not dropped
    f64 = decode_f64(cls, reg, dirp, anchors, THR, s.order, s.dir_offset, s.num_bins, transform_of(s.transform))
    edge = f64["idx"][finite_rows(f64) & (f64["keep_slack"] <= 16 * KEEP_SLACK)]
    if len(edge):
        hw, an = torch.div(edge, A, rounding_mode="floor"), edge % A
        for k in (2, 3, 4, 5):
            reg[0].view(A, 7, H * W)[an, k, hw] = 0.0
    return Case(s, cls, reg, dirp, anchors, transform_of(s.transform), torch.from_numpy(passing))


NONFINITE = {"nan": ((0, float("nan")), (6, float("nan")), (4, float("nan"))),          # x, yaw (x and y corners NaN, z finite), width
             "size100": ((3, 100.0), (4, 100.0), (5, 100.0)),                          # exp overflows: an infinite h / w / l
             "zinf": ((2, float("inf")),)}


def put_nonfinite(kind, cls, reg, passing, A, H, W):
    """Directed candidates with high scores among the ordinary ones: anchor slots spread over the map, each given one non-finite delta."""
    total = A * H * W
    for n, (k, v) in enumerate(NONFINITE[kind]):
        i = (total // 7) * (2 * n + 1) + n
        hw, an = divmod(i, A)
        cls[0, an, hw // W, hw % W] = 3.0 + n
        reg[0, an * 7 + k, hw // W, hw % W] = v
        passing[i] = True


# ------------------------------------------------------------------------------------------------ float64 restatement
def decode_f64(cls, reg, dirp, anchors, thr, order, dir_offset=0.7853, num_bins=2, T=None):
    """voxel_postprocessor.py:291-355 for one agent, read from the float32 inputs and evaluated in float64 throughout: sigmoid, delta_to_boxes3d,
    the direction fix (with the float32-rounded period, 2 * pi and dir_offset both the kernel and the reference use; the lowest index among equal
    maxima), corners, the 4 x 4 projection, and both sanity filters NaN-propagating (torch.max / min) including the y-for-z quirk.
    -> dict(idx, scores, box7, corners_local, corners, keep, floor_args [K, 2], scale [K], keep_slack [K])."""
    A, H, W = cls.shape[1:]
    prob = (1.0 / (1.0 + torch.exp(-cls[0].double()))).permute(1, 2, 0).reshape(-1)
    mask = prob > thr
    idx = torch.nonzero(mask).view(-1)
    d = reg[0].double().view(A, 7, H * W).permute(2, 0, 1).reshape(-1, 7)[mask]
    a = anchors.reshape(-1, 7).float().double()[mask]
    diag = torch.sqrt(a[:, 4] ** 2 + a[:, 5] ** 2)
    b = torch.empty_like(d)
    b[:, 0] = d[:, 0] * diag + a[:, 0]
    b[:, 1] = d[:, 1] * diag + a[:, 1]
    b[:, 2] = d[:, 2] * a[:, 3] + a[:, 2]
    b[:, 3:6] = torch.exp(d[:, 3:6]) * a[:, 3:6]
    b[:, 6] = d[:, 6] + a[:, 6]
    args = torch.full((len(idx), 2), 0.5, dtype=torch.float64)
    if dirp is not None and len(idx):
        dm = dirp[0].double().view(A, num_bins, H * W).permute(2, 0, 1).reshape(-1, num_bins)[mask]
        best = dm.max(dim=1, keepdim=True)[0]
        bins = torch.arange(num_bins)[None, :].expand_as(dm)
        label = torch.where(dm == best, bins, torch.full_like(bins, num_bins)).min(dim=1)[0].double()      # the lowest index among equal maxima
        period = float(np.float32(2 * np.pi / num_bins))
        off = float(np.float32(dir_offset))
        v = b[:, 6] - off
        args[:, 0] = v / period
        rot = v - torch.floor(args[:, 0]) * period
        v = (rot + off) + period * label
        args[:, 1] = v / TWO_PI_F32 + 0.5
        b[:, 6] = v - torch.floor(args[:, 1]) * TWO_PI_F32
    lwh = b[:, [5, 4, 3]] if order == "hwl" else b[:, 3:6]
    template = torch.tensor([[1, -1, -1], [1, 1, -1], [-1, 1, -1], [-1, -1, -1], [1, -1, 1], [1, 1, 1], [-1, 1, 1], [-1, -1, 1]], dtype=torch.float64) / 2
    loc = lwh[:, None, :] * template[None]
    ca, sa = torch.cos(b[:, 6])[:, None], torch.sin(b[:, 6])[:, None]
    local = torch.stack([loc[..., 0] * ca - loc[..., 1] * sa + b[:, None, 0], loc[..., 0] * sa + loc[..., 1] * ca + b[:, None, 1],
                         loc[..., 2] + b[:, None, 2]], dim=-1)
    corners = local
    if T is not None:
        M = T.double()
        corners = torch.stack([M[r, 0] * local[..., 0] + M[r, 1] * local[..., 1] + M[r, 2] * local[..., 2] + M[r, 3] for r in range(3)], dim=-1)
    if len(idx) == 0:
        z = torch.zeros(0, dtype=torch.float64)
        return dict(idx=idx, scores=prob[mask], box7=b, corners_local=local, corners=corners, keep=torch.zeros(0, dtype=torch.bool), floor_args=args, scale=z, keep_slack=z)
    hi, lo = corners.max(dim=1)[0], corners.min(dim=1)[0]                        # NaN-propagating, like the reference's torch.max / torch.min
    x_len, y_len = hi[:, 0] - lo[:, 0], hi[:, 1] - lo[:, 1]
    keep = (x_len <= 6) & (y_len <= 6) & (y_len != 0) & (lo[:, 2] >= -3) & (hi[:, 2] <= 1)
    both = torch.cat([local.reshape(-1, 24), corners.reshape(-1, 24)], dim=1).abs()
    scale = torch.nan_to_num(both, nan=0.0, posinf=0.0).max(dim=1)[0].clamp(min=1.0)
    slack = torch.stack([(x_len - 6).abs(), (y_len - 6).abs(), y_len.abs(), (lo[:, 2] + 3).abs(), (hi[:, 2] - 1).abs()], dim=1).min(dim=1)[0] / scale
    return dict(idx=idx, scores=prob[mask], box7=b, corners_local=local, corners=corners, keep=keep, floor_args=args, scale=scale, keep_slack=slack)


def oracle_decode(case, thr=THR):
    """The float32 oracle on a case: (idx, box7, scores, corners, keep) -- decode_candidates + remove_large_pred_bbx + remove_bbx_abnormal_z."""
    s = case.spec
    idx, box7, scores, corners = oracle.decode_candidates(case.cls, case.reg, case.dir, case.anchors, thr, s.order, s.dir_offset, s.num_bins, case.transform)
    keep = torch.zeros(0, dtype=torch.bool)
    if len(idx):
        keep = torch.logical_and(oracle.remove_large_pred_bbx(corners), oracle.remove_bbx_abnormal_z(corners))
    return idx, box7, scores, corners, keep


@functools.lru_cache(maxsize=None)
def reference(s):
    """The case of a Spec and both references of it, computed once per process; callers must not write into the tensors."""
    case = make_case(s)
    idx, box7, scores, corners, keep = oracle_decode(case)
    f64 = decode_f64(case.cls, case.reg, case.dir, case.anchors, THR, s.order, s.dir_offset, s.num_bins, case.transform)
    return Ref(case, idx, scores, box7, corners, keep, f64)


# ------------------------------------------------------------------------------------------------ comparisons
def wrap_yaw(diff):
    """A yaw difference modulo 2 * pi, in [-pi, pi)."""
    return (diff + math.pi) % (2 * math.pi) - math.pi


def finite_rows(f64):
    """Candidates whose box and corners are all finite in float32 (a float64 value beyond FLT_MAX is an infinity there): the rows whose VALUES are
    compared.  NaN / inf patterns legitimately differ between the kernel's explicit sums and the reference's matmul."""
    flt_max = float(np.finfo(np.float32).max)
    return (f64["box7"].abs() <= flt_max).all(dim=1) & (f64["corners"].abs() <= flt_max).reshape(-1, 24).all(dim=1) \
        & (f64["corners_local"].abs() <= flt_max).reshape(-1, 24).all(dim=1)


def value_rows(f64):
    """finite_rows minus the candidates on a limit_period discontinuity; -> (rows, number left out for the discontinuity)."""
    fa = f64["floor_args"]
    near = ((fa - torch.round(fa)).abs() < NEAR_INTEGER).any(dim=1)
    fin = finite_rows(f64)
    return fin & ~near, int((fin & near).sum())


def error_vs_f64(box7, corners, f64, rows):
    """max over ``rows`` of max |value - float64| / scale (box7 with the yaw modulo 2 * pi, and the 24 corner coordinates)."""
    if not bool(rows.any()):
        return 0.0
    db = box7.double()[rows] - f64["box7"][rows]
    db[:, 6] = wrap_yaw(db[:, 6])
    dc = (corners.double()[rows] - f64["corners"][rows]).reshape(-1, 24)
    err = torch.cat([db, dc], dim=1).abs().max(dim=1)[0] / f64["scale"][rows]
    return float(err.max())


def assert_values_close(score, box7, corners, ref, rows, what=""):
    """Scores, box7 (yaw modulo 2 * pi) and corners within the existing decode tolerances of the float32 oracle, on ``rows``."""
    np.testing.assert_allclose(score.numpy(), ref.scores.numpy(), rtol=SCORE_RTOL, atol=0, err_msg=what + " scores")
    if not bool(rows.any()):
        return
    want = ref.box7[rows].clone()
    got = box7[rows].clone()
    got[:, 6] = want[:, 6] + wrap_yaw(got[:, 6].double() - want[:, 6].double()).float()
    np.testing.assert_allclose(got.numpy(), want.numpy(), err_msg=what + " box7", **BOX7_TOL)
    np.testing.assert_allclose(corners[rows].numpy(), ref.corners[rows].numpy(), err_msg=what + " corners", **CORNER_TOL)


# ------------------------------------------------------------------------------------------------ the cases
SHAPES = [(1, 1, 1), (2, 3, 5), (2, 8, 16), (1, 1, 257), (3, 7, 13), (1, 257, 256), (2, 129, 255)]
BIG = [(1, 257, 256), (2, 129, 255)]                  # 257 blocks: the second trip of emit_kernel's block_counts loop
DENSITIES = ["none", "all", 0.02, "first", "last", "seam"]


def _seed(*key):
    return sum((i + 1) * 7919 * int(k) for i, k in enumerate(key)) % 100003


VALUE_SPECS = [spec(A, H, W, _seed(A, H, W, n), dens) for (A, H, W) in SHAPES for n, dens in enumerate(DENSITIES)]
VALUE_SPECS += [spec(A, H, W, _seed(A, H, W, 9), "blocks", transform="identity") for (A, H, W) in BIG]

_TRANSFORMS = ["none", "identity", "rigid", "general"]
OPTION_SPECS = [spec(3, 7, 13, _seed(3, 7, 13, n), 0.6, order=o, use_dir=ud, transform=t)
                for n, (o, ud, t) in enumerate((o, ud, t) for o in ("hwl", "lhw") for ud in (True, False) for t in _TRANSFORMS)]
OPTION_SPECS += [spec(2, 8, 16, _seed(2, 8, 16, 20 + n), 0.6, order=o, num_bins=nb, dir_offset=off, transform="identity")
                 for n, (o, nb, off) in enumerate((o, nb, off) for o in ("hwl", "lhw") for nb in (1, 2, 4) for off in (0.7853, 0.0))]
OPTION_SPECS += [spec(3, 7, 13, _seed(3, 7, 13, 40 + nb), "all", num_bins=nb, tie_dir=True, dir_offset=off) for nb in (2, 4) for off in (0.7853, 0.0)]

NONFINITE_SPECS = [spec(3, 7, 13, _seed(3, 7, 13, 60 + n), 0.1, transform=t, nonfinite=kind)
                   for n, (kind, t) in enumerate((k, t) for k in ("nan", "size100", "zinf") for t in ("none", "identity"))]

CAPACITY_SPEC = spec(3, 7, 13, _seed(3, 7, 13, 70), 0.3, transform="identity")
CHAIN_SPECS = [spec(3, 7, 13, _seed(3, 7, 13, 80), 0.3, transform="identity"), spec(3, 7, 13, _seed(3, 7, 13, 81), "all", transform="rigid"),
               spec(3, 7, 13, _seed(3, 7, 13, 82), 0.3, transform="rigid_b")]
CLEAR_SPEC = spec(1, 1, 257, _seed(1, 1, 257, 90), 0.3, transform="general")

ALL_DECODE_SPECS = VALUE_SPECS + OPTION_SPECS + NONFINITE_SPECS + [CAPACITY_SPEC, CLEAR_SPEC] + CHAIN_SPECS

# the whole chain through VoxelPostprocessor: mini_coalign's head shape (2 anchors on 16 x 32) and range; frames of 2 and 3 cavs, one of them with a
# non-finite high-score candidate (agent 0: the identity transform, where 0 * inf and NaN reach every projected corner)
MINI = (2, 16, 32)
FRAME_SPECS = {
    "two_cavs": [spec(*MINI, 501, 0.05, transform="identity"), spec(*MINI, 502, 0.05, transform="near")],
    "three_cavs": [spec(*MINI, 503, 0.05, transform="identity"), spec(*MINI, 504, 0.05, transform="near"), spec(*MINI, 505, 0.05, transform="near_b")],
    "nonfinite": [spec(*MINI, 506, 0.05, transform="identity", nonfinite="nan"), spec(*MINI, 507, 0.05, transform="near", nonfinite="size100")],
}


def mini_postprocess_config():
    from coalign_amd.config import builtin_config
    return builtin_config("mini_coalign")["postprocess"]


@functools.lru_cache(maxsize=None)
def frame(name):
    """(agents for oracle.post_process, anchors, the oracle's boxes, scores and info) of one whole-chain frame on the configuration's own anchors
    (a 25.6 m x 12.8 m map: the range filter drops a good part of the kept boxes)."""
    cfg = mini_postprocess_config()
    anchors = torch.from_numpy(oracle.generate_anchor_box(cfg["anchor_args"], cfg["order"]))
    agents = []
    for s in FRAME_SPECS[name]:
        c = make_case(s, anchors)
        agents.append(dict(cls_preds=c.cls, reg_preds=c.reg, dir_preds=c.dir, transformation_matrix=c.transform))
    boxes, scores, info = oracle.post_process(agents, anchors, cfg)
    return agents, anchors, boxes, scores, info
