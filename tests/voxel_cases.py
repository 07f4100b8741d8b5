"""The case table of the voxeliser limit tests (tests/test_voxel_limits_cpu.py, tests/test_voxel_limits_gpu.py): pure numpy, every cloud built from its case's
seed, so the CPU test (which proves from the oracle that a case reaches the branch it is named for) and the GPU tests (which hold csrc/voxelize.hip to the oracle
on it) see identical inputs.

Groups:
  a  segment counts: cells of exactly 1 .. 4097 points at max_points 1 .. 64 -- gather_kernel's 16-lane path, one-wavefront rank, register / streamed bound
  b  block and cloud boundaries: clouds of 0 .. 2049 points, voxel heads on the first / last index of a 1024-point block, max_voxels cutting at a block edge,
     sixteen clouds of which three are empty
  c  owner counts: grids of 1, 5120, 5121, 256 x 128 x 41 and 4096 x 5120 x 1 cells -- split_kernel's owner scan at 1, 2 and 16 bins per thread
  d  capacity: one cloud of 2 097 152 points (2048 blocks, both stride loops of gather_kernel), and one point more
  e  float32 edges: one ulp either side of cell edges, of the range filter's strict and the ego box's closed bounds, NaN / Inf / 1e30, denormals, -0.0,
     arbitrary intensity words
Then the tables of the laboratory entry ``coalign_lab_voxelize_gather`` (include/coalign_amd_lab.h): gather_kernel alone, with the order inside a segment chosen.
"""
import functools
from dataclasses import dataclass
from typing import Callable, Optional, Sequence

import numpy as np

OPV2V_RANGE, OPV2V_VOXEL = [-140.8, -40, -3, 140.8, 40, 1], [0.4, 0.4, 4]

# ---------------------------------------------------------------------------------------------------------------- csrc/voxelize.hip's constants, restated
K_CHUNK = 1024            # points per block of split_kernel / assign_kernel (kChunk)
K_RANGE = 5120            # cells per owner workgroup (kRange); cell -> (owner cell % R, slot cell // R), R = ceil(cells / kRange)
K_SPLIT_THREADS = 256     # split_kernel scans per = ceil(R / 256) owner bins per thread
K_MAX_OWNERS = 4096
K_MAX_BLOCKS = 2048       # 1024-point blocks per cloud
K_OWNER_KEEP = 4096       # points an owner workgroup keeps in registers (1024 threads x kKeep 4)
K_SEG_LDS = 1024          # gather_kernel: ints of the per-wavefront LDS stage; segments up to it are held in registers
SMALL_STRIDE = 8192 * 16  # voxels beyond which the 16-lane workgroups of gather_kernel stride
BIG_STRIDE = 8192 * 4     # big cells beyond which its wavefront-per-cell workgroups stride
MAX_POINTS_PER_CLOUD = K_MAX_BLOCKS * K_CHUNK
MAX_CELLS = K_MAX_OWNERS * K_RANGE


def grid_size(voxel_size, lidar_range) -> np.ndarray:
    """round((max - min) / voxel) in float32, (x, y, z) -- oracle.voxel_grid_size restated (the CPU test holds the two equal)."""
    r, v = np.asarray(lidar_range, dtype=np.float32), np.asarray(voxel_size, dtype=np.float32)
    return np.round((r[3:6] - r[0:3]) / v).astype(np.int32)


def cell_index(points, voxel_size, lidar_range) -> np.ndarray:
    """Flat cell (z * gy + y) * gx + x of every point in float32 arithmetic, -1 outside the grid."""
    vs, lo, grid = np.asarray(voxel_size, np.float32), np.asarray(lidar_range[:3], np.float32), grid_size(voxel_size, lidar_range)
    with np.errstate(all="ignore"):
        q = np.floor((np.asarray(points, np.float32)[:, :3] - lo) / vs)
        ok = np.all((q >= 0) & (q < grid.astype(np.float32)), axis=1)
        qi = np.where(ok[:, None], q, 0).astype(np.int64)
    return np.where(ok, (qi[:, 2] * grid[1] + qi[:, 1]) * grid[0] + qi[:, 0], -1)


def owners(voxel_size, lidar_range):
    """-> (cells, R owner workgroups per cloud, bins per thread of split_kernel's scan)."""
    g = grid_size(voxel_size, lidar_range).astype(np.int64)
    ncell = int(g[0] * g[1] * g[2])
    R = (ncell + K_RANGE - 1) // K_RANGE
    return ncell, R, (R + K_SPLIT_THREADS - 1) // K_SPLIT_THREADS


def blocks(n: int) -> int:
    return (n + K_CHUNK - 1) // K_CHUNK


def points_in_cells(cells, voxel_size, lidar_range, rs) -> np.ndarray:
    """One point per entry of ``cells`` (flat indices), in the middle half of its cell on every axis; random intensity."""
    cells = np.asarray(cells, np.int64)
    g = grid_size(voxel_size, lidar_range).astype(np.int64)
    c = np.stack([cells % g[0], cells // g[0] % g[1], cells // (g[0] * g[1])], 1)
    xyz = np.asarray(lidar_range[:3], np.float64) + (c + rs.uniform(0.25, 0.75, (len(cells), 3))) * np.asarray(voxel_size, np.float64)
    pts = np.empty((len(cells), 4), np.float32)
    pts[:, :3] = xyz
    pts[:, 3] = rs.uniform(0, 1, len(cells))
    assert np.array_equal(cell_index(pts, voxel_size, lidar_range), cells)
    return pts


def cloud_from_pairs(pairs, voxel_size, lidar_range, seed, interleave=True) -> np.ndarray:
    """(cell, count) pairs -> a cloud holding exactly ``count`` points in ``cell``: interleaved by a seeded permutation, or every cell's points contiguous."""
    rs = np.random.RandomState(seed)
    cells = np.concatenate([np.full(k, c, np.int64) for c, k in pairs]) if pairs else np.zeros(0, np.int64)
    if interleave:
        cells = cells[rs.permutation(len(cells))]
    return points_in_cells(cells, voxel_size, lidar_range, rs)


def cloud_from_openings(n, openings, voxel_size, lidar_range, seed) -> np.ndarray:
    """``openings`` = ascending (point index, cell): the cell's first point sits at that index; every other point falls into a cell opened before it."""
    rs = np.random.RandomState(seed)
    at = dict(openings)
    assert openings[0][0] == 0 and len(at) == len(openings)
    cells, opened = np.empty(n, np.int64), []
    for i in range(n):
        if i in at:
            opened.append(at[i])
            cells[i] = at[i]
        else:
            cells[i] = opened[rs.randint(len(opened))]
    return points_in_cells(cells, voxel_size, lidar_range, rs)


def region_cloud(n, seed, x0=300, y0=80, w=30, h=30, voxel_size=OPV2V_VOXEL, lidar_range=OPV2V_RANGE) -> np.ndarray:
    """n points on random cells of a w x h patch of the grid."""
    rs = np.random.RandomState(seed)
    gx = int(grid_size(voxel_size, lidar_range)[0])
    return points_in_cells((y0 + rs.randint(0, h, n)) * gx + x0 + rs.randint(0, w, n), voxel_size, lidar_range, rs)


@dataclass(frozen=True)
class Case:
    name: str
    regime: str                       # the branch of csrc/voxelize.hip the case is built to reach; tests/test_voxel_limits_cpu.py proves it from the oracle
    make: Callable[[], list]
    voxel_size: Sequence[float] = tuple(OPV2V_VOXEL)
    lidar_range: Sequence[float] = tuple(OPV2V_RANGE)
    max_points: int = 32
    max_voxels: int = 70000
    ego: bool = False
    filter_range: Optional[Sequence[float]] = None
    info: tuple = ()                  # what the CPU test needs to prove the regime (pairs, openings, ...)

    @property
    def group(self) -> str:
        return self.name[0]

    def clouds(self) -> list:
        return _clouds(self.name)

    def as_tuple(self):
        """(clouds, voxel_size, range, max_points, max_voxels, flags, filter_range)"""
        return (self.clouds(), list(self.voxel_size), list(self.lidar_range), self.max_points, self.max_voxels,
                (1 if self.ego else 0) | (2 if self.filter_range is not None else 0), None if self.filter_range is None else list(self.filter_range))


@functools.lru_cache(maxsize=None)
def _clouds(name):
    clouds = CASES[name].make()
    for c in clouds:
        c.setflags(write=False)
    return clouds


CASES = {}


def _add(case: Case):
    assert case.name not in CASES
    CASES[case.name] = case


# ---------------------------------------------------------------------------------------------------------------- a: segment counts
A_COUNTS = (1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 1023, 1024, 1025, 4097)
A_MAX_POINTS = (1, 15, 16, 17, 32, 63, 64)


def a_pairs():
    rs = np.random.RandomState(100)
    g = grid_size(OPV2V_VOXEL, OPV2V_RANGE)
    cells = rs.choice(int(g[0]) * int(g[1]), len(A_COUNTS), replace=False)
    return tuple((int(c), k) for c, k in zip(cells, A_COUNTS))


for _mp in A_MAX_POINTS:
    for _inter in (True, False):
        _add(Case(f"a_mp{_mp}_{'interleaved' if _inter else 'contiguous'}",
                  "cells of exactly 1..4097 points: 16-lane DPP rank (<= 16), one-wavefront rank (<= 64), register bound (<= 1024), streamed bound (> 1024); one owner > 4096 points",
                  functools.partial(lambda inter: [cloud_from_pairs(a_pairs(), OPV2V_VOXEL, OPV2V_RANGE, 101, inter)], _inter), max_points=_mp, info=a_pairs()))

# ---------------------------------------------------------------------------------------------------------------- b: block and cloud boundaries
B_SIZES = (0, 1, 1023, 1024, 1025, 2047, 2048, 2049)
_add(Case("b_sizes_together", "clouds of 0 .. 2049 points in one call: empty, partial, exactly full and one-past-full last blocks",
          lambda: [region_cloud(n, 200 + i) for i, n in enumerate(B_SIZES)], max_points=5, info=B_SIZES))
for _i, _n in enumerate(B_SIZES):
    _add(Case(f"b_size_{_n}", f"a cloud of {_n} points alone: {blocks(_n)} blocks", functools.partial(lambda i, n: [region_cloud(n, 200 + i)], _i, _n), max_points=5, info=(_n,)))


def _cells_far_apart(count, seed):
    rs = np.random.RandomState(seed)
    g = grid_size(OPV2V_VOXEL, OPV2V_RANGE)
    return [int(c) for c in rs.choice(int(g[0]) * int(g[1]), count, replace=False)]


B_HEADS_N = 3000
B_HEADS_AT = (0, 1023, 1024, 2047, B_HEADS_N - 1)
B_HEADS_OPENINGS = tuple(zip(B_HEADS_AT, _cells_far_apart(len(B_HEADS_AT), 210)))
_add(Case("b_heads_on_block_edges", "voxel-opening points on the first and the last index of blocks 0 and 1 and on the cloud's last index",
          lambda: [cloud_from_openings(B_HEADS_N, B_HEADS_OPENINGS, OPV2V_VOXEL, OPV2V_RANGE, 211)], max_points=32, info=B_HEADS_OPENINGS))

B_CUT_N = 2500
B_CUT_AT = (0, 3, 50, 200, 400, 600, 800, 1000, 1023, 1024, 1100, 1300, 1500, 1800, 2047, 2048, 2300, 2499)
B_CUT_OPENINGS = tuple(zip(B_CUT_AT, _cells_far_apart(len(B_CUT_AT), 220)))
B_CUT_HEADS_BLOCK0 = sum(1 for i in B_CUT_AT if i < K_CHUNK)          # 9: the last head of block 0 has rank 8, the first head of block 1 rank 9
for _label, _mv in (("one", 1), ("all_cells", len(B_CUT_AT)), ("all_but_one", len(B_CUT_AT) - 1), ("drops_last_head_of_block0", B_CUT_HEADS_BLOCK0 - 1),
                    ("drops_first_head_of_block1", B_CUT_HEADS_BLOCK0), ("keeps_first_head_of_block1", B_CUT_HEADS_BLOCK0 + 1)):
    _add(Case(f"b_max_voxels_{_label}", f"max_voxels = {_mv} of {len(B_CUT_AT)} occupied cells, {B_CUT_HEADS_BLOCK0} of them opened in block 0; dropped cells of > 16 points (v < 0 skip)",
              lambda: [cloud_from_openings(B_CUT_N, B_CUT_OPENINGS, OPV2V_VOXEL, OPV2V_RANGE, 221)], max_points=20, max_voxels=_mv, info=B_CUT_OPENINGS))

B_SIXTEEN = (0, 5, 1024, 300, 2049, 1, 0, 777, 1025, 64, 17, 4000, 1500, 33, 2048, 0)
_add(Case("b_sixteen_clouds", "16 clouds, the first, a middle and the last one empty; max_voxels clamps some clouds and not others",
          lambda: [region_cloud(n, 230 + i) for i, n in enumerate(B_SIXTEEN)], max_points=8, max_voxels=400, info=B_SIXTEEN))

# ---------------------------------------------------------------------------------------------------------------- c: owner counts
C_GRIDS = {   # name -> (voxel, range, expected grid, R, per)
    "c_one_cell": ([4, 4, 4], [0, 0, 0, 4, 4, 4], (1, 1, 1), 1, 1),
    "c_5120_cells": ([0.5, 0.5, 4], [-20, -16, -2, 20, 16, 2], (80, 64, 1), 1, 1),
    "c_5121_cells": ([0.5, 0.5, 4], [-142.25, -2.25, -2, 142.25, 2.25, 2], (569, 9, 1), 2, 1),
    "c_263_owners": ([0.1, 0.1, 0.1], [-12.8, -6.4, -3, 12.8, 6.4, 1.1], (256, 128, 41), 263, 2),
    "c_limit_grid": ([0.25, 0.25, 4], [-512, -640, -2, 512, 640, 2], (4096, 5120, 1), 4096, 16),
}


def c_named_cells(voxel_size, lidar_range):
    """The cells either side of every owner-deal boundary that is cheap to name, with the point count each gets."""
    ncell, R, _ = owners(voxel_size, lidar_range)
    if ncell == 1:
        return [(0, 3000)]
    named = []
    for cell, count in ((0, 40), (1, 3), (R - 1, 17), (R, 16), (R + 1, 2), (ncell - R, 5), (ncell - 2, 1), (ncell - 1, 65)):
        if 0 <= cell < ncell and cell not in [c for c, _ in named]:
            named.append((cell, count))
    return named


def c_cloud(name):
    vs, rng = C_GRIDS[name][:2]
    ncell, R, _ = owners(vs, rng)
    rs = np.random.RandomState(300 + list(C_GRIDS).index(name))
    named = c_named_cells(vs, rng)
    others = [int(c) for c in np.unique(rs.randint(0, ncell, 2500)) if c not in dict(named)] if ncell > 1 else []
    pairs = named + [(c, int(k)) for c, k in zip(others, rs.randint(1, 4, len(others)))]
    cloud = cloud_from_pairs(pairs, vs, rng, 310 + list(C_GRIDS).index(name))
    outside = cloud[:40].copy()               # and some points outside the grid on every side
    outside[:20, 0] = np.float32(rng[3]) + np.float32(1.0)
    outside[20:, 1] = np.float32(rng[1]) - np.float32(1.0)
    cloud = np.concatenate([cloud, outside])[rs.permutation(len(cloud) + 40)]
    # one point of every named cell comes first, so that max_voxels (below the occupied cells on the limit grid) keeps them
    cells = cell_index(cloud, vs, rng)
    first = [int(np.flatnonzero(cells == c)[0]) for c, _ in named]
    rest = np.setdiff1d(np.arange(len(cloud)), first)
    return np.ascontiguousarray(cloud[np.concatenate([first, rest]).astype(np.int64)])


for _name, (_vs, _rng, _grid, _R, _per) in C_GRIDS.items():
    _add(Case(_name, f"grid {_grid[0]} x {_grid[1]} x {_grid[2]}: R = {_R} owners, split_kernel scans {_per} bins per thread", functools.partial(lambda n: [c_cloud(n)], _name),
              voxel_size=tuple(_vs), lidar_range=tuple(_rng), max_points=32, max_voxels=2000 if _name == "c_limit_grid" else 70000, info=(_grid, _R, _per)))

# ---------------------------------------------------------------------------------------------------------------- d: capacity


def d_cloud(extra=0):
    """Uniform on the OPV2V range: about 14.9 points per cell.  ``extra`` points more are appended (the cloud the entry must refuse)."""
    rs = np.random.RandomState(400)
    n = MAX_POINTS_PER_CLOUD
    pts = np.empty((n, 4), np.float32)
    pts[:, 0] = rs.uniform(-140.8, 140.8, n)
    pts[:, 1] = rs.uniform(-40, 40, n)
    pts[:, 2] = rs.uniform(-3, 1, n)
    pts[:, 3] = rs.uniform(0, 1, n)
    return np.concatenate([pts, pts[:extra] + np.float32(0.25)]) if extra else pts


_add(Case("d_two_million_points", "2 097 152 points in one cloud: 2048 blocks in owner_kernel, > 131 072 voxels (small-path stride), > 32 768 big cells (big-path stride)",
          lambda: [d_cloud()], max_points=4, max_voxels=704 * 200))

# ---------------------------------------------------------------------------------------------------------------- e: float32 edges
E_FILTER_TIGHT = (-70.4, -38.4, -2.5, 70.4, 38.4, 0.5)
EGO_BOX = ((-1.95, 2.95), (-1.1, 1.1))         # closed, x and y (pcd_utils.py:69-88)
E_MID = (10.2, 5.0, -1.0)                      # mid-cell on every axis, outside the ego box, inside both filter ranges
E_INSIDE_EGO = (1.0, 0.2)                      # the other coordinate of an ego-bound triple lies inside the box
E_INTENSITY_WORDS = (0x7fc00001, 0xffc12345, 0x7f800001, 0x80000000, 0x00000001, 0x807fffff, 0x7fffffff, 0xffffffff, 0x7f800000, 0xff800000)
F32 = np.float32


def _triple(t):
    t = F32(t)
    return (("below", np.nextafter(t, F32(-np.inf))), ("at", t), ("above", np.nextafter(t, F32(np.inf))))


@functools.lru_cache(maxsize=None)
def e_points():
    """-> (tags, points [n, 4] float32): every point carries a tag the expectation list of tests/test_voxel_limits_cpu.py is keyed by.  The intensity word of the
    points that do not test intensity words is the point's number (exact in float32), so a row of the output names its source."""
    tags, rows = [], []

    def put(tag, x, y, z, word=None):
        tags.append(tag)
        rows.append((F32(x), F32(y), F32(z), word))

    grid = grid_size(OPV2V_VOXEL, OPV2V_RANGE)
    for axis, name in enumerate("xyz"):
        for k in sorted({0, 1, 2, int(grid[axis]) - 1, int(grid[axis])}):
            t = F32(OPV2V_RANGE[axis] + k * OPV2V_VOXEL[axis])                   # lo + k * vs, rounded to float32
            for pos, v in _triple(t):
                p = list(E_MID)
                p[axis] = v
                put(f"cell.{name}.{k}.{pos}", *p)
        for which, rng in (("grid", OPV2V_RANGE), ("tight", E_FILTER_TIGHT)):   # the range filter's six bounds, for both filter ranges the cases use
            for side, t in (("lo", rng[axis]), ("hi", rng[3 + axis])):
                for pos, v in _triple(t):
                    p = list(E_MID)
                    p[axis] = v
                    put(f"filter.{which}.{name}.{side}.{pos}", *p)
    for axis, name in enumerate("xy"):
        for side, t in zip(("lo", "hi"), EGO_BOX[axis]):
            for pos, v in _triple(t):
                p = [E_INSIDE_EGO[0], E_INSIDE_EGO[1], E_MID[2]]
                p[axis] = v
                put(f"ego.{name}.{side}.{pos}", *p)
    for axis, name in enumerate("xyz"):
        for label, v in (("nan", np.nan), ("pinf", np.inf), ("ninf", -np.inf), ("p1e30", 1e30), ("m1e30", -1e30), ("mzero", -0.0), ("mdenorm", -1e-45), ("pdenorm", 1e-45)):
            p = list(E_MID)
            p[axis] = v
            put(f"special.{name}.{label}", *p)
    for w in E_INTENSITY_WORDS:
        put(f"word.{w:08x}", *E_MID, word=w)
        put(f"word.{w:08x}.rejected", 1000.0, E_MID[1], E_MID[2], word=w)
    pts = np.empty((len(rows), 4), np.float32)
    for i, (x, y, z, word) in enumerate(rows):
        pts[i, :3] = (x, y, z)
        pts[i, 3] = F32(i)
        if word is not None:
            pts[i:i + 1, 3].view(np.uint32)[0] = word
    return tuple(tags), pts


for _label, _ego, _fr in (("plain", False, None), ("ego", True, None), ("range_grid", False, tuple(OPV2V_RANGE)), ("ego_range_grid", True, tuple(OPV2V_RANGE)),
                          ("range_tight", False, E_FILTER_TIGHT), ("ego_range_tight", True, E_FILTER_TIGHT)):
    _add(Case(f"e_edges_{_label}", "float32 edges: cell edges, filter bounds and ego bounds +- 1 ulp, NaN / Inf / 1e30, -0.0, denormals, intensity words",
              lambda: [e_points()[1].copy()], max_points=5, ego=_ego, filter_range=_fr))

E_ZERO_MIN = {"e_denormal_voxel4": ([4, 4, 4], [0, 0, 0, 64, 64, 8]), "e_denormal_voxel04": ([0.4, 0.4, 0.4], [0, 0, 0, 6.4, 6.4, 0.8])}
E_ZERO_VALUES = (("mdenorm", -1e-45), ("pdenorm", 1e-45), ("mzero", -0.0), ("pzero", 0.0), ("mdenorm_big", -1.1754942e-38), ("mtiny_normal", -1.17549435e-38))


@functools.lru_cache(maxsize=None)
def e_zero_points(name):
    """A range whose minimum is 0: -1e-45 / 4 rounds to -0 (floor -0: cell 0, accepted), -1e-45 / 0.4 stays denormal (floor -1: rejected)."""
    vs, _ = E_ZERO_MIN[name]
    tags, rows = [], []
    for axis, an in enumerate("xyz"):
        for label, v in E_ZERO_VALUES:
            p = [1.5 * vs[0], 2.5 * vs[1], 0.5 * vs[2]]
            p[axis] = v
            tags.append(f"zero.{an}.{label}")
            rows.append(p + [len(rows)])
    return tuple(tags), np.asarray(rows, np.float32)


for _name, (_vs, _rng) in E_ZERO_MIN.items():
    _add(Case(_name, "range minimum 0: the quotient of a negative denormal rounds to -0 (accepted) or stays denormal (rejected)",
              functools.partial(lambda n: [e_zero_points(n)[1].copy()], _name), voxel_size=tuple(_vs), lidar_range=tuple(_rng), max_points=8))


def group(letter):
    return [c for c in CASES.values() if c.group == letter]


def reference_with(case, generator, late_order=False):
    """((voxels, coords (cloud, z, y, x), num), voxels per cloud) of a case by ``generator`` (oracle.points_to_voxel or its plain-Python twin) behind the oracle's
    two point filters: ego mask then range mask (intermediate fusion), or range mask then ego mask (``late_order``: late fusion; the same set)."""
    from oracle import coalign_oracle as oracle
    per = []
    for c in case.clouds():
        for step in (("range", "ego") if late_order else ("ego", "range")):
            if step == "range" and case.filter_range is not None:
                c = oracle.mask_points_by_range(c, case.filter_range)
            if step == "ego" and case.ego:
                c = oracle.mask_ego_points(c)
        per.append(generator(c, case.voxel_size, case.lidar_range, case.max_points, case.max_voxels))
    return oracle.collate_voxels(per), [len(p[0]) for p in per]


@functools.lru_cache(maxsize=None)
def reference(name):
    """The C oracle's answer to a case: computed once, shared by the tests, left unchanged."""
    from oracle import coalign_oracle as oracle
    (v, c, n), counts = reference_with(CASES[name], oracle.points_to_voxel)
    for a in (v, c, n):
        a.setflags(write=False)
    return (v, c, n), counts


# ---------------------------------------------------------------------------------------------------------------- the laboratory entry's tables
ORDER_RULES = ("ascending", "descending", "random", "transposed")


def order_segment(sorted_idx, rule, rs) -> np.ndarray:
    """The segment's point indices in the order the bucket holds them.  transposed (count % 64 == 0, U = count / 64): the r-th smallest index goes to position
    (r mod U) * 64 + r div U, so lane l's strided share {l, l + 64, ...} holds the ranks [l U, l U + U) and the bound admits (keep - 1) U + 1 candidates.  A count that
    is no multiple of 64 is transposed on its largest multiple of 64, the rest appended (the largest indices)."""
    s = np.asarray(sorted_idx, np.int64)
    n = len(s)
    if rule == "ascending":
        return s.copy()
    if rule == "descending":
        return s[::-1].copy()
    if rule == "random":
        return s[rs.permutation(n)]
    assert rule == "transposed"
    U = n // 64
    if U == 0:
        return s[::-1].copy()
    out = s.copy()
    r = np.arange(U * 64)
    out[(r % U) * 64 + r // U] = s[:U * 64]
    return out


def candidate_count(segment, keep) -> int:
    """gather_kernel's candidate rule restated: lane l's minimum over its strided share, the keep-th smallest of the 64 minima, the entries <= it (segments of > 64)."""
    seg = np.asarray(segment, np.int64)
    assert len(seg) > 64
    minima = np.sort([seg[lane::64].min() for lane in range(64)])
    return int((seg <= minima[min(keep, len(seg)) - 1]).sum())


def gather_regime(count, candidates) -> str:
    if count <= 16:
        return "small"
    if count <= 64:
        return "wave"
    bound = "register" if count <= K_SEG_LDS else "streamed"
    return bound + ("_direct" if candidates <= 64 else "_lds_rounds" if candidates <= K_SEG_LDS else "_global_rounds")


def gather_tables(points, index_sets, rules, max_points, dropped_sets=(), seed=0):
    """Well-formed tables for ``coalign_lab_voxelize_gather`` and the expected output.  ``index_sets[v]`` = the point indices of voxel row v, ``rules[v]`` its order rule;
    ``dropped_sets``: big cells whose cellinfo row carries voxel row -1 (on the big-cell list, skipped).  cellinfo rows and the big-cell list are in seeded random order."""
    rs = np.random.RandomState(seed)
    n = len(points)
    M = len(index_sets)
    every = [(np.sort(np.asarray(s, np.int64)), r, v) for v, (s, r) in enumerate(zip(index_sets, rules))] + [(np.sort(np.asarray(s, np.int64)), "random", -1) for s in dropped_sets]
    place = rs.permutation(len(every))                       # segments lie in the bucket in another order than the voxel rows
    bucket = np.full(n, -1, np.int32)                        # slots outside every segment are never read
    seg = np.zeros((M, 2), np.int32)
    big, orders, at = [], {}, 0
    for j in place:
        s, rule, v = every[j]
        assert len(s) and len(np.unique(s)) == len(s) and s[0] >= 0 and s[-1] < n and at + len(s) <= n
        order = order_segment(s, rule, rs)
        bucket[at:at + len(s)] = order
        if v >= 0:
            seg[v] = (at, len(s))
            orders[v] = order
        if len(s) > 16:
            big.append((len(s), int(s[0]), at, v))
        at += len(s)
    list_cap = n // 17 + 1
    assert len(big) <= list_cap
    rows = rs.permutation(len(big) + 3)[:len(big)]           # three spare cellinfo rows (zero count, row -1) that nothing names
    cellinfo = np.zeros((len(big) + 3, 4), np.int32)
    cellinfo[:, 3] = -1
    for row, info in zip(rows, big):
        cellinfo[row] = info
    biglist = np.zeros(list_cap, np.int32)
    biglist[:len(big)] = rows[rs.permutation(len(big))] if big else []
    biglist[len(big):] = rows[0] if big else 0               # past big_count: fetched, not used; still a real row
    expected = np.zeros((M, max_points, 4), np.float32)
    for v, s in enumerate(index_sets):
        first = np.sort(np.asarray(s, np.int64))[:max_points]
        expected[v, :len(first)] = points[first]
    return {"points": np.ascontiguousarray(points, np.float32), "bucket": bucket, "seg": seg, "cellinfo": cellinfo, "biglist": biglist,
            "big_count": np.asarray([len(big)], np.int32), "total": np.asarray([M], np.int32), "max_points": max_points, "expected": expected, "orders": orders}


def gather_table_from_counts(segments, max_points, seed, dropped=(100,)):
    """``segments`` = [(count, order rule)] -> random points, the point indices dealt to the segments by a seeded permutation (so the segments' index ranges interleave)."""
    rs = np.random.RandomState(seed)
    counts = [c for c, _ in segments] + list(dropped)
    n = sum(counts) + 7                                      # seven points in no segment
    points = rs.uniform(-50, 50, (n, 4)).astype(np.float32)
    perm = rs.permutation(n)
    sets, at = [], 0
    for c in counts:
        sets.append(perm[at:at + c])
        at += c
    return gather_tables(points, sets[:len(segments)], [r for _, r in segments], max_points, sets[len(segments):], seed + 1)


GATHER_COUNTS = (1, 15, 16, 17, 63, 64, 65, 1024, 1088)
# name -> (segments, max_points): several regimes in one table, so that one wavefront walks from one into the next (the LDS stage is reused between items)
GATHER_TABLES = {f"every_count_{rule}_keep{mp}": ([(c, rule) for c in GATHER_COUNTS], mp) for rule in ORDER_RULES for mp in (1, 32, 64)}
GATHER_TABLES.update({
    "transposed_1024_keep32": ([(1024, "transposed"), (40, "random"), (1024, "transposed"), (3, "ascending"), (2048, "transposed"), (200, "random")], 32),
    "transposed_1024_keep64": ([(1024, "transposed"), (30, "random"), (1024, "ascending"), (70, "descending"), (9, "random"), (1024, "transposed")], 64),
    "transposed_4096_keep32": ([(4096, "transposed"), (1024, "transposed"), (4096, "random"), (17, "descending"), (4096, "transposed")], 32),
    "transposed_2048_keep64": ([(2048, "transposed"), (64, "random"), (2048, "transposed"), (1024, "transposed"), (2048, "descending")], 64),
    "transposed_4096_keep1": ([(4096, "transposed"), (16, "random"), (4096, "descending"), (40, "random"), (65, "transposed")], 1),
    "mixed_regimes_keep48": ([(4096, "transposed"), (1024, "transposed"), (65, "random"), (2048, "transposed"), (16, "descending"), (1024, "random"), (4096, "ascending"),
                              (64, "descending"), (1088, "transposed"), (1, "ascending"), (2048, "random")], 48),
})
# the candidate counts the issue names: table -> (count, candidates) of its FIRST segment
GATHER_NAMED_CANDIDATES = {"transposed_1024_keep32": (1024, 497), "transposed_1024_keep64": (1024, 1009), "transposed_4096_keep32": (4096, 1985),
                           "transposed_2048_keep64": (2048, 2017), "transposed_4096_keep1": (4096, 1)}


@functools.lru_cache(maxsize=None)
def gather_table(name):
    segments, mp = GATHER_TABLES[name]
    return gather_table_from_counts(segments, mp, 500 + sorted(GATHER_TABLES).index(name))
