"""The cases of the raw-clouds-to-sites tests (tests/test_sp3d_voxelize_cpu.py: the torch-op route; tests/test_sp3d_voxelize_gpu.py: ``coalign_sp3d_voxelize``), and
the reference every comparison uses: ``oracle.points_to_voxel`` per cloud (after the reference's own numpy point filters), ``oracle.collate_voxels``, the mean in
float32 in slot order in numpy, rows sorted by the linear cell index.  Comparisons are exact.

The tiny grid: range [0, 0, 0, 2.0, 1.2, 0.8], voxel 0.1 -> voxel grid (20, 12, 8), sparse shape (9, 12, 20) = ``sparse3d_cases.SHAPE`` (its cloud stride of 2160 cells
is no multiple of 32); T = 5; two clouds unless a case says otherwise.  One case lives on the OPV2V grid that ``coalign_voxelize`` refuses."""
import functools
from collections import namedtuple

import numpy as np
import torch

from coalign_amd import ops, sparse3d
from oracle import coalign_oracle as oracle

VOXEL, RANGE, SHAPE, T = (0.1, 0.1, 0.1), (0.0, 0.0, 0.0, 2.0, 1.2, 0.8), (9, 12, 20), 5
GRID = (20, 12, 8)                                                   # x, y, z
OPV2V_VOXEL, OPV2V_RANGE, OPV2V_SHAPE = (0.1, 0.1, 0.1), (-140.8, -40.0, -3.0, 140.8, 40.0, 1.0), (41, 800, 2816)
FILTER = (0.25, 0.15, 0.05, 1.75, 1.05, 0.75)                         # a strict range inside the tiny grid, its bounds off the cell edges
F32 = np.float32

Case = namedtuple("Case", "name clouds max_points max_voxels ego filter_range voxel_size lidar_range shape", defaults=(T, 1000, False, None, VOXEL, RANGE, SHAPE))
Want = namedtuple("Want", "features indices cloud_counts reached")


def _cloud(rows) -> np.ndarray:
    return np.asarray(rows, dtype=F32).reshape(-1, 4)


def centre(cx, cy, cz, value=0.0):
    """A point well inside cell (cx, cy, cz) of the tiny grid."""
    return [(cx + 0.5) * 0.1, (cy + 0.5) * 0.1, (cz + 0.5) * 0.1, value]


def cells_cloud(cell_counts, seed, jitter=True):
    """A cloud with ``count`` points in each ``cell`` = (cx, cy, cz), all cells' points INTERLEAVED by a seeded shuffle; the intensity is the point's final index + 1
    and x, y, z wander inside the cell, so that picking any other point than the first T in point order changes the mean."""
    rs = np.random.RandomState(seed)
    cells = np.concatenate([np.tile(np.asarray(c, dtype=np.float64), (n, 1)) for c, n in cell_counts])
    rs.shuffle(cells)
    off = rs.uniform(0.1, 0.9, size=cells.shape) if jitter else np.full(cells.shape, 0.5)
    pts = np.zeros((len(cells), 4), dtype=F32)
    pts[:, :3] = ((cells + off) * 0.1).astype(F32)
    pts[:, 3] = np.arange(1, len(cells) + 1, dtype=F32)
    return pts


def edge_points():
    """Per axis: lo, lo + k vs in float32 for every k (floorf of the quotient can fall either side of k), hi, one point outside on each side, and NaN; the other two
    coordinates mid-cell.  Plus points on and beside the ego box's y bound and on the bounds of ``FILTER``."""
    rows, mid, n = [], [0.55, 0.65, 0.35], 0
    lo, hi, vs = np.asarray(RANGE[:3], dtype=F32), np.asarray(RANGE[3:], dtype=F32), np.asarray(VOXEL, dtype=F32)
    for axis in range(3):
        values = [lo[axis], hi[axis], np.nextafter(lo[axis], F32(-1)), F32(lo[axis] - 0.05), np.nextafter(hi[axis], F32(9)), F32(hi[axis] + 0.05),
                  np.nextafter(hi[axis], F32(0)), F32("nan")]
        values += [F32(lo[axis] + F32(k) * vs[axis]) for k in range(GRID[axis] + 1)]
        values += [np.nextafter(F32(lo[axis] + F32(k) * vs[axis]), F32(-1)) for k in range(1, GRID[axis] + 1)]
        for v in values:
            p = list(mid)
            p[axis] = v
            n += 1
            rows.append(p + [float(n)])
    for y in (F32(1.1), np.nextafter(F32(1.1), F32(9)), np.nextafter(F32(1.1), F32(0)), F32(1.15)):       # the ego box is closed at y = 1.1
        for x in (F32(0.55), F32(1.95)):
            n += 1
            rows.append([x, y, 0.35, float(n)])
    for j in range(3):                                                                                # on, just inside and just outside FILTER's strict bounds
        for b in (F32(FILTER[j]), F32(FILTER[3 + j])):
            for v in (b, np.nextafter(b, F32(9)), np.nextafter(b, F32(-9))):
                p = [1.0, 1.0, 0.4]
                p[j] = v
                n += 1
                rows.append(p + [float(n)])
    return _cloud(rows)


def max_voxels_clouds(mv):
    """Cloud 0: mv + 3 distinct cells opened in order; a later point of a KEPT cell (it still counts), later points of DROPPED cells (they open nothing).  Cloud 1: four
    cells, untouched by the cut of cloud 0 when mv >= 4."""
    cells = [(2 * i % 20, (3 * i) % 12, i % 8) for i in range(mv + 3)]
    rows = [centre(*c, value=10.0 + i) for i, c in enumerate(cells)]
    rows.append(centre(*cells[0], value=100.0))                       # kept cell, again
    rows.append(centre(*cells[mv + 1], value=200.0))                  # dropped cells, again
    rows.append(centre(*cells[mv + 2], value=300.0))
    rows.append(centre(*cells[mv - 1], value=400.0))                  # the last kept cell, again
    rows.append(centre(*cells[mv], value=500.0))                      # the first dropped cell, again
    other = [centre(1, 1, 1, 1.0), centre(5, 5, 5, 2.0), centre(1, 1, 1, 3.0), centre(19, 11, 7, 4.0), centre(0, 0, 0, 5.0)]
    return [_cloud(rows), _cloud(other)]


def every_cell_clouds():
    out = []
    for b in range(2):
        rs = np.random.RandomState(40 + b)
        cells = np.stack(np.meshgrid(np.arange(20), np.arange(12), np.arange(8), indexing="ij"), axis=-1).reshape(-1, 3)
        rs.shuffle(cells)
        pts = np.zeros((len(cells), 4), dtype=F32)
        pts[:, :3] = ((cells + rs.uniform(0.2, 0.8, size=cells.shape)) * 0.1).astype(F32)
        pts[:, 3] = rs.uniform(size=len(cells)).astype(F32)
        out.append(pts)
    return out


def opv2v_clouds():
    """Two clouds of about 3 500 uniformly drawn points on the OPV2V range, some of them outside."""
    out = []
    for b in range(2):
        rs = np.random.RandomState(70 + b)
        lo, hi = np.asarray(OPV2V_RANGE[:3]), np.asarray(OPV2V_RANGE[3:])
        pts = np.zeros((3500 + 13 * b, 4), dtype=F32)
        pts[:, :3] = (lo - 0.1 + rs.uniform(size=(len(pts), 3)) * (hi - lo + 0.2)).astype(F32)
        pts[:, 3] = rs.uniform(size=len(pts)).astype(F32)
        out.append(pts)
    return out


def _build():
    empty = np.zeros((0, 4), dtype=F32)
    a = cells_cloud([((3, 4, 2), T), ((3, 4, 3), T + 1), ((10, 6, 5), 65), ((19, 11, 7), 1100), ((0, 0, 0), 1), ((4, 4, 2), 2)], seed=1)
    b = cells_cloud([((3, 4, 2), 7), ((7, 7, 7), T), ((12, 0, 0), 33)], seed=2)
    small = cells_cloud([((1, 2, 3), 3), ((4, 5, 6), 6), ((19, 0, 7), 1)], seed=3)
    outside = _cloud([[-0.5, 0.5, 0.4, 1.0], [2.5, 0.5, 0.4, 2.0], [0.5, 1.25, 0.4, 3.0], [0.5, 0.5, 0.85, 4.0], [float("nan"), 0.5, 0.4, 5.0]])
    edges = edge_points()
    cases = [
        Case("point_order", [a, b]),
        Case("point_order_T1", [a, b], 1),
        Case("point_order_T8", [a, b], 8),
        Case("edges", [edges, edges[::-1].copy()]),
        Case("edges_ego", [edges, edges[::-1].copy()], ego=True),
        Case("edges_range", [edges, edges[::-1].copy()], filter_range=FILTER),
        Case("edges_both", [edges, edges[::-1].copy()], ego=True, filter_range=FILTER),
        Case("max_voxels", max_voxels_clouds(6), max_voxels=6),
        Case("max_voxels_exactly", max_voxels_clouds(6), max_voxels=9),          # cloud 0 opens exactly max_voxels cells: none is dropped, the bit is set
        Case("max_voxels_1", max_voxels_clouds(6), max_voxels=1),
        Case("max_voxels_interleaved", [a, b], max_voxels=3),
        Case("empty_first_middle_last", [empty, small, empty, b, empty]),
        Case("all_invalid", [outside, outside[::-1].copy()]),
        Case("one_cloud_invalid", [outside, small]),
        Case("same_coordinates_two_clouds", [small, small.copy()]),
        Case("sixteen_clouds", [cells_cloud([((i, i % 12, i % 8), 1 + i % 7), ((19 - i, 3, 4), 2)], seed=20 + i) for i in range(16)]),
        Case("one_cloud", [a]),
        Case("every_cell", every_cell_clouds(), max_voxels=5000),
        Case("every_cell_cut_at_1100", every_cell_clouds(), max_voxels=1100),     # the cut falls into the second 1024-point block of each cloud
        Case("opv2v_grid", opv2v_clouds(), T, 70000, False, None, OPV2V_VOXEL, OPV2V_RANGE, OPV2V_SHAPE),
    ]
    return {c.name: c for c in cases}


CASES = _build()
TINY = [n for n, c in CASES.items() if c.shape == SHAPE]


def linear_cell(indices, shape):
    D, H, W = shape
    i = np.asarray(indices, dtype=np.int64)
    return ((i[:, 0] * D + i[:, 1]) * H + i[:, 2]) * W + i[:, 3]


@functools.lru_cache(maxsize=None)
def reference(name) -> Want:
    """The oracle's chain on the case (computed once, shared, never modified): features [M, 4] float32, indices [M, 4] int32, ascending in the linear cell index;
    cloud_counts [n + 1]; ``reached``: some cloud holds max_voxels voxels."""
    c = CASES[name]
    per = []
    for pts in c.clouds:
        pts = np.ascontiguousarray(pts, dtype=F32)
        if c.filter_range is not None:
            pts = oracle.mask_points_by_range(pts, c.filter_range)
        if c.ego:
            pts = oracle.mask_ego_points(pts)
        per.append(oracle.points_to_voxel(pts, c.voxel_size, c.lidar_range, c.max_points, c.max_voxels))
    voxels, coords, num = oracle.collate_voxels(per)
    s = np.zeros((len(voxels), 4), dtype=F32)
    for t in range(c.max_points):                                      # slot order, float32: MeanVFE's sum over the zero-padded slots
        s = s + voxels[:, t]
    mean = (s / np.maximum(num, 1).astype(F32)[:, None]).astype(F32)
    order = np.argsort(linear_cell(coords, c.shape), kind="stable")
    counts = [len(v) for v, _, _ in per]
    for a in (mean, coords):
        a.setflags(write=False)
    feats, idx = mean[order], coords[order].astype(np.int32)
    feats.setflags(write=False)
    idx.setflags(write=False)
    return Want(feats, idx, np.asarray(counts + [sum(counts)], dtype=np.int32), any(n >= c.max_voxels for n in counts))


def concatenated(case):
    """(points [P, 4] float32, offsets [n + 1] int32) of a case."""
    pts = np.concatenate(case.clouds).astype(F32) if case.clouds else np.zeros((0, 4), F32)
    off = np.concatenate([[0], np.cumsum([len(c) for c in case.clouds])]).astype(np.int32)
    return pts, off


# ---- what both test files do with a case ---------------------------------------------------------------------------------------------------------------------
def sites(case, capacity=None, device="cpu"):
    pts, off = concatenated(case)
    cap = max(len(pts), 1) if capacity is None else capacity
    return sparse3d.voxel_sites(torch.from_numpy(pts).to(device), torch.from_numpy(off).to(device), case.voxel_size, case.lidar_range, case.shape, case.max_points,
                                case.max_voxels, cap, ego_filter=case.ego, filter_range=case.filter_range)


def check(case, got, capacity=None):
    """``got``: a SparseTensor3d on any device.  Features, indices, count, cloud counts and both status bits against the oracle's chain, exactly."""
    want = reference(case.name)
    kept = len(want.features)
    rows = kept if capacity is None else min(kept, capacity)
    count, status = int(got.count.cpu()[0]), int(got.status.cpu()[0])
    print(f"{case.name}: {sum(len(c) for c in case.clouds)} points, {kept} voxels kept, count {count}, status {status}")
    assert got.count.dtype == torch.int32 and count == rows
    assert got.batch_size == len(case.clouds) and tuple(got.spatial_shape) == tuple(case.shape)
    assert torch.equal(got.indices[:rows].cpu(), torch.from_numpy(want.indices[:rows].copy()))
    assert torch.equal(got.features[:rows].cpu().view(torch.int32), torch.from_numpy(want.features[:rows].copy()).view(torch.int32))        # the bits
    assert torch.equal(got.cloud_counts.cpu(), torch.from_numpy(want.cloud_counts.copy()))
    assert bool(status & ops.SP3D_STATUS_OVERFLOW) == (kept > rows)
    assert bool(status & ops.SP3D_STATUS_MAX_VOXELS) == want.reached
    return want


def model_clouds(model, seed):
    """Two clouds inside the mini model's range: a few hundred points on a wavy ground and two box shells, several points per voxel here and there."""
    rs = np.random.RandomState(seed)
    lo, hi = np.asarray(model.lidar_range[:3]), np.asarray(model.lidar_range[3:])
    out = []
    for b in range(2):
        n = 700 + 50 * b
        xy = lo[:2] + rs.uniform(size=(n, 2)) * (hi - lo)[:2] * np.asarray([0.5, 0.5]) + np.asarray([3.0 * b, 1.0])
        z = -1.6 + 0.3 * np.sin(xy[:, 0] / 2.0) + rs.uniform(-0.05, 0.05, size=n)
        pts = np.concatenate([xy, z[:, None], rs.uniform(size=(n, 1))], axis=1)
        pts = np.concatenate([pts, pts[: n // 3] + rs.uniform(-0.03, 0.03, size=(n // 3, 4)) * [1, 1, 1, 0]])      # near-duplicates: several points in a voxel
        rs.shuffle(pts)
        out.append(pts.astype(np.float32))
    return out


def oracle_lidar(model, clouds, max_points=5, max_voxels=70000):
    per = [oracle.points_to_voxel(c, model.voxel_size, model.lidar_range, max_points, max_voxels) for c in clouds]
    v, c, n = oracle.collate_voxels(per)
    return {"voxel_features": torch.from_numpy(v), "voxel_coords": torch.from_numpy(c), "voxel_num_points": torch.from_numpy(n)}
