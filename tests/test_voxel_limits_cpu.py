"""CPU half of the voxeliser limit tests: every case of tests/voxel_cases.py reaches the branch of csrc/voxelize.hip it is named for -- proved from the oracle's output
and plain arithmetic on the case --, the C oracle equals the plain-Python loop on every small case (so it is not its own only witness), the float32 edge cases meet a
hand-written expectation list, and the tables of the laboratory entry ``coalign_lab_voxelize_gather`` hold the candidate counts their names promise and restate the
public semantics.  tests/test_voxel_limits_gpu.py then holds the kernels to the oracle on the same cases."""
import numpy as np
import pytest

from oracle import coalign_oracle as oracle
from tests import voxel_cases as vc

SMALL = [c for c in vc.CASES.values() if c.group != "d"]


reference, _reference = vc.reference, vc.reference_with


def _same(got, ref):
    (gv, gc, gn), gcounts = got
    (rv, rc, rn), rcounts = ref
    assert gcounts == rcounts
    assert np.array_equal(gc, rc) and np.array_equal(gn, rn)
    assert np.array_equal(gv.view(np.uint32), rv.view(np.uint32))


def _cells_of(case, cloud=0):
    return vc.cell_index(case.clouds()[cloud], case.voxel_size, case.lidar_range)


def _heads(cells):
    """-> (cells in order of first appearance, index of that first point, point count)."""
    u, first, count = np.unique(cells[cells >= 0], return_index=True, return_counts=True)
    first = np.flatnonzero(cells >= 0)[first]
    o = np.argsort(first)
    return u[o], first[o], count[o]


def _flat(case, coords):
    g = vc.grid_size(case.voxel_size, case.lidar_range).astype(np.int64)
    return (coords[:, -3].astype(np.int64) * g[1] + coords[:, -2]) * g[0] + coords[:, -1]


def test_the_table_is_complete_and_its_rules_are_the_oracles():
    assert {c.group for c in vc.CASES.values()} == set("abcde") and all(c.regime for c in vc.CASES.values())
    assert len(vc.group("a")) == 2 * len(vc.A_MAX_POINTS) and len(vc.group("b")) == 1 + len(vc.B_SIZES) + 1 + 6 + 1 and len(vc.group("c")) == 5
    for c in vc.CASES.values():
        assert np.array_equal(vc.grid_size(c.voxel_size, c.lidar_range), oracle.voxel_grid_size(c.voxel_size, c.lidar_range)), c.name
        clouds, vs, rng, mp, mv, flags, fr = c.as_tuple()
        assert 1 <= len(clouds) <= 16 and 1 <= mp <= 64 and mv >= 1 and flags == (1 if c.ego else 0) + (2 if fr is not None else 0)
    again = vc.cloud_from_pairs(vc.a_pairs(), vc.OPV2V_VOXEL, vc.OPV2V_RANGE, 101, True)
    assert np.array_equal(again, vc.CASES["a_mp32_interleaved"].clouds()[0])                      # seeded: the same bytes on every machine


@pytest.mark.parametrize("case", SMALL, ids=lambda c: c.name)
def test_c_oracle_equals_the_python_loop(case):
    """...and the late-fusion order of the filters (range mask, then ego mask) selects the same points as the intermediate order."""
    _same(_reference(case, oracle.points_to_voxel_python), reference(case.name))
    if case.ego and case.filter_range is not None:
        _same(_reference(case, oracle.points_to_voxel, late_order=True), reference(case.name))


@pytest.mark.parametrize("case", vc.group("a"), ids=lambda c: c.name)
def test_group_a_cells_hold_exactly_the_named_counts(case):
    pairs = dict(case.info)
    assert sorted(pairs.values()) == sorted(vc.A_COUNTS) == [1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 1023, 1024, 1025, 4097]
    cells = _cells_of(case)
    u, n = np.unique(cells, return_counts=True)
    assert dict(zip(u.tolist(), n.tolist())) == pairs                                             # exact, and no point outside the grid
    (rv, rc, rn), counts = reference(case.name)
    assert counts == [len(pairs)]
    assert {int(c): int(k) for c, k in zip(_flat(case, rc), rn)} == {c: min(k, case.max_points) for c, k in pairs.items()}
    ncell, R, _ = vc.owners(case.voxel_size, case.lidar_range)
    assert R == 28
    big = next(c for c, k in pairs.items() if k == 4097)
    assert sum(k for c, k in pairs.items() if c % R == big % R) > vc.K_OWNER_KEEP                 # owner_kernel walks past its register-held points
    assert vc.blocks(len(cells)) == 8
    runs = 1 + int(np.count_nonzero(np.diff(cells)))
    assert runs == len(pairs) if case.name.endswith("contiguous") else runs > 1000


def test_group_b_block_counts_and_head_positions():
    for n in vc.B_SIZES:
        (cloud,) = vc.CASES[f"b_size_{n}"].clouds()
        assert len(cloud) == n and vc.blocks(n) == {0: 0, 1: 1, 1023: 1, 1024: 1, 1025: 2, 2047: 2, 2048: 2, 2049: 3}[n]
    assert tuple(len(c) for c in vc.CASES["b_sizes_together"].clouds()) == vc.B_SIZES
    for a, b in zip(vc.CASES["b_sizes_together"].clouds(), (vc.CASES[f"b_size_{n}"].clouds()[0] for n in vc.B_SIZES)):
        assert np.array_equal(a, b)
    assert reference("b_size_0")[1] == [0] and reference("b_size_1")[1] == [1]
    # heads on the first and last index of a block
    case = vc.CASES["b_heads_on_block_edges"]
    cells, first, count = _heads(_cells_of(case))
    assert first.tolist() == [0, 1023, 1024, 2047, 2999] == list(vc.B_HEADS_AT) and len(case.clouds()[0]) == 3000
    assert cells.tolist() == [c for _, c in case.info] and count[-1] == 1
    (rv, rc, rn), counts = reference(case.name)
    assert counts == [5] and _flat(case, rc).tolist() == cells.tolist() and rn.tolist() == np.minimum(count, 32).tolist()


@pytest.mark.parametrize("case", [c for c in vc.group("b") if c.name.startswith("b_max_voxels")], ids=lambda c: c.name)
def test_group_b_max_voxels_cuts_where_it_says(case):
    cells, first, count = _heads(_cells_of(case))
    assert first.tolist() == list(vc.B_CUT_AT) and len(cells) == 18
    in_block0 = int((first < vc.K_CHUNK).sum())
    assert in_block0 == vc.B_CUT_HEADS_BLOCK0 == 9 and first[8] == 1023 and first[9] == 1024      # last head of block 0, first head of block 1
    assert case.max_voxels in (1, 18, 17, 8, 9, 10)
    (rv, rc, rn), counts = reference(case.name)
    kept = min(case.max_voxels, 18)
    assert counts == [kept] and _flat(case, rc).tolist() == cells[:kept].tolist() and rn.tolist() == np.minimum(count[:kept], case.max_points).tolist()
    if kept < 18 and case.max_voxels != 17:
        assert count[kept:].max() > 16                                                            # a dropped cell on the big-cell list: gather_kernel's v < 0 skip
    assert count[:kept].max() > case.max_points or kept == 1


def test_group_b_sixteen_clouds_clamp_some_and_not_others():
    case = vc.CASES["b_sixteen_clouds"]
    clouds = case.clouds()
    assert len(clouds) == 16 and [len(c) for c in clouds] == list(vc.B_SIXTEEN) and len(clouds[0]) == len(clouds[6]) == len(clouds[15]) == 0
    occupied = [len(np.unique(_cells_of(case, i))) if len(clouds[i]) else 0 for i in range(16)]
    _, counts = reference(case.name)
    assert counts == [min(o, case.max_voxels) for o in occupied]
    assert sum(o > case.max_voxels for o in occupied) >= 3 and sum(0 < o < case.max_voxels for o in occupied) >= 3
    assert len({len(c) for c in clouds}) == 14


@pytest.mark.parametrize("case", vc.group("c"), ids=lambda c: c.name)
def test_group_c_owner_counts(case):
    grid, R, per = vc.C_GRIDS[case.name][2:]
    ncell, gotR, gotper = vc.owners(case.voxel_size, case.lidar_range)
    assert tuple(vc.grid_size(case.voxel_size, case.lidar_range)) == grid == case.info[0] and ncell == grid[0] * grid[1] * grid[2]
    assert (gotR, gotper) == (R, per) and R == -(-ncell // vc.K_RANGE) and per == -(-R // 256)
    assert {"c_one_cell": 1, "c_5120_cells": 5120, "c_5121_cells": 5121, "c_263_owners": 256 * 128 * 41, "c_limit_grid": vc.MAX_CELLS}[case.name] == ncell
    cells, first, count = _heads(_cells_of(case))
    named = vc.c_named_cells(case.voxel_size, case.lidar_range)
    want = {0, ncell - 1} | ({R - 1, R, ncell - R} if ncell > 1 else set())
    assert want <= {c for c, _ in named}
    assert cells[:len(named)].tolist() == [c for c, _ in named]                                   # they open the first voxels
    assert {c: int(k) for c, k in zip(cells[:len(named)], count[:len(named)])} == dict(named)
    assert int((_cells_of(case) < 0).sum()) == 40 and 3000 <= len(case.clouds()[0]) <= 6000
    (rv, rc, rn), counts = reference(case.name)
    kept = min(len(cells), case.max_voxels)
    assert counts == [kept] and _flat(case, rc).tolist() == cells[:kept].tolist()
    if case.name == "c_limit_grid":
        assert len(cells) > case.max_voxels                                                       # the clamp drops cells on this grid too
        assert {int(c) % R for c in cells} >= {0, R - 1} and {int(c) // R for c in cells} >= {0, vc.K_RANGE - 1}


def test_group_d_reaches_the_block_limit_and_both_stride_loops():
    """From the oracle alone: 2048 blocks, more than 131 072 voxels (the 16-lane workgroups stride), more than 32 768 cells of more than 16 points (the
    wavefront-per-cell workgroups stride)."""
    case = vc.CASES["d_two_million_points"]
    (cloud,) = case.clouds()
    assert len(cloud) == 2 * 1024 * 1024 == vc.MAX_POINTS_PER_CLOUD and vc.blocks(len(cloud)) == 2048 == vc.K_MAX_BLOCKS
    assert case.max_voxels == 704 * 200 and case.max_points == 4
    voxels, coords, num = oracle.points_to_voxel(cloud, case.voxel_size, case.lidar_range, 17, case.max_voxels)
    assert len(num) > 131072 == vc.SMALL_STRIDE
    assert int((num == 17).sum()) > 32768 == vc.BIG_STRIDE
    assert len(vc.d_cloud(1)) == vc.MAX_POINTS_PER_CLOUD + 1 and np.array_equal(vc.d_cloud(1)[:-1], cloud)


# ---------------------------------------------------------------------------------------------------------------- group e: the hand-written expectation list
# cell index along the axis of the points (below, at, above) t = float32(lo + k * vs), None = rejected.  Float32 rounding decides, not the real-number picture: at
# y, k = 2 the point ON the edge falls into cell 1, below y's and z's last edge the quotient rounds up to the grid size (rejected), below x's it does not.
CELL_EDGES = {"x": {0: (None, 0, 0), 1: (0, 1, 1), 2: (1, 2, 2), 703: (702, 703, 703), 704: (703, None, None)},
              "y": {0: (None, 0, 0), 1: (0, 1, 1), 2: (1, 1, 2), 199: (198, 199, 199), 200: (None, None, None)},
              "z": {0: (None, 0, 0), 1: (None, None, None), 2: (None, None, None)}}
GRID = {"x": 704, "y": 200, "z": 1}
POS = ("below", "at", "above")
STRICT_DROPS = {"lo": (True, True, False), "hi": (False, True, True)}         # mask_points_by_range keeps lo < p < hi
CLOSED_DROPS = {"lo": (False, True, True), "hi": (True, True, False)}         # mask_ego_points drops lo <= p <= hi


def _voxel_loop_takes(tag):
    f = tag.split(".")
    if f[0] == "cell":
        return CELL_EDGES[f[1]][int(f[2])][POS.index(f[3])] is not None
    if f[0] == "filter" and f[1] == "grid":                                   # the grid range's own bounds: the same points as cell edge 0 and cell edge `grid`
        return CELL_EDGES[f[2]][0 if f[3] == "lo" else GRID[f[2]]][POS.index(f[4])] is not None
    if f[0] in ("filter", "ego"):
        return True
    if f[0] == "special":
        return f[2] in ("mzero", "mdenorm", "pdenorm")                        # NaN, +-Inf and +-1e30 in any coordinate: rejected
    return f[0] == "word" and f[-1] != "rejected"


def _ego_drops(tag):
    f = tag.split(".")
    return f[0] == "ego" and CLOSED_DROPS[f[2]][POS.index(f[3])]


def _range_drops(tag, which):
    f = tag.split(".")
    if f[0] == "filter" and f[1] == which:
        return STRICT_DROPS[f[3]][POS.index(f[4])]
    if which == "tight":                                                      # every cell edge in the list and every bound of the grid range lies outside the tight range
        return f[0] == "cell" or (f[0] == "filter" and f[1] == "grid") or (f[0] == "special" and f[2] not in ("mzero", "mdenorm", "pdenorm")) or f[-1] == "rejected"
    if f[0] == "cell":
        k = int(f[2])
        return STRICT_DROPS["lo"][POS.index(f[3])] if k == 0 else STRICT_DROPS["hi"][POS.index(f[3])] if k == GRID[f[1]] else k > GRID[f[1]]
    if f[0] == "special":
        return f[2] not in ("mzero", "mdenorm", "pdenorm")
    return f[-1] == "rejected"


def _words(points):
    return points[:, 3].view(np.uint32)


@pytest.mark.parametrize("case", [c for c in vc.group("e") if c.name.startswith("e_edges")], ids=lambda c: c.name)
def test_group_e_accepted_and_rejected_sets(case):
    tags, pts = vc.e_points()
    assert np.array_equal(case.clouds()[0].view(np.uint32), pts.view(np.uint32)) and len(set(tags)) == len(tags) == len(pts) and 100 < len(pts) < 1000
    assert len(set(_words(pts).tolist())) == len(pts) - len(vc.E_INTENSITY_WORDS)                 # a row of the output names its source (accepted / rejected twins share a word)
    which = None if case.filter_range is None else "grid" if tuple(case.filter_range) == tuple(vc.OPV2V_RANGE) else "tight"
    want = [i for i, t in enumerate(tags) if _voxel_loop_takes(t) and not (case.ego and _ego_drops(t)) and not (which and _range_drops(t, which))]
    c = pts
    if case.ego:
        c = oracle.mask_ego_points(c)
    if which:
        c = oracle.mask_points_by_range(c, case.filter_range)
    voxels, coords, num = oracle.points_to_voxel(c, case.voxel_size, case.lidar_range, 64, 70000)
    got = np.concatenate([voxels[v, :num[v], 3].view(np.uint32) for v in range(len(num))])
    assert int(num.max()) < 64 and sorted(got.tolist()) == sorted(_words(pts)[want].tolist())
    assert 0 < len(want) < len(pts)
    if not case.ego and which is None:                                                            # the recorded cell of every edge point, and the words bit for bit
        for i, t in enumerate(tags):
            f = t.split(".")
            if f[0] == "cell" and _voxel_loop_takes(t):
                v = next(v for v in range(len(num)) if _words(pts)[i] in voxels[v, :num[v], 3].view(np.uint32))
                assert coords[v][2 - "xyz".index(f[1])] == CELL_EDGES[f[1]][int(f[2])][POS.index(f[3])], t
        assert {w for w in vc.E_INTENSITY_WORDS} <= set(got.tolist())


def test_group_e_triples_are_one_ulp_apart_and_the_filters_cut_where_the_list_says():
    tags, pts = vc.e_points()
    by = dict(zip(tags, pts))
    for t in tags:
        if t.endswith(".at") and not t.startswith("special"):
            axis = "xyz".index(t.split(".")[-3] if t.startswith(("filter", "ego")) else t.split(".")[1])
            lo, at, hi = (by[t[:-2] + p][axis] for p in POS)
            assert lo < at < hi and np.nextafter(lo, np.float32(np.inf)) == at and np.nextafter(at, np.float32(np.inf)) == hi
            trio = np.stack([by[t[:-2] + p] for p in POS])
            if t.startswith("ego"):
                kept = {float(r[axis]) for r in oracle.mask_ego_points(trio)}
                assert [float(v) not in kept for v in (lo, at, hi)] == list(CLOSED_DROPS[t.split(".")[2]]), t
            if t.startswith("filter"):
                rng = vc.OPV2V_RANGE if t.split(".")[1] == "grid" else vc.E_FILTER_TIGHT
                kept = {float(r[axis]) for r in oracle.mask_points_by_range(trio, rng)}
                assert [float(v) not in kept for v in (lo, at, hi)] == list(STRICT_DROPS[t.split(".")[3]]), t


@pytest.mark.parametrize("name", list(vc.E_ZERO_MIN))
def test_group_e_negative_denormals_on_a_range_starting_at_zero(name):
    """-1e-45 / 4 rounds to -0: floor gives -0, cell 0, accepted.  -1e-45 / 0.4 stays a negative denormal: floor gives -1, rejected.  The largest negative denormal
    and the smallest negative normal are rejected by both; -0.0, 0.0 and +1e-45 land in cell 0."""
    case = vc.CASES[name]
    tags, pts = vc.e_zero_points(name)
    takes = {"mdenorm": name == "e_denormal_voxel4", "pdenorm": True, "mzero": True, "pzero": True, "mdenorm_big": False, "mtiny_normal": False}
    assert pts[0, 0] == np.float32(-1e-45) and pts[0, 0] < 0 and pts[0, 0].view(np.uint32) == 0x80000001
    for tag, p in zip(tags, pts):
        _, axis, label = tag.split(".")
        voxels, coords, num = oracle.points_to_voxel(p[None], case.voxel_size, case.lidar_range, 1, 1)
        assert len(num) == int(takes[label]), tag
        if len(num):
            assert coords[0][2 - "xyz".index(axis)] == 0 and np.array_equal(voxels[0, 0].view(np.uint32), p.view(np.uint32))
    (rv, rc, rn), counts = reference(name)
    assert int(rn.sum()) == sum(takes[t.split(".")[2]] for t in tags)


# ---------------------------------------------------------------------------------------------------------------- the laboratory entry's tables
def test_transposed_segments_hold_the_candidate_counts_their_names_promise():
    """gather_kernel's candidate rule in numpy (lane minima over strided shares, the keep-th smallest, the entries <= it): the GPU test cannot quietly run the easy regime."""
    for name, (count, candidates) in vc.GATHER_NAMED_CANDIDATES.items():
        t = vc.gather_table(name)
        order, keep = t["orders"][0], t["max_points"]
        assert len(order) == count and vc.candidate_count(order, keep) == candidates == (keep - 1) * (count // 64) + 1, name
        U = count // 64
        ranks = np.argsort(np.argsort(order))
        for lane in (0, 1, 63):
            assert sorted(ranks[lane::64].tolist()) == list(range(lane * U, lane * U + U))        # lane l's strided share holds the ranks [l U, l U + U)
    regimes = {"transposed_1024_keep32": "register_lds_rounds", "transposed_1024_keep64": "register_lds_rounds", "transposed_4096_keep32": "streamed_global_rounds",
               "transposed_2048_keep64": "streamed_global_rounds", "transposed_4096_keep1": "streamed_direct"}
    for name, regime in regimes.items():
        count, candidates = vc.GATHER_NAMED_CANDIDATES[name]
        assert vc.gather_regime(count, candidates) == regime
    assert 64 < 497 <= 1009 <= vc.K_SEG_LDS < 1985 < 2017


def test_every_gather_table_is_well_formed_and_walks_through_several_regimes():
    seen = set()
    for name in vc.GATHER_TABLES:
        t = vc.gather_table(name)
        n, M, mp = len(t["points"]), int(t["total"][0]), t["max_points"]
        nbig = int(t["big_count"][0])
        assert t["seg"].shape == (M, 2) and len(t["biglist"]) == n // 17 + 1 >= nbig and t["expected"].shape == (M, mp, 4) and 1 <= M <= n
        assert (t["biglist"] >= 0).all() and (t["biglist"] < len(t["cellinfo"])).all()            # every entry names a real cellinfo row
        listed = t["cellinfo"][t["biglist"][:nbig]]
        assert len(set(t["biglist"][:nbig].tolist())) == nbig and (listed[:, 0] > 16).all() and int((listed[:, 3] == -1).sum()) == 1    # one dropped cell on the list
        assert sorted(listed[listed[:, 3] >= 0][:, 3].tolist()) == [v for v in range(M) if t["seg"][v, 1] > 16]
        used = np.zeros(n, bool)
        for start, count in list(map(tuple, t["seg"])) + [tuple(r[[2, 0]]) for r in listed if r[3] < 0]:
            assert 0 <= start and start + count <= n and not used[start:start + count].any()
            used[start:start + count] = True
            idx = t["bucket"][start:start + count]
            assert idx.min() >= 0 and idx.max() < n and len(set(idx.tolist())) == count
        for row in listed[listed[:, 3] >= 0]:
            assert tuple(t["seg"][row[3]]) == (row[2], row[0])
        mine = set()
        for v in range(M):
            count = int(t["seg"][v, 1])
            cand = vc.candidate_count(t["orders"][v], mp) if count > 64 else count
            mine.add(vc.gather_regime(count, cand))
            assert np.array_equal(t["expected"][v, :min(count, mp)], t["points"][np.sort(t["orders"][v])[:mp]]) and not t["expected"][v, min(count, mp):].any()
        assert len(mine) >= 3, (name, mine)
        seen |= mine
    assert seen == {"small", "wave", "register_direct", "register_lds_rounds", "streamed_direct", "streamed_lds_rounds", "streamed_global_rounds"}, seen
    for rule in vc.ORDER_RULES:
        t = vc.gather_table(f"every_count_{rule}_keep32")
        assert sorted(t["seg"][:, 1].tolist()) == sorted(vc.GATHER_COUNTS) == [1, 15, 16, 17, 63, 64, 65, 1024, 1088]


def test_gather_expectation_equals_the_oracle_on_real_cells():
    """Buckets built from a real cloud's cells, voxel rows in order of first appearance: the numpy expectation of the laboratory tables is the oracle's voxel array, for
    every order inside the segments -- the tables restate the public semantics."""
    vs, rng = vc.OPV2V_VOXEL, vc.OPV2V_RANGE
    rs = np.random.RandomState(7)
    cloud = np.concatenate([vc.region_cloud(1500, 600, w=12, h=12), vc.cloud_from_pairs([(5000, 100), (5001, 70), (5002, 17), (5003, 1)], vs, rng, 601)])
    cloud = cloud[rs.permutation(len(cloud))]
    cells = vc.cell_index(cloud, vs, rng)
    order, first, count = _heads(cells)
    sets = [np.flatnonzero(cells == c) for c in order]
    assert max(count) == 100 and sorted(count)[-3] >= 17 and (count == 1).any()
    for mp in (1, 5, 64):
        voxels, coords, num = oracle.points_to_voxel(cloud, vs, rng, mp, 70000)
        for rule in vc.ORDER_RULES:
            t = vc.gather_tables(cloud, sets, [rule] * len(sets), mp, seed=mp)
            assert np.array_equal(t["expected"].view(np.uint32), voxels.view(np.uint32)), (mp, rule)
            assert t["seg"][:, 1].tolist() == count.tolist() and np.minimum(count, mp).tolist() == num.tolist()


def test_lab_entry_lives_in_the_laboratory_library_only_and_refuses_before_any_launch():
    """NULL pointers, max_points outside 1..64, empty or oversized tables and misaligned float4 / int4 / int2 pointers are answered before anything is launched, so
    this runs without a GPU; the product library does not export the entry, and the table in coalign_amd.hip binds it."""
    import ctypes
    from coalign_amd import hip
    assert "coalign_lab_voxelize_gather" in hip.LAB_SIGNATURES and not any("coalign_lab_voxelize_gather" in t for t in hip.HEADERS.values())
    assert not hasattr(hip.lib(), "coalign_lab_voxelize_gather")
    L = hip.lab_lib()
    one, null = ctypes.c_void_p(4096), ctypes.c_void_p(0)

    def call(n=100, max_points=32, cap=10, **ptr):
        a = {k: one for k in ("points", "bucket", "seg", "cellinfo", "biglist", "big_count", "total", "voxels")}
        a.update(ptr)
        return L.coalign_lab_voxelize_gather(a["points"], n, a["bucket"], a["seg"], a["cellinfo"], a["biglist"], a["big_count"], a["total"], max_points, a["voxels"], cap, null)

    for name in ("points", "bucket", "seg", "cellinfo", "biglist", "big_count", "total", "voxels"):
        assert call(**{name: null}) == -1, name
    assert call(max_points=0) == -2 and call(n=0) == -2 and call(cap=0) == -2
    assert call(max_points=65) == -3 and call(cap=101) == -3 and call(n=(1 << 30) + 1, cap=10) == -3
    for name, off in (("points", 4), ("voxels", 8), ("cellinfo", 4), ("seg", 4)):
        assert call(**{name: ctypes.c_void_p(4096 + off)}) == -3, name
