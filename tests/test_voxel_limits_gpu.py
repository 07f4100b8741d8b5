"""GPU half of the voxeliser limit tests: csrc/voxelize.hip against the sequential oracle, bit for bit, on the case table of tests/voxel_cases.py (what each case
reaches is proved on the CPU by tests/test_voxel_limits_cpu.py); gather_kernel alone through the laboratory entry ``coalign_lab_voxelize_gather`` with the order
inside the bucket segments chosen (the selection rounds over LDS and over global memory, which the public entry cannot reach); canaries around outputs and workspace,
stale and 0xFF-filled workspaces; every refusal of the argument contract on real buffers.  Nothing here has a tolerance: counts, coords, num and the voxel words
are equal or the test fails."""
import ctypes

import numpy as np
import pytest
import torch

from coalign_amd import hip, ops
from tests import voxel_cases as vc

pytestmark = pytest.mark.gpu
T = torch.from_numpy
DEV = "cuda:0"
OK, NULL_POINTER, BAD_SHAPE, UNSUPPORTED, WORKSPACE = 0, -1, -2, -3, -4


def _same_voxels(got, ref):
    (gv, gc, gn), gcounts = got
    (rv, rc, rn), rcounts = ref
    assert gcounts == rcounts
    assert np.array_equal(gc, rc) and np.array_equal(gn, rn)
    assert np.array_equal(gv.view(np.uint32), rv.view(np.uint32))       # bit-exact copies, zero padding included


def _voxelize_hip(case):
    clouds, vs, rng, max_points, max_voxels, flags, frange = case.as_tuple()
    off = np.concatenate([[0], np.cumsum([len(c) for c in clouds])]).tolist()
    pts = T(np.concatenate(clouds)).to(DEV)
    v, c, n, counts = ops.voxelize(pts, off, vs, rng, max_points, max_voxels, ego_filter=case.ego, filter_range=frange)
    counts = counts.cpu().tolist()
    m = counts[-1]
    return (v[:m].cpu().numpy(), c[:m].cpu().numpy(), n[:m].cpu().numpy()), counts[:-1]


def _twice_against_the_oracle(case):
    got = _voxelize_hip(case)
    _same_voxels(got, vc.reference(case.name))
    _same_voxels(_voxelize_hip(case), got)


@pytest.mark.parametrize("case", vc.group("a"), ids=lambda c: c.name)
def test_segment_counts(case):
    _twice_against_the_oracle(case)


@pytest.mark.parametrize("case", vc.group("b"), ids=lambda c: c.name)
def test_block_and_cloud_boundaries(case):
    _twice_against_the_oracle(case)


@pytest.mark.parametrize("case", vc.group("c"), ids=lambda c: c.name)
def test_owner_counts(case):
    _twice_against_the_oracle(case)


@pytest.mark.parametrize("case", vc.group("d"), ids=lambda c: c.name)
def test_capacity(case):
    _twice_against_the_oracle(case)


@pytest.mark.parametrize("case", vc.group("e"), ids=lambda c: c.name)
def test_float32_edges(case):
    _twice_against_the_oracle(case)


# ---------------------------------------------------------------------------------------------------------------- hip.lib() directly: canaries, stale state, refusals
class Direct:
    """One call of coalign_voxelize on buffers of its own: outputs prefilled with 7.0 / 7 and three rows longer than the capacity, the workspace exactly
    ``coalign_voxelize_workspace_bytes`` long inside a larger buffer filled with 0x5A."""
    PAD = 4096

    def __init__(self, clouds, vs, rng, max_points, max_voxels, flags=0, frange=None, ws_buf=None):
        self.L = hip.lib()
        self.n_clouds = len(clouds)
        self.off = (ctypes.c_int64 * (len(clouds) + 1))(*np.concatenate([[0], np.cumsum([len(c) for c in clouds])]).tolist())
        self.n = int(self.off[len(clouds)])
        self.pts = T(np.concatenate(clouds)).to(DEV)
        self.vs, self.rng = (ctypes.c_double * 3)(*vs), (ctypes.c_double * 6)(*rng)
        self.fr = None if frange is None else (ctypes.c_double * 6)(*frange)
        self.max_points, self.max_voxels, self.flags = max_points, max_voxels, flags
        self.cap = self.L.coalign_voxelize_capacity(self.n, self.n_clouds, self.vs, self.rng, max_voxels)
        assert self.cap >= 0
        rows = self.cap + 3
        self.voxels = torch.full((rows, max_points, 4), 7.0, device=DEV)
        self.coords = torch.full((rows, 4), 7, dtype=torch.int32, device=DEV)
        self.num = torch.full((rows,), 7, dtype=torch.int32, device=DEV)
        self.counts = torch.full((self.n_clouds + 1,), 7, dtype=torch.int32, device=DEV)
        self.ws_bytes = self.L.coalign_voxelize_workspace_bytes(self.off, self.n_clouds, self.vs, self.rng, max_voxels)
        self.ws = torch.full((self.ws_bytes + self.PAD,), 0x5A, dtype=torch.uint8, device=DEV) if ws_buf is None else ws_buf
        assert self.ws.numel() >= self.ws_bytes

    def call(self, **over):
        a = dict(points=self.pts, off=self.off, n_clouds=self.n_clouds, vs=self.vs, rng=self.rng, max_points=self.max_points, max_voxels=self.max_voxels, flags=self.flags,
                 fr=self.fr, voxels=self.voxels, coords=self.coords, num=self.num, cap=self.cap, counts=self.counts, ws=self.ws, ws_bytes=self.ws_bytes)
        a.update(over)
        p = lambda t: t if isinstance(t, ctypes.c_void_p) else ops._ptr(t)
        return self.L.coalign_voxelize(p(a["points"]), a["off"], a["n_clouds"], a["vs"], a["rng"], a["max_points"], a["max_voxels"], a["flags"], a["fr"], p(a["voxels"]),
                                       p(a["coords"]), p(a["num"]), a["cap"], p(a["counts"]), p(a["ws"]), a["ws_bytes"], ops._stream())

    def untouched(self):
        torch.cuda.synchronize()
        return bool((self.voxels == 7.0).all()) and bool((self.coords == 7).all()) and bool((self.num == 7).all()) and bool((self.counts == 7).all())

    def result(self):
        """The rows in use; rows >= M of all three outputs must still hold the canary."""
        torch.cuda.synchronize()
        counts = self.counts.cpu().tolist()
        m = counts[-1]
        assert 0 <= m <= self.cap
        assert bool((self.voxels[m:] == 7.0).all()) and bool((self.coords[m:] == 7).all()) and bool((self.num[m:] == 7).all())
        return (self.voxels[:m].cpu().numpy(), self.coords[:m].cpu().numpy(), self.num[:m].cpu().numpy()), counts[:-1]


def _oracle(clouds, vs, rng, max_points, max_voxels):
    from oracle import coalign_oracle as oracle
    per = [oracle.points_to_voxel(c, vs, rng, max_points, max_voxels) for c in clouds]
    return oracle.collate_voxels(per), [len(p[0]) for p in per]


def test_canaries_and_stale_workspace():
    """Rows >= M are not written, nothing is written past workspace_bytes, and a workspace that still holds another call's tables -- or 0xFF in every byte --
    gives the same answer as a fresh one."""
    vs, rng = vc.OPV2V_VOXEL, vc.OPV2V_RANGE
    first = [vc.CASES["a_mp32_interleaved"].clouds()[0], vc.region_cloud(1500, 700)]
    d = Direct(first, vs, rng, 32, 70000)
    assert d.call() == OK
    _same_voxels(d.result(), _oracle(first, vs, rng, 32, 70000))
    assert d.result()[1][0] + d.result()[1][1] < d.cap                                            # there are rows past M to watch
    assert bool((d.ws[d.ws_bytes:] == 0x5A).all())
    # the same workspace, unchanged, for a smaller cloud whose big cells differ
    second = [vc.CASES["b_max_voxels_all_cells"].clouds()[0], vc.region_cloud(40, 701, x0=10, y0=10, w=2, h=1)]
    snapshot = d.ws.clone()
    e = Direct(second, vs, rng, 20, 9, ws_buf=d.ws)
    assert e.ws_bytes < d.ws_bytes
    assert e.call() == OK
    _same_voxels(e.result(), _oracle(second, vs, rng, 20, 9))
    assert torch.equal(d.ws[e.ws_bytes:], snapshot[e.ws_bytes:])                                  # beyond its own workspace_bytes the second call wrote nothing
    # ...and filled with 0xFF: every count, offset and row number of the tables starts as -1
    for clouds, mp, mv in ((second, 20, 9), (first, 32, 70000)):
        d.ws.fill_(0xFF)
        f = Direct(clouds, vs, rng, mp, mv, ws_buf=d.ws)
        assert f.call() == OK
        _same_voxels(f.result(), _oracle(clouds, vs, rng, mp, mv))
        assert bool((d.ws[f.ws_bytes:] == 0xFF).all())


def test_one_point_more_than_two_million_is_refused():
    case = vc.CASES["d_two_million_points"]
    d = Direct([vc.d_cloud(1)], list(case.voxel_size), list(case.lidar_range), case.max_points, case.max_voxels)
    assert d.n == vc.MAX_POINTS_PER_CLOUD + 1
    assert d.call() == UNSUPPORTED and d.untouched()
    assert bool((d.ws == 0x5A).all())


def test_argument_contract_on_real_buffers():
    """Every refusal of coalign_voxelize with the status include/coalign_amd.h documents, on real device buffers: the canary outputs stay untouched by every refused
    call; n = 0 answers OK with zero counts and NULL data pointers; the two size queries answer -1 / 0 for the grids the entry refuses."""
    vs, rng = vc.OPV2V_VOXEL, vc.OPV2V_RANGE
    clouds = [vc.region_cloud(300, 710), vc.region_cloud(200, 711)]
    d = Direct(clouds, vs, rng, 8, 500, flags=2, frange=rng)
    L, null = d.L, ctypes.c_void_p(0)
    i64 = lambda *v: (ctypes.c_int64 * len(v))(*v)
    for name in ("off", "vs", "rng"):
        assert d.call(**{name: None}) == NULL_POINTER, name
    for name in ("points", "voxels", "coords", "num", "counts", "ws"):
        assert d.call(**{name: null}) == NULL_POINTER, name
    assert d.call(fr=None) == NULL_POINTER                                                        # the range flag without filter_range
    assert d.call(n_clouds=0) == BAD_SHAPE and d.call(n_clouds=17, off=i64(*range(0, 18 * 20, 20))) == UNSUPPORTED
    assert d.call(max_points=0) == BAD_SHAPE and d.call(max_points=65) == UNSUPPORTED and d.call(max_voxels=0) == BAD_SHAPE
    assert d.call(flags=4) == UNSUPPORTED and d.call(flags=2 | 8) == UNSUPPORTED
    assert d.call(off=i64(1, 300, 500)) == BAD_SHAPE and d.call(off=i64(0, 400, 300)) == BAD_SHAPE and d.call(off=i64(0, 300, 299)) == BAD_SHAPE
    assert d.cap == 500 and d.call(cap=d.cap - 1) == BAD_SHAPE
    assert d.call(ws_bytes=d.ws_bytes - 1) == WORKSPACE
    off4 = lambda t: ctypes.c_void_p(t.data_ptr() + 4)
    assert d.call(points=off4(d.pts)) == UNSUPPORTED and d.call(voxels=off4(d.voxels)) == UNSUPPORTED and d.call(coords=off4(d.coords)) == UNSUPPORTED
    d6, d3 = lambda *v: (ctypes.c_double * 6)(*v), lambda *v: (ctypes.c_double * 3)(*v)
    too_many = (d3(0.25, 0.25, 4), d6(0, 0, 0, 7541 * 0.25, 2781 * 0.25, 4))                       # 7541 x 2781 x 1 = 20 971 521 cells
    flat = (d3(0.4, 0.4, 4), d6(-140.8, -40, 1, 140.8, 40, 1))                                    # a zero-size axis
    limit = (d3(0.25, 0.25, 4), d6(-512, -640, -2, 512, 640, 2))
    assert d.call(vs=too_many[0], rng=too_many[1]) == UNSUPPORTED and d.call(vs=flat[0], rng=flat[1]) == BAD_SHAPE
    assert L.coalign_voxelize_capacity(500, 2, *too_many, 500) == -1 and L.coalign_voxelize_capacity(500, 2, *flat, 500) == -1
    assert L.coalign_voxelize_workspace_bytes(d.off, 2, *too_many, 500) == 0 and L.coalign_voxelize_workspace_bytes(d.off, 2, *flat, 500) == 0
    assert L.coalign_voxelize_capacity(500, 2, *limit, 500) == 500 and L.coalign_voxelize_workspace_bytes(d.off, 2, *limit, 500) > 2 * vc.MAX_CELLS * 16
    assert L.coalign_voxelize_capacity(-1, 2, d.vs, d.rng, 500) == -1 and L.coalign_voxelize_capacity(500, 0, d.vs, d.rng, 500) == -1
    assert L.coalign_voxelize_capacity(500, 2, d.vs, d.rng, 0) == -1 and L.coalign_voxelize_workspace_bytes(d.off, 17, d.vs, d.rng, 500) == 0
    assert d.untouched() and bool((d.ws == 0x5A).all())
    # n = 0: zero counts, OK, no data pointer needed
    assert d.call(off=i64(0, 0, 0), points=null, voxels=null, coords=null, num=null, ws=null, ws_bytes=0, cap=0) == OK
    torch.cuda.synchronize()
    assert d.counts.cpu().tolist() == [0, 0, 0] and bool((d.voxels == 7.0).all()) and bool((d.coords == 7).all()) and bool((d.num == 7).all())
    # and the call nothing is wrong with
    d.counts.fill_(7)
    assert d.call() == OK
    from oracle import coalign_oracle as oracle
    masked = [oracle.mask_points_by_range(c, rng) for c in clouds]
    _same_voxels(d.result(), _oracle(masked, vs, rng, 8, 500))


# ---------------------------------------------------------------------------------------------------------------- gather_kernel alone (laboratory library)
def _gather(t, L=None, **over):
    L = L or hip.lab_lib()
    M = int(t["total"][0])
    dev = {k: T(np.ascontiguousarray(t[k])).to(DEV) for k in ("points", "bucket", "seg", "cellinfo", "biglist", "big_count", "total")}
    cap = M + 2
    voxels = torch.full((cap, t["max_points"], 4), 7.0, device=DEV)
    a = dict(points=dev["points"], n=len(t["points"]), bucket=dev["bucket"], seg=dev["seg"], cellinfo=dev["cellinfo"], biglist=dev["biglist"], big_count=dev["big_count"],
             total=dev["total"], max_points=t["max_points"], voxels=voxels, cap=cap)
    a.update(over)
    p = lambda x: x if isinstance(x, ctypes.c_void_p) else ops._ptr(x)
    rc = L.coalign_lab_voxelize_gather(p(a["points"]), a["n"], p(a["bucket"]), p(a["seg"]), p(a["cellinfo"]), p(a["biglist"]), p(a["big_count"]), p(a["total"]),
                                       a["max_points"], p(a["voxels"]), a["cap"], ops._stream())
    torch.cuda.synchronize()
    return rc, voxels.cpu().numpy()


@pytest.mark.parametrize("name", list(vc.GATHER_TABLES))
def test_gather_kernel_on_chosen_segment_orders(name):
    """The min(count, max_points) smallest indices of every segment, ascending, gathered from the points, then zeros -- whatever the order inside the segment: the
    16-lane path, the one-wavefront rank, the register and the streamed bound, the selection rounds over the LDS copy and over global memory, several of them in one
    table; a big cell whose row is -1 is skipped; rows >= M stay untouched; twice the same."""
    t = vc.gather_table(name)
    M = int(t["total"][0])
    rc, got = _gather(t)
    assert rc == OK
    assert np.array_equal(got[:M].view(np.uint32), t["expected"].view(np.uint32))
    assert (got[M:] == 7.0).all()
    rc, again = _gather(t)
    assert rc == OK and np.array_equal(again.view(np.uint32), got.view(np.uint32))


def test_gather_entry_refuses_what_its_header_says():
    t = vc.gather_table("every_count_random_keep32")
    null = ctypes.c_void_p(0)
    for name in ("points", "bucket", "seg", "cellinfo", "biglist", "big_count", "total", "voxels"):
        rc, out = _gather(t, **{name: null})
        assert rc == NULL_POINTER and (out == 7.0).all(), name
    for over, status in ((dict(max_points=0), BAD_SHAPE), (dict(max_points=65), UNSUPPORTED), (dict(n=0), BAD_SHAPE), (dict(cap=0), BAD_SHAPE),
                         (dict(cap=len(t["points"]) + 1), UNSUPPORTED)):
        rc, out = _gather(t, **over)
        assert rc == status and (out == 7.0).all(), over
    pts = T(np.concatenate([t["points"], t["points"][:1]])).to(DEV)
    spare = torch.full((int(t["total"][0]) + 3, t["max_points"], 4), 7.0, device=DEV)
    assert _gather(t, points=ctypes.c_void_p(pts.data_ptr() + 4))[0] == UNSUPPORTED
    assert _gather(t, voxels=ctypes.c_void_p(spare.data_ptr() + 4))[0] == UNSUPPORTED
    torch.cuda.synchronize()
    assert bool((spare == 7.0).all())
    assert not hasattr(hip.lib(), "coalign_lab_voxelize_gather")                                  # the product library does not contain the entry
