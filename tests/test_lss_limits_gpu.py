"""GPU half of the frustum-pooling limit tests (csrc/lss_pool.hip), on the case tables of tests/lss_limit_cases.py (what each case reaches is proved on the CPU by
tests/test_lss_limits_cpu.py):

  A  ``lss_pool`` on the list-length ladder, C = 64 and 128: the project's element-wise bound against the float64 restatement; a derived bound on the summation
     alone, per cell; the workgroup route against the wavefront route bit for bit (every chunk a cell of its own, then added in chunk order on the host);
     written everywhere; repeatable.
  B  ``coalign_lss_pool`` through the C ABI on an index that breaks its own rules, against the header's rule in numpy.  Every buffer is an interior view of a
     larger allocation of the test's own and every corrupted value lies next to the valid range, so a missing clamp reads the test's padding -- a wrong value,
     never a stray access.
  C  ``lss_cells`` on rigs where nothing rounds: equal to the restatement on every point, the points exactly on a cell boundary included.
  D  ``lss_depth_prob`` against the float64 softmax, element by element, and the confinement of a non-finite pixel.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

from conftest import assert_elementwise
from coalign_amd import hip, ops
import lss_limit_cases as LC
import lss_reference as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
T = torch.from_numpy


# ---- A: the ladder ------------------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _ladder(C):
    """One run of the ladder per channel count, shared by its tests (never modified): the map written into a NaN-filled buffer, as rows [70, C]."""
    A, N, D, fH, fW = LC.LADDER_FRUSTUM
    nx, ny, nz = LC.LADDER_GRID
    logit, x = R.features(A * N, C, D, fH, fW, seed=200 + C)
    ix = LC.index_on(LC.ladder_index(), DEV)
    out = torch.full((A, ny, nx, nz * C), float("nan"), device=DEV).permute(0, 3, 1, 2)
    got = ops.lss_pool(logit.to(DEV), x.to(DEV), ix, out=out)
    assert got.data_ptr() == out.data_ptr()
    return {"logit": logit, "x": x, "ix": ix, "map": got.cpu(), "rows": got.permute(0, 2, 3, 1).reshape(A * ny * nx, nz * C).cpu()}


@pytest.mark.parametrize("C", [64, 128])
def test_ladder_within_the_project_bound_of_float64(C):
    run = _ladder(C)
    ref = R.pool_f64(run["logit"], run["x"], LC.ladder_cells(), LC.LADDER_FRUSTUM[0], LC.LADDER_GRID)
    print(f"\nladder, C {C}: kernel {assert_elementwise(run['map'], ref, f'ladder C {C}'):.2e} of the scale")
    lens = LC.ladder_lengths()
    err = (run["rows"].double() - ref.permute(0, 2, 3, 1).reshape(len(lens), C)).abs().amax(1) / ref.abs().max()
    for k in np.flatnonzero(lens > LC.CHUNK):
        print(f"  key {k:2d}, {lens[k]:4d} points in {-(-lens[k] // LC.CHUNK)} chunks: {float(err[k]):.2e}")


@pytest.mark.parametrize("C", [64, 128])
def test_ladder_summation_alone_within_its_forward_bound(C):
    """Against the float64 sum of the kernel's OWN float32 probabilities x features, per cell and channel: |got - sum| <= (n + chunks) 2^-24 sum |p x| -- n roundings
    of the fma chain and one per chunk sum, no measured constant.  The softmax's error is not in it, so a dropped or doubled point (an error of a whole term, about
    1 / n of the sum of magnitudes, against a bound of n 2^-24 of it) fails here."""
    run = _ladder(C)
    A, N, D, fH, fW = LC.LADDER_FRUSTUM
    prob = ops.lss_depth_prob(run["logit"].to(DEV)).cpu().numpy()
    rows = run["x"].permute(0, 2, 3, 1).reshape(A * N * fH * fW, C).numpy()
    ix = LC.ladder_index()
    want, mag = LC.sum_f64(rows, prob, ix.points.numpy(), ix.starts.numpy())
    lens = LC.ladder_lengths()
    bound = LC.summation_bound(lens, mag)
    err = np.abs(run["rows"].double().numpy() - want)
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio = np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0)).max(1)
    worst = int(ratio.argmax())
    print(f"\nladder, C {C}: worst error / bound {ratio.max():.3f} at key {worst} ({lens[worst]} points); long lists: " + ", ".join(f"{lens[k]}: {ratio[k]:.3f}" for k in np.flatnonzero(lens > LC.CHUNK)))
    bad = np.flatnonzero(ratio > 1)
    assert bad.size == 0, f"lists of {lens[bad].tolist()} points outside the summation bound, error / bound {ratio[bad].tolist()}"


@pytest.mark.parametrize("C", [64, 128])
def test_ladder_workgroup_route_equals_the_wavefront_route_bit_for_bit(C):
    """The header's "added in chunk order": every chunk summed on its own by the wavefront route (a second index over the same points in which each chunk is a
    cell), the chunk rows then added in float32 from zero, in chunk order, on the host -- the long cell's row of the real result has exactly those bits.  A skipped,
    repeated, stale or misordered chunk sum in any round of the loop fails this."""
    run = _ladder(C)
    cx, owner = LC.chunk_index(LC.ladder_index())
    pieces = ops.lss_pool(run["logit"].to(DEV), run["x"].to(DEV), LC.index_on(cx, DEV))
    assert tuple(pieces.shape) == (1, C, 1, cx.cells)
    pieces = pieces.permute(0, 2, 3, 1).reshape(cx.cells, C).cpu()
    want = torch.zeros_like(run["rows"])
    for j, k in enumerate(owner):                               # (ascending: chunk order within a key)
        want[k] = want[k] + pieces[j]
    lens = LC.ladder_lengths()
    wrong = [int(lens[k]) for k in range(len(lens)) if not torch.equal(run["rows"][k], want[k])]
    assert not wrong, f"lists of {wrong} points differ from the sum of their chunks"
    assert all(np.array_equal(run["rows"][k].numpy().view(np.uint32), pieces[owner.index(k)].numpy().view(np.uint32)) for k in np.flatnonzero((lens > 0) & (lens <= LC.CHUNK)))


@pytest.mark.parametrize("C", [64, 128])
def test_ladder_written_everywhere_and_repeatable(C):
    run = _ladder(C)
    lens = LC.ladder_lengths()
    assert bool(torch.isfinite(run["rows"]).all())              # (the buffer was full of NaN)
    assert float(run["rows"][lens == 0].abs().max()) == 0.0 and bool((run["rows"][lens > 0].abs().amax(1) > 0).all())
    again = ops.lss_pool(run["logit"].to(DEV), run["x"].to(DEV), run["ix"])
    assert torch.equal(again.cpu(), run["map"])
    assert np.array_equal(again.cpu().numpy().view(np.uint32), run["map"].numpy().view(np.uint32))


# ---- B: the index contract, through the C ABI ---------------------------------------------------------------------------------------------------------------------
PAD = 4                     # spare rows / entries on either side of every buffer
PREFILL = -7.0


def _framed(values, fill, pad):
    """``values`` in the middle of a larger device buffer filled with ``fill`` -> (the buffer, the interior view)."""
    values = T(np.array(values))
    buf = torch.empty((values.shape[0] + 2 * pad,) + tuple(values.shape[1:]), dtype=values.dtype, device=DEV)
    buf[:] = torch.as_tensor(fill, dtype=values.dtype, device=DEV)
    inner = buf[pad:pad + values.shape[0]]
    inner.copy_(values)
    return buf, inner


def _call(case, x=None, points=None, starts=None, long_cells=None):
    """coalign_lss_pool on framed buffers.  Padding: feature rows and probabilities of 1e30; index entries that name the sentinel feature row (the last row,
    1e30, which no list uses); starts of 0; the true long key; output rows of 1e30 around an interior of -7.  -> out [cells, C] on the host."""
    rows, D, C, cells = case["rows"], case["D"], case["C"], case["cells"]
    x = np.array(case["x"] if x is None else x, np.float32)
    x[rows - 1] = LC.SENTINEL
    points = case["points"] if points is None else points
    starts = case["starts"] if starts is None else starts
    long_cells = case["long_cells"] if long_cells is None else np.asarray(long_cells, np.int32)
    xb, xv = _framed(x, LC.SENTINEL, PAD)
    pb, pv = _framed(case["prob"], LC.SENTINEL, 2 * D)
    ib, iv = _framed(np.ascontiguousarray(points, np.int32), [rows - 1, (rows - 1) * D], PAD)
    sb, sv = _framed(np.ascontiguousarray(starts, np.int32), 0, PAD)
    lb, lv = _framed(long_cells, LC.CONTRACT_LONG_KEY, PAD)
    ob, ov = _framed(np.full((cells, C), PREFILL, np.float32), LC.SENTINEL, PAD)
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())
    assert all(t.data_ptr() % a == 0 for t, a in ((xv, 16), (ov, 16), (iv, 8), (pv, 4), (sv, 4), (lv, 4)))
    status = hip.lib().coalign_lss_pool(ptr(xv), ptr(pv), rows, C, D, ptr(iv), len(points), ptr(sv), cells, ptr(lv), len(long_cells), ptr(ov), ops._stream())
    torch.cuda.synchronize()
    assert status == 0
    assert bool((ob[:PAD] == LC.SENTINEL).all()) and bool((ob[PAD + cells:] == LC.SENTINEL).all())      # nothing written around the output
    return ov.cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _rule(case, x=None, points=None, starts=None, long_cells=None):
    x = np.array(case["x"] if x is None else x, np.float32)
    x[case["rows"] - 1] = LC.SENTINEL
    return LC.pool_rule(x, case["prob"], case["points"] if points is None else points, case["starts"] if starts is None else starts,
                        case["long_cells"] if long_cells is None else long_cells, case["rows"], case["D"])


def _assert_rule(got, rule, what):
    """Written rows within the summation bound of the rule's float64 value, unwritten rows still the prefill."""
    out, mag, count, written, _ = rule
    assert (got[~written] == PREFILL).all(), what
    err, bound = np.abs(got.astype(np.float64) - out), LC.summation_bound(count, mag)
    bad = np.flatnonzero(~(err <= bound).all(1) & written)
    assert bad.size == 0, f"{what}: rows {bad.tolist()} differ from the header's rule by up to {np.nanmax(err[bad]) if np.isfinite(err[bad]).any() else float('nan'):.3e} (bound {bound[bad].max():.3e}); got {got[bad][:, 0].tolist()}"


@functools.lru_cache(maxsize=None)
def _consistent(C):
    case = LC.contract_case(C)
    got = _call(case)
    _assert_rule(got, _rule(case), "the consistent index")
    assert np.array_equal(_bits(got), _bits(_call(case)))
    return got


@pytest.mark.parametrize("row0", ["finite", "inf", "nan"])
@pytest.mark.parametrize("C", [64, 128])
def test_entries_outside_the_buffers_are_skipped(C, row0):
    """Twenty entries with a row of rows, rows + 1 or -1, or a probability index of rows D or -1, in a short list and in the first, middle and last chunk of the long
    one: they contribute nothing -- also when feature row 0 is +inf or NaN (a kernel that turns such an entry into 0 x row 0 poisons the cell) -- and every list
    without such an entry keeps its bits.  No list of the case uses row 0, so the expectation is finite everywhere."""
    case = LC.contract_case(C)
    pts, _ = LC.corrupt_entries(case)
    x = case["x"].copy()
    if row0 != "finite":
        x[0] = float(row0)
    got = _call(case, x=x, points=pts)
    assert np.isfinite(got).all(), f"row 0 = {row0}: a skipped entry made cells {np.flatnonzero(~np.isfinite(got).all(1)).tolist()} non-finite"
    _assert_rule(got, _rule(case, x=x, points=pts), f"row 0 = {row0}")
    hit = np.zeros(case["cells"], bool)
    hit[[LC.CONTRACT_SHORT_KEY, LC.CONTRACT_LONG_KEY]] = True
    clean = _consistent(C)                                      # (no list uses row 0: the consistent call with the finite row is the reference for the bits)
    assert np.array_equal(_bits(got[~hit]), _bits(clean[~hit])) and (got[hit] != clean[hit]).any(1).all()


@pytest.mark.parametrize("C", [64, 128])
def test_corrupt_starts_empty_their_lists_and_no_other(C):
    case = LC.contract_case(C)
    clean = _consistent(C)
    before = list(zip(case["starts"][:-1].tolist(), case["starts"][1:].tolist()))
    for name, (starts, emptied) in LC.corrupt_starts(case).items():
        got = _call(case, starts=starts)
        rule = _rule(case, starts=starts)
        assert (got[emptied] == 0).all() and (clean[emptied] != 0).any(1).all(), name
        same = [k for k in range(case["cells"]) if rule[4][k] == before[k]]
        assert len(same) >= case["cells"] - 3 and np.array_equal(_bits(got[same]), _bits(clean[same])), name
        _assert_rule(got, rule, name)


@pytest.mark.parametrize("C", [64, 128])
def test_corrupt_long_cells(C):
    """A short key, ``cells``, -1 and the true long key twice in ``long_cells``: the same bits as the consistent call.  The long key missing: its row keeps the
    prefill (the header says that "every element is written" presumes a complete ``long_cells``), every other row keeps its bits."""
    case = LC.contract_case(C)
    clean = _consistent(C)
    k = LC.CONTRACT_LONG_KEY
    got = _call(case, long_cells=[LC.CONTRACT_SHORT_KEY, case["cells"], -1, k, k])
    assert np.array_equal(_bits(got), _bits(clean))
    for listed in ([], [LC.CONTRACT_SHORT_KEY, case["cells"], -1]):
        got = _call(case, long_cells=listed)
        others = np.arange(case["cells"]) != k
        assert (got[k] == PREFILL).all() and np.array_equal(_bits(got[others]), _bits(clean[others])), listed
        _assert_rule(got, _rule(case, long_cells=listed), f"long_cells = {listed}")


@pytest.mark.parametrize("value", ["nan", "inf"])
@pytest.mark.parametrize("C", [64, 128])
def test_a_non_finite_feature_row_stays_in_the_cells_that_list_it(C, value):
    case = LC.contract_case(C)
    clean = _consistent(C)
    b = int(case["starts"][LC.CONTRACT_LONG_KEY])
    row = int(case["points"][b + 600, 0])                       # a row of the long list's second chunk
    lens = np.diff(case["starts"])
    listed = np.zeros(case["cells"], bool)
    listed[np.repeat(np.arange(case["cells"]), lens)[case["points"][:, 0] == row]] = True
    assert listed[LC.CONTRACT_LONG_KEY] and 1 <= listed.sum() < (lens > 0).sum() and row != case["rows"] - 1
    x = case["x"].copy()
    x[row] = float(value)
    got = _call(case, x=x)
    assert not np.isfinite(got[listed]).any() and np.isfinite(got[~listed]).all()
    assert np.array_equal(_bits(got[~listed]), _bits(clean[~listed]))


# ---- C: lss_cells on exact lattices -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(LC.CELL_CASES))
def test_cells_on_exact_lattices(name):
    """Nothing rounds on these rigs (proved on the CPU), so the kernel's cells equal the restatement's on every point: coordinates exactly 0, 1, n - 1, n, -1, -0.5,
    -0.0, one float32 ulp either side of 1 and n, +-2^31 and 2^31 - 1, NaN and infinite translations, a depth of 0, and 255 / 256 / 257 points per camera."""
    case = LC.CELL_CASES[name]
    v, cell = LC.cell_args(case)
    axes = [T(case[k]).to(DEV) for k in ("xs", "ys", "ds")]
    got = ops.lss_cells(*R.rig_tensors(case["rig"], DEV), *axes, case["lower"], LC.CELL_DX, LC.CELL_N, case["N"]).cpu().numpy()
    assert got.shape == cell.shape and got.dtype == np.int32
    wrong = np.argwhere(got != cell)
    assert wrong.size == 0, f"{name}: {len(wrong)} of {cell.size} points; first (m, d, h, w) = {wrong[0].tolist()}: v = {v[tuple(wrong[0])].tolist()}, kernel {got[tuple(wrong[0])]}, restatement {cell[tuple(wrong[0])]}"
    print(f"\n{name}: {cell.size} points, {int((cell >= 0).sum())} kept, all equal")


# ---- D: lss_depth_prob --------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pixels", list(LC.PROB_PIXELS))
@pytest.mark.parametrize("D", LC.PROB_DEPTHS)
def test_depth_prob_against_float64(D, pixels):
    """|p - p64| <= p64 (|x - max| + 8) 2^-23 + 2^-126 per element (``LC.prob_bound``) for every kind of logits; -inf bins give exactly 0 and the rest still sums to
    1; all-equal rows give 1 / D to the division's rounding; plain and channels-last memory give equal bits.  The worst error / bound is printed, float32
    ``torch.softmax`` on the same device beside it."""
    for kind in LC.PROB_KINDS:
        x = LC.prob_logits(kind, D, pixels)
        p64 = LC.softmax_f64(x)
        bound = LC.prob_bound(x, p64)
        got = ops.lss_depth_prob(x.to(DEV))
        assert tuple(got.shape) == (pixels, D) and got.dtype == torch.float32
        assert torch.equal(got, ops.lss_depth_prob(x.to(DEV).contiguous(memory_format=torch.channels_last))), kind
        got = got.cpu().double()
        lib = torch.softmax(x.to(DEV), 1).permute(0, 2, 3, 1).reshape(pixels, D).cpu().double()
        r_k, r_l = float(((got - p64).abs() / bound).max()), float(((lib - p64).abs() / bound).max())
        print(f"\nD {D}, {pixels} pixels, {kind}: worst error / bound: kernel {r_k:.3f}, float32 torch.softmax {r_l:.3f}")
        assert r_k <= 1.0, f"{kind}: the kernel is outside the bound ({r_k:.3f} of it); float32 torch.softmax is at {r_l:.3f} of it ({'outside too' if r_l > 1 else 'inside'})"
        assert float((got.sum(1) - 1).abs().max()) <= (D + 1) * 2.0 ** -24, kind       # D - 1 roundings of the sum, one of the division, the host adds in float64
        if kind == "masked":
            gone = torch.isinf(x).permute(0, 2, 3, 1).reshape(pixels, D)
            assert bool((got[gone] == 0).all()) and bool((got[~gone] > 0).all())
        if kind == "equal":
            assert float((got * D - 1).abs().max()) <= 2.0 ** -24                        # exp(0) = 1 and the sum D are exact: one rounding, the division's


def test_a_non_finite_pixel_stays_in_its_own_outputs():
    """A pixel whose logits are all -inf, one with a NaN (first bin, last bin) and one with +inf give NaN in that pixel's D outputs, as float64 ``torch.softmax``
    does; every other pixel keeps its bits -- in both memory layouts."""
    clean = LC.prob_logits("gauss3", 127, 257)
    x, pixels = LC.prob_poison(clean)
    bad = torch.zeros(257, dtype=torch.bool)
    bad[list(pixels)] = True
    assert bool(torch.isnan(LC.softmax_f64(x)[bad]).all())
    want = ops.lss_depth_prob(clean.to(DEV)).cpu()
    for layout in (torch.contiguous_format, torch.channels_last):
        got = ops.lss_depth_prob(x.to(DEV).contiguous(memory_format=layout)).cpu()
        for p, what in pixels.items():
            assert bool(torch.isnan(got[p]).all()), (what, got[p][:4].tolist())
        assert bool(torch.isfinite(got[~bad]).all()) and np.array_equal(_bits(got[~bad].numpy()), _bits(want[~bad].numpy()))
