"""Case tables of the frustum-pooling limit tests (csrc/lss_pool.hip: ``lss_pool``, ``lss_cells``, ``lss_depth_prob``), built on the CPU, seeded and deterministic.
tests/test_lss_limits_cpu.py proves that every case reaches the branch it is named for; tests/test_lss_limits_gpu.py holds the kernels to their references on
the same cases.

  A  ``ladder_*``    hand-made cells whose lists have exactly the lengths at which ``sum_points`` and the long-list loop of ``lss_pool`` change their path, and a
                     numpy model of the split rule (``split_model``);
  B  ``contract_*``  a small consistent index, its corruptions, and the header's rule for an inconsistent index in numpy (``pool_rule``);
  C  ``CELL_CASES``  camera rigs and axes on which every float64 operation of ``lss_cells`` is exact, so that cell boundaries are hit exactly;
  D  ``PROB_*``      shapes and logits of the softmax.
"""
import functools
from fractions import Fraction

import numpy as np
import torch

from coalign_amd import ops
import lss_reference as R

CHUNK = ops.LSS_CHUNK
U24 = 2.0 ** -24


# ---- A: the list-length ladder ------------------------------------------------------------------------------------------------------------------------------------
# wavefront route: the 8-way walk with every tail 0 .. 7, the 64-entry batch on both sides, the hand-over at 512.  (3, 5, 6 and 12 are there for the tails 3, 5, 6
# and 4, which the other lengths do not leave.)
LADDER_WAVE = (1, 2, 3, 5, 6, 7, 8, 9, 12, 15, 16, 17, 63, 64, 65, 71, 72, 73, 127, 128, 129, 511, 512)
# workgroup route: 2, 2, 3, 4, 4, 5, 5, 6, 7, 8 and 9 chunks -- one, two and three rounds of the c0 loop, 1 .. 4 chunk sums in a last round; 3 244 is the longest list
# of the cfg-5 rig
LADDER_GROUP = (513, 1024, 1025, 2047, 2048, 2049, 2560, 2561, 3244, 4096, 4097)
LADDER_FRUSTUM = (2, 4, 80, 6, 8)              # A, N, D, fH, fW: 15 360 points per agent
LADDER_GRID = (7, 5, 1)                        # nx, ny, nz: 35 cells per agent, 70 keys -- no multiple of 4: the last workgroup of the per-cell part has two idle wavefronts
# per agent {cell: list length}.  Long lists on key 0 and on the last key (69), never on adjacent keys; every cell not named is empty.
LADDER_PLACEMENT = (
    {0: 4097, 2: 1, 4: 2, 6: 7, 9: 2561, 11: 8, 13: 9, 18: 3244, 20: 15, 22: 16, 24: 17, 27: 4096, 29: 3, 31: 5, 33: 6, 34: 12},
    {0: 63, 1: 64, 2: 65, 4: 2049, 6: 71, 7: 72, 9: 2048, 11: 73, 12: 127, 14: 2047, 16: 128, 17: 129, 19: 1025, 21: 511, 22: 512, 24: 1024, 29: 513, 34: 2560},
)


def ladder_lengths():
    """[70] list length per key."""
    nx, ny, nz = LADDER_GRID
    n = np.zeros(len(LADDER_PLACEMENT) * nx * ny * nz, np.int64)
    for a, table in enumerate(LADDER_PLACEMENT):
        for c, length in table.items():
            n[a * nx * ny * nz + c] = length
    return n


@functools.lru_cache(maxsize=None)
def ladder_cells(seed=11):
    """int32 [A N, D, fH, fW]: the points of an agent's frustum are dealt to its cells by a seeded permutation, so the rows and probability indices of a list are
    scattered over the cameras, depth bins and pixels; what is left over is dropped (-1)."""
    A, N, D, fH, fW = LADDER_FRUSTUM
    per = N * D * fH * fW
    rs = np.random.RandomState(seed)
    cell = np.full(A * per, -1, np.int32)
    for a, table in enumerate(LADDER_PLACEMENT):
        free = a * per + rs.permutation(per)
        at = 0
        for c in sorted(table):
            cell[free[at:at + table[c]]] = c
            at += table[c]
        assert at <= per
    cell = cell.reshape(A * N, D, fH, fW)
    cell.setflags(write=False)
    return cell


@functools.lru_cache(maxsize=None)
def ladder_index():
    A, N = LADDER_FRUSTUM[:2]
    return ops.build_lss_index(torch.from_numpy(ladder_cells().copy()), A, N, *LADDER_GRID)


def split_model(n):
    """What ``lss_pool`` does with a list of ``n`` points, restated from the kernel: the route, the chunks (``pieces``), per chunk the 64-entry batches (``cnt``),
    per batch the number of 8-groups and the tail, and per round of the long-list loop how many chunk sums wavefront 0 adds (``have``)."""
    route = "empty" if n == 0 else "wavefront" if n <= CHUNK else "workgroup"
    pieces = [min(CHUNK, n - b) for b in range(0, n, CHUNK)]
    batches = [min(64, length - i) for length in pieces for i in range(0, length, 64)]
    have = [min(4, len(pieces) - c0) for c0 in range(0, len(pieces), 4)] if route == "workgroup" else []
    return {"route": route, "pieces": pieces, "batches": batches, "groups8": [c // 8 for c in batches], "tails": [c % 8 for c in batches], "have": have}


def index_on(ix, device):
    return ops.LiftSplatIndex(ix.starts.to(device), ix.points.to(device), ix.long_cells.to(device), ix.order.to(device), ix.dims)


def chunk_index(ix):
    """A second index over the same ``points``: every piece ``ix.chunks()`` names -- a short list, or one chunk of a long one -- is a cell of its own (one agent,
    a grid of n_pieces x 1 x 1) and no list is long, so the wavefront route sums every piece.  -> (index, the key each piece belongs to)."""
    pieces = ix.chunks()
    starts = torch.tensor([b for _, b, _ in pieces] + [ix.n_points], dtype=torch.int32)
    A, N, D, fH, fW = ix.dims[:5]
    return ops.LiftSplatIndex(starts, ix.points, torch.zeros(0, dtype=torch.int32), ix.order, (1, A * N, D, fH, fW, len(pieces), 1, 1)), [k for k, _, _ in pieces]


def sum_f64(x_rows, prob, points, starts):
    """float64 sum per list of prob[p.prob] x_rows[p.row], and of its absolute values, for a CONSISTENT index: ([cells, C], [cells, C])."""
    x_rows, prob, points, starts = (np.asarray(v) for v in (x_rows, prob, points, starts))
    lens = np.diff(starts.astype(np.int64))
    key = np.repeat(np.arange(len(lens)), lens)
    term = prob.reshape(-1).astype(np.float64)[points[:, 1]][:, None] * x_rows.astype(np.float64)[points[:, 0]]
    out, mag = np.zeros((len(lens), x_rows.shape[1])), np.zeros((len(lens), x_rows.shape[1]))
    np.add.at(out, key, term)
    np.add.at(mag, key, np.abs(term))
    return out, mag


def summation_bound(n, mag):
    """The forward bound of the kernel's summation alone: a list of n points in ceil(n / 512) chunks is an fma chain of n roundings plus one add per chunk sum,
    |got - exact| <= (n + chunks) 2^-24 sum |p x|.  n [cells], mag [cells, C]."""
    n = np.asarray(n, np.float64)
    return ((n + np.ceil(n / CHUNK)) * U24)[:, None] * mag


# ---- B: the index contract ----------------------------------------------------------------------------------------------------------------------------------------
CONTRACT_FRUSTUM = (4, 8, 6, 8)                # M (one agent), D, fH, fW: 192 feature rows, 1 536 points
CONTRACT_GRID = (7, 5, 1)
CONTRACT_LONG = 1100                           # 512 + 512 + 76: a first, a middle and a last chunk (the smallest list that has a middle one)
CONTRACT_LONG_KEY, CONTRACT_SHORT_KEY = 2 * 7 + 3, 0
SENTINEL = 1e30


@functools.lru_cache(maxsize=None)
def contract_cells(seed=3):
    """int32 [M, D, fH, fW] in the manner of ``R.skewed_cells``: cell (3, 2) holds 1 100 points, its eight neighbours 1 .. 5, cell (0, 0) 40; no list uses feature
    row 0 (the GPU test makes it +inf or NaN: whatever reaches a cell from it is an entry that should have been skipped) or the LAST row (191: the GPU test fills it
    with 1e30 and lets the padding entries of its ``points`` buffer name it)."""
    M, D, fH, fW = CONTRACT_FRUSTUM
    nx = CONTRACT_GRID[0]
    rs = np.random.RandomState(seed)
    pid = np.arange(M * D * fH * fW)
    row = (pid // (D * fH * fW)) * (fH * fW) + pid % (fH * fW)
    free = rs.permutation(pid[(row != 0) & (row != M * fH * fW - 1)])
    cell = np.full(pid.size, -1, np.int32)
    cell[free[:CONTRACT_LONG]] = CONTRACT_LONG_KEY
    at = CONTRACT_LONG
    for k, (dy, dx) in enumerate((dy, dx) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (dy, dx) != (0, 0)):
        cell[free[at:at + 1 + k % 5]] = CONTRACT_LONG_KEY + dy * nx + dx
        at += 1 + k % 5
    cell[free[at:at + 40]] = CONTRACT_SHORT_KEY
    cell = cell.reshape(M, D, fH, fW)
    cell.setflags(write=False)
    return cell


@functools.lru_cache(maxsize=None)
def contract_case(C):
    """The consistent call of coalign_lss_pool as numpy arrays: x [rows, C] and prob [rows D] float32 (the float32 softmax of moderate logits: no probability is
    0), points [n, 2], starts [cells + 1], long_cells int32; plus the logits, the image features and the cells they came from."""
    M, D, fH, fW = CONTRACT_FRUSTUM
    logit, x_img = R.features(M, C, D, fH, fW, seed=50 + C)
    ix = ops.build_lss_index(torch.from_numpy(contract_cells().copy()), 1, M, *CONTRACT_GRID)
    prob = torch.softmax(logit, 1).permute(0, 2, 3, 1).reshape(-1).contiguous().numpy()
    case = {"x": x_img.permute(0, 2, 3, 1).reshape(M * fH * fW, C).contiguous().numpy(), "prob": prob, "points": ix.points.numpy().copy(), "starts": ix.starts.numpy().copy(),
            "long_cells": ix.long_cells.numpy().copy(), "rows": M * fH * fW, "D": D, "C": C, "cells": ix.cells, "logit": logit, "x_img": x_img}
    for v in case.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return case


def pool_rule(x, prob, points, starts, long_cells, rows, D):
    """The header's rule for ANY index, in float64: a list with b < 0, e > n_points or e < b is empty; an entry whose row is outside [0, rows) or whose
    probability index is outside [0, rows D) contributes nothing -- whatever the feature rows hold; a list longer than a chunk is written only when ``long_cells``
    names it.  -> (out [cells, C], sum of |terms| [cells, C], entries that count [cells], lists written [cells] bool, (b, e) per list after the rule)."""
    x, prob, points, starts = np.asarray(x, np.float64), np.asarray(prob, np.float64), np.asarray(points, np.int64), np.asarray(starts, np.int64)
    cells, n_points = len(starts) - 1, len(points)
    out, mag = np.zeros((cells, x.shape[1])), np.zeros((cells, x.shape[1]))
    count, written, spans = np.zeros(cells, np.int64), np.zeros(cells, bool), []
    named = {int(k) for k in np.asarray(long_cells).reshape(-1) if 0 <= int(k) < cells}
    for k in range(cells):
        b, e = int(starts[k]), int(starts[k + 1])
        if b < 0 or e > n_points or e < b:
            b = e = 0
        spans.append((b, e))
        written[k] = e - b <= CHUNK or k in named
        for r, p in points[b:e]:
            if 0 <= r < rows and 0 <= p < rows * D:
                out[k] += prob[p] * x[r]
                mag[k] += np.abs(prob[p] * x[r])
                count[k] += 1
    return out, mag, count, written, spans


ENTRY_KINDS = ("row=rows", "row=rows+1", "row=-1", "prob=rows*D", "prob=-1")


def corrupt_entries(case):
    """``points`` with twenty entries replaced, every kind of ``ENTRY_KINDS`` once in the short list and in the first, the middle and the last chunk of the long
    one, at offsets that fall into the 8-way walk, its tail, and either side of a 64-entry batch -> (points, [(position, place, kind)]).  Only values just outside
    the valid range."""
    rows, D, s = case["rows"], case["D"], case["starts"]
    pts = case["points"].copy()
    b = int(s[CONTRACT_LONG_KEY])
    places = {"short": (int(s[CONTRACT_SHORT_KEY]), (0, 7, 8, 33, 39)), "first chunk": (b, (0, 63, 64, 300, 511)), "middle chunk": (b + CHUNK, (0, 9, 127, 128, 511)),
              "last chunk": (b + 2 * CHUNK, (0, 31, 64, 70, 75))}
    placed = []
    for place, (base, offsets) in places.items():
        for off, kind in zip(offsets, ENTRY_KINDS):
            at = base + off
            field, value = kind.split("=")
            pts[at, 0 if field == "row" else 1] = {"rows": rows, "rows+1": rows + 1, "-1": -1, "rows*D": rows * D}[value]
            placed.append((at, place, kind))
    return pts, placed


def corrupt_starts(case):
    """Three corruptions of ``starts``, one per call: {name: (starts, keys the rule empties)}."""
    s, n = case["starts"], len(case["points"])
    out = {}
    k = CONTRACT_LONG_KEY - 8                                     # a short list followed by a short list
    t = s.copy()
    t[k + 1] = t[k] - 1
    out["starts[k+1] < starts[k]"] = (t, [k])                     # (list k + 1 now begins earlier and is still a list)
    k = CONTRACT_LONG_KEY + 7
    t = s.copy()
    t[k] = -1
    out["starts[k] = -1"] = (t, [k - 1, k])
    k = CONTRACT_LONG_KEY - 1                                     # the list in front of the long one: the long list loses its begin
    t = s.copy()
    t[k + 1] = n + 1
    out["starts[k+1] = n_points + 1"] = (t, [k, k + 1])
    return out


# ---- C: lss_cells on exact lattices -------------------------------------------------------------------------------------------------------------------------------
CELL_N = (6, 5, 4)                             # nx, ny, nz
CELL_DX = (0.5, 2.0, 1.0)
CELL_LOWER = (-4.0, 8.0, -1.0)
BIG = 2.0 ** 31
EYE = np.eye(3, dtype=np.float32)


def _f32(v):
    a = np.asarray(v, dtype=np.float64)
    assert np.array_equal(a.astype(np.float32).astype(np.float64), a, equal_nan=True), "a case value is no float32"
    return a.astype(np.float32)


def edge_values(n):
    """The coordinates a boundary test needs, in cells: 0, 1, n - 1, n, -1, -0.5, one float32 ulp either side of 1 and of n, and one interior value."""
    one, top = np.float32(1), np.float32(n)
    lo, hi = np.float32(-np.inf), np.float32(np.inf)
    return np.array([0, 1, n - 1, n, -1, -0.5, np.nextafter(one, lo), np.nextafter(one, hi), np.nextafter(top, lo), np.nextafter(top, hi), 2.5], np.float64)


def _rig(rots, trans, intrins, post_rots, post_trans):
    M = len(trans)
    rep = lambda m: np.broadcast_to(np.asarray(m, np.float32), (M, 3, 3)).copy()
    return {"rots": torch.from_numpy(rep(rots)), "trans": torch.from_numpy(np.asarray(trans, np.float32).reshape(M, 3)), "intrins": torch.from_numpy(rep(intrins)),
            "post_rots": torch.from_numpy(rep(post_rots)), "post_trans": torch.from_numpy(np.broadcast_to(np.asarray(post_trans, np.float32), (M, 3)).copy())}


def _shifted(offsets, lower=CELL_LOWER):
    """trans per camera = lower + offset (in cells) x dx: the camera's coordinates are the lattice's plus ``offset``."""
    return [[_f32(lower[k] + o[k] * CELL_DX[k]) if np.isfinite(o[k]) else np.float32(o[k]) for k in range(3)] for o in offsets]


def _scatter(count, mult, mod, shift, scale):
    """``count`` dyadic values that differ between any two positions 256 apart (``mod`` is odd): (i mult mod ``mod`` - shift) scale."""
    return _f32((((np.arange(count) * mult) % mod) - shift) * scale)


def _cell_cases():
    nx, ny, nz = CELL_N
    cases = {}
    # rig 1: rots = intrins = post_rots = I, post_trans = 0: g = (xs ds + t_x, ys ds + t_y, ds + t_z).  Camera 0 sits on the lattice (v = (xs ds / dx_x,
    # ys ds / dx_y, ds)), camera 1 has a NaN and camera 2 an infinite translation, camera 3 is camera 0 moved by one cell in x.
    nan, inf = float("nan"), float("inf")
    cases["identity_edges"] = dict(rig=_rig(EYE, _shifted([(0, 0, 0), (nan, 0, 0), (0, inf, 0), (1, 0, 0)]), EYE, EYE, (0, 0, 0)), xs=_f32(edge_values(nx) * CELL_DX[0]),
                                   ys=_f32(edge_values(ny) * CELL_DX[1]), ds=_f32(edge_values(nz) * CELL_DX[2]), lower=CELL_LOWER, N=4, dead=(1, 2))
    # rig 1 at +-2^31 through a large translation, on a coarse lattice (so that lattice + 2^31 is still exact): v = lattice + 2^31 - 256 per axis in cameras 0 .. 2
    # (the lattice values 255 and 256 give 2^31 - 1 and 2^31), v = lattice - 2^31 in cameras 3 .. 5, camera 6 on the lattice.
    big_lower = (-512.0, 512.0, -256.0)
    coarse = np.array([0, 1, 255, 256], np.float64)
    offs = [tuple((BIG - 256) * (k == a) for k in range(3)) for a in range(3)] + [tuple(-BIG * (k == a) for k in range(3)) for a in range(3)] + [(0, 0, 0)]
    cases["identity_2^31"] = dict(rig=_rig(EYE, _shifted(offs, big_lower), EYE, EYE, (0, 0, 0)), xs=_f32(coarse * CELL_DX[0]), ys=_f32(coarse * CELL_DX[1]), ds=_f32(coarse * CELL_DX[2]),
                                  lower=big_lower, N=7, dead=())
    # rig 1 with a negative depth, x = 0, y > 0 and trans_x = -0.0 over lower_x = +0: every addend of g_x is -0, so v_x = -0.0 (index 0, kept); the same for y in
    # camera 1.  (In round-to-nearest a sum is -0 only when all its addends are; for z that would need f_x < 0 and f_x > 0 at once: v_z = -0.0 cannot occur on rig 1.)
    zero_lower = (0.0, 0.0, -4.0)
    cases["identity_signed_zero"] = dict(rig=_rig(EYE, [[-0.0, 8.0, 0.0], [2.0, -0.0, 0.0]], EYE, EYE, (0, 0, 0)), xs=_f32([0.0, 0.5, 1.0]), ys=_f32([0.0, 2.0, 4.0]), ds=_f32([-1.0, -2.0]),
                                         lower=zero_lower, N=2, dead=())
    # rig 2: a quarter turn about z, intrins [[2, 0, p], [0, 4, q], [0, 0, 1]], post_rots diag(0.5, 0.5, 1), post_trans (0.25, -0.5, 0), p = -2 post_trans_x,
    # q = -2 post_trans_y: g = (-ds ys / 2 + t_x, ds xs + t_y, ds + t_z), so v = (-ds ys, ds xs / 2, ds) in camera 0: the adjugate signs and the axis mapping
    turn = np.array([[0, -1, 0], [1, 0, 0], [0, 0, 1]], np.float32)
    ptx, pty = 0.25, -0.5
    K = np.array([[2, 0, -2 * ptx], [0, 4, -2 * pty], [0, 0, 1]], np.float32)
    PR = np.diag([0.5, 0.5, 1.0]).astype(np.float32)
    cases["rotated_edges"] = dict(rig=_rig(turn, _shifted([(0, 0, 0), (0, 1, 0)]), K, PR, (ptx, pty, 0)), xs=_f32(edge_values(ny) * 2.0), ys=_f32(-edge_values(nx)), ds=_f32(edge_values(nz)),
                                  lower=CELL_LOWER, N=2, dead=())
    # the block arithmetic: D fH fW = 255, 256, 257 points per camera (one block, exactly one, one point into a second), three cameras, the middle one moved
    for D, fH, fW in ((5, 3, 17), (4, 8, 8), (1, 1, 257)):
        for name, rots, K_, PR_, pt in (("identity", EYE, EYE, EYE, (0, 0, 0)), ("rotated", turn, K, PR, (ptx, pty, 0))):
            cases[f"{name}_block_{D * fH * fW}"] = dict(rig=_rig(rots, _shifted([(0, 0, 0), (1, 1, 0), (0, 0, 0)]), K_, PR_, pt), xs=_scatter(fW, 7, 37, 4, 0.125 if name == "identity" else 0.5),
                                                        ys=_scatter(fH, 5, 11, 3, 0.5), ds=_f32([1.0]) if D == 1 else _scatter(D, 3, 7, 0, 0.5), lower=CELL_LOWER, N=3, dead=())
    return cases


CELL_CASES = _cell_cases()


def cell_args(case):
    """The float64 coordinates and cells of a case by the restatement of tests/lss_reference.py -> (v [M, D, fH, fW, 3], cell [M, D, fH, fW])."""
    v = R.scaled_coordinates(case["rig"], case["xs"], case["ys"], case["ds"], case["lower"], CELL_DX)
    return v, R.cells_f64(v, CELL_N)


def kernel_order(case, m, exact=False):
    """v of camera ``m`` in the operation order of the ``lss_cells`` kernel (the library is built with -ffp-contract=off: what is written is what runs), every
    intermediate result recorded: in float64 (numpy), or exactly (``fractions.Fraction`` in object arrays).  -> (v [D, fH, fW, 3], [every intermediate])."""
    lift = (lambda a: np.vectorize(Fraction, otypes=[object])(np.asarray(a, np.float32).astype(np.float64))) if exact else (lambda a: np.asarray(a, np.float32).astype(np.float64))
    zero = Fraction(0) if exact else 0.0
    tape = []

    def t(v):
        tape.append(v)
        return v

    def inverse3(a):
        c00, c01, c02 = t(t(a[4] * a[8]) - t(a[5] * a[7])), t(t(a[5] * a[6]) - t(a[3] * a[8])), t(t(a[3] * a[7]) - t(a[4] * a[6]))
        det = t(t(t(a[0] * c00) + t(a[1] * c01)) + t(a[2] * c02))
        adj = [c00, t(t(a[2] * a[7]) - t(a[1] * a[8])), t(t(a[1] * a[5]) - t(a[2] * a[4])), c01, t(t(a[0] * a[8]) - t(a[2] * a[6])), t(t(a[2] * a[3]) - t(a[0] * a[5])),
               c02, t(t(a[1] * a[6]) - t(a[0] * a[7])), t(t(a[0] * a[4]) - t(a[1] * a[3]))]
        return [t(v / det) for v in adj]

    rig = {k: lift(case["rig"][k].numpy()[m]).reshape(-1) for k in R.CAMS}
    undo, iin = inverse3(rig["post_rots"]), inverse3(rig["intrins"])
    comb = []
    for r in range(3):
        for c in range(3):
            s = zero
            for k in range(3):
                s = t(s + t(rig["rots"][r * 3 + k] * iin[k * 3 + c]))
            comb.append(s)
    xs, ys, ds = lift(case["xs"])[None, None, :], lift(case["ys"])[None, :, None], lift(case["ds"])[:, None, None]
    f = [t(xs - rig["post_trans"][0]), t(ys - rig["post_trans"][1]), t(ds - rig["post_trans"][2])]
    q = [t(t(t(undo[3 * r] * f[0]) + t(undo[3 * r + 1] * f[1])) + t(undo[3 * r + 2] * f[2])) for r in range(3)]
    q[0], q[1] = t(q[0] * q[2]), t(q[1] * q[2])
    lower, dx = lift(case["lower"]), lift(CELL_DX)
    v = []
    for r in range(3):
        g = t(t(t(t(comb[3 * r] * q[0]) + t(comb[3 * r + 1] * q[1])) + t(comb[3 * r + 2] * q[2])) + rig["trans"][r])
        v.append(t(t(g - lower[r]) / dx[r]))
    shape = np.broadcast_shapes(*(np.shape(a) for a in v))
    return np.stack([np.broadcast_to(a, shape) for a in v], -1), tape


def deciding(v, axis):
    """[...] bool: the points whose two OTHER coordinates are inside the grid, so that ``axis`` alone decides between kept and dropped."""
    ok = np.ones(v.shape[:-1], bool)
    for k in range(3):
        if k != axis:
            with np.errstate(invalid="ignore"):
                ok &= (v[..., k] >= 0) & (v[..., k] < CELL_N[k])
    return ok


# ---- D: lss_depth_prob --------------------------------------------------------------------------------------------------------------------------------------------
PROB_DEPTHS = (1, 2, 127, 128)
PROB_PIXELS = {255: (1, 3, 85), 256: (2, 8, 16), 257: (1, 1, 257)}         # pixels: (M, fH, fW) -- one block less one, exactly one (over two cameras), one pixel into a second
PROB_KINDS = ("gauss3", "wide", "masked", "equal")


def prob_logits(kind, D, pixels, seed=0):
    """float32 [M, D, fH, fW]: Gaussian x 3; x 80 / 3 (beyond +-200); Gaussian x 3 with about a third of the bins at -inf, at least one finite bin per pixel;
    rows that are all equal (a different value per pixel)."""
    M, fH, fW = PROB_PIXELS[pixels]
    g = torch.Generator().manual_seed(1000 * D + pixels + seed)
    x = torch.randn(M, D, fH, fW, generator=g) * 3.0
    if kind == "wide":
        x = x * (80.0 / 3.0)
    elif kind == "masked":
        gone = torch.rand(M, D, fH, fW, generator=g) < 0.35
        keep = torch.randint(0, D, (M, 1, fH, fW), generator=g)
        gone.scatter_(1, keep, False)
        x = x.masked_fill(gone, float("-inf"))
    elif kind == "equal":
        x = (x[:, :1] * 4.0).expand(M, D, fH, fW).contiguous()
    else:
        assert kind == "gauss3"
    return x


def prob_poison(logit):
    """-> (a copy with four pixels made non-finite, {pixel: what}): pixel 0 all -inf, pixel 100 NaN in bin 0, the last pixel of the first block (255) NaN in the
    last bin, the first pixel of the second block (256) +inf in a middle bin."""
    M, D, fH, fW = logit.shape
    flat = logit.permute(0, 2, 3, 1).reshape(-1, D).clone()
    assert flat.shape[0] > 256
    nan, inf = float("nan"), float("inf")
    flat[0] = -inf
    flat[100, 0] = nan
    flat[255, D - 1] = nan
    flat[256, D // 2] = inf
    return flat.reshape(M, fH, fW, D).permute(0, 3, 1, 2).contiguous(), {0: "all -inf", 100: "NaN first", 255: "NaN last", 256: "+inf"}


def softmax_f64(logit):
    """float64 [M fH fW, D] from float32 logits [M, D, fH, fW]."""
    M, D, fH, fW = logit.shape
    return torch.softmax(logit.double(), 1).permute(0, 2, 3, 1).reshape(M * fH * fW, D)


def prob_bound(logit, p64):
    """|p - p64| <= p64 (|x - max| + 8) 2^-23 + 2^-126 per element: the float32 roundings of x - max and of its product with log2(e) move the result by
    |x - max| 2^-24 each; 8 units of 2^-23 for the hardware exponential, the sum and the division; flush-to-zero of a denormal result below the floor."""
    M, D, fH, fW = logit.shape
    x = logit.double()
    dist = (x - x.amax(1, keepdim=True)).abs().permute(0, 2, 3, 1).reshape(M * fH * fW, D)
    dist = torch.where(torch.isfinite(dist), dist, torch.zeros_like(dist))          # (a -inf bin: p64 = 0, the bound is the floor)
    return p64 * (dist + 8.0) * 2.0 ** -23 + 2.0 ** -126
