"""Pose-aware warp + multi-agent fusion at every agent count, against float64 (csrc/warp_fuse.hip, csrc/warp_fuse_nhwc.hip, through the C ABI).

Both kernels are compiled for NA in {1, 2, 3, 5, 8} agent slots: 4 agents run NA = 5 with a masked slot, 6 and 7 run NA = 8.  Every count 1 ... 8 is
run here, on every route of the NCHW kernel (the LDS patch with its straight-line, masked and two-pass variants; the direct-gather fallback taken for
W % 4 != 0, an unaligned map or a footprint larger than the patch), with the route asserted by construction from the kernel's own predicates.

Yardsticks: the oracle's own functions (``oracle.warp_affine_simple`` / ``att_fuse`` / ``max_fuse``) evaluated on the float32 maps (the reference
itself) and on float64 copies of them, sampling at the reference's float32 positions.  (The oracle's float64 path keeps the float32 grid but redoes
the un-normalise ``(g + 1) * (W / 2) - 0.5`` in float64.  At W = 352 that moves a sample by up to 3e-5 px, and the reference's own float32
evaluation then misses the element-wise bound below at 2 / 47 / 177 elements of the full-size C = 64 ATT / MAX / NONE maps.  Sampling at the float32
ix, iy, which both kernels reproduce bit for bit, leaves it at ~2e-7 of the scale: pure arithmetic.)
  * NONE and MAX do the reference's float32 operations in the reference's order: bit-equal to the float32 oracle, and element-wise close to float64.
  * ATT: element-wise close to float64 (``assert_elementwise``), and the kernel's max error at most 4x the float32 oracle's on the same case
    + 1e-7 of the scale.  Measured kernel / float32-oracle max-error ratios on the MI355X (max over the cases of this file; the median is 1.00
    everywhere, the kernels' largest error 5.5e-7 of the scale): NCHW patch route 1.13 (straight-line, masked and two-pass variants alone: 1.00),
    W % 4 != 0 1.07, unaligned map 1.13, zoomed agent 1.10; channels-last kernel 1.15; the full-size OPV2V frame 1.00 on both kernels.
Values are chosen to expose padded slots (all-negative maps: a MAX started from 0 or a padded slot in the ATT denominator shows; small maps and an
ego out of view: scores near 0, where a padded slot would take a weight near 1) and an unstable softmax (|x| ~ 30 ... 100 at C = 256: the raw
scores overflow float32 exp, only a max-subtracted softmax stays finite).
"""
import numpy as np
import pytest
import torch

from coalign_amd import fusion, ops
from coalign_amd.config import builtin_config
from coalign_amd.pose import get_pairwise_transformation
from coalign_amd.synthetic import make_frame, make_poses
from conftest import assert_elementwise
from oracle import coalign_oracle as oracle

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MODES = (("att", ops.FUSE_ATT), ("max", ops.FUSE_MAX), ("none", ops.FUSE_NONE))
EXP_MAX = 88.72                 # log(FLT_MAX): float32 exp overflows above it


# ------------------------------------------------------------------------------------------------ yardsticks
def logical_rows(groups, rows):
    """Per frame, the physical row of x holding logical agent i -> one index over the whole batch."""
    idx, off = [], 0
    for n in groups:
        idx += [off + int(r) for r in rows[off:off + n]]
        off += n
    return idx


def warp_at_float32_positions(src, theta, dsize):
    """oracle.warp_affine_simple for float64 maps, sampling at the reference's float32 positions ix, iy: the grid handed to
    oracle.grid_sample_bilinear_zeros is the one whose float64 un-normalise lands on them (to ~1e-13 px)."""
    H, W = src.shape[2:]
    ix, iy = sample_positions(theta, H, W, *dsize)
    return oracle.grid_sample_bilinear_zeros(src, torch.stack([(ix.double() + 0.5) / (W / 2.0) - 1.0, (iy.double() + 0.5) / (H / 2.0) - 1.0], -1))


def reference(x, theta, groups, mode, out_hw, dtype, rows=None):
    """The oracle's own functions on ``x.to(dtype)`` (host).  x [n_total, C, H, W] as the kernel reads it, theta [n_total, 2, 3].
    float64: every warp inside them samples at the float32 positions (``warp_at_float32_positions``)."""
    x = x.detach().cpu().contiguous()
    theta = theta.detach().cpu().double()
    if rows is not None:
        x = x[logical_rows(groups, rows)]
    x = x.to(dtype)
    warp = oracle.warp_affine_simple
    if dtype == torch.float64:
        oracle.warp_affine_simple = warp_at_float32_positions          # (att_fuse / max_fuse look it up at call time)
    try:
        if mode == ops.FUSE_NONE:
            return oracle.warp_affine_simple(x, theta, out_hw)
        assert tuple(out_hw) == tuple(x.shape[2:])
        aff = torch.zeros(len(groups), 1, max(groups), 2, 3, dtype=torch.float64)      # row [b, 0, :n] of the normalised affine matrix
        off = 0
        for b, n in enumerate(groups):
            aff[b, 0, :n] = theta[off:off + n]
            off += n
        return (oracle.att_fuse if mode == ops.FUSE_ATT else oracle.max_fuse)(x, torch.tensor(groups), aff)
    finally:
        oracle.warp_affine_simple = warp


def check(got, x, theta, groups, mode, what, out_hw=None, rows=None):
    """NONE / MAX bit-equal to the float32 oracle; every mode element-wise against float64; ATT within 4x the float32 oracle's error + 1e-7."""
    got = got.detach().cpu().contiguous()
    assert bool(torch.isfinite(got).all()), f"{what}: NaN / Inf in the output"
    hw = tuple(x.shape[2:]) if out_hw is None else tuple(out_hw)
    ref64 = reference(x, theta, groups, mode, hw, torch.float64, rows)
    ref32 = reference(x, theta, groups, mode, hw, torch.float32, rows)
    assert_elementwise(got, ref64, what)
    if mode != ops.FUSE_ATT:
        assert torch.equal(got, ref32), f"{what}: {int((got != ref32).sum())} elements differ from the float32 oracle"
        return ref32
    scale = max(float(ref64.abs().max()), 1e-30)
    err = float((got.double() - ref64).abs().max()) / scale
    err32 = float((ref32.double() - ref64).abs().max()) / scale
    assert err <= 4 * err32 + 1e-7, f"{what}: kernel error {err:.3e} of the scale, float32 oracle {err32:.3e}"
    print(f"ATT-RATIO {what}: kernel {err:.3e} float32-oracle {err32:.3e} ratio {err / max(err32, 1e-30):.3f}")
    return ref32


# ------------------------------------------------------------------------------------------------ poses
def yaw_thetas(n, H, W, seed, yaw=180.0):
    """Ego -> agent thetas of a random frame (make_poses: agents within +-20 m / +-10 m, yaw up to +-``yaw`` degrees) for an H x W map spanning the
    OPV2V range (281.6 m wide), normalised at the map's own pixel size: rotation + translation at unit scale (warp_fuse.hip's rigid case)."""
    poses = make_poses(np.random.RandomState(seed), n, spread_xy=(20.0, 10.0), spread_yaw=yaw)
    pair = torch.from_numpy(get_pairwise_transformation(poses, n))[None]
    return oracle.normalize_pairwise_tfm(pair, H, W, 281.6 / W)[0, 0, :n].contiguous()


def pose_thetas(kind, n, H, W, seed=0):
    """Hand-built poses; agent 0 is the ego.  Shifts are in pixels of the H x W map; quarter turns use exact cos / sin."""
    th = yaw_thetas(n, H, W, seed) if kind in ("out_of_view", "ego_out_of_view") else torch.zeros(n, 2, 3, dtype=torch.float64)
    if kind not in ("out_of_view", "ego_out_of_view"):
        th[:, 0, 0] = 1.0
        th[:, 1, 1] = 1.0

    def turn(i, q):
        c, s = ((1, 0), (0, 1), (-1, 0), (0, -1))[q % 4]
        th[i, 0, 0], th[i, 0, 1], th[i, 1, 0], th[i, 1, 1] = c, -s * H / W, s * W / H, c

    def shift(i, dx, dy):
        th[i, 0, 2], th[i, 1, 2] = 2.0 * dx / W, 2.0 * dy / H

    for i in range(n):
        if kind == "quarter":                          # 0, 90, 180, 270 degrees
            turn(i, i)
        elif kind == "half":                           # every other agent turned around, shifted by whole pixels
            turn(i, 2 * (i % 2))
            shift(i, i % 3, -(i % 2))
        elif kind == "int_shift":                      # taps at exact integers: weight 0 on the far side
            shift(i, (i % 5) - 2, 3 - (i % 7))
        elif kind == "edge_shift":                     # samples exactly on ix = -1, W - 1, W (and iy = -1, H - 1, H)
            shift(i, *((1, -1), (-1, 1), (1, 1), (-1, -1))[i % 4])
    if kind == "out_of_view":                          # the last agent sees none of the ego's area: its warped map is zero
        th[n - 1, 0, 2] = 3.0
    if kind == "ego_out_of_view":                      # half of the ego's own map out of view: X0 = 0, every score 0 there
        th[0, 0, 2] = 1.0
    return th


def sample_positions(theta, H, W, Ho, Wo):
    """float32 sampling positions ix, iy [n, Ho, Wo] exactly as both kernels and the oracle compute them."""
    g = oracle.affine_grid_f64(theta.cpu(), Ho, Wo)
    return (g[..., 0] + 1.0) * (W / 2.0) - 0.5, (g[..., 1] + 1.0) * (H / 2.0) - 0.5


# ------------------------------------------------------------------------------------------------ which NCHW route runs
def patch_fit(theta, H, W, Ho, Wo):
    """warp_fuse.hip phase 0 in host arithmetic: per agent and 8 x 8 output tile, does the tile's tap footprint fit the 16 x 16 LDS patch
    (nc4 <= 4 float4 columns from a 4-aligned origin, <= 16 rows)?  -> bool [n, tiles] (True where the agent is not live in the tile)."""
    ix, iy = sample_positions(theta, H, W, Ho, Wo)
    live = (ix > -1) & (ix < W) & (iy > -1) & (iy < H)
    x0, y0 = torch.floor(ix).long(), torch.floor(iy).long()
    ty, tx = (Ho + 7) // 8, (Wo + 7) // 8
    big = 1 << 28

    def tiles(v, fill):
        p = torch.full((v.shape[0], ty * 8, tx * 8), fill, dtype=torch.long)
        p[:, :Ho, :Wo] = torch.where(live, v, torch.full_like(v, fill))
        return p.view(-1, ty, 8, tx, 8).permute(0, 1, 3, 2, 4).reshape(v.shape[0], ty * tx, 64)

    xmin, xmax = tiles(x0, big).amin(-1), tiles(x0 + 1, -big).amax(-1)
    ymin, ymax = tiles(y0, big).amin(-1), tiles(y0 + 1, -big).amax(-1)
    ax0 = torch.div(xmin, 4, rounding_mode="floor") * 4
    fit = (torch.div(xmax - ax0, 4, rounding_mode="floor") + 1 <= 4) & (ymax - ymin + 1 <= 16)
    return fit | (xmin == big)


def nchw_route(x, theta, Ho, Wo):
    """'patch' when every tile takes the LDS-patch route, 'direct' when none does, 'mixed' otherwise (warp_fuse.hip :171-174, :512)."""
    H, W = x.shape[2:]
    vec_ok = W % 4 == 0 and x.data_ptr() % 16 == 0
    fast = patch_fit(theta, H, W, Ho, Wo).all(0) & vec_ok
    return "patch" if bool(fast.all()) else "direct" if not bool(fast.any()) else "mixed"


def nchw_variant(n, C):
    """Phase-1 variant of the patch route for one frame of n agents (dispatch<NA>): straight-line (:223), masked (:253), two-pass (:307)."""
    NA = n if n <= 3 else 5 if n <= 5 else 8
    cpt = 8 if C <= 128 else 16
    if NA == 8 and cpt == 16:
        return "two-pass"
    if n != NA:
        return "masked"
    return "straight" if C % cpt == 0 else "straight+masked"       # a partial last channel group takes the masked variant


def unaligned(x):
    """A copy of x on the device whose base is 4 bytes past a 16-byte boundary."""
    buf = torch.empty(x.numel() + 4, device=DEV)
    v = buf[1:1 + x.numel()].view(x.shape)
    v.copy_(x)
    assert v.data_ptr() % 16 == 4
    return v


def stale_nan_lds(n, C):
    """Leave NaN in the LDS patch slabs of the NCHW kernel (a launch of the same n and C: the same workgroup size and LDS layout, on an all-NaN map
    with a tile on every CU), as any earlier launch may leave any bits there.  A launch after it must read only slab positions it staged itself:
    an agent with no live pixel in a tile still multiplies its (weight 0) taps with what the slab holds."""
    ops.warp_fuse(torch.full((n, C, 64, 256), float("nan"), device=DEV), torch.tensor([[1.0, 0, 0], [0, 1, 0]], dtype=torch.float64, device=DEV).repeat(n, 1, 1),
                  [n], ops.FUSE_NONE)


def nchw_inputs(route, n, C, H, W, x, theta, zoom_agent):
    """(device map, theta) that force ``route``; asserts the route the kernel's predicates choose."""
    if route == "zoom":                                # one agent at scale 2.5: its 8 x 8-tile footprint spans 20 source pixels
        theta = theta.clone()
        theta[zoom_agent, :, :2] *= 2.5
    xd = unaligned(x) if route == "unaligned" else x.to(DEV)
    if route == "patch":
        got = nchw_route(xd, theta, H, W)
        assert got == "patch", got
    elif route in ("direct", "unaligned"):
        assert (W % 4 != 0 if route == "direct" else xd.data_ptr() % 16 != 0) and nchw_route(xd, theta, H, W) == "direct"
    else:
        fit = patch_fit(theta, H, W, H, W)
        others = [i for i in range(n) if i != zoom_agent]
        assert not bool(fit[zoom_agent].all()) and bool(fit[others].all()), "the zoomed agent alone leaves the patch"
        assert nchw_route(xd, theta, H, W) != "patch"
    return xd, theta.to(DEV)


# ------------------------------------------------------------------------------------------------ NCHW kernel
@pytest.mark.parametrize("C", [20, 64, 72, 100, 128, 200, 256])
@pytest.mark.parametrize("n", range(1, 9))
def test_warp_fuse_every_agent_count_and_route(n, C):
    """Every agent count at channel widths on both sides of the 8 / 16 channels-per-thread split, with partial channel groups (C = 20, 100, 200;
    C = 72 fills nine whole groups of 8: the 1024-thread launch with an odd wave count), random yaw up to 180 degrees, each mode on each route:
    the LDS patch (W % 4 == 0), the direct fallback (W % 4 != 0; a map 4 bytes off 16-byte alignment; one agent zoomed 2.5x beyond the patch).
    Each launch follows one that leaves NaN in the LDS slabs (``stale_nan_lds``): at n = 1 the zoomed ego is live in no pixel of the outer tiles,
    which take the patch route, and used to return NaN / -inf there."""
    gen = torch.Generator().manual_seed(1000 * n + C)
    H = 20
    variant = nchw_variant(n, C)
    for route, W in (("patch", 44), ("direct", 42), ("unaligned", 44), ("zoom", 44)):
        x = torch.randn(n, C, H, W, generator=gen)
        theta = yaw_thetas(n, H, W, seed=n * 31 + C + W)
        xd, th = nchw_inputs(route, n, C, H, W, x, theta, zoom_agent=n - 1)
        for name, mode in MODES:
            stale_nan_lds(n, C)
            check(ops.warp_fuse(xd, th, [n], mode), x, th, [n], mode, f"nchw n={n} C={C} {route}/{variant} {name}")


@pytest.mark.parametrize("permuted", [False, True], ids=["rows-identity", "rows-permuted"])
@pytest.mark.parametrize("groups", [[4, 1, 7], [8, 6], [6, 4, 7]])
@pytest.mark.parametrize("C", [64, 200])
def test_warp_fuse_mixed_batches(C, groups, permuted):
    """Frames of different agent counts in one call (per-frame x / theta / output offsets, a different NA per frame), with and without a row table
    (agents stored in another order inside every frame: the agent-sharded caller)."""
    gen = torch.Generator().manual_seed(C + sum(groups) * 10 + permuted)
    H, W = 20, 44
    total = sum(groups)
    x = torch.randn(total, C, H, W, generator=gen)
    theta = torch.cat([yaw_thetas(n, H, W, seed=b * 7 + n) for b, n in enumerate(groups)])
    rows = None
    if permuted:
        rows = sum((torch.randperm(n, generator=gen).tolist() for n in groups), [])
    xd, th = x.to(DEV), theta.to(DEV)
    for name, mode in MODES:
        got = ops.warp_fuse(xd, th, groups, mode, rows=rows)
        check(got, x, th, groups, mode, f"nchw groups={groups} C={C} rows={rows} {name}", rows=rows)


POSES = ["identity", "quarter", "half", "int_shift", "edge_shift", "out_of_view", "ego_out_of_view"]


@pytest.mark.parametrize("n", [1, 4, 6, 7, 8])
@pytest.mark.parametrize("kind", POSES)
def test_poses_both_kernels(kind, n):
    """Identity, exact quarter and half turns, whole-pixel shifts (taps on integers), shifts that put samples exactly on ix = -1, W - 1, W, an agent
    entirely out of view and an ego half out of its own view -- on the NCHW patch and direct routes and on the channels-last kernel (three scales)."""
    H, W = 16, 32
    th = pose_thetas(kind, n, H, W, seed=n)
    ix, iy = sample_positions(th, H, W, H, W)
    if kind in ("identity", "int_shift"):
        assert torch.equal(ix, ix.floor()) and torch.equal(iy, iy.floor())
    if kind == "edge_shift" and n >= 2:
        assert {-1.0, W - 1.0, float(W)} <= set(ix.unique().tolist()) and {-1.0, H - 1.0, float(H)} <= set(iy.unique().tolist())
    gen = torch.Generator().manual_seed(len(kind) * 10 + n)
    thd = th.to(DEV)
    for C in (64, 200):
        x = torch.randn(n, C, H, W, generator=gen)
        for route, xd in (("patch", x.to(DEV)), ("unaligned", unaligned(x))):
            assert nchw_route(xd, th, H, W) == ("patch" if route == "patch" else "direct")
            for name, mode in MODES:
                stale_nan_lds(n, C)
                got = ops.warp_fuse(xd, thd, [n], mode)
                check(got, x, thd, [n], mode, f"nchw pose={kind} n={n} C={C} {route} {name}")
                if mode == ops.FUSE_NONE and kind == "out_of_view":
                    assert float(got[n - 1].abs().max()) == 0.0
    xs = [torch.randn(n, C, H // d, W // d, generator=gen) for C, d in ((64, 1), (128, 2), (256, 4))]
    xd = [x.to(DEV).contiguous(memory_format=torch.channels_last) for x in xs]
    for name, mode in MODES:
        outs = ops.warp_fuse_nhwc(xd, thd, mode)
        for x, got in zip(xs, outs):
            check(got, x, thd, [n], mode, f"nhwc pose={kind} n={n} C={x.shape[1]} {name}")


def values(kind, shape, gen):
    if kind == "negative":                             # every warped value in view is negative: MAX < 0, ATT scores > 0
        return -(torch.rand(shape, generator=gen) + 0.5)
    if kind == "small":                                # scores ~ 1e-3: a padded slot with exp(0 - smax) would weigh ~1
        return torch.randn(shape, generator=gen) * 0.01
    mag = torch.rand(shape, generator=gen) * 70 + 30   # "huge": |x| in [30, 100]
    return torch.where(torch.rand(shape, generator=gen) < 0.5, -mag, mag)


@pytest.mark.parametrize("n", [4, 6, 7])
@pytest.mark.parametrize("kind", ["negative", "small", "huge"])
def test_padded_slots_and_softmax_range(kind, n):
    """The masked slots of NA = 5 / 8 (n = 4, 6, 7): all-negative maps (a MAX started from 0 returns 0; a padded slot in the ATT sum pulls every
    output toward 0), small maps (scores near 0), |x| in [30, 100] at C = 256 (raw scores far above float32 exp's range).  Small rotations and
    shifts keep nearly every pixel in view of every agent."""
    gen = torch.Generator().manual_seed(n * 3 + len(kind))
    H, W = 20, 44
    th = yaw_thetas(n, H, W, seed=n + 100, yaw=10.0)
    thd = th.to(DEV)
    widths = (256,) if kind == "huge" else (64, 200, 256)
    for C in widths:
        x = values(kind, (n, C, H, W), gen)
        if kind == "huge":
            assert float((x[0] * x[0]).sum(0).max()) / C ** 0.5 > 10 * EXP_MAX
        for route, xd in (("patch", x.to(DEV)), ("unaligned", unaligned(x))):
            assert nchw_route(xd, th, H, W) == ("patch" if route == "patch" else "direct")
            for name, mode in MODES:
                ref = check(ops.warp_fuse(xd, thd, [n], mode), x, thd, [n], mode, f"nchw {kind} n={n} C={C} {route}/{nchw_variant(n, C)} {name}")
                if kind == "negative" and mode == ops.FUSE_MAX:
                    assert float((ref < 0).float().mean()) > 0.5
    xs = [values(kind, (n, C, h, w), gen) for C, h, w in ((256, 6, 11),) + (() if kind == "huge" else ((64, 20, 44), (128, 10, 22)))]
    xd = [x.to(DEV).contiguous(memory_format=torch.channels_last) for x in xs]
    for name, mode in MODES:
        for x, got in zip(xs, ops.warp_fuse_nhwc(xd, thd, mode)):
            check(got, x, thd, [n], mode, f"nhwc {kind} n={n} C={x.shape[1]} {name}")


def test_fullsize_opv2v_frame_of_four():
    """The everyday OPV2V frame the benchmark never runs: 4 agents (NA = 5, one masked slot) at the three full feature-map sizes, both kernels."""
    h = builtin_config("opv2v_coalign")
    fr = make_frame(h, 4, pillars_per_agent=10, seed=44, spread_yaw=180.0)
    theta = oracle.normalize_pairwise_tfm(fr["pairwise_t_matrix"], 200, 704, 0.4)[0, 0, :4].contiguous()
    thd = theta.to(DEV)
    gen = torch.Generator().manual_seed(4)
    xs = [torch.randn(4, C, H, W, generator=gen) for C, H, W in ((64, 100, 352), (128, 50, 176), (256, 25, 88))]
    for x in xs:
        xd = x.to(DEV)
        assert nchw_route(xd, theta, *x.shape[2:]) == "patch"
        for name, mode in MODES:
            check(ops.warp_fuse(xd, thd, [4], mode), x, thd, [4], mode, f"nchw full-size n=4 C={x.shape[1]} {name}")
    xd = [x.to(DEV).contiguous(memory_format=torch.channels_last) for x in xs]
    for name, mode in MODES:
        for x, got in zip(xs, ops.warp_fuse_nhwc(xd, thd, mode)):
            check(got, x, thd, [4], mode, f"nhwc full-size n=4 C={x.shape[1]} {name}")


# ------------------------------------------------------------------------------------------------ channels-last kernel
# (C, H, W): W not a multiple of the 512 / C pixels a wave covers (8, 4, 2), H not a multiple of the 4 rows of a workgroup
NHWC_SCALES = {64: (18, 45), 128: (9, 23), 256: (5, 11)}
NHWC_OUT = {64: (13, 37), 128: (7, 19), 256: (3, 5)}


@pytest.mark.parametrize("n", range(1, 9))
def test_warp_fuse_nhwc_every_agent_count(n):
    """One to three scales in one launch, given in ascending and descending channel order (the host sorts them by C), a row table (permuted at
    every n > 1), partial edge tiles, and out_hw != (H, W) for the warp."""
    gen = torch.Generator().manual_seed(500 + n)
    th = yaw_thetas(n, 18, 45, seed=n + 7)
    thd = th.to(DEV)
    perm = torch.randperm(n, generator=gen).tolist()
    for chans in ((64,), (256, 128), (64, 128, 256), (256, 128, 64), (128, 64)):
        xs = [torch.randn(n, C, *NHWC_SCALES[C], generator=gen) for C in chans]
        for rows in (None, perm):
            xd = [x.to(DEV).contiguous(memory_format=torch.channels_last) for x in xs]
            for name, mode in MODES:
                outs = ops.warp_fuse_nhwc(xd, thd, mode, rows=rows)
                for x, got in zip(xs, outs):
                    assert ops.is_channels_last(got) or got.shape[0] * got.shape[2] * got.shape[3] == 1
                    check(got, x, thd, [n], mode, f"nhwc n={n} scales={chans} C={x.shape[1]} rows={rows} {name}", rows=rows)
        hw = [NHWC_OUT[C] for C in chans]
        outs = ops.warp_fuse_nhwc(xd, thd, ops.FUSE_NONE, rows=perm, out_hw=hw)
        for x, got, o in zip(xs, outs, hw):
            check(got, x, thd, [n], ops.FUSE_NONE, f"nhwc n={n} scales={chans} C={x.shape[1]} out_hw={o}", out_hw=o, rows=perm)


def test_fuse_multiscale_ragged_frames_with_row_table():
    """fusion.fuse_multiscale with record_len [4, 2, 5] and an agent row table (the agent-sharded caller), three channels-last scales, against the
    oracle frame by frame; and the maps it must refuse (returns None, the caller falls back to coalign_warp_fuse).  (11 agents in all: it used to
    refuse every batch of more than 8 agents, applying the per-frame limit to the whole batch.)"""
    groups = [4, 2, 5]
    gen = torch.Generator().manual_seed(425)
    L = max(groups)
    aff = torch.zeros(len(groups), L, L, 2, 3, dtype=torch.float64)
    for b, n in enumerate(groups):
        aff[b, 0, :n] = yaw_thetas(n, 18, 45, seed=b + 50)
    rows = sum((torch.randperm(n, generator=gen).tolist() for n in groups), [])
    xs = [torch.randn(sum(groups), C, *NHWC_SCALES[C], generator=gen) for C in (64, 128, 256)]
    xd = [x.to(DEV).contiguous(memory_format=torch.channels_last) for x in xs]
    theta = torch.cat([aff[b, 0, :n] for b, n in enumerate(groups)])
    for name, mode in MODES:
        outs = fusion.fuse_multiscale(xd, torch.tensor(groups), aff.to(DEV), mode, rows=rows)
        assert outs is not None and len(outs) == 3
        for x, got in zip(xs, outs):
            check(got, x, theta, groups, mode, f"fuse_multiscale {groups} C={x.shape[1]} {name}", rows=rows)
    a = aff.to(DEV)
    assert fusion.fuse_multiscale([xd[0].contiguous()], groups, a, ops.FUSE_ATT) is None                          # NCHW memory
    assert fusion.fuse_multiscale([torch.randn(11, 96, 8, 8, device=DEV).contiguous(memory_format=torch.channels_last)], groups, a, ops.FUSE_ATT) is None
    assert fusion.fuse_multiscale([xd[0][:9]], [9], a, ops.FUSE_ATT) is None                                     # a group of 9
    assert fusion.fuse_multiscale(xd + xd[:1], groups, a, ops.FUSE_ATT) is None                                  # 4 scales
    assert fusion.fuse_multiscale(xd, [4, 2, 4], a, ops.FUSE_ATT) is None                                        # record_len does not cover x
    assert fusion.fuse_multiscale([xd[0], xd[1][:10]], groups, a, ops.FUSE_ATT) is None                          # scales with different agent counts


# ------------------------------------------------------------------------------------------------ drop-in API
@pytest.mark.parametrize("n", [9, 17])
def test_warp_affine_simple_chunks_of_eight(n):
    """fusion.warp_affine_simple splits n > 8 agents into launches of <= 8 (chunks [8, 1] and [8, 8, 1]); every agent has its own map and pose, so a
    wrong per-chunk offset shows.  dsize != (H, W)."""
    assert fusion._chunks(n) == {9: [8, 1], 17: [8, 8, 1]}[n]
    gen = torch.Generator().manual_seed(n)
    H, W = 20, 44
    x = torch.randn(n, 64, H, W, generator=gen)
    th = yaw_thetas(n, H, W, seed=n)
    for dsize in ((20, 44), (13, 30)):
        got = fusion.warp_affine_simple(x.to(DEV), th.to(DEV), dsize)
        check(got, x, th, [n], ops.FUSE_NONE, f"warp_affine_simple n={n} dsize={dsize}", out_hw=dsize)
