"""The SplitMap kernels at their limits against float64, and the layers' routes at the edges of their predicates (all through the C ABI).

Kernel level: ``coalign_conv3x3_sp`` / ``_sp_s2`` (+ the fused skip) at Cout up to their LDS limits (1024; 512 for the skip), every tile geometry, with output
channels on scales 2^-20 ... 2^6 (a scale word read for the wrong channel shows), compared with float64 PER OUTPUT CHANNEL, relative to that channel's own scale.
The float64 reference convolves the 22-bit values the kernel reads (``SplitMap.dense()``) with the unrounded weights.  A SplitMap output holds values below
2^-13 only to an absolute 2^-33 (csrc/common.h): it is held to the same launch's float32 output instead (``assert_split_map_holds``).

Module level: BasicBlock / ResNetStages / DoubleConv / the merged heads built on both sides of every route predicate, float32 forward against the module's own
float64 forward (the reference's op sequence), with the kernels that ran recorded.
"""
import copy

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from coalign_amd import backbone as bb
from coalign_amd import detector, ops
from coalign_amd.config import builtin_config
from coalign_amd.routes import NARROW, SP, plan
from coalign_amd.synthetic import fill_parameters_, make_frame
from conftest import assert_elementwise
from sp_helpers import assert_split_map_holds, sparse_canvas

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BOUND = 3e-6                     # of the channel's own scale: the bound of test_fp16_split_scale_free_with_mixed_channel_scales_and_strided_layers
SP_ABS = 2.0 ** -33              # what a SplitMap holds of a value below 2^-13
ZERO_CH = 3                      # the all-zero output channel of every mixed-scale layer


def mixed_scales(g, n, lo, hi):
    """n channel scales 2^lo ... 2^hi, randomly permuted."""
    return (2.0 ** torch.linspace(lo, hi, n, device=DEV, dtype=torch.float64)).float()[torch.randperm(n, generator=g, device=DEV)]


def mixed_layer(g, Co, Ci, k=3, lo=-20, hi=6):
    """Weights whose output channels sit on the scales of ``mixed_scales`` (one of them all zero) and a bias on the same per-channel scale."""
    cs = mixed_scales(g, Co, lo, hi)
    w = torch.randn((Co, Ci, k, k), generator=g, device=DEV) / (k * k * Ci) ** 0.5 * cs.view(-1, 1, 1, 1)
    w[ZERO_CH] = 0
    b = torch.randn(Co, generator=g, device=DEV) * cs
    return w, b, cs


def channel_error(got, ref, pre=None):
    """max over channels of max |got - ref| / the channel's scale: max |pre-activation| in that channel (``pre``; ``ref`` itself when there is no activation).
    (After a ReLU the largest surviving value of a channel whose bias pushes most outputs below zero says nothing about the size of its sums.)"""
    scale = (ref if pre is None else pre).abs().amax(dim=(0, 2, 3))
    err = (got.double() - ref).abs().amax(dim=(0, 2, 3))
    return float(torch.where(scale > 0, err / scale.clamp_min(1e-300), err).max())


def assert_channels_close(got, ref, what, abs_floor=0.0, pre=None):
    """Every output channel within BOUND of its own scale (+ ``abs_floor``), as an element-wise bound."""
    scale = (ref if pre is None else pre).abs().amax(dim=(0, 2, 3), keepdim=True)
    bad = (got.double() - ref).abs() > BOUND * scale + abs_floor
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} elements outside {BOUND:g} of their channel's scale; worst {channel_error(got, ref, pre):.3e}"
    return channel_error(got, ref, pre)


# (N, Cin, Cout, H, W, geometry, residual, output, relu): geometry 0 = the product's choice, 100000 + g = whole tiles of g, 200000 + g = g with its tiles cut
SP_CASES = [
    (2, 16, 64, 9, 37, 0, "none", "nhwc", True),
    (1, 48, 512, 12, 40, 100081, "sp", "sp", False),
    (2, 256, 1024, 8, 24, 100121, "nhwc", "both", True),
    (1, 512, 1024, 16, 20, 100124, "none", "nhwc", False),
    (2, 16, 1024, 10, 50, 100148, "sp", "both", False),
    (1, 48, 64, 17, 70, 100326, "nhwc", "sp", True),
    (2, 256, 1024, 9, 60, 100326, "none", "both", False),
    (1, 256, 512, 20, 64, 200081, "sp", "nhwc", False),
    (2, 48, 1024, 12, 40, 200148, "nhwc", "nhwc", True),
    (1, 128, 1024, 25, 88, 0, "sp", "sp", False),
]


def _conv64_linear(x, w, b, r, stride=1):
    """The pre-activation of conv64 (tests/test_round5_gpu.py) in float64: conv3x3(x, w, stride, pad 1) + b (+ r)."""
    N, Ci, H, W = x.shape
    xp = F.pad(x.double(), (1, 1, 1, 1))
    Ho, Wo = (H + stride - 1) // stride, (W + stride - 1) // stride
    out = torch.zeros((N, w.shape[0], Ho, Wo), dtype=torch.float64, device=x.device)
    for dy in range(3):
        for dx in range(3):
            out += torch.einsum("oc,nchw->nohw", w.double()[:, :, dy, dx], xp[:, :, dy:dy + stride * Ho:stride, dx:dx + stride * Wo:stride])
    out += b.double().view(1, -1, 1, 1)
    return out if r is None else out + r.double()


def _sp_case(case):
    N, Ci, Co, H, W, geo, res, out, relu = case
    g = torch.Generator(device=DEV).manual_seed(N + Ci + Co + H + W + geo % 1000)
    xs = ops.SplitMap.pack(torch.randn((N, Ci, H, W), generator=g, device=DEV))
    w, b, cs = mixed_layer(g, Co, Ci)
    rs = ops.SplitMap.pack(torch.randn((N, Co, H, W), generator=g, device=DEV) * cs.view(1, -1, 1, 1))
    r = None if res == "none" else rs.dense()              # (what the pairs hold)
    res_arg = {"none": None, "sp": rs, "nhwc": None if r is None else r.contiguous(memory_format=torch.channels_last)}[res]
    pre = _conv64_linear(xs.dense(), w, b, r)
    return xs, w, b, res_arg, torch.relu(pre) if relu else pre, pre, r


@pytest.mark.parametrize("case", SP_CASES, ids=lambda c: f"{c[0]}x{c[1]}to{c[2]}@{c[3]}x{c[4]}-g{c[5]}-res_{c[6]}-out_{c[7]}-{'relu' if c[8] else 'linear'}")
def test_conv3x3_sp_mixed_channel_scales_against_float64(case):
    """Every output channel of ``coalign_conv3x3_sp`` within 3e-6 of its own scale of the float64 convolution, at Cout 64 ... 1024, Cin 16 ... 512, every
    geometry (whole tiles and a forced stream-K cut), residual none / SplitMap / channels-last, outputs SplitMap / channels-last / both; the all-zero channel is
    exactly act(bias (+ residual))."""
    N, Ci, Co, H, W, geo, res, out, relu = case
    xs, w, b, res_arg, ref, pre, r = _sp_case(case)
    w16 = ops.pack_conv3x3_emu_weight(w, 16, True)
    cl = ops.conv3x3_sp(xs, w16, b, Co, res_arg, relu, out_split=False, geometry=geo)
    err = assert_channels_close(cl, ref, case, pre=pre)
    zero = b[ZERO_CH].view(1, 1, 1).expand(N, H, W) + (0 if r is None else r[:, ZERO_CH])
    assert torch.equal(cl[:, ZERO_CH], torch.relu(zero) if relu else zero), case
    if not relu:
        assert float(cl.min()) < 0                                  # (negative outputs are compared too)
    if out == "sp":
        assert_split_map_holds(ops.conv3x3_sp(xs, w16, b, Co, res_arg, relu, out_split=True, geometry=geo), cl, case)
    elif out == "both":
        y, ysp = ops.conv3x3_sp(xs, w16, b, Co, res_arg, relu, geometry=geo, out_both=True)
        assert torch.equal(y, cl), case
        assert_split_map_holds(ysp, cl, case)
    assert not ops.sp_range_exceeded(DEV)
    print(f"\nconv3x3_sp {case}: worst channel error {err:.2e} of the channel scale (bound {BOUND:g})")


def _round11(x):
    """x rounded to 11 significant bits (the high fp16 term of the pair; low term dropped), scale free."""
    return ((x.contiguous().view(torch.int32) + (1 << 12)) & -(1 << 13)).view(torch.float32)


def test_the_channel_bound_separates_the_split_from_a_kernel_that_drops_the_low_term():
    """The per-channel bound can fail: the float64 convolution of the operands rounded to 11 bits -- a kernel that kept only the high fp16 term -- is
    refused, at the shape where the kernel itself passes."""
    case = SP_CASES[1]
    N, Ci, Co, H, W, geo, res, out, relu = case
    xs, w, b, res_arg, ref, pre, r = _sp_case(case)
    lossy = _conv64_linear(_round11(xs.dense()), _round11(w), b, r).float()
    with pytest.raises(AssertionError):
        assert_channels_close(lossy, ref, "11-bit operands", pre=pre)
    print(f"\n11-bit operands: worst channel error {channel_error(lossy, ref):.2e} of the channel scale (bound {BOUND:g})")
    assert_channels_close(ops.conv3x3_sp(xs, ops.pack_conv3x3_emu_weight(w, 16, True), b, Co, res_arg, relu, out_split=False, geometry=geo), ref, case, pre=pre)


def _s2_ref(x, w, b, relu):
    """-> (float64 stride-2 output, its pre-activation)."""
    pre = _conv64_linear(x, w, b, None, stride=2)
    return (torch.relu(pre) if relu else pre), pre


# (N, Cin, Cout, H, W, skip, relu): the strided kernel without the skip up to Cout 1024, with the fused skip at its 512 limit; odd and one-pixel maps
S2_CASES = [(2, 64, 1024, 3, 131, False, True), (8, 32, 1024, 1, 1, False, False), (3, 16, 1024, 131, 3, False, False), (1, 64, 512, 131, 3, True, False),
            (2, 48, 512, 3, 1, True, True)]


@pytest.mark.parametrize("case", S2_CASES, ids=lambda c: f"{c[0]}x{c[1]}to{c[2]}@{c[3]}x{c[4]}-{'skip' if c[5] else 'noskip'}-{'relu' if c[6] else 'linear'}")
def test_conv3x3_sp_s2_mixed_channel_scales_against_float64(case):
    """``coalign_conv3x3_sp_s2`` (+ the skip as a tenth tap) with output channels on 2^-12 ... 2^6 (the skip's channels too): the SplitMap's values within
    3e-6 of the channel scale + 2^-33 of the float64 stride-2 convolution, the skip map within 3e-6 of its channel scale of a float64 1 x 1 / stride-2 one."""
    N, Ci, Co, H, W, skip, relu = case
    g = torch.Generator(device=DEV).manual_seed(sum(case[:5]))
    xs = ops.SplitMap.pack(torch.randn((N, Ci, H, W), generator=g, device=DEV))
    w, b, _ = mixed_layer(g, Co, Ci, lo=-12, hi=6)
    img = ops.pack_conv3x3_emu_weight(w, 16, True)
    ref, pre = _s2_ref(xs.dense(), w, b, relu)
    if skip:
        wd, _, _ = mixed_layer(g, Co, Ci, k=1, lo=-12, hi=6)
        y, sk = ops.conv3x3_sp_s2(xs, img, b, Co, relu, w_skip=ops.pack_conv1x1_sp_weight(wd))
        sref = torch.einsum("oc,nchw->nohw", wd[:, :, 0, 0].double(), xs.dense().double()[:, :, ::2, ::2])
        es = assert_channels_close(sk, sref, (case, "skip"))
        assert float(sk[:, ZERO_CH].abs().max()) == 0
        print(f"\nconv3x3_sp_s2 skip {case}: worst channel error {es:.2e}")
    else:
        y = ops.conv3x3_sp_s2(xs, img, b, Co, relu)
    e = assert_channels_close(y.dense(), ref, case, abs_floor=SP_ABS, pre=pre)
    assert not ops.sp_range_exceeded(DEV)
    print(f"\nconv3x3_sp_s2 {case}: worst channel error {e:.2e} of the channel scale (bound {BOUND:g} + 2^-33)")


def test_conv3x3_sp_s2_on_the_sparse_canvas_mixed_channel_scales_and_fused_skip_at_512():
    """The sparse-canvas form of the strided kernel, fused skip at Cout 512, both on mixed channel scales, against float64 of the canvas's 22-bit values."""
    sc = sparse_canvas(2, 200, 704, 3000, 21)
    g = torch.Generator(device=DEV).manual_seed(21)
    w, b, _ = mixed_layer(g, 512, 64, lo=-12, hi=6)
    wd, _, _ = mixed_layer(g, 512, 64, k=1, lo=-12, hi=6)
    x = ops.SplitMap.pack(sc.dense()).dense()
    for relu in (True, False):
        y, sk = ops.conv3x3_sp_s2(sc, ops.pack_conv3x3_emu_weight(w, 16, True), b, 512, relu, w_skip=ops.pack_conv1x1_sp_weight(wd))
        ref, pre = _s2_ref(x, w, b, relu)
        e = assert_channels_close(y.dense(), ref, ("sparse", relu), abs_floor=SP_ABS, pre=pre)
        es = assert_channels_close(sk, torch.einsum("oc,nchw->nohw", wd[:, :, 0, 0].double(), x.double()[:, :, ::2, ::2]), ("sparse skip", relu))
        print(f"\nconv3x3_sp_s2 sparse canvas relu={relu}: worst channel error {e:.2e}, skip {es:.2e}")
    assert not ops.sp_range_exceeded(DEV)


# ------------------------------------------------------------------------------------------------ modules at the edges of their route predicates
class _Spy:
    """Records which kernel served which layer during one forward; ``more``: further ``ops`` names, recorded as (name, output channels or None, None)."""

    def __init__(self, monkeypatch, more=()):
        self.calls, self.more = [], tuple(more)
        for name in ("conv3x3_sp", "conv3x3_sp_s2", "heads_sp") + self.more:
            monkeypatch.setattr(ops, name, self._wrap(name, getattr(ops, name)))
        monkeypatch.setattr(F, "conv2d", self._wrap("F.conv2d", F.conv2d))

    def _wrap(self, name, fn):
        def spy(*args, **kwargs):
            if name == "F.conv2d":
                self.calls.append((name, tuple(args[1].shape[:2]), None))
            elif name in self.more:
                self.calls.append((name, args[3] if len(args) > 3 and isinstance(args[3], int) else None, None))
            elif name == "heads_sp":
                self.calls.append((name, args[0].shape[1], args[3]))
            else:
                self.calls.append((name, (args[3], args[0].shape[1]), kwargs.get("w_skip") is not None if name == "conv3x3_sp_s2" else None))
            return fn(*args, **kwargs)
        return spy

    def of(self, name):
        return [c for c in self.calls if c[0] == name]


def _block(cin, cout, stride):
    down = nn.Sequential(nn.Conv2d(cin, cout, 1, stride=stride, bias=False), nn.BatchNorm2d(cout)) if stride != 1 or cin != cout else None
    return bb.BasicBlock(cin, cout, stride, down)


def _run(module, x, monkeypatch, what):
    """float32 CUDA forward under the default flags against the module's float64 forward; -> the spy of the float32 forward."""
    fill_parameters_(module, seed=len(what))
    module = module.to(DEV).eval()
    with torch.no_grad():
        ref = copy.deepcopy(module).double()(x.double())
        spy = _Spy(monkeypatch)
        got = module(x)
    ref, got = (ref[-1], got[-1]) if isinstance(ref, list) else (ref, got)
    e = assert_elementwise(got, ref, what)
    print(f"\n{what}: {e:.2e} of the scale against float64; kernels {sorted(set(c[0] for c in spy.calls))}")
    return spy


# (Cin, Cout, stride, H, W): both sides of BasicBlock.takes_split_maps (Cout 1024 / 1088, Cin 24 / 32) and of the fused skip (Cout 512 / 576)
BLOCKS = [(1024, 1024, 1, 6, 20), (1088, 1088, 1, 6, 20), (256, 1024, 2, 9, 31), (256, 1088, 2, 9, 31), (24, 64, 2, 17, 40), (32, 64, 2, 17, 40),
          (256, 512, 2, 9, 31), (256, 576, 2, 9, 31)]


@pytest.mark.parametrize("cin,cout,stride,H,W", BLOCKS)
def test_basic_block_route_at_its_limits_against_float64(cin, cout, stride, H, W, monkeypatch):
    blk = _block(cin, cout, stride)
    x = torch.relu(torch.randn((2, cin, H, W), generator=torch.Generator(device=DEV).manual_seed(cin + cout), device=DEV))
    on_split = blk.eval().takes_split_maps()
    assert on_split == (bb.sp_channels_ok(None if stride == 2 else cin, cout) and (stride == 1 or (cin % 16 == 0 and cin <= 256)))
    spy = _run(blk, x, monkeypatch, f"BasicBlock {cin}->{cout} stride {stride}")
    if not on_split:
        assert spy.of("conv3x3_sp") == [] and spy.of("conv3x3_sp_s2") == []
        return
    assert spy.of("F.conv2d") == []                                          # a SplitMap layer never reaches the library
    assert [c[1] for c in spy.of("conv3x3_sp")] == ([(cout, cin), (cout, cout)] if stride == 1 else [(cout, cout)])
    if stride == 2:
        assert [c[1:] for c in spy.of("conv3x3_sp_s2")] == [((cout, cin), bb.sp_channels_ok(cin, cout, skip=True))]     # the skip rides along up to 512 channels


def test_resnet_stages_on_the_split_map_route_against_float64(monkeypatch):
    st = bb.ResNetStages([2, 2], [2, 2], [64, 128], inplanes=64)
    x = torch.relu(torch.randn((2, 64, 34, 70), generator=torch.Generator(device=DEV).manual_seed(2), device=DEV))
    spy = _run(st, x, monkeypatch, "ResNetStages 64 -> [64, 128]")
    assert spy.of("F.conv2d") == []
    assert len(spy.of("conv3x3_sp_s2")) == 2 and len(spy.of("conv3x3_sp")) == 6


@pytest.mark.parametrize("cout", [1024, 1088])
@pytest.mark.parametrize("split_in", [False, True])
def test_double_conv_route_at_its_limit_against_float64(cout, split_in, monkeypatch):
    """Both DoubleConv routes (SplitMap input from the heads, float32 input): 1024 channels on ``conv3x3_sp``, 1088 back on the consumer-split kernel."""
    dc = bb.DoubleConv(128, cout, 3, 1, 1)
    x = torch.relu(torch.randn((1, 128, 10, 36), generator=torch.Generator(device=DEV).manual_seed(cout), device=DEV))
    fill_parameters_(dc, seed=cout)
    dc = dc.to(DEV).eval()
    with torch.no_grad():
        ref = copy.deepcopy(dc).double()(ops.SplitMap.pack(x).dense().double() if split_in else x.double())
        spy = _Spy(monkeypatch)
        got = dc(ops.SplitMap.pack(x) if split_in else x)
    e = assert_elementwise(got, ref, f"DoubleConv 128 -> {cout}, SplitMap in: {split_in}")
    print(f"\nDoubleConv 128 -> {cout} SplitMap in {split_in}: {e:.2e}; kernels {sorted(set(c[0] for c in spy.calls))}")
    assert dc.takes_split_maps() == (cout <= 1024)
    if cout <= 1024:
        assert spy.of("F.conv2d") == [] and [c[1] for c in spy.of("conv3x3_sp")] == ([(cout, 128)] if split_in else []) + [(cout, cout)]
    else:
        assert spy.of("conv3x3_sp") == []


def test_shrink_header_over_the_limit_falls_back_layer_by_layer(monkeypatch):
    """DownsampleConv [1024, 1088] fed a SplitMap: the first layer stays on ``conv3x3_sp``, the second falls back; no layer raises."""
    ds = bb.DownsampleConv({"input_dim": 128, "dim": [1024, 1088], "kernal_size": [3, 3], "stride": [1, 1], "padding": [1, 1]})
    x = torch.relu(torch.randn((1, 128, 6, 20), generator=torch.Generator(device=DEV).manual_seed(5), device=DEV))
    fill_parameters_(ds, seed=5)
    ds = ds.to(DEV).eval()
    with torch.no_grad():
        ref = copy.deepcopy(ds).double()(ops.SplitMap.pack(x).dense().double())
        spy = _Spy(monkeypatch)
        got = ds(ops.SplitMap.pack(x), out_split=True)
    assert not isinstance(got, ops.SplitMap)
    assert_elementwise(got, ref, "DownsampleConv [1024, 1088]")
    assert [c[1] for c in spy.of("conv3x3_sp")] == [(1024, 128), (1024, 1024)]


class _Heads(nn.Module):
    def __init__(self, cin, rows):
        super().__init__()
        self.use_dir = True
        self.cls_head, self.reg_head, self.dir_head = nn.Conv2d(cin, 2, 1), nn.Conv2d(cin, 14, 1), nn.Conv2d(cin, rows - 16, 1)


@pytest.mark.parametrize("rows", [32, 33])
def test_merged_heads_route_at_32_rows_against_float64(rows, monkeypatch):
    m = _Heads(256, rows)
    fill_parameters_(m, seed=rows)
    m = m.to(DEV).eval()
    xs = ops.SplitMap.pack(torch.relu(torch.randn((1, 256, 20, 44), generator=torch.Generator(device=DEV).manual_seed(rows), device=DEV)))
    with torch.no_grad():
        xd = xs.dense().double()
        ref = {k: F.conv2d(xd, h.weight.double(), h.bias.double()) for k, h in (("cls_preds", m.cls_head), ("reg_preds", m.reg_head), ("dir_preds", m.dir_head))}
        spy = _Spy(monkeypatch)
        out = detector._run_heads(m, xs)
    for k in ref:
        assert_elementwise(out[k], ref[k], f"{rows} head rows: {k}")
    assert detector.heads_take_split_map(m) == (rows <= 32)
    assert [c[1:] for c in spy.of("heads_sp")] == ([(256, rows)] if rows <= 32 else [])
    assert spy.of("F.conv2d") == []                                          # (33 rows: the pointwise kernel on the float32 map)


@pytest.mark.parametrize("cfg,compression", [("mini_coalign", None), ("opv2v_coalign", None), ("opv2v_coalign", 4)])
def test_one_forward_launches_the_kernels_the_plan_names(cfg, compression, monkeypatch):
    """``routes.plan`` against what ``forward`` launches (not against the kernels' argument checks): one forward of the whole detector under a spy calls
    ``conv3x3_sp`` once per layer the plan puts on it, ``conv3x3_sp_s2`` once per strided SplitMap opener, ``conv3x3_sp_narrow`` for the compressor's encoder,
    one of ``heads_sp`` / ``pointwise_conv`` for the merged heads where the plan names the pointwise kernel, and the library not at all when the plan lists
    no fallback."""
    h = copy.deepcopy(builtin_config(cfg))
    if compression is not None:
        h["model"]["args"]["compression"] = compression
    assert bb.CONV_EMU_TERMS == bb.DEFAULT_CONV_EMU_TERMS          # (the plan below is the default arithmetic's)
    p = plan(h)
    model = detector.build_model(h)
    fill_parameters_(model, seed=7)
    model = model.to(DEV).eval()
    frame = detector.to_device(make_frame(h, 2, pillars_per_agent=150, seed=3, spread_xy=(4.0, 2.0), spread_yaw=45.0), DEV)
    with torch.no_grad():
        spy = _Spy(monkeypatch, more=("conv3x3_sp_narrow", "pointwise_conv"))
        out = model(frame)
    assert all(bool(torch.isfinite(v).all()) for v in out.values())
    mods = dict(model.named_modules())
    routes = p["layers"]
    # the strided openers of the plan ("..., SplitMap out" inside the ResNet): conv3x3_sp_s2 where the block's own decision says so for the input it gets
    # (a sparse canvas for the first block when the encoder hands one over, a dense map or a SplitMap otherwise), else the consumer-split kernel
    blocks = [mods[n.rsplit(".", 1)[0]] for n, r in routes.items() if r.endswith("SplitMap out") and ".resnet." in n]
    first = model.backbone.resnet.layer0[0]
    openers = [b for b in blocks if (b.route().s2_sparse if b is first and detector.sparse_canvas_route(model) else b.route().s2_dense)]
    assert len(blocks) == 3 and (cfg != "opv2v_coalign" or p["fallbacks"] == [])
    print(f"\n{cfg} compression {compression}: kernels {sorted(set(c[0] for c in spy.calls))}, fallbacks {p['fallbacks']}")
    assert len(spy.of("conv3x3_sp")) == sum(r.startswith(SP) for r in routes.values()) > 0
    assert len(spy.of("conv3x3_sp_s2")) == len(openers) > 0
    assert len(spy.of("conv3x3_sp_narrow")) == sum(r.startswith(NARROW) for r in routes.values()) == (0 if compression is None else 1)
    rows = sum(getattr(model, k).out_channels for k in ("cls_head", "reg_head", "dir_head"))
    head_launches = len(spy.of("heads_sp")) + len([c for c in spy.of("pointwise_conv") if c[1] == rows])
    assert head_launches == (1 if routes["cls_head"].startswith("pointwise") else 0)
    # the heads read a SplitMap where their route allows it and a one-layer shrink header on the SplitMap route, fed by the heads, hands one over
    handed = (routes.get("shrink_conv.layers.0.double_conv.0") == SP and len(model.shrink_conv.layers) == 1)
    assert len(spy.of("heads_sp")) == int(detector.heads_route(model).split_in and handed)
    if p["fallbacks"] == []:
        assert spy.of("F.conv2d") == []


# ------------------------------------------------------------------------------------------------ device placement of the ops (ops._device_op)
def test_device_placement_finds_the_tensor_inside_maps_lists_and_buffers():
    """``ops._device_tensor`` -- what ``_device_op`` places an op by -- looks through a SplitMap, a SparseCanvas, DecodeBuffers and lists / tuples (the first CUDA
    tensor in them, host tensors skipped)."""
    sm = ops.SplitMap.pack(torch.randn((1, 16, 4, 4), device=DEV))
    cuda_t, cpu_t = torch.randn(3, device=DEV), torch.randn(3)
    assert ops._device_tensor(sm) is sm.data
    assert ops._device_tensor([(cpu_t, None), (cuda_t, 3)]) is cuda_t
    assert ops._device_tensor(((cpu_t,), [sm, cuda_t])) is sm.data
    feats = torch.zeros((4, 16), device=DEV)
    sc = ops.SparseCanvas(feats, torch.zeros(16, dtype=torch.int64, device=DEV), torch.zeros(4, dtype=torch.int32, device=DEV), None, 1, 16, 4, 4)
    assert ops._device_tensor(sc) is feats
    db = ops.DecodeBuffers(64, 2, 4, 4, 16, DEV)
    assert ops._device_tensor(db) is db.counts


class _OtherDeviceCurrent:
    """The caller's current device is "1": ``torch.cuda.current_device()`` answers 1 outside a ``torch.cuda.device(...)`` block and the block's device inside it;
    every device entered is recorded.  (The kernels still run on cuda:0, the only device of the box: this checks what the wrapper selects, on one GPU.)"""

    def __init__(self, m):
        self.current, self.entered = [1], []
        fake = self

        class device:
            def __init__(self, d):
                self.idx = d if isinstance(d, int) else torch.device(d).index

            def __enter__(self):
                fake.entered.append(self.idx)
                fake.current.append(self.idx)

            def __exit__(self, *exc):
                fake.current.pop()
                return False
        m.setattr(torch.cuda, "current_device", lambda: fake.current[-1])
        m.setattr(torch.cuda, "device", device)


def test_ops_run_on_the_device_of_a_split_map_a_list_or_a_tensor_argument(monkeypatch):
    """With another device current, ``pointwise_heads_split`` (a list of layers first), ``heads_sp`` / ``conv3x3_sp`` (a SplitMap first) and ``boxes_overlap_bev``
    (tensors) select their arguments' device for the launch -- and compute what they compute with that device current."""
    from coalign_amd.backbone import PointwisePack
    g = torch.Generator(device=DEV).manual_seed(9)
    layers, c = [], 0
    for cin, up, cout in ((64, 1, 64), (128, 2, 32)):
        x = torch.relu(torch.randn((1, cin, 16 // up, 24 // up), generator=g, device=DEV))
        wt = torch.randn((cin, cout, up, up), generator=g, device=DEV) / cin ** 0.5
        layers.append((x, PointwisePack(wt, True).get(), torch.randn(cout, generator=g, device=DEV) * 0.1, cout, up, c))
        c += cout
    sm = ops.SplitMap.pack(torch.randn((1, 64, 16, 24), generator=g, device=DEV))
    w_heads = torch.randn((20, 64), generator=g, device=DEV) / 8.0
    img_heads, b_heads = ops.pack_heads_sp_weight(w_heads), torch.randn(20, generator=g, device=DEV)
    w16, b64 = ops.pack_conv3x3_emu_weight(torch.randn((64, 64, 3, 3), generator=g, device=DEV) / 24.0, 16, True), torch.randn(64, generator=g, device=DEV)
    boxes = torch.rand((5, 7), generator=g, device=DEV) * torch.tensor([10, 10, 1, 4, 2, 1, 3.0], device=DEV)
    calls = {
        "pointwise_heads_split": lambda: ops.pointwise_heads_split(layers, ops.SplitMap.empty(1, c, 16, 24, DEV)).data,
        "heads_sp": lambda: ops.heads_sp(sm, img_heads, b_heads, 20),
        "conv3x3_sp": lambda: ops.conv3x3_sp(sm, w16, b64, 64, None, True, out_split=False),
        "boxes_overlap_bev": lambda: ops.boxes_overlap_bev(boxes, boxes),
    }
    want = {k: f() for k, f in calls.items()}
    torch.cuda.synchronize()
    for k, f in calls.items():
        with monkeypatch.context() as m:
            fake = _OtherDeviceCurrent(m)
            got = f()
        torch.cuda.synchronize()
        assert fake.entered and set(fake.entered) == {0}, (k, fake.entered)
        assert got.device == torch.device(DEV) and torch.equal(got, want[k]), k
