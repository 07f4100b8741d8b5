"""NaiveCompressor on the SplitMap kernels: the narrow-output convolution against float64 and against the 64-channel kernel, the module on
both sides of its route predicate, and the detector with ``compression`` in its config.

Kernel level: ``coalign_conv3x3_sp_narrow`` (include/coalign_amd_narrow.h, csrc/conv3x3_narrow.hip) with output channels on scales 2^-20 ... 2^6 and one
all-zero channel, compared PER OUTPUT CHANNEL with the float64 convolution of the 22-bit values it reads (bound and helpers of tests/test_sp_limits_gpu.py,
copied); bit equality of its two input kinds and with ``coalign_conv3x3_sp`` on the same weights zero-padded to 64 output channels (same matrix instruction,
same products in the same order: csrc/conv3x3_narrow.hip's header).

Module / model level: the float32 forward against the module's own float64 forward at the project's model-level tolerance (conftest ``assert_elementwise``), with
the kernels that ran recorded by a spy; the error is also printed as a ratio to the error of the plain float32 ``nn.Sequential`` forward (recorded in DESIGN.md
section 8, not asserted).
"""
import copy

import pytest
import torch
import torch.nn.functional as F

from coalign_amd import backbone as bb
from coalign_amd import ops
from coalign_amd.config import builtin_config
from coalign_amd.detector import build_model, to_device
from coalign_amd.synthetic import fill_parameters_, make_frame
from conftest import assert_elementwise
from sp_helpers import assert_split_map_holds

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BOUND = 3e-6                     # of the channel's own scale: the bound the project uses for sp16 layers (tests/test_sp_limits_gpu.py)
SP_ABS = 2.0 ** -33              # what a SplitMap holds of a value below 2^-13
ZERO_CH = 3                      # the all-zero output channel of every mixed-scale layer


# ---- copied from tests/test_sp_limits_gpu.py (that file is a yardstick and stays as it is)
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
    """max over channels of max |got - ref| / the channel's scale: max |pre-activation| in that channel (``pre``; ``ref`` itself when there is no activation)."""
    scale = (ref if pre is None else pre).abs().amax(dim=(0, 2, 3))
    err = (got.double() - ref).abs().amax(dim=(0, 2, 3))
    return float(torch.where(scale > 0, err / scale.clamp_min(1e-300), err).max())


def assert_channels_close(got, ref, what, abs_floor=0.0, pre=None):
    """Every output channel within BOUND of its own scale (+ ``abs_floor``), as an element-wise bound."""
    scale = (ref if pre is None else pre).abs().amax(dim=(0, 2, 3), keepdim=True)
    bad = (got.double() - ref).abs() > BOUND * scale + abs_floor
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} elements outside {BOUND:g} of their channel's scale; worst {channel_error(got, ref, pre):.3e}"
    return channel_error(got, ref, pre)


def _conv64_linear(x, w, b):
    """The pre-activation in float64: conv3x3(x, w, stride 1, pad 1) + b."""
    N, Ci, H, W = x.shape
    xp = F.pad(x.double(), (1, 1, 1, 1))
    out = torch.zeros((N, w.shape[0], H, W), dtype=torch.float64, device=x.device)
    for dy in range(3):
        for dx in range(3):
            out += torch.einsum("oc,nchw->nohw", w.double()[:, :, dy, dx], xp[:, :, dy:dy + H, dx:dx + W])
    return out + b.double().view(1, -1, 1, 1)


def _round11(x):
    """x rounded to 11 significant bits (the high fp16 term of the pair; low term dropped), scale free."""
    return ((x.contiguous().view(torch.int32) + (1 << 12)) & -(1 << 13)).view(torch.float32)


# (N, Cin, Cout, H, W, relu): Cin 16 / 64 / 256 x Cout 16 / 32, ReLU on and off, one-pixel, thin, canvas-sized maps and two that no tile edge (16 x 32) divides
NARROW_CASES = [
    (8, 16, 16, 1, 1, True),
    (3, 64, 32, 3, 131, False),
    (2, 256, 16, 131, 3, True),
    (1, 64, 16, 200, 704, True),
    (2, 64, 32, 200, 704, False),
    (5, 256, 32, 37, 75, False),
    (2, 16, 32, 9, 33, True),
    (3, 64, 16, 21, 45, False),
]


def _narrow_case(case):
    N, Ci, Co, H, W, relu = case
    g = torch.Generator(device=DEV).manual_seed(sum(case[:5]))
    x = torch.randn((N, Ci, H, W), generator=g, device=DEV)
    xs = ops.SplitMap.pack(x)
    w, b, _ = mixed_layer(g, Co, Ci)
    pre = _conv64_linear(xs.dense(), w, b)                  # (the 22-bit values both input kinds hold)
    return x, xs, w, b, (torch.relu(pre) if relu else pre), pre


def _padded64(w, b):
    w64, b64 = w.new_zeros((64,) + tuple(w.shape[1:])), b.new_zeros(64)
    w64[:w.shape[0]], b64[:w.shape[0]] = w, b
    return w64, b64


@pytest.mark.parametrize("case", NARROW_CASES, ids=lambda c: f"{c[0]}x{c[1]}to{c[2]}@{c[3]}x{c[4]}-{'relu' if c[5] else 'linear'}")
def test_conv3x3_sp_narrow_mixed_channel_scales_against_float64(case):
    """Every output channel of ``coalign_conv3x3_sp_narrow`` within 3e-6 of its own scale (+ 2^-33, what a SplitMap keeps of small values) of the float64
    convolution, for a SplitMap input and for a channels-last float32 input; the two kinds agree bit for bit; the SplitMap holds the float32 result of the
    64-channel kernel on the zero-padded weights; the all-zero channel is exactly act(bias)."""
    N, Ci, Co, H, W, relu = case
    x, xs, w, b, ref, pre = _narrow_case(case)
    img = ops.pack_conv3x3_narrow_weight(w)
    y_sp = ops.conv3x3_sp_narrow(xs, img, b, Co, relu)
    x_cl = x.contiguous(memory_format=torch.channels_last)
    assert ops.nhwc_memory(x_cl)
    y_cl = ops.conv3x3_sp_narrow(x_cl, img, b, Co, relu)
    assert y_sp.shape == (N, Co, H, W) and torch.equal(y_sp.data, y_cl.data), case
    if H * W > 1:                                           # an NCHW tensor goes through SplitMap.pack inside the op: the same bits again
        assert not ops.nhwc_memory(x) and torch.equal(ops.conv3x3_sp_narrow(x, img, b, Co, relu).data, y_sp.data), case
    got = y_sp.dense()
    err = assert_channels_close(got, ref, case, abs_floor=SP_ABS, pre=pre)
    zero = b[ZERO_CH].view(1, 1, 1).expand(N, H, W)
    want = got.clone()                                      # (what the pairs hold is canonical: rounding it to 22 bits again changes nothing)
    want[:, ZERO_CH] = torch.relu(zero) if relu else zero
    assert_split_map_holds(y_sp, want, (case, "the all-zero channel is act(bias)"))
    if not relu:
        assert float(got.min()) < 0                         # (negative outputs are compared too)
    w64, b64 = _padded64(w, b)
    cl = ops.conv3x3_sp(xs, ops.pack_conv3x3_emu_weight(w64, 16, True), b64, 64, None, relu, out_split=False)[:, :Co]
    err32 = assert_channels_close(cl, ref, (case, "float32 of the 64-channel kernel"), pre=pre)
    assert_split_map_holds(y_sp, cl, case)
    assert not ops.sp_range_exceeded(DEV)
    print(f"\nconv3x3_sp_narrow {case}: worst channel error of the pairs {err:.2e} of the channel scale (bound {BOUND:g} + 2^-33: the 2^-20 channels sit below what a pair"
          f" resolves), of the float32 values they hold {err32:.2e} (bound {BOUND:g})")


@pytest.mark.parametrize("case", NARROW_CASES, ids=lambda c: f"{c[0]}x{c[1]}to{c[2]}@{c[3]}x{c[4]}-{'relu' if c[5] else 'linear'}")
def test_conv3x3_sp_narrow_is_bit_equal_to_the_64_channel_kernel(case):
    """The first Cout channels of ``coalign_conv3x3_sp`` on the same weights zero-padded to 64 output channels equal the narrow kernel's SplitMap bit for bit (both
    use v_mfma_f32_32x32x16_f16, interval by interval and tap by tap, w_h x_l' + w_l' x_h then w_h x_h; Cout 16 repeats its rows in the instruction's upper half
    and never stores them), whichever geometry the wide kernel picks; and a narrower layer zero-padded to the kernel's width has exactly zero padded channels."""
    N, Ci, Co, H, W, relu = case
    x, xs, w, b, ref, pre = _narrow_case(case)
    y = ops.conv3x3_sp_narrow(xs, ops.pack_conv3x3_narrow_weight(w), b, Co, relu)
    w64, b64 = _padded64(w, b)
    for geo in (0, 100081):
        wide = ops.conv3x3_sp(xs, ops.pack_conv3x3_emu_weight(w64, 16, True), b64, 64, None, relu, out_split=True, geometry=geo)
        assert torch.equal(wide.data[:, :Co // 16], y.data), (case, geo)
    mid = Co - 11                                           # 5 or 21 real channels in a 16- or 32-wide launch
    wp, bp = w.clone(), b.clone()
    wp[mid:], bp[mid:] = 0, 0
    yp = ops.conv3x3_sp_narrow(x.contiguous(memory_format=torch.channels_last), ops.pack_conv3x3_narrow_weight(wp), bp, Co, relu)
    d = yp.dense()
    assert float(d[:, mid:].abs().max()) == 0 and int(yp.data.view(torch.int16)[:, (mid + 15) // 16:].ne(0).sum()) == 0, case
    if mid > ZERO_CH + 1:
        assert torch.equal(d[:, :mid], y.dense()[:, :mid]), case
    assert not ops.sp_range_exceeded(DEV)


def test_the_channel_bound_separates_the_split_from_a_kernel_that_drops_the_low_term():
    """The per-channel bound can fail: the float64 convolution of the operands rounded to 11 bits -- a kernel that kept only the high fp16 term -- is refused
    at a shape where the kernel itself passes."""
    case = NARROW_CASES[1]
    x, xs, w, b, ref, pre = _narrow_case(case)
    lossy = _conv64_linear(_round11(xs.dense()), _round11(w), b).float()
    with pytest.raises(AssertionError):
        assert_channels_close(lossy, ref, "11-bit operands", abs_floor=SP_ABS, pre=pre)
    print(f"\n11-bit operands: worst channel error {channel_error(lossy, ref):.2e} of the channel scale (bound {BOUND:g})")
    assert_channels_close(ops.conv3x3_sp_narrow(xs, ops.pack_conv3x3_narrow_weight(w), b, case[2], case[5]).dense(), ref, case, abs_floor=SP_ABS, pre=pre)


def test_range_flag_reports_a_value_beyond_the_pairs_range():
    """``range_flag`` as include/coalign_amd.h (9e): an output beyond 65504 sets bit 0."""
    ops.sp_range_exceeded(DEV)
    x = torch.full((1, 16, 4, 4), 100.0, device=DEV)
    w = torch.full((16, 16, 3, 3), 10.0, device=DEV)
    y = ops.conv3x3_sp_narrow(ops.SplitMap.pack(x), ops.pack_conv3x3_narrow_weight(w), torch.zeros(16, device=DEV), 16, True)
    assert float(y.dense().max()) > 65504 * 0.99
    assert ops.sp_range_exceeded(DEV) and not ops.sp_range_exceeded(DEV)


# ------------------------------------------------------------------------------------------------ module
class _Spy:
    """Records which kernel served which layer during one forward (pattern: tests/test_sp_limits_gpu.py)."""

    def __init__(self, monkeypatch):
        self.calls, self.returned, self.packs = [], [], []
        for name in ("conv3x3_sp", "conv3x3_sp_s2", "conv3x3_sp_narrow", "conv3x3_emu_bias_act"):
            monkeypatch.setattr(ops, name, self._wrap(name, getattr(ops, name)))
        monkeypatch.setattr(F, "conv2d", self._wrap("F.conv2d", F.conv2d))
        monkeypatch.setattr(ops.SplitMap, "pack", staticmethod(self._wrap("SplitMap.pack", ops.SplitMap.pack)))

    def _wrap(self, name, fn):
        def spy(*args, **kwargs):
            if name == "SplitMap.pack":
                self.packs.append(tuple(args[0].shape))
                return fn(*args, **kwargs)
            if name == "F.conv2d":
                self.calls.append((name, tuple(args[1].shape[:2]), None, None))
            else:
                self.calls.append((name, (args[3], args[0].shape[1]), kwargs.get("w_skip") is not None if name == "conv3x3_sp_s2" else None, args[0]))
            out = fn(*args, **kwargs)
            self.returned.append((name, out))
            return out
        return spy

    def of(self, name):
        return [c for c in self.calls if c[0] == name]

    def names(self):
        return [c[0] for c in self.calls]


def _compressor(dim, ratio, seed):
    m = bb.NaiveCompressor(dim, ratio)
    fill_parameters_(m, seed=seed)
    return m.to(DEV).eval()


RATIO_LOG = {}


@pytest.mark.parametrize("memory", ["channels_last", "nchw"])
@pytest.mark.parametrize("ratio", [1, 2, 3, 4, 8, 64])
def test_naive_compressor_on_the_split_map_route(ratio, memory, monkeypatch):
    """``NaiveCompressor(64, r)`` (mid 64, 32, 21, 16, 8, 1; randomised BatchNorm statistics): no ``F.conv2d``; the encoder on the narrow kernel at the padded
    width (on ``conv3x3_sp`` for mid 64), both decoder layers on ``conv3x3_sp``; the output within the model-level tolerance of the module's own float64 forward;
    ``module(x)`` returns a tensor, ``module(x, out_split=True)`` the SplitMap of the same values.  Printed, not asserted: this error as a ratio to the plain
    float32 ``nn.Sequential`` forward's error against the same float64 result."""
    m = _compressor(64, ratio, 50 + ratio)
    g = torch.Generator(device=DEV).manual_seed(ratio)
    x = torch.randn((2, 64, 37, 75), generator=g, device=DEV)
    if memory == "channels_last":
        x = x.contiguous(memory_format=torch.channels_last)
    mid, cp = 64 // ratio, (64 // ratio + 15) // 16 * 16
    with torch.no_grad():
        ref = copy.deepcopy(m).double()(x.double())
        plain = m.decoder(m.encoder(x))
        spy = _Spy(monkeypatch)
        got = m(x)
        calls = list(spy.calls)
        got_sp = m(x, out_split=True)
    assert "F.conv2d" not in [c[0] for c in calls] and "conv3x3_emu_bias_act" not in [c[0] for c in calls]
    if cp <= 32:
        assert [(c[0], c[1]) for c in calls] == [("conv3x3_sp_narrow", (cp, 64)), ("conv3x3_sp", (64, cp)), ("conv3x3_sp", (64, 64))], calls
        assert len(spy.packs) == 2 * (memory == "nchw")        # (two forwards) the channels-last canvas is read in place, the NCHW one packed first
        mid_map = [o for n, o in spy.returned if n == "conv3x3_sp_narrow"][0].dense()
        assert mid_map.shape[1] == cp and (cp == mid or float(mid_map[:, mid:].abs().max()) == 0)
    else:
        assert [(c[0], c[1]) for c in calls] == [("conv3x3_sp", (64, 64))] * 3, calls
    assert torch.is_tensor(got) and got.shape == ref.shape and isinstance(got_sp, ops.SplitMap)
    assert_split_map_holds(got_sp, got, ("out_split", ratio))
    e = assert_elementwise(got, ref, f"NaiveCompressor(64, {ratio}) {memory}")
    scale = float(ref.abs().max())
    e_plain = float((plain.double() - ref).abs().max()) / scale
    RATIO_LOG[ratio, memory] = e / max(e_plain, 1e-30)
    assert not ops.sp_range_exceeded(DEV)
    print(f"\nNaiveCompressor(64, {ratio}) {memory}: SplitMap route {e:.2e} of the scale against float64, plain float32 nn.Sequential {e_plain:.2e}: ratio {e / max(e_plain, 1e-30):.2f}"
          f" (worst so far {max(RATIO_LOG.values()):.2f})")


@pytest.mark.parametrize("why", ["training", "split_maps_off", "half", "input_dim_24", "conv_emu_3"])
def test_naive_compressor_keeps_the_old_route_outside_the_predicate(why, monkeypatch):
    """Training mode, ``COALIGN_SPLIT_MAPS`` off, another arithmetic mode, a half input and ``input_dim = 24`` all take the route of before: ``F.conv2d`` three
    times, none of the SplitMap kernels."""
    dim = 24 if why == "input_dim_24" else 64
    m = _compressor(dim, 2, 7)
    x = torch.randn((2, dim, 19, 40), device=DEV)
    if why == "training":
        m.train()
    elif why == "split_maps_off":
        monkeypatch.setattr(bb, "SPLIT_MAPS", False)
    elif why == "conv_emu_3":
        monkeypatch.setattr(bb, "CONV_EMU_TERMS", 3)
    elif why == "half":
        m, x = m.half(), x.half()
    with torch.no_grad():
        ref = copy.deepcopy(m).double()(x.double()) if why != "training" else None
        spy = _Spy(monkeypatch)
        got = m(x)
    assert [c[0] for c in spy.calls] == ["F.conv2d"] * 3, (why, spy.names())
    assert torch.is_tensor(got) and got.dtype == x.dtype
    if ref is not None:
        assert_elementwise(got, ref, why, rtol=1e-2 if why == "half" else 1e-4, floor=1e-2 if why == "half" else 1e-5)
    with torch.no_grad():                                   # asking for a SplitMap does not change the route: the caller gets the tensor
        assert torch.is_tensor(m(x, out_split=True))


# ------------------------------------------------------------------------------------------------ model
def _model(cfg, ratio=4, resnet=True):
    h = copy.deepcopy(builtin_config(cfg))
    h["model"]["args"]["compression"] = ratio
    if not resnet:
        h["model"]["args"]["base_bev_backbone"]["resnet"] = False
    model = build_model(h)
    fill_parameters_(model, seed=0, cls_bias=-1.0)
    return h, model


def _oracle_heads(model, h, frame):
    from oracle import coalign_oracle as oracle
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    return oracle.coalign_forward(sd, h["model"]["args"], frame)


@pytest.mark.parametrize("cfg", ["mini_coalign", "opv2v_coalign"])
def test_model_with_compression_runs_the_compressor_on_split_maps(cfg, monkeypatch):
    """``compression: 4`` in the config (two agents): no ``F.conv2d`` anywhere in the forward, the narrow kernel once, and the first ResNet block's strided
    convolution + fused skip reading the very SplitMap the compressor's last layer returned; the heads match, element-wise at the model-level tolerance, those of the same model with
    the compressor on the library route."""
    h, model = _model(cfg)
    frame = make_frame(h, 2, pillars_per_agent=150 if cfg.startswith("mini") else 3000, seed=5)
    model = model.to(DEV).eval()
    with torch.no_grad():
        spy = _Spy(monkeypatch)
        out = model(to_device(frame, DEV))
    assert spy.of("F.conv2d") == [], spy.of("F.conv2d")
    assert [c[1] for c in spy.of("conv3x3_sp_narrow")] == [(16, 64)]
    handed = [o for n, o in spy.returned if n == "conv3x3_sp"][1]          # the compressor's third layer = the second conv3x3_sp of the forward
    assert spy.names()[:3] == ["conv3x3_sp_narrow", "conv3x3_sp", "conv3x3_sp"] and isinstance(handed, ops.SplitMap)
    s2 = spy.of("conv3x3_sp_s2")
    assert s2[0][3] is handed and s2[0][2] is True and s2[0][1] == (64, 64), s2[0][:3]
    monkeypatch.undo()
    # the same weights with the compressor on the library route (SplitMaps off inside the compressor only): the heads agree at the model-level tolerance
    with torch.no_grad():
        monkeypatch.setattr(bb.NaiveCompressor, "takes_split_maps", lambda self: False)
        old = model(to_device(frame, DEV))
    for k in ("cls_preds", "reg_preds", "dir_preds"):
        e = assert_elementwise(out[k], old[k], (cfg, k))
        print(f"\n{cfg} compression 4, {k}: SplitMap compressor against the library compressor {e:.2e} of the scale")
    assert not ops.sp_range_exceeded(DEV)


def test_mini_model_with_compression_matches_the_oracle_and_a_plain_backbone_gets_a_tensor(monkeypatch):
    """The mini model's heads against the CPU oracle (the reference's op sequence) with the compressor on the new route, for the ResNet backbone and for
    ``resnet: false`` -- whose first block reads a tensor: the compressor is then asked for one and the heads still match."""
    for resnet in (True, False):
        h, model = _model("mini_coalign", resnet=resnet)
        frame = make_frame(h, 2, pillars_per_agent=150, seed=3)
        with torch.no_grad():
            ref = _oracle_heads(model, h, frame)
        model = model.to(DEV).eval()
        seen = []
        orig = bb.NaiveCompressor.forward

        def forward(self, x, out_split=False):
            y = orig(self, x, out_split=out_split)
            seen.append((out_split, type(y)))
            return y
        monkeypatch.setattr(bb.NaiveCompressor, "forward", forward)
        with torch.no_grad():
            spy = _Spy(monkeypatch)
            out = model(to_device(frame, DEV))
        monkeypatch.undo()
        assert seen == [(True, ops.SplitMap)] if resnet else seen == [(False, torch.Tensor)], seen
        assert len(spy.of("conv3x3_sp_narrow")) == 1 and (resnet or spy.of("conv3x3_sp_s2") == [])
        for k in ("cls_preds", "reg_preds", "dir_preds"):
            e = assert_elementwise(out[k], ref[k], (resnet, k))
            print(f"\nmini_coalign compression 4, resnet={resnet}, {k}: {e:.2e} of the scale against the oracle")


def test_compressor_and_backbone_inside_a_captured_graph_replay_to_the_same_bits():
    """No allocation-dependent state, no workspace, everything on the caller's stream: the compressor (narrow kernel included) and the ResNet stages behind it
    are captured by ``torch.cuda.graph`` and the replays reproduce the eager result bit for bit, also after the input buffer's content changed."""
    h, model = _model("mini_coalign")
    model = model.to(DEV).eval()
    gy, gx = [int(v) for v in h["model"]["args"]["point_pillar_scatter"]["grid_size"]][1::-1]
    g = torch.Generator(device=DEV).manual_seed(11)
    canvases = [torch.randn((2, 64, gy, gx), generator=g, device=DEV).relu_().contiguous(memory_format=torch.channels_last) for _ in range(2)]

    def body(x):
        return model.backbone.get_multiscale_feature(model.naive_compressor(x, out_split=True))
    stream = torch.cuda.Stream(device=DEV)
    with torch.no_grad(), torch.cuda.stream(stream):
        eager = [[f.clone() for f in body(c)] for c in canvases]      # (also the warm-up: weight images, the range word)
        static = canvases[0].clone()
        stream.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            feats = body(static)
        for i in (0, 1, 0):
            static.copy_(canvases[i])
            graph.replay()
            stream.synchronize()
            for a, b in zip(feats, eager[i]):
                assert torch.equal(a, b), i
    torch.cuda.synchronize()
