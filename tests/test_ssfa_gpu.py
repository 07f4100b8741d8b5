"""The SSFA neck of the SECOND detectors on kernels, on the GPU (csrc/ssfa_neck.hip): ``ops.deconv3x3_s2_sp`` against the float64 scatter definition per output
channel (the project's sp16 bound), single taps bit for bit, the residual behind the activation, range word, determinism, graph replay and bit equality with
``ops.conv3x3_sp`` on the zero-stuffed map; ``ops.ssfa_blend`` against float64, ``SplitMap.pack`` and its saturated ends; ``second.SSFA`` on the kernel route against
its own float64 forward with the kernels that ran compared with ``plan()``; both mini models with the switch on against the switch off, under a captured graph, and
outside the predicate."""
import functools

import pytest
import torch

import sparse3d_cases as cases
from conftest import assert_elementwise
from coalign_amd import hip, ops, second
from coalign_amd.config import builtin_config
from coalign_amd.detector import build_model, to_device
from ssfa_reference import blend_f64, deconv_f64, fill_by_formula_, ssfa_f64
from test_lss_bev_gpu import BOUND, SP_ABS, ZERO_CH, assert_channels_close, channel_error, mixed_layer

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
T_H, T_W = ops.DECONV3X3_TILE


@pytest.fixture(autouse=True)
def _trunk_on_kernels(monkeypatch):
    monkeypatch.setenv("COALIGN_SP3D", "1")


def _round22(x):
    return ((x.contiguous().view(torch.int32) + 2) & -4).view(torch.float32)


def _image(w):
    """The weight image of a ConvTranspose2d weight [Cin, Cout, 3, 3]: no new packer."""
    return ops.pack_conv3x3_emu_weight(w.permute(1, 0, 2, 3).contiguous(), 16, True)


# ---- deconv3x3_s2_sp --------------------------------------------------------------------------------------------------------------------------------------------
# (N, Cin, Cout, h, w): every neighbour out of range | smallest map with all neighbours | odd sizes | the mini config's layer | one pixel past a tile edge in both
# directions | one full-size map | the widest supported shape
DECONV_CASES = [(3, 16, 64, 1, 1), (2, 32, 64, 2, 2), (2, 64, 64, 3, 5), (2, 256, 128, 8, 16), (1, 256, 128, T_H + 1, T_W + 1), (1, 256, 128, 50, 176), (1, 512, 256, 4, 4)]
_DECONV = {}


def _deconv_case(case):
    """Inputs and the float64 pre-activation of a case, computed once and shared by its tests (never modified)."""
    if case not in _DECONV:
        N, Ci, Co, h, w = case
        g = torch.Generator(device=DEV).manual_seed(sum(case))
        x = torch.randn((N, Ci, h, w), generator=g, device=DEV)
        wc, b = mixed_layer(g, Co, Ci, 3)                              # [Co, Ci, 3, 3]: output channels on scales 2^-20 ... 2^6, channel ZERO_CH all zero
        wt = wc.permute(1, 0, 2, 3).contiguous()                       # the ConvTranspose2d layout [Ci, Co, 3, 3]
        xs = ops.SplitMap.pack(x)
        _DECONV[case] = (xs, wt, b, _image(wt), deconv_f64(xs.dense(), _round22(wt), b), xs.dense())
    return _DECONV[case]


@pytest.mark.parametrize("relu", [True, False], ids=["relu", "linear"])
@pytest.mark.parametrize("case", DECONV_CASES, ids=lambda c: "x".join(str(v) for v in c))
def test_deconv_mixed_channel_scales_against_float64(case, relu):
    """Every output channel within 3e-6 of its own scale + 2^-33 of the float64 scatter definition on the 22-bit operands; the all-zero channel is exactly
    act(bias) as a SplitMap holds it; every element of a NaN-poisoned output buffer is written; the range word stays clear."""
    N, Ci, Co, h, w = case
    xs, wt, b, image, pre, x22 = _deconv_case(case)
    ref = torch.relu(pre) if relu else pre
    ops.sp_range_exceeded(DEV)
    y = ops.deconv3x3_s2_sp(xs, image, b, Co, relu=relu)
    assert y.shape == (N, Co, 2 * h, 2 * w) and tuple(y.data.shape) == (N, Co // 16, 4, 2 * h, 2 * w, 8)
    got = y.dense()
    lib = torch.nn.functional.conv_transpose2d(x22, wt, b, stride=2, padding=1, output_padding=1)
    print(f"\ndeconv3x3_s2_sp {case} {'relu' if relu else 'linear'}: worst channel error beyond 2^-33 {channel_error(got, ref, pre, SP_ABS):.2e} of the channel scale "
          f"(bound {BOUND:g}); float32 F.conv_transpose2d {channel_error(torch.relu(lib) if relu else lib, ref, pre):.2e}")
    assert_channels_close(got, ref, case, pre)
    zero = b[ZERO_CH].view(1, 1, 1, 1).expand(N, 16, 2 * h, 2 * w)
    assert torch.equal(got[:, ZERO_CH], ops.SplitMap.pack(torch.relu(zero) if relu else zero).dense()[:, 0]), case
    if not relu:
        assert float(got.min()) < 0
    assert not ops.sp_range_exceeded(DEV)
    poisoned = torch.full_like(y.data, float("nan"))
    hip.check(hip.lib().coalign_deconv3x3_s2_sp(xs.data.data_ptr(), image.data_ptr(), b.data_ptr(), None, poisoned.data_ptr(), N, Ci, Co, h, w, int(relu), None, None),
              "coalign_deconv3x3_s2_sp")
    torch.cuda.synchronize()
    assert not bool(torch.isnan(poisoned).any()) and torch.equal(poisoned, y.data)


@pytest.mark.parametrize("ky,kx", [(ky, kx) for ky in range(3) for kx in range(3)])
def test_deconv_single_taps_land_where_the_definition_puts_them(ky, kx):
    """A one-hot weight w[ci0, co0, ky, kx] = 1: the output is the 22-bit input channel at (2y - 1 + ky, 2x - 1 + kx) and zero elsewhere, bit for bit -- a wrong
    tap-to-class or tap-to-offset mapping cannot hide behind a tolerance."""
    N, Ci, Co, h, w = 2, 32, 64, T_H + 3, T_W + 2
    ci0, co0 = 21, 37
    g = torch.Generator(device=DEV).manual_seed(9 + 3 * ky + kx)
    xs = ops.SplitMap.pack(torch.randn((N, Ci, h, w), generator=g, device=DEV))
    x22 = xs.dense()
    wt = torch.zeros((Ci, Co, 3, 3), device=DEV)
    wt[ci0, co0, ky, kx] = 1.0
    got = ops.deconv3x3_s2_sp(xs, _image(wt), torch.zeros(Co, device=DEV), Co, relu=False).dense()
    want = torch.zeros((N, Co, 2 * h, 2 * w), device=DEV)
    y0, x0 = int(ky == 0), int(kx == 0)
    ys, xs0 = 2 * y0 - 1 + ky, 2 * x0 - 1 + kx
    want[:, co0, ys:ys + 2 * (h - y0):2, xs0:xs0 + 2 * (w - x0):2] = x22[:, ci0, y0:, x0:]
    assert float(want.abs().sum()) > 0 and torch.equal(got, want)
    assert torch.equal(want.double(), deconv_f64(x22, wt))


def test_deconv_adds_the_residual_behind_the_activation():
    """``relu(bn(deconv(x))) + x_trans_0`` (cia_ssd_utils.py:45), not ``relu(... + x_trans_0)``: on inputs where at least a tenth of the elements have a negative
    pre-activation AND a positive residual the kernel matches the first and the second is outside the bound."""
    case = DECONV_CASES[3]
    N, Ci, Co, h, w = case
    xs, wt, b, image, pre, x22 = _deconv_case(case)
    g = torch.Generator(device=DEV).manual_seed(77)
    scale = pre.abs().amax(dim=(0, 2, 3), keepdim=True)
    r = (torch.randn(pre.shape, generator=g, device=DEV, dtype=torch.float64) * 0.5 * scale).float().contiguous(memory_format=torch.channels_last)
    share = float(((pre.cpu() < 0) & (r.cpu() > 0)).double().mean())              # (from the float64 reference and the residual alone, counted on the CPU)
    assert share >= 0.10, share
    right, wrong = torch.relu(pre) + r.double(), torch.relu(pre + r.double())
    got = ops.deconv3x3_s2_sp(xs, image, b, Co, residual=r, relu=True).dense()
    both = torch.maximum(pre.abs(), right.abs())
    assert_channels_close(got, right, "relu(d) + r", both)
    with pytest.raises(AssertionError):
        assert_channels_close(got, wrong, "relu(d + r)", both)
    assert torch.equal(ops.deconv3x3_s2_sp(xs, image, b, Co, residual=r.contiguous(), relu=True).data, ops.deconv3x3_s2_sp(xs, image, b, Co, residual=r, relu=True).data)
    lin = ops.deconv3x3_s2_sp(xs, image, b, Co, residual=r, relu=False).dense()
    assert_channels_close(lin, pre + r.double(), "d + r", both)
    with pytest.raises(ValueError):
        ops.deconv3x3_s2_sp(xs, image, b, Co, residual=r[:, :, :-1])


def test_deconv_range_word():
    """One output above 65504 sets bit 0; a run below it leaves the word 0."""
    case = DECONV_CASES[2]
    xs, wt, b, image, pre, x22 = _deconv_case(case)
    ops.sp_range_exceeded(DEV)
    y = ops.deconv3x3_s2_sp(xs, image, b, case[2], relu=False)
    assert float(y.dense().abs().max()) < 65504 and not ops.sp_range_exceeded(DEV)
    big = b.clone()
    big[17] = 70000.0
    y = ops.deconv3x3_s2_sp(xs, image, big, case[2], relu=False)
    assert bool(torch.isfinite(y.data).all()) and ops.sp_range_exceeded(DEV) and not ops.sp_range_exceeded(DEV)


def test_deconv_repeats_and_replays_under_a_captured_graph():
    """Two runs give the same bits; a captured graph replayed onto new input contents gives the eager bits of those."""
    case = DECONV_CASES[4]
    N, Ci, Co, h, w = case
    xs, wt, b, image, pre, x22 = _deconv_case(case)
    g = torch.Generator(device=DEV).manual_seed(3)
    r = torch.randn((N, 2 * h, 2 * w, Co), generator=g, device=DEV).permute(0, 3, 1, 2)
    first = ops.deconv3x3_s2_sp(xs, image, b, Co, residual=r)
    assert torch.equal(ops.deconv3x3_s2_sp(xs, image, b, Co, residual=r).data, first.data)
    static = ops.SplitMap(xs.data.clone())
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        ops.deconv3x3_s2_sp(static, image, b, Co, residual=r)
    torch.cuda.current_stream().wait_stream(stream)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        out = ops.deconv3x3_s2_sp(static, image, b, Co, residual=r)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out.data, first.data)
    other = ops.SplitMap.pack(torch.randn((N, Ci, h, w), generator=g, device=DEV))
    static.data.copy_(other.data)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out.data, ops.deconv3x3_s2_sp(other, image, b, Co, residual=r).data) and not torch.equal(out.data, first.data)


@pytest.mark.parametrize("relu", [True, False], ids=["relu", "linear"])
@pytest.mark.parametrize("case", [DECONV_CASES[1], DECONV_CASES[2], DECONV_CASES[3], DECONV_CASES[4], DECONV_CASES[6]], ids=lambda c: "x".join(str(v) for v in c))
def test_deconv_equals_conv3x3_sp_on_the_zero_stuffed_map(case, relu):
    """The transposed convolution IS the 3 x 3 convolution of the zero-stuffed map (zeros interleaved, the convolution's own padding as the row and column at the
    end) with the 180-degree-flipped kernel.  Added zeros do not change an fp32 sum and the kernel meets the non-zero taps of every class in ``conv3x3_sp``'s
    order (intervals ascending, taps in the flipped kernel's order, whole tiles: policy ``geometry + 100000``), so the two agree bit for bit."""
    N, Ci, Co, h, w = case
    xs, wt, b, image, pre, x22 = _deconv_case(case)
    z = torch.zeros((N, Ci, 2 * h, 2 * w), device=DEV)
    z[:, :, ::2, ::2] = x22
    flipped = wt.permute(1, 0, 2, 3).flip(2, 3).contiguous()                  # [Co, Ci, 3, 3]
    want = ops.conv3x3_sp(ops.SplitMap.pack(z), ops.pack_conv3x3_emu_weight(flipped, 16, True), b, Co, None, relu, out_split=True, geometry=100000)
    got = ops.deconv3x3_s2_sp(xs, image, b, Co, relu=relu)
    assert torch.equal(got.dense(), want.dense()) and torch.equal(got.data, want.data)


# ---- ssfa_blend -------------------------------------------------------------------------------------------------------------------------------------------------
BLEND_CASES = [(2, 16, 1, 1), (2, 128, 3, 5), (1, 128, 16, 32)]


def _blend_inputs(case, seed=0):
    N, C, H, W = case
    g = torch.Generator(device=DEV).manual_seed(sum(case) + seed)
    a = torch.randn((N, H, W, C), generator=g, device=DEV).permute(0, 3, 1, 2)
    b = (torch.randn((N, H, W, C), generator=g, device=DEV) * 2 + 0.5).permute(0, 3, 1, 2)
    wa, wb = torch.randn(C, generator=g, device=DEV) / C ** 0.5, torch.randn(C, generator=g, device=DEV) / C ** 0.5
    return a, b, wa, wb


@pytest.mark.parametrize("case", BLEND_CASES, ids=lambda c: "x".join(str(v) for v in c))
def test_blend_against_float64_and_pack(case):
    """Both outputs, and each alone, into NaN-poisoned buffers: per element within ``assert_elementwise``'s defaults of the float64 blend; the SplitMap holds
    ``SplitMap.pack`` of the float32 output bit for bit; whichever outputs are asked for, the bits are the same."""
    N, C, H, W = case
    a, b, wa, wb = _blend_inputs(case)
    ref, p = blend_f64(a, b, wa, wb, 0.3, -0.2)
    ops.sp_range_exceeded(DEV)
    y, ysp = ops.ssfa_blend(a, b, wa, wb, 0.3, -0.2, out_split=True, out_nhwc=True)
    assert tuple(y.shape) == case and ops.nhwc_memory(y) and ysp.shape == case
    print(f"\nssfa_blend {case}: {assert_elementwise(y, ref, str(case)):.2e} of the scale")
    assert torch.equal(ysp.dense(), ops.SplitMap.pack(y).dense()) and torch.equal(ysp.data, ops.SplitMap.pack(y).data)
    assert torch.equal(ops.ssfa_blend(a, b, wa, wb, 0.3, -0.2, out_split=False, out_nhwc=True), y)
    assert torch.equal(ops.ssfa_blend(a, b, wa, wb, 0.3, -0.2, out_split=True, out_nhwc=False).data, ysp.data)
    assert torch.equal(ops.ssfa_blend(a.contiguous(), b.contiguous(), wa, wb, 0.3, -0.2), y)                     # NCHW inputs: converted first, same bits
    assert not ops.sp_range_exceeded(DEV)
    L = hip.lib()
    for want_y, want_sp in ((True, True), (True, False), (False, True)):
        py, psp = torch.full_like(y, float("nan")), torch.full_like(ysp.data, float("nan"))
        hip.check(L.coalign_ssfa_blend(a.data_ptr(), b.data_ptr(), wa.data_ptr(), wb.data_ptr(), 0.3, -0.2, py.data_ptr() if want_y else None,
                                       psp.data_ptr() if want_sp else None, N, C, H, W, None, None), "coalign_ssfa_blend")
        torch.cuda.synchronize()
        assert (torch.equal(py, y) if want_y else bool(torch.isnan(py).all())) and (torch.equal(psp, ysp.data) if want_sp else bool(torch.isnan(psp).all()))


@pytest.mark.parametrize("case", BLEND_CASES, ids=lambda c: "x".join(str(v) for v in c))
def test_blend_equal_and_saturated_logits(case):
    """Equal logits give p = 0.5; a logit difference of +-200 gives p = 1 or p = 0 exactly -- the output equals ``a`` or ``b`` (to 1 ulp) and no NaN appears."""
    a, b, wa, wb = _blend_inputs(case, seed=1)
    zero = torch.zeros_like(wa)
    assert torch.equal(ops.ssfa_blend(a, b, zero, zero, 1.5, 1.5), a * 0.5 + b * 0.5)
    assert torch.equal(ops.ssfa_blend(a, a, wa, wa, 0.0, 0.0), a * 0.5 + a * 0.5)
    for ba, bb, want in ((200.0, 0.0, a), (0.0, 200.0, b), (100.0, -100.0, a), (-100.0, 100.0, b)):
        y, ysp = ops.ssfa_blend(a, b, zero, zero, ba, bb, out_split=True, out_nhwc=True)
        assert bool(torch.isfinite(y).all()) and bool(torch.isfinite(ysp.data).all())
        ulp = torch.abs(torch.nextafter(want, torch.full_like(want, float("inf"))) - want)
        assert bool(((y - want).abs() <= ulp).all())
    big = wa.sign() * 1e4                                         # logits of the order of 1e6: still finite, still no NaN
    y = ops.ssfa_blend(a, b, big, -big, 0.0, 0.0)
    assert bool(torch.isfinite(y).all())


def test_blend_range_word_and_shape_errors():
    a = torch.full((1, 16, 1, 1), 70000.0, device=DEV)
    w = torch.zeros(16, device=DEV)
    ops.sp_range_exceeded(DEV)
    assert float(ops.ssfa_blend(a, a, w, w, 0.0, 0.0).max()) == 70000.0 and not ops.sp_range_exceeded(DEV)          # (a float32 output alone has no range)
    ysp = ops.ssfa_blend(a, a, w, w, 0.0, 0.0, out_split=True, out_nhwc=False)
    assert bool(torch.isfinite(ysp.data).all()) and ops.sp_range_exceeded(DEV)
    for args in ((a, a[:, :8], w, w), (a, torch.zeros((1, 16, 1, 2), device=DEV), w, w), (a, a, w[:8], w)):
        with pytest.raises(ValueError):
            ops.ssfa_blend(*args, 0.0, 0.0)


# ---- the module against its own float64 forward ---------------------------------------------------------------------------------------------------------------
KERNEL_OF = {"conv3x3_sp": "conv3x3_sp", "conv3x3_sp_s2": "conv3x3_sp_s2", "pointwise": "pointwise_conv", "deconv3x3_s2_sp": "deconv3x3_s2_sp", "ssfa_blend": "ssfa_blend"}


def _launches(fn):
    """{kernel: launches} of ``fn()``, recorded through ``ops.PROFILE``."""
    ops.PROFILE = {}
    try:
        with torch.no_grad():
            out = fn()
        torch.cuda.synchronize()
        return out, {k: len(v) for k, v in ops.PROFILE.items()}
    finally:
        ops.PROFILE = None


def _planned(lines):
    want = {}
    for text in lines.values():
        word = text.split(" ")[0]
        if word in KERNEL_OF:
            want[KERNEL_OF[word]] = want.get(KERNEL_OF[word], 0) + 1
        elif word == "heads_sp":
            want["heads_sp"] = 1                                      # (one launch for all the heads)
    return want


@pytest.mark.parametrize("shape", [(2, 128, 16, 32), (1, 128, 6, 10)], ids=lambda s: "x".join(str(v) for v in s))
def test_ssfa_kernel_route_against_its_own_float64_forward(shape):
    """``second.SSFA`` with non-default BatchNorm statistics: the kernel route against the module's own float64 forward (every convolution tap by tap) with
    ``assert_elementwise``, the torch route's error printed beside it; the kernels that ran, recorded through ``ops.PROFILE``, are the ones ``plan()`` names."""
    m = fill_by_formula_(second.SSFA({"feature_num": 128})).eval().to(DEV)
    g = torch.Generator(device=DEV).manual_seed(sum(shape))
    x = torch.randn((shape[0], shape[2], shape[3], shape[1]), generator=g, device=DEV).permute(0, 3, 1, 2)
    ref = ssfa_f64(m, x)
    m.neck_kernels = False
    with torch.no_grad():
        off = m(x)
    m.neck_kernels = True
    assert m.kernel_shape_reason(x) is None and m.kernel_route(x)
    ops.sp_range_exceeded(DEV)
    on, ran = _launches(lambda: m(x))
    assert ran == _planned(m.plan()) == {"conv3x3_sp": 7, "conv3x3_sp_s2": 1, "pointwise_conv": 2, "deconv3x3_s2_sp": 2, "ssfa_blend": 1}, ran
    assert tuple(on.shape) == shape and ops.nhwc_memory(on)
    e_off = float((off.double() - ref).abs().max() / ref.abs().max())
    e_on = assert_elementwise(on, ref, f"SSFA {shape}")
    print(f"\nSSFA {shape}: kernel route {e_on:.2e}, torch route {e_off:.2e} of the scale")
    y, ysp = m.forward_kernels(x, out_split=True, out_nhwc=True)
    assert torch.equal(y, on) and torch.equal(ysp.data, ops.SplitMap.pack(on).data)
    assert not ops.sp_range_exceeded(DEV)


# ---- the models -----------------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _mini(name):
    h = builtin_config("second/" + name)
    model = cases.seed_backbone_(build_model(h), 2).eval()
    fill_by_formula_(model.ssfa)
    model = model.to(DEV)
    vox = cases.voxels(model.spconv_block.sparse_shape, 2, seed=4)
    return h, model, to_device({"processed_lidar": vox, "record_len": torch.tensor([2])}, DEV)


@pytest.mark.parametrize("name", ["mini_second_uncertainty", "mini_second"])
def test_models_switch_on_against_switch_off(name):
    """Every head map of the kernel route (neck, shrink header and merged heads) against the torch route, which is the parent's code path, element-wise; the
    launches are the ones ``second.plan`` names."""
    h, model, data = _mini(name)
    try:
        model.ssfa.neck_kernels = False
        with torch.no_grad():
            off = model(data)
        model.ssfa.neck_kernels = True
        on, ran = _launches(lambda: model(data))
    finally:
        model.ssfa.neck_kernels = False
    assert list(on) == list(off)
    for k in on:
        assert tuple(on[k].shape) == tuple(off[k].shape), k
        print(f"\n{name} {k}: kernel route vs torch route {assert_elementwise(on[k], off[k], k):.2e} of the scale")
        assert not torch.equal(on[k], off[k])
    shrink = 2 if name.endswith("uncertainty") else 0
    for kernel, n in {"conv3x3_sp": 7 + shrink, "conv3x3_sp_s2": 1, "pointwise_conv": 2, "deconv3x3_s2_sp": 2, "ssfa_blend": 1, "heads_sp": 1}.items():
        assert ran.get(kernel) == n, (kernel, ran)


@pytest.mark.parametrize("name", ["mini_second_uncertainty", "mini_second"])
def test_models_replay_to_the_same_bits_under_a_captured_graph(name, monkeypatch):
    """Neck, shrink header and heads on the kernel route behind a static BEV map, warmed up and captured: a replay gives the eager bits, and new contents of the
    captured map give the eager bits of those."""
    h, model, data = _mini(name)
    with torch.no_grad():
        bev = model.bev_features(data).clone()
    monkeypatch.setattr(model, "bev_features", lambda data_dict: bev)
    monkeypatch.setattr(model.ssfa, "neck_kernels", True)
    with torch.no_grad():
        eager = {k: v.clone() for k, v in model({}).items()}
        stream = torch.cuda.Stream()
        stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(stream):
            model({})
        torch.cuda.current_stream().wait_stream(stream)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            out = model({})
        graph.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(out[k], eager[k]) for k in eager)
        bev.copy_(bev.flip(0).flip(3))
        graph.replay()
        torch.cuda.synchronize()
        again = model({})
        assert all(torch.equal(out[k], again[k]) for k in again) and not torch.equal(out["reg_preds"], eager["reg_preds"])


def test_outside_the_predicate_the_torch_route_is_taken():
    """Odd H and training mode are outside the predicate: with the switch on no kernel of the route runs and ``forward`` does what the switch-off call does (at
    an odd size both fail alike, as the reference does: the transposed map does not match x_trans_0)."""
    m = fill_by_formula_(second.SSFA({"feature_num": 128})).eval().to(DEV)
    for shape, word in (((1, 128, 7, 10), "7 x 10"), ((1, 128, 6, 9), "6 x 9")):
        x = torch.randn(shape, generator=torch.Generator().manual_seed(3)).to(DEV)
        m.neck_kernels = True
        assert word in m.kernel_shape_reason(x) and not m.kernel_route(x)
        outs = []
        for switch in (True, False):
            m.neck_kernels = switch
            try:
                (out, ran) = _launches(lambda: m(x))
                assert not ran
                outs.append(out)
            except RuntimeError as exc:
                outs.append(str(exc))
        assert outs[0] == outs[1] if isinstance(outs[1], str) else torch.equal(outs[0], outs[1])
    x = torch.randn((2, 128, 6, 10), generator=torch.Generator().manual_seed(4)).to(DEV)
    m.neck_kernels = True
    assert m.kernel_route(x)
    m.train()
    assert m.kernel_shape_reason(x) == "training mode" and not m.kernel_route(x)
    ops.PROFILE = {}
    try:
        a = m(x)
        assert not ops.PROFILE and a.requires_grad                          # no kernel of the route ran: the torch ops, with their graph
    finally:
        ops.PROFILE = None
    assert tuple(a.shape) == (2, 128, 6, 10) and a.is_contiguous()
