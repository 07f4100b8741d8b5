"""The camera model's BEV encoder on kernels, on the GPU (csrc/lss_bev.hip): ``ops.conv7x7_s2_sp`` against the float64 convolution per output channel, its
layouts and range word; ``ops.up2x_concat_sp`` against ``SplitMap.pack`` (skip channels, bit for bit) and the float64 interpolation, into a poisoned buffer;
``lss.BevEncodeMSFusion`` on the kernel route against its own float64 forward with the kernels that ran recorded; the camera model with the switch on against
the switch off, under a captured graph, and outside the predicate."""
import copy

import pytest
import torch
import torch.nn.functional as F

from conftest import assert_elementwise
from coalign_amd import hip, lss, ops
from coalign_amd.config import builtin_config
from coalign_amd.detector import build_model, to_device
from coalign_amd.inference import inference_intermediate_fusion
from coalign_amd.postprocess import build_postprocessor
from coalign_amd.synthetic import fill_parameters_, make_camera_frame

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BOUND = 3e-6                     # of the channel's own scale: the sp16 bound of tests/test_sp_limits_gpu.py
SP_ABS = 2.0 ** -33              # what a SplitMap holds of a value below 2^-13
ZERO_CH = 3                      # the all-zero output channel of the mixed-scale stem
UP_BOUND = 2.0 ** -21            # of the channel's scale: the pair rounding (2^-23) plus three float32 roundings


# ---- helpers (mixed_layer, channel_error, _round11: copied from tests/test_sp_limits_gpu.py) ------------------------------------------------------------------
def mixed_layer(g, Co, Ci, k, lo=-20, hi=6):
    """Weights whose output channels sit on scales 2^lo ... 2^hi, randomly permuted (one of them all zero), and a bias on the same per-channel scale."""
    cs = (2.0 ** torch.linspace(lo, hi, Co, device=DEV, dtype=torch.float64)).float()[torch.randperm(Co, generator=g, device=DEV)]
    w = torch.randn((Co, Ci, k, k), generator=g, device=DEV) / (k * k * Ci) ** 0.5 * cs.view(-1, 1, 1, 1)
    w[ZERO_CH] = 0
    return w, torch.randn(Co, generator=g, device=DEV) * cs


def channel_error(got, ref, pre, floor=0.0):
    """max over channels of (max |got - ref| - ``floor``) / the channel's scale (max |pre-activation|); ``floor`` = 2^-33 for a SplitMap, which holds values
    below 2^-13 to that absolute precision only (without it the channels on scale 2^-20 report 1e-4 for an error of 1e-10)."""
    scale = pre.abs().amax(dim=(0, 2, 3))
    err = ((got.double() - ref).abs().amax(dim=(0, 2, 3)) - floor).clamp_min(0.0)
    return float(torch.where(scale > 0, err / scale.clamp_min(1e-300), err).max())


def assert_channels_close(got, ref, what, pre, bound=BOUND):
    """Every output channel within ``bound`` of its own scale (max |pre-activation| of the channel) + 2^-33, as an element-wise bound."""
    scale = pre.abs().amax(dim=(0, 2, 3), keepdim=True)
    bad = (got.double() - ref).abs() > bound * scale + SP_ABS
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} elements outside {bound:g} of their channel's scale; worst {channel_error(got, ref, pre, SP_ABS):.3e}"
    return channel_error(got, ref, pre, SP_ABS)


def _round11(x):
    return ((x.contiguous().view(torch.int32) + (1 << 12)) & -(1 << 13)).view(torch.float32)


def conv7_f64(x, w, b):
    """conv7x7(x, w, stride 2, pad 3) + b in float64, tap by tap (49 float64 matrix products)."""
    N, Ci, H, W = x.shape
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    xp = F.pad(x.double(), (3, 3, 3, 3))
    out = torch.zeros((N, w.shape[0], Ho, Wo), dtype=torch.float64, device=x.device)
    for ky in range(7):
        for kx in range(7):
            out += torch.einsum("oc,nchw->nohw", w.double()[:, :, ky, kx], xp[:, :, ky:ky + 2 * Ho - 1:2, kx:kx + 2 * Wo - 1:2])
    return out + b.double().view(1, -1, 1, 1)


# (N, Cin, H, W): centre tap only | smallest even map | odd sizes | smallest map the route accepts | the mini config | outputs no tile edge divides |
# straddles tile edges | one full-size map (K = 6272) | two and three channel intervals (the one patch buffer restaged once and twice) | above the model's channel
# counts, up to the entry's limit (K = 12 544 and 25 088)
STEM_CASES = [(3, 16, 1, 1), (2, 64, 2, 2), (2, 64, 7, 9), (1, 128, 8, 8), (5, 64, 16, 32), (2, 128, 40, 24), (1, 64, 66, 130), (1, 128, 240, 240),
              (1, 32, 9, 9), (1, 48, 16, 16), (1, 256, 8, 8), (1, 512, 8, 8)]
_STEM = {}


def _stem_case(case):
    """Inputs and the float64 pre-activation of a case, computed once and shared by its tests (never modified)."""
    if case not in _STEM:
        N, Ci, H, W = case
        g = torch.Generator(device=DEV).manual_seed(N + Ci + H + W)
        x = torch.randn((N, Ci, H, W), generator=g, device=DEV).contiguous(memory_format=torch.channels_last)
        w, b = mixed_layer(g, 64, Ci, 7)
        x22 = ops.SplitMap.pack(x).dense()                          # the 22-bit values the kernel reads
        _STEM[case] = (x, w, b, ops.pack_conv7x7_s2_weight(w), conv7_f64(x22, w, b), x22)
    return _STEM[case]


@pytest.mark.parametrize("relu", [True, False], ids=["relu", "linear"])
@pytest.mark.parametrize("case", STEM_CASES, ids=lambda c: "x".join(str(v) for v in c))
def test_stem_mixed_channel_scales_against_float64(case, relu):
    """Every output channel of ``conv7x7_s2_sp`` within 3e-6 of its own scale + 2^-33 of the float64 convolution of the 22-bit inputs with the unrounded
    weights, output channels on scales 2^-20 ... 2^6; the all-zero channel is exactly act(bias) as a SplitMap holds it; float32 ``F.conv2d``'s error on the same
    inputs is printed beside the kernel's.  Above Cin = 128 (K beyond 6 272, where the 3e-6 had been measured) the bound is the larger of 3e-6 and TWICE the
    library's own worst-channel error on the same inputs: both accumulate in fp32, the sp16 pair holds 22 operand bits where float32 holds 24."""
    N, Ci, H, W = case
    x, w, b, image, pre, x22 = _stem_case(case)
    ref = torch.relu(pre) if relu else pre
    ops.sp_range_exceeded(DEV)
    y = ops.conv7x7_s2_sp(x, image, b, relu=relu)
    assert y.shape == (N, 64, (H - 1) // 2 + 1, (W - 1) // 2 + 1) and tuple(y.data.shape) == (N, 4, 4, y.shape[2], y.shape[3], 8)
    got = y.dense()
    lib = F.conv2d(x22, w, b, stride=2, padding=3)
    e_lib = channel_error(torch.relu(lib) if relu else lib, ref, pre)
    bound = BOUND if Ci <= 128 else max(BOUND, 2.0 * e_lib)
    print(f"\nconv7x7_s2_sp {case} {'relu' if relu else 'linear'}: K = {49 * Ci}, worst channel error beyond 2^-33 {channel_error(got, ref, pre, SP_ABS):.2e} of the channel scale "
          f"(bound {bound:g}); float32 F.conv2d {e_lib:.2e}")
    assert_channels_close(got, ref, case, pre, bound)
    zero = b[ZERO_CH].view(1, 1, 1, 1).expand(N, 16, y.shape[2], y.shape[3])
    assert torch.equal(got[:, ZERO_CH], ops.SplitMap.pack(torch.relu(zero) if relu else zero).dense()[:, 0]), case
    if not relu and H * W > 1:
        assert float(got.min()) < 0
    assert not ops.sp_range_exceeded(DEV)


def test_stem_layouts_give_equal_bits_and_repeat():
    case = STEM_CASES[5]
    x, w, b, image, pre, x22 = _stem_case(case)
    first = ops.conv7x7_s2_sp(x, image, b)
    nchw = x.contiguous()
    assert nchw.is_contiguous() and not ops.nhwc_memory(nchw) and ops.nhwc_memory(x)
    assert torch.equal(ops.conv7x7_s2_sp(nchw, image, b).data, first.data) and torch.equal(ops.conv7x7_s2_sp(x, image, b).data, first.data)
    with pytest.raises(ValueError):
        ops.conv7x7_s2_sp(x[:, :24], image, b)
    with pytest.raises(ValueError):
        ops.conv7x7_s2_sp(x, image[:-16], b)


def test_the_channel_bound_separates_the_split_from_a_kernel_that_drops_the_low_term():
    """The per-channel bound can fail: the float64 convolution of the operands rounded to 11 bits -- a kernel that kept only the high fp16 term -- is refused, at
    a shape where the kernel itself passes."""
    case = STEM_CASES[4]
    x, w, b, image, pre, x22 = _stem_case(case)
    lossy = conv7_f64(_round11(x22), _round11(w), b).float()
    with pytest.raises(AssertionError):
        assert_channels_close(lossy, pre, "11-bit operands", pre)
    print(f"\n11-bit operands: worst channel error {channel_error(lossy, pre, pre, SP_ABS):.2e} of the channel scale (bound {BOUND:g})")
    assert_channels_close(ops.conv7x7_s2_sp(x, image, b, relu=False).dense(), pre, case, pre)


def test_stem_range_word():
    """Set by a value beyond 65504, clear otherwise."""
    g = torch.Generator(device=DEV).manual_seed(5)
    x = torch.randn((1, 16, 9, 9), generator=g, device=DEV)
    w = torch.randn((64, 16, 7, 7), generator=g, device=DEV) * 0.05
    b = torch.zeros(64, device=DEV)
    ops.sp_range_exceeded(DEV)
    y = ops.conv7x7_s2_sp(x, ops.pack_conv7x7_s2_weight(w), b, relu=False)
    assert float(y.dense().abs().max()) < 65504 and not ops.sp_range_exceeded(DEV)
    b[17] = 70000.0
    y = ops.conv7x7_s2_sp(x, ops.pack_conv7x7_s2_weight(w), b, relu=False)
    assert bool(torch.isfinite(y.data).all()) and ops.sp_range_exceeded(DEV) and not ops.sp_range_exceeded(DEV)


# ---- up2x_concat_sp -------------------------------------------------------------------------------------------------------------------------------------------
UP_CASES = [(1, 16, 16, 1, 1), (2, 64, 256, 1, 3), (3, 128, 256, 5, 3), (6, 128, 256, 15, 15), (2, 64, 256, 60, 60), (1, 128, 256, 33, 65)]


@pytest.mark.parametrize("case", UP_CASES, ids=lambda c: "x".join(str(v) for v in c))
def test_up2x_concat_against_pack_and_the_float64_interpolation(case):
    """The skip channels hold exactly what ``SplitMap.pack(skip)`` holds; the up-sampled channels are within 2^-21 of their channel's scale of
    ``F.interpolate(low.double(), scale_factor=2, mode='bilinear', align_corners=True)``; NCHW inputs give the same bits; every element of a NaN-poisoned
    output buffer is written."""
    N, Cs, Cl, h, w = case
    g = torch.Generator(device=DEV).manual_seed(sum(case))
    cl = torch.channels_last
    skip = (torch.randn((N, Cs, 2 * h, 2 * w), generator=g, device=DEV) * 3).contiguous(memory_format=cl)
    scales = 2.0 ** torch.randint(-6, 7, (Cl,), generator=g, device=DEV).float()
    low = (torch.randn((N, Cl, h, w), generator=g, device=DEV) * scales.view(1, -1, 1, 1)).contiguous(memory_format=cl)
    ops.sp_range_exceeded(DEV)
    y = ops.up2x_concat_sp(skip, low)
    assert y.shape == (N, Cs + Cl, 2 * h, 2 * w)
    assert torch.equal(y.data[:, :Cs // 16], ops.SplitMap.pack(skip).data)
    ref = F.interpolate(low.double(), scale_factor=2, mode="bilinear", align_corners=True)
    got = y.dense()[:, Cs:].double()
    scale = ref.abs().amax(dim=(0, 2, 3), keepdim=True)
    err = (got - ref).abs()
    worst = float((err / scale).max())
    print(f"\nup2x_concat_sp {case}: worst {worst:.2e} of the channel scale (bound 2^-21 = {UP_BOUND:.2e})")
    assert not bool((err > UP_BOUND * scale).any()), worst
    assert torch.equal(ops.up2x_concat_sp(skip.contiguous(), low.contiguous()).data, y.data)
    assert not ops.sp_range_exceeded(DEV)
    poisoned = torch.full_like(y.data, float("nan"))
    hip.check(hip.lib().coalign_up2x_concat_sp(skip.data_ptr(), low.data_ptr(), poisoned.data_ptr(), N, Cs, Cl, h, w, None, None), "coalign_up2x_concat_sp")
    torch.cuda.synchronize()
    assert not bool(torch.isnan(poisoned).any()) and torch.equal(poisoned, y.data)


def test_up2x_range_word_and_shape_errors():
    skip = torch.zeros((1, 16, 2, 2), device=DEV)
    low = torch.full((1, 16, 1, 1), 70000.0, device=DEV)
    ops.sp_range_exceeded(DEV)
    y = ops.up2x_concat_sp(skip, low)
    assert bool(torch.isfinite(y.data).all()) and ops.sp_range_exceeded(DEV)
    for s, lo in ((torch.zeros((1, 16, 2, 3), device=DEV), low), (torch.zeros((2, 16, 2, 2), device=DEV), low), (torch.zeros((1, 8, 2, 2), device=DEV), low)):
        with pytest.raises(ValueError):
            ops.up2x_concat_sp(s, lo)


# ---- the module against its own float64 forward ---------------------------------------------------------------------------------------------------------------
def _encoder(C, seed):
    m = lss.BevEncodeMSFusion({"core_method": "att_ms", "args": {"in_channels": C, "voxel_size": [0.4, 0.4, 20.0]}})
    fill_parameters_(m, seed=seed)
    return m


def _pairwise(agents, seed):
    import numpy as np
    from coalign_amd.pose import get_pairwise_transformation
    from coalign_amd.synthetic import make_poses
    poses = make_poses(np.random.RandomState(seed), agents, spread_xy=(2.0, 1.0), spread_yaw=20.0)
    return torch.from_numpy(np.stack([get_pairwise_transformation(poses, 5)]))


class _Spy:
    """Counts the calls of the two new ops and records every ``F.conv2d`` kernel size while active."""

    def __init__(self, monkeypatch):
        self.calls, self.conv2d = {"conv7x7_s2_sp": 0, "up2x_concat_sp": 0, "conv3x3_sp": 0, "conv3x3_sp_s2": 0}, []
        for name in self.calls:
            monkeypatch.setattr(ops, name, self._count(name, getattr(ops, name)))
        real = F.conv2d

        def conv2d(x, w, *a, **kw):
            self.conv2d.append(tuple(w.shape[2:]))
            return real(x, w, *a, **kw)
        monkeypatch.setattr(F, "conv2d", conv2d)
        monkeypatch.setattr(torch.nn.functional, "conv2d", conv2d)

    def _count(self, name, fn):
        def wrapped(*a, **kw):
            self.calls[name] += 1
            return fn(*a, **kw)
        return wrapped


MODULE_CASES = [(64, 8, 8, 1), (64, 16, 32, 3), (128, 40, 24, 2), (64, 8, 24, 5)]


@pytest.mark.parametrize("C,H,W,agents", MODULE_CASES, ids=lambda v: str(v))
def test_encoder_kernel_route_against_its_own_float64_forward(C, H, W, agents, monkeypatch):
    """``BevEncodeMSFusion`` with non-default BatchNorm statistics and non-identity poses: both outputs of the kernel route against the module's own float64
    forward (CPU, the reference's op sequence) with ``assert_elementwise``; the torch route's error is printed beside it (the ratio is recorded, not asserted); a spy
    asserts which kernels ran."""
    m = _encoder(C, seed=C + H).eval()
    x = torch.randn((agents, C, H, W), generator=torch.Generator().manual_seed(H * W + agents))
    pair = _pairwise(agents, seed=agents)
    assert float((pair[0, 0, 1] - torch.eye(4, dtype=pair.dtype)).abs().max()) > 0 or agents == 1
    with torch.no_grad():
        ref = copy.deepcopy(m).double()(x.double(), [agents], pair)
    md = m.to(DEV)
    xd = x.to(DEV).contiguous(memory_format=torch.channels_last)
    md.bev_kernels = False
    with torch.no_grad():
        off = md(xd, [agents], pair.to(DEV))
    md.bev_kernels = True
    assert md.kernel_shape_reason(xd) is None and md.kernel_route(xd)
    spy = _Spy(monkeypatch)
    with torch.no_grad():
        on = md(xd, [agents], pair.to(DEV))
    assert spy.calls["conv7x7_s2_sp"] == 1 and spy.calls["up2x_concat_sp"] == 2 and spy.calls["conv3x3_sp_s2"] == 2 and spy.calls["conv3x3_sp"] == 10 + 6
    assert spy.conv2d == [], spy.conv2d
    for name, a, b, r in (("x_single", on[0], off[0], ref[0]), ("x_fuse", on[1], off[1], ref[1])):
        assert tuple(a.shape) == tuple(r.shape) == ((agents if name == "x_single" else 1), 128, H // 2, W // 2)
        e_off = float((b.double().cpu() - r).abs().max() / r.abs().max())
        e_on = assert_elementwise(a, r, f"{name} {C, H, W, agents}")
        print(f"\n{name} {C, H, W, agents}: kernel route {e_on:.2e}, torch route {e_off:.2e} of the scale, ratio {e_on / max(e_off, 1e-30):.2f}")
    assert not ops.sp_range_exceeded(DEV)


# ---- the model, graph replay and the predicate ----------------------------------------------------------------------------------------------------------------
def _model(agents=2):
    h = builtin_config("camera/mini_lss_coalign")
    model = build_model(h)
    fill_parameters_(model, seed=1)
    return h, model.to(DEV).eval(), to_device(make_camera_frame(h, agents, seed=5), DEV)


def test_camera_model_switch_on_against_switch_off():
    """``camera/mini_lss_coalign``, 2 agents: every head of the kernel route against the torch route (the parent's code path), element-wise; boxes out of
    ``inference_intermediate_fusion``."""
    h, model, frame = _model()
    enc = model.bevencode
    assert enc.bev_kernels is lss.LSS_BEV
    with torch.no_grad():
        enc.bev_kernels = False
        off = model(frame)
        enc.bev_kernels = True
        on = model(frame)
    assert list(on.keys()) == list(off.keys())
    for k in on:
        if k != "depth_items":
            print(f"\n{k}: BEV kernels vs torch route {assert_elementwise(on[k], off[k], k):.2e} of the scale")
            assert not torch.equal(on[k], off[k])
    post = build_postprocessor(h["postprocess"], False)
    with torch.no_grad():
        model.cls_head.bias.add_(3.0)
    batch = {"ego": dict(frame, transformation_matrix=torch.eye(4, device=DEV), anchor_box=torch.from_numpy(post.generate_anchor_box()).to(DEV))}
    res = inference_intermediate_fusion(batch, model, post)
    assert res["pred_box_tensor"] is not None and res["pred_box_tensor"].shape[1:] == (8, 3) and len(res["pred_score"]) == len(res["pred_box_tensor"]) > 0


def test_warmed_up_forward_replays_to_the_same_bits_under_a_captured_graph():
    """The encoder's kernel route, warmed up (weight images and the stream's workspace exist), captured with the default queue settings: a replay gives the
    eager bits, and new inputs in the captured buffers give the eager bits of those."""
    h, model, frame = _model(3)
    enc = model.bevencode
    enc.bev_kernels = True
    with torch.no_grad():
        x = model.get_voxels(frame["image_inputs"]).clone()
        pair = frame["pairwise_t_matrix"]
        eager = [t.clone() for t in enc(x, [3], pair)]
        stream = torch.cuda.Stream()
        stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(stream):
            enc(x, [3], pair)                                       # warm-up on the capturing stream
        torch.cuda.current_stream().wait_stream(stream)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            out = enc(x, [3], pair)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out[0], eager[0]) and torch.equal(out[1], eager[1])
        x.copy_(x.flip(0))
        graph.replay()
        torch.cuda.synchronize()
        again = enc(x, [3], pair)
        assert torch.equal(out[0], again[0]) and torch.equal(out[1], again[1]) and not torch.equal(out[1], eager[1])


def test_a_map_outside_the_predicate_takes_the_torch_route():
    """H = 20 is no multiple of 8, so the map is outside the predicate: with the switch on, ``forward`` is the torch route and does what the switch-off call does,
    bit for bit.  (At H = 20 the three scales are 10, 5 and 3 rows and ``Up`` cannot concatenate 2 * 3 rows to 5, in the reference as here: what both calls give
    is then the same error; the comparison covers either outcome.)  No kernel of the route runs."""
    m = _encoder(64, seed=2).to(DEV).eval()
    pair = _pairwise(2, seed=2).to(DEV)
    for shape, words in (((2, 64, 20, 16), "20 x 16"), ((2, 64, 16, 20), "16 x 20")):
        x = torch.randn(shape, generator=torch.Generator().manual_seed(3)).to(DEV)
        m.bev_kernels = True
        assert words in m.kernel_shape_reason(x) and not m.kernel_route(x)
        outs = []
        for switch in (True, False):
            m.bev_kernels = switch
            try:
                with torch.no_grad():
                    outs.append(m(x, [2], pair))
            except RuntimeError as exc:
                outs.append(str(exc))
        if isinstance(outs[1], str):
            assert outs[0] == outs[1]
        else:
            assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    x = torch.randn((2, 64, 24, 16), generator=torch.Generator().manual_seed(3)).to(DEV)          # the neighbouring size inside the predicate
    m.bev_kernels = True
    assert m.kernel_route(x)
    with torch.no_grad():
        on = m(x, [2], pair)
        m.bev_kernels = False
        off = m(x, [2], pair)
    assert not torch.equal(on[1], off[1])
    assert_elementwise(on[1], off[1], "24 x 16")
