"""The camera model's BEV encoder on kernels, the part that needs no GPU: include/coalign_amd_lss_bev.h against the product library and ``hip.LSS_BEV_SIGNATURES``,
argument refusals before any HIP call, ``ops.pack_conv7x7_s2_weight`` against a restatement of the image from its documented layout, the route predicate of
``lss.BevEncodeMSFusion`` on both sides, the switch (off: today's forward, bit for bit) and ``plan()`` for the two shipped camera configs."""
import ctypes
import math
import os
import re

import pytest
import torch
import torch.nn.functional as F

import abi_headers
from coalign_amd import backbone, build, hip, lss, ops
from coalign_amd.config import builtin_config
from coalign_amd.detector import build_model
from coalign_amd.pose import normalize_pairwise_tfm
from coalign_amd.synthetic import fill_parameters_, make_camera_frame

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NULL, ONE = ctypes.c_void_p(0), ctypes.c_void_p(16)      # (a non-NULL, aligned token: none of these calls gets as far as touching memory)
HEADER = "coalign_amd_lss_bev.h"
NAMES = {"coalign_conv7x7_s2_weight_bytes", "coalign_conv7x7_s2_sp", "coalign_up2x_concat_sp"}
STEM_CITES = ("lss_submodule.py:19-38, 369-372, 402-404",)


# ---- the ABI --------------------------------------------------------------------------------------------------------------------------------------------------
def test_lss_bev_header_table_and_library_agree():
    """The header declares exactly ``NAMES``, the keys of ``hip.LSS_BEV_SIGNATURES`` (types, counts and exports: tests/test_abi_cpu.py); every declaration's comment
    cites the reference lines it replaces; build.py lists the source; the source reads no environment variable."""
    text = open(abi_headers.path(HEADER)).read()
    assert '#include "coalign_amd.h"' in text
    declared = abi_headers.declarations(HEADER)
    assert set(declared) == set(hip.LSS_BEV_SIGNATURES) == abi_headers.names(HEADER) == NAMES
    comments = re.findall(r"/\*.*?\*/", text, flags=re.S)
    cites = {"coalign_conv7x7_s2_weight_bytes": STEM_CITES, "coalign_conv7x7_s2_sp": STEM_CITES,
             "coalign_up2x_concat_sp": STEM_CITES + ("lss_submodule.py:23-24", "nn.Upsample(scale_factor=2, mode='bilinear', align_corners=True)")}
    for name in declared:
        last = [c for c in comments if c in text[:text.index(name + "(")]][-1]
        assert all(c in last for c in cites[name]), name
    assert '"lss_bev.hip"' in open(os.path.join(REPO, "coalign_amd", "build.py")).read() and "lss_bev.hip" in build.SOURCES
    assert int(re.search(r"#define COALIGN_CONV7X7_MAX_CIN (\d+)", text).group(1)) == ops.CONV7X7_MAX_CIN >= 256
    assert int(re.search(r"#define COALIGN_CONV7X7_COUT (\d+)", text).group(1)) == ops.CONV7X7_COUT == 64
    kernel = open(os.path.join(REPO, "coalign_amd", "csrc", "lss_bev.hip")).read()
    assert "getenv" not in kernel and "lab_env" not in kernel
    for k in ("conv7x7_s2_sp", "up2x_concat_sp"):
        assert re.search(r"__global__[^\n]*\bvoid " + k + r"\(", kernel), k


def test_entry_points_refuse_before_any_hip_call():
    L = hip.lib()
    assert [L.coalign_conv7x7_s2_weight_bytes(c) for c in (0, 8, 16, 24, 128, 512, 528)] == [0, 0, 16 * 12544 + 528, 0, 128 * 12544 + 528, 512 * 12544 + 528, 0]

    def stem(x=ONE, w=ONE, b=ONE, y=ONE, N=1, Cin=64, H=8, W=8, relu=1, flag=NULL):
        return L.coalign_conv7x7_s2_sp(x, w, b, y, N, Cin, H, W, relu, flag, NULL)

    def up(s=ONE, lo=ONE, y=ONE, N=1, Cs=64, Cl=256, h=4, w=4, flag=NULL):
        return L.coalign_up2x_concat_sp(s, lo, y, N, Cs, Cl, h, w, flag, NULL)

    assert stem(N=0) == 0 and up(N=0) == 0                                                       # (nothing to do: no launch)
    for kw in (dict(x=NULL), dict(w=NULL), dict(b=NULL), dict(y=NULL), dict(x=ctypes.c_void_p(24)), dict(b=ctypes.c_void_p(18)), dict(flag=ctypes.c_void_p(18))):
        assert stem(**kw) == -1, kw
    for kw in (dict(N=-1), dict(H=0), dict(W=0), dict(N=1 << 20, H=1 << 6, W=1 << 6)):
        assert stem(**kw) == -2, kw
    for kw in (dict(Cin=0), dict(Cin=8), dict(Cin=72), dict(Cin=ops.CONV7X7_MAX_CIN + 16), dict(relu=2)):
        assert stem(**kw) == -3, kw
    for kw in (dict(s=NULL), dict(lo=NULL), dict(y=NULL), dict(lo=ctypes.c_void_p(8)), dict(flag=ctypes.c_void_p(17))):
        assert up(**kw) == -1, kw
    for kw in (dict(N=-1), dict(h=0), dict(w=0), dict(N=1 << 11, h=1 << 9, w=1 << 9)):
        assert up(**kw) == -2, kw
    for kw in (dict(Cs=0), dict(Cs=24), dict(Cl=0), dict(Cl=8)):
        assert up(**kw) == -3, kw
    with pytest.raises(hip.CoalignHipError):
        ops.conv7x7_s2_sp(torch.zeros(1, 64, 8, 8), torch.zeros(16, dtype=torch.uint8), torch.zeros(64))
    with pytest.raises(hip.CoalignHipError):
        ops.up2x_concat_sp(torch.zeros(1, 16, 2, 2), torch.zeros(1, 16, 1, 1))


# ---- the weight image -------------------------------------------------------------------------------------------------------------------------------------------
def _round22_f64(x):
    """x (float64) rounded to 22 significant bits, ties away from zero -- in float64 arithmetic, not by the bit trick of the packer."""
    mag = x.abs()
    e = torch.floor(torch.log2(torch.where(mag > 0, mag, torch.ones_like(mag))))
    q = torch.pow(torch.full_like(mag, 2.0), e - 21)
    return torch.sign(x) * torch.floor(mag / q + 0.5) * q


@pytest.mark.parametrize("cin", [16, 64, 144])
def test_weight_image_against_its_documented_layout(cin):
    """[Cin / 16][7 ky][7 kx][2 terms][2 channel halves][64 cout][8 cin] fp16, 16 zero bytes, [64] 2^-k, [64] 2^k: every element from index arithmetic on the
    float64 restatement of the rounding; the pairs decode back to the 22-bit scaled weights EXACTLY; output channels on scales 2^-20 ... 2^6 and one all-zero."""
    g = torch.Generator().manual_seed(cin)
    cs = (2.0 ** torch.linspace(-20, 6, 64, dtype=torch.float64)).float()[torch.randperm(64, generator=g)]
    w = torch.randn((64, cin, 7, 7), generator=g) / (49 * cin) ** 0.5 * cs.view(-1, 1, 1, 1)
    w[3] = 0
    img = ops.pack_conv7x7_s2_weight(w)
    body = cin * 49 * 64 * 2 * 2
    assert img.dtype == torch.uint8 and img.numel() == body + 16 + 512 == hip.lib().coalign_conv7x7_s2_weight_bytes(cin)
    assert int(img[body:body + 16].max()) == 0
    inv, scale = img[body + 16:body + 272].view(torch.float32), img[body + 272:].view(torch.float32)
    amax = w.abs().reshape(64, -1).amax(1)
    for c in range(64):
        k = 0 if float(amax[c]) == 0 else 14 - math.frexp(float(amax[c]))[1]
        assert float(scale[c]) == 2.0 ** k and float(inv[c]) == 2.0 ** -k, c
        assert float(amax[c]) == 0 or 2.0 ** 13 <= float(amax[c]) * float(scale[c]) < 2.0 ** 14, c
    w22 = _round22_f64(w.double() * scale.double().view(-1, 1, 1, 1))                            # the 22-bit scaled weights, [cout, cin, ky, kx]
    pairs = img[:body].view(torch.float16).reshape(cin // 16, 7, 7, 2, 2, 64, 8)
    iv, ky, kx, hf, co, ci = torch.meshgrid(torch.arange(cin // 16), torch.arange(7), torch.arange(7), torch.arange(2), torch.arange(64), torch.arange(8), indexing="ij")
    want = w22[co, 16 * iv + 8 * hf + ci, ky, kx]                                                 # element [iv, ky, kx, half, cout, cin] of either term
    hi, lo = pairs[:, :, :, 0].double(), pairs[:, :, :, 1].double()
    assert torch.equal(hi + lo / 1024.0, want)                                                    # decodes back exactly
    assert torch.equal(hi, want.half().double())                                                  # term 0: the value to fp16, to nearest
    assert torch.equal(lo, (want - hi) * 1024.0)                                                  # term 1: the rest, scaled by 2^10
    assert float(pairs[:, :, :, :, :, 3].abs().max()) == 0 and float(want.abs().max()) < 2.0 ** 14
    for bad in (torch.zeros(64, 24, 7, 7), torch.zeros(32, 16, 7, 7), torch.zeros(64, 16, 3, 3), torch.zeros(64, ops.CONV7X7_MAX_CIN + 16, 7, 7)):
        with pytest.raises(ValueError):
            ops.pack_conv7x7_s2_weight(bad)


# ---- the route predicate, the switch and the plan -----------------------------------------------------------------------------------------------------------------
def _encoder(in_channels=64, method="att_ms"):
    torch.manual_seed(0)
    return lss.BevEncodeMSFusion({"core_method": method, "args": {"in_channels": in_channels, "voxel_size": [0.4, 0.4, 20.0]}})


def test_route_predicate_in_words(monkeypatch):
    assert lss.LSS_BEV is (os.environ.get("COALIGN_LSS_BEV", "0") != "0")
    m = _encoder().eval()
    assert m.bev_kernels is lss.LSS_BEV
    monkeypatch.setattr(lss, "LSS_BEV", True)
    assert _encoder().bev_kernels is True
    m.bev_kernels = True
    x = torch.zeros(2, 64, 16, 32)
    assert "float32 CUDA" in m.kernel_shape_reason(x) and not m.kernel_route(x)                   # a CPU tensor
    assert "16 x 20" in m.kernel_shape_reason(torch.zeros(2, 64, 16, 20)) and "multiples of 8" in m.kernel_shape_reason(torch.zeros(2, 64, 20, 16))
    assert "in_channels = 64" in m.kernel_shape_reason(torch.zeros(2, 32, 16, 32))
    m.train()
    assert m.kernel_shape_reason(x) == "training mode" and not m.kernel_route(x)
    m.eval()
    for bad in (40, 8, ops.CONV7X7_MAX_CIN + 16):
        assert "in_channels = %d outside" % bad in _encoder(bad).eval().kernel_shape_reason(torch.zeros(1, bad, 8, 8)), bad
    monkeypatch.setattr(backbone, "SPLIT_MAPS", False)
    assert "SplitMap arithmetic" in m.kernel_shape_reason(x)
    monkeypatch.setattr(backbone, "SPLIT_MAPS", True)
    monkeypatch.setattr(backbone, "FAST_INFERENCE", False)
    assert "off the SplitMap route" in m.kernel_shape_reason(x)


def _todays_forward(m, x, record_len, pairwise):
    """``BevEncodeMSFusion.forward`` as it stood before the kernel route existed, op for op."""
    _, _, H, W = x.shape
    affine = normalize_pairwise_tfm(pairwise, H, W, m.discrete_ratio, m.downsample_rate)

    def block(b, t):
        out = b.bn2(b.conv2(F.relu(b.bn1(b.conv1(t)))))
        return F.relu(out + (t if b.downsample is None else b.downsample(t)))

    def stage(layer, t):
        for b in layer:
            t = block(b, t)
        return t

    def up(u, lo, skip):
        return u.conv(torch.cat([skip, F.interpolate(lo, scale_factor=2, mode="bilinear", align_corners=True)], dim=1))

    t = F.relu(m.bn1(m.conv1(x)))
    x1 = stage(m.layer1, t)
    x2 = stage(m.layer2, x1)
    x3 = stage(m.layer3, x2)
    single = m.down_layer(up(m.up_layer1, up(m.up_layer2, x3, x2), x1))
    f1, f2, f3 = (lss._fuse_torch(v, record_len, affine, True) for v in (x1, x2, x3))
    return single, m.down_layer(up(m.up_layer1, up(m.up_layer2, f3, f2), f1))


@pytest.mark.parametrize("switch", [False, True])
def test_forward_off_the_kernel_route_is_todays(switch):
    """On the CPU, with the switch off and with it on (a CPU tensor is outside the predicate): outputs ``torch.equal`` to the op sequence of the module as it was,
    in eval and in training mode; state-dict names and seeded values do not depend on the switch."""
    h = builtin_config("camera/mini_lss_coalign")
    frame = make_camera_frame(h, 3, seed=7)
    m = _encoder()
    fill_parameters_(m, seed=3)
    m.bev_kernels = switch
    x = torch.randn(3, 64, 16, 32, generator=torch.Generator().manual_seed(1))
    for mode in ("eval", "train"):
        getattr(m, mode)()
        ref_m = _encoder()
        ref_m.load_state_dict(m.state_dict())
        getattr(ref_m, mode)()
        with torch.no_grad():
            got = m(x, [3], frame["pairwise_t_matrix"])
            want = _todays_forward(ref_m, x, [3], frame["pairwise_t_matrix"])
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]) and got[0].is_contiguous(), mode
    a, b = _encoder().state_dict(), _encoder().state_dict()
    assert list(a) == list(b) and all(torch.equal(a[k], b[k]) for k in a) and not any("stride" in k or "bev_kernels" in k for k in a)
    assert not isinstance(m.layer1[0], backbone.BasicBlock)                                      # (what walks a model for backbone.BasicBlock sees what it saw before)


@pytest.mark.parametrize("config,cin", [("camera/mini_lss_coalign", 64), ("camera/opv2v_lss_coalign", 128)])
def test_plan_of_the_shipped_camera_configs(config, cin):
    m = build_model(builtin_config(config)).eval().bevencode
    assert m.conv1.in_channels == cin
    m.bev_kernels = False
    off = m.plan()
    convs = [n for n, c in m.named_modules() if isinstance(c, torch.nn.Conv2d)]
    assert len(convs) == 1 + 12 + 2 + 4 + 2 and set(off) == set(convs) | {"up_layer1.up", "up_layer2.up", "fuse_module"}
    assert all(off[n] == f"{backbone.MIOPEN} ({m.SWITCHED_OFF})" for n in convs) and "torch bilinear" in off["up_layer1.up"]
    m.bev_kernels = True
    on = m.plan()
    assert set(on) == set(off) and on["conv1"] == m.STEM_KERNEL and on["up_layer1.up"] == on["up_layer2.up"] == m.UP_KERNEL
    assert "conv7x7_s2_sp" in m.STEM_KERNEL and "up2x_concat_sp" in m.UP_KERNEL
    sp = [n for n in convs if n != "conv1" and not n.endswith("downsample.0") and n not in ("layer2.0.conv1", "layer3.0.conv1")]
    assert len(sp) == 16 and all(on[n] == backbone.SP for n in sp)
    assert on["layer2.0.conv1"] == on["layer3.0.conv1"] == backbone.SP_S2 and "tenth tap of conv3x3_sp_s2" in on["layer2.0.downsample.0"]
    assert on["fuse_module"] == off["fuse_module"] and "warp_fuse" in on["fuse_module"]
    m.train()
    assert all(m.plan()[n] == f"{backbone.MIOPEN} (training mode)" for n in convs)
