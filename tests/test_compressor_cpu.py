"""NaiveCompressor on the SplitMap kernels, the part that needs no GPU: the extension header against the binding table and the library, the narrow
convolution's argument checks (all before any HIP call), its weight image, and ``routes.plan`` with ``compression`` in the config.

``coalign_conv3x3_sp_narrow`` (include/coalign_amd_narrow.h) is the 3x3 / stride 1 convolution with 16 or 32 output channels that writes a SplitMap: the
encoder of opencood/models/sub_modules/naive_compress.py:5-31.  ``backbone.narrow_channels_ok`` is the one statement of its limits.
"""
import copy
import ctypes
import os
import re

import pytest
import torch
import torch.nn as nn

from coalign_amd import backbone as bb
from coalign_amd import hip, ops
from coalign_amd.config import builtin_config
from coalign_amd.detector import build_model
from coalign_amd.routes import NARROW, SP, plan

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NULL, ONE = ctypes.c_void_p(0), ctypes.c_void_p(16)      # (a non-NULL, 16-byte aligned token: none of the calls below gets as far as touching memory)
HW = 8


def _declared(header):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", header)).read(), flags=re.S)
    return set(re.findall(r"\b(coalign_[a-z0-9_]+)\s*\(", text))


def _narrow(cin, cout, n=0, x=ONE, kind=0, w=ONE, bias=ONE, y=ONE, h=HW, wd=HW):
    return hip.lib().coalign_conv3x3_sp_narrow(x, kind, w, bias, y, n, cin, cout, h, wd, 1, NULL, NULL)


def test_extension_header_table_and_library_agree():
    """Every name of include/coalign_amd_narrow.h is exported by the product library and mirrored in ``hip.NARROW_SIGNATURES``; the frozen header keeps its
    68 names, and each declaration of the extension cites the reference module it replaces."""
    declared = _declared("coalign_amd_narrow.h")
    assert declared == set(hip.NARROW_SIGNATURES) and len(declared) == 2
    lib = hip.lib()
    for name in declared:
        fn = getattr(lib, name)
        assert fn.restype is hip.NARROW_SIGNATURES[name][0] and list(fn.argtypes) == hip.NARROW_SIGNATURES[name][1], name
    assert len(_declared("coalign_amd.h")) == 68 and not (declared & set(hip.SIGNATURES))
    assert lib.coalign_abi_version() == 2
    text = open(os.path.join(REPO, "include", "coalign_amd_narrow.h")).read()
    assert '#include "coalign_amd.h"' in text
    comments = re.findall(r"/\*.*?\*/", text, flags=re.S)
    for name in declared:                                  # the comment in front of each declaration names naive_compress.py:5-31
        before = text[:text.index(name + "(")]
        last = [c for c in comments if c in before][-1]
        assert "opencood/models/sub_modules/naive_compress.py:5-31" in last, name


def test_narrow_argument_validation_without_a_gpu():
    """NULL pointers -1, negative sizes -2, Cin % 16 / Cout outside {16, 32} / unknown in_kind / misaligned pointers -3, N = 0 returns 0: all before any HIP call."""
    assert _narrow(64, 16) == 0 and _narrow(64, 32) == 0 and _narrow(16, 16, kind=1) == 0             # N = 0: validated, nothing launched
    for arg in ("x", "w", "bias", "y"):
        assert _narrow(64, 16, n=1, **{arg: NULL}) == -1, arg
    assert _narrow(64, 16, n=-1) == -2 and _narrow(64, 16, h=0) == -2 and _narrow(64, 16, wd=-3) == -2 and _narrow(-16, 16) == -2 and _narrow(64, 0) == -2
    assert _narrow(24, 16) == -3 and _narrow(8, 16) == -3
    for cout in (8, 24, 48, 64, 128):
        assert _narrow(64, cout) == -3, cout
    assert _narrow(64, 16, kind=2) == -3 and _narrow(64, 16, kind=-1) == -3
    for arg in ("x", "w", "y"):
        assert _narrow(64, 16, **{arg: ctypes.c_void_p(24)}) == -3, arg                                # 16-byte alignment
    assert _narrow(64, 16, bias=ctypes.c_void_p(18)) == -3
    assert _narrow(64, 32, n=1 << 20, h=1 << 10, wd=1 << 10) == -3                                     # group offsets are 32-bit
    size = hip.lib().coalign_conv3x3_narrow_weight_bytes
    assert size(64, 16) == 64 * 16 * 36 + 16 + 16 * 8 and size(64, 32) == 64 * 32 * 36 + 16 + 32 * 8 <= 74 * 1024
    assert size(24, 16) == 0 and size(64, 64) == 0 and size(64, 8) == 0 and size(0, 16) == 0 and size(-16, 16) == 0


def test_narrow_predicate_equals_the_kernels_checks():
    """``backbone.narrow_channels_ok`` says yes exactly where the entry point (and the weight size function) accepts the pair; the 64-channel kernel's own
    limits are not widened."""
    for cin in (8, 16, 24, 64, 256):
        for cout in (8, 16, 24, 32, 48, 64):
            ok = bb.narrow_channels_ok(cin, cout)
            assert ok == (_narrow(cin, cout) == 0) == (hip.lib().coalign_conv3x3_narrow_weight_bytes(cin, cout) > 0), (cin, cout)
    assert not bb.sp_channels_ok(64, 32) and not bb.sp_channels_ok(64, 16)
    assert hip.lib().coalign_conv3x3_sp(ONE, ONE, ONE, NULL, 0, ONE, ops.SP_OUT_SP, 0, 64, 32, HW, HW, 1, 0, NULL, NULL, 0, NULL) == -3


@pytest.mark.parametrize("co,ci", [(16, 64), (32, 64), (32, 16), (16, 256)])
def test_narrow_weight_image_layout_and_values(co, ci):
    """``ops.pack_conv3x3_narrow_weight``: [Cin / 16][9 taps][2 terms][2 channel halves][Cout][8 cin] fp16 sp16 pairs of the per-output-channel scaled weights, 16
    zero bytes, [Cout] 2^-k_c, [Cout] 2^k_c: the two terms summed and the scale undone give the weights rounded to 22 significant bits, and the pairs are those
    of the 64-channel tap-major image of the same weights zero-padded to 64 output channels."""
    torch.manual_seed(co + ci)
    w = torch.randn(co, ci, 3, 3) * torch.logspace(-6, 2, co).reshape(co, 1, 1, 1)       # channel scales 2^-20 ... 2^6
    w[3] = 0.0                                                                            # a dead channel (a zero-padded mid channel)
    img = ops.pack_conv3x3_narrow_weight(w)
    n = co * ci * 36
    assert img.dtype == torch.uint8 and img.numel() == hip.lib().coalign_conv3x3_narrow_weight_bytes(ci, co) == n + 16 + co * 8
    body = img[:n].view(torch.float16).reshape(ci // 16, 9, 2, 2, co, 8).float()
    assert int(img[n:n + 16].sum()) == 0
    inv, scale = img[n + 16:n + 16 + co * 4].view(torch.float32), img[n + 16 + co * 4:].view(torch.float32)
    assert torch.equal(inv * scale, torch.ones(co)) and bool((torch.frexp(scale)[0] == 0.5).all())          # exact powers of two
    val = body[:, :, 0] + body[:, :, 1] / 1024.0                                          # [interval, tap, half, cout, cin]
    got = val.permute(3, 0, 2, 4, 1).reshape(co, ci, 3, 3) * inv.reshape(co, 1, 1, 1)     # channel = 16 * interval + 8 * half + cin
    ws = w * scale.reshape(co, 1, 1, 1)
    want = ((ws.contiguous().view(torch.int32) + 2) & -4).view(torch.float32) * inv.reshape(co, 1, 1, 1)
    assert torch.equal(got, want)
    amax = (w.abs() * scale.reshape(co, 1, 1, 1)).reshape(co, -1).amax(dim=1)
    live = w.abs().reshape(co, -1).amax(dim=1) > 0
    assert bool(((amax[live] >= 2.0 ** 13) & (amax[live] < 2.0 ** 14)).all()) and float(scale[3]) == 1.0
    w64 = torch.zeros(64, ci, 3, 3)
    w64[:co] = w
    wide = ops.pack_conv3x3_emu_weight(w64, 16, tap_major=True)
    wide_body = wide[:64 * ci * 36].view(torch.float16).reshape(ci // 16, 9, 2, 2, 64, 8)
    assert torch.equal(wide_body[:, :, :, :, :co], img[:n].view(torch.float16).reshape(ci // 16, 9, 2, 2, co, 8))
    assert torch.equal(wide[64 * ci * 36 + 16:64 * ci * 36 + 16 + co * 4].view(torch.float32), inv)
    for bad in (torch.zeros(24, 64, 3, 3), torch.zeros(64, 64, 3, 3), torch.zeros(16, 24, 3, 3), torch.zeros(16, 64, 1, 1)):
        with pytest.raises(ValueError):
            ops.pack_conv3x3_narrow_weight(bad)


def _with_compression(cfg, ratio):
    h = copy.deepcopy(builtin_config(cfg))
    h["model"]["args"]["compression"] = ratio
    return h


@pytest.mark.parametrize("cfg", ["opv2v_coalign", "mini_coalign"])
@pytest.mark.parametrize("ratio", [1, 2, 4, 8])
def test_route_plan_of_the_compressor(cfg, ratio):
    """With ``compression`` in the config no layer is left on MIOpen and nothing is a fallback; ratios 2, 4, 8 put the encoder on the narrow kernel, ratio 1 all
    three layers on the 64-channel SplitMap kernel; and every kernel the plan names for a compressor layer accepts that layer's (padded) shape at its entry point."""
    h = _with_compression(cfg, ratio)
    p = plan(h)
    assert p["outside_hot_path"] is None and p["fallbacks"] == [], p["fallbacks"]
    assert all(not r.startswith("MIOpen") for r in p["layers"].values())
    comp = {n: r for n, r in p["layers"].items() if n.startswith("naive_compressor.")}
    assert set(comp) == {"naive_compressor.encoder.0", "naive_compressor.decoder.0", "naive_compressor.decoder.3"}
    enc = comp["naive_compressor.encoder.0"]
    if ratio == 1:
        assert all(r == SP for r in comp.values()), comp
    else:
        assert enc.startswith(NARROW) and comp["naive_compressor.decoder.0"].startswith(SP) and comp["naive_compressor.decoder.3"] == SP, comp
    model = build_model(h).eval()
    c = model.naive_compressor
    kind, cp = c.split_widths()
    mid = 64 // ratio
    assert cp >= mid and (kind, cp) == (("narrow", (mid + 15) // 16 * 16) if ratio > 1 else ("wide", 64))
    assert ("zero-padded to %d" % cp in enc) == (cp != mid)
    sp = lambda cin, cout: hip.lib().coalign_conv3x3_sp(ONE, ONE, ONE, NULL, 0, ONE, ops.SP_OUT_SP, 0, cin, cout, HW, HW, 1, 0, NULL, NULL, 0, NULL)
    assert (_narrow(64, cp) if enc.startswith(NARROW) else sp(64, cp)) == 0
    assert sp(cp, 64) == 0 and sp(64, 64) == 0
    # what the plan says is what the module decides
    assert c.takes_split_maps()
    assert isinstance(c.encoder[0], nn.Conv2d) and c.encoder[0].out_channels == mid


def test_route_plan_keeps_the_library_text_where_the_fallback_conditions_hold(monkeypatch):
    """Another arithmetic mode, SplitMaps switched off, or an input width the kernels do not take: the compressor's layers are reported on MIOpen, unchanged in
    words, and listed as fallbacks."""
    lib_text = "MIOpen (compressor: SURVEY 8a row D keeps it on the library)"
    names = ["naive_compressor.encoder.0", "naive_compressor.decoder.0", "naive_compressor.decoder.3"]
    h = _with_compression("mini_coalign", 4)
    p = plan(h, terms=3)
    assert [p["layers"][n] for n in names] == [lib_text] * 3 and set(names) <= set(p["fallbacks"])
    monkeypatch.setattr(bb, "SPLIT_MAPS", False)
    p = plan(h)
    assert [p["layers"][n] for n in names] == [lib_text] * 3 and set(names) <= set(p["fallbacks"])
    monkeypatch.setattr(bb, "SPLIT_MAPS", True)
    for dim, ratio, want in ((24, 2, None), (48, 2, None), (64, 3, ("narrow", 32)), (64, 64, ("narrow", 16)), (64, 1, ("wide", 64)), (128, 2, ("wide", 64)), (128, 4, ("narrow", 32))):
        c = bb.NaiveCompressor(dim, ratio).eval()
        assert c.split_widths() == want and c.takes_split_maps() == (want is not None), (dim, ratio)
    assert not bb.NaiveCompressor(64, 4).train().takes_split_maps()
