"""NaiveCompressor's encoder reading the sparse canvas, the part that needs no GPU: the third extension header against the binding table and the library, the
argument checks of ``coalign_conv3x3_sp_narrow_sparse`` (all before any HIP call), and ``routes.plan`` / the two route predicates with ``compression`` in the
config.

``coalign_conv3x3_sp_narrow_sparse`` (include/coalign_amd_narrow_sparse.h) is ``coalign_conv3x3_sp_narrow`` with the pair (sp16 feature rows, cell stamps) of
csrc/pillar_sparse.hip as its input: the encoder of opencood/models/sub_modules/naive_compress.py:5-31 without a dense canvas in front of it.
"""
import copy
import ctypes
import os
import re

import pytest

import abi_headers
from coalign_amd import backbone as bb
from coalign_amd import detector, hip
from coalign_amd.config import builtin_config
from coalign_amd.detector import build_model
from coalign_amd.routes import COMPRESSOR_LIBRARY, NARROW, SP, plan

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NULL, ONE = ctypes.c_void_p(0), ctypes.c_void_p(16)      # (a non-NULL, 16-byte aligned token: none of the calls below gets as far as touching memory)
HW = 8
HEADER = "coalign_amd_narrow_sparse.h"
NAME = "coalign_conv3x3_sp_narrow_sparse"
ENCODER, PILLAR_SPARSE, PILLAR_DENSE = "naive_compressor.encoder.0", "sparse canvas read by the compressor's encoder", "persistent dense canvas"


def _call(cin=64, cout=16, n=0, rows=ONE, m=4, stamps=ONE, state=ONE, w=ONE, bias=ONE, y=ONE, h=HW, wd=HW):
    return hip.lib().coalign_conv3x3_sp_narrow_sparse(rows, m, stamps, state, w, bias, y, n, cin, cout, h, wd, 1, NULL, NULL)


def test_third_extension_header_table_and_library_agree():
    """include/coalign_amd_narrow_sparse.h declares exactly one name; the product library exports it; it equals ``hip.NARROW_SPARSE_SIGNATURES``, argument types
    included (``const int32_t *`` is a device buffer here: its own mapping, not the rule of tests/abi_headers.py); the declaration's comment cites
    naive_compress.py:5-31."""
    decl = abi_headers.declarations(HEADER)
    assert set(decl) == abi_headers.names(HEADER) == set(hip.NARROW_SPARSE_SIGNATURES) == {NAME}
    ctype = {"int": ctypes.c_int, "constvoid*": ctypes.c_void_p, "void*": ctypes.c_void_p, "constint32_t*": ctypes.c_void_p, "int32_t*": ctypes.c_void_p,
             "constfloat*": ctypes.c_void_p}
    ret, args = decl[NAME]
    args = [re.sub(r"\s*\w+$", "", a).replace(" ", "") for a in args]                              # "const int32_t *stamps" -> "constint32_t*"
    assert ret is ctypes.c_int and hip.NARROW_SPARSE_SIGNATURES[NAME] == (ctypes.c_int, [ctype[a] for a in args]) and len(args) == 15
    fn = getattr(hip.lib(), NAME)
    assert fn.restype is ctypes.c_int and list(fn.argtypes) == hip.NARROW_SPARSE_SIGNATURES[NAME][1]
    text = open(abi_headers.path(HEADER)).read()
    assert '#include "coalign_amd.h"' in text
    comments = re.findall(r"/\*.*?\*/", text, flags=re.S)
    last = [c for c in comments if c in text[:text.index(NAME + "(")]][-1]
    assert "opencood/models/sub_modules/naive_compress.py:5-31" in last


def test_sparse_narrow_argument_validation_without_a_gpu():
    """NULL pointers -1; M_rows < 0 and the shape limits -2; Cin % 16, Cin = 16 (one interval: no lead for the stamps), Cout outside {16, 32}, misaligned
    pointers (stamps: 8 bytes), M_rows * Cin / 4 >= 2^31 and the 32-bit group offsets -3; N = 0 returns 0 -- on a machine without a GPU, so before any HIP call."""
    assert _call() == 0 and _call(64, 32) == 0 and _call(32, 16) == 0 and _call(256, 32, m=0) == 0      # N = 0: validated, nothing launched
    for arg in ("rows", "stamps", "state", "w", "bias", "y"):
        assert _call(n=1, **{arg: NULL}) == -1, arg
    assert _call(m=-1) == -2
    assert _call(n=-1) == -2 and _call(h=0) == -2 and _call(wd=-3) == -2 and _call(cin=-16) == -2 and _call(cout=0) == -2      # narrow_check
    assert _call(cin=24) == -3 and _call(cin=40) == -3
    for cout in (8, 24, 48, 64, 128):
        assert _call(cout=cout) == -3, cout
    assert _call(cin=16) == -3 and _call(cin=16, cout=32) == -3                                        # documented: Cin >= 32
    for arg in ("rows", "w", "y"):
        assert _call(**{arg: ctypes.c_void_p(24)}) == -3, arg                                          # 16-byte alignment
    assert _call(bias=ctypes.c_void_p(18)) == -3
    assert _call(stamps=ctypes.c_void_p(20)) == -3 and _call(stamps=ctypes.c_void_p(24)) == 0          # 8-byte alignment
    assert _call(m=(1 << 31) // 16) == -3 and _call(m=(1 << 31) // 16 - 1) == 0                        # M_rows * 64 / 4 < 2^31
    assert _call(cin=256, m=(1 << 31) // 64) == -3 and _call(cin=256, m=(1 << 31) // 64 - 1) == 0
    assert _call(64, 32, n=1 << 20, h=1 << 10, wd=1 << 10) == -3                                       # group offsets are 32-bit
    # the dense entry point keeps its two input kinds
    assert hip.lib().coalign_conv3x3_sp_narrow(ONE, 2, ONE, ONE, ONE, 0, 64, 16, HW, HW, 1, NULL, NULL) == -3


def _with_compression(cfg, ratio):
    h = copy.deepcopy(builtin_config(cfg))
    h["model"]["args"]["compression"] = ratio
    return h


@pytest.mark.parametrize("cfg", ["opv2v_coalign", "mini_coalign"])
@pytest.mark.parametrize("ratio", [2, 4, 8])
def test_route_plan_puts_the_compressors_encoder_on_the_sparse_canvas(cfg, ratio):
    """Ratios 2, 4, 8: the encoder line starts with NARROW and names the sparse canvas, the pillar line names the one-launch encoder, nothing is a fallback;
    ``compressor_sparse_route`` holds while ``sparse_canvas_route`` (the FIRST BLOCK reads the canvas) does not."""
    h = _with_compression(cfg, ratio)
    p = plan(h)
    enc = p["layers"][ENCODER]
    assert enc.startswith(NARROW) and enc.startswith(NARROW + ", sparse canvas in"), enc
    assert "sparse canvas" in p["pillar"] and PILLAR_SPARSE in p["pillar"] and "ONE launch" in p["pillar"], p["pillar"]
    assert p["fallbacks"] == [] and p["outside_hot_path"] is None
    model = build_model(h).eval()
    assert detector.compressor_sparse_route(model) and not detector.sparse_canvas_route(model)
    assert model.naive_compressor.takes_sparse_canvas() and model.naive_compressor.takes_sparse_canvas(16)
    assert not model.train().naive_compressor.takes_sparse_canvas() and not detector.compressor_sparse_route(model)


def test_other_routes_read_as_before(monkeypatch):
    """``compression: 1`` (the wide route), the selector off and ``terms = 3`` keep both lines as they were; a model without a compressor keeps
    "read by the first ResNet block"."""
    h1 = _with_compression("mini_coalign", 1)
    p = plan(h1)
    assert p["layers"][ENCODER] == SP and PILLAR_DENSE in p["pillar"] and "sparse canvas" not in p["pillar"]
    m1 = build_model(h1).eval()
    assert not detector.compressor_sparse_route(m1) and not m1.naive_compressor.takes_sparse_canvas()
    h4 = _with_compression("mini_coalign", 4)
    p3 = plan(h4, terms=3)
    assert p3["layers"][ENCODER] == COMPRESSOR_LIBRARY and "sparse canvas" not in p3["pillar"]
    m4 = build_model(h4).eval()
    assert not detector.compressor_sparse_route(m4, 3) and detector.compressor_sparse_route(m4, 16)
    on = plan(h4)
    monkeypatch.setattr(bb, "COMPRESS_SPARSE", False)
    off = plan(h4)
    assert off["layers"][ENCODER] == NARROW and on["layers"][ENCODER] == NARROW + ", sparse canvas in"
    assert PILLAR_DENSE in off["pillar"] and "sparse canvas" not in off["pillar"] and off["fallbacks"] == []
    assert {k: v for k, v in on["layers"].items() if k != ENCODER} == {k: v for k, v in off["layers"].items() if k != ENCODER}
    assert not detector.compressor_sparse_route(m4) and not m4.naive_compressor.takes_sparse_canvas()
    monkeypatch.setattr(bb, "COMPRESS_SPARSE", True)
    monkeypatch.setattr(detector, "SPARSE_CANVAS", False)                                              # the encoder side's own switch
    assert not detector.compressor_sparse_route(m4) and PILLAR_DENSE in plan(h4)["pillar"]
    monkeypatch.setattr(detector, "SPARSE_CANVAS", True)
    plain = plan(builtin_config("mini_coalign"))
    assert "sparse canvas read by the first ResNet block" in plain["pillar"]
