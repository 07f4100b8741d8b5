"""Stage 1 of all agents in one pass, host side (no GPU): the extension header include/coalign_amd_stage1.h against the product library and
``hip.STAGE1_SIGNATURES``, the frozen headers, argument validation before any HIP call, and ``ops.stage1_boxes`` refusing CPU tensors."""
import ctypes
import os
import re

import pytest
import torch

import abi_headers
from coalign_amd import hip, ops

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NULL, ONE = ctypes.c_void_p(0), ctypes.c_void_p(16)      # (a non-NULL token: none of these calls gets as far as touching memory)
HEADER = "coalign_amd_stage1.h"


def test_stage1_header_table_and_library_agree():
    """include/coalign_amd_stage1.h declares exactly the keys of ``hip.STAGE1_SIGNATURES`` (types, counts and exports: tests/test_abi_cpu.py); the header includes
    coalign_amd.h and cites the reference lines each entry point replaces."""
    text = open(abi_headers.path(HEADER)).read()
    assert '#include "coalign_amd.h"' in text
    declared = abi_headers.declarations(HEADER)
    assert set(declared) == set(hip.STAGE1_SIGNATURES) == abi_headers.names(HEADER) and len(declared) == 3
    comments = re.findall(r"/\*.*?\*/", text, flags=re.S)
    for name in declared:
        last = [c for c in comments if c in text[:text.index(name + "(")]][-1]
        assert "uncertainty_voxel_postprocessor.py:26-112" in last, name


def test_build_lists_the_new_header_among_the_rebuild_dependencies():
    src = open(os.path.join(REPO, "coalign_amd", "build.py")).read()
    assert '"coalign_amd_stage1.h"' in src


def _boxes(cls=ONE, reg=ONE, dir_=ONE, unc=ONE, anchors=ONE, n=2, A=2, H=15, W=31, bins=2, udim=3, top=1000, store=ONE, store_unc=ONE, count=ONE, status=ONE,
           ws=ONE, ws_bytes=None):
    L = hip.lib()
    if ws_bytes is None:
        ws_bytes = max(1, L.coalign_stage1_boxes_workspace_bytes(n, A, H, W, top))
    return L.coalign_stage1_boxes(cls, reg, dir_, unc, anchors, n, A, H, W, bins, udim, 0.2, 0.7853, 1, 0.15, top, store, store_unc, count, status, ws, ws_bytes, NULL)


def test_stage1_argument_validation_without_a_gpu():
    """NULL -1; n_agents outside 1 .. 8, udim outside 0 .. 3, non-positive A / H / W / top, dir with num_bins <= 0 -2; top > 1024 -3; a short workspace -4: all
    before any HIP call (token pointers, no GPU)."""
    L = hip.lib()
    for arg in ("cls", "reg", "anchors", "store", "count", "status", "ws", "unc", "store_unc"):
        assert _boxes(**{arg: NULL}) == -1, arg
    assert _boxes(unc=NULL, store_unc=NULL, udim=0, ws_bytes=0) == -4          # (udim 0 takes no uncertainty arrays; dir may be NULL: it gets as far as the workspace)
    assert _boxes(dir_=NULL, bins=0, ws_bytes=0) == -4
    for bad in (dict(n=0), dict(n=9), dict(n=-1), dict(udim=-1), dict(udim=4), dict(A=0), dict(H=0), dict(W=-3), dict(top=0), dict(top=-5), dict(bins=0), dict(bins=-1)):
        assert _boxes(**bad) == -2, bad
    assert _boxes(top=1025) == -3 and _boxes(top=4096) == -3
    need = L.coalign_stage1_boxes_workspace_bytes(2, 2, 15, 31, 1000)
    assert need > 2 * 2 * 15 * 31 * 24 * 4
    assert _boxes(ws_bytes=need - 1) == -4 and _boxes(ws_bytes=0) == -4
    assert L.coalign_stage1_boxes_workspace_bytes(8, 2, 15, 31, 1000) > L.coalign_stage1_boxes_workspace_bytes(2, 2, 15, 31, 1000)
    for bad in ((0, 2, 15, 31, 1000), (9, 2, 15, 31, 1000), (2, 0, 15, 31, 1000), (2, 2, 15, 31, 0), (2, 2, 15, 31, 1025)):
        assert L.coalign_stage1_boxes_workspace_bytes(*bad) == 0, bad


def test_strided_entry_point_validates_like_the_dense_one():
    """``coalign_stage1_boxes_strided``: the dense entry point's codes, and -2 for an agent stride below the size of one agent's maps."""
    L = hip.lib()
    hw = 2 * 15 * 31

    def strided(strides=(hw, 7 * hw, 2 * hw, 3 * hw), cls=ONE, n=2, top=1000, udim=3, ws_bytes=0):
        return L.coalign_stage1_boxes_strided(cls, ONE, ONE, ONE, *strides, ONE, n, 2, 15, 31, 2, udim, 0.2, 0.7853, 1, 0.15, top, ONE, ONE, ONE, ONE, ONE, ws_bytes, NULL)

    assert strided() == -4 and strided(strides=(26 * hw,) * 4) == -4            # dense, and the channel slices of one merged-heads tensor
    assert strided(cls=NULL) == -1 and strided(n=9) == -2 and strided(top=1025) == -3
    for k in range(4):
        short = [hw, 7 * hw, 2 * hw, 3 * hw]
        short[k] -= 1
        assert strided(strides=tuple(short)) == -2, k
    assert strided(strides=(hw, 7 * hw, 2 * hw, 0), udim=0) == -4


def test_stage1_boxes_refuses_cpu_tensors():
    """No CPU fallback: ``ops.stage1_boxes`` raises ``CoalignHipError`` on CPU tensors."""
    store = ops.Stage1Store("cpu")
    n, A, H, W = 2, 2, 15, 31
    cls, reg, dirp, unc = torch.zeros(n, A, H, W), torch.zeros(n, 7 * A, H, W), torch.zeros(n, 2 * A, H, W), torch.zeros(n, 3 * A, H, W)
    with pytest.raises(hip.CoalignHipError):
        ops.stage1_boxes(cls, reg, dirp, unc, torch.zeros(A * H * W, 7), store, torch.zeros(1024, dtype=torch.uint8), 0.2, 0.7853, 2, "hwl", 0.15)
    with pytest.raises(ValueError):
        ops.stage1_workspace(9, A, H, W, 1000, "cpu")
