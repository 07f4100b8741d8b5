"""Where2comm's messages, host side (no GPU): the extension header include/coalign_amd_where2comm_msg.h against
``hip.W2COMM_MSG_SIGNATURES``, argument refusals before any HIP call, ``where2comm.pack_messages_torch`` against a
numpy statement of the format (bit order, raster order, size), the wire round trip, the refusal of routes the message kernels do not serve, and the route plan's
wording with and without ``packed_wire``."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import abi_headers
from coalign_amd import hip, ops, routes, where2comm
from coalign_amd.backbone import BaseBEVBackbone
from coalign_amd.config import builtin_config
from coalign_amd.detector import PointPillarWhere2comm, build_model
from coalign_amd.fusion import Where2commFusion
from coalign_amd.where2comm import W2Message, pack_bits_torch, pack_messages_torch, rank_torch, unpack_bits_torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NULL, ONE = ctypes.c_void_p(0), ctypes.c_void_p(16)      # (a non-NULL, 16-byte aligned token: none of these calls gets as far as touching memory)
HEADER = "coalign_amd_where2comm_msg.h"
NAMES = {"coalign_w2comm_msg_index", "coalign_w2comm_msg_pack", "coalign_w2comm_fuse_packed"}
LEVELS = ((64, 5, 37), (128, 2, 18), (256, 1, 9))


def test_msg_header_table_and_library_agree():
    """The header declares exactly ``NAMES``, the keys of ``hip.W2COMM_MSG_SIGNATURES`` (types, counts and exports: tests/test_abi_cpu.py); every declaration says
    what it replaces or that the reference has no counterpart; build.py lists the source; the header documents the wire layout."""
    text = open(abi_headers.path(HEADER)).read()
    assert '#include "coalign_amd.h"' in text
    declared = abi_headers.declarations(HEADER)
    assert set(declared) == set(hip.W2COMM_MSG_SIGNATURES) == abi_headers.names(HEADER) == NAMES
    comments = re.findall(r"/\*.*?\*/", text, flags=re.S)
    for name in declared:
        last = [c for c in comments if c in text[:text.index(name + "(")]][-1]
        assert "the reference has no counterpart" in last and re.search(r"where2comm(_attn)?\.py:\d+", last), name
    assert "where2comm_attn.py:224-341" in [c for c in comments if c in text[:text.index("coalign_w2comm_fuse_packed(")]][-1]
    assert "ON THE WIRE" in text and hex(W2Message.MAGIC).upper()[2:] in text and "64 bytes" in text
    assert int(re.search(r"#define COALIGN_W2COMM_SRC_PACKED (\d+)", text).group(1)) == ops.W2COMM_SRC_PACKED
    assert int(re.search(r"#define COALIGN_W2COMM_SRC_DENSE (\d+)", text).group(1)) == ops.W2COMM_SRC_DENSE
    assert '"w2comm_msg.hip"' in open(os.path.join(REPO, "coalign_amd", "build.py")).read()


def _arr(ctype, values, size=3):
    return None if values is None else (ctype * max(size, len(values)))(*values)


def _index(n=3, levels=3, H=(9, 4, 2), W=(33, 16, 8), masks=(16, 16, 16), bits=(16, 16, 16), rank=(16, 16, 16), count=ONE):
    vp, i32 = ctypes.c_void_p, ctypes.c_int32
    return hip.lib().coalign_w2comm_msg_index(n, levels, _arr(i32, H), _arr(i32, W), _arr(vp, masks), _arr(vp, bits), _arr(vp, rank), count, NULL)


def _pack(n=3, levels=3, x=(16, 16, 16), C=(64, 128, 256), H=(9, 4, 2), W=(33, 16, 8), bits=(16, 16, 16), rank=(16, 16, 16), rows=(16, 16, 16)):
    vp, i32 = ctypes.c_void_p, ctypes.c_int32
    return hip.lib().coalign_w2comm_msg_pack(n, levels, _arr(vp, x), _arr(i32, C), _arr(i32, H), _arr(i32, W), _arr(vp, bits), _arr(vp, rank), _arr(vp, rows), NULL)


def _fuse(n_scales=1, C=(64,), H=(9,), W=(14,), kind=(0, 1, 1), src=(16, 16, 16), aux=(0, 16, 16), rank=(0, 16, 16), out=(32,), n=3, theta=ONE, mode=ops.FUSE_ATT):
    vp, i32 = ctypes.c_void_p, ctypes.c_int32
    return hip.lib().coalign_w2comm_fuse_packed(n_scales, _arr(i32, C), _arr(i32, H), _arr(i32, W), _arr(i32, kind, 24), _arr(vp, src, 24), _arr(vp, aux, 24), _arr(vp, rank, 24),
                                                _arr(vp, out), _arr(i32, H), _arr(i32, W), n, theta, mode, NULL)


def test_msg_argument_refusals_without_a_gpu():
    """NULL -1 (a packed source without rank or bits included); counts and sizes < 1, maps of 2^31 values -2; more than 8 agents, more than 3 levels, other channel
    counts, an unknown source kind or mode, misaligned rows / maps / bitmaps -3: all before any HIP call (token pointers, no GPU)."""
    for arg in ("H", "W", "bits", "rank"):
        assert _index(**{arg: None}) == -1, arg
    assert _index(count=NULL) == -1 and _index(bits=(16, 0, 16)) == -1 and _index(rank=(16, 16, 0)) == -1 and _index(masks=(16, 0, 16)) == -1
    for bad in (dict(n=0), dict(n=-1), dict(levels=0), dict(H=(0, 4, 2)), dict(W=(33, -1, 8)), dict(H=(65536, 4, 2), W=(65536, 16, 8))):
        assert _index(**bad) == -2, bad
    for bad in (dict(n=9), dict(levels=4), dict(bits=(18, 16, 16)), dict(rank=(16, 16, 17)), dict(count=ctypes.c_void_p(18))):
        assert _index(**bad) == -3, bad
    for arg in ("x", "C", "H", "W", "bits", "rank", "rows"):
        assert _pack(**{arg: None}) == -1, arg
    for arg in ("x", "bits", "rank", "rows"):
        assert _pack(**{arg: (16, 0, 16)}) == -1, arg
    for bad in (dict(n=0), dict(levels=0), dict(C=(0, 128, 256)), dict(H=(9, 0, 2)), dict(W=(33, 16, -8)), dict(C=(256, 128, 64), H=(4096, 4, 2), W=(4096, 16, 8))):
        assert _pack(**bad) == -2, bad
    for bad in (dict(n=9), dict(levels=4), dict(C=(96, 128, 256)), dict(C=(64, 128, 32)), dict(rows=(16, 24, 16)), dict(rows=(20, 16, 16)), dict(x=(16, 16, 8)), dict(bits=(16, 18, 16)),
                dict(rank=(17, 16, 16))):
        assert _pack(**bad) == -3, bad
    for arg in ("C", "H", "W", "kind", "src", "aux", "rank", "out"):
        assert _fuse(**{arg: None}) == -1, arg
    assert _fuse(theta=NULL) == -1 and _fuse(out=(0,)) == -1 and _fuse(src=(16, 0, 16)) == -1
    assert _fuse(rank=(0, 16, 0)) == -1 and _fuse(aux=(0, 0, 16)) == -1          # a packed source without its rank table / its bitmap
    assert _fuse(kind=(0, 0, 0), aux=(0, 0, 0), rank=(0, 0, 0), mode=7) == -3          # ... which dense sources do not need: this call gets as far as the mode
    for bad in (dict(n_scales=0), dict(n=0), dict(n=-1), dict(H=(0,)), dict(W=(-1,)), dict(C=(256,), H=(4096,), W=(4096,))):
        assert _fuse(**bad) == -2, bad
    for bad in (dict(n_scales=4), dict(n=9), dict(mode=ops.FUSE_NONE), dict(mode=7), dict(C=(96,)), dict(C=(32,)), dict(kind=(0, 2, 1)), dict(src=(16, 20, 16)), dict(src=(24, 16, 16)),
                dict(out=(8,)), dict(aux=(0, 18, 16)), dict(rank=(0, 16, 17))):
        assert _fuse(**bad) == -3, bad
    assert ops.w2comm_msg_shape_ok([64, 128, 256], 8, [(100, 352), (50, 176), (25, 88)]) and ops.w2comm_msg_shape_ok([256], 1)
    assert not ops.w2comm_msg_shape_ok([96], 2) and not ops.w2comm_msg_shape_ok([64], 9) and not ops.w2comm_msg_shape_ok([64] * 4, 2) and not ops.w2comm_msg_shape_ok([], 2)
    assert not ops.w2comm_msg_shape_ok([256], 2, [(4096, 4096)]) and not ops.w2comm_msg_shape_ok([64], 2, [(0, 4)])
    assert ops.w2comm_msg_index_shape_ok(8, [(1, 1)]) and not ops.w2comm_msg_index_shape_ok(9, [(1, 1)]) and not ops.w2comm_msg_index_shape_ok(2, [(1, 1)] * 4)


def test_msg_ops_refuse_cpu_tensors():
    x = torch.zeros(2, 64, 4, 4).contiguous(memory_format=torch.channels_last)
    m = torch.ones(2, 4, 4, dtype=torch.uint8)
    words = torch.zeros(2, 4, 1, dtype=torch.int32)
    with pytest.raises(hip.CoalignHipError):
        ops.w2comm_msg_index([m])
    with pytest.raises(hip.CoalignHipError):
        ops.w2comm_msg_index(None, [words], [(4, 4)])
    with pytest.raises(hip.CoalignHipError):
        ops.w2comm_msg_pack([x], [words], [words])
    with pytest.raises(hip.CoalignHipError):
        ops.w2comm_fuse_packed([[(x[0], m[0]), (torch.zeros(16, 64), words[0], words[0])]], [(64, 4, 4)], torch.zeros(2, 2, 3, dtype=torch.float64), ops.FUSE_MAX)


# ---- the format ------------------------------------------------------------------------------------------------------------------------------------------------------
def numpy_message(x, mask):
    """The format in numpy, loops and all: x [C, H, W], mask [H, W] -> (words uint32 [H, Wd], rank int32 [H, Wd], rows [K, C])."""
    C, H, W = x.shape
    Wd = (W + 31) // 32
    words, rank, rows = np.zeros((H, Wd), dtype=np.uint32), np.zeros((H, Wd), dtype=np.int32), []
    for y in range(H):
        for xx in range(W):
            if xx % 32 == 0:
                rank[y, xx // 32] = len(rows)
            if mask[y, xx]:
                words[y, xx >> 5] |= np.uint32(1) << np.uint32(xx & 31)
                rows.append(x[:, y, xx])
    return words, rank, np.stack(rows) if rows else np.zeros((0, C), dtype=np.float32)


def level_inputs(n, density, seed, levels=LEVELS):
    g = torch.Generator().manual_seed(seed)
    xs = [torch.randn(n, C, H, W, generator=g) for C, H, W in levels]
    masks = [(torch.rand(n, H, W, generator=g) < density).to(torch.uint8) for _, H, W in levels]
    return xs, masks


@pytest.mark.parametrize("density", [0.0, 0.1, 0.55, 1.0])
def test_pack_messages_torch_is_the_format(density):
    """Bit (x & 31) of word [y, x >> 5]; zero padding bits; rows in raster order, copied bit for bit; rank = set bits before the word; count = K; ``nbytes`` =
    64 + sum 4 (H Wd + K C) = ``len(to_wire())``; the wire's words are the header, the bitmaps and ``rows[:K]``, little-endian."""
    xs, masks = level_inputs(3, density, seed=11)
    masks[0][2, -1, -1] = 1                                                            # (agent 2: the last pixel of a map whose width is 5 mod 32)
    msgs = pack_messages_torch(xs, masks)
    assert len(msgs) == 3
    for j, msg in enumerate(msgs):
        assert msg.levels == 3 and msg.shapes == [tuple(s) for s in LEVELS] and msg.count.dtype == torch.int32 and tuple(msg.count.shape) == (3,)
        size, wire_bits, wire_rows = 64, [], []
        for l, (C, H, W) in enumerate(LEVELS):
            words, rank, rows = numpy_message(xs[l][j].numpy(), masks[l][j].numpy())
            K = rows.shape[0]
            assert K == int(masks[l][j].sum()) == msg.counts()[l]
            assert msg.bits[l].dtype == torch.int32 and np.array_equal(msg.bits[l].numpy().view(np.uint32), words)
            assert np.array_equal(msg.rank[l].numpy(), rank)
            assert tuple(msg.rows[l].shape) == (max(1, H * W), C) and np.array_equal(msg.rows[l][:K].numpy().view(np.uint32), rows.view(np.uint32))
            assert torch.equal(msg.masks()[l], masks[l][j])
            size += 4 * (H * ((W + 31) // 32) + K * C)
            wire_bits.append(words.astype("<u4").tobytes()); wire_rows.append(rows.astype("<f4").tobytes())
        wire = msg.to_wire()
        assert wire.dtype == torch.uint8 and wire.dim() == 1 and wire.is_contiguous()
        assert msg.nbytes == size == wire.numel() == int(msg.nbytes_device())
        head = np.zeros(16, dtype="<u4")
        head[:3] = (0x4D433257, 1, 3)
        for l, (C, H, W) in enumerate(LEVELS):
            head[4 + 4 * l: 8 + 4 * l] = (C, H, W, msg.counts()[l])
        assert wire.numpy().tobytes() == head.tobytes() + b"".join(wire_bits) + b"".join(wire_rows)
        assert wire.numpy()[:4].tobytes() == b"W2CM"


def test_bit_helpers_at_the_word_boundary():
    for W in (1, 31, 32, 33, 64, 70):
        m = (torch.rand(3, W, generator=torch.Generator().manual_seed(W)) < 0.5).to(torch.uint8)
        m[0, W - 1] = 1
        b = pack_bits_torch(m)
        assert tuple(b.shape) == (3, (W + 31) // 32) and torch.equal(unpack_bits_torch(b, W), m)
        if W % 32:
            assert bool((((b[:, -1].to(torch.int64) % 2 ** 32) >> (W % 32)) == 0).all())          # padding bits are zero
        rank, K = rank_torch(b, W)
        assert int(K) == int(m.sum()) and int(rank[0, 0]) == 0 and int(rank[-1, -1]) == int(m.sum()) - int(m[-1, 32 * (b.shape[1] - 1):].sum())
        dirty = b.clone()
        if W % 32:                                                                     # padding bits are ignored by a receiver
            dirty[:, -1] |= torch.tensor(-(2 ** 31), dtype=torch.int32)
            assert torch.equal(unpack_bits_torch(dirty, W), m) and torch.equal(rank_torch(dirty, W)[0], rank)


@pytest.mark.parametrize("levels", [LEVELS, LEVELS[:1], ((128, 3, 4),)])
def test_wire_round_trip_on_the_cpu(levels):
    xs, masks = level_inputs(2, 0.4, seed=5, levels=levels)
    masks[0][1].zero_()                                                                # agent 1 sends nothing at level 0
    for msg in pack_messages_torch(xs, masks):
        wire = msg.to_wire()
        back = W2Message.from_wire(wire, "cpu")
        assert back.shapes == msg.shapes and torch.equal(back.count, msg.count) and back.nbytes == msg.nbytes
        for l in range(msg.levels):
            assert torch.equal(back.bits[l], msg.bits[l]) and torch.equal(back.rank[l], msg.rank[l])
            assert back.rows[l].shape == msg.rows[l].shape and np.array_equal(back.rows[l].numpy().view(np.uint32), msg.rows[l].numpy().view(np.uint32))
        assert torch.equal(back.to_wire(), wire)
        for bad in (wire[:-4], torch.cat([wire, wire[:4]]), wire[:60]):
            with pytest.raises(ValueError):
                W2Message.from_wire(bad)
        for word, value in ((0, 0), (1, 2), (2, 4), (4, 96), (7, 10 ** 6)):          # magic, version, levels, C_0, K_0
            broken = wire.clone()
            broken[4 * word: 4 * word + 4] = torch.from_numpy(np.array([value], dtype="<u4").view(np.uint8).copy())
            with pytest.raises(ValueError):
                W2Message.from_wire(broken)
    flipped = pack_messages_torch(xs, masks)[0].to_wire().clone()
    flipped[64] ^= 1                                                                   # one mask bit: the population no longer equals the header's count
    with pytest.raises(ValueError, match="population"):
        W2Message.from_wire(flipped)


# ---- routes ----------------------------------------------------------------------------------------------------------------------------------------------------------
def module_args(multi_scale, channels=(64, 128, 256), communication=True):
    args = {"voxel_size": [0.4, 0.4, 4], "downsample_rate": 1, "multi_scale": multi_scale, "agg_operator": {"mode": "MAX", "feature_dim": channels[0]}}
    if communication:
        args["communication"] = {"thre": 0.3, "gaussian_smooth": {"k_size": 5, "c_sigma": 1.0}}
    if multi_scale:
        args.update(layer_nums=[1] * len(channels), num_filters=list(channels))
    return args


def identity(n):
    A = torch.zeros(1, n, n, 2, 3, dtype=torch.float64)
    A[..., 0, 0] = A[..., 1, 1] = 1.0
    return A


def test_unserved_packed_routes_raise_with_the_reason():
    """CPU maps, training mode, a plain ``BaseBEVBackbone`` in multi-scale mode, no communication section, channels outside the kernels': ``wire="packed"`` raises and
    says why; the default wire still serves every one of them op by op."""
    x, psm, A = torch.randn(2, 64, 6, 8), torch.randn(2, 2, 6, 8), identity(2)
    m = Where2commFusion(module_args(False)).eval()
    with pytest.raises(NotImplementedError, match="maps on the CPU"):
        m.fuse(x, psm, [2], A, wire="packed")
    assert m.packed_route_reason([64], 2) is None
    out, _, extra = m.fuse(x, psm, [2], A)
    assert tuple(out.shape) == (1, 64, 6, 8) and extra == {}
    with pytest.raises(ValueError, match="dense | packed"):
        m.fuse(x, psm, [2], A, wire="sparse")
    m.train()
    with pytest.raises(NotImplementedError, match="training mode"):
        m.fuse(x, psm, [2], A, wire="packed")
    assert "training mode" in m.packed_route_reason([64], 2)
    m.eval()
    m.force_torch = True
    with pytest.raises(NotImplementedError, match="force_torch"):
        m.fuse(x, psm, [2], A, wire="packed")
    none = Where2commFusion(module_args(False, communication=False)).eval()
    with pytest.raises(NotImplementedError, match="no communication section"):
        none.fuse(x, None, [2], A, wire="packed")
    odd = Where2commFusion(module_args(False, channels=(16,))).eval()
    with pytest.raises(NotImplementedError, match=r"outside the kernel's 64 / 128 / 256"):
        odd.fuse(torch.randn(2, 16, 6, 8), psm, [2], A, wire="packed")
    cfg = {"layer_nums": [1, 1], "layer_strides": [1, 2], "num_filters": [64, 128], "upsample_strides": [1, 2], "num_upsample_filter": [8, 8]}
    plain = BaseBEVBackbone(cfg, 4).eval()
    ms = Where2commFusion(module_args(True, channels=(64, 128))).eval()
    reason = ms.kernel_shape_reason([64, 128], 2, resnet=False)
    assert reason.startswith("a plain BaseBEVBackbone")
    with pytest.raises(NotImplementedError) as err:
        ms.fuse(torch.randn(2, 4, 8, 12), torch.randn(2, 2, 8, 12), [2], A, plain, wire="packed")
    assert reason in str(err.value)
    out, _, _ = ms.fuse(torch.randn(2, 4, 8, 12), torch.randn(2, 2, 8, 12), [2], A, plain)
    assert tuple(out.shape) == (1, 16, 8, 12)


def test_model_flag_defaults_off_and_refuses_on_the_cpu():
    h = builtin_config("mini_pointpillar_where2comm")
    model = build_model(h).eval()
    assert PointPillarWhere2comm.packed_wire is False and model.packed_wire is False and "packed_wire" not in vars(model)
    keys = list(model.state_dict())
    flagged = build_model({**h, "model": {**h["model"], "args": {**h["model"]["args"], "packed_wire": True}}}).eval()
    assert flagged.packed_wire is True and list(flagged.state_dict()) == keys
    C = model._level_channels()
    maps = [torch.randn(2, c, 16 >> l, 32 >> l) for l, c in enumerate(C)]
    psm = torch.randn(2, model.cls_head.out_channels, 16, 32)
    with pytest.raises(NotImplementedError, match="maps on the CPU"):
        flagged.fuse_and_head([*maps, psm], [2], identity(2))
    with torch.no_grad():
        out = model.fuse_and_head([*maps, psm], [2], identity(2))
    assert set(out) == {"cls_preds", "reg_preds", "dir_preds", "comm_rates"}


@pytest.mark.parametrize("name", ("opv2v_pointpillar_where2comm", "mini_pointpillar_where2comm"))
def test_route_plan_words_the_packed_route_with_the_flag(name, monkeypatch):
    h = builtin_config(name)
    plain = routes.plan(h, baselines=True)
    assert plain["fusion"] == routes.W2COMM == Where2commFusion.KERNELS and "fusion" not in plain["fallbacks"]
    monkeypatch.setattr(PointPillarWhere2comm, "packed_wire", True)
    packed = routes.plan(h, baselines=True)
    assert packed["fusion"] == Where2commFusion.KERNELS_PACKED != routes.W2COMM and "fusion" not in packed["fallbacks"]
    for kernel in ("w2comm_msg_index", "w2comm_msg_pack", "w2comm_fuse_packed"):
        assert kernel in packed["fusion"], kernel
    assert {k: v for k, v in packed.items() if k != "fusion"} == {k: v for k, v in plain.items() if k != "fusion"}
    monkeypatch.setattr(PointPillarWhere2comm, "packed_wire", False)
    assert routes.plan(h, baselines=True) == plain
    by_key = routes.plan({**h, "model": {**h["model"], "args": {**h["model"]["args"], "packed_wire": True}}}, baselines=True)
    assert by_key["fusion"] == Where2commFusion.KERNELS_PACKED
