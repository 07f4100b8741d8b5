"""Where2comm's messages on the GPU (csrc/w2comm_msg.hip through the C ABI): the index kernel against numpy with integer equality, in both forms; the pack kernel
against ``x.permute(0, 2, 3, 1)[mask]`` with ``torch.equal`` and a sentinel behind the count; ``w2comm_fuse_packed`` against ``w2comm_fuse_nhwc`` on the same maps,
masks and theta with ``torch.equal`` -- all agents packed, a mix of dense and packed, an all-zero and an all-ones mask, NaN behind the count -- and against float64
at the dense kernel's own bound; the module's packed wire against its default route, single and multi scale, and under graph capture; the wire round trip on the
device; the model (``mini_pointpillar_where2comm.yaml``) with ``packed_wire`` on and off."""
import numpy as np
import pytest
import torch

from conftest import assert_elementwise
from coalign_amd import ops
from coalign_amd.inference import inference_intermediate_fusion
from coalign_amd.postprocess import build_postprocessor
from coalign_amd.where2comm import W2Message, pack_messages_torch
from test_where2comm_gpu import DEV, LEVELS, MODES, _mini_world, affine_of, decode_backbone, dev, fuse_inputs, level_maps, module_of, nhwc
from v2v_reference import make_thetas, student_t
from where2comm_reference import mask_case, where2comm_levels_f64

pytestmark = pytest.mark.gpu


# ---- index -----------------------------------------------------------------------------------------------------------------------------------------------------------
def numpy_index(mask):
    """[n, H, W] 0 / 1 -> (words uint32 [n, H, Wd], rank int32 [n, H, Wd], count [n])."""
    n, H, W = mask.shape
    Wd = (W + 31) // 32
    padded = np.zeros((n, H, Wd * 32), dtype=np.uint8)
    padded[:, :, :W] = mask != 0
    words = np.packbits(padded.reshape(n, H, Wd, 32), axis=-1, bitorder="little").view("<u4").reshape(n, H, Wd)
    per_word = padded.reshape(n, H * Wd, 32).sum(-1).astype(np.int64)
    inc = per_word.cumsum(-1)
    return words, (inc - per_word).reshape(n, H, Wd).astype(np.int32), inc[:, -1].astype(np.int32)


def density_masks(n, hw, density, seed):
    g = torch.Generator().manual_seed(seed)
    out = []
    for H, W in hw:
        if density == "last":
            m = torch.zeros(n, H, W, dtype=torch.uint8)
            m[:, -1, -1] = 1
        else:
            m = (torch.rand(n, H, W, generator=g) < density).to(torch.uint8)
        out.append(m)
    return out


# (100, 352) is the one shape beside the listed ones: 1100 words, five passes of the 256-lane scan (the largest of the others, (41, 70), has 123 words: one pass).
@pytest.mark.parametrize("density", [0.0, 1.0, 0.1, 0.55, "last"])
@pytest.mark.parametrize("H,W", [(1, 1), (3, 4), (9, 31), (9, 32), (9, 33), (16, 64), (25, 88), (41, 70), (100, 352)])
def test_index_against_numpy_in_both_forms(H, W, density):
    for n in (1, 5, 8):
        for levels in (1, 3):
            hw = [(max(1, H >> l), max(1, W >> l)) for l in range(levels)]
            masks = density_masks(n, hw, density, seed=H * W + n)
            bits, rank, count = ops.w2comm_msg_index([m.to(DEV) for m in masks])
            assert tuple(count.shape) == (n, levels) and count.dtype == torch.int32
            for l, m in enumerate(masks):
                words, want_rank, want_count = numpy_index(m.numpy())
                assert bits[l].dtype == rank[l].dtype == torch.int32 and tuple(bits[l].shape) == tuple(rank[l].shape) == words.shape
                assert np.array_equal(bits[l].cpu().numpy().view(np.uint32), words), (n, levels, l)
                assert np.array_equal(rank[l].cpu().numpy(), want_rank), (n, levels, l)
                assert np.array_equal(count[:, l].cpu().numpy(), want_count), (n, levels, l)
            # the receiver form, from the produced bits -- and from bits whose padding is dirty, which a receiver ignores
            bits2, rank2, count2 = ops.w2comm_msg_index(None, bits, hw)
            dirty = [b.clone() for b in bits]
            for b, (_, w) in zip(dirty, hw):
                if w % 32:
                    b[..., -1] |= torch.tensor(-(2 ** 31), dtype=torch.int32, device=DEV)
            _, rank3, count3 = ops.w2comm_msg_index(None, dirty, hw)
            assert torch.equal(count2, count) and torch.equal(count3, count)
            for a, b, c, d in zip(rank, rank2, rank3, bits2):
                assert torch.equal(a, b) and torch.equal(a, c)
            assert all(a is b for a, b in zip(bits, bits2))          # (read, not rewritten)


def test_index_unaligned_mask_rows_take_the_byte_path():
    """A mask whose rows start off a 4-byte boundary (a view one byte into its storage) with a width that is a multiple of 4."""
    store = (torch.rand(2 * 9 * 32 + 1, generator=torch.Generator().manual_seed(3)) < 0.5).to(torch.uint8).to(DEV)
    m = store[1:].view(2, 9, 32)
    assert m.data_ptr() % 4 == 1 and m.is_contiguous()
    bits, rank, count = ops.w2comm_msg_index([m])
    words, want_rank, want_count = numpy_index(m.cpu().numpy())
    assert np.array_equal(bits[0].cpu().numpy().view(np.uint32), words) and np.array_equal(rank[0].cpu().numpy(), want_rank) and np.array_equal(count[:, 0].cpu().numpy(), want_count)


# ---- pack ------------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shapes", [LEVELS, ((64, 9, 14),), ((128, 9, 33),), ((256, 9, 14),), ((64, 1, 3),)], ids=["three-levels", "odd-64", "odd-128", "odd-256", "one-row"])
@pytest.mark.parametrize("n", [1, 5, 8])
def test_pack_rows_and_sentinel(shapes, n):
    xs = [nhwc(student_t((n, C, H, W), 3 * n + i).to(DEV)) for i, (C, H, W) in enumerate(shapes)]
    masks = [m.to(DEV) for m in density_masks(n, [(H, W) for _, H, W in shapes], 0.55, seed=n)]
    if n > 1:
        masks[0][0].zero_()                                                            # an agent that sends nothing ...
        masks[0][1].fill_(1)                                                           # ... and one that sends everything
    bits, rank, count = ops.w2comm_msg_index(masks)
    sentinel = -12345.0
    rows = [torch.full((n, max(1, H * W), C), sentinel, device=DEV) for C, H, W in shapes]
    got = ops.w2comm_msg_pack(xs, bits, rank, rows=rows)
    fresh = ops.w2comm_msg_pack(xs, bits, rank)
    for l, (x, m) in enumerate(zip(xs, masks)):
        assert got[l] is rows[l] and tuple(fresh[l].shape) == tuple(rows[l].shape)
        for j in range(n):
            K = int(m[j].sum())
            assert int(count[j, l]) == K
            want = x.permute(0, 2, 3, 1)[j][m[j].bool()]
            assert torch.equal(got[l][j, :K], want) and torch.equal(fresh[l][j, :K], want), (l, j)
            assert bool((got[l][j, K:] == sentinel).all()), (l, j)


# ---- fuse ------------------------------------------------------------------------------------------------------------------------------------------------------------
def packed_levels(xs, masks, fill=None):
    """-> per level (rows [n, cap, C], bits, rank) of ALL agents; ``fill``: what the rows hold before the pack (and keep behind the count)."""
    bits, rank, _ = ops.w2comm_msg_index(masks)
    rows = None if fill is None else [torch.full((x.shape[0], max(1, x.shape[2] * x.shape[3]), x.shape[1]), fill, device=DEV) for x in xs]
    return ops.w2comm_msg_pack(xs, bits, rank, rows=rows), bits, rank


def fuse_from(xs, masks, theta, mode, packed_agents, fill=None, maskless=()):
    rows, bits, rank = packed_levels(xs, masks, fill)
    sources = [[(rows[l][j], bits[l][j], rank[l][j]) if j in packed_agents else (x[j], None if j in maskless else masks[l][j]) for j in range(x.shape[0])] for l, x in enumerate(xs)]
    return ops.w2comm_fuse_packed(sources, [tuple(x.shape[1:]) for x in xs], theta, MODES[mode])


@pytest.mark.parametrize("mode", ["ATTEN", "MAX"])
@pytest.mark.parametrize("n", [1, 2, 5, 8])
@pytest.mark.parametrize("shapes", [LEVELS, ((64, 9, 14),), ((128, 9, 14),), ((256, 9, 14),)], ids=["three-levels", "odd-64", "odd-128", "odd-256"])
def test_fuse_packed_equals_the_dense_kernel(shapes, n, mode):
    xs, masks, theta = fuse_inputs(shapes, n, seed=7 * n + len(shapes))
    others, nan = set(range(1, n)), float("nan")
    want = ops.w2comm_fuse_nhwc(xs, masks, theta, MODES[mode])

    def same(got, ref, what):
        for a, b in zip(got, ref):
            assert a.shape == b.shape and torch.equal(a, b), (what, int((a != b).sum()))

    same(fuse_from(xs, masks, theta, mode, others), want, "all non-ego agents packed")
    same(fuse_from(xs, masks, theta, mode, others, fill=nan), want, "rows prefilled with NaN behind K")
    same(fuse_from(xs, masks, theta, mode, set(range(n)), fill=nan), want, "the ego packed too")
    same(fuse_from(xs, masks, theta, mode, set(range(1, n, 2)), fill=nan), want, "odd agents packed, even agents dense")
    same(fuse_from(xs, masks, theta, mode, set()), want, "every agent dense")
    if n > 1:
        assert bool(torch.isnan(packed_levels(xs, masks, nan)[0][0][1]).any())          # (the NaN is there: behind agent 1's count)
    for value in (0, 1):                                                                 # the last agent sends nothing / everything
        edge = [m.clone() for m in masks]
        for m in edge:
            m[n - 1].fill_(value)
        ref = ops.w2comm_fuse_nhwc(xs, edge, theta, MODES[mode])
        same(fuse_from(xs, edge, theta, mode, others if n > 1 else {0}, fill=nan), ref, f"a mask of all {value}")
        if value == 1:
            same(fuse_from(xs, edge, theta, mode, others - {n - 1}, fill=nan, maskless={n - 1}), ref, "a dense source without a mask is one with all ones")
    f64 = where2comm_levels_f64([x.cpu() for x in xs], [m.cpu() for m in masks], [n], theta.cpu().unsqueeze(0).unsqueeze(0), mode)
    for a, r in zip(fuse_from(xs, masks, theta, mode, others, fill=nan), f64):
        assert_elementwise(a, r, f"w2comm_fuse_packed vs float64, {mode}, n={n}")


# ---- the module ------------------------------------------------------------------------------------------------------------------------------------------------------
def check_messages(messages, xs, masks, groups):
    off = 0
    for sent, n in zip(messages, groups):
        assert len(sent) == n - 1
        for j, msg in enumerate(sent, start=off + 1):
            assert isinstance(msg, W2Message) and msg.shapes == [tuple(x.shape[1:]) for x in xs] and msg.count.is_cuda
            for l, m in enumerate(masks):
                K = int(m[j].sum())
                assert int(msg.count[l]) == K
                assert torch.equal(msg.rows[l][:K], xs[l].permute(0, 2, 3, 1)[j][m[j].bool()]) and torch.equal(msg.masks()[l], m[j])
        off += n


@pytest.mark.parametrize("mode", ["ATTEN", "MAX"])
@pytest.mark.parametrize("multi_scale", [False, True])
def test_module_packed_wire_equals_the_default_route(multi_scale, mode):
    groups = [3, 1, 2]
    H, W = (16, 32) if multi_scale else (9, 14)
    psm, _, _, thre = mask_case(6, 2, H, W, 5, seed=80)
    m = module_of(mode, multi_scale, thre)
    xs = level_maps(6, 81) if multi_scale else [nhwc(student_t((6, 64, H, W), 81).to(DEV))]
    A = affine_of([make_thetas(n, H, W, seed=60 + n) for n in groups]).to(DEV)
    comm = m.naive_communication
    with torch.no_grad():
        want, want_rate = m.fuse_levels(xs, dev(psm), groups, A)
        got, rate, messages = m.fuse_levels(xs, dev(psm), groups, A, wire="packed")
        masks, _ = ops.w2comm_masks(dev(psm), groups, comm.gaussian_filter.weight.detach(), comm.gaussian_filter.bias.detach(), thre, levels=len(xs))
        if multi_scale:
            bb = decode_backbone().to(DEV)
            lv, rate2, sent2 = m.fuse(None, dev(psm), groups, A, bb, feats=xs, decode=False, wire="packed")
            out, _, extra = m.fuse(None, dev(psm), groups, A, bb, feats=xs, wire="packed")
            assert torch.equal(out, m.fuse(None, dev(psm), groups, A, bb, feats=xs)[0])
        else:
            masks = [m.frame_masks(masks[0], groups).contiguous()]
            out, rate2, extra = m.fuse(xs[0], dev(psm), groups, A, wire="packed")
            lv, sent2 = [out], extra["messages"]
    assert len(got) == len(want) == len(xs) and float(rate) == float(want_rate) == float(rate2)
    for a, b, c in zip(got, want, lv):
        assert torch.equal(a, b) and torch.equal(c, b)
    assert len(extra["messages"]) == len(sent2) == len(groups)
    check_messages(messages, xs, masks, groups)
    # the op-by-op statement of the format gives the same messages, bit for bit
    for sent, first in zip(messages, (0, 3, 4)):
        for j, msg in enumerate(sent, start=first + 1):
            ref = pack_messages_torch([x[j:j + 1].cpu() for x in xs], [mk[j:j + 1].cpu() for mk in masks])[0]
            assert torch.equal(msg.to_wire().cpu(), ref.to_wire()) and msg.nbytes == ref.nbytes == int(msg.nbytes_device())


def test_wire_round_trip_on_the_device_then_fuse():
    n, mode = 3, "ATTEN"
    xs, masks, theta = fuse_inputs(LEVELS, n, seed=31)
    masks[0][2].zero_()                                                                # agent 2 sends nothing at level 0
    m = module_of(mode, True, 0.3)
    sent = m.pack_messages([x[1:] for x in xs], [mk[1:] for mk in masks])
    direct = m.fuse_messages([x[:1] for x in xs], [mk[:1] for mk in masks], sent, theta)
    wires = [msg.to_wire() for msg in sent]
    assert all(w.is_cuda and w.dtype == torch.uint8 and w.numel() == msg.nbytes for w, msg in zip(wires, sent))
    assert sent[1].counts()[0] == 0 and sent[1].nbytes < sent[0].nbytes
    back = [W2Message.from_wire(w.cpu(), DEV) for w in wires]                          # (over a wire: through host memory)
    for a, b in zip(back, sent):
        assert torch.equal(a.count, b.count) and all(torch.equal(p, q) for p, q in zip(a.rank, b.rank)) and all(torch.equal(p, q) for p, q in zip(a.bits, b.bits))
    again = m.fuse_messages([x[:1] for x in xs], [mk[:1] for mk in masks], back, theta)
    want = ops.w2comm_fuse_nhwc(xs, masks, theta, MODES[mode])
    for a, b, c in zip(again, direct, want):
        assert torch.equal(a, b) and torch.equal(a, c)


@pytest.mark.parametrize("multi_scale", [False, True])
def test_packed_wire_under_graph_capture(multi_scale):
    groups = [3]
    H, W = (16, 32) if multi_scale else (9, 14)
    psm, _, _, thre = mask_case(3, 2, H, W, 5, seed=76)
    m = module_of("ATTEN", multi_scale, thre)
    xs = level_maps(3, 77) if multi_scale else [nhwc(student_t((3, 64, H, W), 77).to(DEV))]
    A = affine_of([make_thetas(3, H, W, seed=9)]).to(DEV)
    p = dev(psm)

    def run():
        lv, rate, messages = m.fuse_levels(xs, p, groups, A, wire="packed")
        sent = messages[0]
        return [*lv, rate, sum(msg.nbytes_device() for msg in sent), *[msg.count for msg in sent], *[b for msg in sent for b in msg.bits]]

    with torch.no_grad():
        run()
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            outs = run()
        seen = set()
        for seed in (1, 2):
            for x in xs:
                x.copy_(nhwc(student_t(tuple(x.shape), 100 * seed + x.shape[1]).to(DEV)))
            p.copy_(2 * torch.randn(p.shape, generator=torch.Generator().manual_seed(seed)).to(DEV) - 2)
            graph.replay()
            torch.cuda.synchronize()
            eager = run()
            for a, b in zip(outs, eager):
                assert torch.equal(a, b), seed
            for a, b in zip(outs[:len(xs)], m.fuse_levels(xs, p, groups, A)[0]):
                assert torch.equal(a, b), seed
            seen.add(int(outs[len(xs) + 1]))
        # multi scale: agent 1's mask follows the logits, so the inputs changed what was sent; single scale: every agent of the one frame carries the ego's
        # all-ones mask (``Where2comm.frame_masks``), so both agents send everything, whatever the logits
        assert len(seen) == 2 if multi_scale else seen == {2 * (64 + 4 * H * ((W + 31) // 32) + 4 * H * W * 64)}


# ---- the model -------------------------------------------------------------------------------------------------------------------------------------------------------
def test_model_with_and_without_the_packed_wire():
    h, model, anchors, frames, _ = _mini_world(2)
    assert model.packed_wire is False
    pp = build_postprocessor(h["postprocess"], False)
    eye = torch.eye(4, device=DEV)

    def detect(f):
        r = inference_intermediate_fusion({"ego": dict(f, anchor_box=anchors.to(DEV), transformation_matrix=eye)}, model, pp)
        return r["pred_box_tensor"], r["pred_score"]

    keys = list(model.state_dict())
    with torch.no_grad():
        want = [model(f) for f in frames]
        boxes = [detect(f) for f in frames]
        model.packed_wire = True
        try:
            got = [model(f) for f in frames]
            boxes_packed = [detect(f) for f in frames]
        finally:
            model.packed_wire = False
    assert list(model.state_dict()) == keys and sum(0 if b is None else b.shape[0] for b, _ in boxes) > 0
    for f, g, w, (gb, gs), (wb, ws) in zip(frames, got, want, boxes_packed, boxes):
        assert set(w) == {"cls_preds", "reg_preds", "dir_preds", "comm_rates"} and set(g) == set(w) | {"comm_bytes", "messages"}
        for k in w:
            assert torch.equal(g[k], w[k]), k
        assert (gb is None) == (wb is None) and (wb is None or (torch.equal(gb, wb) and torch.equal(gs, ws)))
        sent = g["messages"]
        assert len(sent) == 1 and len(sent[0]) == 2                                    # one frame, its two non-ego agents
        assert g["comm_bytes"].dtype == torch.int64 and g["comm_bytes"].dim() == 0 and g["comm_bytes"].is_cuda
        assert int(g["comm_bytes"]) == sum(msg.nbytes for msg in sent[0])
        # agent 2's masks are all ones (the even-agent rule): its message is the dense maps, the bitmaps and the header
        full = sent[0][1]
        assert full.nbytes == 64 + sum(4 * H * ((W + 31) // 32) + 4 * H * W * C for C, H, W in full.shapes) == len(full.to_wire())
        assert sent[0][0].nbytes < full.nbytes and sent[0][0].counts()[0] == int(sent[0][0].masks()[0].sum())
