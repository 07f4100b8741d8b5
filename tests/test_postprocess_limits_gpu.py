"""Anchor decode (csrc/decode.hip) and the post-processing chain behind it at their limits, through ``ops.anchor_decode`` and the C ABI.

Yardsticks (tests/postprocess_cases.py builds the cases; tests/test_postprocess_cases_cpu.py shows that the references alone meet every cap and
tolerance used here):
  * selection, order, ``cand_index``, the count word and ``cand_keep`` are EXACTLY the float32 oracle's (``oracle.decode_candidates`` + the two
    sanity filters);
  * scores, ``cand_box7`` (yaw modulo 2 * pi) and ``cand_corners`` are within the existing decode tolerances of the float32 oracle (scores rtol 3e-7;
    box7 rtol 2e-6 + 2e-6; corners rtol 2e-6 + 4e-6);
  * against the float64 restatement ``decode_f64``: per candidate err = max |value - float64| / scale, scale = the largest |coordinate| of its corners
    before and after the projection (at least 1); the kernel's maximum err is at most 4x the float32 oracle's on the same case + 1e-7 -- both are
    valid float32 evaluations that differ in libm and in the order of the projection's sum, the factor 4 is head-room for a maximum over ~1000
    samples.  Scores: the kernel's sigmoid is a float64 evaluation rounded once, i.e. within 6e-8 of float64.
  * candidates on a ``limit_period`` discontinuity (floor argument within 1e-5 of an integer; at most 1 % of a case) are left out of the value
    comparisons only; non-finite rows are compared in selection, index, score and keep flag only;
  * every buffer is pre-filled with sentinel bytes: rows at or beyond the written count keep them bit for bit.

Kernel / float32-oracle max-error ratios: every case prints its ``DECODE-RATIO`` line (``pytest -s``).  NOT YET MEASURED on the MI355X: this file
was written, and its references and test logic checked on the host (tests/test_postprocess_cases_cpu.py), without a GPU run; the largest ratios
belong here after the first one.  The float32 oracle's own error on these cases is at most 2.4e-7 of the scale (the two 65 536-candidate cases).
"""
import numpy as np
import pytest
import torch

import postprocess_cases as pc
from coalign_amd import ops
from coalign_amd.postprocess import PostProcessHandle, build_postprocessor
from oracle import coalign_oracle as oracle

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = 0xA5
THR = pc.THR


# ------------------------------------------------------------------------------------------------ running the kernel
def new_buffers(A, H, W, rows):
    """DecodeBuffers with ``rows`` allocated candidate rows (callers lower ``buf.capacity`` afterwards, never raise it), every candidate array
    filled with sentinel bytes."""
    buf = ops.DecodeBuffers(max(1, rows), A, H, W, 1000, DEV)
    for t in candidate_arrays(buf):
        t.view(torch.uint8).fill_(SENTINEL)
    return buf


def candidate_arrays(buf):
    return (buf.cand_index, buf.cand_score, buf.cand_box7, buf.cand_corners, buf.cand_keep)


def decode(buf, slot, case, clear_frame=False):
    s = case.spec
    T = None if case.transform is None else case.transform.to(DEV)
    ops.anchor_decode(buf, slot, case.cls.to(DEV), case.reg.to(DEV), None if case.dir is None else case.dir.to(DEV),
                      case.anchors.reshape(-1, 7).float().to(DEV), THR, s.dir_offset, s.num_bins, s.order, T, clear_frame=clear_frame)


def snapshot(buf):
    """The candidate arrays as raw bytes on the host (bit-for-bit comparisons, NaN included), and the 67 frame words."""
    torch.cuda.synchronize()
    return [t.reshape(t.shape[0], -1).view(torch.uint8).cpu().clone() for t in candidate_arrays(buf)], buf.frame_words.cpu().clone()


def assert_untouched(snap, lo, hi=None, what=""):
    for name, t in zip(("cand_index", "cand_score", "cand_box7", "cand_corners", "cand_keep"), snap[0]):
        assert bool((t[lo:hi] == SENTINEL).all()), f"{what}: {name} written in rows [{lo}, {hi})"


def rows_of(buf, lo, hi):
    return (buf.cand_index[lo:hi].cpu().long(), buf.cand_score[lo:hi].cpu(), buf.cand_box7[lo:hi].cpu(), buf.cand_corners[lo:hi].cpu(),
            buf.cand_keep[lo:hi].cpu())


def check_rows(got, ref, n, what, values=True):
    """Rows ``got`` = (index, score, box7, corners, keep) against the first ``n`` candidates of the reference ``ref``."""
    idx, score, box7, corners, keep = got
    assert torch.equal(idx, ref.idx[:n]), f"{what}: selection / order"
    assert bool(((keep == 0) | (keep == 1)).all()) and torch.equal(keep.bool(), ref.keep[:n]), \
        f"{what}: cand_keep differs at candidates {torch.nonzero(keep.bool() != ref.keep[:n]).view(-1).tolist()[:8]}"
    f64 = {k: v[:n] for k, v in ref.f64.items()}
    sub = pc.Ref(ref.case, ref.idx[:n], ref.scores[:n], ref.box7[:n], ref.corners[:n], ref.keep[:n], f64)
    rows, left_out = pc.value_rows(f64)
    assert left_out <= pc.MAX_LEFT_OUT * max(n, 1), f"{what}: {left_out} of {n} candidates on a discontinuity"
    if not values:
        rows = rows & False
    pc.assert_values_close(score, box7, corners, sub, rows, what)
    if n:
        assert float((score.double() - f64["scores"]).abs().max()) <= 6e-8, f"{what}: sigmoid is not a correctly rounded float32"
    err = pc.error_vs_f64(box7, corners, f64, rows)
    err32 = pc.error_vs_f64(sub.box7, sub.corners, f64, rows)
    print(f"DECODE-RATIO {what}: n {n} compared {int(rows.sum())} kernel {err:.3e} float32-oracle {err32:.3e} ratio {err / max(err32, 1e-30):.3f}")
    assert err <= 4 * err32 + 1e-7, f"{what}: kernel error {err:.3e} of the scale, float32 oracle {err32:.3e}"


def run_value_case(s):
    ref = pc.reference(s)
    n, total = len(ref.idx), s.A * s.H * s.W
    buf = new_buffers(s.A, s.H, s.W, total + 3)
    buf.capacity = total
    buf.reset_frame()
    decode(buf, 0, ref.case)
    snap = snapshot(buf)
    words = snap[1]
    assert int(words[1]) == n, f"count word {int(words[1])}, reference {n}"
    assert int(words[0]) == 0 and int(words[64]) == 0 and not bool(words[2:64].any()) and not bool(words[65:].any())
    check_rows(rows_of(buf, 0, n), ref, n, pc.spec_id(s))
    assert_untouched(snap, n, None, pc.spec_id(s))
    return buf, ref


# ------------------------------------------------------------------------------------------------ shapes x densities, options
@pytest.mark.parametrize("s", pc.VALUE_SPECS, ids=pc.spec_id)
def test_decode_shapes_and_densities(s):
    """One anchor, less than a wavefront, one exact block, one lane into a second block, A = 3 ragged, and the two 257-block shapes (the second trip
    of emit_kernel's block_counts loop, with and without a partial last block) x nothing / everything / 2 % / only the first / only the last anchor /
    lanes 63 and 64 of every block passing."""
    run_value_case(s)


@pytest.mark.parametrize("s", pc.OPTION_SPECS, ids=pc.spec_id)
def test_decode_options(s):
    """Order hwl / lhw x dir present / NULL x transform NULL / identity / rigid with a large translation / general without a zero entry; num_bins
    1 / 2 / 4 x dir_offset 0.7853 / 0; equal direction logits (the lowest bin wins)."""
    run_value_case(s)


# ------------------------------------------------------------------------------------------------ capacity
@pytest.mark.parametrize("short", [0, 1, "all"])
def test_decode_capacity_and_overflow_flag(short):
    s = pc.CAPACITY_SPEC
    ref = pc.reference(s)
    n = len(ref.idx)
    assert n > 64
    cap = 0 if short == "all" else n - short
    buf = new_buffers(s.A, s.H, s.W, n + 8)
    buf.capacity = cap
    buf.reset_frame()
    decode(buf, 0, ref.case)
    snap = snapshot(buf)
    assert int(snap[1][1]) == cap, "the count is clamped to capacity"
    assert int(snap[1][64]) == (1 if cap < n else 0), "COALIGN_FLAG_CANDIDATE_OVERFLOW iff more candidates than capacity"
    check_rows(rows_of(buf, 0, cap), ref, cap, f"capacity {cap} of {n}")
    assert_untouched(snap, cap, None, f"capacity {cap} of {n}")


def test_decode_capacity_zero_without_candidates():
    s = pc.spec(3, 7, 13, 5, "none")
    buf = new_buffers(s.A, s.H, s.W, 8)
    buf.capacity = 0
    buf.reset_frame()
    decode(buf, 0, pc.reference(s).case)
    snap = snapshot(buf)
    assert not bool(snap[1].any()), "no candidate, no capacity: count 0 and no flag"
    assert_untouched(snap, 0)


# ------------------------------------------------------------------------------------------------ chaining
def test_decode_chain_of_three_agents():
    refs = [pc.reference(s) for s in pc.CHAIN_SPECS]
    ns = [len(r.idx) for r in refs]
    s = pc.CHAIN_SPECS[0]
    buf = new_buffers(s.A, s.H, s.W, sum(ns) + 8)
    buf.capacity = sum(ns)
    buf.reset_frame()
    starts = np.concatenate([[0], np.cumsum(ns)])
    before = None
    for slot, ref in enumerate(refs):
        decode(buf, slot, ref.case)
        snap = snapshot(buf)
        assert snap[1][:4].tolist()[: slot + 2] == starts[: slot + 2].tolist(), "counts[1 .. slot + 1] are the running totals"
        assert not bool(snap[1][slot + 2:].any())
        if before is not None:
            for a, b in zip(before[0], snap[0]):
                assert torch.equal(a[: starts[slot]], b[: starts[slot]]), "earlier agents' rows changed by a later call"
        check_rows(rows_of(buf, int(starts[slot]), int(starts[slot + 1])), ref, ns[slot], f"chain agent {slot}")
        assert_untouched(snap, int(starts[slot + 1]), None, f"chain agent {slot}")
        before = snap


def test_decode_chain_overflows_in_the_middle_of_a_block():
    refs = [pc.reference(s) for s in pc.CHAIN_SPECS]
    ns = [len(r.idx) for r in refs]
    assert ns[1] == 273 and ns[2] > 0
    part = 100                                              # agent 1 passes everywhere: its row 100 is lane 36 of wave 1 of block 0
    cap = ns[0] + part
    s = pc.CHAIN_SPECS[0]
    buf = new_buffers(s.A, s.H, s.W, sum(ns) + 8)
    buf.capacity = cap
    buf.reset_frame()
    decode(buf, 0, refs[0].case)
    assert snapshot(buf)[1][[1, 64]].tolist() == [ns[0], 0]
    decode(buf, 1, refs[1].case)
    snap1 = snapshot(buf)
    assert snap1[1][[1, 2, 64]].tolist() == [ns[0], cap, 1], "agent 1 is truncated at capacity and raises the flag"
    check_rows(rows_of(buf, 0, ns[0]), refs[0], ns[0], "agent 0 under a later overflow")
    check_rows(rows_of(buf, ns[0], cap), refs[1], part, "agent 1 truncated")
    assert_untouched(snap1, cap, None, "agent 1 truncated")
    decode(buf, 2, refs[2].case)
    snap2 = snapshot(buf)
    assert snap2[1][[1, 2, 3, 64]].tolist() == [ns[0], cap, cap, 1], "agent 2 behind a full buffer: nothing written, the flag stays"
    assert all(torch.equal(a, b) for a, b in zip(snap1[0], snap2[0])), "agent 2 wrote candidate rows"


# ------------------------------------------------------------------------------------------------ first-launch clear
def test_decode_first_clears_the_frame_words():
    s = pc.CLEAR_SPEC
    ref = pc.reference(s)
    n, total = len(ref.idx), s.A * s.H * s.W
    plain = new_buffers(s.A, s.H, s.W, total)
    plain.reset_frame()
    decode(plain, 0, ref.case)
    want = snapshot(plain)
    first = new_buffers(s.A, s.H, s.W, total)
    first.frame_words.fill_(0x5A5A5A5A)
    decode(first, 0, ref.case, clear_frame=True)
    got = snapshot(first)
    expect = torch.zeros(67, dtype=torch.int32)
    expect[1] = n
    assert torch.equal(got[1], expect), "all 67 frame words are 0 except counts[1]"
    assert torch.equal(want[1], expect)
    assert all(torch.equal(a, b) for a, b in zip(got[0], want[0])), "clear_frame decode differs from reset_frame + plain decode"
    with pytest.raises(ValueError):
        decode(first, 1, ref.case, clear_frame=True)
    torch.cuda.synchronize()
    assert torch.equal(first.frame_words.cpu(), expect)


# ------------------------------------------------------------------------------------------------ non-finite regression values
@pytest.mark.parametrize("s", pc.NONFINITE_SPECS, ids=pc.spec_id)
def test_decode_nonfinite_candidates_are_not_kept(s):
    """A NaN delta, a size delta of 100 (expf overflows; under a transform 0 * inf = NaN) and a +inf z delta on high-score anchors among ordinary
    ones, with transform NULL and the identity: selection, index, score and cand_keep are the oracle's -- whose torch.max / torch.min propagate
    NaN, so that every such candidate is dropped.  (fminf / fmaxf return the non-NaN operand: before the NaN rule of decode_and_store a candidate
    with all-NaN corners kept its initial +-inf extents, passed both filters and entered the NMS as valid.)  Ordinary rows: all values as usual."""
    buf, ref = run_value_case(s)
    bad = ~pc.finite_rows(ref.f64)
    assert int(bad.sum()) == len(pc.NONFINITE[s.nonfinite])
    assert not bool(buf.cand_keep[: len(ref.idx)].cpu().bool()[bad].any())


# ------------------------------------------------------------------------------------------------ the whole chain through VoxelPostprocessor
def _frame_dicts(agents, anchors):
    data = {f"a{i}": {"transformation_matrix": ag["transformation_matrix"], "anchor_box": anchors} for i, ag in enumerate(agents)}
    outd = {f"a{i}": {k: v.to(DEV) for k, v in ag.items() if k.endswith("_preds")} for i, ag in enumerate(agents)}
    return data, outd


@pytest.mark.parametrize("name", sorted(pc.FRAME_SPECS))
def test_voxel_postprocessor_frames_vs_oracle(name):
    """Two and three cavs with transforms, and a frame with non-finite high-score candidates: final boxes and scores at the tolerances of
    test_post_process_golden, candidates / kept / final exactly the oracle's (a non-finite candidate that enters the NMS as valid shows as kept + 1)."""
    agents, anchors, boxes, scores, info = pc.frame(name)
    pp = build_postprocessor(pc.mini_postprocess_config(), False)
    got_b, got_s = pp.post_process(*_frame_dicts(agents, anchors))
    want = {"candidates": len(info["cand_index"]), "kept": len(info["keep_nms"]), "final": int(info["keep_range"].sum())}
    assert pp.last_counts == want
    assert got_b.shape == boxes.shape
    np.testing.assert_allclose(got_s.cpu().numpy(), scores.numpy(), rtol=3e-7, atol=0)
    np.testing.assert_allclose(got_b.cpu().numpy(), boxes.numpy(), rtol=2e-6, atol=1e-5)


def _handle(pp, buf):
    done = torch.cuda.Event()
    done.record()
    return PostProcessHandle(pp, buf, done)


def test_voxel_postprocessor_overflow_raises_and_empty_frame_is_none():
    agents, anchors, _, _, info = pc.frame("three_cavs")
    total = len(info["cand_index"])
    A, H, W = pc.MINI
    pp = build_postprocessor(pc.mini_postprocess_config(), False)
    buf = new_buffers(A, H, W, total + 8)
    buf.capacity = total - 5
    pp.enqueue(*_frame_dicts(agents, anchors), buf)
    with pytest.raises(RuntimeError, match="overflow"):
        _handle(pp, buf).result()
    assert int(buf.host[3]) == total - 5 and int(buf.host[64]) == 1
    assert_untouched(snapshot(buf), total - 5)
    buf.capacity = total                                   # the same buffers, next frame: the first decode clears the flag
    pp.enqueue(*_frame_dicts(agents, anchors), buf)
    b, s = _handle(pp, buf).result()
    assert pp.last_counts["candidates"] == total and b.shape[0] == int(info["keep_range"].sum())
    pp.enqueue({}, {}, buf)                                # no cav at all
    assert _handle(pp, buf).result() == (None, None)
    assert pp.last_counts == {"candidates": 0, "kept": 0, "final": 0}


# ------------------------------------------------------------------------------------------------ NMS on the reused buffers, the range limit
def _axis_box(x0, x1, y0, y1, z0=-1.0, z1=0.0):
    xy = [(x1, y0), (x1, y1), (x0, y1), (x0, y0)]
    return torch.tensor([[x, y, z] for z in (z0, z1) for x, y in xy], dtype=torch.float32)


def _both_gather_paths(corners, scores, valid, k_dev, rng, top=1000):
    """coalign_nms_rotated_gather and coalign_nms_rotated + coalign_gather_in_range on the same inputs -> (keep list, gathered corners, scores) twice."""
    c, s, v = corners.to(DEV), scores.to(DEV), None if valid is None else valid.to(DEV)
    kd = None if k_dev is None else torch.tensor([k_dev], dtype=torch.int32, device=DEV)
    ws = torch.empty(ops.hip.lib().coalign_nms_rotated_workspace_bytes(c.shape[0], top), dtype=torch.uint8, device=DEV)
    out = []
    for fused in (True, False):
        keep = torch.full((top,), -1, dtype=torch.int32, device=DEV)
        cnt = torch.zeros(1, dtype=torch.int32, device=DEV)
        oc, osc, on = torch.zeros(top, 8, 3, device=DEV), torch.zeros(top, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)
        if fused:
            ops.nms_rotated_gather(c, s, 0.15, top, v, kd, keep, cnt, rng, oc, osc, on, ws)
        else:
            ops.nms_rotated_device(c, s, 0.15, top, valid=v, k_dev=kd, keep=keep, keep_count=cnt, ws=ws)
            ops.gather_in_range(c, s, keep, cnt, rng, oc, osc, on)
        n, m = int(cnt), int(on)
        out.append((keep[:n].cpu().numpy(), oc[:m].cpu(), osc[:m].cpu()))
    return out


@pytest.mark.parametrize("what", ["stale_tail", "range_edge"])
def test_nms_on_reused_buffers_and_at_the_range_limit(what):
    """stale_tail: a device candidate count below the buffer's rows, the rows beyond it holding top scores, valid = 1 and NaN corners -- the state the
    reused candidate buffers are in every frame.  range_edge: a kept box with a corner at float32(140.8) = 140.80000305... against the limit 140.8
    (compared in float64: outside), a second box exactly on the representable limit 40.0 (inside)."""
    if what == "stale_tail":
        rs = np.random.RandomState(11)
        K, k_dev = 300, 200
        b7 = np.zeros((K, 7), np.float32)
        b7[:, 0] = rs.uniform(-30, 30, K); b7[:, 1] = rs.uniform(-12, 12, K); b7[:, 2] = -1; b7[:, 3] = 1.5
        b7[:, 4] = rs.uniform(1.4, 2.2, K); b7[:, 5] = rs.uniform(3, 5.5, K); b7[:, 6] = rs.uniform(-3.2, 3.2, K)
        corners = oracle.boxes_to_corners_3d(torch.from_numpy(b7), "hwl")
        scores = torch.from_numpy(rs.uniform(0.2, 1, K).astype(np.float32))
        valid = torch.from_numpy((rs.uniform(0, 1, K) > 0.1).astype(np.uint8))
        corners[k_dev:] = float("nan")
        scores[k_dev:] = 2.0
        valid[k_dev:] = 1
        rng = [-25.0, -10.0, -3.0, 25.0, 10.0, 1.0]
    else:
        k_dev = None
        edge = float(np.float32(140.8))
        assert edge > 140.8
        corners = torch.stack([_axis_box(136.0, edge, 0.0, 2.0), _axis_box(0.0, 4.0, 38.0, 40.0), _axis_box(-10.0, -6.0, -1.0, 1.0),
                               _axis_box(-140.0, -136.0, -40.0, -38.0)])
        assert float(corners[0, :, 0].max()) == edge and float(corners[1, :, 1].max()) == 40.0
        scores = torch.tensor([0.9, 0.8, 0.7, 0.6])
        valid = torch.ones(4, dtype=torch.uint8)
        rng = list(pc.RANGE)
    live = corners.shape[0] if k_dev is None else k_dev
    idx = np.nonzero(valid.numpy()[:live])[0]
    want = idx[oracle.nms_rotated(corners.numpy()[idx], scores.numpy()[idx], 0.15)].astype(np.int32)
    inside = want[oracle.mask_boxes_outside_range(corners.numpy()[want].astype(np.float64), rng)]
    if what == "range_edge":
        assert want.tolist() == [0, 1, 2, 3] and inside.tolist() == [1, 2, 3]
    else:
        assert 0 < len(inside) < len(want) < len(idx)
    for keep, oc, osc in _both_gather_paths(corners, scores, valid, k_dev, rng):
        assert np.array_equal(keep, want)
        assert torch.equal(oc, corners[inside]) and torch.equal(osc, scores[inside])
