"""The references of tests/test_postprocess_limits_gpu.py, checked on their own (no GPU): for every case of that file the float32 oracle
(``oracle.decode_candidates`` + the two sanity filters) and the float64 restatement ``postprocess_cases.decode_f64`` select the same anchors in the
same order and agree on the keep flag, the score-margin, discontinuity and keep-edge conditions hold within their caps, the float32 oracle stays
within the decode tolerances of float64 (scores rtol 3e-7; box7 rtol 2e-6 + 2e-6; corners rtol 2e-6 + 4e-6), and the oracle's filters drop every
non-finite candidate.  What the GPU file then asks of the kernel is therefore something the reference's own float32 evaluation meets.
"""
import numpy as np
import pytest
import torch

import postprocess_cases as pc
from oracle import coalign_oracle as oracle


def check_reference(case, idx, scores, box7, corners, keep, f64, what):
    assert torch.equal(idx, f64["idx"]), f"{what}: the float32 oracle and float64 select different anchors"
    assert torch.equal(idx, torch.nonzero(case.passing).view(-1)), f"{what}: selection differs from the case's passing mask"
    assert torch.equal(keep, f64["keep"]), f"{what}: keep flags differ at {torch.nonzero(keep != f64['keep']).view(-1).tolist()}"
    p = torch.sigmoid(case.cls.double())
    assert bool(((p - pc.THR).abs() > pc.MARGIN).all()), f"{what}: a score inside the margin"
    rows, left_out = pc.value_rows(f64)
    assert left_out <= pc.MAX_LEFT_OUT * len(idx), f"{what}: {left_out} of {len(idx)} candidates on a limit_period discontinuity"
    fin = pc.finite_rows(f64)
    if bool(fin.any()):
        assert float(f64["keep_slack"][fin].min()) > pc.KEEP_SLACK, f"{what}: a candidate sits on an edge of the sanity filters"
    np.testing.assert_allclose(scores.numpy(), f64["scores"].numpy(), rtol=pc.SCORE_RTOL, atol=0)
    if bool(rows.any()):
        d7 = box7.double()[rows] - f64["box7"][rows]
        d7[:, 6] = pc.wrap_yaw(d7[:, 6])
        assert bool((d7.abs() <= pc.BOX7_TOL["atol"] + pc.BOX7_TOL["rtol"] * f64["box7"][rows].abs()).all()), f"{what}: box7, worst {float(d7.abs().max()):.3e}"
        dc = corners.double()[rows] - f64["corners"][rows]
        assert bool((dc.abs() <= pc.CORNER_TOL["atol"] + pc.CORNER_TOL["rtol"] * f64["corners"][rows].abs()).all()), f"{what}: corners, worst {float(dc.abs().max()):.3e}"
    return pc.error_vs_f64(box7, corners, f64, rows)


@pytest.mark.parametrize("s", pc.ALL_DECODE_SPECS, ids=pc.spec_id)
def test_decode_references_agree(s):
    r = pc.reference(s)
    err = check_reference(r.case, r.idx, r.scores, r.box7, r.corners, r.keep, r.f64, pc.spec_id(s))
    assert err <= 1e-6, "the float32 oracle's error against float64 is a few roundings of the candidate's scale"


def test_spec_ids_are_unique_and_every_mechanism_is_present():
    ids = [pc.spec_id(s) for s in pc.ALL_DECODE_SPECS]
    assert len(set(ids)) == len(ids)
    for A, H, W in pc.BIG:
        assert (A * H * W + 255) // 256 == 257
        r = pc.reference(pc.spec(A, H, W, pc._seed(A, H, W, 9), "blocks", transform="identity"))
        i = r.idx.numpy()
        assert (i < 256).any() and (i >= 256 * 256).any() and i[-1] == A * H * W - 1
    seam = pc.reference(next(s for s in pc.VALUE_SPECS if s.density == "seam" and (s.A, s.H, s.W) == (3, 7, 13)))
    assert seam.idx.tolist() == [63, 64]
    ties = [pc.reference(s) for s in pc.OPTION_SPECS if s.tie_dir]
    assert len(ties) == 4 and all(len(r.idx) == 273 for r in ties)


@pytest.mark.parametrize("s", pc.NONFINITE_SPECS, ids=pc.spec_id)
def test_oracle_filters_drop_every_nonfinite_candidate(s):
    r = pc.reference(s)
    bad = ~pc.finite_rows(r.f64)
    assert int(bad.sum()) == len(pc.NONFINITE[s.nonfinite]), "every directed candidate is selected and non-finite"
    assert not bool(r.keep[bad].any()) and not bool(r.f64["keep"][bad].any())
    assert bool(r.keep[~bad].any()), "ordinary candidates around them are kept"
    nonfin32 = ~(torch.isfinite(r.corners).reshape(len(r.idx), -1).all(dim=1) & torch.isfinite(r.box7).all(dim=1))
    assert torch.equal(nonfin32, bad), "float32 and float64 agree on which candidates are non-finite"


@pytest.mark.parametrize("name", sorted(pc.FRAME_SPECS))
def test_whole_chain_frames(name):
    """The frames of the VoxelPostprocessor cases: per agent the same checks as above (on the configuration's anchors), every stage of the chain
    non-trivial, and in the non-finite frame the sanity filters are what removes the directed candidates."""
    agents, anchors, boxes, scores, info = pc.frame(name)
    cfg = pc.mini_postprocess_config()
    da = cfg["dir_args"]
    n_bad = 0
    for s, ag in zip(pc.FRAME_SPECS[name], agents):
        case = pc.make_case(s, anchors)
        idx, box7, sc, corners, keep = pc.oracle_decode(case)
        f64 = pc.decode_f64(case.cls, case.reg, case.dir, anchors, pc.THR, cfg["order"], da["dir_offset"], da["num_bins"], case.transform)
        check_reference(case, idx, sc, box7, corners, keep, f64, f"{name} {pc.spec_id(s)}")
        bad = ~pc.finite_rows(f64)
        n_bad += int(bad.sum())
        assert not bool(keep[bad].any())
    n_cand, n_valid, n_kept, n_final = len(info["cand_index"]), int(info["keep_filter"].sum()), len(info["keep_nms"]), int(info["keep_range"].sum())
    assert n_cand > n_valid > n_kept > n_final > 0, (n_cand, n_valid, n_kept, n_final)
    assert n_bad == (6 if name == "nonfinite" else 0)            # three directed candidates in each of the two agents
    assert boxes.shape[0] == n_final and bool(torch.isfinite(boxes).all())
    s_kept = info["cand_scores"][info["keep_filter"]]
    assert len(torch.unique(s_kept)) == len(s_kept), "distinct scores: the NMS order does not hang on the tie rule"
