"""Online pose correction, host side (no GPU): the extension header include/coalign_amd_align.h against the product library and ``hip.ALIGN_SIGNATURES``,
argument validation before any HIP call, ops / ``PoseCorrector`` refusing CPU tensors, and ``inference_intermediate_fusion_aligned`` without a corrector."""
import ctypes
import os
import re
import types

import pytest
import torch

import abi_headers
from coalign_amd import box_align, hip, inference, ops

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NULL, ONE = ctypes.c_void_p(0), ctypes.c_void_p(16)      # (a non-NULL token: none of these calls gets as far as touching memory)

HEADER = "coalign_amd_align.h"
C_TYPES = {"int": ctypes.c_int, "double": ctypes.c_double, "size_t": ctypes.c_size_t}


def test_align_header_table_and_library_agree():
    """Every name of include/coalign_amd_align.h is exported by the product library and equals ``hip.ALIGN_SIGNATURES``, argument types included (every pointer of
    this header, host or device, crosses as ``hip.P``: its own mapping, not the rule of tests/abi_headers.py); the header includes coalign_amd.h and cites the
    reference lines each entry point replaces."""
    text = open(abi_headers.path(HEADER)).read()
    assert '#include "coalign_amd.h"' in text
    declared = abi_headers.declarations(HEADER)
    assert set(declared) == set(hip.ALIGN_SIGNATURES) and len(declared) == 4
    lib = hip.lib()
    for name, (res, args) in declared.items():
        args = [hip.P if "*" in a else C_TYPES[a.split()[-2]] for a in args]
        fn = getattr(lib, name)
        assert hip.ALIGN_SIGNATURES[name][0] is res and hip.ALIGN_SIGNATURES[name][1] == args, name
        assert fn.restype is res and list(fn.argtypes) == args, name
    comments = re.findall(r"/\*.*?\*/", text, flags=re.S)
    cites = {"coalign_stage1_gather": "uncertainty_voxel_postprocessor.py:26-112", "coalign_pose_graph_build": "box_align_v2.py:150-372",
             "coalign_pose_correct_matrices": "transformation_utils.py:22-67"}
    for name, cite in cites.items():
        last = [c for c in comments if c in text[:text.index(name + "(")]][-1]
        assert cite in last, name
    assert lib.coalign_align_store_boxes() >= 256


def _build(n_samples=1, n_agents=2, corners=ONE, unc=ONE, wide=0, udim=3, count=ONE, noisy=ONE, flags=3, outs=ONE, status=ONE):
    return hip.lib().coalign_pose_graph_build(n_samples, n_agents, corners, unc, wide, udim, count, noisy, flags, 1.5, 0.2, *([outs] * 9), status, NULL)


def _gather(keep=ONE, capacity=100, unc=ONE, A=2, udim=3, H=8, W=8, slot=0, store=ONE, status=ONE):
    return hip.lib().coalign_stage1_gather(keep, ONE, ONE, ONE, capacity, unc, A, udim, H, W, slot, store, store, store, status, NULL)


def _matrices(n_samples=1, n_agents=2, noisy=ONE, max_cav=5, H=100, W=252, den=100.8, out=ONE):
    return hip.lib().coalign_pose_correct_matrices(n_samples, n_agents, noisy, ONE, ONE, max_cav, 0, H, W, den, den, out, out, out, NULL)


def test_align_argument_validation_without_a_gpu():
    """NULL pointers -1, negative sizes -2, more than 8 agents / slots, an uncertainty dimension above 3 or max_cav above 16 -3, zero samples 0 without a launch:
    all before any HIP call."""
    assert _build(n_samples=0) == 0 and _build(n_samples=0, corners=NULL, outs=NULL) == 0 and _matrices(n_samples=0) == 0
    for arg in ("corners", "count", "noisy", "outs", "status"):
        assert _build(**{arg: NULL}) == -1, arg
    assert _build(n_samples=-1) == -2 and _build(n_agents=0) == -2 and _build(n_agents=-3) == -2 and _build(udim=-1) == -2 and _build(flags=-1) == -2
    assert _build(n_agents=9) == -3 and _build(udim=4) == -3 and _build(wide=2) == -3 and _build(flags=128) == -3
    assert _gather(keep=NULL) == -1 and _gather(store=NULL) == -1 and _gather(status=NULL) == -1 and _gather(unc=NULL) == -1
    assert _gather(capacity=0) == -2 and _gather(A=0) == -2 and _gather(H=-1) == -2 and _gather(slot=-1) == -2 and _gather(udim=-1) == -2
    assert _gather(slot=8) == -3 and _gather(udim=4) == -3
    assert _matrices(noisy=NULL) == -1 and _matrices(out=NULL) == -1
    assert _matrices(n_samples=-1) == -2 and _matrices(n_agents=0) == -2 and _matrices(H=0) == -2 and _matrices(den=0.0) == -2 and _matrices(n_agents=6, max_cav=5) == -2
    assert _matrices(n_agents=9, max_cav=12) == -3 and _matrices(max_cav=17) == -3


def test_align_ops_refuse_cpu_tensors():
    """No CPU fallback: the new ops and ``PoseCorrector.correct`` raise ``CoalignHipError`` on CPU tensors."""
    store, graph = ops.Stage1Store("cpu"), ops.PoseGraphArrays("cpu")
    poses = torch.zeros(2, 6, dtype=torch.float64)
    with pytest.raises(hip.CoalignHipError):
        ops.pose_graph_build(store, poses, graph, ops.align_flags())
    with pytest.raises(hip.CoalignHipError):
        ops.pose_graph_solve(graph)
    with pytest.raises(hip.CoalignHipError):
        ops.pose_correct_matrices(poses, graph.vertices, store.status, 5, 100, 252, 100.8, 40.0, False, torch.zeros(2, 6, dtype=torch.float64),
                                  torch.zeros(1, 5, 5, 4, 4, dtype=torch.float64), torch.zeros(1, 5, 5, 2, 3, dtype=torch.float64))
    with pytest.raises(hip.CoalignHipError):
        ops.stage1_gather(types.SimpleNamespace(counts=torch.zeros(64, dtype=torch.int32), dec_A=2, dec_HW=(8, 8)), torch.zeros(6, 8, 8), store, 0)
    corrector = box_align.PoseCorrector({"abandon_hard_cases": True, "drop_hard_boxes": True}, 5, 100, 252, 0.4, 2, device="cpu")
    with pytest.raises(hip.CoalignHipError):
        corrector.correct(None, poses)
    assert ops.align_flags(abandon_hard_cases=True, use_uncertainty=False) == 2 + 16
    with pytest.raises(ValueError):
        ops.align_flags(no_such_flag=True)


class _Raises:
    def __call__(self, *a, **k):
        raise AssertionError("a stage-1 object was touched without a corrector")

    def __getattr__(self, name):
        raise AssertionError(f"a stage-1 object was touched without a corrector ({name})")


def test_aligned_inference_without_a_corrector_is_the_plain_driver():
    """``corrector=None``: neither stage-1 object is touched, and the model and post-processor are called exactly as ``inference_intermediate_fusion`` calls them."""
    class Model:
        def __init__(self):
            self.calls = []

        def __call__(self, data):
            self.calls.append(data)
            return {"cls_preds": torch.zeros(1)}

    class Post:
        def __init__(self):
            self.calls = []

        def post_process(self, data, out):
            self.calls.append((data, out))
            return torch.ones(2, 8, 3), torch.ones(2)

    batch = {"ego": {"processed_lidar": {}, "record_len": [2], "lidar_poses": torch.zeros(2, 6)}}
    gt = torch.zeros(1, 8, 3)
    m1, p1, m2, p2 = Model(), Post(), Model(), Post()
    plain = inference.inference_intermediate_fusion(batch, m1, p1, gt)
    aligned = inference.inference_intermediate_fusion_aligned(batch, m2, p2, stage1_model=_Raises(), stage1_post_processor=_Raises(), corrector=None, gt_box_tensor=gt)
    assert set(plain) == set(aligned)
    assert len(m1.calls) == len(m2.calls) == 1 and m1.calls[0] is m2.calls[0] is batch["ego"]
    assert len(p1.calls) == len(p2.calls) == 1 and p2.calls[0][0] is batch and list(p2.calls[0][1]) == ["ego"]
    for k in plain:
        assert torch.equal(plain[k], aligned[k]), k
