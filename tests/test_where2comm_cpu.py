"""Where2comm, host side (no GPU): the extension header include/coalign_amd_where2comm.h against the product library and ``hip.W2COMM_SIGNATURES``, argument
refusals before any HIP call, ``fusion.Where2commFusion``'s op-by-op route against the reference's recorded outputs, masks and rates
(tests/golden/where2comm_fuse.npz, written by tests/golden/make_where2comm_golden.py) and against the float64 restatement of tests/where2comm_reference.py, the
even-agent quirk, the refusals, the route plan and ``build_model`` on both configs."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import abi_headers
from conftest import assert_elementwise
from coalign_amd import fusion, hip, opencood_compat, ops, routes, where2comm
from coalign_amd.backbone import BaseBEVBackbone, ResNetBEVBackbone
from coalign_amd.config import builtin_config
from coalign_amd.detector import BASELINE_REGISTRY, PointPillarWhere2comm, build_model
from coalign_amd.fusion import Where2commFusion
from coalign_amd.pose import normalize_pairwise_tfm
from where2comm_reference import check_mask_inputs, gaussian_weight, mask_case, masks_f64, rate_of, single_scale_masks, where2comm_levels_f64

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NULL, ONE = ctypes.c_void_p(0), ctypes.c_void_p(16)      # (a non-NULL, 16-byte aligned token: none of these calls gets as far as touching memory)
HEADER = "coalign_amd_where2comm.h"
NAMES = {"coalign_w2comm_masks", "coalign_w2comm_fuse_nhwc"}
CONFIGS = ("opv2v_pointpillar_where2comm", "mini_pointpillar_where2comm")
GOLDEN = np.load(os.path.join(REPO, "tests", "golden", "where2comm_fuse.npz"))
VOXEL = [0.4, 0.4, 4]
BACKBONE = {"layer_nums": [1, 1, 1], "layer_strides": [1, 2, 2], "num_filters": [16, 32, 64], "upsample_strides": [1, 2, 4], "num_upsample_filter": [32, 32, 32], "inplanes": 16}


def module_args(mode, multi_scale, smooth, C=16, thre=None):
    comm = {"thre": float(GOLDEN["thre"]) if thre is None else thre}
    if smooth:
        comm["gaussian_smooth"] = {"k_size": 5, "c_sigma": 1.0}
    args = {"voxel_size": VOXEL, "downsample_rate": 1, "multi_scale": multi_scale, "agg_operator": {"mode": mode, "feature_dim": C}, "communication": comm}
    if multi_scale:
        args.update(layer_nums=BACKBONE["layer_nums"], num_filters=BACKBONE["num_filters"])
    return args


def test_w2comm_header_table_and_library_agree():
    """The header declares exactly ``NAMES``, the keys of ``hip.W2COMM_SIGNATURES`` (types, counts and exports: tests/test_abi_cpu.py); every declaration's comment
    cites the reference lines it replaces; build.py lists the header and the source."""
    text = open(abi_headers.path(HEADER)).read()
    assert '#include "coalign_amd.h"' in text
    declared = abi_headers.declarations(HEADER)
    assert set(declared) == set(hip.W2COMM_SIGNATURES) == abi_headers.names(HEADER) == NAMES
    comments = re.findall(r"/\*.*?\*/", text, flags=re.S)
    cites = {"coalign_w2comm_masks": ("where2comm.py:34-78", "where2comm_attn.py:273-275"), "coalign_w2comm_fuse_nhwc": ("where2comm_attn.py:224-341", "AttenFusion :44-54")}
    for name in declared:
        last = [c for c in comments if c in text[:text.index(name + "(")]][-1]
        assert all(c in last for c in cites[name]), name
    assert int(re.search(r"#define COALIGN_W2COMM_MAX_GROUPS (\d+)", text).group(1)) == ops.W2COMM_MAX_GROUPS
    src = open(os.path.join(REPO, "coalign_amd", "build.py")).read()
    assert '"coalign_amd_where2comm.h"' in src and '"w2comm.hip"' in src


def _masks(psm=ONE, n_total=4, A=2, H=9, W=14, groups=(3, 1), weights=ONE, bias=ONE, k=5, thre=0.3, levels=3, masks=(16, 16, 16), rates=ONE):
    gl = (ctypes.c_int32 * max(1, len(groups)))(*groups) if groups is not None else None
    mp = (ctypes.c_void_p * 3)(*masks) if masks is not None else None
    return hip.lib().coalign_w2comm_masks(psm, n_total, A, H, W, gl, 0 if groups is None else len(groups), weights, bias, k, thre, levels, mp, rates, NULL)


def _fuse(n_scales=1, x=(16,), C=(64,), H=(9,), W=(14,), masks=(16,), out=(32,), n=3, theta=ONE, rows=None, mode=ops.FUSE_ATT):
    vp, i32 = ctypes.c_void_p * 3, ctypes.c_int32 * 3
    pad = lambda v: tuple(v) + (0,) * (3 - len(v))      # noqa: E731
    rw = None if rows is None else (ctypes.c_int32 * len(rows))(*rows)
    return hip.lib().coalign_w2comm_fuse_nhwc(n_scales, None if x is None else vp(*pad(x)), i32(*pad(C)), i32(*pad(H)), i32(*pad(W)), None if masks is None else vp(*pad(masks)),
                                              None if out is None else vp(*pad(out)), i32(*pad(H)), i32(*pad(W)), n, theta, rw, mode, NULL)


def test_w2comm_argument_refusals_without_a_gpu():
    """NULL -1; sizes < 1, group lengths that do not add up, levels that leave no pixel, maps of 2^31 values -2; an even k, k > 9, more than 8 anchors or agents,
    more than 64 frames, four levels, the no-fusion mode, other channel counts, unaligned maps -3: all before any HIP call (token pointers, no GPU)."""
    for arg in ("psm", "rates", "weights", "bias"):
        assert _masks(**{arg: NULL}) == -1, arg
    assert _masks(masks=None) == -1 and _masks(masks=(16, 0, 16)) == -1 and _masks(groups=None) == -2
    for bad in (dict(n_total=0), dict(A=0), dict(H=0), dict(W=-2), dict(k=-1), dict(levels=0), dict(groups=(3, 2)), dict(groups=(4, 0)), dict(groups=(5, -1)),
                dict(H=3, W=40, levels=3), dict(H=1, levels=2), dict(n_total=8, groups=(8,), A=8, H=8192, W=8192)):
        assert _masks(**bad) == -2, bad
    for bad in (dict(k=4), dict(k=2), dict(k=11), dict(A=9), dict(n_total=9, groups=(9,)), dict(levels=4), dict(n_total=65, groups=(1,) * 65)):
        assert _masks(**bad) == -3, bad
    for arg in ("x", "masks", "out"):
        assert _fuse(**{arg: None}) == -1 and _fuse(**{arg: (0,)}) == -1, arg
    assert _fuse(theta=NULL) == -1
    for bad in (dict(n_scales=0), dict(n_scales=4), dict(n=0), dict(n=-1), dict(H=(0,)), dict(W=(-1,)), dict(rows=(0, 0, 1)), dict(rows=(0, 1, 3)), dict(C=(256,), H=(4096,), W=(4096,))):
        assert _fuse(**bad) == -2, bad
    for bad in (dict(n=9), dict(mode=ops.FUSE_NONE), dict(mode=7), dict(C=(96,)), dict(C=(32,)), dict(x=(20,)), dict(out=(8,))):
        assert _fuse(**bad) == -3, bad
    assert ops.w2comm_masks_shape_ok(2, [3, 1], 5, 3, (16, 32)) and ops.w2comm_masks_shape_ok(1, [8], 0, 1) and not ops.w2comm_masks_shape_ok(2, [3], 4, 1)
    assert not ops.w2comm_masks_shape_ok(9, [3], 5, 1) and not ops.w2comm_masks_shape_ok(2, [9], 5, 1) and not ops.w2comm_masks_shape_ok(2, [3], 5, 3, (3, 40))


def test_w2comm_ops_refuse_cpu_tensors():
    x = torch.zeros(2, 64, 4, 4).contiguous(memory_format=torch.channels_last)
    with pytest.raises(hip.CoalignHipError):
        ops.w2comm_masks(torch.zeros(2, 2, 4, 4), [2], None, None, 0.3)
    with pytest.raises(hip.CoalignHipError):
        ops.w2comm_fuse_nhwc([x], [torch.ones(2, 4, 4, dtype=torch.uint8)], torch.zeros(2, 2, 3, dtype=torch.float64), ops.FUSE_MAX)


# ---- the module against the reference's recorded outputs ------------------------------------------------------------------------------------------------------------
def golden_close(got, want, what):
    """The project's golden bound: rtol 1e-5 + 1e-6 of the scale (the same fp32 operations; summation order may differ)."""
    return assert_elementwise(got, torch.from_numpy(want), what, rtol=1e-5, floor=1e-6)


@pytest.mark.parametrize("smooth", [False, True])
def test_golden_inputs_meet_the_mask_conditions(smooth):
    """The stored logits give mixed masks (20-80 % ones per agent) and no smoothed confidence within 2e-5 of the threshold, in float64; the float64 masks and rates
    equal the reference's recorded ones."""
    psm = torch.from_numpy(GOLDEN[f"single_psm_{int(smooth)}"])
    w, b = (torch.from_numpy(GOLDEN["gaussian_weight"]).reshape(5, 5), torch.from_numpy(GOLDEN["gaussian_bias"])) if smooth else (None, None)
    check_mask_inputs(psm, w, b, float(GOLDEN["thre"]))
    masks, rates = masks_f64(psm, [3, 1], w, b, float(GOLDEN["thre"]))
    assert np.array_equal(masks[0].numpy(), GOLDEN[f"single_masks_{int(smooth)}"])
    assert float(rate_of(rates)) == float(GOLDEN[f"single_MAX_{int(smooth)}_0_rate"])
    if smooth:
        mp = torch.from_numpy(GOLDEN["multi_psm"])
        check_mask_inputs(mp, w, b, float(GOLDEN["thre"]))
        assert np.array_equal(masks_f64(mp, [3, 1], w, b, float(GOLDEN["thre"]))[0][0].numpy(), GOLDEN["multi_masks"])


@pytest.mark.parametrize("mode", ["ATTEN", "MAX"])
@pytest.mark.parametrize("smooth", [False, True])
def test_forward_torch_single_scale_against_the_golden(mode, smooth):
    m = Where2commFusion(module_args(mode, False, smooth)).eval()
    assert list(m.state_dict().keys()) == list(GOLDEN[f"single_keys_{int(smooth)}"])
    if smooth:
        assert list(m.state_dict().keys()) == ["naive_communication.gaussian_filter.weight", "naive_communication.gaussian_filter.bias"]
        assert np.array_equal(m.naive_communication.gaussian_filter.weight.detach().numpy(), GOLDEN["gaussian_weight"])          # the reference's formula, 1 / (2 pi sigma) included
        assert np.array_equal(m.naive_communication.gaussian_filter.bias.detach().numpy(), GOLDEN["gaussian_bias"])
    x, psm = torch.from_numpy(GOLDEN["single_x"]), torch.from_numpy(GOLDEN[f"single_psm_{int(smooth)}"])
    for half_out in (0, 1):
        T = torch.from_numpy(GOLDEN[f"single_pairwise_{half_out}"])
        keep = T.clone()
        with torch.no_grad():
            out, rate, extra = m(x, psm, torch.tensor([3, 1]), T)
            _, masks, _ = m.naive_communication(m.regroup(psm, [3, 1]), [3, 1])
        tag = f"single_{mode}_{int(smooth)}_{half_out}"
        assert extra == {} and torch.equal(T, keep)
        golden_close(out, GOLDEN[tag + "_out"], tag)
        assert rate.dim() == 0 and float(rate) == float(GOLDEN[tag + "_rate"])
        assert np.array_equal(masks[:, 0].numpy().astype(np.uint8), GOLDEN[f"single_masks_{int(smooth)}"])
        # ... and the float64 restatement agrees with the recorded output at the standing bound
        affine = normalize_pairwise_tfm(T, 10, 12, VOXEL[0], 1)
        ref = where2comm_levels_f64([x], [single_scale_masks(torch.from_numpy(GOLDEN[f"single_masks_{int(smooth)}"]), [3, 1])], [3, 1], affine, mode)[0]
        assert_elementwise(torch.from_numpy(GOLDEN[tag + "_out"]), ref, tag + " golden vs float64")


def golden_backbone():
    bb = ResNetBEVBackbone(dict(BACKBONE), 16)
    assert list(bb.state_dict().keys()) == list(GOLDEN["backbone_keys"])
    bb.load_state_dict({k: torch.from_numpy(GOLDEN["backbone." + k]) for k in GOLDEN["backbone_keys"]})
    return bb.eval()


@pytest.mark.parametrize("mode", ["ATTEN", "MAX"])
def test_forward_torch_multi_scale_against_the_golden(mode):
    """The reference's ResNetBEVBackbone state in this project's; the module recomputes ``backbone.resnet(x)`` like the reference, and takes the levels through its
    internal entry point (``fuse(..., feats=...)``) to the same values."""
    bb = golden_backbone()
    m = Where2commFusion(module_args(mode, True, True)).eval()
    assert list(m.state_dict().keys()) == list(GOLDEN["multi_keys"])
    x, psm, T = torch.from_numpy(GOLDEN["multi_x"]), torch.from_numpy(GOLDEN["multi_psm"]), torch.from_numpy(GOLDEN["multi_pairwise"])
    with torch.no_grad():
        out, rate, _ = m(x, psm, torch.tensor([3, 1]), T, bb)
        affine = normalize_pairwise_tfm(T, 16, 24, VOXEL[0], 1)
        again, rate2, _ = m.fuse(None, psm, [3, 1], affine, bb, feats=bb.resnet(x))
    assert tuple(out.shape) == (2, 96, 16, 24)
    golden_close(out, GOLDEN[f"multi_{mode}_out"], f"multi {mode}")
    assert float(rate) == float(rate2) == float(GOLDEN[f"multi_{mode}_rate"])
    assert torch.equal(out, again)


def test_plain_backbone_feeds_the_masked_map_to_the_next_block():
    """A ``BaseBEVBackbone`` (no ``.resnet``): level i + 1 is ``blocks[i + 1]`` of the MASKED level i (where2comm_attn.py:262) -- stated here with the module's parts."""
    cfg = {"layer_nums": [1, 1], "layer_strides": [1, 2], "num_filters": [8, 16], "upsample_strides": [1, 2], "num_upsample_filter": [8, 8]}
    torch.manual_seed(3)
    bb = BaseBEVBackbone(cfg, 4).eval()
    args = module_args("MAX", True, True)
    args.update(layer_nums=cfg["layer_nums"], num_filters=cfg["num_filters"])
    m = Where2commFusion(args).eval()
    psm, w, b, thre = mask_case(3, 2, 8, 12, 5, seed=50)
    m.naive_communication.thre = thre
    x = torch.randn(3, 4, 8, 12, generator=torch.Generator().manual_seed(4))
    A = torch.zeros(1, 3, 3, 2, 3, dtype=torch.float64)
    A[..., 0, 0] = A[..., 1, 1] = 1.0
    A[0, 0, 1, 0, 2] = 0.21
    with torch.no_grad():
        out, rate, _ = m.fuse(x, psm, [3], A, bb)
        masks, rates = masks_f64(psm, [3], w, b, thre, levels=2)
        l0 = bb.blocks[0](x) * masks[0].float().unsqueeze(1)
        l1 = bb.blocks[1](l0) * masks[1].float().unsqueeze(1)
        fused = [f.float() for f in where2comm_levels_f64([l0, l1], None, [3], A, "MAX")]
        want = torch.cat([bb.deblocks[0](fused[0]), bb.deblocks[1](fused[1])], dim=1)
    assert_elementwise(out, want, "plain backbone, multi scale")
    assert float(rate) == float(rate_of(rates))


def test_even_agent_quirk_at_three_agents():
    """``communication_mask_nodiag[::2] = 1`` (where2comm.py:71): in a frame of three, agent 2's mask is all ones, agent 1's is not; the rate counts agent 0's mask
    before the override."""
    psm, w, b, thre = mask_case(3, 2, 12, 16, 5, seed=51)
    comm = where2comm.Communication({"thre": thre, "gaussian_smooth": {"k_size": 5, "c_sigma": 1.0}}).eval()
    with torch.no_grad():
        _, masks, rate = comm([psm], [3])
    _, on = check_mask_inputs(psm, w, b, thre)
    assert bool(masks[0].all()) and bool(masks[2].all()) and not bool(masks[1].all()) and torch.equal(masks[1, 0].bool(), on[1])
    assert not bool(on[0].all()) and not bool(on[2].all())
    assert float(rate) == float(torch.tensor(float(on[0].sum())) / (12 * 16))


def test_refusals():
    args = module_args("ATTEN", False, True)
    args["agg_operator"] = {"mode": "Transformer", "feature_dim": 16, "n_head": 8, "with_spe": True, "with_scm": True}
    with pytest.raises(NotImplementedError, match="cannot run in the reference"):
        Where2commFusion(args)
    m = Where2commFusion(module_args("MAX", False, True)).eval()
    x, A = torch.zeros(2, 16, 10, 12), torch.zeros(1, 2, 2, 2, 3, dtype=torch.float64)
    with pytest.raises(ValueError, match="confidence map"):
        m.fuse(x, torch.zeros(2, 2, 5, 6), [2], A)
    with pytest.raises(NotImplementedError):
        m.fuse(x, torch.zeros(2, 2, 10, 12), [2], A, rows=[1, 0])
    none = Where2commFusion({k: v for k, v in module_args("MAX", False, False).items() if k != "communication"}).eval()
    out, rate, _ = none.fuse(x, None, [2], A)
    assert rate.dtype == torch.int64 and int(rate) == 0 and list(none.state_dict()) == []


def test_aliases_and_registry():
    assert fusion.Where2commFusion is where2comm.Where2comm and BASELINE_REGISTRY["point_pillar_where2comm"] is PointPillarWhere2comm
    opencood_compat.install()
    import importlib
    assert importlib.import_module("opencood.models.fuse_modules.where2comm_attn").Where2comm is where2comm.Where2comm
    assert importlib.import_module("opencood.models.comm_modules.where2comm").Communication is where2comm.Communication


@pytest.mark.parametrize("name", CONFIGS)
def test_build_model_and_route_plan(name):
    h = builtin_config(name)
    model = build_model(h).eval()
    assert isinstance(model, PointPillarWhere2comm) and isinstance(model.fusion_net, Where2commFusion)
    assert "THIS PROJECT'S" in PointPillarWhere2comm.__doc__          # the reference ships no model class for the module
    assert model.accepts_normalized_affine and model.accepts_pillar_frame
    keys = [k for k in model.state_dict() if k.startswith("fusion_net.")]
    assert keys == ["fusion_net.naive_communication.gaussian_filter.weight", "fusion_net.naive_communication.gaussian_filter.bias"]
    w = model.fusion_net.naive_communication.gaussian_filter.weight.detach()
    assert torch.equal(w.reshape(5, 5), gaussian_weight(5, 1.0))
    assert model.kernel_route(5) and not model.kernel_route(9) and model.kernel_route_reason() is None
    p = routes.plan(h, baselines=True)
    assert p["outside_hot_path"] is None and p["fusion"] == routes.W2COMM and "fusion" not in p["fallbacks"]
    assert p["layers"]["fusion_net.naive_communication.gaussian_filter"] == routes.W2COMM_MASKS
    assert not [f for f in p["fallbacks"] if f.startswith("fusion_net")]
    assert routes.plan(h)["outside_hot_path"] is not None          # the default walk still reports the family outside the hot path
    model.train()
    assert not model.kernel_route(3)
