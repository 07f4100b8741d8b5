"""DiscoNet's pixel-weight fusion, host side (no GPU): the extension header include/coalign_amd_disco.h against the product library and ``hip.DISCO_SIGNATURES``, the
frozen headers, argument validation before any HIP call, ``fusion.DiscoFusion`` against the reference's recorded output (tests/golden/disco_fuse.npz, written by
tests/golden/make_disco_golden.py) and against float64, the weight image's layout, and the ``point_pillar_disconet`` model: construction, route plan, names, forward."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import abi_headers
from conftest import assert_elementwise
from coalign_amd import hip, ops
from coalign_amd.config import builtin_config
from coalign_amd.detector import BASELINE_REGISTRY, MODEL_REGISTRY, PointPillarDiscoNet, build_model
from coalign_amd.fusion import DiscoFusion
from coalign_amd.synthetic import disco_parameters_, fill_parameters_, make_frame
from disco_reference import assert_not_degenerate, disco_fuse_f64

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NULL, ONE = ctypes.c_void_p(0), ctypes.c_void_p(16)      # (a non-NULL, 16-byte aligned token: none of these calls gets as far as touching memory)
HEADER = "coalign_amd_disco.h"
CONFIGS = ("opv2v_pointpillar_disconet", "mini_pointpillar_disconet")


def test_disco_header_table_and_library_agree():
    """include/coalign_amd_disco.h declares exactly the keys of ``hip.DISCO_SIGNATURES`` (types, counts and exports: tests/test_abi_cpu.py); the header includes
    coalign_amd.h and cites the reference lines each entry point replaces."""
    text = open(abi_headers.path(HEADER)).read()
    assert '#include "coalign_amd.h"' in text
    declared = abi_headers.declarations(HEADER)
    assert set(declared) == set(hip.DISCO_SIGNATURES) == abi_headers.names(HEADER) and len(declared) == 2
    comments = re.findall(r"/\*.*?\*/", text, flags=re.S)
    for name in declared:
        last = [c for c in comments if c in text[:text.index(name + "(")]][-1]
        assert "fusion_in_one.py:144-171" in last and "disco_fuse.py:76-99" in last, name


def test_build_lists_the_new_header_and_source():
    src = open(os.path.join(REPO, "coalign_amd", "build.py")).read()
    assert '"coalign_amd_disco.h"' in src and '"disco_fuse.hip"' in src


def _fuse(x=ONE, n=3, C=64, H=9, W=14, theta=ONE, params=ONE, params_bytes=None, out=ONE):
    L = hip.lib()
    if params_bytes is None:
        params_bytes = L.coalign_disco_param_bytes(C)
    return L.coalign_disco_fuse(x, n, C, H, W, theta, params, params_bytes, out, NULL)


def test_disco_argument_validation_without_a_gpu():
    """NULL -1; n < 0, C / H / W < 1, a wrong image size -2; n > 8, C = 48 / 416 (not a multiple of 32 / above 384), unaligned pointers -3; n = 0 is OK without a
    launch: all before any HIP call (token pointers, no GPU)."""
    L = hip.lib()
    for arg in ("x", "theta", "params", "out"):
        assert _fuse(**{arg: NULL}) == -1, arg
    for bad in (dict(n=-1), dict(C=0), dict(H=0), dict(W=0), dict(H=-2), dict(W=-7), dict(C=-32)):
        assert _fuse(**bad) == -2, bad
    for bad in (dict(n=9), dict(n=64), dict(C=48), dict(C=416), dict(C=16), dict(C=100)):
        assert _fuse(**bad) == -3, bad
    assert _fuse(n=0) == 0 and _fuse(n=0, x=NULL, out=NULL) == 0
    assert _fuse(params_bytes=17) == -2 and _fuse(C=256, params_bytes=L.coalign_disco_param_bytes(64)) == -2
    assert _fuse(H=46341, W=46341) == -2                                   # C * H * W beyond 32-bit offsets
    assert _fuse(x=ctypes.c_void_p(20)) == -3 and _fuse(out=ctypes.c_void_p(8)) == -3 and _fuse(params=ctypes.c_void_p(4)) == -3
    for C in range(32, 385, 32):
        assert L.coalign_disco_param_bytes(C) == 2 * (C // 16) * 8192 + 16384 + 436 * 4, C
    for C in (0, 16, 48, 416, -32):
        assert L.coalign_disco_param_bytes(C) == 0, C


def test_disco_fuse_refuses_cpu_tensors():
    with pytest.raises(hip.CoalignHipError):
        ops.disco_fuse(torch.zeros(2, 32, 3, 3).contiguous(memory_format=torch.channels_last), torch.zeros(2, 2, 3, dtype=torch.float64), torch.zeros(16, dtype=torch.uint8))


@pytest.fixture(scope="module")
def recorded(golden):
    g = golden("disco_fuse.npz")
    m = DiscoFusion(int(g["x"].shape[1]))
    state = {str(k): torch.from_numpy(g["sd." + str(k)]) for k in g["state_keys"]}
    m.load_state_dict(state, strict=True)                                  # the reference's parameter names
    return g, m.eval(), state


def test_disco_fusion_reproduces_the_reference_recording(recorded):
    """``DiscoFusion`` loaded from the reference's ``state_dict`` gives the reference's recorded output on the CPU; the float64 restatement agrees with both, and the
    recorded case is one in which the MLP matters."""
    g, m, state = recorded
    x, rl, A = torch.from_numpy(g["x"]), torch.from_numpy(g["record_len"]), torch.from_numpy(g["affine"])
    with torch.no_grad():
        got = m(x, rl, A)
    assert_elementwise(got, torch.from_numpy(g["out"]), "DiscoFusion on the CPU vs the reference's recording")
    off = 0
    for b, n in enumerate(rl.tolist()):
        ref, s, a = disco_fuse_f64(state, x[off:off + n], A[b, 0, :n])
        assert_not_degenerate(s, a, f"frame {b}")
        assert_elementwise(torch.from_numpy(g["out"][b]), ref, f"the reference's recording vs float64, frame {b}")
        off += n


def test_folded_weights_give_the_unfolded_result(recorded):
    g, m, _ = recorded
    x, rl, A = torch.from_numpy(g["x"]), torch.from_numpy(g["record_len"]), torch.from_numpy(g["affine"])
    with torch.no_grad():
        assert_elementwise(m.forward_torch(x, rl, A, folded=True), m.forward_torch(x, rl, A), "folded vs unfolded PixelWeightLayer")
    w1 = m.pixel_weight_layer.folded()[0][0]
    assert m.pixel_weight_layer.folded()[0][0] is w1                       # cached ...
    with torch.no_grad():
        m.pixel_weight_layer.bn1_1.running_var.mul_(2.0)
    assert m.pixel_weight_layer.folded()[0][0] is not w1                   # ... until a tensor is written
    with torch.no_grad():
        m.pixel_weight_layer.bn1_1.running_var.mul_(0.5)


def test_weight_image_layout(recorded):
    """The image ``ops.pack_disco_weights`` writes, read back by the layout the header states: every sp16 pair rejoins to the folded weight within 2^-22, at the
    (step, row tile, lane, element) the matrix instruction's operand map asks for; the float section in order; out-of-range weights are refused."""
    _, m, _ = recorded
    (w1, b1), (w2, b2), (w3, b3), (w4, b4) = m.pixel_weight_layer.folded()
    img = m.pixel_weight_layer.packed()
    C = w1.shape[1] // 2
    assert img.dtype == torch.uint8 and img.numel() == hip.lib().coalign_disco_param_bytes(C)
    n1 = (C // 16) * 8192
    w1 = w1.reshape(128, 2 * C)
    for part, w in ((img[:n1], w1[:, :C]), (img[n1:2 * n1], w1[:, C:]), (img[2 * n1:2 * n1 + 16384], w2.reshape(32, 128))):
        R, K = w.shape
        halves = part.view(torch.float16).reshape(K // 16, R // 32, 2, 32, 2, 8).float()      # [step, tile, lane half, lane row, h | l, element]
        joined = halves[..., 0, :] + halves[..., 1, :] / 1024.0
        want = w.reshape(R // 32, 32, K // 16, 2, 8).permute(2, 0, 3, 1, 4)
        assert float((joined - want).abs().max()) <= 2.0 ** -21 * float(w.abs().max())
    f = img[2 * n1 + 16384:].view(torch.float32)
    assert f.numel() == 436 and torch.equal(f[:128], b1) and torch.equal(f[128:160], b2) and torch.equal(f[416:424], b3) and torch.equal(f[424:432], w4.reshape(-1))
    assert torch.equal(f[432:433], b4) and not bool(f[433:].any())
    w3p = f[160:416].reshape(2, 8, 16)
    for half in range(2):
        for q in range(16):
            assert torch.equal(w3p[half, :, q], w3.reshape(8, 32)[:, 8 * (q >> 2) + 4 * half + (q & 3)])
    assert ops.pack_disco_weights(w1 * 1e6, b1, w2, b2, w3, b3, w4, b4) is None


@pytest.mark.parametrize("cfg", CONFIGS)
def test_build_model_constructs_disconet(cfg):
    """``build_model`` constructs ``point_pillar_disconet`` from both shipped yamls (a KeyError before this model existed); ``plan(hypes, baselines=True)`` names the one-launch fusion."""
    from coalign_amd.routes import DISCO, plan
    hypes = builtin_config(cfg)
    model = build_model(hypes)
    assert isinstance(model, PointPillarDiscoNet) and BASELINE_REGISTRY["point_pillar_disconet"] is PointPillarDiscoNet and "point_pillar_disconet" not in MODEL_REGISTRY
    assert isinstance(model.fusion_net, DiscoFusion) and model.out_channel == 256
    assert plan(hypes)["outside_hot_path"] == "model family 'point_pillar_disconet' is not part of the CoAlign hot path"      # a baseline: planned on request
    p = plan(hypes, baselines=True)
    assert p["outside_hot_path"] is None and p["fusion"] == DISCO == "disco_fuse: warp + pixel-weight MLP + softmax in one launch"
    assert p["fallbacks"] == [] and all(not r.startswith("MIOpen") for r in p["layers"].values())
    odd = builtin_config(cfg)
    odd["model"]["args"]["shrink_header"]["dim"] = [48]
    p = plan(odd, baselines=True)
    assert "fusion" in p["fallbacks"] and p["fusion"].startswith("DiscoFusion op by op")


def test_state_dict_names_match_the_reference(golden):
    g = golden("disco_fuse.npz")
    sd = build_model(builtin_config("opv2v_pointpillar_disconet")).state_dict()
    assert list(sd.keys()) == [str(k) for k in g["model_state_keys"]]
    assert [v.numel() for v in sd.values()] == list(g["model_state_numel"])


def test_opencood_alias_resolves_the_model():
    import sys
    if os.path.isdir("/root/reference") and "/root/reference" in sys.path:
        pytest.skip("a real opencood checkout is on sys.path in this process")
    import importlib
    from coalign_amd import opencood_compat
    opencood_compat.install()
    mod = importlib.import_module("opencood.models.point_pillar_disconet")
    assert mod.PointPillarDiscoNet is PointPillarDiscoNet
    from opencood.models.fuse_modules.fusion_in_one import DiscoFusion as D
    assert D is DiscoFusion


class _CpuEncoder(torch.nn.Module):
    """Stands in for the pillar encoder + scatter (HIP only) on the CPU: a fixed random canvas per agent."""

    def __init__(self, ny, nx):
        super().__init__()
        self.ny, self.nx = ny, nx

    def forward(self, batch):
        n = sum(batch["record_len"])
        batch["spatial_features"] = torch.randn(n, 64, self.ny, self.nx, generator=torch.Generator().manual_seed(5))
        return batch


def test_forward_on_the_cpu_without_the_teacher_keys():
    """The model's forward on the CPU (op-by-op fusion; the HIP pillar encoder replaced by a stand-in canvas): the reference's four outputs, no ``teacher_processed_lidar``."""
    hypes = builtin_config("mini_pointpillar_disconet")
    model = build_model(hypes)
    fill_parameters_(model, seed=3)
    disco_parameters_(model.fusion_net.pixel_weight_layer, seed=3)
    model.eval()
    model.pillar_vfe, model.scatter = torch.nn.Identity(), _CpuEncoder(model.scatter.ny, model.scatter.nx)
    pair = torch.eye(4, dtype=torch.float64).repeat(1, 5, 5, 1, 1)
    pair[0, 0, 1, 0, 3] = 1.3
    batch = {"processed_lidar": {"voxel_features": torch.zeros(1, 32, 4), "voxel_coords": torch.zeros(1, 4, dtype=torch.int32), "voxel_num_points": torch.ones(1, dtype=torch.int32)},
             "record_len": torch.tensor([3]), "pairwise_t_matrix": pair}
    assert "teacher_processed_lidar" not in batch
    with torch.no_grad():
        out = model(batch)
    H, W = model.scatter.ny // 2, model.scatter.nx // 2
    assert set(out) == {"feature", "cls_preds", "reg_preds", "dir_preds"}
    assert out["feature"].shape == (1, 256, H, W) and out["cls_preds"].shape == (1, 2, H, W) and out["reg_preds"].shape == (1, 14, H, W) and out["dir_preds"].shape == (1, 4, H, W)
    assert all(bool(torch.isfinite(v).all()) for v in out.values())
