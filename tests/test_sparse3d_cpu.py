"""The sparse 3-D trunk of the SECOND detectors without a GPU: the torch-op route of every layer against the dense float64 restatement on every case of
tests/sparse3d_cases.py, the checkpoint names and layouts, the yaml parser against the reference's own, the extension header against the rules of
tests/test_abi_cpu.py, the plan's wording, and both models on the mini config."""
import copy
import functools
import json
import os
import re

import pytest
import torch

import abi_headers
import sparse3d_cases as cases
import sparse3d_reference as ref
from conftest import GOLDEN, assert_elementwise
from coalign_amd import build, config, hip, sparse3d
from coalign_amd.config import builtin_config
from coalign_amd.detector import SECOND_REGISTRY, build_model
from coalign_amd.second import SecondSSFA, SecondSSFAUncertainty

HEADER = "coalign_amd_sparse3d.h"


def _close64(got, want, what):
    scale = max(float(want.abs().max()), 1e-300)
    err = float((got.detach().double() - want).abs().max())
    assert err <= 1e-12 * scale, f"{what}: {err / scale:.3e} of the scale"


@pytest.mark.parametrize("group", cases.GROUPS)
@pytest.mark.parametrize("combo", cases.COMBOS, ids=lambda c: f"{c[0]}_{c[1]}_k{''.join(map(str, sparse3d._triple(c[2])))}")
def test_torch_route_equals_the_dense_reference(combo, group):
    cin, cout, kernel = combo
    ran = 0
    for case in cases.of_group(group):
        for subm, k, s, p in cases.geometries(case, kernel):
            layer = cases.make_layer(cin, cout, subm, k, s, p, seed=cin + cout, site_capacity=case.site_capacity).double()
            feats = cases.features(case, cin, seed=3)
            count = None if case.count is None else torch.tensor([case.count], dtype=torch.int32)
            x = sparse3d.SparseTensor3d(feats.double(), case.indices, case.shape, case.batch, count, torch.zeros(1, dtype=torch.int32))
            assert layer[0].kernel_reason(x) is not None                      # CPU tensors: the torch-op route
            out = layer(x)
            what = f"{case.name} {'subm' if subm else 'strided'} {k}/{s}/{p}"
            dense, _ = cases.check(case, layer, feats, out, out.rows(), _close64, what)
            if group == "to_dense":
                got = sparse3d.HeightCompression({"feature_num": 128}).compress(out)
                want = ref.height_compression(dense)
                assert got.shape == want.shape
                _close64(got, want, what + " dense") if want.numel() and float(want.abs().max()) > 0 else None
                assert not bool(got[want == 0].any()), what
                D = dense.shape[2]
                for r in range(min(out.rows(), 5)):                          # channel c D + d, spelled out
                    b, z, y, xx = (int(v) for v in out.indices[r])
                    if 0 <= b < case.batch and 0 <= z < D and 0 <= y < dense.shape[3] and 0 <= xx < dense.shape[4]:
                        assert torch.equal(got[b, z::D, y, xx], out.features[r]), what
            ran += 1
    assert ran > 0 or (group == "strided")


def test_strided_cases_cover_both_kernels():
    """Every case of the strided group runs with some combination (none is filtered out)."""
    for case in cases.of_group("strided"):
        assert any(cases.geometries(case, k) for _, _, k in cases.COMBOS), case.name


# the reference's module tree, spelled out from sparse_backbone_3d.py:48-91: (name, Cin, Cout, kernel)
LAYERS = [("conv_input.0", 4, 16, (3, 3, 3)), ("conv1.0.0", 16, 16, (3, 3, 3)),
          ("conv2.0.0", 16, 32, (3, 3, 3)), ("conv2.1.0", 32, 32, (3, 3, 3)), ("conv2.2.0", 32, 32, (3, 3, 3)),
          ("conv3.0.0", 32, 64, (3, 3, 3)), ("conv3.1.0", 64, 64, (3, 3, 3)), ("conv3.2.0", 64, 64, (3, 3, 3)),
          ("conv4.0.0", 64, 64, (3, 3, 3)), ("conv4.1.0", 64, 64, (3, 3, 3)), ("conv4.2.0", 64, 64, (3, 3, 3)),
          ("conv_out.0", 64, 64, (3, 1, 1))]


def _expected_state():
    want = {}
    for name, cin, cout, k in LAYERS:
        want[f"spconv_block.{name}.weight"] = (cout, *k, cin)
        bn = name[:-1] + "1"
        for leaf in ("weight", "bias", "running_mean", "running_var"):
            want[f"spconv_block.{bn}.{leaf}"] = (cout,)
        want[f"spconv_block.{bn}.num_batches_tracked"] = ()
    return want


def test_state_dict_keys_and_shapes_are_the_references():
    model = build_model(builtin_config("second/mini_second_uncertainty"))
    got = {k: tuple(v.shape) for k, v in model.state_dict().items() if k.startswith("spconv_block.")}
    assert got == _expected_state()
    assert not [k for k in model.state_dict() if k.startswith(("vfe.", "map_to_bev."))]
    heads = {k for k in model.state_dict() if k.split(".")[0] in ("cls_head", "reg_head", "unc_head", "dir_head")}
    assert heads == {f"{h}.{p}" for h in ("cls_head", "reg_head", "unc_head", "dir_head") for p in ("weight", "bias")}
    assert "ssfa.bottom_up_block_0.1.weight" in model.state_dict() and "ssfa.deconv_block_1.0.weight" in model.state_dict() and "ssfa.w_1.1.running_var" in model.state_dict()
    assert "shrink_conv.layers.0.double_conv.0.weight" in model.state_dict()
    late = build_model(builtin_config("second/mini_second"))
    assert {k for k in late.state_dict() if k.startswith("head.")} == {"head.conv_box.weight", "head.conv_box.bias", "head.conv_cls.weight", "head.conv_cls.bias",
                                                                      "head.conv_iou.weight", "head.conv_dir.weight", "head.conv_dir.bias"}


def test_spconv1_layout_checkpoint_round_trip():
    """A checkpoint written by spconv 1.2.1 holds [kd, kh, kw, Cin, Cout]: recognised by shape, permuted on load, and the model computes the same."""
    a = cases.seed_backbone_(build_model(builtin_config("second/mini_second_uncertainty")), 1)
    sd = {k: v.clone() for k, v in a.state_dict().items()}
    old = {k: (v.permute(1, 2, 3, 4, 0).contiguous() if v.dim() == 5 else v) for k, v in sd.items()}
    assert tuple(old["spconv_block.conv_out.0.weight"].shape) == (3, 1, 1, 64, 64) and tuple(old["spconv_block.conv_input.0.weight"].shape) == (3, 3, 3, 4, 16)
    b = build_model(builtin_config("second/mini_second_uncertainty"))
    b.load_state_dict(old)
    for k, v in b.state_dict().items():
        assert torch.equal(v, sd[k]), k
    b.load_state_dict(sd)                                                    # spconv 2's layout loads as it is
    assert torch.equal(b.state_dict()["spconv_block.conv2.0.0.weight"], sd["spconv_block.conv2.0.0.weight"])


def test_load_voxel_params_equals_the_references_own():
    table = json.load(open(os.path.join(GOLDEN, "second_voxel_params.json")))
    assert len(table) == 6
    for rel, rec in table.items():
        got = config.load_voxel_params(copy.deepcopy(rec["input"]))
        assert got == rec["output"], rel
        a = got["postprocess"]["anchor_args"]
        assert all(isinstance(a[k], int) for k in "WHD") and [got["model"]["args"][k] for k in "WHD"] == [a[k] for k in "WHD"], rel
    assert "load_voxel_params" in config.YAML_PARSERS
    h = {"preprocess": {"args": {"voxel_size": [0.4, 0.4, 0.3]}}, "postprocess": {"anchor_args": {"cav_lidar_range": [-1.0, -1.0, -1, 1.0, 1.0, 1]}},
         "box_align_pre_calc": {"stage1_postprocessor_config": {}}}
    got = config.load_voxel_params(h)                                         # int() truncates: 2 / 0.4 = 5.000000000000001 -> 5, 2 / 0.3 -> 6; no model section
    assert (got["postprocess"]["anchor_args"]["W"], got["postprocess"]["anchor_args"]["D"]) == (5, 6) and "model" not in got
    assert got["box_align_pre_calc"]["stage1_postprocessor_config"]["anchor_args"] is got["postprocess"]["anchor_args"]


def test_configs_build_and_register():
    assert SECOND_REGISTRY == {"second_ssfa": SecondSSFA, "second_ssfa_uncertainty": SecondSSFAUncertainty}
    for name, cls, shape in (("mini_second_uncertainty", SecondSSFAUncertainty, (41, 128, 256)), ("mini_second", SecondSSFA, (41, 128, 256)),
                             ("opv2v_second_uncertainty", SecondSSFAUncertainty, (41, 800, 2816)), ("opv2v_second", SecondSSFA, (41, 800, 2816))):
        h = builtin_config("second/" + name)
        m = build_model(h)
        assert type(m) is cls and m.spconv_block.sparse_shape == shape
    assert m.spconv_block.level_shapes() == [(41, 800, 2816), (21, 400, 1408), (11, 200, 704), (5, 100, 352), (2, 100, 352)]
    assert not [f for f in os.listdir(config.CONFIG_DIR) if "second" in f and f.endswith(".yaml")]      # in the subdirectory: the plan snapshot globs the top level


# ---- the extension header, held to the rules of tests/test_abi_cpu.py ----------------------------------------------------------------------------------------
def _ext_text():
    src = open(os.path.join(build.EXT_INCLUDE, HEADER)).read()
    return re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", src, flags=re.S)), src


def test_extension_header_table_and_library_agree():
    assert build.EXT_HEADERS == (HEADER,) and os.listdir(build.EXT_INCLUDE) == [HEADER] and list(hip.EXT_HEADERS) == [HEADER]
    assert f"-I{build.EXT_INCLUDE}" in build.FLAGS and "sparse_conv3d.hip" in build.SOURCES
    assert HEADER not in build.ABI_HEADERS and HEADER not in abi_headers.FROZEN
    text, src = _ext_text()
    assert '#include "coalign_amd.h"' in text
    table = hip.EXT_HEADERS[HEADER]
    assert table is hip.SPARSE3D_SIGNATURES
    names = set(re.findall(r"\b(coalign_[a-z0-9_]+)\s*\(", text))
    declared = {}
    for ret, name, args in re.findall(r"\b(int|size_t|int64_t|const char \*)\s*(coalign_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", text):
        declared[name] = (abi_headers.RETURNS[ret], [" ".join(a.split()) for a in args.split(",")])
    assert set(declared) == names == set(table), set(declared) ^ set(table)
    for name, (res, args) in declared.items():
        assert table[name][0] is res and len(table[name][1]) == len(args), name
        assert table[name][1] == [abi_headers.ctype(a) for a in args], name
    for other in build.ABI_HEADERS:
        assert not (set(table) & abi_headers.names(other)), other
    lib = hip.lib()
    assert lib.coalign_abi_version() == 2
    for name, (res, args) in table.items():
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == args, name
    # every declaration cites the reference lines it replaces
    for block in re.findall(r"/\*\s*\(18[a-h]\).*?\*/", src, flags=re.S):
        assert re.search(r"\.py:\d+", block) or "(18b)" in block or "(18f)" in block, block[:60]
    assert len(re.findall(r"/\*\s*\(18[a-h]\)", src)) == len(table)


def test_entry_points_refuse_before_any_hip_call():
    """Shape / support / pointer refusals need no GPU: they come before the first HIP call."""
    L = hip.lib()
    assert L.coalign_sp3d_index_workspace_bytes(2, 9, 12, 20, 100) == 2304 and L.coalign_sp3d_index_workspace_bytes(5, 41, 800, 2816, 1) > 0
    assert L.coalign_sp3d_index_workspace_bytes(24, 41, 800, 2816, 1) == 0                                   # N D H W >= 2^31
    assert L.coalign_sp3d_index_build(None, None, 4, 24, 41, 800, 2816, None, 0, None) == -2
    assert L.coalign_sp3d_index_build(None, None, 4, 2, 9, 12, 20, None, 0, None) == -4
    assert L.coalign_sp3d_index_build(None, None, 4, 2, 9, 12, 20, None, 1 << 20, None) == -1
    for cin, cout, k in cases.COMBOS:
        taps = 27 if k == 3 else 3
        assert L.coalign_sp3d_weight_bytes(cin, cout, taps) == (taps * cin * cout * 4 if cin == 4 else taps * (cin // 16) * ((cout + 31) // 32) * 2048 + (cout + 31) // 32 * 128)
    for cin, cout, taps in ((8, 16, 27), (64, 128, 27), (16, 16, 3), (4, 16, 3), (128, 128, 27), (64, 64, 9)):
        assert L.coalign_sp3d_weight_bytes(cin, cout, taps) == 0
        assert L.coalign_sp3d_conv(None, 0, None, taps, None, 0, cin, cout, None, 0, None, None, None) == -3
    assert L.coalign_sp3d_conv(None, 0, None, 27, None, 0, 16, 16, None, 0, None, None, None) == -4
    assert L.coalign_sp3d_to_dense(None, None, 0, 64, None, 0, 24, 41, 800, 2816, None, None) == -2
    assert L.coalign_sp3d_mean_vfe(None, None, 0, 5, 4, None, None) == 0 and L.coalign_sp3d_mean_vfe(None, None, 3, 5, 4, None, None) == -1


def test_plan_words_every_layer(monkeypatch):
    monkeypatch.delenv("COALIGN_SP3D", raising=False)
    monkeypatch.setattr(sparse3d, "KERNEL_DEFAULT", True)
    lines = sparse3d.plan(builtin_config("second/opv2v_second_uncertainty"))
    assert list(lines) == ["vfe"] + [f"spconv_block.{n}" for n, *_ in LAYERS] + ["map_to_bev"]
    assert lines["vfe"] == "coalign_sp3d_mean_vfe" and lines["map_to_bev"].startswith("coalign_sp3d_to_dense")
    assert lines["spconv_block.conv_input.0"] == "coalign_sp3d_conv (27 taps, fp32 vector arithmetic)"
    assert lines["spconv_block.conv3.1.0"] == "coalign_sp3d_conv (27 taps, sp16 pairs on v_mfma_f32_32x32x16_f16)"
    assert lines["spconv_block.conv_out.0"] == "coalign_sp3d_conv (3 taps, sp16 pairs on v_mfma_f32_32x32x16_f16)"
    monkeypatch.setenv("COALIGN_SP3D", "0")
    off = sparse3d.plan(builtin_config("second/opv2v_second_uncertainty"))
    assert all(v == f"{sparse3d.TORCH_TEXT} (COALIGN_SP3D=0)" for k, v in off.items() if k.startswith("spconv_block."))
    assert off["vfe"].startswith("torch ops") and off["map_to_bev"].startswith("torch ops")
    monkeypatch.setenv("COALIGN_SP3D", "1")
    odd = sparse3d.SubMConv3d(8, 16, 3).eval()
    assert "not one of VoxelBackBone8x's combinations" in odd.kernel_reason() and odd.route_text().startswith(sparse3d.TORCH_TEXT)
    ok = sparse3d.SubMConv3d(16, 16, 3)
    assert ok.kernel_reason() == "training mode" and ok.eval().kernel_reason() is None
    x = sparse3d.SparseTensor3d(torch.zeros(1, 16), torch.zeros(1, 4, dtype=torch.int32), (9, 12, 20), 2)
    assert ok.kernel_reason(x) == "CPU tensors"


@functools.lru_cache(maxsize=None)
def _mini_reference():
    """The mini config's voxels and the dense float64 trunk on them, computed once for both models (their trunks are seeded alike)."""
    bb = cases.seed_backbone_(build_model(builtin_config("second/mini_second_uncertainty")), 2).eval().spconv_block
    vox = cases.voxels(bb.sparse_shape, 2, seed=4)
    mean = vox["voxel_features"].double().sum(dim=1) / vox["voxel_num_points"].clamp(min=1).view(-1, 1).double()
    dense, _ = ref.backbone(bb, mean, vox["voxel_coords"], 2)
    return vox, ref.height_compression(dense).float(), bb.state_dict()


@pytest.mark.parametrize("name", ["mini_second_uncertainty", "mini_second"])
def test_models_on_the_mini_config(name):
    """Output keys and shapes; values against the dense reference composed with the same SSFA / shrink header / heads."""
    h = builtin_config("second/" + name)
    model = cases.seed_backbone_(build_model(h), 2).eval()
    bb = model.spconv_block
    assert bb.sparse_shape == (41, 128, 256)
    vox, bev, trunk = _mini_reference()
    assert all(torch.equal(v, trunk[k]) for k, v in bb.state_dict().items())
    with torch.no_grad():
        out = model({"processed_lidar": vox, "record_len": torch.tensor([2])})
        assert bev.shape == (2, 128, 16, 32)
        neck = model.ssfa(bev)
        neck = model.shrink_conv(neck) if model.shrink_flag else neck
        if name == "mini_second":
            want = model.head(neck)
            assert set(out) == {"reg_preds", "cls_preds", "dir_preds", "iou_preds"}
            shapes = {"reg_preds": 14, "cls_preds": 2, "dir_preds": 4, "iou_preds": 2}
        else:
            want = {"cls_preds": model.cls_head(neck), "reg_preds": model.reg_head(neck), "unc_preds": model.unc_head(neck), "dir_preds": model.dir_head(neck)}
            assert set(out) == {"cls_preds", "reg_preds", "unc_preds", "dir_preds"}
            shapes = {"cls_preds": 2, "reg_preds": 14, "unc_preds": 6, "dir_preds": 4}
    for k, c in shapes.items():
        assert tuple(out[k].shape) == (2, c, 16, 32), k
        assert_elementwise(out[k], want[k], f"{name} {k}")
    # the reference's batch size when nothing else says it: coords[:, 0].max() + 1
    with torch.no_grad():
        again = model({"processed_lidar": vox})
    assert torch.equal(again["cls_preds"], out["cls_preds"])
