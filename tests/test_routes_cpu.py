"""Route plan against the kernels' own limits, and the device placement of the ops -- CPU only.

``coalign_amd.routes.plan`` names the kernel of every layer of a config; the kernels check their shapes at the C ABI before any HIP call
(``N = 0`` validates and returns).  The configs are mutated across the SplitMap kernels' channel limits (Cout 1024 of ``coalign_conv3x3_sp`` /
``_sp_s2``, 512 of the fused skip, 32 rows of ``coalign_heads_sp``) and every layer the plan puts on a hand-written kernel is put to that kernel's
entry point.  ``ops._device_op`` must wrap every op that launches on ``_stream()`` exactly once.
"""
import ast
import copy
import ctypes
import inspect

import pytest
import torch
import torch.nn as nn

from coalign_amd import backbone as bb
from coalign_amd import hip, ops
from coalign_amd.config import builtin_config
from coalign_amd import detector
from coalign_amd.detector import build_model
from coalign_amd.routes import SP, plan

NULL, ONE = ctypes.c_void_p(0), ctypes.c_void_p(16)      # (a non-NULL, 16-byte aligned token: with N = 0 no entry point below touches memory)
HW = 8


def _mutant(num_filters=None, shrink=None, upf=None, anchors=None, layer_nums=None, stem=None):
    h = copy.deepcopy(builtin_config("opv2v_coalign"))
    a = h["model"]["args"]
    if num_filters is not None:
        a["base_bev_backbone"]["num_filters"] = list(num_filters)
        a["att"]["feat_dim"] = list(num_filters)
    if upf is not None:
        a["base_bev_backbone"]["num_upsample_filter"] = list(upf)
        a["shrink_header"]["input_dim"] = sum(upf)
    if shrink is not None:
        n = len(shrink)
        a["shrink_header"].update(dim=list(shrink), kernal_size=[3] * n, stride=[1] * n, padding=[1] * n)
    if anchors is not None:
        a["anchor_number"] = anchors
    if layer_nums is not None:                  # (one block per stage: the stage's last block is its strided opener, no SplitMap is handed to the next stage)
        a["base_bev_backbone"]["layer_nums"] = list(layer_nums)
    if stem is not None:                        # (a canvas of `stem` channels: below 32 the first block's opener on a sparse canvas is the consumer-split kernel)
        a["pillar_vfe"]["num_filters"] = [stem]
        a["point_pillar_scatter"]["num_features"] = stem
        a["base_bev_backbone"]["inplanes"] = stem
    return h


def _late_resnet():
    """The single-agent detector on the ResNet backbone: its forward never asks the encoder for a sparse canvas (only the multi-agent ``encode`` does)."""
    h = copy.deepcopy(builtin_config("opv2v_pointpillar_late"))
    h["model"]["args"]["base_bev_backbone"]["resnet"] = True
    return h


MUTANTS = {
    "shipped": _mutant(),
    "stage3_1024": _mutant(num_filters=(64, 128, 1024)),
    "stage3_1088": _mutant(num_filters=(64, 128, 1088)),
    "stage2_512_stage3_576": _mutant(num_filters=(64, 512, 576)),
    "stage1_24": _mutant(num_filters=(24, 128, 256)),
    "shrink_1024": _mutant(shrink=(1024,)),
    "shrink_1088": _mutant(shrink=(1088,)),
    "shrink_1024_then_1088": _mutant(shrink=(1024, 1088)),
    "upsample_64_wide": _mutant(upf=(64, 64, 64)),
    "upsample_48": _mutant(upf=(48, 48, 48)),
    "anchors_1": _mutant(anchors=1),
    "anchors_3": _mutant(anchors=3),
    "anchors_4": _mutant(anchors=4),
    "one_block_stages": _mutant(layer_nums=(1, 1, 1)),
    "stem_16": _mutant(stem=16),
    "late_resnet": _late_resnet(),
}


def _sp(cin, cout):
    return hip.lib().coalign_conv3x3_sp(ONE, ONE, ONE, NULL, 0, ONE, ops.SP_OUT_SP, 0, cin, cout, HW, HW, 1, 0, NULL, NULL, 0, NULL)


def _sp_s2(cin, cout):
    return hip.lib().coalign_conv3x3_sp_s2(ONE, ONE, ONE, ONE, 0, cin, cout, HW, HW, 1, NULL, NULL)


def _sp_s2_skip(cin, cout):
    return hip.lib().coalign_conv3x3_sp_s2_skip(ONE, ONE, ONE, ONE, ONE, ONE, 0, cin, cout, HW, HW, 1, NULL, NULL)


def _pointwise(route, cin, cout, up=1, in_stride=1):
    """The pointwise kernel the route names: split-bf16 (``coalign_pointwise_conv_emu``) or fp32 (``coalign_pointwise_conv_ex``), GEMM rows padded to 32."""
    m = cout * up * up
    fn = hip.lib().coalign_pointwise_conv_ex if "fp32 matrix cores" in route else hip.lib().coalign_pointwise_conv_emu
    return fn(ONE, ONE, ONE, ONE, 0, cin, HW, HW, in_stride, cout, up, (m + 31) // 32 * 32 if up == 1 else m, cout, 0, 0, 0, NULL)


def _heads_sp(cin, rows):
    return hip.lib().coalign_heads_sp(ONE, ONE, ONE, ONE, 0, cin, rows, HW, HW, NULL)


@pytest.mark.parametrize("name", list(MUTANTS))
def test_route_plan_never_names_a_kernel_that_refuses_the_layer(name):
    """Every layer ``plan`` puts on ``conv3x3_sp`` is accepted by ``coalign_conv3x3_sp``; the strided first convolution of a SplitMap block by
    ``coalign_conv3x3_sp_s2`` (and by the fused-skip form when its block takes the skip as a tenth tap); the merged heads, the up-sampling heads and
    the skip convolutions on the pointwise kernel by ``coalign_pointwise_conv_emu`` / ``_ex``; the merged heads on a SplitMap by ``coalign_heads_sp``."""
    h = MUTANTS[name]
    p = plan(h)
    assert p["outside_hot_path"] is None
    model = build_model(h).eval()
    mods = dict(model.named_modules())
    refused = []
    for lname, route in p["layers"].items():
        m = mods.get(lname)
        if isinstance(m, nn.ConvTranspose2d):
            rc = _pointwise(route, m.in_channels, m.out_channels, up=m.stride[0]) if route.startswith("pointwise") else 0
        elif not isinstance(m, nn.Conv2d):
            continue
        elif route == SP:
            rc = _sp(m.in_channels, m.out_channels)
        elif route.endswith("SplitMap out") and ".resnet." in lname and m.stride == (2, 2) and m.in_channels % 16 == 0:
            blk = mods[lname.rsplit(".", 1)[0]]
            rc = _sp_s2(m.in_channels, m.out_channels)
            d = blk.downsample[0]
            if rc == 0 and d.out_channels == m.out_channels and bb.sp_channels_ok(m.in_channels, m.out_channels, skip=True):
                rc = _sp_s2_skip(m.in_channels, m.out_channels)
        elif route.startswith("pointwise") and lname.endswith("_head"):
            rc = _pointwise(route, m.in_channels, sum(c.out_channels for c in (model.cls_head, model.reg_head, model.dir_head)))
        elif route.startswith("pointwise") and ".downsample." in lname:
            rc = _pointwise(route, m.in_channels, m.out_channels, in_stride=2)
        else:
            continue
        if rc != 0:
            refused.append((lname, route, m.in_channels, m.out_channels, rc))
    if detector.heads_sp_shape_ok(model):
        rows = sum(c.out_channels for c in (model.cls_head, model.reg_head, model.dir_head))
        if _heads_sp(model.cls_head.in_channels, rows) != 0:
            refused.append(("merged heads on a SplitMap", rows))
    assert refused == [], (name, refused)


def test_route_plan_at_the_limits():
    """The limits move layers as documented: a 1024-channel shrink header stays on the SplitMap kernel, a 1088-channel one falls back to the
    consumer-split kernel (as before round 6) and is listed as such; stage 3 at 1088 channels leaves the SplitMap route; 40 head rows leave heads_sp."""
    sp_layers = lambda p: {n for n, r in p["layers"].items() if r == SP}
    p = plan(MUTANTS["shrink_1024"])
    assert {"shrink_conv.layers.0.double_conv.0", "shrink_conv.layers.0.double_conv.2"} <= sp_layers(p)
    p = plan(MUTANTS["shrink_1088"])
    assert not {n for n in sp_layers(p) if n.startswith("shrink_conv.")}, p["layers"]
    assert p["layers"]["shrink_conv.layers.0.double_conv.2"].startswith("conv3x3_emu")
    p = plan(MUTANTS["shrink_1024_then_1088"])
    assert "shrink_conv.layers.0.double_conv.2" in sp_layers(p) and "shrink_conv.layers.1.double_conv.2" not in sp_layers(p)
    p = plan(MUTANTS["stage3_1088"])
    assert not {n for n in sp_layers(p) if ".layer2." in n} and "backbone.resnet.layer1.1.conv1" in sp_layers(p)
    assert detector.heads_sp_shape_ok(build_model(MUTANTS["anchors_3"])) and not detector.heads_sp_shape_ok(build_model(MUTANTS["anchors_4"]))


@pytest.mark.parametrize("cin", [8, 16, 24, 32, 48, 256, 512, 1024, 1088])
def test_split_map_predicate_equals_the_kernels_checks(cin):
    """``backbone.sp_channels_ok`` -- the one statement of the SplitMap kernels' channel limits that the layers and the plan ask -- says yes exactly where the
    stride-1, stride-2 and fused-skip entry points accept the shape."""
    for cout in (32, 64, 96, 448, 512, 576, 960, 1024, 1088, 2048):
        assert bb.sp_channels_ok(cin, cout) == (_sp(cin, cout) == 0) == (_sp_s2(cin, cout) == 0), (cin, cout)
        assert bb.sp_channels_ok(cin, cout, skip=True) == (_sp_s2_skip(cin, cout) == 0), (cin, cout)
        assert bb.sp_channels_ok(None, cout) == (_sp(16, cout) == 0), cout
    for rows in (1, 31, 32, 33, 40):
        assert (rows <= ops.HEADS_SP_MAX_ROWS and cin % 16 == 0) == (_heads_sp(cin, rows) == 0), (cin, rows)


@pytest.mark.parametrize("name", list(MUTANTS))
def test_route_plan_prints_what_the_modules_decide(name):
    """One implementation: the string ``plan`` prints for a layer is the wording of the decision its module's ``forward`` dispatches on (``BasicBlock.route``,
    ``DoubleConv.on_split_maps``, the decode mixin, ``detector.heads_route``) -- in the default arithmetic asked without ``terms``, as ``forward`` asks.
    Fails when ``routes.py`` grows a rule of its own again."""
    h = MUTANTS[name]
    for terms in (None, 3):
        p = plan(h) if terms is None else plan(h, terms)
        r = p["layers"]
        model = build_model(h).eval()
        heads_split = (bb.HEAD_SPLIT_MAPS and model.shrink_conv.layers[0].on_split_maps(terms)) and model.backbone.heads_write_split(terms)
        for n, m in model.named_modules():
            if isinstance(m, bb.BasicBlock):
                d = m.route(terms)
                split = d.kind == bb.BLOCK_SPLIT
                assert (r[f"{n}.conv2"] == SP) == split and (r[f"{n}.conv1"] == SP) == (split and m.stride == 1), (n, d)
                assert r[f"{n}.conv1"].endswith("SplitMap out") == (split and m.stride == 2), (n, d)
                assert m.downsample is None or r[f"{n}.downsample.0"].startswith("pointwise") == m.skip_pointwise(), (n, d)
                assert m.takes_split_maps() == (m.route().kind == bb.BLOCK_SPLIT)
            elif isinstance(m, bb.DoubleConv):
                assert (r[f"{n}.double_conv.2"] == SP) == m.on_split_maps(terms), n
                assert (r[f"{n}.double_conv.0"] == SP) == bool(m is model.shrink_conv.layers[0] and heads_split), n
                assert r[f"{n}.double_conv.0"].endswith("SplitMap out") == (m.on_split_maps(terms) and r[f"{n}.double_conv.0"] != SP), n
        for i in range(model.backbone.num_levels):
            assert r[f"backbone.deblocks.{i}"].startswith("pointwise") == model.backbone.heads_pointwise()
            assert ("concatenated SplitMap" in r[f"backbone.deblocks.{i}"]) == bool(heads_split)
        assert r["cls_head"].startswith("pointwise") == detector.heads_route(model, terms).pointwise
        assert ("sparse canvas" in p["pillar"]) == detector.sparse_canvas_route(model, terms)


def _calls_stream(fn) -> bool:
    tree = ast.parse(inspect.getsource(fn))
    return any(isinstance(n, ast.Call) and isinstance(n.func, ast.Name) and n.func.id == "_stream" for n in ast.walk(tree))


def test_every_stream_launching_op_is_placed_on_its_arguments_device_once():
    """A public function of ``ops`` that launches on ``_stream()`` runs with its tensors' device current (``_device_op``) -- else, on a process with
    several GPUs, it launches on the current device's stream with another device's pointers.  Exactly one wrapper: a second one only costs a scan."""
    probe = ops._device_op(lambda: None).__code__
    wrong = []
    for name, fn in vars(ops).items():
        if name.startswith("_") or not inspect.isfunction(fn) or fn.__module__ != ops.__name__:
            continue
        depth, inner = 0, fn
        while hasattr(inner, "__wrapped__"):
            assert inner.__code__ is probe, name              # (the only decorator in the module)
            depth, inner = depth + 1, inner.__wrapped__
        if _calls_stream(inner) and depth != 1:
            wrong.append((name, depth))
        elif not _calls_stream(inner) and depth:
            wrong.append((name, depth))
    assert wrong == [], wrong


def test_device_placement_ignores_host_arguments():
    """``ops._device_tensor`` (what ``_device_op`` places an op by) looks through SplitMaps and lists / tuples, and finds nothing on the host."""
    cpu = torch.zeros(2)
    assert ops._device_tensor(ops.SplitMap.empty(1, 16, 2, 2, "cpu")) is None
    assert ops._device_tensor([(cpu, None, 3)]) is None and ops._device_tensor(cpu) is None and ops._device_tensor(None) is None
