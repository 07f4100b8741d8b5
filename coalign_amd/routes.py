"""Which kernel serves which layer of a config -- decided from the config alone, no GPU needed.

The detector picks its kernels per layer at run time; a layer whose shape a hand-written kernel does not take falls back to MIOpen / the per-scale NCHW fusion kernel /
the fp32 VALU encoder -- correct, slower, and until round 3 silent.  ``plan(hypes)`` builds the model of a hypes dictionary and asks every module the decision function
its ``forward`` dispatches on, with the arithmetic mode passed in, and words the answers -- this module holds no shape rule of its own -- so that a yaml that would
leave the fast path shows up in a CPU test (tests/test_host_cpu.py walks the reference's ``hypes_yaml/**/pointpillar*.yaml`` with it) instead of in a profile.

The generic walk asks ``backbone.conv3x3_route`` / ``pointwise_split``, ``BasicBlock.route`` / ``skip_pointwise``, ``DoubleConv.on_split_maps``, the decode mixin's
``heads_pointwise`` / ``heads_write_split``, ``NaiveCompressor.takes_split_maps`` / ``split_widths``, ``detector.heads_route`` / ``sparse_canvas_route`` /
``compressor_sparse_route`` and ``PillarVFE.matrix_core_ok``.  The fusion line and every layer under ``fusion_net.`` are worded by the family itself, beside its route
decision (``kernel_route`` = eval mode, not ``force_torch``, no ``kernel_shape_reason``): the hooks ``plan_fusion(channels, terms) -> (line, fallback, {layers noted
with it})`` and ``plan_layer(name, layer, channels, terms) -> (line, fallback) | None`` of the fusion module, or of the model where the decision is the model's
(the multi-scale fusion: ``detector.fusion_route``; Where2comm; the pose-robust V2VNet, which also words ``pose_reg_net.`` and ``attention_net.``).  Adding a family
adds no line here.
The line of the merged 1x1 heads names the kernel that reads a float32 map (pointwise within its Cin limit, else rocBLAS, listed as a fallback): where a one-layer shrink header
hands them a SplitMap (``detector.heads_route(model).split_in``) they run on ``heads_sp`` whatever that line says.

    python -m coalign_amd.routes [--baselines] <hypes.yaml> [...]          # prints the plan(s) as JSON; --baselines: plan DiscoNet and point_pillar_baseline too
"""
from __future__ import annotations

import json
import sys
from typing import Dict

import torch.nn as nn

from . import backbone as bb
from . import detector, fusion, v2v_robust
from .backbone import MIOPEN, POINTWISE, ROCBLAS, SP, SP_S2, SPLIT_OUT, pointwise_text  # noqa: F401  (the shared kernel names, importable from here)
from .detector import BASELINE_REGISTRY, MODEL_REGISTRY, build_model

# the families' own wording, importable from here
DISCO, V2V = fusion.DiscoFusion.KERNELS, fusion.V2VNetFusion.KERNELS
V2X, V2X_WINDOW = fusion.V2XViTFusion.KERNELS, fusion.V2XViTFusion.KERNELS_WINDOW
V2X_FFN, V2X_WINDOW_FFN = fusion.V2XViTFusion.KERNELS_FFN, fusion.V2XViTFusion.KERNELS_WINDOW_FFN
W2C, W2C_TORCH, W2C_SCORE, W2C_UNREAD = fusion.When2comFusion.KERNELS, fusion.When2comFusion.TORCH, fusion.When2comFusion.SCORE, fusion.When2comFusion.UNREAD
V2VR, V2VR_TORCH = v2v_robust.KERNELS, v2v_robust.TORCH
W2COMM, W2COMM_MASKS = fusion.Where2commFusion.KERNELS, fusion.Where2commFusion.MASKS

EMU, F32 = "conv3x3_emu (split 16-bit matrix cores)", "conv3x3 (fp32 matrix cores) / MIOpen by shape"
WINO = "conv3x3_wino (Winograd F(2x2,3x3), split-bf16 matrix cores)"
NARROW = "conv3x3_sp_narrow (16 / 32 output channels, weight-stationary, SplitMap out, fp16 x 2)"
COMPRESSOR_LIBRARY = MIOPEN + " (compressor: SURVEY 8a row D keeps it on the library)"
STRIDED_SHRINK = MIOPEN + " (strided shrink-header convolution: library route)"
SPARSE_IN = ", sparse canvas in"
DEFAULT_TERMS = bb.DEFAULT_CONV_EMU_TERMS      # the 2-way fp16 split since round 4


def conv3x3_text(conv: nn.Conv2d, terms: int) -> str:
    """backbone.conv3x3_route in words."""
    s = conv.stride[0]
    if tuple(conv.kernel_size) != (3, 3) or conv.stride[0] != conv.stride[1]:
        return MIOPEN
    r = bb.conv3x3_route(conv.in_channels, conv.out_channels, s, terms)
    if r.kernel == bb.C3_EMU:
        if r.wino:
            return WINO + " when its input is channels-last (COALIGN_WINOGRAD=1)"
        return EMU + (", tap-major image" if r.tap_major else ", tap-pair image") + ", " + bb.EMU_MODE_NAMES[terms]
    if r.kernel == bb.C3_F32:
        return F32 + (" (the fp16 split serves the tap-major and the strided images)" if bb.emu_active(terms) else "")
    if bb.conv3x3_shape_ok(conv.in_channels, conv.out_channels, s):
        return MIOPEN + " (native mode, strided)"
    return MIOPEN + f" (unpackable: Cout {conv.out_channels} % 64 or Cin {conv.in_channels} % 8 or stride {s})"


def plan(hypes: dict, terms: int = DEFAULT_TERMS, baselines: bool = False) -> Dict[str, object]:
    """-> {"model", "layers": {module name: route}, "pillar", "fusion", "fallbacks": [names of 3x3 / pointwise layers NOT on a hand-written
    kernel], "outside_hot_path": reason or None}.  ``baselines``: also plan the comparison baselines (``detector.BASELINE_REGISTRY``: DiscoNet), which ``build_model``
    constructs but which are no family of the CoAlign hot path -- without it they are reported as outside it, like every other family."""
    name = hypes["model"]["core_method"]
    if name not in MODEL_REGISTRY and not (baselines and name in BASELINE_REGISTRY):
        return {"model": name, "outside_hot_path": f"model family '{name}' is not part of the CoAlign hot path", "layers": {}, "fallbacks": []}
    model = build_model(hypes).eval()                       # (the decision functions answer for the module's mode)
    layers: Dict[str, str] = {}
    fallbacks = []

    def note(n, route, is_fallback=None):
        layers[n] = route
        if route.startswith(MIOPEN) if is_fallback is None else is_fallback:
            fallbacks.append(n)

    # the up-sampling heads write the concatenated map as ONE SplitMap: the shrink header's first DoubleConv takes it (detector.fuse_and_head) and the heads can write it
    first_shrink = model.shrink_conv.layers[0] if getattr(model, "shrink_flag", False) and len(model.shrink_conv.layers) else None
    heads_split = bool(first_shrink is not None and bb.HEAD_SPLIT_MAPS and first_shrink.on_split_maps(terms) and model.backbone.heads_write_split(terms))
    # the family words its own lines: the model where the decision is the model's, else its fusion module
    hook = model if hasattr(model, "plan_fusion") else getattr(model, "fusion_net", None)
    owned = tuple(getattr(hook, "plan_prefixes", ("fusion_net.",))) if hasattr(hook, "plan_layer") else ()
    channels = getattr(model, "out_channel", None)
    for n, m in model.named_modules():
        if isinstance(m, bb.NaiveCompressor):
            # the SplitMap route puts the encoder on the narrow kernel or on conv3x3_sp (split_widths), both decoder layers on conv3x3_sp; else the library
            widths = m.split_widths() if m.takes_split_maps(terms) else None
            sparse_in = SPARSE_IN if detector.compressor_sparse_route(model, terms) else ""
            for cn, c in m.named_modules():
                if isinstance(c, nn.Conv2d) and widths is None:
                    note(f"{n}.{cn}", COMPRESSOR_LIBRARY, True)
                elif isinstance(c, nn.Conv2d):
                    pad = f", mid {m.encoder[0].out_channels} zero-padded to {widths[1]}" if widths[1] != m.encoder[0].out_channels else ""
                    note(f"{n}.{cn}", (NARROW + sparse_in if widths[0] == "narrow" and cn == "encoder.0" else SP) + (pad if cn in ("encoder.0", "decoder.0") else ""), False)
        elif isinstance(m, bb.BasicBlock):
            split = m.route(terms).kind == bb.BLOCK_SPLIT
            note(f"{n}.conv1", SP if split and m.stride == 1 else conv3x3_text(m.conv1, terms) + (SPLIT_OUT if split else ""))
            note(f"{n}.conv2", SP if split else conv3x3_text(m.conv2, terms))
            if m.downsample is not None:
                note(f"{n}.downsample.0", pointwise_text(m.downsample[0].in_channels, terms) if m.skip_pointwise() else MIOPEN + " (skip convolution outside the pointwise kernel's shapes)")
        elif isinstance(m, bb.DoubleConv):
            split, c1, c2 = m.on_split_maps(terms), m.double_conv[0], m.double_conv[2]
            if getattr(model, "plan_words_library_shrink", False) and not m._layer_ok(c1, bb.conv3x3_shape_ok):      # DoubleConv.forward builds no weight image for it
                note(f"{n}.double_conv.0", STRIDED_SHRINK if c1.stride != (1, 1) else MIOPEN + " (no weight image for the shape)", True)
                note(f"{n}.double_conv.2", conv3x3_text(c2, terms))
                continue
            note(f"{n}.double_conv.0", SP if split and heads_split and m is first_shrink else conv3x3_text(c1, terms) + (SPLIT_OUT if split else ""))
            note(f"{n}.double_conv.2", SP if split else conv3x3_text(c2, terms))
        elif isinstance(m, (nn.Conv2d, nn.Linear)) and n.startswith(owned) and (line := hook.plan_layer(n, m, channels, terms)) is not None:
            note(n, *line)
        elif isinstance(m, nn.Conv2d) and n not in layers and "naive_compressor" not in n:
            if tuple(m.kernel_size) == (1, 1) and n.endswith("_head"):
                ok = detector.heads_route(model, terms).pointwise
                note(n, pointwise_text(m.in_channels, terms) + ", merged 1x1 heads" if ok else ROCBLAS, not ok)
            else:
                note(n, conv3x3_text(m, terms))
    backbone = model.backbone
    for i in range(len(backbone.deblocks)):
        ok = backbone.heads_pointwise() and i < backbone.num_levels
        note(f"backbone.deblocks.{i}", pointwise_text(backbone.deblocks[i][0].in_channels, terms) + (", writes its slice of the concatenated SplitMap" if heads_split else ", writes its slice of the concatenation")
             if ok else MIOPEN + " + bias_act")
    vfe = model.pillar_vfe
    P = int(hypes.get("preprocess", {}).get("args", {}).get("max_points_per_voxel", 0))      # (absent: the preprocessor's default fits the matrix-core encoders)
    if len(vfe.pfn_layers) != 1:
        pillar = "unsupported: stacked PFN layers"
    elif not vfe.matrix_core_ok(P):
        pillar = "fp32 VALU encoder (distance feature / P > 32 / C > 64)"
    else:
        pillar = ("matrix-core encoder (one fp16 matrix instruction per pillar and 32 channels on a 22-bit operand split), ONE launch, sparse canvas read by the first ResNet block"
                  if detector.sparse_canvas_route(model, terms) else
                  "matrix-core encoder (one fp16 matrix instruction per pillar and 32 channels on a 22-bit operand split), ONE launch, sparse canvas read by the compressor's encoder"
                  if detector.compressor_sparse_route(model, terms) else
                  "matrix-core encoder (linearised PFN, split-bf16), persistent dense canvas" if bb.emu_active(terms) else "matrix-core encoder, NCHW strip writer")
    fusion_line = None
    if hasattr(hook, "plan_fusion"):
        fusion_line, is_fallback, noted_with_it = hook.plan_fusion(channels, terms)
        for n, line in noted_with_it.items():
            note(n, *line)
        if is_fallback:
            fallbacks.append("fusion")
    return {"model": name, "outside_hot_path": None, "layers": layers, "pillar": pillar, "fusion": fusion_line, "fallbacks": fallbacks}


def summary(p: dict) -> dict:
    """Counts per route + the fallback list: what the walk test records per yaml."""
    counts: Dict[str, int] = {}
    for r in p["layers"].values():
        key = r.split(" (")[0].split(",")[0]
        counts[key] = counts.get(key, 0) + 1
    return {"model": p["model"], "outside_hot_path": p["outside_hot_path"], "routes": counts, "pillar": p.get("pillar"), "fusion": p.get("fusion"),
            "fallbacks": p["fallbacks"]}


if __name__ == "__main__":
    from .config import load_yaml
    out = {}
    for path in [a for a in sys.argv[1:] if a != "--baselines"]:
        try:
            out[path] = summary(plan(load_yaml(path), baselines="--baselines" in sys.argv[1:]))
        except Exception as e:      # noqa: BLE001  (other model families' yamls need parsers / keys outside the hot path)
            out[path] = {"outside_hot_path": f"{type(e).__name__}: {str(e)[:120]}"}
    print(json.dumps(out, indent=1))
