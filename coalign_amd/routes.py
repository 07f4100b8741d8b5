"""Which kernel serves which layer of a config -- decided from the config alone, no GPU needed.

The detector picks its kernels per layer at run time; a layer whose shape a hand-written kernel does not take falls back to MIOpen / the per-scale NCHW fusion kernel /
the fp32 VALU encoder -- correct, slower, and until round 3 silent.  ``plan(hypes)`` builds the model of a hypes dictionary, asks every module the decision function its
``forward`` dispatches on (``backbone.conv3x3_route`` / ``pointwise_split``, ``BasicBlock.route``, ``DoubleConv.on_split_maps``, the decode mixin's ``heads_pointwise`` /
``heads_write_split``, ``NaiveCompressor.split_widths``, ``detector.heads_route`` / ``sparse_canvas_route`` / ``compressor_sparse_route`` / ``fusion_route``, ``DiscoFusion.kernel_route``, ``V2VNetFusion.kernel_route``, ``V2XViTFusion.kernel_route`` / ``window_kernel_reason``, ``When2comFusion.kernel_route`` / ``kernel_shape_reason``, ``PointPillarWhere2comm.kernel_route`` / ``kernel_route_reason``, ``PillarVFE.matrix_core_ok``) with the arithmetic
mode passed in, and words the answers -- this module holds no shape rule of its own -- so that a yaml that would leave the fast path shows up in a CPU test
(tests/test_host_cpu.py walks the reference's ``hypes_yaml/**/pointpillar*.yaml`` with it) instead of in a profile.
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
from . import detector
from .detector import BASELINE_REGISTRY, MODEL_REGISTRY, build_model
from .fusion import DiscoFusion, V2VNetFusion, V2XViTFusion, When2comFusion, Where2commFusion

EMU, F32, MIOPEN, ROCBLAS, POINTWISE = "conv3x3_emu (split 16-bit matrix cores)", "conv3x3 (fp32 matrix cores) / MIOpen by shape", "MIOpen", "rocBLAS (1x1 heads)", "pointwise"
WINO = "conv3x3_wino (Winograd F(2x2,3x3), split-bf16 matrix cores)"
SP = "conv3x3_sp (SplitMap input: operands by LDS-DMA, fp16 x 2)"
NARROW = "conv3x3_sp_narrow (16 / 32 output channels, weight-stationary, SplitMap out, fp16 x 2)"
COMPRESSOR_LIBRARY = MIOPEN + " (compressor: SURVEY 8a row D keeps it on the library)"
DISCO = "disco_fuse: warp + pixel-weight MLP + softmax in one launch"
DISCO_TORCH = "DiscoFusion op by op in PyTorch (channels outside the kernel's C % 32 == 0, 32 .. 384)"
V2V = "v2v_warp_split + conv3x3_sp + v2v_aggregate + conv3x3_sp + v2v_gate per iteration, one launch per stage over all (receiver, sender) pairs"
V2V_TORCH = "V2VNetFusion op by op in PyTorch"
V2X = ("v2x_agent_attention per encoder layer: LayerNorm + folded q | k' | v' projection + softmax over the agents + output projection + residual in two launches; "
       "pyramid window attention, split attention and feed-forward as torch ops on the device (library kernels)")
V2X_WINDOW = ("v2x_agent_attention + v2x_window_attention per encoder layer: the agent attention in two launches, the pyramid window attention with its split attention "
              "(LayerNorm + folded 9C x C projection, attention inside the 4 / 8 / 16 windows, branch weights, output projections + residual) in three or four; "
              "the feed-forward is still torch ops on the device (library kernels)")
V2X_WIN = "v2x_window_attention"
V2X_TORCH = "V2XViTFusion op by op in PyTorch"
V2X_ATT, V2X_UNREAD, V2X_LIBRARY = "v2x_agent_attention", "never read (every agent is of type 0; prior_feed has no caller)", ROCBLAS.split(" (")[0] + " (nn.Linear"
SP_S2 = "conv3x3_sp_s2 (SplitMap input and output, stride 2, fp16 x 2)"
W2C = ("v2v_warp_split + conv3x3_sp x 3 + conv3x3_sp_s2 x 3 + w2c_score + w2c_fuse per frame: the warped maps as SplitMaps, policy_net4 and the stacked key | query block on "
       "the SplitMap convolutions, the pooled heads with the softmax over the agents in two launches, warp and weighted sum in one; a one-agent frame is w2c_fuse alone")
W2C_TORCH = "When2comFusion op by op in PyTorch"
W2C_SCORE, W2C_UNREAD = "w2c_score", "never read (AdditiveAttentin.forward does not use linear_out)"
V2VR = ("v2vr_pairwise + v2v_warp_split + [conv3x3_sp + v2vr_pool_act] x 3 + conv3x3_sp_s2 + v2vr_pose_head (pose regression over all pairs) + v2vr_consistency (the whole "
        "weighted EM in one launch) + v2v_warp_split + conv3x3_sp + v2vr_pool_act + conv3x3_sp + v2vr_score_head (attention; its warp also serves the fusion's first "
        "iteration) + V2VNet's message passing with v2vr_aggregate (weighted sum over the senders)")
V2VR_TORCH = "PointPillarV2VNetRobust op by op in PyTorch"
V2VR_HEAD, V2VR_SCORE = "v2vr_pose_head", "v2vr_score_head"
W2COMM = ("w2comm_masks + w2comm_fuse_nhwc: the communication masks of every agent and level and the rates in one launch, then per frame the warp and fusion of "
          "the masked maps of all levels in one launch (channels-last; no masked map is written)")
W2COMM_PLAIN = "warp_fuse_nhwc: all scales in one launch (channels-last); no communication section: no masks, rate 0"
W2COMM_TORCH = "Where2comm op by op in PyTorch"
W2COMM_MASKS = "w2comm_masks (the smoothing runs inside the mask launch, fp32)"
STRIDED_SHRINK = MIOPEN + " (strided shrink-header convolution: library route)"
SPLIT_OUT = ", SplitMap out"
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


def pointwise_text(cin: int, terms: int) -> str:
    """backbone.pointwise_split in words."""
    return POINTWISE + (" (split-bf16 matrix cores)" if bb.pointwise_split(cin, terms) else " (fp32 matrix cores)")


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
            if isinstance(model, (detector.PointPillarBaseline, detector.PointPillarV2VNetRobust)) and not m._layer_ok(c1, bb.conv3x3_shape_ok):      # DoubleConv.forward builds no weight image for it
                note(f"{n}.double_conv.0", STRIDED_SHRINK if c1.stride != (1, 1) else MIOPEN + " (no weight image for the shape)", True)
                note(f"{n}.double_conv.2", conv3x3_text(c2, terms))
                continue
            note(f"{n}.double_conv.0", SP if split and heads_split and m is first_shrink else conv3x3_text(c1, terms) + (SPLIT_OUT if split else ""))
            note(f"{n}.double_conv.2", SP if split else conv3x3_text(c2, terms))
        elif isinstance(model, detector.PointPillarV2VNetRobust) and isinstance(m, (nn.Conv2d, nn.Linear)) and n.startswith(("pose_reg_net.", "attention_net.", "fusion_net.")):
            ok = model.kernel_route(model.out_channel, 1, terms)      # one decision for the three parts: the model's forward takes the kernels for all of them or for none
            if isinstance(m, nn.Linear) and n.startswith("fusion_net."):
                continue                                                # (fusion_net.mlp: noted with the fusion below)
            if isinstance(m, nn.Linear):
                head = V2VR_HEAD + " (all pairs in one workgroup, every row read once, fp32)" if n.startswith("pose_reg_net.") else V2VR_SCORE + " (cropped global max, linear, sigmoid and the weights, fp32)"
                note(n, head if ok else ROCBLAS.split(" (")[0] + " (nn.Linear, PointPillarV2VNetRobust op by op)", not ok)
            elif n.startswith("fusion_net."):
                what = (" (V2VNet: the warped-map and the ego columns as two C -> C convolutions)" if n.endswith("msg_cnn") else
                        " (V2VNet: update-gate rows of conv_gates stacked on conv_can, one convolution per GRU cell)")
                note(n, SP + what if ok else MIOPEN + " (V2VNetFusion op by op)", not ok)
            else:
                first = " (the warped-map and the ego columns as two C -> hidden convolutions over all pairs; bias, pooling and LeakyReLU in v2vr_pool_act)" if n.endswith("model.0") else ""
                note(n, (SP_S2 + " (LeakyReLU, pooling and the mean in v2vr_pose_head)" if m.stride[0] == 2 else SP + first) if ok else MIOPEN + " (PointPillarV2VNetRobust op by op)", not ok)
        elif isinstance(m, nn.Conv2d) and n.startswith("fusion_net.") and isinstance(model.fusion_net, DiscoFusion):
            ok = model.fusion_net.kernel_route(model.out_channel)      # the four 1x1 layers of PixelWeightLayer run inside the fusion launch
            note(n, "disco_fuse (pixel-weight MLP layer inside the fusion launch)" if ok else MIOPEN + " (DiscoFusion op by op)", not ok)
        elif isinstance(m, nn.Conv2d) and n.startswith("fusion_net.") and isinstance(model.fusion_net, V2VNetFusion):
            ok = model.fusion_net.kernel_route(model.out_channel, 1, terms)
            what = (" (V2VNet: the warped-map and the ego columns as two C -> C convolutions)" if n.endswith("msg_cnn") else
                    " (V2VNet: update-gate rows of conv_gates stacked on conv_can, one convolution per GRU cell)")
            note(n, SP + what if ok else MIOPEN + " (V2VNetFusion op by op)", not ok)
        elif isinstance(m, nn.Conv2d) and n.startswith("fusion_net.") and isinstance(model.fusion_net, When2comFusion):
            ok = model.fusion_net.kernel_route(model.out_channel, 1, terms)
            what = (" (When2com: stacked under key_net.conv1 in one launch; the ego's rows are read)" if n.startswith("fusion_net.query_net.") else
                    " (When2com: query_net.conv1 stacked under it in one launch)" if n.startswith("fusion_net.key_net.") else " (When2com: every agent's warped map)")
            note(n, (SP_S2 if m.stride[0] == 2 else SP + SPLIT_OUT) + what if ok else MIOPEN + " (When2comFusion op by op)", not ok)
        elif isinstance(m, nn.Linear) and n.startswith("fusion_net.") and isinstance(model.fusion_net, When2comFusion):
            ok = model.fusion_net.kernel_route(model.out_channel, 1, terms)
            if n.endswith("attention_net.linear_out"):
                note(n, W2C_UNREAD, False)
            elif ok:
                part = ("first layer, 4480 inputs spread over 256 workgroups" if n.endswith("fc.0") else "second layer" if n.endswith("fc.2") else
                        "folded with the attention's linear into one 128 x 128 matrix" if n.endswith("fc.4") else "folded into the key / query net's last layer")
                note(n, f"{W2C_SCORE} ({part}, fp32)", False)
            else:
                note(n, ROCBLAS.split(" (")[0] + " (nn.Linear, When2comFusion op by op)", True)
        elif isinstance(m, nn.Conv2d) and n.startswith("fusion_net.") and isinstance(model.fusion_net, Where2commFusion):      # naive_communication.gaussian_filter
            ok = model.kernel_route()
            note(n, W2COMM_MASKS if ok else MIOPEN + " (Where2comm op by op)", not ok)
        elif isinstance(m, nn.Linear) and n.startswith("fusion_net.") and isinstance(model.fusion_net, V2XViTFusion):
            ok = model.fusion_net.kernel_route(model.out_channel)
            leaf = n.split(".")
            if n.endswith("prior_feed") or (leaf[-2] in ("q_linears", "k_linears", "v_linears", "a_linears") and leaf[-1] != "0"):
                note(n, V2X_UNREAD, False)
            elif leaf[-2] in ("q_linears", "k_linears", "v_linears", "a_linears"):
                part = "output projection" if leaf[-2] == "a_linears" else "one third of the folded q | k' | v' projection"
                note(n, f"{V2X_ATT} ({part}, fp16 x 2 on the matrix cores)" if ok else V2X_LIBRARY + ", V2XViTFusion op by op)", not ok)
            elif ok and (".pwmsa." in n or ".split_attn." in n) and isinstance(m, nn.Linear) and model.fusion_net.window_kernel_reason(model.out_channel) is None:
                part = ("one third of the folded 9C x C projection, fp16 x 2 on the matrix cores" if leaf[-1] == "to_qkv" else "output projection, fp16 x 2 on the matrix cores"
                        if ".to_out." in n else "split attention's branch weights, fp32")
                note(n, f"{V2X_WIN} ({part})", False)
            else:
                block = "pyramid window attention" if ".pwmsa." in n else "split attention" if ".split_attn." in n else "feed-forward" if ".net." in n else "agent attention" if ".to_" in n else "time encoding"
                note(n, V2X_LIBRARY + f", {block}: torch op on the device)", True)
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
    fusion = None
    if isinstance(model, detector.PointPillarV2VNetRobust):                    # pose regression, EM, attention and the weighted V2VNet on the shrunk map
        f = model.fusion_net
        ok = model.kernel_route(model.out_channel, 1, terms)
        note("fusion_net.mlp", pointwise_text(f.mlp.in_features, terms) + ", 1 x 1 on the fused map" if ok else ROCBLAS.split(" (")[0] + " (nn.Linear, V2VNetFusion op by op)", not ok)
        if ok:
            fusion = V2VR
        else:
            hidden = model.pose_reg_net.pose_regression.model[0].out_channels
            why = ("the three warps normalise differently (robust vs v2vfusion downsample_rate x discrete_ratio)" if not model.one_normalisation() else
                   f"{model.out_channel} channels or hidden {hidden} outside C % 64 == 0" if model.out_channel % 64 or hidden % 64 else
                   "the fusion's own conditions (3 x 3 GRU kernels, widths) or the SplitMap arithmetic (fp16 x 2) is not in force")
            fusion = V2VR_TORCH + f" ({why})"
            fallbacks.append("fusion")
    elif isinstance(getattr(model, "fusion_net", None), V2VNetFusion):         # ONE single-scale module on the shrunk map
        f = model.fusion_net
        ok = f.kernel_route(model.out_channel, 1, terms)
        note("fusion_net.mlp", pointwise_text(f.mlp.in_features, terms) + ", 1 x 1 on the fused map" if ok else ROCBLAS.split(" (")[0] + " (nn.Linear, V2VNetFusion op by op)", not ok)
        if ok:
            fusion = V2V
        else:
            k3 = all(tuple(c.conv_gates.kernel_size) == (3, 3) for c in f.conv_gru.cell_list)
            why = ("GRU kernels other than 3 x 3" if not k3 else f"{model.out_channel} channels outside C % 64 == 0, C <= 512" if model.out_channel % 64 or model.out_channel > 512
                   or model.out_channel != f.msg_cnn.out_channels else "the SplitMap arithmetic (fp16 x 2) is not in force")
            fusion = V2V_TORCH + f" ({why})"
            fallbacks.append("fusion")
    elif isinstance(getattr(model, "fusion_net", None), V2XViTFusion):         # ONE single-scale module on the shrunk map
        f = model.fusion_net
        if f.kernel_route(model.out_channel):
            fusion = V2X_WINDOW if f.window_kernel_reason(model.out_channel) is None else V2X
        else:
            fusion = V2X_TORCH + f" ({f.kernel_shape_reason(model.out_channel) or 'training mode or force_torch'})"
            fallbacks.append("fusion")
    elif isinstance(getattr(model, "fusion_net", None), When2comFusion):       # ONE single-scale module on the shrunk map
        f = model.fusion_net
        if f.kernel_route(model.out_channel, 1, terms):
            fusion = W2C
        else:
            fusion = W2C_TORCH + f" ({f.kernel_shape_reason(model.out_channel, 1, terms) or 'training mode or force_torch'})"
            fallbacks.append("fusion")
    elif isinstance(getattr(model, "fusion_net", None), Where2commFusion):     # ONE module: the backbone's levels (multi_scale) or the shrunk map
        f = model.fusion_net
        if model.kernel_route() and (not f.multi_scale or (bb.NHWC_STAGE_OUTPUTS and bb.emu_active(terms))):      # (channels-last stage outputs)
            fusion = W2COMM if f.communication else W2COMM_PLAIN
        else:
            fusion = W2COMM_TORCH + f" ({model.kernel_route_reason() or 'stage outputs not channels-last, training mode or force_torch'})"
            fallbacks.append("fusion")
    elif isinstance(getattr(model, "fusion_net", None), (detector.MaxFusion, detector.AttFusion)):      # point_pillar_baseline: ONE module, the NCHW kernel
        fusion = "warp_fuse: one launch (NCHW, LDS-staged patches)"
        fallbacks.append("fusion")
    elif isinstance(getattr(model, "fusion_net", None), DiscoFusion):          # ONE single-scale module on the shrunk map, not a ModuleList
        if model.fusion_net.kernel_route(model.out_channel):
            fusion = DISCO
        else:
            fusion = DISCO_TORCH
            fallbacks.append("fusion")
    elif hasattr(model, "fusion_net"):
        dims = [int(d) for d in hypes["model"]["args"]["base_bev_backbone"]["num_filters"]]
        if len(model.fusion_net) != len(dims):
            dims = dims[-len(model.fusion_net):]
        if bb.NHWC_STAGE_OUTPUTS and bb.emu_active(terms) and detector.fusion_route(model, dims):      # (channels-last stage outputs)
            fusion = "warp_fuse_nhwc: all scales in one launch (channels-last)"
        else:
            fusion = "warp_fuse: one launch per scale (NCHW, LDS-staged patches)"
            fallbacks.append("fusion")
    return {"model": name, "outside_hot_path": None, "layers": layers, "pillar": pillar, "fusion": fusion, "fallbacks": fallbacks}


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
