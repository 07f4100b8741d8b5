"""Regenerate tests/golden/plan_snapshot.json.gz: what ``coalign_amd.routes.plan`` prints and what a seeded construction builds, recorded BEFORE the detectors were
given one pillar trunk and the fusion families their own plan wording.  tests/test_plan_snapshot_cpu.py recomputes all of it (``snapshot()`` below) and compares with
``==``: a refactor of ``detector.py`` / ``routes.py`` must reproduce the file, never regenerate it.  CPU only.

  * ``plans``: ``plan(h, terms, baselines=True)`` at terms 0 / 2 / 3 / 16 for every shipped config with a ``model`` section, for the 16 mutants of
    tests/test_routes_cpu.py and for the fallback mutants below (one per baseline family and reason it can give for leaving its kernel route);
  * ``state``: per shipped config the ORDERED ``state_dict`` keys with shapes and, after ``torch.manual_seed(0); build_model(h)``, the SHA-256 of every tensor.

    python tests/golden/make_plan_snapshot.py
"""
import copy
import glob
import gzip
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.dirname(HERE)):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

from coalign_amd import build as _build  # noqa: E402
from coalign_amd import routes, v2xvit  # noqa: E402
from coalign_amd.config import builtin_config  # noqa: E402
from coalign_amd.detector import build_model  # noqa: E402

PATH = os.path.join(HERE, "plan_snapshot.json.gz")
TERMS = (0, 2, 3, 16)


def shipped() -> dict:
    out = {}
    for path in sorted(glob.glob(os.path.join(_build.PKG, "configs", "*.yaml"))):
        name = os.path.splitext(os.path.basename(path))[0]
        h = builtin_config(name)
        if "model" in h:                      # (lss_coalign_fusion has none)
            out[name] = h
    return out


def _edit(cfg: str, fn) -> dict:
    h = copy.deepcopy(builtin_config(cfg))
    fn(h["model"]["args"])
    return h


def _robust_grid(a):
    a["point_pillar_scatter"]["grid_size"] = [112, 56, 1]


def fallback_mutants() -> dict:
    """name -> hypes.  A name ending in ``@window`` is planned with V2X-ViT's window kernels switched on."""
    def v2v_width(c):
        def fn(a):
            a["shrink_header"]["dim"] = [c]
            a["v2vnet"]["in_channels"] = c
        return fn

    def robust(fn):
        def both(a):
            _robust_grid(a)
            fn(a)
        return both

    def w2comm_plain_backbone(a):
        a["base_bev_backbone"]["resnet"] = False

    def w2comm_single(a):
        a["where2comm"]["multi_scale"] = False

    m = {
        "disco_48": _edit("mini_pointpillar_disconet", lambda a: a["shrink_header"].update(dim=[48])),
        "disco_416": _edit("mini_pointpillar_disconet", lambda a: a["shrink_header"].update(dim=[416])),
        "v2vnet_48": _edit("mini_pointpillar_v2vnet", v2v_width(48)),
        "v2vnet_96": _edit("mini_pointpillar_v2vnet", v2v_width(96)),
        "v2vnet_576": _edit("mini_pointpillar_v2vnet", v2v_width(576)),
        "v2vnet_gru_5x5": _edit("mini_pointpillar_v2vnet", lambda a: a["v2vnet"]["conv_gru"].update(kernel_size=[[5, 5]])),
        "v2vnet_map_128_module_64": _edit("mini_pointpillar_v2vnet", lambda a: a["shrink_header"].update(dim=[128])),
        "v2xvit_4_heads_of_16": _edit("mini_pointpillar_v2xvit", lambda a: a["v2xvit"]["transformer"]["encoder"]["cav_att_config"].update(heads=4, dim_head=16)),
        "v2xvit_not_hetero": _edit("mini_pointpillar_v2xvit", lambda a: a["v2xvit"]["transformer"]["encoder"]["cav_att_config"].update(use_hetero=False)),
        "v2xvit_mini@window": builtin_config("mini_pointpillar_v2xvit"),
        "v2xvit_opv2v@window": builtin_config("opv2v_pointpillar_v2xvit"),
        "v2xvit_4_heads_of_16@window": _edit("mini_pointpillar_v2xvit", lambda a: a["v2xvit"]["transformer"]["encoder"]["cav_att_config"].update(heads=4, dim_head=16)),
        "when2com_map_128_module_64": _edit("mini_pointpillar_when2com", lambda a: a["shrink_header"].update(dim=[128])),
        "when2com_40": _edit("mini_pointpillar_when2com", lambda a: (a["shrink_header"].update(dim=[40]), a["when2comm"].update(in_channels=40))),
        "robust_hidden_48": _edit("mini_pointpillar_v2vnet_robust", robust(lambda a: a["robust"].update(hidden_dim=48))),
        "robust_two_normalisations": _edit("mini_pointpillar_v2vnet_robust", robust(lambda a: a["v2vfusion"].update(downsample_rate=4))),
        "robust_96": _edit("mini_pointpillar_v2vnet_robust", robust(lambda a: (a["shrink_header"].update(dim=[96]), a["v2vfusion"].update(in_channels=96), a["robust"].update(feature_dim=96)))),
        "robust_gru_5x5": _edit("mini_pointpillar_v2vnet_robust", robust(lambda a: a["v2vfusion"]["conv_gru"].update(kernel_size=[[5, 5]]))),
        "robust_compression": _edit("mini_pointpillar_v2vnet_robust", robust(lambda a: (a["shrink_header"].update(dim=[256]), a["v2vfusion"].update(in_channels=256), a["robust"].update(feature_dim=256), a.update(compression=4)))),
        "where2comm_plain_backbone": _edit("mini_pointpillar_where2comm", w2comm_plain_backbone),
        "where2comm_single_scale": _edit("mini_pointpillar_where2comm", w2comm_single),
        "where2comm_96": _edit("mini_pointpillar_where2comm", lambda a: (a["base_bev_backbone"].update(num_filters=[96, 128, 256]), a["where2comm"].update(num_filters=[96, 128, 256]))),
        "where2comm_feature_dim": _edit("mini_pointpillar_where2comm", lambda a: a["where2comm"].update(num_filters=[64, 128, 128])),
        "where2comm_even_smoothing": _edit("mini_pointpillar_where2comm", lambda a: a["where2comm"]["communication"]["gaussian_smooth"].update(k_size=4)),
        "where2comm_9_anchors": _edit("mini_pointpillar_where2comm", lambda a: a.update(anchor_number=9)),
        "where2comm_no_communication": _edit("mini_pointpillar_where2comm", lambda a: a["where2comm"].pop("communication")),
        "where2comm_max": _edit("mini_pointpillar_where2comm", lambda a: a["where2comm"].update(agg_operator={"mode": "MAX"})),
        "baseline_max": _edit("mini_pointpillar_v2vnet", lambda a: a.update(fusion_method="max")),
        "baseline_att": _edit("mini_pointpillar_v2vnet", lambda a: a.update(fusion_method="att", att={"feat_dim": 64})),
        "baseline_disconet": _edit("mini_pointpillar_v2vnet", lambda a: a.update(fusion_method="disconet", disconet={"feat_dim": 64})),
        "baseline_disconet_48": _edit("mini_pointpillar_v2vnet", lambda a: (a.update(fusion_method="disconet", disconet={"feat_dim": 48}), a["shrink_header"].update(dim=[48]))),
        "baseline_v2vnet_compression": _edit("mini_pointpillar_v2vnet", lambda a: a.update(compression=4)),
        "baseline_v2vnet_resnet": _edit("mini_pointpillar_v2vnet", lambda a: a["base_bev_backbone"].update(resnet=True)),
        "multiscale_att_feat_dim": _edit("mini_coalign", lambda a: a["att"].update(feat_dim=[32, 128, 256])),
        "multiscale_max": _edit("mini_coalign", lambda a: a.update(fusion_method="max")),
        "multiscale_plain_backbone": _edit("mini_coalign", lambda a: a["base_bev_backbone"].update(resnet=False)),
        "multiscale_compression": _edit("mini_coalign", lambda a: a.update(compression=4)),
    }
    return m


def _plans(h: dict, window: bool = False) -> dict:
    keep = v2xvit.V2X_WINDOW_KERNELS
    v2xvit.V2X_WINDOW_KERNELS = window
    try:
        return {str(t): routes.plan(copy.deepcopy(h), t, baselines=True) for t in TERMS}
    finally:
        v2xvit.V2X_WINDOW_KERNELS = keep


def _state(h: dict) -> list:
    torch.manual_seed(0)
    sd = build_model(copy.deepcopy(h)).state_dict()
    return [[k, list(v.shape), hashlib.sha256(v.detach().contiguous().cpu().numpy().tobytes()).hexdigest()] for k, v in sd.items()]


def snapshot() -> dict:
    from test_routes_cpu import MUTANTS
    configs = shipped()
    plans = {"config:" + n: _plans(h) for n, h in configs.items()}
    plans.update({"mutant:" + n: _plans(h) for n, h in MUTANTS.items()})
    plans.update({"fallback:" + n: _plans(h, n.endswith("@window")) for n, h in fallback_mutants().items()})
    return {"plans": plans, "state": {n: _state(h) for n, h in configs.items()}}


def load() -> dict:
    with gzip.open(PATH, "rt") as f:
        return json.load(f)


if __name__ == "__main__":
    snap = snapshot()
    text = json.dumps(snap, indent=0)
    with gzip.GzipFile(PATH, "wb", mtime=0) as f:
        f.write(text.encode())
    reasons = sorted({p["fusion"] for per in snap["plans"].values() for p in per.values() if "fusion" in p.get("fallbacks", [])})
    print(f"{len(snap['plans'])} plan sets, {len(snap['state'])} state dicts, {len(text)} bytes of JSON, {os.path.getsize(PATH)} gzipped")
    print("\n".join(reasons))
