#!/usr/bin/env python
"""Generate tests/golden/disco_fuse.npz by IMPORTING THE REFERENCE ITSELF (build container only: needs /root/reference; the ``.npz`` travels, this script's
import does not).  Usage:  python tests/golden/make_disco_golden.py

What is pinned: the reference's ``DiscoFusion`` (opencood/models/fuse_modules/fusion_in_one.py:138-171, with ``PixelWeightLayer``,
fuse_modules/disco_fuse.py:76-99) called unmodified in eval mode on a small batch -- C = 64, 9 x 14, record_len [3, 1] -- with non-default BatchNorm running
statistics and weight scales chosen so that the last ReLU leaves most logits positive (the softmax weights then differ between agents: the fixture sees the
MLP).  Stored: the inputs, the ``state_dict`` (names and tensors), the output, and the ``state_dict`` key list of the reference's ``PointPillarDiscoNet`` built
from its unchanged OPV2V yaml.  Only data goes into the fixture.

Optional third-party modules the reference imports at module scope but that are absent here (icecream, turtle's tkinter, ...) are replaced by inert stubs.
"""
import importlib
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"
YAML_DISCO = REF + "/opencood/hypes_yaml/opv2v/lidar_only_with_noise/pointpillar_disconet.yaml"
sys.path.insert(0, REPO)
sys.path.insert(0, REF)


class _Inert(types.ModuleType):
    __path__ = []

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        return _Inert(self.__name__ + "." + name)

    def __call__(self, *a, **k):
        return None


def import_reference(name):
    for stub in ("icecream", "turtle"):              # (turtle: the standard module would pull in tkinter)
        sys.modules.setdefault(stub, _Inert(stub))
    for _ in range(64):
        try:
            return importlib.import_module(name)
        except ModuleNotFoundError as e:
            if e.name is None or (e.name.startswith("opencood") and e.name != "opencood.utils.box_overlaps"):      # (the un-built Cython extension)
                raise
            sys.modules[e.name] = _Inert(e.name)
    raise ImportError(name)


def affines(L=5):
    """normalized_affine_matrix [2, L, L, 2, 3] float64: row [b, 0, j] maps the ego grid into agent j -- identity, a sub-pixel shift, a 30 degree rotation."""
    A = torch.zeros(2, L, L, 2, 3, dtype=torch.float64)
    A[..., 0, 0] = A[..., 1, 1] = 1.0
    A[0, 0, 1, :, 2] = torch.tensor([0.043, -0.031], dtype=torch.float64)
    c, s = np.cos(np.pi / 6), np.sin(np.pi / 6)
    A[0, 0, 2] = torch.tensor([[c, -s * 9 / 14, 0.11], [s * 14 / 9, c, -0.07]], dtype=torch.float64)
    return A


def main():
    fio = import_reference("opencood.models.fuse_modules.fusion_in_one")
    torch.manual_seed(20)
    C, H, W = 64, 9, 14
    m = fio.DiscoFusion(C)
    from coalign_amd.synthetic import disco_parameters_
    disco_parameters_(m.pixel_weight_layer, seed=20)
    m.eval()
    g = torch.Generator().manual_seed(21)
    x = torch.randn(4, C, H, W, generator=g)
    record_len = torch.tensor([3, 1])
    A = affines()
    with torch.no_grad():
        out = m(x, record_len, A)
        logits = m.pixel_weight_layer(torch.cat((x[:3], x[:1].expand(3, -1, -1, -1)), dim=1))
    print("output", tuple(out.shape), "share of positive logits (unwarped probe)", float((logits > 0).float().mean()))
    sd = m.state_dict()
    fixture = {"x": x.numpy(), "record_len": record_len.numpy(), "affine": A.numpy(), "out": out.numpy(),
               "state_keys": np.array(list(sd.keys())), **{"sd." + k: v.numpy() for k, v in sd.items()}}
    # the model's state_dict names, from the reference's unchanged yaml (its range shrunk: the names do not depend on it)
    yaml_utils = import_reference("opencood.hypes_yaml.yaml_utils")
    hypes = yaml_utils.load_yaml(YAML_DISCO)
    model_mod = import_reference("opencood.models.point_pillar_disconet")
    model = model_mod.PointPillarDiscoNet(hypes["model"]["args"])
    fixture["model_state_keys"] = np.array(list(model.state_dict().keys()))
    fixture["model_state_numel"] = np.array([v.numel() for v in model.state_dict().values()], dtype=np.int64)
    path = os.path.join(HERE, "disco_fuse.npz")
    np.savez_compressed(path, **fixture)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
