#!/usr/bin/env python
"""Generate tests/golden/when2com_fuse.npz by IMPORTING THE REFERENCE ITSELF (build container only: needs /root/reference; the ``.npz`` travels, this script's
import does not).  Usage:  python tests/golden/make_when2com_golden.py

What is pinned: the reference's ``When2commFusion`` (opencood/models/fuse_modules/fusion_in_one.py:354-431, with fuse_modules/when2com_fuse.py:133-363) called
unmodified in eval mode on a small batch -- C = 16, 9 x 14, record_len [3, 1], query_size 32, key_size 1024 -- with the affines of ``make_thetas`` on the ego row
(shift, rotation, one agent half outside) and the weights of ``synthetic.when2com_parameters_`` (seed 30: a softmax that is neither uniform nor one-hot).  The
module has six million parameters, so no tensor of them is stored: the fixture holds the inputs, the output, the per-frame logits and weights (the reference's own
sub-modules called on the reference's intermediate maps), per parameter its name, numel and float64 sum and sum of squares -- the test regenerates the parameters
and compares -- and the ``state_dict`` key list and numels of the reference's ``PointPillarBaseline`` built from its v2vnet yaml with ``fusion_method: when2comm``
and this project's ``when2comm`` section.  Only data goes into the fixture.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from make_disco_golden import REF, import_reference      # noqa: E402  (puts the repository and the reference on sys.path)
from v2v_reference import make_thetas                    # noqa: E402
from when2com_reference import parameter_checksums       # noqa: E402

YAML_V2V = REF + "/opencood/hypes_yaml/opv2v/lidar_only_with_noise/pointpillar_v2vnet.yaml"
ARGS = {"in_channels": 16, "H": 9, "W": 14, "query_size": 32, "key_size": 1024}
MODEL_SECTION = {"in_channels": 256, "H": 50, "W": 176, "query_size": 32, "key_size": 1024}
SEED = 30


def affines(L=5):
    """normalized_affine_matrix [2, L, L, 2, 3] float64: the ego row of frame 0's three agents from ``make_thetas`` (the other rows too; only row 0 is read)."""
    A = torch.zeros(2, L, L, 2, 3, dtype=torch.float64)
    A[..., 0, 0] = A[..., 1, 1] = 1.0
    A[0, :3, :3] = make_thetas(3, ARGS["H"], ARGS["W"], seed=40)
    return A


def inputs():
    C, H, W = ARGS["in_channels"], ARGS["H"], ARGS["W"]
    return torch.randn(4, C, H, W, generator=torch.Generator().manual_seed(41)), torch.tensor([3, 1]), affines()


def main():
    fio = import_reference("opencood.models.fuse_modules.fusion_in_one")
    from coalign_amd.synthetic import when2com_parameters_
    m = fio.When2commFusion(ARGS)
    when2com_parameters_(m, seed=SEED)
    m.eval()
    x, record_len, A = inputs()
    logits, weights = [], []
    with torch.no_grad():
        out = m(x, record_len, A)
        off = 0
        for b, n in enumerate(record_len.tolist()):      # the reference's own sub-modules, in the order of its forward
            v = fio.warp_affine_simple(x[off:off + n], A[b, 0, :n], (ARGS["H"], ARGS["W"]))
            off += n
            maps = m.query_key_net(v)
            keys, query = m.key_net(maps).unsqueeze(0), m.query_net(maps[0].unsqueeze(0)).unsqueeze(0)
            lg = torch.bmm(m.attention_net.linear_feat(keys), m.attention_net.linear_context(query).transpose(2, 1)).reshape(-1)
            logits.append(lg)
            weights.append(m.attention_net(query, keys, v.unsqueeze(0), sparse=False)[1].reshape(-1))
    print("output", tuple(out.shape), "max |out|", float(out.abs().max()), "logits", [t.tolist() for t in logits], "weights", [t.tolist() for t in weights])
    sums = parameter_checksums(m)
    fixture = {"x": x.numpy(), "record_len": record_len.numpy(), "affine": A.numpy(), "out": out.numpy(),
               "logits": torch.cat(logits).numpy(), "weights": torch.cat(weights).numpy(), "seed": np.array(SEED),
               "state_keys": np.array(list(m.state_dict().keys())), "param_names": np.array(list(sums.keys())),
               "param_numel": np.array([v[0] for v in sums.values()], dtype=np.int64),
               "param_sums": np.array([[v[1], v[2]] for v in sums.values()], dtype=np.float64)}
    yaml_utils = import_reference("opencood.hypes_yaml.yaml_utils")
    hypes = yaml_utils.load_yaml(YAML_V2V)
    hypes["model"]["args"]["fusion_method"] = "when2comm"
    hypes["model"]["args"]["when2comm"] = dict(MODEL_SECTION)
    model = import_reference("opencood.models.point_pillar_baseline").PointPillarBaseline(hypes["model"]["args"])
    fixture["model_state_keys"] = np.array(list(model.state_dict().keys()))
    fixture["model_state_numel"] = np.array([v.numel() for v in model.state_dict().values()], dtype=np.int64)
    path = os.path.join(HERE, "when2com_fuse.npz")
    np.savez_compressed(path, **fixture)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
