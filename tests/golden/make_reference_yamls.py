"""Regenerate tests/golden/reference_yamls.json: three of the reference's own hypes yamls as coalign_amd.config.load_yaml reads them -- the optimizer's
``eps`` and the ``model`` and ``postprocess`` sections (``grid_size``, an int64 array after the yaml parser, stored as a list).
tests/test_host_cpu.py::test_unchanged_reference_yamls_load_and_build compares the shipped configs against it and builds the models from it.

    python tests/golden/make_reference_yamls.py <reference checkout>/opencood/hypes_yaml
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from coalign_amd.config import load_yaml  # noqa: E402

YAMLS = ("opv2v/lidar_only_with_noise/coalign/pointpillar_coalign.yaml", "opv2v/lidar_only_with_noise/pointpillar_single.yaml",
         "dairv2x/lidar_only_with_noise/coalign/pointpillar_coalign.yaml")


def main(base):
    table = {}
    for rel in YAMLS:
        h = load_yaml(os.path.join(base, rel))
        table[rel] = {"optimizer_eps": h["optimizer"]["args"]["eps"], "model": h["model"], "postprocess": h["postprocess"]}
    out = os.path.join(os.path.dirname(os.path.abspath(__file__)), "reference_yamls.json")
    json.dump(table, open(out, "w"), indent=1, sort_keys=True, default=lambda a: a.tolist() if isinstance(a, np.ndarray) else a)
    print(f"{len(table)} yamls -> {out}")


if __name__ == "__main__":
    main(sys.argv[1])
