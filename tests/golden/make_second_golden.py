"""Regenerate tests/golden/second_voxel_params.json: the reference's OWN ``load_voxel_params`` (opencood/hypes_yaml/yaml_utils.py:52-94, loaded from its file: yaml
and numpy only) on its six SECOND yamls -- ``SECOND.yaml`` and ``coalign/SECOND_uncertainty.yaml`` of opv2v, v2xsim and dairv2x.  Per yaml the sections the parser
reads as they stand in the file (``input``) and what the parser makes of them (``output``).  tests/test_sparse3d_cpu.py holds ``coalign_amd.config.load_voxel_params``
to it.

    python tests/golden/make_second_golden.py <reference checkout>/opencood/hypes_yaml
"""
import copy
import importlib.util
import json
import os
import sys

import yaml

YAMLS = tuple(f"{d}/lidar_only_with_noise/{f}" for d in ("opv2v", "v2xsim", "dairv2x") for f in ("SECOND.yaml", "coalign/SECOND_uncertainty.yaml"))
SECTIONS = ("preprocess", "postprocess", "model", "box_align_pre_calc")


def main(base):
    spec = importlib.util.spec_from_file_location("reference_yaml_utils", os.path.join(base, "yaml_utils.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    table = {}
    for rel in YAMLS:
        raw = yaml.load(open(os.path.join(base, rel)), Loader=yaml.Loader)
        assert raw["yaml_parser"] == "load_voxel_params", rel
        raw = {k: raw[k] for k in SECTIONS if k in raw}
        table[rel] = {"input": copy.deepcopy(raw), "output": mod.load_voxel_params(copy.deepcopy(raw))}
    out = os.path.join(os.path.dirname(os.path.abspath(__file__)), "second_voxel_params.json")
    json.dump(table, open(out, "w"), indent=1, sort_keys=True)
    print(f"{len(table)} yamls -> {out}")


if __name__ == "__main__":
    main(sys.argv[1])
