"""Writes tests/golden/ssfa_reference.npz: the reference's OWN ``SSFA`` module (opencood/models/sub_modules/cia_ssd_utils.py:6-55) run in eval mode in float64 on a
[1, 128, 4, 6] input, with every parameter and buffer filled by the closed formula of tests/ssfa_reference.py (a function of the tensor's name and flat index;
no RNG, so the weights themselves need not be stored).  The fixture holds the state-dict names and shapes, the input and the output.

    python tests/golden/make_ssfa_golden.py <root of an OpenCOOD checkout>      (or OPENCOOD_ROOT=<root>)

Nothing of the reference is copied: its module is imported, filled, run and forgotten.  tests/test_ssfa_cpu.py rebuilds the same parameters in ``second.SSFA`` and
compares names, shapes and the output."""
import importlib
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from ssfa_reference import fill_by_formula_, formula_input      # noqa: E402

OUT = os.path.join(HERE, "ssfa_reference.npz")


def reference_ssfa(root: str):
    """The reference's SSFA class, through its package when that imports here, else from the module's file (it needs torch alone)."""
    sys.path.insert(0, root)
    try:
        return importlib.import_module("opencood.models.sub_modules.cia_ssd_utils").SSFA
    except Exception:      # noqa: BLE001 -- a package __init__ that needs modules absent here
        spec = importlib.util.spec_from_file_location("cia_ssd_utils", os.path.join(root, "opencood", "models", "sub_modules", "cia_ssd_utils.py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        return mod.SSFA


def main() -> int:
    root = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("OPENCOOD_ROOT", "")
    if not root or not os.path.isdir(os.path.join(root, "opencood")):
        print("no OpenCOOD checkout given: nothing written")
        return 1
    m = fill_by_formula_(reference_ssfa(root)({"feature_num": 128}).double()).eval()
    x = formula_input()
    with torch.no_grad():
        y = m(x)
    sd = m.state_dict()
    np.savez_compressed(OUT, names=np.array(list(sd)), shapes=np.array([",".join(str(int(v)) for v in t.shape) for t in sd.values()]), input=x.numpy(),
                        output=y.numpy())
    print(f"{OUT}: {len(sd)} tensors, output {tuple(y.shape)}, max |y| = {float(y.abs().max()):.4f}, {os.path.getsize(OUT)} bytes")
    return 0


if __name__ == "__main__":
    sys.exit(main())
