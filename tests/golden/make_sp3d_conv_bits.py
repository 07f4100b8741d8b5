"""Writes tests/golden/sp3d_conv_bits.npz: one ordinary (16, 32, 3) submanifold layer on the 257-row case of tests/sparse3d_cases.py -- folded weight
[Cout, taps, Cin], shift, features, indices -- and the bits ``coalign_sp3d_conv`` gives for it on the MI355X.

The fixture was recorded at the LAST COMMIT WHOSE WEIGHT IMAGE HAD NO PER-CHANNEL POWER OF TWO (``pack_sp3d_weights`` fed the folded weights straight to the sp16
split).  Every folded |w| is at least 2^-7, so both halves of every pair are normal fp16 numbers, and scaling a row by a power of two changes no bit of the sum:
tests/test_sparse3d_limits_gpu.py asserts that the present kernel still gives these bits.  Running this script again records the present kernel's bits instead,
which proves nothing -- keep the file.

    python tests/golden/make_sp3d_conv_bits.py [out.npz]        (needs the GPU)
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]
import sparse3d_cases as cases  # noqa: E402
import sparse3d_limit_cases as limits  # noqa: E402
from coalign_amd import ops  # noqa: E402


def main():
    dev = torch.device("cuda:0")
    case = next(c for c in cases.CASES if c.name == "rows_257")
    layer = limits.ordinary_layer()
    w, shift = limits.folded(layer)
    w = w.reshape(32, 27, 16).contiguous()
    assert float(w.abs().min()) >= 2.0 ** -7 and float(w.abs().max()) < 1.0
    feats = cases.features(case, 16, seed=3)
    n = case.indices.shape[0]
    idx, count = case.indices.to(dev), torch.tensor([n], dtype=torch.int32, device=dev)
    index = ops.sp3d_index_build(idx, count, case.batch, case.shape)
    nbr = ops.sp3d_neighbors(idx, count, case.batch, case.shape, index, n, case.shape, 3, 1, 1)
    y = ops.sp3d_conv(feats.to(dev), nbr, count, 32, ops.pack_sp3d_weights(w).to(dev), shift.to(dev))
    assert bool((y > 0).any()) and bool((y == 0).any()) and bool(((nbr >= 0).sum(dim=0) > 1).any())       # ReLU cuts; some rows have neighbours
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "sp3d_conv_bits.npz")
    np.savez(out, weight=w.numpy(), shift=shift.numpy(), feats=feats.numpy(), indices=case.indices.numpy(), batch=np.int32(case.batch),
             shape=np.asarray(case.shape, dtype=np.int32), out=y.cpu().numpy())
    print(f"wrote {out}: {n} rows, {int((nbr >= 0).sum())} neighbour entries")


if __name__ == "__main__":
    main()
