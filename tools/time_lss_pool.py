"""Time Lift-Splat's frustum pooling at the shape of the camera config (5 agents x 4 cameras x 48 depth bins x 60 x 80 pixels, C = 128, a 240 x 240 grid): the
kernel route (``ops.lss_pool`` with a reused index: two launches) against the reference's route op for op (``LiftSplat.forward_reference_ops``: outer product,
kept, argsort, cumsum, difference, scatter) on the same device and inputs.  Also: the index build on its own, and the kernel route with the index rebuilt every frame.

Protocol (that of tools/time_disco_fusion.py): all versions in ONE process; warm-up of each; then ``--rounds`` rounds, alternating the versions, a round being
device events around that version's repetitions.  Per version: the median over the rounds and their spread (min .. max).  Before timing, every version's output is
compared element-wise at the timed size with a float64 sum over that version's own cells (the kernel's come from the float64 geometry, the torch routes' from the
reference's float32 geometry; the number of points on which the two disagree is printed).

Bytes: the ALGORITHMIC bytes are features + logits in and the map out, once each; the ROW READS ISSUED are one C-channel row per kept point (the same rows again
and again, from cache).  The bound that applies to the second figure is the rate at which indexed rows come out of the L2 / Infinity Cache, not HBM's: 16.8 - 18.8
TB/s for rows that live in the XCDs' L2, 8.6 TB/s for rows spread over a table that only fits the Infinity Cache (measured with 1 152-byte rows); the feature rows
of 5 agents are 49 MB, more than the eight L2s hold and less than the Infinity Cache does.

    python tools/time_lss_pool.py [--agents 5] [--cams 4] [--channels 128] [--reps 20] [--ref-reps 3] [--rounds 5] [--out FILE]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from coalign_amd import ops  # noqa: E402
from coalign_amd.config import builtin_config  # noqa: E402
from coalign_amd.lss import LiftSplat  # noqa: E402
from coalign_amd.synthetic import make_camera_rig  # noqa: E402

L2_ROW_RATE, IC_ROW_RATE = 16.8e12, 8.6e12
CAMS = ("rots", "trans", "intrins", "post_rots", "post_trans")


def float64_sum(logit, x, cell, A, N, n):
    """[A, nz C, ny, nx] float64 on the device: softmax x features summed per cell of ``cell`` ((z ny + y) nx + x or -1), one camera at a time."""
    nx, ny, nz = n
    M, D, fH, fW = logit.shape
    C = x.shape[1]
    out = torch.zeros((A * nz * ny * nx, C), dtype=torch.float64, device=x.device)
    for m in range(M):
        vol = (torch.softmax(logit[m].double(), 0)[:, :, :, None] * x[m].double().permute(1, 2, 0)[None]).reshape(-1, C)
        c = cell[m].reshape(-1).long()
        kept = c >= 0
        out.index_add_(0, (m // N) * (nz * ny * nx) + c[kept], vol[kept])
    return out.view(A, nz, ny, nx, C).permute(0, 1, 4, 2, 3).reshape(A, nz * C, ny, nx)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--agents", type=int, default=5)
    ap.add_argument("--cams", type=int, default=4)
    ap.add_argument("--channels", type=int, default=128)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--ref-reps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--seed", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_lss_pool.py measures on the MI355X: no GPU found")
    dev = torch.device("cuda:0")
    margs = builtin_config("camera/opv2v_lss_coalign")["model"]["args"]
    sp = LiftSplat(margs["grid_conf"], margs["data_aug_conf"], margs["img_downsample"]).to(dev)
    A, N, C, D, fH, fW = a.agents, a.cams, a.channels, sp.D, sp.fH, sp.fW
    rig = make_camera_rig(A, N, margs["data_aug_conf"]["final_dim"], seed=a.seed)      # the golden generator's rig at full size: four cameras at 90 degrees, f ~ 400 px
    cams = [rig[k].to(dev) for k in CAMS]
    g = torch.Generator().manual_seed(a.seed)
    logit = (torch.randn(A * N, D, fH, fW, generator=g) * 3.0).to(dev)
    x = torch.randn(A * N, C, fH, fW, generator=g).to(dev).contiguous(memory_format=torch.channels_last)

    index = sp.build_index(*cams)
    lens = (index.starts[1:] - index.starts[:-1]).long()
    kept = index.n_points
    stats = {"points": A * N * D * fH * fW, "kept": kept, "cells": index.cells, "occupied": int((lens > 0).sum()), "longest_list": int(lens.max()),
             "mean_list": kept / max(1, int((lens > 0).sum())), "long_lists": int(index.long_cells.numel())}

    def kernel():
        return ops.lss_pool(logit, x, index)

    def kernel_rebuilt():
        return ops.lss_pool(logit, x, sp.build_index(*cams))

    def build_only():
        return sp.build_index(*cams)

    def reference_ops():
        with torch.no_grad():
            return sp.forward_reference_ops(logit, x, *cams)

    # every route against a float64 sum over ITS OWN cells: the kernel route's come from the float64 geometry, the torch routes' from the reference's float32 geometry
    cell = ops.lss_cells(*cams, *(v.to(dev) for v in sp.axes), sp.lower, sp.cell_size, sp.nx, N)
    idx, k32 = sp.voxel_indices(sp.get_geometry(*cams))
    c32 = torch.where(k32, (idx[:, 2] * sp.nx[1] + idx[:, 1]) * sp.nx[0] + idx[:, 0], torch.full_like(idx[:, 0], -1)).view_as(cell)
    stats["cells_float32_vs_float64_differ"] = int((c32 != cell.long()).sum())
    errors = {}
    for cells_of, routes in ((cell, (("lss_pool", kernel),)), (c32, (("forward_reference_ops", reference_ops), ("forward_torch", lambda: sp.forward_torch(logit, x, *cams))))):
        want = float64_sum(logit, x, cells_of, A, N, sp.nx)
        scale = float(want.abs().max())
        for name, fn in routes:
            err = (fn().double() - want).abs()
            errors[name] = {"max_err_of_scale": float(err.max()) / scale, "elements_outside_1e-4+1e-5": int((err > 1e-4 * want.abs() + 1e-5 * scale).sum())}
    del want, err, idx, k32, c32
    torch.cuda.empty_cache()

    versions = {"lss_pool (index reused: two launches)": (kernel, a.reps), "lss_pool + index rebuilt every frame": (kernel_rebuilt, max(1, a.reps // 4)),
                "index build alone": (build_only, max(1, a.reps // 4)), "forward_reference_ops (the reference's route)": (reference_ops, a.ref_reps)}
    for fn, _ in versions.values():
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in versions}
    for _ in range(a.rounds):
        for name, (fn, reps) in versions.items():
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(reps):
                fn()
            t1.record()
            t1.synchronize()
            times[name].append(t0.elapsed_time(t1) / reps)
    result = {"shape": {"agents": A, "cams": N, "D": D, "fH": fH, "fW": fW, "C": C, "grid": sp.nx}, "reps": a.reps, "ref_reps": a.ref_reps, "rounds": a.rounds, **stats,
              "errors_vs_float64": errors}
    for name, ts in times.items():
        ts = sorted(ts)
        result[name] = {"median_ms": ts[len(ts) // 2], "min_ms": ts[0], "max_ms": ts[-1]}
    k = result["lss_pool (index reused: two launches)"]["median_ms"] * 1e-3
    algorithmic = 4.0 * (A * N * fH * fW * (C + D) + index.cells * C)
    rows_issued = 4.0 * kept * C
    result["speedup_median_vs_reference_ops"] = result["forward_reference_ops (the reference's route)"]["median_ms"] * 1e-3 / k
    result["algorithmic_bytes"], result["row_read_bytes_issued"] = algorithmic, rows_issued
    result["algorithmic_TB_per_s"], result["row_reads_TB_per_s"] = algorithmic / k / 1e12, rows_issued / k / 1e12
    result["row_reads_share_of_L2_gather_rate_16.8TBps"] = rows_issued / k / L2_ROW_RATE
    result["row_reads_share_of_infinity_cache_gather_rate_8.6TBps"] = rows_issued / k / IC_ROW_RATE
    line = json.dumps(result)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(line + "\n")


if __name__ == "__main__":
    main()
