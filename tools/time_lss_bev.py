"""Time the camera model's BEV encoder at cfg 5 (5 agents, C = 128, 240 x 240 cells, ``att_ms``): ``BevEncodeMSFusion.forward`` on the kernel route
(``bev_kernels = True``: stem, stages, ``Up`` and ``down_layer`` on the SplitMap kernels) against the torch route (``bev_kernels = False``: the library's
convolutions, the code path of the commit before the route existed), and the two kernels of csrc/lss_bev.hip alone.

Protocol (that of tools/time_lss_pool.py): ONE process; every version and shape warmed up; then ``--rounds`` rounds, alternating the versions, a round being device
events around that version's repetitions; per version the median over the rounds and their spread.  Before timing, the two routes' outputs are compared at the timed
size.  A kernel's yardstick is the least time the hardware could take -- the larger of its bytes over 8 TB/s and its EXECUTED fp16 FLOP (padding lanes of live
wavefronts included) over 2.5 PFLOP/s -- over its measured time; which of the two bounds it is recorded.

    python tools/time_lss_bev.py [--agents 5] [--channels 128] [--size 240] [--reps 10] [--rounds 5] [--out profiles/lss_bev/timing.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from coalign_amd import lss, ops  # noqa: E402
from coalign_amd.pose import get_pairwise_transformation  # noqa: E402
from coalign_amd.synthetic import fill_parameters_, make_poses  # noqa: E402

HBM, FP16 = 8.0e12, 2.5e15


def bound(byte_count, flop):
    t_b, t_f = byte_count / HBM, flop / FP16
    return max(t_b, t_f), ("bytes / 8 TB/s" if t_b >= t_f else "fp16 FLOP / 2.5 PFLOP/s")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--agents", type=int, default=5)
    ap.add_argument("--channels", type=int, default=128)
    ap.add_argument("--size", type=int, default=240)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--seed", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_lss_bev.py measures on the MI355X: no GPU found")
    dev = torch.device("cuda:0")
    A, C, S = a.agents, a.channels, a.size
    enc = lss.BevEncodeMSFusion({"core_method": "att_ms", "args": {"in_channels": C, "voxel_size": [0.4, 0.4, 20.0]}})
    fill_parameters_(enc, seed=a.seed)
    enc = enc.to(dev).eval()
    g = torch.Generator().manual_seed(a.seed)
    x = torch.randn(A, C, S, S, generator=g).to(dev).contiguous(memory_format=torch.channels_last)
    pair = torch.from_numpy(np.stack([get_pairwise_transformation(make_poses(np.random.RandomState(a.seed), A, spread_xy=(8.0, 4.0), spread_yaw=20.0), 5)])).to(dev)

    def route(on):
        def run():
            enc.bev_kernels = on
            with torch.no_grad():
                return enc(x, [A], pair)
        return run

    enc.bev_kernels = True
    reason = enc.kernel_shape_reason(x)
    if reason is not None:
        raise SystemExit(f"the kernel route does not take this shape: {reason}")
    on, off = route(True)(), route(False)()
    agree = {}
    for name, p, q in (("x_single", on[0], off[0]), ("x_fuse", on[1], off[1])):
        err, scale = (p.double() - q.double()).abs(), float(q.abs().max())
        agree[name] = {"max_diff_of_scale": float(err.max()) / scale, "elements_outside_1e-4+1e-5": int((err > 1e-4 * q.double().abs() + 1e-5 * scale).sum())}

    # the two new kernels alone, at the shapes of this frame
    w, b = enc._folded()[0]
    Ho = (S - 1) // 2 + 1
    n_dec = A + 1
    skip2, low2 = (torch.randn(n_dec, c, s, s, generator=g).to(dev).contiguous(memory_format=torch.channels_last) for c, s in ((128, S // 4), (256, S // 8)))
    skip1, low1 = (torch.randn(n_dec, c, s, s, generator=g).to(dev).contiguous(memory_format=torch.channels_last) for c, s in ((64, S // 2), (256, S // 4)))
    tiles_x = (Ho + 31) // 32
    stem_flop = 2.0 * 3 * A * Ho * tiles_x * 32 * 64 * 49 * C                      # executed: live wavefronts (one output row x 32 columns each), three products
    stem_useful = 2.0 * A * Ho * Ho * 64 * 49 * C                                  # fp32-equivalent
    stem_bytes = 4.0 * (A * S * S * C + A * Ho * Ho * 64) + w.numel()

    def up_bytes(s, lo):
        return 4.0 * (s.numel() + lo.numel() + s.shape[0] * (s.shape[1] + lo.shape[1]) * s.shape[2] * s.shape[3])

    kernels = {"conv7x7_s2_sp": (lambda: ops.conv7x7_s2_sp(x, w, b), stem_bytes, stem_flop),
               "up2x_concat_sp (up_layer2: 128 + 256 channels)": (lambda: ops.up2x_concat_sp(skip2, low2), up_bytes(skip2, low2), 0.0),
               "up2x_concat_sp (up_layer1: 64 + 256 channels)": (lambda: ops.up2x_concat_sp(skip1, low1), up_bytes(skip1, low1), 0.0)}
    versions = {"forward, bev_kernels = True": (route(True), a.reps), "forward, bev_kernels = False (torch route)": (route(False), a.reps)}
    versions.update({k: (fn, 4 * a.reps) for k, (fn, _, _) in kernels.items()})
    for fn, _ in versions.values():
        for _ in range(3):
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
    result = {"shape": {"agents": A, "C": C, "H": S, "W": S, "fusion": "att_ms"}, "reps": a.reps, "rounds": a.rounds, "routes_agree": agree,
              "launch_count_kernel_route": {"conv7x7_s2_sp": 1, "conv3x3_sp": 16, "conv3x3_sp_s2": 2, "up2x_concat_sp": 2, "warp_fuse": 3, "normalize_pairwise": 1}}
    for name, ts in times.items():
        ts = sorted(ts)
        result[name] = {"median_ms": ts[len(ts) // 2], "min_ms": ts[0], "max_ms": ts[-1]}
    result["torch_route_over_kernel_route"] = result["forward, bev_kernels = False (torch route)"]["median_ms"] / result["forward, bev_kernels = True"]["median_ms"]
    for name, (_, nbytes, flop) in kernels.items():
        least, which = bound(nbytes, flop)
        t = result[name]["median_ms"] * 1e-3
        result[name].update({"bytes": nbytes, "executed_fp16_flop": flop, "least_time_ms": least * 1e3, "bound_by": which, "share_of_bound": least / t,
                             "TB_per_s": nbytes / t / 1e12, "executed_PFLOP_per_s": flop / t / 1e15})
    result["conv7x7_s2_sp"]["fp32_equivalent_TFLOP_per_s"] = stem_useful / (result["conv7x7_s2_sp"]["median_ms"] * 1e-3) / 1e12
    line = json.dumps(result)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(line + "\n")


if __name__ == "__main__":
    main()
