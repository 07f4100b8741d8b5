"""Time V2VNet's message passing at the OPV2V shape (5 agents x 256 x 50 x 176, 2 iterations, max): the kernel route (``V2VNetFusion.forward``: conv3x3_sp +
the three coalign_v2v_* kernels) against the module's own op-by-op PyTorch route (``forward_torch``: the reference's loops) and against ``forward_reduced`` (the
three identities in PyTorch ops) on the same device and inputs.  Kernel route vs ``forward_torch`` is the comparison of record; ``forward_reduced`` separates
what the identities buy from what the kernels buy.

Protocol: the three versions in ONE process; warm-up of each; then ``--rounds`` rounds, interleaving the versions, a round being device events around ``--reps``
calls.  Per version: the median over the rounds and their spread (min .. max).  Before timing, the outputs are compared element-wise at the timed size.
``--breakdown`` adds a pass of its own over the kernel route with one event pair per launch (``ops.PROFILE``): the time per stage, the share of the fp16 matrix
peak (2.5 PFLOP/s dense) of the products the convolutions execute (three fp16 products per fp32 product), and the bytes per second of the three new kernels
against HBM's 8 TB/s (minimum traffic: every operand read once, every result written once).  ``--route-only`` runs nothing but the kernel route: the program
to put behind ``rocprofv3 --kernel-trace --stats --`` for kernel times without launch gaps.

    python tools/time_v2v_fusion.py [--agents 5] [--channels 256] [--hw 50 176] [--iterations 2] [--agg max] [--reps 5] [--rounds 7] [--breakdown] [--route-only] [--out FILE]
"""
import argparse
import json
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from coalign_amd import ops  # noqa: E402
from coalign_amd.fusion import V2VNetFusion  # noqa: E402
from coalign_amd.synthetic import v2v_parameters_  # noqa: E402

FP16_MATRIX_PEAK = 2.5e15
HBM_PEAK = 8.0e12


def poses(n, H, W, seed=0):
    """Every (receiver, sender) pair: turned by up to 30 degrees and shifted by up to a quarter of the map -- mostly inside, the borders out of view."""
    g = torch.Generator().manual_seed(seed)
    th = torch.zeros(n, n, 2, 3, dtype=torch.float64)
    th[:, :, 0, 0] = th[:, :, 1, 1] = 1.0
    for i in range(n):
        for j in range(n):
            if i != j:
                yaw = math.radians(float(torch.rand(1, generator=g)) * 60.0 - 30.0)
                c, s = math.cos(yaw), math.sin(yaw)
                tx, ty = (torch.rand(2, generator=g) - 0.5).tolist()
                th[i, j] = torch.tensor([[c, -s * H / W, tx], [s * W / H, c, ty]], dtype=torch.float64)
    return th


def stage_names(K, layers):
    """The _Timed launches of one kernel-route forward, in order."""
    names = []
    for it in range(K):
        names += [f"it{it} conv3x3_sp ego term", f"it{it} v2v_warp_split", f"it{it} conv3x3_sp warped maps", f"it{it} v2v_aggregate"]
        for k in range(layers):
            names += [f"it{it} conv3x3_sp GRU cell {k}", f"it{it} v2v_gate {k}"]
    return names + ["pointwise_conv mlp"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--agents", type=int, default=5)
    ap.add_argument("--channels", type=int, default=256)
    ap.add_argument("--hw", type=int, nargs=2, default=[50, 176])
    ap.add_argument("--iterations", type=int, default=2)
    ap.add_argument("--agg", default="max")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--breakdown", action="store_true")
    ap.add_argument("--route-only", action="store_true", help="run the kernel route alone, --reps times after one warm call, and print nothing else: the program a kernel trace wraps")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_v2v_fusion.py measures on the MI355X: no GPU found")
    dev = torch.device("cuda:0")
    n, C, (H, W), K = a.agents, a.channels, a.hw, a.iterations
    m = V2VNetFusion({"num_iteration": K, "in_channels": C, "gru_flag": True, "agg_operator": a.agg, "conv_gru": {"H": H, "W": W, "num_layers": 1, "kernel_size": [[3, 3]]}})
    v2v_parameters_(m, seed=1)
    m = m.eval().to(dev)
    x = torch.relu(torch.randn(n, C, H, W, generator=torch.Generator().manual_seed(2))).to(dev).contiguous(memory_format=torch.channels_last)      # post-ReLU maps, like the shrink header's
    A = poses(n, H, W)[None].to(dev)
    if not m.kernel_route(C, n):
        raise SystemExit("the kernel route does not take this shape")

    def run(fn):
        with torch.no_grad():
            return fn(x, [n], A)
    if a.route_only:
        for _ in range(1 + a.reps):
            run(m.forward)
        torch.cuda.synchronize()
        return
    versions = {"kernel route": lambda: run(m.forward), "forward_torch (op by op)": lambda: run(m.forward_torch), "forward_reduced (identities, PyTorch ops)": lambda: run(m.forward_reduced)}
    outs = {k: fn() for k, fn in versions.items()}
    torch.cuda.synchronize()
    want = outs["forward_torch (op by op)"]
    scale = float(want.abs().max())
    result = {"shape": [n, C, H, W], "iterations": K, "agg": a.agg, "reps": a.reps, "rounds": a.rounds}
    for k in ("kernel route", "forward_reduced (identities, PyTorch ops)"):
        err = (outs[k] - want).abs()
        result[k + ": max_err_of_scale vs forward_torch"] = float(err.max()) / scale
        result[k + ": elements_outside_1e-4+1e-5"] = int((err > 1e-4 * want.abs() + 1e-5 * scale).sum())
    del outs
    for fn in versions.values():
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in versions}
    for _ in range(a.rounds):
        for name, fn in versions.items():
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(a.reps):
                fn()
            t1.record()
            t1.synchronize()
            times[name].append(t0.elapsed_time(t1) / a.reps)
    for name, ts in times.items():
        ts = sorted(ts)
        result[name] = {"median_ms": ts[len(ts) // 2], "min_ms": ts[0], "max_ms": ts[-1]}
    k_ms = result["kernel route"]["median_ms"]
    result["speedup_median_vs_forward_torch"] = result["forward_torch (op by op)"]["median_ms"] / k_ms
    result["speedup_median_vs_forward_reduced"] = result["forward_reduced (identities, PyTorch ops)"]["median_ms"] / k_ms
    px = H * W
    receivers = [n if it < K - 1 else 1 for it in range(K)]
    conv_cc = sum(r * n + r for r in receivers)                      # C -> C convolutions: warped maps + ego terms
    conv_gru = sum(receivers)                                        # 2C -> 2C convolutions
    result["convolutions"] = {"C_to_C": conv_cc, "2C_to_2C": conv_gru}
    result["fp32_flop_kernel_route"] = 2.0 * 9 * px * (conv_cc * C * C + conv_gru * 4 * C * C)
    result["fp32_flop_forward_torch"] = 2.0 * 9 * px * K * n * (n * 2 * C * C + 3 * C * 2 * C + 3 * C * C)
    if a.breakdown:
        names = stage_names(K, 1)
        ops.PROFILE = {}
        for _ in range(a.reps):
            versions["kernel route"]()
        torch.cuda.synchronize()
        per_op = {name: [s.elapsed_time(e) for s, e in pairs] for name, pairs in ops.PROFILE.items()}
        ops.PROFILE = None
        # replay the call order: each op's list is in call order, the stage list says which op comes next
        cursor = {k: 0 for k in per_op}
        stage_ms = {s: [] for s in names}
        for _ in range(a.reps):
            for s in names:
                op = "pointwise_conv" if s.startswith("pointwise") else s.split()[1]
                stage_ms[s].append(per_op[op][cursor[op]])
                cursor[op] += 1
        med = {s: sorted(v)[len(v) // 2] for s, v in stage_ms.items()}
        el = C * px * 4.0                                            # bytes of one float32 map (a SplitMap of it takes the same)
        bd = {}
        for it, r in enumerate(receivers):
            traffic = {f"it{it} v2v_warp_split": n * el + r * n * el, f"it{it} v2v_aggregate": r * n * el + 2 * r * el + 2 * r * el, f"it{it} v2v_gate 0": 2 * r * el + r * el}
            flop = {f"it{it} conv3x3_sp ego term": r * C * C, f"it{it} conv3x3_sp warped maps": r * n * C * C, f"it{it} conv3x3_sp GRU cell 0": r * 4 * C * C}
            for s, b in traffic.items():
                bd[s] = {"ms": med[s], "bytes": b, "bytes_per_s": b / (med[s] * 1e-3), "fraction_of_hbm_peak": b / (med[s] * 1e-3) / HBM_PEAK}
            for s, f in flop.items():
                executed = 3.0 * 2.0 * 9 * px * f
                bd[s] = {"ms": med[s], "matrix_flop_executed": executed, "fraction_of_fp16_matrix_peak": executed / (med[s] * 1e-3) / FP16_MATRIX_PEAK}
        bd["pointwise_conv mlp"] = {"ms": med["pointwise_conv mlp"]}
        result["breakdown"] = bd
        result["breakdown_sum_ms"] = sum(med.values())
    line = json.dumps(result)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(line + "\n")


if __name__ == "__main__":
    main()
