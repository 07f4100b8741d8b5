"""Time When2com's handshake fusion at the OPV2V shape (5 agents x 256 x 50 x 176): the kernel route (``When2comFusion.forward``: v2v_warp_split, conv3x3_sp /
conv3x3_sp_s2, w2c_score, w2c_fuse) against the module's own op-by-op PyTorch route (``forward_torch``: the reference's operations) and against
``forward_reduced`` (the identities in PyTorch ops) on the same device and inputs.  Kernel route vs ``forward_torch`` is the comparison of record;
``forward_reduced`` separates what the identities buy from what the kernels buy.

Protocol: the three versions in ONE process; warm-up of each; then ``--rounds`` rounds, interleaving the versions, a round being device events around ``--reps``
calls.  Per version: the median over the rounds and their spread (min .. max).  Before timing, the outputs are compared element-wise at the timed size.
``--breakdown`` adds a pass of its own over the kernel route with one event pair per launch (``ops.PROFILE``): the time per stage, ``w2c_fuse``'s bytes per second
against HBM's 8 TB/s on its algorithmic bytes (every agent's map read once, the fused map written once), and ``w2c_score``'s time against the parameter image it
must read (9.2 MB).  Event pairs around single launches include the launch gap: the kernel times of record come from a kernel trace.  ``--route-only`` runs nothing
but the kernel route: the program to put behind ``rocprofv3 --kernel-trace --stats --``.

    python tools/time_when2com_fusion.py [--agents 5] [--channels 256] [--hw 50 176] [--reps 5] [--rounds 7] [--breakdown] [--route-only] [--out FILE]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from coalign_amd import ops  # noqa: E402
from coalign_amd.fusion import When2comFusion  # noqa: E402
from coalign_amd.synthetic import when2com_parameters_  # noqa: E402
from time_v2v_fusion import poses  # noqa: E402

HBM_PEAK = 8.0e12
STAGES = ["v2v_warp_split", "conv3x3_sp conv1", "conv3x3_sp conv2", "conv3x3_sp_s2 conv3", "conv3x3_sp conv4", "conv3x3_sp_s2 conv5", "conv3x3_sp_s2 key | query",
          "w2c_score", "w2c_fuse"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--agents", type=int, default=5)
    ap.add_argument("--channels", type=int, default=256)
    ap.add_argument("--hw", type=int, nargs=2, default=[50, 176])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--breakdown", action="store_true")
    ap.add_argument("--route-only", action="store_true", help="run the kernel route alone, --reps times after one warm call, and print nothing else: the program a kernel trace wraps")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_when2com_fusion.py measures on the MI355X: no GPU found")
    dev = torch.device("cuda:0")
    n, C, (H, W) = a.agents, a.channels, a.hw
    m = When2comFusion({"in_channels": C, "H": H, "W": W, "query_size": 32, "key_size": 1024})
    when2com_parameters_(m, seed=1, attention_gain=0.07)
    m = m.eval().to(dev)
    x = torch.relu(torch.randn(n, C, H, W, generator=torch.Generator().manual_seed(2))).to(dev).contiguous(memory_format=torch.channels_last)      # post-ReLU maps, like the shrink header's
    A = poses(n, H, W)[None].to(dev)
    if not m.kernel_route(C, n):
        raise SystemExit("the kernel route does not take this shape: " + str(m.kernel_shape_reason(C, n)))

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
    details = []
    with torch.no_grad():
        m.forward_torch(x, [n], A, details)
    torch.cuda.synchronize()
    want = outs["forward_torch (op by op)"]
    scale = float(want.abs().max())
    result = {"shape": [n, C, H, W], "reps": a.reps, "rounds": a.rounds, "softmax_weights": [float(v) for v in details[0][1]]}
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
    sizes = [(H, W)]
    for _ in range(3):
        sizes.append(((sizes[-1][0] + 1) // 2, (sizes[-1][1] + 1) // 2))
    (h0, w0), (h1, w1), (h2, w2), (h3, w3) = sizes
    conv_flop = 2.0 * 9 * (n * h0 * w0 * (C * 512 + 512 * 256) + n * h1 * w1 * (256 * 256 + 256 * 256) + n * h2 * w2 * 256 * 256 + n * h3 * w3 * 256 * 256)
    result["fp32_flop_convolutions_kernel_route"] = conv_flop
    result["fuse_algorithmic_bytes"] = (n + 1) * C * H * W * 4.0
    result["score_parameter_bytes"] = ops.W2C_PARAM_FLOATS * 4.0
    if a.breakdown:
        ops.PROFILE = {}
        for _ in range(a.reps):
            versions["kernel route"]()
        torch.cuda.synchronize()
        per_op = {name: [s.elapsed_time(e) for s, e in pairs] for name, pairs in ops.PROFILE.items()}
        ops.PROFILE = None
        cursor = {k: 0 for k in per_op}
        stage_ms = {s: [] for s in STAGES}
        for _ in range(a.reps):
            for s in STAGES:
                op = s.split()[0]
                stage_ms[s].append(per_op[op][cursor[op]])
                cursor[op] += 1
        med = {s: sorted(v)[len(v) // 2] for s, v in stage_ms.items()}
        bd = {s: {"ms": v} for s, v in med.items()}
        b = result["fuse_algorithmic_bytes"]
        bd["w2c_fuse"].update(bytes=b, bytes_per_s=b / (med["w2c_fuse"] * 1e-3), fraction_of_hbm_peak=b / (med["w2c_fuse"] * 1e-3) / HBM_PEAK)
        p = result["score_parameter_bytes"]
        bd["w2c_score"].update(bytes=p, bytes_per_s=p / (med["w2c_score"] * 1e-3), fraction_of_hbm_peak=p / (med["w2c_score"] * 1e-3) / HBM_PEAK)
        result["breakdown"] = bd
        result["breakdown_sum_ms"] = sum(med.values())
    line = json.dumps(result)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(line + "\n")


if __name__ == "__main__":
    main()
