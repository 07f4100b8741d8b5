"""Time the pose-robust V2VNet behind the shrink header at the OPV2V shape (5 agents x 256 x 50 x 176, hidden 256, stage 2: pose regression over all pairs, the
weighted EM, attention, weighted message passing, heads): the kernel route (``PointPillarV2VNetRobust.forward_kernels``) against the model's own op-by-op route
(``forward_torch``: the reference's loops, the EM as thousands of small torch ops with host control flow) and against ``forward_reduced`` (the identities in torch
ops) on the same device and inputs.

Protocol: the three versions in ONE process; warm-up of each; then ``--rounds`` rounds, interleaving the versions, a round being device events around ``--reps``
calls.  Per version: the median over the rounds and their spread (min .. max); run the tool three times for the spread across runs.  Before timing, the outputs
are compared at the timed size.  ``--breakdown`` adds a pass over the kernel route with one event pair per launch (``ops.PROFILE``): per kernel its launches per
frame and its time per frame, and for the new memory-bound kernels the bytes per second of their minimum traffic against HBM's 8 TB/s.  ``--stacked`` measures
identity (c)'s open question: the attention's warped-half convolution and ``msg_cnn``'s as ONE C -> hidden + C launch over the shared warp against the two
launches the route uses.  ``--route-only`` runs nothing but the kernel route (the program to put behind a kernel trace).

    python tools/time_v2v_robust.py [--agents 5] [--channels 256] [--hw 50 176] [--reps 3] [--rounds 5] [--breakdown] [--stacked] [--route-only] [--out FILE]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from coalign_amd import ops  # noqa: E402
from coalign_amd.backbone import Conv3x3Pack  # noqa: E402
from coalign_amd.config import builtin_config  # noqa: E402
from coalign_amd.detector import build_model  # noqa: E402
from coalign_amd.synthetic import fill_parameters_, v2v_robust_parameters_  # noqa: E402

HBM_PEAK = 8.0e12


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


def event_ms(fn, reps):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(reps):
        fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--agents", type=int, default=5)
    ap.add_argument("--channels", type=int, default=256)
    ap.add_argument("--hw", type=int, nargs=2, default=[50, 176])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--breakdown", action="store_true")
    ap.add_argument("--stacked", action="store_true")
    ap.add_argument("--route-only", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_v2v_robust.py measures on the MI355X: no GPU found")
    dev = torch.device("cuda:0")
    n, C, (H, W) = a.agents, a.channels, a.hw
    h = builtin_config("opv2v_pointpillar_v2vnet_robust")
    args = h["model"]["args"]
    args["shrink_header"]["dim"] = [C]
    args["v2vfusion"].update(in_channels=C)
    args["v2vfusion"]["conv_gru"].update(H=H, W=W)
    args["robust"].update(H=H, W=W, feature_dim=C, hidden_dim=C)
    args["max_cav"] = max(args["max_cav"], n)
    m = build_model(h)
    fill_parameters_(m, seed=0)
    v2v_robust_parameters_(m, seed=1)
    m = m.eval().to(dev)
    x = torch.relu(torch.randn(n, C, H, W, generator=torch.Generator().manual_seed(2))).to(dev).contiguous(memory_format=torch.channels_last)
    g = torch.Generator().manual_seed(3)
    poses = torch.zeros(n, 3)
    poses[1:, :2] = (torch.rand(n - 1, 2, generator=g) - 0.5) * torch.tensor([60.0, 20.0])
    poses[1:, 2] = (torch.rand(n - 1, generator=g) - 0.5) * 40.0
    poses[:, :2] += torch.randn(n, 2, generator=g) * 0.4
    poses = poses.to(dev)
    if not m.kernel_route(C, n):
        raise SystemExit("the kernel route does not take this shape")

    def run(fn):
        with torch.no_grad():
            return fn(x, [n], poses)
    if a.route_only:
        for _ in range(1 + a.reps):
            run(m.forward_kernels)
        torch.cuda.synchronize()
        return
    versions = {"kernel route": lambda: run(m.forward_kernels), "forward_torch (op by op)": lambda: run(m.forward_torch),
                "forward_reduced (identities, PyTorch ops)": lambda: run(m.forward_reduced)}
    outs = {k: fn() for k, fn in versions.items()}
    torch.cuda.synchronize()
    want = outs["forward_torch (op by op)"]
    result = {"shape": [n, C, H, W], "hidden": C, "stage": 2, "iterations": args["v2vfusion"]["num_iteration"], "reps": a.reps, "rounds": a.rounds}
    for k in ("kernel route", "forward_reduced (identities, PyTorch ops)"):
        for q in ("pairwise_corr", "lidar_pose_corrected", "scores", "cls_preds", "reg_preds"):
            scale = float(want[q].abs().max()) if q.endswith("_preds") else 1.0
            result[f"{k}: max |{q} - forward_torch|" + (" of the scale" if q.endswith("_preds") else "")] = float((outs[k][q].float() - want[q].float()).abs().max()) / scale
    del outs
    for fn in versions.values():
        fn()
    torch.cuda.synchronize()
    times = {k: [] for k in versions}
    for _ in range(a.rounds):
        for name, fn in versions.items():
            times[name].append(event_ms(fn, a.reps))
    for name, ts in times.items():
        result[name] = {"median_ms": median(ts), "min_ms": min(ts), "max_ms": max(ts)}
    k_ms = result["kernel route"]["median_ms"]
    result["speedup_median_vs_forward_torch"] = result["forward_torch (op by op)"]["median_ms"] / k_ms
    result["speedup_median_vs_forward_reduced"] = result["forward_reduced (identities, PyTorch ops)"]["median_ms"] / k_ms
    if a.breakdown:
        ops.PROFILE = {}
        for _ in range(a.reps):
            versions["kernel route"]()
        torch.cuda.synchronize()
        bd = {}
        for name, pairs in ops.PROFILE.items():
            ms = [s.elapsed_time(e) for s, e in pairs]
            per_frame = len(ms) // a.reps
            frames = [sum(ms[r * per_frame:(r + 1) * per_frame]) for r in range(a.reps)]
            bd[name] = {"launches_per_frame": per_frame, "ms_per_frame": median(frames), "longest_launch_ms": max(ms[-per_frame:])}
        ops.PROFILE = None
        el = C * H * W * 4.0                                        # bytes of one float32 map at full size (a SplitMap of it takes the same)
        P = n * n
        # minimum traffic per frame: every operand read once, every result written once
        traffic = {"v2vr_pool_act": (P + n + P / 4) * el * 2 + (P / 4 + P / 16) * el + (P / 16 + P / 64) * el,     # both nets' first pool (with the ego term), the regression's second and third
                   "v2vr_aggregate": (P + 2 * n + 2 * n) * el + (n + 2 + 2) * el}
        for name, b in traffic.items():
            if name in bd:
                bd[name].update(bytes_per_frame=b, bytes_per_s=b / (bd[name]["ms_per_frame"] * 1e-3), fraction_of_hbm_peak=b / (bd[name]["ms_per_frame"] * 1e-3) / HBM_PEAK)
        result["breakdown"] = bd
        result["breakdown_sum_ms"] = sum(v["ms_per_frame"] for v in bd.values())
    if a.stacked:
        # identity (c), second half: ONE convolution C -> hidden + C over the shared warp against the two launches of the route
        att, fus = m.attention_net, m.fusion_net
        wn_att, wn_msg = att._first_split()[0], fus.reduced_weights()[0]
        img_att, img_msg = Conv3x3Pack(wn_att).emu(16, True), Conv3x3Pack(wn_msg).emu(16, True)
        img_both = Conv3x3Pack(torch.cat([wn_att, wn_msg], dim=0).contiguous()).emu(16, True)
        zero, zero2 = torch.zeros(C, device=dev), torch.zeros(2 * C, device=dev)
        T, theta = ops.v2vr_pairwise(poses.double(), args["max_cav"], H, W, 1.6 * W, 1.6 * H)
        warped = ops.v2v_warp_split(x, theta[:n, :n])

        def two():
            ops.conv3x3_sp(warped, img_att, zero, C, None, False, out_split=False)
            ops.conv3x3_sp(warped, img_msg, zero, C, None, False, out_split=False)

        def one():
            ops.conv3x3_sp(warped, img_both, zero2, 2 * C, None, False, out_split=False)
        for fn in (two, one):
            fn()
        torch.cuda.synchronize()
        t2, t1 = [], []
        for _ in range(a.rounds):
            t2.append(event_ms(two, a.reps))
            t1.append(event_ms(one, a.reps))
        result["stacked_convolution"] = {"two launches C -> hidden, C -> C": {"median_ms": median(t2), "min_ms": min(t2), "max_ms": max(t2)},
                                         "one launch C -> hidden + C": {"median_ms": median(t1), "min_ms": min(t1), "max_ms": max(t1)},
                                         "note": "the stacked output [n n, H, W, hidden + C] would further need v2vr_pool_act and v2vr_aggregate to read channel slices of a wider map"}
    line = json.dumps(result)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "a").write(line + "\n")


if __name__ == "__main__":
    main()
