"""Time Where2comm at the OPV2V shapes (5 agents x {64 @ 100 x 352, 128 @ 50 x 176, 256 @ 25 x 88}, logits 2 @ 100 x 352, 5 x 5 smoothing):

* the two kernels alone: ``ops.w2comm_masks`` (all masks of the three levels and the rate) and ``ops.w2comm_fuse_nhwc`` (warp and fusion of the masked maps),
  the latter next to ``ops.warp_fuse_nhwc`` on the same maps (what the mask bytes cost) and next to the multiply-first alternative (three products writing masked
  copies, then ``warp_fuse_nhwc``);
* the module: ``Where2comm.fuse`` on its kernel route against ``forward_torch`` (the reference's operations) on the same device and inputs, both with the
  backbone's up-sampling heads behind the fusion, as the reference's forward has them.

Protocol: all versions in ONE process; warm-up of each; then ``--rounds`` rounds, interleaving the versions, a round being device events around ``--reps`` calls.
Per version: the median over the rounds and their spread (min .. max).  Event pairs around calls include the launch gaps and the host's work between launches: the
kernel times of record come from a kernel trace (``--route-only`` is the program to put behind it).  Before timing, the outputs are compared at the timed size.

    python tools/time_where2comm.py [--agents 5] [--reps 20] [--rounds 7] [--route-only] [--out FILE]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from coalign_amd import ops  # noqa: E402
from coalign_amd.backbone import ResNetBEVBackbone  # noqa: E402
from coalign_amd.fusion import Where2commFusion  # noqa: E402
from coalign_amd.synthetic import fill_parameters_  # noqa: E402
from time_v2v_fusion import poses  # noqa: E402

LEVELS = ((64, 100, 352), (128, 50, 176), (256, 25, 88))
BACKBONE = {"layer_nums": [3, 5, 8], "layer_strides": [2, 2, 2], "num_filters": [64, 128, 256], "upsample_strides": [1, 2, 4], "num_upsample_filter": [128, 128, 128]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--agents", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--thre", type=float, default=0.3)
    ap.add_argument("--route-only", action="store_true", help="run the module's kernel route alone, --reps times after one warm call: the program a kernel trace wraps")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_where2comm.py measures on the MI355X: no GPU found")
    dev = torch.device("cuda:0")
    n = a.agents
    g = torch.Generator().manual_seed(1)
    xs = [torch.relu(torch.randn(n, C, H, W, generator=g)).to(dev).contiguous(memory_format=torch.channels_last) for C, H, W in LEVELS]      # post-ReLU maps
    psm = (2 * torch.randn(n, 2, LEVELS[0][1], LEVELS[0][2], generator=g) - 2).to(dev)      # about half of every mask is on at thre 0.3
    A = poses(n, LEVELS[0][1], LEVELS[0][2])[None].to(dev)
    theta = A[0, 0, :n].contiguous()
    m = Where2commFusion({"voxel_size": [0.4, 0.4, 4], "downsample_rate": 1, "multi_scale": True, "layer_nums": BACKBONE["layer_nums"], "num_filters": BACKBONE["num_filters"],
                          "agg_operator": {"mode": "ATTEN", "feature_dim": 256}, "communication": {"thre": a.thre, "gaussian_smooth": {"k_size": 5, "c_sigma": 1.0}}}).eval().to(dev)
    bb = ResNetBEVBackbone(dict(BACKBONE), 64)
    fill_parameters_(bb, seed=0)
    bb = bb.eval().to(dev)
    w, b = m.naive_communication.gaussian_filter.weight.detach(), m.naive_communication.gaussian_filter.bias.detach()

    def route():
        with torch.no_grad():
            return m.fuse(None, psm, [n], A, bb, feats=xs)[0]
    if a.route_only:
        for _ in range(1 + a.reps):
            route()
        torch.cuda.synchronize()
        return
    masks, rates = ops.w2comm_masks(psm, [n], w, b, a.thre, levels=3)

    def torch_route():
        with torch.no_grad():
            return m.forward_torch(None, psm, [n], A, bb, feats=xs)[0]

    def multiply_first():
        return ops.warp_fuse_nhwc([(x * k.unsqueeze(1)).contiguous(memory_format=torch.channels_last) for x, k in zip(xs, masks)], theta, ops.FUSE_ATT)
    versions = {"w2comm_masks": lambda: ops.w2comm_masks(psm, [n], w, b, a.thre, levels=3),
                "w2comm_fuse_nhwc": lambda: ops.w2comm_fuse_nhwc(xs, masks, theta, ops.FUSE_ATT),
                "warp_fuse_nhwc (no masks)": lambda: ops.warp_fuse_nhwc(xs, theta, ops.FUSE_ATT),
                "multiply first, then warp_fuse_nhwc": multiply_first,
                "module, kernel route": route, "module, forward_torch (op by op)": torch_route}
    got, want = route(), torch_route()
    scale = float(want.abs().max())
    err = (got - want).abs()
    result = {"agents": n, "levels": LEVELS, "reps": a.reps, "rounds": a.rounds, "rate": float(rates[0]), "mask_fractions_on": [float(k.float().mean()) for k in masks],
              "kernel route: max_err_of_scale vs forward_torch": float(err.max()) / scale,
              "kernel route: elements_outside_1e-4+1e-5": int((err > 1e-4 * want.abs() + 1e-5 * scale).sum()),
              "masked equals multiply-first bit for bit": all(torch.equal(p, q) for p, q in zip(versions["w2comm_fuse_nhwc"](), multiply_first()))}
    del got, want, err
    for fn in versions.values():
        for _ in range(3):
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
    result["module speedup (medians), kernel route vs forward_torch"] = result["module, forward_torch (op by op)"]["median_ms"] / result["module, kernel route"]["median_ms"]
    # algorithmic bytes of the fusion: every agent's map read once, its mask bytes read once, the fused map written once
    result["fuse_algorithmic_bytes"] = float(sum((n + 1) * C * H * W * 4 + n * H * W for C, H, W in LEVELS))
    line = json.dumps(result)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(line + "\n")


if __name__ == "__main__":
    main()
