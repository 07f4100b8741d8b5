"""Time DiscoNet's pixel-weight fusion at the OPV2V shape (5 agents x 100 x 352 x 256): the one-launch kernel (``ops.disco_fuse``) against the module's op-by-op
PyTorch route (``DiscoFusion.forward_torch``: grid_sample, concatenation, four 1x1 convolutions with BatchNorm, softmax, weighted sum) on the same device and inputs.

Protocol: both versions in ONE process; warm-up of each; then ``--rounds`` rounds, alternating the versions, a round being device events around ``--reps`` calls.
Per version: the median over the rounds and their spread (min .. max).  Before timing, the two outputs are compared element-wise at the timed size.
Also printed: the floating-point operations the kernel executes on the matrix cores (three fp16 products per fp32 product of layers 1 and 2, the ego half of layer 1
once per pixel) and the fraction of the fp16 matrix peak (2.5 PFLOP/s dense) they amount to over the kernel's time.

    python tools/time_disco_fusion.py [--agents 5] [--channels 256] [--hw 100 352] [--reps 50] [--rounds 7] [--out FILE]
"""
import argparse
import json
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from coalign_amd import ops  # noqa: E402
from coalign_amd.fusion import DiscoFusion  # noqa: E402
from coalign_amd.synthetic import disco_parameters_  # noqa: E402

FP16_MATRIX_PEAK = 2.5e15


def poses(n, H, W, seed=0):
    """Ego identity; neighbours turned by up to 30 degrees and shifted by up to a quarter of the map: mostly inside, the borders out of view."""
    g = torch.Generator().manual_seed(seed)
    th = torch.zeros(n, 2, 3, dtype=torch.float64)
    th[:, 0, 0] = th[:, 1, 1] = 1.0
    for j in range(1, n):
        yaw = math.radians(float(torch.rand(1, generator=g)) * 60.0 - 30.0)
        c, s = math.cos(yaw), math.sin(yaw)
        tx, ty = (torch.rand(2, generator=g) - 0.5).tolist()
        th[j] = torch.tensor([[c, -s * H / W, tx], [s * W / H, c, ty]], dtype=torch.float64)
    return th


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--agents", type=int, default=5)
    ap.add_argument("--channels", type=int, default=256)
    ap.add_argument("--hw", type=int, nargs=2, default=[100, 352])
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_disco_fusion.py measures on the MI355X: no GPU found")
    dev = torch.device("cuda:0")
    n, C, (H, W) = a.agents, a.channels, a.hw
    m = DiscoFusion(C)
    disco_parameters_(m.pixel_weight_layer, seed=1)
    m = m.eval().to(dev)
    x = torch.relu(torch.randn(n, C, H, W, generator=torch.Generator().manual_seed(2))).to(dev).contiguous(memory_format=torch.channels_last)      # post-ReLU maps, like the shrink header's
    th = poses(n, H, W).to(dev)
    A = torch.zeros(1, n, n, 2, 3, dtype=torch.float64, device=dev)
    A[0, 0] = th
    image = m.pixel_weight_layer.packed()

    def kernel():
        return ops.disco_fuse(x, th, image)

    def torch_route():
        with torch.no_grad():
            return m.forward_torch(x, [n], A)

    got, want = kernel(), torch_route()
    torch.cuda.synchronize()
    scale = float(want.abs().max())
    err = (got - want).abs()
    outside = int((err > 1e-4 * want.abs() + 1e-5 * scale).sum())
    versions = {"disco_fuse (one launch)": kernel, "op-by-op PyTorch route": torch_route}
    for fn in versions.values():
        for _ in range(5):
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
    px = H * W
    executed = 2.0 * 3.0 * px * (C * 128 * (n + 1) + 128 * 32 * n)
    result = {"shape": [n, C, H, W], "reps": a.reps, "rounds": a.rounds, "max_err_of_scale": float(err.max()) / scale, "elements_outside_1e-4+1e-5": outside,
              "matrix_flop_executed": executed, "fp32_flop_one_launch": 2.0 * px * (C * 128 * (n + 1) + (128 * 32 + 32 * 8 + 8) * n),
              "fp32_flop_op_by_op": 2.0 * px * n * (2 * C * 128 + 128 * 32 + 32 * 8 + 8)}
    for name, ts in times.items():
        ts = sorted(ts)
        result[name] = {"median_ms": ts[len(ts) // 2], "min_ms": ts[0], "max_ms": ts[-1]}
    k = result["disco_fuse (one launch)"]["median_ms"]
    result["speedup_median"] = result["op-by-op PyTorch route"]["median_ms"] / k
    result["fraction_of_fp16_matrix_peak_on_executed_products"] = executed / (k * 1e-3) / FP16_MATRIX_PEAK
    line = json.dumps(result)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(line + "\n")


if __name__ == "__main__":
    main()
